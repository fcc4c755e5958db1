"""Seeded ES perturbations (cp_policy_es), the parts that need no GPU: the ctypes layout against gcc, the
unchanged ABI version, the four exported symbols, cp_policy_es_check's rejections, and self-checks of the numpy
restatement (tests/policy_es_ref.py) the GPU tests compare against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cartpoleplusplus_amd import abi, native
from tests import policy_es_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpole_amd.h")
NEW = ("cp_policy_es_check", "cp_set_policy_es", "cp_policy_es_weights", "cp_policy_es_gradient")
STAT_SEED = (7 << 32) | 3      # fixed: test_draw_statistics checks that its 2^16 draws pass with it


def test_cp_policy_es_ctypes_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %zu %zu\\n", sizeof(cp_policy_es),
         offsetof(cp_policy_es, kind), offsetof(cp_policy_es, flags), offsetof(cp_policy_es, sigma),
         offsetof(cp_policy_es, generation), offsetof(cp_policy_es, seed), offsetof(cp_policy_es, population),
         offsetof(cp_policy_es, group), CP_ES_OFF, CP_ES_BYTES4, CP_ES_ANTITHETIC, CP_ABI_VERSION,
         sizeof(cp_policy), sizeof(cp_policy_noise));
  return 0;
}}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    E = abi.cp_policy_es
    assert out == [C.sizeof(E), E.kind.offset, E.flags.offset, E.sigma.offset, E.generation.offset, E.seed.offset,
                   E.population.offset, E.group.offset, abi.CP_ES_OFF, abi.CP_ES_BYTES4, abi.CP_ES_ANTITHETIC,
                   abi.CP_ABI_VERSION, C.sizeof(abi.cp_policy), C.sizeof(abi.cp_policy_noise)]
    assert out[:8] == [32, 0, 4, 8, 12, 16, 24, 28]
    assert out[-2:] == [56, 32]               # additive: cp_policy and cp_policy_noise are byte for byte ABI 8's
    assert (eref.OFF, eref.BYTES4, eref.ANTITHETIC) == (abi.CP_ES_OFF, abi.CP_ES_BYTES4, abi.CP_ES_ANTITHETIC)


def test_abi_version_is_unchanged_and_the_symbols_are_exported():
    lib = native.load()
    assert lib.cp_abi_version() == 8 and abi.CP_ABI_VERSION == 8
    for name in NEW:
        assert name in native.EXPORTS
        assert getattr(lib, name).argtypes is not None
    header = open(HEADER).read()
    for name in NEW:
        assert f"int {name}(" in header


def _es(kind=abi.CP_ES_BYTES4, flags=abi.CP_ES_ANTITHETIC, sigma=0.1, generation=0, seed=0, population=8, group=1):
    p = abi.cp_policy_es()
    p.kind, p.flags, p.sigma, p.generation, p.seed = kind, flags, sigma, generation, seed
    p.population, p.group = population, group
    return p


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=2), b"kind must be"),
    (dict(kind=-1), b"kind must be"),
    (dict(flags=0x2), b"unknown CP_ES_* bit"),
    (dict(flags=0x1 | 0x100), b"unknown CP_ES_* bit"),
    (dict(sigma=-0.5), b"sigma must be finite and >= 0"),
    (dict(sigma=float("nan")), b"sigma must be finite and >= 0"),
    (dict(sigma=float("inf")), b"sigma must be finite and >= 0"),
    (dict(population=0), b"population must be >= 1"),
    (dict(population=-3), b"population must be >= 1"),
    (dict(group=0), b"group must be >= 1"),
    (dict(group=-64), b"group must be >= 1"),
])
def test_es_check_rejections(kw, msg):
    lib = native.load()
    assert lib.cp_policy_es_check(C.byref(_es(**kw))) < 0
    err = lib.cp_last_error(None)
    assert err.startswith(b"cp_policy_es_check: ") and msg in err, err


def test_es_check_null_and_accepted():
    lib = native.load()
    assert lib.cp_policy_es_check(None) < 0 and b"null" in lib.cp_last_error(None)
    for p in (_es(), _es(flags=0, sigma=0.0, population=1), _es(kind=abi.CP_ES_OFF),
              _es(generation=(1 << 32) - 1, seed=(1 << 64) - 1, population=(1 << 31) - 1, group=(1 << 31) - 1)):
        assert lib.cp_policy_es_check(C.byref(p)) == 0


# ---- the restatement's own checks

def test_philox_matches_the_oracles():
    from oracle import oracle as O
    rng = np.random.default_rng(2)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    ctr[0], ctr[1] = 0, 0xFFFFFFFF
    for seed in (0, 1, (0xDEADBEEF << 32) | 0x12345678, (1 << 64) - 1):
        w = eref.philox(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], seed)
        assert w.dtype == np.uint32 and w.shape == (64, 4)
        for i in range(64):
            assert w[i].tolist() == O.philox4x32_10([int(x) for x in ctr[i]], (seed & 0xFFFFFFFF, seed >> 32))


def test_k_and_the_extreme_words():
    assert eref.K == np.float32(0.006765875) and float(eref.K).hex() == "0x1.bb688c0000000p-8"
    # the float32 nearest to 21845^(-1/2): its neighbours are further away
    exact = 21845.0 ** -0.5
    for nb in (np.nextafter(eref.K, np.float32(0)), np.nextafter(eref.K, np.float32(1))):
        assert abs(float(eref.K) - exact) < abs(float(nb) - exact)
    e = eref.epsilon_of_words(np.array([0, 0xFFFFFFFF, 0x01020304, 0xFF000000], np.uint32))
    assert e.dtype == np.float32
    assert e[0] == -(np.float32(510) * eref.K) and e[1] == np.float32(510) * eref.K
    assert e[2] == np.float32(10 - 510) * eref.K and e[3] == np.float32(255 - 510) * eref.K
    assert abs(float(e[1])) <= 3.451


def test_draw_statistics():
    """2^16 draws (4 members x 2^14 parameters): mean within 4 / sqrt(N) of 0; variance within 4 standard errors
    of 1, the standard error of a sample variance being sqrt((kurtosis - 1) / N) with kurtosis 3 - 0.3."""
    eps = eref.es_epsilon(np.arange(4), 1 << 14, seed=STAT_SEED, flags=0).reshape(-1).astype(np.float64)
    N = eps.size
    assert N == 1 << 16
    se_var = np.sqrt((2.7 - 1.0) / N)
    print(f"mean {eps.mean():+.5f} (4 se = {4 / np.sqrt(N):.5f}), var {eps.var():.5f} (4 se = {4 * se_var:.5f})")
    assert abs(eps.mean()) <= 4 / np.sqrt(N)
    assert abs(eps.var() - 1.0) <= 4 * se_var
    assert np.abs(eps).max() <= 3.451
    # the four words of a block are not copies of each other
    assert abs(np.corrcoef(eps.reshape(-1, 4).T)[0, 1]) < 0.05


def test_antithetic_members_are_exact_negatives():
    F, sigma = 169, 0.37
    d = eref.es_delta(np.arange(7), F, sigma, seed=5, generation=2, flags=eref.ANTITHETIC)
    assert d.dtype == np.float32 and d.shape == (7, F)
    for k in range(3):
        assert np.array_equal(d[2 * k], -d[2 * k + 1]) and d[2 * k].any()
    assert not np.array_equal(d[0], d[2]) and not np.array_equal(d[6], d[4])
    plain = eref.es_delta(np.arange(7), F, sigma, seed=5, generation=2, flags=0)
    assert np.array_equal(plain[[0, 1, 2, 3]], d[[0, 2, 4, 6]])     # the draw of member m without the flag is e = m
    theta = np.linspace(-1, 1, F).astype(np.float32)
    w = eref.es_weights(theta, np.arange(7), sigma, seed=5, generation=2)
    assert np.array_equal(w[0], theta + d[0]) and np.array_equal(w[1], theta - d[0])


def test_generation_seed_and_draw_each_give_other_words():
    F = 64
    base = eref.es_words([3], F, seed=9, generation=4)
    for other in (eref.es_words([3], F, seed=9, generation=5), eref.es_words([3], F, seed=10, generation=4),
                  eref.es_words([3], F, seed=9 | (1 << 32), generation=4), eref.es_words([4], F, seed=9, generation=4)):
        assert other.shape == base.shape and (other != base).mean() > 0.9
    # parameter f reads word f & 3 of block f >> 2
    blk = eref.philox(eref.ES_CTR0 + 5, 4, 3, 0, 9)
    assert base[0, 20:24].tolist() == blk.tolist()


def test_the_counters_high_word_is_reached():
    F = 16
    big = (1 << 32) + 3
    hi = eref.es_words([big], F, seed=1)
    assert not np.array_equal(hi, eref.es_words([3], F, seed=1))    # e_hi = 1 against e_hi = 0
    assert hi[0, :4].tolist() == eref.philox(eref.ES_CTR0, 0, 3, 1, 1).tolist()
    # with ANTITHETIC the members 2^33 + 6 and 2^33 + 7 read that draw
    e, s = eref.member_draw(np.array([2 * big, 2 * big + 1], np.uint64), eref.ANTITHETIC)
    assert e.tolist() == [big, big] and s.tolist() == [1.0, -1.0]


def test_gradient64_and_gamma():
    F, lo = 37, 3
    c = np.array([0.5, -1.25, 2.0, 0.75], np.float32)
    g, scale = eref.es_gradient64(c, lo, F, seed=4, generation=1, flags=eref.ANTITHETIC)
    eps = eref.es_epsilon(np.arange(lo, lo + 4), F, seed=4, generation=1).astype(np.float64)
    want = -0.5 * eps[0] - 1.25 * eps[1] - 2.0 * eps[2] + 0.75 * eps[3]    # members 3 4 5 6: signs - + - +
    assert np.allclose(g, want, rtol=0, atol=1e-12) and (scale >= np.abs(g)).all()
    assert np.array_equal(eps[1], eps[2]) and not np.array_equal(eps[0], eps[1])
    assert eref.gamma(9) == 9 * 2.0 ** -24 / (1 - 9 * 2.0 ** -24)
    layers = eref.unpacked(np.arange(7 * 15 + 4 * 8, dtype=np.float32), (14, 7, 4))
    assert [w.shape for w, _ in layers] == [(7, 14), (4, 7)] and layers[1][1].tolist() == [133, 134, 135, 136]
