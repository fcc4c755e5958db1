"""In-kernel exploration noise (cp_policy_noise), the parts that need no GPU: the ctypes layout against gcc,
the unchanged ABI version, the four exported symbols, cp_policy_noise_check's rejections, and self-checks of
the numpy restatement (tests/policy_noise_ref.py) the GPU tests compare against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cartpoleplusplus_amd import abi, native
from tests import policy_noise_ref as nref
from tests import policy_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpole_amd.h")
NEW = ("cp_policy_noise_check", "cp_set_policy_noise", "cp_policy_noise_get", "cp_policy_noise_set")
STAT_SEED = (11 << 32) | 5      # fixed: test_draw_statistics checks that its 2^16 draws pass with it


def test_cp_policy_noise_ctypes_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %zu\\n", sizeof(cp_policy_noise),
         offsetof(cp_policy_noise, kind), offsetof(cp_policy_noise, flags), offsetof(cp_policy_noise, theta),
         offsetof(cp_policy_noise, sigma), offsetof(cp_policy_noise, max_magnitude), offsetof(cp_policy_noise, seed),
         CP_NOISE_OFF, CP_NOISE_GAUSSIAN, CP_NOISE_OU, CP_NOISE_RESET_ON_EPISODE, CP_NOISE_CLIP_SYMMETRIC,
         CP_ABI_VERSION, sizeof(cp_policy));
  return 0;
}}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    N = abi.cp_policy_noise
    assert out == [C.sizeof(N), N.kind.offset, N.flags.offset, N.theta.offset, N.sigma.offset, N.max_magnitude.offset,
                   N.seed.offset, abi.CP_NOISE_OFF, abi.CP_NOISE_GAUSSIAN, abi.CP_NOISE_OU,
                   abi.CP_NOISE_RESET_ON_EPISODE, abi.CP_NOISE_CLIP_SYMMETRIC, abi.CP_ABI_VERSION, C.sizeof(abi.cp_policy)]
    assert out[:7] == [32, 0, 4, 8, 12, 16, 24]
    assert abi.NOISE_KINDS == {"off": 0, "gaussian": 1, "ou": 2}
    assert C.sizeof(abi.cp_policy) == 56      # additive: cp_policy is byte for byte ABI 8's


def test_abi_version_is_unchanged_and_the_symbols_are_exported():
    lib = native.load()
    assert lib.cp_abi_version() == 8 and abi.CP_ABI_VERSION == 8
    for name in NEW:
        assert name in native.EXPORTS
        assert getattr(lib, name).argtypes is not None
    header = open(HEADER).read()
    for name in NEW:
        assert f"int {name}(" in header


def _noise(kind=abi.CP_NOISE_OU, flags=0, theta=0.15, sigma=0.2, max_magnitude=1.5, seed=0):
    p = abi.cp_policy_noise()
    p.kind, p.flags, p.theta, p.sigma, p.max_magnitude, p.seed = kind, flags, theta, sigma, max_magnitude, seed
    return p


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=3), b"kind must be"),
    (dict(kind=-1), b"kind must be"),
    (dict(flags=0x4), b"unknown CP_NOISE_* bit"),
    (dict(flags=0x1 | 0x2 | 0x100), b"unknown CP_NOISE_* bit"),
    (dict(sigma=-0.5), b"sigma must be finite and >= 0"),
    (dict(sigma=float("nan")), b"sigma must be finite and >= 0"),
    (dict(sigma=float("inf")), b"sigma must be finite and >= 0"),
    (dict(theta=-1e-3), b"theta must be finite and >= 0"),
    (dict(theta=float("nan")), b"theta must be finite and >= 0"),
    (dict(theta=float("inf")), b"theta must be finite and >= 0"),
])
def test_noise_check_rejections(kw, msg):
    lib = native.load()
    assert lib.cp_policy_noise_check(C.byref(_noise(**kw))) < 0
    err = lib.cp_last_error(None)
    assert err.startswith(b"cp_policy_noise_check: ") and msg in err, err


def test_noise_check_null_and_accepted():
    lib = native.load()
    assert lib.cp_policy_noise_check(None) < 0 and b"null" in lib.cp_last_error(None)
    for p in (_noise(), _noise(kind=abi.CP_NOISE_GAUSSIAN, theta=0.0, sigma=0.0, max_magnitude=0.0),
              _noise(kind=abi.CP_NOISE_OFF), _noise(flags=0x3, max_magnitude=-1.0, seed=(1 << 64) - 1)):
        assert lib.cp_policy_noise_check(C.byref(p)) == 0


# ---- the restatement's own checks

def test_u1_is_in_0_1_and_the_extreme_words_give_finite_draws():
    ones = np.full((1, 4), 0xFFFFFFFF, np.uint32)
    zeros = np.zeros((1, 4), np.uint32)
    rng = np.random.default_rng(1)
    some = rng.integers(0, 1 << 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    for w in (ones, zeros, some):
        u1, t = nref.uniforms(w)
        assert u1.dtype == np.float32 and t.dtype == np.float32
        assert (u1 > 0).all() and (u1 <= 1).all()
        g, r = nref.gauss64(w)
        assert np.isfinite(g).all() and np.isfinite(r).all() and g.shape == (len(w), 4) and r.shape == (len(w), 4)
    assert nref.uniforms(ones)[0].max() == 1.0              # (2^24 - 1) + 1: r = 0, the draw is 0
    assert not nref.gauss64(ones)[0].any()
    assert nref.uniforms(zeros)[0].min() == np.float32(2.0 ** -24)
    g0, r0 = nref.gauss64(zeros)                            # the largest radius, at angle 0
    assert np.allclose(r0, np.sqrt(48 * np.log(2.0))) and np.allclose(g0, [[r0[0, 0], 0.0, r0[0, 0], 0.0]])


def test_draw_statistics():
    """2^16 draws (2^14 envs' blocks at step 0): mean within 4 / sqrt(N) of 0, variance within 4 sqrt(2 / N) of 1."""
    n_env = 1 << 14
    w = nref.noise_words(np.zeros(n_env, np.int64), np.zeros(n_env, np.int64), np.arange(n_env), STAT_SEED)
    g = nref.gauss64(w)[0].reshape(-1)
    N = g.size
    assert N == 1 << 16
    print(f"mean {g.mean():+.5f} (4 se = {4 / np.sqrt(N):.5f}), var {g.var():.5f} (4 se = {4 * np.sqrt(2 / N):.5f})")
    assert abs(g.mean()) <= 4 / np.sqrt(N)
    assert abs(g.var() - 1.0) <= 4 * np.sqrt(2.0 / N)
    # the four components of a block are not copies of each other
    assert abs(np.corrcoef(g.reshape(-1, 4).T)[0, 1]) < 0.05


def test_clips():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((257, 4)) * 2).astype(np.float32)
    m = 1.5
    assert np.array_equal(nref.clip(x, 0, m), np.minimum(x, np.float32(m)))
    assert np.array_equal(nref.clip(x, nref.CLIP_SYMMETRIC, m), np.clip(x, np.float32(-m), np.float32(m)))
    assert (nref.clip(x, 0, m) < -m).any()                  # the default leaves the low side alone
    for off in (0.0, -1.0):
        assert np.array_equal(nref.clip(x, nref.CLIP_SYMMETRIC, off), x)
    # the reference's own expression (util.py:155), on the same numbers
    assert np.array_equal(nref.clip(x, 0, m), np.clip(np.float32(m), np.float32(-m), x))


def test_ou_update_roundings():
    """Each product and sum is one float32 rounding: against float64 arithmetic rounded step by step."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((100, 4)).astype(np.float32)
    n = (rng.standard_normal((100, 4)) * 0.2).astype(np.float32)
    theta = 0.15
    steps = np.arange(100) % 3
    f64, f32 = np.float64, np.float32
    for flags in (0, nref.RESET_ON_EPISODE):
        x0 = x.copy()
        if flags:
            x0[steps == 0] = 0
        pull = (f64(f32(theta)) * -x0.astype(f64)).astype(f32)
        x1 = (x0.astype(f64) + pull.astype(f64)).astype(f32)
        x2 = (x1.astype(f64) + n.astype(f64)).astype(f32)
        got = nref.ou_update(x, n, theta, flags, 0.0, steps)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x2.view(np.uint32))
    assert np.array_equal(nref.ou_update(x, n, theta, 0, 0.0, steps), nref.ou_update(x, n, theta, 0, 0.0, steps * 0 + 1))
    assert not np.array_equal(x, nref.ou_update(x, n * 0, theta, 0, 0.0, steps))


def test_word_stream_differs_from_the_sample_heads():
    steps, episode, gid, seed = np.array([0, 1, 7, 150]), np.array([0, 3, 3, 9]), np.array([0, 1, 64, (1 << 32) + 5]), 77
    wn = nref.noise_words(steps, episode, gid, seed)
    ws = ref.sample_words(steps, episode, gid, seed)
    assert wn.shape == (4, 4) and ws.shape == (4, 2, 4)
    for c in range(2):
        assert not (wn == ws[:, c]).all(axis=1).any()
    assert len({tuple(r) for r in wn}) == 4
    # the counters never meet: SAMPLE's first word stays below 0x80000000 for any step counter an episode reaches
    assert ref.SAMPLE_CTR0 + 2 * (1 << 29) <= nref.NOISE_CTR0
