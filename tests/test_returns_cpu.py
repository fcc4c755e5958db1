"""Returns and advantages (cp_returns), the parts that need no GPU: the ctypes layout against gcc, the unchanged
ABI version, the three exported symbols, cp_returns_check's rejections, cp_returns_scratch_bytes, and self-checks
of the numpy restatement (tests/returns_ref.py) the GPU tests compare against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cartpoleplusplus_amd import abi, native
from tests import returns_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpole_amd.h")
NEW = ("cp_returns_check", "cp_returns_scratch_bytes", "cp_returns_compute")
f32 = np.float32


def test_cp_returns_ctypes_layout_matches_c(tmp_path):
    fields = ("kind", "boundary", "flags", "gamma", "lambda", "steps", "num_envs", "env_id_offset", "population",
              "group")
    consts = ("CP_RET_EPISODE_TOTAL", "CP_RET_DISCOUNTED", "CP_RET_GAE", "CP_RET_BOUNDARY_SAME_STEP",
              "CP_RET_BOUNDARY_STICKY", "CP_RET_BOUNDARY_NEXT_STEP", "CP_RET_MASK_OPEN", "CP_RET_STANDARDISE",
              "CP_ABI_VERSION")
    prog = tmp_path / "layout.c"
    prog.write_text(f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof(cp_returns));
  {' '.join(f'printf(" %zu", offsetof(cp_returns, {f}));' for f in fields)}
  {' '.join(f'printf(" %d", (int){c});' for c in consts)}
  printf(" %zu %zu\\n", sizeof(cp_policy), sizeof(cp_policy_es));
  return 0;
}}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    R = abi.cp_returns
    py_fields = [f if f != "lambda" else "lam" for f in fields]
    assert [n for n, _ in R._fields_] == py_fields
    assert out == [C.sizeof(R)] + [getattr(R, f).offset for f in py_fields] + \
        [getattr(abi, c) for c in consts] + [C.sizeof(abi.cp_policy), C.sizeof(abi.cp_policy_es)]
    assert out[:11] == [48, 0, 4, 8, 12, 16, 20, 24, 32, 40, 44]
    assert abi.RET_KINDS == {"episode_total": 0, "discounted": 1, "gae": 2}
    assert abi.RET_BOUNDARIES == {"same_step": 0, "sticky": 1, "next_step": 2}
    assert C.sizeof(abi.cp_policy) == 56 and C.sizeof(abi.cp_policy_es) == 32   # additive: ABI 8's structs stay


def test_abi_version_is_unchanged_and_the_symbols_are_exported():
    lib = native.load()
    assert lib.cp_abi_version() == 8 and abi.CP_ABI_VERSION == 8
    header = open(HEADER).read()
    for name in NEW:
        assert name in native.EXPORTS
        assert getattr(lib, name).argtypes is not None
        assert f" {name}(" in header
    assert len(lib.cp_returns_compute.argtypes) == 14


def _ret(kind=abi.CP_RET_EPISODE_TOTAL, boundary=0, flags=0, gamma=0.99, lam=0.95, steps=200, num_envs=4096,
         env_id_offset=0, population=1, group=1):
    p = abi.cp_returns()
    p.kind, p.boundary, p.flags, p.gamma, p.lam = kind, boundary, flags, gamma, lam
    p.steps, p.num_envs, p.env_id_offset, p.population, p.group = steps, num_envs, env_id_offset, population, group
    return p


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=3), b"kind must be"),
    (dict(kind=-1), b"kind must be"),
    (dict(boundary=3), b"boundary must be"),
    (dict(boundary=-1), b"boundary must be"),
    (dict(flags=0x4), b"unknown CP_RET_* bit"),
    (dict(flags=0x3 | 0x80000000), b"unknown CP_RET_* bit"),
    (dict(steps=0), b"steps must be >= 1"),
    (dict(num_envs=0), b"num_envs must be >= 1"),
    (dict(num_envs=-5), b"num_envs must be >= 1"),
    (dict(gamma=-0.1), b"gamma must be finite and in [0, 1]"),
    (dict(gamma=1.5), b"gamma must be finite and in [0, 1]"),
    (dict(gamma=float("nan")), b"gamma must be finite and in [0, 1]"),
    (dict(gamma=float("inf")), b"gamma must be finite and in [0, 1]"),
    (dict(lam=-0.1), b"lambda must be finite and in [0, 1]"),
    (dict(lam=1.0001), b"lambda must be finite and in [0, 1]"),
    (dict(lam=float("nan")), b"lambda must be finite and in [0, 1]"),
    (dict(population=-1), b"population must be >= 0"),
    (dict(population=2, group=0), b"group must be >= 1"),
    (dict(population=16, group=-3), b"group must be >= 1"),
    (dict(env_id_offset=-1), b"env_id_offset"),
])
def test_returns_check_rejections(kw, msg):
    lib = native.load()
    p = _ret(**kw)
    assert lib.cp_returns_check(C.byref(p)) < 0
    err = lib.cp_last_error(None)
    assert err.startswith(b"cp_returns_check: ") and msg in err, err
    assert lib.cp_returns_scratch_bytes(C.byref(p)) < 0
    assert lib.cp_last_error(None).startswith(b"cp_returns_scratch_bytes: ")
    # cp_returns_compute applies the same checks before it looks at a pointer or touches the GPU
    assert lib.cp_returns_compute(C.byref(p), *([None] * 13)) < 0
    assert lib.cp_last_error(None).startswith(b"cp_returns_compute: ") and msg in lib.cp_last_error(None)


def test_returns_check_null_and_accepted():
    lib = native.load()
    assert lib.cp_returns_check(None) < 0 and b"null" in lib.cp_last_error(None)
    for p in (_ret(), _ret(kind=abi.CP_RET_GAE, boundary=2, flags=3, gamma=0.0, lam=1.0, steps=1, num_envs=1),
              _ret(population=0, group=0), _ret(population=1, group=-7),
              _ret(kind=abi.CP_RET_DISCOUNTED, boundary=1, gamma=1.0, env_id_offset=(1 << 32) + 5, population=16,
                   group=256)):
        assert lib.cp_returns_check(C.byref(p)) == 0, lib.cp_last_error(None)


def test_scratch_bytes_and_null_pointer_rejections_need_no_gpu():
    lib = native.load()
    plain = lib.cp_returns_scratch_bytes(C.byref(_ret()))
    assert plain > 0
    std = lib.cp_returns_scratch_bytes(C.byref(_ret(flags=abi.CP_RET_STANDARDISE, population=16, group=256)))
    assert std >= 4096 * (4 + 8 + 8)          # per env: a count and two fp64 sums
    big = lib.cp_returns_scratch_bytes(C.byref(_ret(flags=abi.CP_RET_STANDARDISE, num_envs=65536)))
    assert big > std
    # the pointer checks come before any launch
    assert lib.cp_returns_compute(C.byref(_ret()), *([None] * 13)) < 0
    assert b"null reward, done, adv_out, valid_out or scratch" in lib.cp_last_error(None)


# ---- the restatement's own checks

R63 = (np.arange(1, 7, dtype=f32)[:, None] * np.array([1, 10, 100], f32)[None, :]).astype(f32)
D63 = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8)


def _cols(a):
    return [list(map(float, a[:, i])) for i in range(a.shape[1])]


def test_episode_total_hand_written_6x3():
    # env 0: done at k = 2; env 1: done at k = 1 and 4; env 2: never
    adv, valid, carry, ret = rr.raw(R63, D63, rr.EPISODE_TOTAL, rr.SAME_STEP)
    assert ret is None
    assert _cols(adv) == [[6, 6, 6, 0, 0, 0], [30, 30, 120, 120, 120, 0], [0] * 6]
    assert _cols(valid) == [[1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0], [0] * 6]
    assert list(carry) == [15, 60, 2100]

    adv, valid, carry, _ = rr.raw(R63, D63, rr.EPISODE_TOTAL, rr.STICKY)
    assert _cols(adv) == [[6, 6, 6, 0, 0, 0], [30, 30, 0, 0, 0, 0], [0] * 6]
    assert _cols(valid) == [[1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0] * 6]
    assert list(carry) == [0, 0, 2100]

    adv, valid, carry, _ = rr.raw(R63, D63, rr.EPISODE_TOTAL, rr.NEXT_STEP)
    assert _cols(adv) == [[6, 6, 6, 0, 0, 0], [30, 30, 0, 90, 90, 0], [0] * 6]
    assert _cols(valid) == [[1, 1, 1, 0, 0, 0], [1, 1, 0, 1, 1, 0], [0] * 6]
    assert list(carry) == [11, 0, 2100]          # env 0: k = 3 is the reset step, 5 + 6 stay open

    head = np.array([100, 0, 0.5], f32)
    din = np.array([1, 0, 0], np.uint8)
    adv, valid, carry, _ = rr.raw(R63, D63, rr.EPISODE_TOTAL, rr.SAME_STEP, head=head, done_in=din)
    assert _cols(adv)[0] == [106, 106, 106, 0, 0, 0] and list(carry) == [15, 60, 2100.5]   # done_in: no padding here
    adv, valid, carry, _ = rr.raw(R63, D63, rr.EPISODE_TOTAL, rr.NEXT_STEP, head=head, done_in=din)
    assert _cols(adv)[0] == [0, 5, 5, 0, 0, 0] and _cols(valid)[0] == [0, 1, 1, 0, 0, 0]    # head is not the segment's
    adv, valid, carry, _ = rr.raw(R63, D63, rr.EPISODE_TOTAL, rr.STICKY, head=head, done_in=din)
    assert _cols(adv)[0] == [0] * 6 and _cols(valid)[0] == [0] * 6 and carry[0] == 0
    assert _cols(adv)[1] == [30, 30, 0, 0, 0, 0] and carry[2] == f32(2100.5)


def test_padding_definitions():
    din = np.array([0, 0, 1], np.uint8)
    assert not rr.padding(D63, rr.SAME_STEP, din).any()
    s = rr.padding(D63, rr.STICKY, din)
    assert _cols(s) == [[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 1], [1] * 6]
    n = rr.padding(D63, rr.NEXT_STEP, din)
    assert _cols(n) == [[0, 0, 0, 1, 0, 0], [0, 0, 1, 0, 0, 1], [1, 0, 0, 0, 0, 0]]


def test_episode_total_is_lrpgs_sum_rewards_times_len_on_ragged_episodes():
    rng = np.random.default_rng(7)
    K, B = 40, 9
    reward = np.zeros((K, B), f32)
    done = np.zeros((K, B), np.uint8)
    want = np.zeros((K, B), f32)
    want_valid = np.zeros((K, B), np.uint8)
    for i in range(B):
        k = 0
        while k < K:
            n = int(rng.integers(1, 14))
            rewards = [f32(x) for x in rng.uniform(0.1, 2.0, n)]
            if k + n > K:                       # cut by the window: no done, no advantages
                reward[k:, i] = rewards[:K - k]
                break
            total = f32(0)
            for x in rewards:                   # sum(rewards), in float32
                total = f32(total + x)
            batch_advantages = [total] * len(rewards)
            reward[k:k + n, i] = rewards
            done[k + n - 1, i] = 1
            want[k:k + n, i] = batch_advantages
            want_valid[k:k + n, i] = 1
            k += n
    adv, valid, carry, _ = rr.raw(reward, done, rr.EPISODE_TOTAL, rr.SAME_STEP)
    assert np.array_equal(adv.view(np.uint32), want.view(np.uint32)) and np.array_equal(valid, want_valid)
    assert want_valid.min() == 0 and want_valid.sum() > K * B // 2
    for i in range(B):
        open_rewards = reward[:, i][np.flatnonzero(want_valid[:, i] == 0)]
        t = f32(0)
        for x in open_rewards:
            t = f32(t + x)
        assert carry[i] == t


def test_gae_with_lambda_1_is_discounted_minus_v_on_powers_of_two():
    rng = np.random.default_rng(3)
    K, B = 8, 16
    reward = (2.0 ** rng.integers(-1, 3, (K, B))).astype(f32)
    values = (2.0 ** rng.integers(-2, 4, (K + 1, B))).astype(f32)
    done = (rng.random((K, B)) < 0.2).astype(np.uint8)
    for boundary in rr.BOUNDARIES:
        for mask_open in (False, True):
            G, gv, _, _ = rr.raw(reward, done, rr.DISCOUNTED, boundary, gamma=0.5, tail=values[K], mask_open=mask_open)
            A, av, _, ret = rr.raw(reward, done, rr.GAE, boundary, gamma=0.5, lam=1.0, values=values,
                                   mask_open=mask_open)
            assert np.array_equal(gv, av) and gv.any()
            want = np.where(gv != 0, G - values[:K], 0).astype(f32)
            assert np.array_equal(A, want)
            assert np.array_equal(ret, G)         # A + V on the valid samples, 0 elsewhere
    # lambda = 0: the one-step TD error
    A, av, _, _ = rr.raw(reward, done, rr.GAE, rr.SAME_STEP, gamma=0.5, lam=0.0, values=values)
    td = reward + np.where(done != 0, 0, f32(0.5) * values[1:]) - values[:K]
    assert np.array_equal(A, td.astype(f32))


def test_discounted_by_hand_and_mask_open():
    r = np.array([[1], [2], [4], [8]], f32)
    d = np.array([[0], [1], [0], [0]], np.uint8)
    G, v, carry, _ = rr.raw(r, d, rr.DISCOUNTED, rr.SAME_STEP, gamma=0.5, tail=np.array([16], f32))
    assert _cols(G) == [[2, 2, 4 + 0.5 * (8 + 8), 8 + 8]] and _cols(v) == [[1, 1, 1, 1]] and carry[0] == 0
    G, v, _, _ = rr.raw(r, d, rr.DISCOUNTED, rr.SAME_STEP, gamma=0.5, tail=np.array([16], f32), mask_open=True)
    assert _cols(G) == [[2, 2, 0, 0]] and _cols(v) == [[1, 1, 0, 0]]
    G, v, _, _ = rr.raw(r, d, rr.DISCOUNTED, rr.NEXT_STEP, gamma=0.5)
    assert _cols(G) == [[2, 2, 0, 8]] and _cols(v) == [[1, 1, 0, 1]]
    G, v, _, _ = rr.raw(r, d, rr.DISCOUNTED, rr.STICKY, gamma=0.5)
    assert _cols(G) == [[2, 2, 0, 0]] and _cols(v) == [[1, 1, 0, 0]]


def test_standardise_is_util_standardise_per_member():
    rng = np.random.default_rng(5)
    K, B = 11, 12
    x = rng.normal(3.0, 2.0, (K, B)).astype(f32)
    valid = (rng.random((K, B)) < 0.8).astype(np.uint8)
    x = np.where(valid != 0, x, 0).astype(f32)
    out, stats = rr.standardise(x, valid)
    xs = x[valid != 0].astype(np.float64)
    mean = xs.mean()                                             # util.py:40-43, in float64
    std = np.sqrt(np.square(xs - mean).mean())
    assert np.allclose(out[valid != 0], (xs - mean) / std, rtol=1e-6, atol=1e-7)
    assert not out[valid == 0].any()
    assert stats.shape == (1, 4) and stats[0, 0] == xs.size and stats[0, 3] == 0
    assert abs(stats[0, 1] - mean) < 1e-12 and abs(stats[0, 2] - std) < 1e-12
    # per member: ((offset + i) // group) % population
    off, P, G = (1 << 32) + 5, 3, 2
    mem = rr.members(B, off, P, G)
    assert list(mem) == [((off + i) // G) % P for i in range(B)] and set(mem) == {0, 1, 2}
    out, stats = rr.standardise(x, valid, off, P, G)
    for m in range(P):
        sel = (valid != 0) & (mem == m)[None, :]
        xs = x[sel].astype(np.float64)
        assert stats[m, 0] == xs.size
        assert np.allclose(out[sel], (xs - xs.mean()) / xs.std(), rtol=1e-6, atol=1e-7)
        assert abs(out[sel].astype(np.float64).mean()) < 1e-6 and abs(out[sel].astype(np.float64).std() - 1) < 1e-6
    assert list(rr.members(5, 7, 1, 3)) == [0] * 5 and list(rr.members(5, 7, 0, 0)) == [0] * 5


def test_standardise_degenerate_members():
    x = np.full((4, 6), 5.0, f32)
    valid = np.ones((4, 6), np.uint8)
    valid[:, 4:] = 0                                             # member 2 (envs 4, 5) has no valid sample
    x[:, 2] = 7.0                                                # member 1 (envs 2, 3) is not constant
    out, stats = rr.standardise(x, valid, 0, 3, 2)
    assert not out[:, :2].any() and not out[:, 4:].any()         # "converged?": all totals equal -> zeros
    assert list(stats[0]) == [8, 5.0, 0.0, 1.0] and list(stats[2]) == [0, 0, 0, 1.0]
    assert list(stats[1]) == [8, 6.0, 1.0, 0.0]
    assert np.array_equal(out[:, 2], np.full(4, 1, f32)) and np.array_equal(out[:, 3], np.full(4, -1, f32))
