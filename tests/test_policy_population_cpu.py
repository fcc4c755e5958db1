"""Policy populations (cp_policy.population / group, ABI 8), the parts that need no GPU: the ctypes layout
against gcc, cp_policy_floats' per-member values and the two new rejections, policy.pack_population's layout,
policy.member_of against a brute-force loop, and the member path's work split (tests/policy_runs.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native, policy
from tests import policy_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpole_amd.h")
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")


def _pol(widths, head, population=0, group=0):
    p = abi.cp_policy()
    p.num_layers = len(widths) - 1
    for k, w in enumerate(widths):
        p.width[k] = w
    p.head = head
    p.population, p.group = population, group
    return p


def test_cp_policy_ctypes_layout_with_population_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(cp_policy), offsetof(cp_policy, num_layers),
         offsetof(cp_policy, width), offsetof(cp_policy, head), offsetof(cp_policy, epsilon),
         offsetof(cp_policy, seed), offsetof(cp_policy, weights), offsetof(cp_policy, population),
         offsetof(cp_policy, group), CP_ABI_VERSION);
  return 0;
}}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    P = abi.cp_policy
    assert out == [C.sizeof(P), P.num_layers.offset, P.width.offset, P.head.offset, P.epsilon.offset, P.seed.offset,
                   P.weights.offset, P.population.offset, P.group.offset, abi.CP_ABI_VERSION]
    # appended after weights: the ABI 7 fields keep their offsets
    assert (P.num_layers.offset, P.width.offset, P.head.offset, P.epsilon.offset, P.seed.offset,
            P.weights.offset) == (0, 4, 24, 28, 32, 40)
    assert P.population.offset == 48 and P.group.offset == 52 and abi.CP_ABI_VERSION == 8
    assert native.load().cp_abi_version() == 8


@pytest.mark.parametrize("population,group", [(0, 0), (1, 0), (1, -3), (7, 1), (7, 64)])
def test_policy_floats_is_per_member(population, group):
    lib = native.load()
    assert lib.cp_policy_floats(C.byref(_pol((42, 100, 50, 10), abi.CP_HEAD_ARGMAX, population, group))) == \
        100 * 43 + 50 * 101 + 10 * 51
    assert lib.cp_policy_floats(C.byref(_pol((42, 100, 100, 50, 4), abi.CP_HEAD_TANH, population, group))) == \
        100 * 43 + 100 * 101 + 50 * 101 + 4 * 51
    assert lib.cp_policy_floats(C.byref(_pol((14, 4), abi.CP_HEAD_CLIP, population, group))) == 4 * 15


@pytest.mark.parametrize("population,group,msg", [
    (-1, 1, b"population must be >= 0"),
    (-5, 0, b"population must be >= 0"),
    (2, 0, b"group must be >= 1"),
    (7, -64, b"group must be >= 1"),
])
def test_policy_floats_population_rejections(population, group, msg):
    lib = native.load()
    assert lib.cp_policy_floats(C.byref(_pol((42, 8, 10), abi.CP_HEAD_ARGMAX, population, group))) < 0
    err = lib.cp_last_error(None)
    assert err.startswith(b"cp_policy_floats: ") and msg in err, err


def _t(layers):
    return [(torch.from_numpy(W), torch.from_numpy(b)) for W, b in layers]


def test_pack_population_layout():
    rng = np.random.default_rng(4)
    widths = (28, 7, 5, 10)
    members = [ref.random_layers(rng, widths) for _ in range(5)]
    packed, pol = policy.pack_population([_t(m) for m in members], "sample", group=8, epsilon=0.25,
                                         seed=(5 << 32) | 9, device="cpu")
    F = 7 * 29 + 5 * 8 + 10 * 6
    assert packed.shape == (5, F) and packed.dtype == torch.float32 and packed.is_contiguous()
    for m, layers in enumerate(members):
        single, _ = policy.pack(_t(layers), "sample", device="cpu")
        assert torch.equal(packed[m], single), f"member {m}"
        assert np.array_equal(packed[m].numpy(), ref.packed(layers))
    assert pol.population == 5 and pol.group == 8 and pol.num_layers == 3 and list(pol.width)[:4] == list(widths)
    assert pol.head == abi.CP_HEAD_SAMPLE and pol.epsilon == 0.25 and pol.seed == (5 << 32) | 9
    assert pol.weights == packed.data_ptr()
    # nn.Sequential members, and one already stacked list, pack the same
    seqs = []
    for layers in members:
        seq = torch.nn.Sequential(torch.nn.Linear(28, 7), torch.nn.ReLU(), torch.nn.Linear(7, 5), torch.nn.ReLU(),
                                  torch.nn.Linear(5, 10))
        with torch.no_grad():
            for mod, (W, b) in zip([seq[0], seq[2], seq[4]], layers):
                mod.weight.copy_(torch.from_numpy(W))
                mod.bias.copy_(torch.from_numpy(b))
        seqs.append(seq)
    assert torch.equal(policy.pack_population(seqs, "argmax", group=1, device="cpu")[0], packed)
    stacked = [(torch.from_numpy(np.stack([m[k][0] for m in members])), torch.from_numpy(np.stack([m[k][1] for m in members])))
               for k in range(3)]
    packed3, pol3 = policy.pack_population(stacked, "argmax", group=3, device="cpu")
    assert torch.equal(packed3, packed) and pol3.population == 5 and pol3.group == 3
    # repack on a row view: one member in place, the others and the buffer untouched
    before, ptr = packed.clone(), packed.data_ptr()
    new = ref.random_layers(rng, widths)
    policy.repack(packed[3], _t(new))
    assert packed.data_ptr() == ptr and np.array_equal(packed[3].numpy(), ref.packed(new))
    keep = [0, 1, 2, 4]
    assert torch.equal(packed[keep], before[keep])


def test_pack_population_errors():
    rng = np.random.default_rng(5)
    a, b = _t(ref.random_layers(rng, (28, 7, 5, 10))), _t(ref.random_layers(rng, (28, 7, 6, 10)))
    with pytest.raises(ValueError, match="member 1 has widths"):
        policy.pack_population([a, b], "argmax", group=4, device="cpu")
    with pytest.raises(ValueError, match="group"):
        policy.pack_population([a, a], "argmax", group=0, device="cpu")
    with pytest.raises(ValueError, match="head"):
        policy.pack_population([a, a], "softmax", group=1, device="cpu")
    with pytest.raises(ValueError, match="at least one member"):
        policy.pack_population([], "argmax", group=1, device="cpu")
    with pytest.raises(native.CartpoleError):      # head / out width mismatch, through cp_policy_floats
        policy.pack_population([a, a], "tanh", group=1, device="cpu")


@pytest.mark.parametrize("off,G,P,n", [
    (0, 64, 3, 200), (0, 1, 7, 50), (32, 64, 3, 128), (0, 5, 2, 33), (7, 96, 130, 130),
    ((1 << 32) + 7, 5, 7, 130), ((1 << 40) + 3, 4096, 16, 64), (0, 1, 3, 3),
])
def test_member_of_against_a_loop(off, G, P, n):
    k0, r = divmod(off, G)          # Python ints: exact above 2^32
    m, exp = k0 % P, []
    for _ in range(n):              # walk the ids one by one: a new member every G ids, wrapping after P
        exp.append(m)
        r += 1
        if r == G:
            r, m = 0, m + 1
            if m == P:
                m = 0
    got = policy.member_of(off + np.arange(n, dtype=np.int64), G, P)
    assert got.dtype == np.int64 and got.tolist() == exp
    assert [policy.member_of(off + i, G, P) for i in range(n)] == exp
    if P * G < n:
        assert exp[P * G] == exp[0] and len(set(exp)) == P      # the members wrap


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_member_path_work_split(tmp_path):
    exe = str(tmp_path / "policy_runs")
    subprocess.run([CXX, "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "policy_runs.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
