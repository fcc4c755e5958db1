"""In-kernel MLP policy, the parts that need no GPU: the restatement's fmaf emulation against exact
rational rounding, cp_policy_floats' values and rejections, the cp_policy ctypes layout against gcc, and
policy.pack's weight layout."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native, policy
from tests import policy_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpole_amd.h")


def _round_f32(q):
    """The float32 nearest to the rational q, ties to even (finite, in float32's range)."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                   # 2^e <= q < 2^(e+1)
    ulp = Fraction(2) ** (max(e, -126) - 23)     # subnormals share the smallest normal's spacing
    n, rem = divmod(q, ulp)
    n = int(n)
    if rem * 2 > ulp or (rem * 2 == ulp and n % 2 == 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * ulp))


def _exact_fmaf(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fmaf_emulation_random_triples():
    rng = np.random.default_rng(0)
    n = 4000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    c[::7] = (-(a[::7].astype(np.float64) * b[::7].astype(np.float64))).astype(np.float32)   # heavy cancellation
    got = ref.fmaf(a, b, c)
    exp = np.array([_exact_fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_fmaf_emulation_tie_cases():
    """a * b + c whose float64 sum lands exactly on a float32 tie while the exact value does not: rounding
    the float64 sum to float32 would go to even, the fused operation follows the residue."""
    f = np.float32
    cases = []
    for k in (1, 3, 12345, 2 ** 22 + 1):
        for sgn in (1.0, -1.0):
            base = f(1.0) + f(k) * f(2.0 ** -23)                 # a float32 in [1, 2) with an odd mantissa
            # half an ulp of [1, 2) is 2^-24: the product supplies it, exactly or a little off
            a, b = f(2.0 ** -12), f(2.0 ** -12)                  # a * b = 2^-24 exactly: a true tie
            cases.append((a, b, base))
            a2 = f(2.0 ** -12) * (f(1.0) + f(sgn) * f(2.0 ** -23))   # a2 * b = 2^-24 (1 +- 2^-23): off the tie
            cases.append((a2, b, base))
            a3 = f(2.0 ** -12) * (f(1.0) + f(2.0 ** -23))
            b3 = f(2.0 ** -12) * (f(1.0) - f(2.0 ** -23))        # a3 * b3 = 2^-24 (1 - 2^-46): below the tie by 2^-70
            cases.append((a3, b3, base))
            cases.append((a3, b3, -base))
            cases.append((-a3, b3, base))
    a, b, c = (np.array(x, np.float32) for x in zip(*cases))
    got = ref.fmaf(a, b, c)
    exp = np.array([_exact_fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # the cases do exercise the double rounding: the plain float64 route gets some of them wrong
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive.view(np.uint32) != exp.view(np.uint32)).any()


def _pol(widths, head, epsilon=0.0):
    p = abi.cp_policy()
    p.num_layers = len(widths) - 1
    for k, w in enumerate(widths[:abi.CP_POLICY_MAX_LAYERS + 1]):
        p.width[k] = w
    p.head = head
    p.epsilon = epsilon
    return p


def test_policy_floats_values():
    lib = native.load()
    assert lib.cp_policy_floats(C.byref(_pol((42, 100, 50, 10), abi.CP_HEAD_SAMPLE, 0.25))) == \
        100 * 43 + 50 * 101 + 10 * 51
    assert lib.cp_policy_floats(C.byref(_pol((42, 100, 100, 50, 4), abi.CP_HEAD_TANH))) == \
        100 * 43 + 100 * 101 + 50 * 101 + 4 * 51
    assert lib.cp_policy_floats(C.byref(_pol((14, 4), abi.CP_HEAD_CLIP))) == 4 * 15


@pytest.mark.parametrize("pol,msg", [
    (None, b"null"),
    (_pol((42,), abi.CP_HEAD_TANH), b"num_layers"),
    ((lambda p: (setattr(p, "num_layers", 5), p)[1])(_pol((42, 8, 8, 8, 4), abi.CP_HEAD_TANH)), b"num_layers"),
    (_pol((42, 0, 4), abi.CP_HEAD_TANH), b"width[1]"),
    (_pol((42, 129, 4), abi.CP_HEAD_TANH), b"width[1]"),
    (_pol((200, 8, 4), abi.CP_HEAD_TANH), b"width[0]"),
    (_pol((42, 8, 4), 4), b"head"),
    (_pol((42, 8, 4), -1), b"head"),
    (_pol((42, 8, 10), abi.CP_HEAD_TANH), b"out width must be 4"),
    (_pol((42, 8, 10), abi.CP_HEAD_CLIP), b"out width must be 4"),
    (_pol((42, 8, 4), abi.CP_HEAD_ARGMAX), b"out width must be 10"),
    (_pol((42, 8, 5), abi.CP_HEAD_SAMPLE), b"out width must be 10"),
    (_pol((42, 8, 10), abi.CP_HEAD_SAMPLE, 1.5), b"epsilon"),
    (_pol((42, 8, 10), abi.CP_HEAD_SAMPLE, -0.1), b"epsilon"),
    (_pol((42, 8, 10), abi.CP_HEAD_SAMPLE, float("nan")), b"epsilon"),
])
def test_policy_floats_rejections(pol, msg):
    lib = native.load()
    assert lib.cp_policy_floats(None if pol is None else C.byref(pol)) < 0
    err = lib.cp_last_error(None)
    assert err.startswith(b"cp_policy_floats: ") and msg in err, err


def test_set_policy_null_handle_rejected():
    lib = native.load()
    assert lib.cp_set_policy(None, None) != 0
    assert lib.cp_policy_act(None, None, None, None, None) != 0


def test_cp_policy_ctypes_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cp_policy), offsetof(cp_policy, num_layers),
         offsetof(cp_policy, width), offsetof(cp_policy, head), offsetof(cp_policy, epsilon),
         offsetof(cp_policy, seed), offsetof(cp_policy, weights));
  printf("%d %d %d %d %d %d %d\\n", CP_POLICY_MAX_LAYERS, CP_POLICY_MAX_WIDTH, CP_HEAD_TANH, CP_HEAD_CLIP,
         CP_HEAD_ARGMAX, CP_HEAD_SAMPLE, CP_ABI_VERSION);
  return 0;
}}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    P = abi.cp_policy
    assert list(map(int, out[0].split())) == [C.sizeof(P), P.num_layers.offset, P.width.offset, P.head.offset,
                                              P.epsilon.offset, P.seed.offset, P.weights.offset]
    assert list(map(int, out[1].split())) == [abi.CP_POLICY_MAX_LAYERS, abi.CP_POLICY_MAX_WIDTH, abi.CP_HEAD_TANH,
                                              abi.CP_HEAD_CLIP, abi.CP_HEAD_ARGMAX, abi.CP_HEAD_SAMPLE,
                                              abi.CP_ABI_VERSION]


def test_pack_layout():
    rng = np.random.default_rng(3)
    layers = ref.random_layers(rng, (28, 7, 5, 10))
    packed, pol = policy.pack([(torch.from_numpy(W), torch.from_numpy(b)) for W, b in layers], "sample",
                              epsilon=0.25, seed=(5 << 32) | 9, device="cpu")
    assert packed.dtype == torch.float32 and packed.is_contiguous()
    assert np.array_equal(packed.numpy(), ref.packed(layers))
    assert pol.num_layers == 3 and list(pol.width)[:4] == [28, 7, 5, 10] and pol.head == abi.CP_HEAD_SAMPLE
    assert pol.epsilon == 0.25 and pol.seed == (5 << 32) | 9 and pol.weights == packed.data_ptr()
    # W[out][in] row-major then b[out]: layer 1 starts after layer 0's 7 * 28 + 7 floats
    assert packed[7 * 29 + 2 * 7 + 3].item() == layers[1][0][2, 3]
    assert packed[7 * 28 + 4].item() == layers[0][1][4]
    # an nn.Sequential of Linear / ReLU packs the same
    seq = torch.nn.Sequential(torch.nn.Linear(28, 7), torch.nn.ReLU(), torch.nn.Linear(7, 5), torch.nn.ReLU(),
                              torch.nn.Linear(5, 10))
    with torch.no_grad():
        for m, (W, b) in zip([seq[0], seq[2], seq[4]], layers):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    packed2, _ = policy.pack(seq, "argmax", device="cpu")
    assert torch.equal(packed, packed2)
    # repack writes in place
    layers2 = ref.random_layers(rng, (28, 7, 5, 10))
    ptr = packed.data_ptr()
    policy.repack(packed, [(torch.from_numpy(W), torch.from_numpy(b)) for W, b in layers2])
    assert packed.data_ptr() == ptr and np.array_equal(packed.numpy(), ref.packed(layers2))
    with pytest.raises(ValueError):
        policy.pack([(torch.zeros(7, 28), torch.zeros(7)), (torch.zeros(10, 8), torch.zeros(10))], "argmax", device="cpu")
    with pytest.raises(ValueError):
        policy.pack(layers[:1], "softmax", device="cpu")
    with pytest.raises(native.CartpoleError):   # head / out width mismatch, through cp_policy_floats
        policy.pack([(torch.zeros(7, 28), torch.zeros(7))], "argmax", device="cpu")


def test_restatement_heads():
    z = np.array([[0.5, 2.0, -3.0, 0.25, 1.0, 1.0, 1.0, 0.0, -1.0, 1.0]], np.float32)
    assert ref.act_argmax(z).tolist() == [[1, 0]]          # the lowest index among equal maxima
    zc = np.array([[0.5, 2.0, -3.0, 0.25]], np.float32)
    assert ref.act_clip(zc, np.array([[[0.25, 0.0], [0.0, -0.5]]], np.float32)).tolist() == [[[0.75, 1.0], [-1.0, -0.25]]]
    # one ReLU layer by hand
    layers = [(np.array([[1.0, -2.0], [0.5, 0.5]], np.float32), np.array([0.0, -1.0], np.float32)),
              (np.array([[1.0, 1.0]], np.float32), np.array([0.25], np.float32))]
    assert ref.forward(layers, np.array([[3.0, 1.0]], np.float32)).tolist() == [[1.0 + 1.0 + 0.25]]
