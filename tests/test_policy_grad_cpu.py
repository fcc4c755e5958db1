"""cp_policy_gradient, the parts that need no GPU: the two exported symbols, the NULL-handle rejection of
cp_policy_gradient_scratch_bytes, self-checks of the numpy restatement (tests/policy_grad_ref.py) the GPU tests
compare against (torch float64 autograd of INTEGRATION.md's loss, a central finite difference, a hand-written
one-layer case, a unit at acc == 0), policy.unpack, and the work split (tests/policy_grad_plan.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import native, policy
from tests import policy_grad_ref as gref
from tests import policy_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpole_amd.h")
NEW = ("cp_policy_gradient_scratch_bytes", "cp_policy_gradient")
CXX = shutil.which("c++") or shutil.which("g++")


def test_the_symbols_are_declared_listed_and_exported():
    header = open(HEADER).read()
    assert "int64_t cp_policy_gradient_scratch_bytes(const cp_handle* h, int steps);" in header
    assert "int cp_policy_gradient(cp_handle* h, int steps" in header
    assert "#define CP_ABI_VERSION 8" in header
    for name in NEW:
        assert name in native.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported


def test_scratch_bytes_rejects_a_null_handle():
    lib = native.load()
    assert lib.cp_policy_gradient_scratch_bytes(None, 1) < 0
    assert b"null handle" in lib.cp_last_error(None)


def _case(rng, widths, N, scale=1.0):
    layers = ref.random_layers(rng, widths, scale=scale)
    x = rng.standard_normal((N, widths[0])).astype(np.float32)
    a = rng.integers(0, 5, (N, 2)).astype(np.int8)
    c = rng.standard_normal(N).astype(np.float32)
    return layers, x, a, c


@pytest.mark.parametrize("widths", [(14, 7, 5, 10), (42, 100, 50, 10), (28, 10), (14, 12, 12, 12, 10)])
def test_reference_against_torch_autograd(widths):
    """INTEGRATION.md's loss -(chosen * adv).mean() in float64: its gradient is -1/N times the reference's sum."""
    rng = np.random.default_rng(sum(widths))
    N = 48
    layers, x, a, c = _case(rng, widths, N)
    g = gref.gradient(layers, x, a, c)
    params = [(torch.tensor(W, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True))
              for W, b in layers]
    h = torch.tensor(x, dtype=torch.float64)
    for k, (W, b) in enumerate(params):
        h = h @ W.T + b
        if k + 1 < len(params):
            h = torch.relu(h)
    logp = torch.log_softmax(h.view(-1, 2, 5), -1)
    chosen = logp.gather(-1, torch.tensor(a, dtype=torch.int64).unsqueeze(-1)).squeeze(-1).sum(-1)
    loss = -(chosen * torch.tensor(c, dtype=torch.float64)).mean()
    loss.backward()
    want = -N * np.concatenate([np.concatenate([W.grad.numpy().reshape(-1), b.grad.numpy()]) for W, b in params])
    # the reference's forward pass is fp32 (relative error ~ width * 2^-24), torch's float64
    err = np.abs(g["grad"] - want)
    assert (err <= 2e-5 * g["absscale"] + 1e-12).all(), float((err / (g["absscale"] + 1e-30)).max())
    assert np.abs(g["logp"] - chosen.detach().numpy()).max() < 1e-4
    assert g["n"] == N and (g["absscale"] >= np.abs(g["grad"]) * (1 - 1e-12)).all()


def _objective64(layers, x, a, c):
    h = x.astype(np.float64)
    for k, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        if k + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return float((c.astype(np.float64) * gref.logp64(h, a)[0]).sum())


def test_reference_against_a_central_finite_difference():
    rng = np.random.default_rng(5)
    widths = (14, 9, 6, 10)
    layers, x, a, c = _case(rng, widths, 32)
    g = gref.gradient(layers, x, a, c)
    flat = ref.packed(layers).astype(np.float64)

    def unflat(v):
        out, at = [], 0
        for i, o in zip(widths[:-1], widths[1:]):
            out.append((v[at:at + o * i].reshape(o, i), v[at + o * i:at + o * i + o]))
            at += o * i + o
        return out

    h = 1e-6
    for f in rng.choice(len(flat), 40, replace=False):
        up, dn = flat.copy(), flat.copy()
        up[f] += h
        dn[f] -= h
        fd = (_objective64(unflat(up), x, a, c) - _objective64(unflat(dn), x, a, c)) / (2 * h)
        assert abs(fd - g["grad"][f]) <= 1e-4 * g["absscale"][f] + 1e-7, (f, fd, g["grad"][f])


def test_hand_written_one_layer_case():
    """W = 0, b = 0: z = 0, every probability 1/5, logp = 2 log(1/5); db = c (onehot - 1/5), dW = db x^T."""
    x = np.arange(1, 15, dtype=np.float32)[None, :] / 8
    layers = [(np.zeros((10, 14), np.float32), np.zeros(10, np.float32))]
    g = gref.gradient(layers, x, np.array([[3, 0]], np.int8), np.array([2.0], np.float32))
    assert np.isclose(g["logp"][0], 2 * np.log(0.2), rtol=0, atol=1e-15)
    db = np.full(10, -0.4)
    db[3] = db[5] = 1.6
    assert np.allclose(g["grad"][140:], db, rtol=0, atol=1e-15)
    assert np.allclose(g["grad"][:140].reshape(10, 14), db[:, None] * x.astype(np.float64), rtol=0, atol=1e-15)
    # skipped samples: coeff 0, or an action outside 0..4
    for a, c in (([3, 0], 0.0), ([3, 0], -0.0), ([5, 0], 1.0), ([0, -1], 1.0)):
        s = gref.gradient(layers, x, np.array([a], np.int8), np.array([c], np.float32))
        assert s["n"] == 0 and not s["grad"].any() and not s["absscale"].any() and s["logp"][0] == 0 and not s["z"].any()


def test_a_unit_at_acc_zero_passes_no_gradient():
    """Hidden unit 1 has W = 0 and b = 0: acc == 0 exactly, relu'(0) = 0, so its row of dW and its db are 0 although
    the next layer's weights on it are not; unit 0 (acc > 0) does pass gradient."""
    x = np.ones((3, 14), np.float32)
    W0 = np.zeros((2, 14), np.float32)
    W0[0] = 0.25
    rng = np.random.default_rng(1)
    W1 = rng.standard_normal((10, 2)).astype(np.float32)
    layers = [(W0, np.zeros(2, np.float32)), (W1, np.zeros(10, np.float32))]
    g = gref.gradient(layers, x, np.array([[1, 2]] * 3, np.int8), np.ones(3, np.float32))
    dW0, db0 = g["grad"][:28].reshape(2, 14), g["grad"][28:30]
    assert not dW0[1].any() and db0[1] == 0 and not g["absscale"][14:28].any()
    assert dW0[0].all() and db0[0] != 0


def test_unpack_is_the_inverse_of_repack():
    rng = np.random.default_rng(2)
    widths = (28, 7, 5, 10)
    layers = ref.random_layers(rng, widths)
    packed, _ = policy.pack([(torch.from_numpy(W), torch.from_numpy(b)) for W, b in layers], "sample", device="cpu")
    for like in (list(widths), [(torch.zeros(o, i), torch.zeros(o)) for i, o in zip(widths[:-1], widths[1:])]):
        got = policy.unpack(packed, like)
        for (W, b), (Wr, br) in zip(got, layers):
            assert np.array_equal(W.numpy(), Wr) and np.array_equal(b.numpy(), br)
    net = torch.nn.Sequential(torch.nn.Linear(28, 7), torch.nn.ReLU(), torch.nn.Linear(7, 5), torch.nn.ReLU(),
                              torch.nn.Linear(5, 10))
    policy.unpack(packed, net)
    assert torch.equal(policy.repack(torch.empty_like(packed), net), packed)
    with pytest.raises(ValueError):
        policy.unpack(packed[:-1], list(widths))


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_work_split(tmp_path):
    exe = str(tmp_path / "policy_grad_plan")
    subprocess.run([CXX, "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "policy_grad_plan.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
