"""Packing of a dense ReLU MLP for the in-kernel policy (include/cartpole_amd.h: cp_policy).

    packed, pol = policy.pack(actor, "tanh", device=env.device)     # nn.Sequential of Linear / ReLU
    packed, pol = policy.pack([(W0, b0), (W1, b1)], "sample", epsilon=0.05, seed=7)

The packed tensor holds the layers one after another, per layer W[out][in] row-major, then b[out].
The library reads it at every launch and never copies it: keep it alive while the policy is set, and
write new weights into it in place (`policy.repack`) to have the next launch use them.
"""
import ctypes as C

import torch

from . import abi, native


def _layers(layers):
    """[(W (out, in), b (out,)), ...] from a list of pairs or an nn.Sequential of Linear / ReLU."""
    if isinstance(layers, torch.nn.Module):
        mods = list(layers.children()) if isinstance(layers, torch.nn.Sequential) else [layers]
        out = []
        for k, m in enumerate(mods):
            if isinstance(m, torch.nn.Linear):
                if out and not isinstance(mods[k - 1], torch.nn.ReLU):
                    raise ValueError("policy: consecutive Linear layers need a ReLU between them")
                b = m.bias if m.bias is not None else torch.zeros(m.out_features)
                out.append((m.weight, b))
            elif isinstance(m, torch.nn.ReLU):
                if not out or k + 1 == len(mods) or not isinstance(mods[k + 1], torch.nn.Linear):
                    raise ValueError("policy: a ReLU stands between two Linear layers (the head is separate)")
            else:
                raise ValueError(f"policy: only Linear and ReLU modules are supported, got {type(m).__name__}")
        return out
    return [(torch.as_tensor(W), torch.as_tensor(b)) for W, b in layers]


def _flat(layers):
    ls = _layers(layers)
    if not 1 <= len(ls) <= abi.CP_POLICY_MAX_LAYERS:
        raise ValueError(f"policy: 1..{abi.CP_POLICY_MAX_LAYERS} dense layers, got {len(ls)}")
    widths, parts = [], []
    for k, (W, b) in enumerate(ls):
        if W.dim() != 2 or b.dim() != 1 or b.shape[0] != W.shape[0]:
            raise ValueError(f"policy: layer {k} needs W (out, in) and b (out,), got {tuple(W.shape)} and {tuple(b.shape)}")
        if widths and W.shape[1] != widths[-1]:
            raise ValueError(f"policy: layer {k} takes {W.shape[1]} inputs, the layer before gives {widths[-1]}")
        if not widths:
            widths.append(int(W.shape[1]))
        widths.append(int(W.shape[0]))
        parts += [W.detach().to(torch.float32).reshape(-1), b.detach().to(torch.float32).reshape(-1)]
    return widths, parts


def pack(layers, head, epsilon=0.0, seed=0, device="cuda"):
    """-> (packed float32 device tensor, abi.cp_policy pointing at it)."""
    if head not in abi.HEADS:
        raise ValueError(f"policy: head must be one of {sorted(abi.HEADS)}, got {head!r}")
    widths, parts = _flat(layers)
    device = torch.device(device)
    packed = torch.cat([p.to(device) for p in parts]).contiguous()
    pol = abi.cp_policy()
    pol.num_layers = len(widths) - 1
    for k, w in enumerate(widths):
        pol.width[k] = w
    pol.head = abi.HEADS[head]
    pol.epsilon = float(epsilon)
    pol.seed = int(seed)
    pol.weights = packed.data_ptr()
    n = native.load().cp_policy_floats(C.byref(pol))
    if n < 0:
        native.check(None, -1, "cp_policy_floats")
    if n != packed.numel():
        raise native.CartpoleError(f"policy: packed {packed.numel()} floats, cp_policy_floats says {n}")
    return packed, pol


def repack(packed, layers):
    """Write new weights of the same architecture into `packed` in place (read by the next launch)."""
    _, parts = _flat(layers)
    flat = torch.cat([p.to(packed.device) for p in parts])
    if flat.numel() != packed.numel():
        raise ValueError(f"policy: {flat.numel()} floats for a packed tensor of {packed.numel()}")
    packed.copy_(flat)
    return packed
