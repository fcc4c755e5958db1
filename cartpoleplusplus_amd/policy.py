"""Packing of a dense ReLU MLP for the in-kernel policy (include/cartpole_amd.h: cp_policy).

    packed, pol = policy.pack(actor, "tanh", device=env.device)     # nn.Sequential of Linear / ReLU
    packed, pol = policy.pack([(W0, b0), (W1, b1)], "sample", epsilon=0.05, seed=7)

The packed tensor holds the layers one after another, per layer W[out][in] row-major, then b[out].
The library reads it at every launch and never copies it: keep it alive while the policy is set, and
write new weights into it in place (`policy.repack`) to have the next launch use them.

A population is P networks of one architecture behind one handle: `group` consecutive global env ids share a
member, and the members wrap (`member_of`):

    packed, pol = policy.pack_population([actor_0, ..., actor_15], "sample", group=4096)   # packed (16, F)
    policy.repack(packed[3], actor_3)                          # member 3 alone, in place
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


def _is_stacked(members):
    """One stacked population [(W (P, out, in), b (P, out)), ...] rather than a list of members."""
    if isinstance(members, torch.nn.Module) or not len(members):
        return False
    first = members[0]
    return (isinstance(first, (tuple, list)) and len(first) == 2 and hasattr(first[0], "ndim") and first[0].ndim == 3)


def member_of(gid, group, population):
    """The member that the env with global id `gid` (env_id_offset + i; an int or an integer array) reads:
    (gid // group) % population."""
    return (gid // group) % population


def pack_population(members, head, group, epsilon=0.0, seed=0, device="cuda"):
    """-> (packed (P, F) float32 device tensor, abi.cp_policy pointing at it) for P members of one architecture:
    a list of nn.Sequentials or of [(W, b), ...] lists, or one already stacked list [(W (P, out, in), b (P, out)),
    ...].  packed[m] is what pack(members[m]) gives.  Head, epsilon and seed are shared by all members."""
    if head not in abi.HEADS:
        raise ValueError(f"policy: head must be one of {sorted(abi.HEADS)}, got {head!r}")
    if int(group) < 1:
        raise ValueError(f"policy: group must be >= 1, got {group}")
    device = torch.device(device)
    if _is_stacked(members):
        pairs = [(torch.as_tensor(W), torch.as_tensor(b)) for W, b in members]
        P = pairs[0][0].shape[0]
        if any(W.dim() != 3 or b.dim() != 2 or W.shape[0] != P or b.shape[0] != P for W, b in pairs):
            raise ValueError("policy: a stacked population needs W (P, out, in) and b (P, out) in every layer")
        widths, _ = _flat([(W[0], b[0]) for W, b in pairs])   # member 0 stands for the architecture checks
        packed = torch.cat([t.detach().to(device=device, dtype=torch.float32).reshape(P, -1)
                            for W, b in pairs for t in (W, b)], dim=1).contiguous()
    else:
        members = list(members)
        if not members:
            raise ValueError("policy: a population needs at least one member")
        flat = [_flat(m) for m in members]
        widths = flat[0][0]
        for k, (w, _) in enumerate(flat):
            if w != widths:
                raise ValueError(f"policy: member {k} has widths {w}, member 0 has {widths} (one architecture per population)")
        packed = torch.stack([torch.cat([p.to(device) for p in parts]) for _, parts in flat]).contiguous()
    pol = abi.cp_policy()
    pol.num_layers = len(widths) - 1
    for k, w in enumerate(widths):
        pol.width[k] = w
    pol.head = abi.HEADS[head]
    pol.epsilon = float(epsilon)
    pol.seed = int(seed)
    pol.weights = packed.data_ptr()
    pol.population = packed.shape[0]
    pol.group = int(group)
    n = native.load().cp_policy_floats(C.byref(pol))
    if n < 0:
        native.check(None, -1, "cp_policy_floats")
    if n != packed.shape[1]:
        raise native.CartpoleError(f"policy: {packed.shape[1]} floats per member, cp_policy_floats says {n}")
    return packed, pol


def repack(packed, layers):
    """Write new weights of the same architecture into `packed` in place (read by the next launch)."""
    _, parts = _flat(layers)
    flat = torch.cat([p.to(packed.device) for p in parts])
    if flat.numel() != packed.numel():
        raise ValueError(f"policy: {flat.numel()} floats for a packed tensor of {packed.numel()}")
    packed.copy_(flat)
    return packed


def unpack(packed_row, like):
    """The inverse of repack: [(W (out, in), b (out,)), ...] views of one packed row (F,), for the architecture
    of `like` (an nn.Sequential, a list of (W, b) pairs, or a list of widths (in, h1, .., out)).  With `like` a
    module, its parameters are also overwritten with the row's values (a checkpoint loaded back into torch)."""
    if isinstance(like, (list, tuple)) and like and all(isinstance(w, int) for w in like):
        widths = list(like)
    else:
        widths, _ = _flat(like)
    row = packed_row.reshape(-1)
    n = sum(o * (i + 1) for i, o in zip(widths[:-1], widths[1:]))
    if row.numel() != n:
        raise ValueError(f"policy: a packed row of {row.numel()} floats for widths {widths} ({n} floats)")
    out, at = [], 0
    for i, o in zip(widths[:-1], widths[1:]):
        out.append((row[at:at + o * i].view(o, i), row[at + o * i:at + o * i + o]))
        at += o * i + o
    if isinstance(like, torch.nn.Module):
        with torch.no_grad():
            for (W, b), (Wm, bm) in zip(out, _layers(like)):
                Wm.copy_(W)
                if isinstance(bm, torch.nn.Parameter):
                    bm.copy_(b)
    return out
