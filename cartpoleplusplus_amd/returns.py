"""Episode returns, GAE and standardised advantages of a rollout window, on the device (cp_returns_compute;
the arithmetic contract is spelled out in include/cartpole_amd.h).

    adv = advantages(reward, done, standardise=True)                 # lrpg: episode totals, standardised
    adv = advantages(reward, done, "gae", gamma=0.99, lam=0.95, values=v)

reward (K, B) float32 and done (K, B) uint8 are what K `BatchedCartpole.step` calls or one `rollout` return;
`BatchedCartpole.advantages` fills in the boundary convention, env_id_offset and the population from the handle.
"""
import collections
import ctypes as C

import torch

from . import abi, native

Advantages = collections.namedtuple("Advantages", "adv valid carry ret stats")
Advantages.__doc__ = """adv (K, B) float32, valid (K, B) uint8, carry (B,) float32 (the next window's `head`),
ret (K, B) float32 (GAE: adv + V, never standardised; None otherwise), stats (P, 4) float64 (standardise: n, mean,
std, degenerate per member; None otherwise)."""

_scratch = {}   # (device, stream) -> uint8 tensor, grow-only: calls on one stream are ordered, so they may share it


def _scratch_for(device, stream, nbytes):
    t = _scratch.get((device, stream))
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 256), device=device, dtype=torch.uint8)
        _scratch[(device, stream)] = t
    return t


def _buffer(t, shape, dtype, device, name):
    """t as it is, or ValueError: the library reads raw device pointers of exactly this layout."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name}: expected device {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def advantages(reward, done, kind="episode_total", *, gamma=1.0, lam=1.0, values=None, head=None, done_in=None,
               tail=None, boundary="same_step", mask_open=False, standardise=False, population=1, group=1,
               env_id_offset=0, stream=None):
    """Advantages(adv, valid, carry, ret, stats) of the window reward / done (K, B).

    kind "episode_total" (every step of a finished episode gets the episode's total reward; `head` (B,) carries
    the partial totals of the previous window in, `carry` out), "discounted" (reward-to-go with gamma; `tail`
    (B,) is the return after the window) or "gae" (GAE(gamma, lam) on values (K + 1, B)).  boundary "same_step"
    (autoreset), "sticky" (no autoreset: everything after an env's first done is padding) or "next_step" (the
    sample after a done sample is the reset step); done_in (B,) uint8 is the done row before the window.
    mask_open invalidates the samples of an episode still open at the window's end (always so for
    "episode_total").  standardise: (x - mean) / std over the valid samples, per population member
    ((env_id_offset + i) // group) % population, in float64; a member with no valid sample or std 0 gets zeros.
    Invalid samples have adv 0.  Inputs must be contiguous tensors of exactly these dtypes on one GPU."""
    if kind not in abi.RET_KINDS:
        raise ValueError(f"kind must be one of {sorted(abi.RET_KINDS)}, got {kind!r}")
    if boundary not in abi.RET_BOUNDARIES:
        raise ValueError(f"boundary must be one of {sorted(abi.RET_BOUNDARIES)}, got {boundary!r}")
    if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
        raise ValueError("reward: expected a (K, B) float32 tensor")
    if reward.device.type != "cuda":
        raise ValueError(f"reward: expected a GPU tensor, got device {reward.device} (there is no CPU fallback)")
    K, B = reward.shape
    dev = reward.device
    f32, u8 = torch.float32, torch.uint8
    reward = _buffer(reward, (K, B), f32, dev, "reward")
    done = _buffer(done, (K, B), u8, dev, "done")
    gae = kind == "gae"
    if gae and values is None:
        raise ValueError("kind 'gae' needs values (K + 1, B)")
    if not gae and values is not None:
        raise ValueError("values is for kind 'gae'")
    values = _buffer(values, (K + 1, B), f32, dev, "values")
    head = _buffer(head, (B,), f32, dev, "head")
    done_in = _buffer(done_in, (B,), u8, dev, "done_in")
    tail = _buffer(tail, (B,), f32, dev, "tail")

    p = abi.cp_returns()
    p.kind, p.boundary = abi.RET_KINDS[kind], abi.RET_BOUNDARIES[boundary]
    p.flags = (abi.CP_RET_MASK_OPEN if mask_open else 0) | (abi.CP_RET_STANDARDISE if standardise else 0)
    p.gamma, p.lam = float(gamma), float(lam)
    p.steps, p.num_envs = int(K), int(B)
    p.env_id_offset, p.population, p.group = int(env_id_offset), int(population), int(group)
    lib = native.load()
    nbytes = lib.cp_returns_scratch_bytes(C.byref(p))
    if nbytes < 0:
        native.check(None, -1, "cp_returns_scratch_bytes")
    with torch.cuda.device(dev):
        adv = torch.empty((K, B), device=dev, dtype=f32)
        valid = torch.empty((K, B), device=dev, dtype=u8)
        carry = torch.empty((B,), device=dev, dtype=f32)
        ret = torch.empty((K, B), device=dev, dtype=f32) if gae else None
        stats = torch.empty((max(p.population, 1), 4), device=dev, dtype=torch.float64) if standardise else None
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else \
            getattr(stream, "cuda_stream", stream)
        scratch = _scratch_for(dev, int(st), nbytes)
        native.check(None, lib.cp_returns_compute(
            C.byref(p), _ptr(reward), _ptr(done), _ptr(values), _ptr(head), _ptr(done_in), _ptr(tail), _ptr(adv),
            _ptr(valid), _ptr(carry), _ptr(ret), _ptr(stats), _ptr(scratch), C.c_void_p(st)), "cp_returns_compute")
    return Advantages(adv, valid, carry, ret, stats)
