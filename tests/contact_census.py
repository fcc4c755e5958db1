"""Census of the contacts a state SoA ended its last substep with, decoded from the warm-start feature ids.

CP_SF_WS_ID(island, j) holds four id bytes per local pair, 0xFF for an empty slot.  An id is
32 * kind + feature: kind 0-2 a face of A (its axis), 3-5 a face of B, 6 an edge pair (feature 3 i + j);
for the face kinds the feature is 0-3 for class C1 (incident vertices inside the reference face), 4-7 for
C2 (reference corners inside the incident face), 8-23 for C3 (edge crossings).  The GPU's state is
bit-equal to the oracle's, so the census is taken on the oracle's state and never looks at device code:
it states which paths a scenario reached, as the precondition of the directed GPU tests.
"""
from collections import Counter

import numpy as np

from cartpoleplusplus_amd import abi

AXES = "xyz"


def branch_kind(i):
    """Name of one id byte: 'A.x/C1', 'B.z/C3', 'edge.xy' (A's axis, B's axis)."""
    kind, feat = int(i) // 32, int(i) % 32
    if kind < 3:
        side, axis = "A", AXES[kind]
    elif kind < 6:
        side, axis = "B", AXES[kind - 3]
    elif kind == 6 and feat < 9:
        return f"edge.{AXES[feat // 3]}{AXES[feat % 3]}"
    else:
        raise ValueError(f"feature id {int(i)} is none the narrowphase writes")
    if feat >= 24:
        raise ValueError(f"feature id {int(i)}: face feature {feat}")
    return f"{side}.{axis}/C{1 if feat < 4 else 2 if feat < 8 else 3}"


def pair_ids(state):
    """(CP_NUM_PAIRS, B, 4) uint8: the id bytes of every global pair (0xFF: empty)."""
    words = abi.state_ints(np.asarray(state))
    B = words.shape[-1]
    out = np.full((abi.CP_NUM_PAIRS, B, 4), 0xFF, np.uint8)
    for p in range(abi.CP_NUM_ISLANDS):
        for j in range(abi.CP_ISLAND_PAIRS):
            w = np.ascontiguousarray(words[abi.CP_SF_WS_ID(p, j)]).astype(np.int32).view(np.uint32)
            for k in range(4):
                out[abi.ISLAND_PAIR[p][j], :, k] = (w >> np.uint32(8 * k)) & np.uint32(0xFF)
    return out


def point_counts(state):
    """(CP_NUM_PAIRS, B) contact points per global pair at the end of the last substep."""
    return (pair_ids(state) != 0xFF).sum(-1)


class Census:
    """Accumulates step-end states: per global pair a Counter of branch kinds and one of point counts,
    and the envs in which the pair had a contact at some step end."""

    def __init__(self, B):
        self.kinds = [Counter() for _ in range(abi.CP_NUM_PAIRS)]
        self.points = [Counter() for _ in range(abi.CP_NUM_PAIRS)]
        self.touched = np.zeros((abi.CP_NUM_PAIRS, B), bool)

    def add(self, state):
        ids = pair_ids(state)
        cnt = (ids != 0xFF).sum(-1)
        self.touched |= cnt > 0
        for g in range(abi.CP_NUM_PAIRS):
            vals, n = np.unique(ids[g][ids[g] != 0xFF], return_counts=True)
            for v, c in zip(vals, n):
                self.kinds[g][branch_kind(v)] += int(c)
            vals, n = np.unique(cnt[g], return_counts=True)
            for v, c in zip(vals, n):
                self.points[g][int(v)] += int(c)
        return self

    def envs(self, pair):
        """Number of envs in which `pair` had a contact at some counted step end."""
        return int(self.touched[pair].sum())

    def sides(self, pair):
        """The set of 'A', 'B', 'edge' seen on `pair`."""
        return {k.split(".")[0] for k in self.kinds[pair]}
