"""Shared by tests/test_int32_edge_goal_host.py and tests/test_gpu_int32_edge_goal.py: the edge rule (mi355sw_set_prune_end) and
goal bounds (mi355sw_set_goal_bounds) on the int32 kernel family (MI355SW_F_INT32_PRUNE_EDGE_GOAL, opt-in).  No GPU here.

The pairs and shapes at which a skipped-cell count is asserted, and a CPU CENSUS per shape, rule and strip height: how many
slabs a slab rule may skip WHOLE.  A slab is what csrc/sw_kernel.hip tests at once -- the 64 R rows of a whole strip by 64
columns from column 128 on, the last of them a full chunk -- widened to its bounding box by the 63 columns of systolic skew
(lane k sits k columns behind lane 0) and by the bus row above.  It may go when every H in the box has

    edge rule   H + reach(mode, rows left, columns left) + 16 < optimum       (edge_prune_cases.reach; 16: NW32_PRUNE_MARGIN)
    goal rule   H + columns left + 16 < B

with H from a plain numpy Gotoh matrix (H >= E, F cell by cell, so H decides).  The kernel's own bounds are weaker -- a lane
spans R rows, and skipped slabs turn the cells next to them into lower bounds only after the fact --, so this count is the
CEILING of what a run skips, not the expectation.  pruned_cells > 0 is demanded only at shapes where the ceiling is at
least a tenth of the eligible slabs (WORTH): a condition on the input, not a measurement of the engine."""
import numpy as np

import edge_prune_cases as ec

CFG = 71                                   # seqgen.related_pair(m, n, cfg=CFG): the pair of tests/test_gpu_goal_prune.py
GOAL_SLACK = 200                           # B = max H of the last column - 200
MARGIN = 16                                # csrc/sw_kernel.hip, NW32_PRUNE_MARGIN
CHUNK = 64
HEIGHTS = (4, 8, 16)                       # rows per lane: strips of 256, 512, 1024 rows
RULES = ("goal", 1, 2, 3)                  # goal bounds; edge modes last row, last column, either
SHAPES = ((2048, 1536), (4096, 3072))      # wide enough for every height
WORTH = 0.1
_H = {}


ROUTES = ("iupac", "forced", "wide63")     # the ways into the int32 family (tests/test_gpu_int32_prune_global.py::_route)
F_FORCE_INT32, F_WIDE = 2, 65536


def pair(pkg, m, n, route="forced"):
    """(seq0, seq1, engine flags) of one way into the int32 family: 15 IUPAC letters, MI355SW_F_FORCE_INT32 on an ACGT pair,
    63 letters under MI355SW_F_WIDE_ALPHABET"""
    if route == "forced":
        return pkg.seqgen.related_pair(m, n, cfg=CFG) + (F_FORCE_INT32,)
    from test_gpu_wide_alphabet import IUPAC, POOL, common_letters, wide_pair
    letters, flags = {"iupac": (IUPAC, 0), "wide63": (POOL, F_WIDE)}[route]
    s0, s1 = wide_pair(pkg, m, n, letters, cfg=CFG, ensure=True)       # (ensure: every letter in both sequences, at any size)
    assert common_letters(s0, s1) == len(letters)
    return s0, s1, flags


def gotoh_h(s0, s1):
    """H of the whole matrix with gap-initialised borders, (m + 1) x (n + 1) int32, swept by anti-diagonals"""
    s0, s1 = np.asarray(s0), np.asarray(s1)
    m, n = len(s0), len(s1)
    NEG = -(1 << 28)
    H = np.zeros((m + 1, n + 1), dtype=np.int32)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int32)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int32)
    H[0, 1:] = -ec.GAP_OPEN - ec.GAP_EXT * np.arange(1, n + 1)
    H[1:, 0] = -ec.GAP_OPEN - ec.GAP_EXT * np.arange(1, m + 1)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        sc = np.where(s0[i - 1] == s1[j - 1], ec.MATCH, ec.MISMATCH).astype(np.int32)
        e = np.maximum(E[i, j - 1] - ec.GAP_EXT, H[i, j - 1] - ec.GAP_FIRST)
        f = np.maximum(F[i - 1, j] - ec.GAP_EXT, H[i - 1, j] - ec.GAP_FIRST)
        E[i, j], F[i, j] = e, f
        H[i, j] = np.maximum(H[i - 1, j - 1] + sc, np.maximum(e, f))
    return H


def matrix(pkg, m, n, route="forced"):
    """the pair's H, computed once per shape and route and left unchanged"""
    if (m, n, route) not in _H:
        h = gotoh_h(*pair(pkg, m, n, route)[:2])
        h.setflags(write=False)
        _H[(m, n, route)] = h
    return _H[(m, n, route)]


def bound_of(H, rule):
    """what the rule holds a value against: the goal bound B, or the optimum of the named edge(s)"""
    if rule == "goal":
        return int(H[:, -1].max()) - GOAL_SLACK
    return ec.edge_optimum(rule, H[-1, :, None], H[:, -1, None])


def census(H, rule, R):
    """(slabs that may be skipped whole, eligible slabs) at 64 R-row strips"""
    m, n = H.shape[0] - 1, H.shape[1] - 1
    di, dj = (m - np.arange(m + 1))[:, None], (n - np.arange(n + 1))[None, :]
    gain = np.broadcast_to(dj, H.shape) if rule == "goal" else ec.reach(rule, di, dj)
    live = H.astype(np.int64) + gain + MARGIN >= bound_of(H, rule)
    SH = CHUNK * R
    skippable = eligible = 0
    for s in range(m // SH):
        for col0 in range(2 * CHUNK, n - CHUNK + 1, CHUNK):
            eligible += 1
            # 1-based DP coordinates: rows s SH .. (s + 1) SH (the bus row above first), columns col0 - 63 + 1 .. col0 + 64
            if not live[s * SH:(s + 1) * SH + 1, col0 - 62:col0 + CHUNK + 1].any():
                skippable += 1
    return skippable, eligible


def worth(H, rule, R):
    k, e = census(H, rule, R)
    return e > 0 and k >= WORTH * e


def worth_asserting(pkg, m, n, rule, R, route="forced"):
    """the condition under which pruned_cells > 0 is demanded of a run"""
    return worth(matrix(pkg, m, n, route), rule, R)
