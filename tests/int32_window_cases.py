"""Shared by tests/test_int32_window_host.py and tests/test_gpu_int32_window.py: the pruning window of the int32 kernel family
(MI355SW_F_INT32_WINDOW, opt-in; csrc/sw_kernel.hip, WINDOW).  No GPU here: the pairs, the shapes and a CPU census.

The retire pair is tests/test_gpu_window.py::test_strips_below_the_end_of_the_alignment_retire's construction at a twelfth of
the size: seq1 is a mutated copy of the head of seq0 followed by 512 unrelated bases, so the local alignment runs down the
diagonal from the corner and ends 512 columns short of the last one, after less than a sixth of the rows.  Every strip below
it holds noise.

CENSUS of the retire pair (what the local rule may skip in the strips below the alignment, 256-row strips).  Eligible slabs
are what csrc/sw_kernel.hip tests without the window: whole strips x full chunks from column 128 on, n / 64 - 2 per strip.  A
slab of a strip whose first row lies below the best cell may go when everything that enters it from ABOVE -- the oracle's row
at the strip's upper boundary, DP columns col0 - 63 .. col0 + 64, the 63 columns of systolic skew included -- has

    H + min(m + 1 - row0, n + 64 - col0) + 8 < best            (the kernel's `left`; 8: SW32_PRUNE_MARGIN)

What enters from the left is inside the strip and not known from boundary rows, so this is the CEILING of what a run skips
there, and it counts no slab of the strips the alignment crosses.  pruned_cells >= half the matrix is demanded of the GPU run
only because the ceiling leaves room above it: a condition on the input, not a measurement of the engine."""
import numpy as np

CHUNK = 64
MARGIN = 8                                  # csrc/sw_kernel.hip, SW32_PRUNE_MARGIN
INF = 999999999
F_FORCE_INT32, F_NO_WINDOW, F_DET, F_WIDE = 2, 1024, 16384, 65536
IUPAC = np.frombuffer(b"ACGTNRYKMSWBDHV", dtype=np.uint8)

# ---- 1. retire, local ----------------------------------------------------------------------------------------------------------
RETIRE_M, RETIRE_N = 49152, 8192
RETIRE_TAIL = 512
RETIRE_BEST = (7682, 7680, 6959)            # the oracle's canonical best cell over the whole matrix (1-based)
RETIRE_QUIET_FROM = 12288                   # no special row below this row holds an H above RETIRE_QUIET_H
RETIRE_QUIET_H = 8
RETIRE_ROWS_FROM = 16384                    # the special rows at or below this row, and the last row, must read as the constant at their end
RETIRE_SH = 256
RETIRE_HALF = 0.5                           # pruned_cells >= RETIRE_HALF * m * n with the window


def retire_pair(pkg, route="forced"):
    """(seq0, seq1, engine flags): the ACGT pair under MI355SW_F_FORCE_INT32, or the same pair with every 50th base of both
    sequences an ambiguity code (15 letters in common: the int32 family by the alphabet)"""
    sg = pkg.seqgen
    m, n = RETIRE_M, RETIRE_N
    s0 = sg.random_dna(sg.SEED0 + 720, m)
    s1 = np.ascontiguousarray(np.concatenate([sg.mutate_dna(s0[:n + n // 8 + 64], sg.SEED1 + 720, inversion=0.0)[:n - RETIRE_TAIL],
                                              sg.random_dna(77, RETIRE_TAIL)]))
    assert len(s1) == n
    if route == "forced":
        return s0, s1, F_FORCE_INT32
    s0, s1 = iupac_codes(s0, s1, 720)
    return s0, s1, 0


def iupac_codes(s0, s1, seed):
    """tests/test_gpu_prune32.py::_iupac_pair's substitution on a given pair; every one of the 15 letters ends up in both"""
    s0, s1 = s0.copy(), s1.copy()
    rng = np.random.default_rng(seed)
    for s in (s0, s1):
        pos = np.arange(7, len(s), 50)
        s[pos] = IUPAC[4 + rng.integers(0, 11, size=len(pos))]
    assert len(np.intersect1d(s0, s1)) == 15
    return s0, s1


def retire_census(boundary_rows, best, m, n, SH=RETIRE_SH):
    """(strips below the alignment, strips, slabs of those strips that may go, eligible slabs of all strips).
    boundary_rows: {dp row: (n + 1, 2) cells of the unpruned oracle} with every multiple of SH below m"""
    strips = m // SH
    per_strip = n // CHUNK - 2
    below = skippable = 0
    for s in range(strips):
        row0 = s * SH
        if row0 < best[0]:                  # the strip above this boundary holds the best cell or lies above it
            continue
        below += 1
        h = boundary_rows[row0][:, 0].astype(np.int64)
        for col0 in range(2 * CHUNK, n - CHUNK + 1, CHUNK):
            left = min(m + 1 - row0, n + CHUNK - col0)
            if int(h[col0 - 63:col0 + CHUNK + 1].max()) + left + MARGIN < best[2]:
                skippable += 1
    return below, strips, skippable, strips * per_strip


# ---- 2. every rule against the oracle and against the walk -----------------------------------------------------------------------
M2, N2 = 24000, 20000
HEIGHTS = (4, 8, 16)
LOCAL_KINDS = ("corner", "middle", "tail")
RULES = LOCAL_KINDS + ("last_cell", 1, 2, 3, "goal")
GOAL_SLACK = 200
CLOSE = 0.05                                # the three runs' pruned_cells lie within CLOSE * m * n of each other


def local_pair(pkg, kind, m=M2, n=N2):
    """corner: related from the corner; middle / tail: tests/test_gpu_window.py::_pair kinds 1 and 3 at this shape -- seq1 a piece
    from the middle of seq0, and a short homology followed by a long unrelated tail"""
    sg = pkg.seqgen
    if kind == "corner":
        return sg.related_pair(m, n, cfg=812)
    if kind == "middle":
        s0 = sg.random_dna(sg.SEED0 + 701, m)
        i0 = m // 4
        s1 = sg.mutate_dna(s0[i0:i0 + n + n // 8 + 64], sg.SEED1 + 701, inversion=0.0)
        return s0, np.ascontiguousarray(np.concatenate([s1, sg.random_dna(6, max(0, n - len(s1)))])[:n])
    assert kind == "tail"
    s0 = sg.random_dna(sg.SEED0 + 703, m)
    L = min(m, n) // 3
    return s0, np.ascontiguousarray(np.concatenate([sg.mutate_dna(s0[:L + L // 8 + 64], sg.SEED1 + 703, inversion=0.0)[:L], sg.random_dna(12, n - L)]))


# ---- 3. runs of skipped slabs ----------------------------------------------------------------------------------------------------
M3 = N3 = 16384

# ---- 4. ragged and narrow edges --------------------------------------------------------------------------------------------------
EDGE_ROWS = tuple(4096 + d for d in (1, 255, 256, 257))
EDGE_COLS = tuple(3072 + d for d in (0, 1, 63, 64, 65))


def kernel_name(R, rule, profile):
    """mi355sw_stats.kernel of the windowed instantiation: all eight template arguments"""
    p = "true" if profile else "false"
    if rule in LOCAL_KINDS or rule == "local":
        return "sw_strip_kernel<%d,true,%s,true,true,false,false,true>" % (R, p)
    tail = {"last_cell": "false,false", "goal": "true,false"}.get(rule, "false,true")
    return "sw_strip_kernel<%d,false,%s,false,true,%s,true>" % (R, p, tail)


def walking_name(R, rule, profile):
    """... and of the instantiation that walks (the flag off, or MI355SW_F_NO_WINDOW)"""
    p = "true" if profile else "false"
    if rule in LOCAL_KINDS or rule == "local":
        return "sw_strip_kernel<%d,true,%s,true,true>" % (R, p)
    tail = {"last_cell": "", "goal": ",true"}.get(rule, ",false,true")
    return "sw_strip_kernel<%d,false,%s,false,true%s>" % (R, p, tail)
