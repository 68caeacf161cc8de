"""Inputs that put stage 4 (csrc/stage4.hip) on its structural edges -- shared by tests/test_stage4_edge_inputs.py (CPU: holds
the inputs to their conditions with the oracle alone) and tests/test_gpu_stage4_edges.py (GPU: engine against oracle).
A plain module: no fixtures, nothing here touches a GPU.

Every builder returns (seq0, seq1, crosspoints).  Many INDEPENDENT partitions are concatenated into one pair and one list:
seq0 = A_1 + A_2 + ..., seq1 = B_1 + B_2 + ..., crosspoint k = (0, sum |A|, sum |B|, sum of the global scores), each score
the oracle's Needleman-Wunsch score of (A_k, B_k) with gap-initialised borders -- so one stage4() call refines hundreds of
independent partitions at once, which is how the kernel is meant to be used.

What the kernel's structure makes worth placing a partition on:
  * mm_half_kernel sweeps a half-matrix 4 rows per lane, 256 rows per pass; the last row of a pass is re-read in place as the
    next pass's top row; sequence B and that row are prefetched 64 columns per chunk.  k_last, nv, the bprev / bcur hand-over
    and the in-place bus row change behaviour at rows 1..5, 255..257, 259..261, 511..513 and at columns 1, 2, 63..65, 127..129.
  * the forward half's borders depend on the start crosspoint's type SEEN IN THE SPLIT'S ORIENTATION (row_open = 0 for type 1,
    col_open = 0 for type 2, corner = -INF for both); the reverse half's corner on the end crosspoint's.
  * mm_match_kernel takes the first of 2 * (lenB / 2 + 1) candidate columns in the reference's order, 64 per ballot."""
import numpy as np

INV_TYPE = (0, 2, 1)
LADDER = (2000, 1040, 520, 260, 130, 66, 16, 4, 1)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CACHE = {}


def nw_score(oracle, a, b):
    """the global score of (a, b), as tests/test_gpu_stage4.py::_global_endpoints computes it"""
    ref = oracle.stage1(a, b, recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=oracle.INIT_WITH_GAPS,
                        first_col_type=oracle.INIT_WITH_GAPS, best_mode=oracle.BEST_LAST_CELL, want_last_row=True)
    return int(ref["last_row"][-1][0])


def concatenate(oracle, parts):
    """[(A_k, B_k), ...] -> (seq0, seq1, crosspoints): one type-0 crosspoint after every part"""
    cp = [(0, 0, 0, 0)]
    i = j = score = 0
    for a, b in parts:
        score += nw_score(oracle, a, b)
        i += len(a)
        j += len(b)
        cp.append((0, i, j, score))
    seq0 = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), dtype=np.uint8)
    seq1 = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), dtype=np.uint8)
    seq0.setflags(write=False)
    seq1.setflags(write=False)
    return seq0, seq1, cp


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------
# geometry: every row / column count at which the sweep changes behaviour
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRY_LONG = list(range(2, 12)) + list(range(510, 516)) + list(range(518, 524)) + list(range(1022, 1028))
GEOMETRY_SHORT = [1, 2, 3, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193]


def geometry_parts(seqgen):
    """related pairs of la x lb, la the split side (forward half: la / 2 rows, reverse half: la - la / 2), lb in GEOMETRY_SHORT
    or la itself; each in both orientations (the longer side in seq0, and swapped: the `inv` partitions)"""
    parts, cfg = [], 0
    for la in GEOMETRY_LONG:
        for lb in sorted(set([x for x in GEOMETRY_SHORT if x <= la] + [la])):
            for swap in (False, True):
                if swap and lb == la:
                    continue
                cfg += 1
                a, b = seqgen.related_pair(la, lb, cfg=5000 + cfg)
                parts.append((b, a) if swap else (a, b))
    return parts


def geometry(seqgen, oracle):
    return cached("geometry", lambda: concatenate(oracle, geometry_parts(seqgen)))


# ---------------------------------------------------------------------------------------------------------------------
# gapped: crosspoints of type 1 and 2 at the start and at the end of a split, in both orientations, at more than 256 rows
# ---------------------------------------------------------------------------------------------------------------------
# Seeds of gapped_pair() chosen by a search with the oracle alone (oracle/make_golden_stage4_edges.py --search-gapped) so that
# the census conditions of tests/test_stage4_edge_inputs.py hold; the conditions are what counts, the seeds are one way there.
GAPPED_SEEDS = (79, 129, 190, 210, 218, 250, 278, 290)


def gapped_pair(seed):
    """a common core of 200 to 1500 letters with one to four insertions of random length on EACH side: gaps that change a
    partition's orientation between two levels, which is what makes the oriented start type 1 (row_open = 0)"""
    rng = np.random.default_rng(seed)
    core = int(rng.integers(200, 1500))
    a = rng.choice(_ACGT, size=core)

    def with_insertions():
        pieces, p = [], 0
        for _ in range(int(rng.integers(1, 5))):
            q = int(rng.integers(p, core + 1))
            pieces += [a[p:q], rng.choice(_ACGT, size=int(rng.integers(5, max(core // 2, 6))))]
            p = q
        pieces.append(a[p:])
        return np.concatenate(pieces)

    x = with_insertions()
    y = with_insertions()
    return x, y


def gapped(oracle):
    return cached("gapped", lambda: concatenate(oracle, [gapped_pair(s) for s in GAPPED_SEEDS]))


def geometry_and_gapped(seqgen, oracle):
    return cached("geometry+gapped", lambda: concatenate(oracle, geometry_parts(seqgen) + [gapped_pair(s) for s in GAPPED_SEEDS]))


# ---------------------------------------------------------------------------------------------------------------------
# low complexity: where the order of the candidates decides
# ---------------------------------------------------------------------------------------------------------------------
LOW_COMPLEXITY_SIZES = [(700, 700), (700, 431), (431, 700), (1030, 130), (130, 1030), (520, 513)]


def repeat(unit, n):
    return np.frombuffer((unit * (n // len(unit) + 1))[:n], dtype=np.uint8).copy()


def low_complexity_parts():
    parts = []
    for m, n in LOW_COMPLEXITY_SIZES:
        parts += [(repeat(b"A", m), repeat(b"A", n)), (repeat(b"AC", m), repeat(b"AC", n)), (repeat(b"ACG", m), repeat(b"CGA", n)),
                  (repeat(b"A", m), repeat(b"C", n)), (repeat(b"AACAG", m), repeat(b"AACAGT", n))]
    x = repeat(b"ACGT", 900)
    y = x.copy()
    y[450] = ord("A")                                   # one substitution ...
    parts.append((x, np.delete(y, slice(200, 260))))    # ... and a 60-letter deletion
    return parts


def low_complexity(oracle):
    return cached("low_complexity", lambda: concatenate(oracle, low_complexity_parts()))


def low_complexity_single():
    """one low-complexity pair on its own (the live-reference comparison aligns a pair, not a list)"""
    x = np.concatenate([repeat(b"ACGT", 900), repeat(b"AACAG", 700), repeat(b"AC", 431)])
    y = np.concatenate([repeat(b"ACGT", 900), repeat(b"AACAGT", 520), repeat(b"AC", 700)])
    y[450] = ord("A")
    return np.ascontiguousarray(x), np.ascontiguousarray(np.delete(y, slice(200, 260)))


# ---------------------------------------------------------------------------------------------------------------------
# foreign bytes: letters that occur in one sequence only
# ---------------------------------------------------------------------------------------------------------------------
# ACGT first (the commonest by construction: they get the codes below 4), then what fills the alphabet
POOL = b"ACGTN" + b"RYKMSWBDHVEFIJLOPQUXZ" + b"abcdefghijklmnopqrstuvwxyz" + b"0123456789?"
GAP_AT, GAP_LEN = 1000, 40


def foreign_pair(seqgen, n_common, only0=b"@$", only1=b"#%", m=3000, cfg=0):
    """A related pair of m x (m - 40) with exactly `n_common` byte values common to both sequences, two different bytes
    (`only0`) that occur in seq0 only and two (`only1`) that occur in seq1 only.

    seq0 = seqgen.random_dna with the letters POOL[4:n_common] written in at about one position in 25; seq1 = seq0 with 2 % of
    the positions substituted and seq0[1000:1040] deleted, so seq0[i] is aligned with seq1[i] below 1000 and with seq1[i - 40]
    from 1040 on.  The foreign bytes go to ALIGNED positions (the true alignment has them as mismatches: a byte of seq0 only
    against a different byte of seq1 only, which the reference scores -3), to positions where only one side has one, and to
    both sides of the gap (seq0[999] / seq1[999] and seq0[1040] / seq1[1000])."""
    assert 4 <= n_common <= len(POOL) and len(only0) == 2 and len(only1) == 2
    assert not (set(only0) | set(only1)) & set(POOL[:n_common]) and not set(only0) & set(only1)
    rng = np.random.default_rng(9000 + 100 * n_common + cfg)
    s0 = seqgen.random_dna(seqgen.SEED0 + 9000 + n_common + cfg, m).copy()
    extras = np.frombuffer(POOL[4:n_common], dtype=np.uint8)
    if len(extras):
        at = rng.choice(np.arange(50, m - 50), size=max(m // 25, 3 * len(extras)), replace=False)
        s0[at] = extras[np.arange(len(at)) % len(extras)]
    s1_full = s0.copy()
    sub = rng.choice(np.arange(50, m - 50), size=m // 50, replace=False)
    s1_full[sub] = _ACGT[rng.integers(0, 4, len(sub))]
    # every common letter stays common: one aligned copy of each at the far end of both
    both = np.frombuffer(POOL[:n_common], dtype=np.uint8)
    s0[m - 50 + np.arange(n_common) % 50] = both
    s1_full[m - 50 + np.arange(n_common) % 50] = both
    # aligned foreign bytes, alternating the two bytes of each side; then one-sided ones
    aligned = np.concatenate([np.arange(60, GAP_AT - 60, 97), np.arange(GAP_AT + GAP_LEN + 60, m - 120, 89), [GAP_AT - 1, GAP_AT + GAP_LEN]])
    o0, o1 = np.frombuffer(only0, dtype=np.uint8), np.frombuffer(only1, dtype=np.uint8)
    s0[aligned] = o0[np.arange(len(aligned)) % 2]
    s1_full[aligned] = o1[(np.arange(len(aligned)) // 2) % 2]
    s0[np.arange(33, m - 120, 211)] = o0[0]
    s1_full[np.arange(47, GAP_AT - 60, 199)] = o1[1]
    s1 = np.delete(s1_full, slice(GAP_AT, GAP_AT + GAP_LEN))
    s0, s1 = np.ascontiguousarray(s0), np.ascontiguousarray(s1)
    common = np.intersect1d(np.unique(s0), np.unique(s1))
    assert len(common) == n_common and len(s1) == m - GAP_LEN, (len(common), n_common)
    assert np.isin(o0, s0).all() and np.isin(o1, s1).all() and not np.isin(o0, s1).any() and not np.isin(o1, s0).any()
    return s0, s1


# ---------------------------------------------------------------------------------------------------------------------
# the census: what a list makes stage 4 do
# ---------------------------------------------------------------------------------------------------------------------
def oriented(s, e):
    """(inverse, lenA, lenB, oriented start type, oriented end type) of the partition between two crosspoints, as
    split_thread orients it: the longer side is split; None for a partition with a zero side"""
    di, dj = e[1] - s[1], e[2] - s[2]
    if di == 0 or dj == 0:
        return None
    inv = di < dj
    return (inv, dj, di, INV_TYPE[s[0]], INV_TYPE[e[0]]) if inv else (inv, di, dj, s[0], e[0])


def first_step_partitions(points, limit):
    """indices k of the partitions (points[k - 1], points[k]) that stage 4 splits in its FIRST step at this limit"""
    out = []
    for k in range(1, len(points)):
        o = oriented(points[k - 1], points[k])
        if o is not None and o[1] > limit:
            out.append(k)
    return out


def first_step_halves(points, limit):
    """for every partition stage 4 would split first at that limit, its two half-matrices as
    (rows, columns, oriented type of the crosspoint at the half's corner, 'f' or 'r', inverse)"""
    out = []
    for k in first_step_partitions(points, limit):
        inv, lenA, lenB, ts, te = oriented(points[k - 1], points[k])
        out.append((lenA // 2, lenB, ts, "f", inv))
        out.append((lenA - lenA // 2, lenB, te, "r", inv))
    return out


def split_column(s, e, point):
    """(column, lenB) of `point`, the crosspoint that splits partition (s, e), in the split's orientation"""
    inv, lenA, lenB, _, _ = oriented(s, e)
    mid = (s[2] if inv else s[1]) + lenA // 2
    assert (point[2] if inv else point[1]) == mid, (s, e, point)
    return ((point[1] - s[1]) if inv else (point[2] - s[2])), lenB


def winning_candidate(s, e, point):
    """the index q of the chosen column in mm_match_kernel's order: candidate 2 k is column jmid1 + k, candidate 2 k + 1 the
    mirrored column lenB - (jmid1 + k), jmid1 = lenB - lenB / 2"""
    col, lenB = split_column(s, e, point)
    jmid1 = lenB - lenB // 2
    return 2 * (col - jmid1) if col >= jmid1 else 2 * (lenB - col - jmid1) + 1


def first_step_point(oracle, seq0, seq1, s, e):
    """the crosspoint the oracle's first step puts into partition (s, e): the partition alone, refined with a limit one below its
    split side, is split exactly once -- unless the point lands on an extreme column of a square partition, whose other half
    is then as long as the limit and split again; the first point is then the one on the middle line at that extreme column"""
    inv, lenA, lenB, _, _ = oriented(s, e)
    pts, steps = oracle.stage4(seq0, seq1, [s, e], lenA - 1)
    if steps == 1 and len(pts) == 3:
        return pts[1]
    mid = (s[2] if inv else s[1]) + lenA // 2
    ends = [(mid, s[1]), (mid, e[1])] if inv else [(mid, s[2]), (mid, e[2])]
    cand = [p for p in pts[1:-1] if ((p[2], p[1]) if inv else (p[1], p[2])) in ends]
    assert lenA == lenB and len(cand) == 1, (s, e, pts)
    return cand[0]


def ladder(oracle, seq0, seq1, crosspoints, key=None):
    """[(limit, input list, the oracle's refined list, steps), ...] down LADDER, each rung fed the oracle's list of the rung
    before; computed once per key and left unchanged"""
    def run():
        rungs, lst = [], list(crosspoints)
        for limit in LADDER:
            out, steps = oracle.stage4(seq0, seq1, lst, limit)
            rungs.append((limit, tuple(lst), tuple(out), steps))
            lst = out
        return rungs
    return cached(("ladder", key), run) if key is not None else run()


def first_difference(got, want, given, limit):
    """a short description of where two refined lists part: the first differing point and the partition of the list GIVEN to
    stage 4 it lies in -- index, lenA x lenB, oriented types, orientation -- instead of two lists of 70 000 tuples"""
    got, want = [tuple(p) for p in got], [tuple(p) for p in want]
    if got == want:
        return None
    n = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
    g = got[n] if n < len(got) else None
    w = want[n] if n < len(want) else None
    p = w or g
    where = "?"
    for k in range(1, len(given)):
        s, e = given[k - 1], given[k]
        if s[1] <= p[1] <= e[1] and s[2] <= p[2] <= e[2]:
            o = oriented(s, e)
            if o is None:
                continue
            where = "partition %d of the given list, %s -> %s: lenA x lenB = %d x %d, oriented types %d -> %d, %s" % (
                k, s, e, o[1], o[2], o[3], o[4], "inverse (seq1 is split)" if o[0] else "direct (seq0 is split)")
            break
    return "limit %d: %d points against the oracle's %d; first difference at point %d: got %s, want %s; in %s" % (
        limit, len(got), len(want), n, g, w, where)
