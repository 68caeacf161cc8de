"""Inputs and shape lists of the per-strip record tests: tests/test_gpu_block_scores.py (GPU) and
tests/test_block_score_case_inputs.py (CPU: shows that the inputs are what they claim).  No GPU here.

Every best cell the engine reports is a reduction of the per-strip records strip_best[s] = {score, i, j, valid}.  The block-score
mode (config.block_score_columns = W) sweeps the partition once more as a chain of W-column bands in which EVERY strip of
every band must report its own exact canonical cell (score desc, row asc, column asc): one run, hundreds of oracle
comparisons.  The lists below are crossed so that each height, row count, band width and pair meets each kernel ROUTE once."""
import numpy as np

F_FORCE_INT32, F_TWO_PHASE, F_WIDE = 2, 32, 65536        # include/mi355sw.h, engine.py
INF = 999999999
AT_ANYWHERE, AT_SEQUENCE_1, AT_SEQUENCE_2, AT_SEQUENCE_1_AND_2 = 0, 1, 2, 4

# ACGT first, then N, then whatever fills the alphabet (the pool of tests/test_gpu_wide_alphabet.py)
POOL = b"ACGTN" + bytes(b for b in b"RYKMSWBDHVEFIJLOPQUXZ" b"abcdefghijklmnopqrstuvwxyz" b"0123456789?")
assert len(POOL) == 63 and len(set(POOL)) == 63

# route: (letters common to both sequences, flags, packed)
ROUTES = {
    "onehot": (b"ACGT", 0, True),                        # packed kernels, one-hot scoring form (K <= 14)
    "wide15": (POOL[:15], F_WIDE, True),                 # their wide-alphabet twins at the first K that needs them ...
    "wide62": (POOL[:62], F_WIDE, True),                 # ... and at the last
    "int32flag": (b"ACGTNRYK", F_FORCE_INT32, False),    # int32 family by flag (K = 8: byte compare on the codes)
    "int32alpha": (POOL[:15], 0, False),                 # int32 family by alphabet: 15 letters, no wide flag
    "profile7": (b"ACGTNRY", F_FORCE_INT32, False),      # the 7-letter profile route of the int32 family (tests/int32_cases.py, "profile")
}
ROW_KINDS = ("below", "exact", "plus1", "km1", "ragged_lo", "ragged_hi")
WIDTH_KINDS = ("63", "64", "65", "127", "one_band", "last1", "wide")
PAIR_KINDS = ("ones", "periodic", "two", "four", "alphabet")
TIE_PAIRS = ("ones", "periodic", "two", "four")
MAX_CELLS, MAX_BANDS = 5000 * 5000, 80


def letters(route):
    return np.frombuffer(ROUTES[route][0], dtype=np.uint8)


def kernel_name(route, R, sw):
    """mi355sw_stats.kernel of the main pass (runtime.cpp): tracked, unpruned"""
    b = "true" if sw else "false"
    if route == "onehot":
        return "sw_strip_kernel_pk16<%d,true,%s,false>" % (R // 2, b)
    if route.startswith("wide"):
        return "sw_strip_kernel_pk16_wide<%d,true,%s,false>" % (R // 2, b)
    return "sw_strip_kernel<%d,%s,%s,true>" % (R, b, "true" if route == "profile7" else "false")


def rerun_kernel_name(route, R, sw):
    """... and of its rerun after an overflow report: the int32 family on the coded sequences (the profile kernel for up to 7
    letters, else byte compare), at the packed height where the family has it (4, 8, 16) and at 512 / 1024 rows for 12 / 24, 32
    -- the main pass only: the block GRID keeps the packed height"""
    R32 = R if R in (4, 8, 16) else (16 if R > 16 else 8)
    return "sw_strip_kernel<%d,%s,%s,true>" % (R32, "true" if sw else "false", "true" if len(ROUTES[route][0]) <= 7 else "false")


def rows_of(kind, R):
    """the row counts of the issue's list for strips of SH = 64 R rows.  A lane of the packed kernels holds R consecutive rows,
    the first R / 2 in the LO halves of its registers and the others in the HI halves (sw_kernel_pk16.inc: lrow_lo, lrow_hi)."""
    SH = 64 * R
    return {"below": SH - 37, "exact": SH, "plus1": SH + 1, "km1": (3 if R == 4 else 2) * SH - 1,
            "ragged_lo": SH + 37 * R + max(R // 2 - 2, 0) + 1,      # last row: lane 37, LO row R/2 - 2 (R = 4: row 0)
            "ragged_hi": SH + 21 * R + R // 2 + 1}[kind]            # last row: lane 21, the first HI row


def last_row_place(R, m):
    """(ragged, lane, half, rows of that half in use) of the last row of an m-row partition under 64 R-row strips"""
    last = (m - 1) % (64 * R)
    q = last % R
    return m % (64 * R) != 0, last // R, ("LO" if q < R // 2 else "HI"), (q if q < R // 2 else q - R // 2) + 1


def width_of(kind, t):
    """(n, W) of a band-width kind; t varies the column count from case to case"""
    if kind in ("63", "64", "65", "127"):
        W = int(kind)
        return (9 + (t % 3)) * W + 17 + 5 * t, W                   # 9 to 12 bands, a ragged last one
    if kind == "one_band":
        return 700 + 31 * t, 900 + 31 * t                          # W >= n
    if kind == "last1":
        W = 301 + 16 * t
        return 3 * W + 1, W                                        # n mod W = 1: the last band is one column wide
    if kind == "wide":
        return 2117 + 450 + 13 * t, 2117                           # wider than 2048, no multiple of 64
    raise ValueError(kind)


PERIOD, BREAK = 53, 30       # the periodic pair: |P|, and a breaker no gap bridges for less than a copy of P brings (5 + 2 * 29 > 53)


def make_pair(kind, alpha, m, n, seed):
    """the pairs where ties decide (TIE_PAIRS), and "alphabet": a related pair over all of the route's letters.  The tie pairs
    use the first letters of the alphabet and are the same pair, letter for letter renamed, on every route."""
    rng = np.random.default_rng([seed, m, n])
    rep = lambda unit, length: np.resize(np.asarray(unit, dtype=np.uint8), length)
    if kind == "ones":                                             # H(i, j) = min(i, j): every block's best tied along a row or column
        s0, s1 = rep([alpha[0]], m), rep([alpha[0]], n)
    elif kind == "periodic":
        # P^k against copies of P kept apart: every copy of P in seq1 scores |P| against every copy in seq0 -- the best of a
        # block stands at every 53rd row of the copy's last column, and a band wider than a copy and a breaker holds two such columns
        P = alpha[rng.integers(0, 3, PERIOD)]
        x = rep([alpha[3]], BREAK)                                 # a letter P does not hold
        s0, s1 = rep(P, m), rep(np.concatenate([P, x]), n)
    elif kind == "two":
        s0, s1 = alpha[rng.integers(0, 2, m)], alpha[rng.integers(0, 2, n)]
    elif kind == "four":
        s0, s1 = alpha[rng.integers(0, 4, m)], alpha[rng.integers(0, 4, n)]
    elif kind == "alphabet":
        s0 = rng.choice(alpha, size=m)
        s1 = np.resize(s0, n).copy()
        hit = rng.random(n) < 0.08
        s1[hit] = rng.choice(alpha, size=int(hit.sum()))
        if n > 200:
            s1 = np.concatenate([s1[:n // 2], rng.choice(alpha, size=17), s1[n // 2:n - 17]])
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(s0, dtype=np.uint8), np.ascontiguousarray(s1, dtype=np.uint8)


LO_HI_LANE, LO_HI_COL = 5, 150


def lo_hi_place(R):
    """(r, r', j, T) of the planted tie, 0-based rows of the partition: in lane 5 of strip 1 the LO rows hold a word X of
    T = R / 2 letters and the HI rows the word y X[:-1]; seq1 holds y X ending in column j.  So H = T at (r, j), the last LO row,
    and at (r', j - 1), the last HI row -- the two cells a lane of the packed kernels looks at in the SAME step (its HI half
    runs one column behind), where LO must win: the smaller row."""
    T = R // 2
    a = 64 * R + LO_HI_LANE * R
    return a + T - 1, a + 2 * T - 1, LO_HI_COL, T


def lo_hi_pair(alpha, R, m, n, seed):
    """backgrounds that match nothing (seq0 all alpha[2], seq1 all alpha[1]) and the two planted words over alpha[0] / alpha[3]"""
    rng = np.random.default_rng([seed, R])
    r, r2, j, T = lo_hi_place(R)
    s0, s1 = np.full(m, alpha[2], dtype=np.uint8), np.full(n, alpha[1], dtype=np.uint8)
    while True:                                                    # (drawn again while the word fits itself somewhere else as well)
        word = np.array([alpha[0], alpha[3]], dtype=np.uint8)[rng.integers(0, 2, T + 1)]     # y X
        s0[r - T + 1:r + 1] = word[1:]
        s0[r2 - T + 1:r2 + 1] = word[:-1]
        s1[j - T:j + 1] = word
        H = local_matrix(s0[r - T + 1:r2 + 1], s1[j - T:j + 1])    # nothing outside these rows and columns matches anything
        if H.max() == T and np.count_nonzero(H == T) == 2:
            return s0, s1


class Case:
    """one block-score run.  R: config.rows_per_lane (0: the engine picks); box: the partition inside the sequences;
    start / end: the manager's alignment edges; fault: config.fault_overflow_strip_plus1"""

    def __init__(self, name, route, R, m, n, W, pair, start=AT_ANYWHERE, end=AT_ANYWHERE, fault=0, origin=(0, 0), seed=0,
                 row_kind=None, width_kind=None):
        self.name, self.route, self.R, self.m, self.n, self.W, self.pair = name, route, R, m, n, W, pair
        self.start, self.end, self.fault, self.origin, self.seed = start, end, fault, origin, seed
        self.row_kind, self.width_kind = row_kind, width_kind

    def __repr__(self):
        return self.name

    @property
    def flags(self):
        return ROUTES[self.route][1]

    @property
    def sw(self):
        return self.start == AT_ANYWHERE

    @property
    def box(self):
        return self.origin[0], self.origin[1], self.origin[0] + self.m, self.origin[1] + self.n

    def bands(self):
        return -(-self.n // self.W)

    def sequences(self):
        """the whole sequences: `origin` letters of their own in front of the pair, the route's alphabet behind it -- the number
        of common byte values, which decides the kernel, is the route's K whatever the pair holds"""
        alpha = letters(self.route)
        i0, j0 = self.origin
        if self.pair == "seqgen":                                  # ACGT, the generator of the existing cases
            import __graft_entry__ as graft
            a, b = graft.load_package().seqgen.unrelated_pair(i0 + self.m, j0 + self.n, cfg=self.seed)
        elif self.pair == "related4":
            import __graft_entry__ as graft
            a, b = graft.load_package().seqgen.related_pair(i0 + self.m, j0 + self.n, cfg=self.seed)
        elif self.pair == "lo_hi":
            a, b = lo_hi_pair(alpha, self.R, self.m, self.n, self.seed)
        else:
            a, b = make_pair(self.pair, alpha, i0 + self.m, j0 + self.n, self.seed)
        return np.concatenate([a, alpha]).astype(np.uint8), np.concatenate([b, alpha]).astype(np.uint8)

    def slices(self):
        s0, s1 = self.sequences()
        i0, j0, i1, j1 = self.box
        return s0[i0:i1], s1[j0:j1]

    def oracle_kwargs(self, oracle):
        """recurrence and borders of the oracle run that matches Stage1Manager(alignment_start=start)"""
        gaps_row = self.start in (AT_SEQUENCE_2, AT_SEQUENCE_1_AND_2)      # manager.py: Stage1Manager.__init__
        gaps_col = self.start in (AT_SEQUENCE_1, AT_SEQUENCE_1_AND_2)
        return dict(recurrence=oracle.SMITH_WATERMAN if self.sw else oracle.NEEDLEMAN_WUNSCH,
                    first_row_type=oracle.INIT_WITH_GAPS if gaps_row else oracle.INIT_WITH_ZEROES,
                    first_col_type=oracle.INIT_WITH_GAPS if gaps_col else oracle.INIT_WITH_ZEROES)

    def reference(self, oracle, strip_rows=None):
        """the oracle on the partition's letters: blocks of (strip height) x W, best cell, last row"""
        s0, s1 = self.slices()
        return oracle.stage1(s0, s1, block_h=strip_rows or 64 * self.R, block_w=self.W, want_last_row=True, **self.oracle_kwargs(oracle))


def grid_cases():
    """section 1: per route one case per band width; heights, row counts and pairs cycle beside them at strides of their own, so
    that every value of every list meets every route (tests/test_block_score_case_inputs.py counts them)"""
    out = []
    for ri, route in enumerate(ROUTES):
        heights = (4, 8, 16, 0) + ((12, 24, 32) if ROUTES[route][2] else (8, 16, 4))      # (one engine's pick per route)
        rk = ri                                                     # row kinds: a counter of their own, R = 0 has none
        for t, wk in enumerate(WIDTH_KINDS):
            R = heights[(t + ri) % len(heights)]
            pair = PAIR_KINDS[(t + 2 * ri) % len(PAIR_KINDS)]
            n, W = width_of(wk, t + ri)
            if R == 0:
                kind, m = None, 2500 + 101 * ri                     # the engine's pick: 256-, 512- or 1024-row strips
            else:
                kind = ROW_KINDS[rk % len(ROW_KINDS)]
                rk += 1
                m = rows_of(kind, R)
            out.append(Case("%s-R%d-%s-W%s-%s" % (route, R, kind or "any", wk, pair), route, R, m, n, W, pair, seed=1 + 10 * ri + t,
                            row_kind=kind, width_kind=wk))
    return out


# Global recurrence with gap borders on an unrelated pair: every block's best is negative and finite, none may come back as
# "no score".  2000 x 1900, 256-row strips, W = 65: 8 x 30 blocks.
NEGATIVE = Case("negative-onehot-R4", "onehot", 4, 2000, 1900, 65, "seqgen", start=AT_SEQUENCE_1_AND_2, seed=53)

# One border of zeroes and one of gap penalties: the custom_col branch of the block pass with either border
ONE_SIDED = [
    Case("start1-onehot-R8", "onehot", 8, 1500, 1400, 200, "related4", start=AT_SEQUENCE_1, seed=52),
    Case("start2-wide15-R4", "wide15", 4, 900, 1100, 127, "alphabet", start=AT_SEQUENCE_2, seed=53),
    Case("start2-onehot-R16", "onehot", 16, 2100, 1400, 333, "four", start=AT_SEQUENCE_2, seed=54),
    Case("start1-int32flag-R4", "int32flag", 4, 700, 800, 65, "alphabet", start=AT_SEQUENCE_1, seed=55),
]

# A partition inside longer sequences: i0 and j0 no multiples of 64 (seq0 is read from an odd offset, the codes of seq1 from an
# unaligned one), the oracle runs on the slices
SLICED = [
    Case("sliced-onehot-R4-local", "onehot", 4, 1500, 1300, 300, "four", origin=(137, 211), seed=56),
    Case("sliced-onehot-R12-global", "onehot", 12, 1700, 900, 127, "related4", start=AT_SEQUENCE_1_AND_2, origin=(1001, 77), seed=57),
    Case("sliced-wide62-R8-local", "wide62", 8, 1100, 1000, 64, "alphabet", origin=(63, 129), seed=58),
    Case("sliced-profile7-R4-local", "profile7", 4, 600, 700, 65, "two", origin=(5, 321), seed=59),
]

# Injected overflow report at strip 1 (m > strip height): the main pass and every band restart on the int32 family.  Height 12:
# the int32 family has no 768-row strips -- the band is rerun at 256 rows and three records merged into each block's
OVERFLOW = [
    Case("overflow-%s-R%d-%s" % (route, R, kind), route, R, rows_of(kind, R), n, W, pair, fault=2, seed=60 + k, start=start)
    for k, (route, R, kind, n, W, pair, start) in enumerate([
        ("onehot", 4, "ragged_hi", 900, 127, "four", AT_ANYWHERE),
        ("onehot", 8, "plus1", 700, 300, "alphabet", AT_ANYWHERE),
        ("onehot", 16, "km1", 600, 65, "periodic", AT_ANYWHERE),
        ("wide15", 4, "km1", 800, 64, "alphabet", AT_ANYWHERE),
        ("wide62", 8, "ragged_lo", 900, 127, "alphabet", AT_SEQUENCE_1_AND_2),
        ("wide15", 16, "plus1", 500, 63, "two", AT_ANYWHERE),
        ("onehot", 12, "ragged_hi", 900, 127, "four", AT_ANYWHERE),
        ("onehot", 12, "km1", 700, 200, "alphabet", AT_SEQUENCE_1_AND_2),
        ("onehot", 24, "plus1", 500, 127, "two", AT_ANYWHERE),
        ("wide15", 32, "ragged_lo", 400, 150, "four", AT_ANYWHERE),
    ])
]


# A tie between the two halves of one lane in one step (lo_hi_place): every packed height on the one-hot route, two on the wide one.
# Two full strips, two bands; the tie stands in strip 1 of band 0.
LO_HI = [Case("lo_hi-%s-R%d" % (route, R), route, R, 2 * 64 * R, 300, 200, "lo_hi", seed=80 + k)
         for k, (route, R) in enumerate([("onehot", 4), ("onehot", 8), ("onehot", 12), ("onehot", 16), ("onehot", 24), ("onehot", 32),
                                         ("wide15", 8), ("wide62", 24)])]


def all_block_cases():
    return grid_cases() + [NEGATIVE] + ONE_SIDED + SLICED + LO_HI + OVERFLOW


# ---------------------------------------------------------------------------------------------------------------------
# canonical cells from a dense matrix (numpy): what the CPU file counts ties with and the strip-score tests read H from
# ---------------------------------------------------------------------------------------------------------------------
def local_matrix(s0, s1, match=1, mismatch=-3, gap_first=5, gap_ext=2):
    """H of the local recurrence with affine gaps (score parameters of include/mi355sw.h), (m + 1) x (n + 1) int32, row by row:
    E along the row is a running maximum, which numpy does as a prefix scan of H[j] + gap_ext * j"""
    m, n = len(s0), len(s1)
    H = np.zeros((m + 1, n + 1), dtype=np.int32)
    F = np.full(n + 1, -INF, dtype=np.int64)
    j = np.arange(n + 1, dtype=np.int64)
    for i in range(1, m + 1):
        F = np.maximum(F - gap_ext, H[i - 1].astype(np.int64) - gap_first)
        diag = H[i - 1, :-1] + np.where(s1 == s0[i - 1], match, mismatch)
        base = np.maximum(0, np.maximum(diag, F[1:]))               # H without the horizontal gap
        # E[j] = max_{k < j} (H[k] - gap_first - gap_ext (j - k - 1)); H[j] = max(base[j], E[j]).  A gap never follows a gap-made
        # cell more cheaply than from that gap's own source, so the scan may run on `base` alone.
        src = np.concatenate([[0], base]).astype(np.int64) + gap_ext * j
        run = np.maximum.accumulate(src)
        E = run[:-1] - gap_first + gap_ext - gap_ext * j[1:]
        H[i, 1:] = np.maximum(base, E)
    return H


def canonical_cell(H, r0, r1, c0, c1):
    """(i, j, score) of the block H[r0:r1, c0:c1] (1-based DP rows / columns), score desc, row asc, column asc; and how many cells
    hold that score"""
    blk = H[r0:r1, c0:c1]
    best = int(blk.max())
    ii, jj = np.nonzero(blk == best)
    return (r0 + int(ii[0]), c0 + int(jj[0]), best), len(ii)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: mi355sw_stream_strip_scores
# ---------------------------------------------------------------------------------------------------------------------
# (route, rows_per_lane, waves, recurrence is local); n < 16384 and no initial_bound: no seed pass writes the running best first
STRIP_M, STRIP_N = 2000, 2000
STRIP_RUNS = [
    ("onehot", 4, 0, True), ("onehot", 4, 3, True), ("onehot", 8, 2, False), ("wide15", 4, 5, True), ("wide62", 8, 0, False),
    ("int32flag", 4, 0, True), ("int32alpha", 8, 3, False), ("profile7", 4, 2, True),
]
SERIAL_M, SERIAL_N, SERIAL_CFG = 4000, 3000, 51          # waves = 1: sixteen 256-row strips of the four-letter unrelated pair


def strip_pair(route, sw):
    """2000 x 2000 in the route's alphabet, the alphabet behind it: unrelated four-letter for local runs (low scores, ties in
    every strip), related for global ones"""
    alpha = letters(route)
    a, b = make_pair("four" if sw else "alphabet", alpha, STRIP_M, STRIP_N, 72)
    return np.concatenate([a, alpha]).astype(np.uint8), np.concatenate([b, alpha]).astype(np.uint8)


def strip_bests(oracle, s0, s1, SH, sw=True):
    """[(i, j, score)] 0-based, the canonical best cell of every SH-row strip: the oracle's grid with one band"""
    kw = {} if sw else dict(recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=oracle.INIT_WITH_GAPS, first_col_type=oracle.INIT_WITH_GAPS)
    ref = oracle.stage1(s0, s1, block_h=SH, block_w=len(s1) + 1, **kw)
    gh, gw = ref["grid"]
    assert gw == 1
    return [ref["block_scores"][(0, by)] for by in range(gh)], ref


def prefix_maxima(scores):
    """strips whose best is at least the best of all strips above them: (strict, tied) index lists"""
    strict, tied, run = [], [], None
    for s, v in enumerate(scores):
        if run is None or v > run:
            strict.append(s)
            run = v
        elif v == run:
            tied.append(s)
    return strict, tied
