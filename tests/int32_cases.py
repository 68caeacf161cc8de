"""Inputs and shape lists of tests/test_gpu_int32_family.py (GPU) and tests/test_int32_case_inputs.py (CPU: shows that the
inputs are what they claim).  No GPU here.

The int32 kernel family (csrc/sw_kernel.hip: sw_strip_kernel<R, SW, PROFILE, TRACK[, PRUNE]>, R in {4, 8, 16}) runs whatever the
packed kernels cannot: pairs with 15 or more common byte values, every rerun after MI355SW_EOVERFLOW16, MI355SW_F_FORCE_INT32 and
MI355SW_F_FORCE_GENERIC_COMPARE.  Four WAYS lead into it; per way one alphabet, the flags, and what mi355sw_stats reports."""
import numpy as np

F_FORCE_GENERIC_COMPARE, F_FORCE_INT32 = 1, 2          # include/mi355sw.h, engine.py
INF = 999999999
OFFSET = 120_000_000                                     # special-row values deep in a C5-sized alignment

# way: (letters common to both sequences, flags, mi355sw_stats.profile_kernel, PROFILE template argument, seq0_shift != 0)
#   profile: K = 7 exactly -- code 7 is then the foreign code of BOTH sequences (runtime.cpp, foreign_codes), and the test of
#            n_match_codes in the profile is all that keeps two foreign bytes from matching
#   coded:   K = 8, the first alphabet past the nibble profile: byte compare on the codes (seq0 code << 2 against seq1 code * 4)
#   raw15:   K = 15, the full IUPAC set, default flags: byte compare on raw bytes
#   generic: ACGT with MI355SW_F_FORCE_GENERIC_COMPARE: byte compare on raw bytes
WAYS = {
    "profile": (b"ACGTNRY", F_FORCE_INT32, 1, True, True),
    "coded": (b"ACGTNRYK", F_FORCE_INT32, 0, False, True),
    "raw15": (b"ACGTNRYKMSWBDHV", 0, 0, False, False),
    "generic": (b"ACGT", F_FORCE_GENERIC_COMPARE, 0, False, False),
}
FOREIGN0, FOREIGN1 = b"@$", b"#%"                        # byte values of seq0 only / of seq1 only
HEIGHTS = (4, 8, 16)
COLS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300)   # first chunk masked, last chunk masked, every step of nchunks = (n + 126) / 64
EDGE_FORMS = ((0, 0), (4, 4), (1, 3), (2, 3), (3, 3), (1, 1), (2, 2))   # test_gpu_parity.py::test_nw_and_semiglobal_edges, plus local
BASE = 300                                               # length of the string every region of a grid pair is a noisy copy of


def letters(way):
    """the alphabet of a way of WAYS -- or, for callers with ways of their own (tests/packed_cases.py), the alphabet itself as bytes"""
    return np.frombuffer(way if isinstance(way, bytes) else WAYS[way][0], dtype=np.uint8)


def flags(way):
    return WAYS[way][1]


def kernel_name(R, sw, profile, track, prune=False):
    """mi355sw_stats.kernel of the instantiation (runtime.cpp)"""
    b = lambda x: "true" if x else "false"
    return "sw_strip_kernel<%d,%s,%s,%s%s>" % (R, b(sw), b(profile), b(track), ",true" if prune else "")


def row_counts(R):
    """1, 2, R-1, R, R+1; SH-1, SH, SH+1; 2SH-1, 2SH+1; SH + R k + d at k = 0, 1, 62; about five strips.
    In a ragged second strip of SH + R k + d rows the last valid row is R k + d - 1: lane (R k + d - 1) / R, row (R k + d - 1) % R.
    d in {0, 1, R-1} gives rows R-1 (of the lane above), 0 and R-2; d = 2 and d = R are added so that emit_row is 1 and R-1 in
    lane k itself as well (emit_lane 0, 1, 62 with emit_row 0, 1, R-2, R-1)."""
    SH = 64 * R
    rows = [1, 2, R - 1, R, R + 1, SH - 1, SH, SH + 1, 2 * SH - 1, 2 * SH + 1]
    for k in (0, 1, 62):
        for d in (0, 1, 2, R - 1, R):
            rows.append(SH + R * k + d)
    rows.append(4 * SH + SH // 2 + 3)
    return sorted(set(rows))


def emit_position(R, m):
    """(ragged, emit_lane, emit_row) of the last strip of an m-row partition (sw_kernel.hip, process_strip)"""
    SH = 64 * R
    last = (m - 1) % SH
    return m % SH != 0, last // R, last % R


def _mutate(rng, a, alpha, rate):
    a = a.copy()
    hit = rng.random(len(a)) < rate
    a[hit] = rng.choice(alpha, size=int(hit.sum()))
    return a


FACING = (0,) + tuple(range(9, BASE, 37))                # foreign bytes of both sequences at the same place of the base string ...
BESIDE = tuple(range(23, BASE - 1, 41))                  # ... and one place apart


def _foreign0(tile):
    tile[[p for p in FACING if p < len(tile)]] = FOREIGN0[0]
    tile[[p for p in BESIDE if p < len(tile)]] = FOREIGN0[1]


def _foreign1(reg):
    reg[[p for p in FACING if p < len(reg)]] = FOREIGN1[0]
    reg[[p + 1 for p in BESIDE if p + 1 < len(reg)]] = FOREIGN1[1]


class GridPair:
    """one pair of sequences that holds a partition of every (rows, columns) shape at an offset of its own:
    seq1 = one region per column count, a noisy copy of base[:c]; seq0 = one region per row count, tiles of noisy copies of
    the base (two of three) and of unrelated letters (every third), so that the best cell of a tall partition may sit in any
    strip.  kind "iid": letters of the way's alphabet only; "foreign": two byte values of seq0 only and two of seq1 only, facing
    each other on the diagonal of every tile (FACING) and beside it (BESIDE).  Both sequences end with the whole alphabet: the
    number of common byte values is the way's K whatever the regions hold."""

    def __init__(self, way, rows, cols=COLS, kind="iid", seed=0):
        alpha = letters(way)
        rng = np.random.default_rng([seed, len(alpha), len(rows), kind == "foreign"])
        base = rng.choice(alpha, size=BASE)
        self.way, self.kind, self.rows, self.cols = way, kind, tuple(rows), tuple(cols)
        s0, s1 = [rng.choice(alpha, size=7)], [rng.choice(alpha, size=5)]
        self.i0, self.j0 = {}, {}
        pos = 7
        for r in self.rows:
            self.i0[r] = pos
            left = r
            t = 0
            while left > 0:
                tile = rng.choice(alpha, size=BASE) if t % 3 == 2 else _mutate(rng, base, alpha, 0.08)
                if kind == "foreign":
                    _foreign0(tile)
                s0.append(tile[:left])
                left -= len(tile[:left])
                t += 1
            s0.append(rng.choice(alpha, size=3))
            pos += r + 3
        pos = 5
        for c in self.cols:
            self.j0[c] = pos
            reg = _mutate(rng, base, alpha, 0.05)[:c]
            if c > BASE:
                reg = np.concatenate([reg, rng.choice(alpha, size=c - BASE)])
            if kind == "foreign":
                _foreign1(reg)
            s1.append(reg)
            s1.append(rng.choice(alpha, size=3))
            pos += c + 3
        self.s0 = np.concatenate(s0 + [alpha]).astype(np.uint8)
        self.s1 = np.concatenate(s1 + [alpha]).astype(np.uint8)

    def box(self, r, c):
        """(i0, j0, i1, j1) of the r x c partition"""
        return self.i0[r], self.j0[c], self.i0[r] + r, self.j0[c] + c

    def boxes(self):
        return [self.box(r, c) for r in self.rows for c in self.cols]


def related_pair(way, m, n, seed, rate=0.06):
    """a related pair in the way's alphabet: seq1 a noisy copy of seq0 with a short insertion, as seqgen.related_pair makes for ACGT"""
    alpha = letters(way)
    rng = np.random.default_rng([seed, m, n, len(alpha)])
    s0 = rng.choice(alpha, size=m)
    s1 = _mutate(rng, np.resize(s0, n), alpha, rate)
    if n > 200:
        s1 = np.concatenate([s1[:n // 2], rng.choice(alpha, size=17), s1[n // 2:n - 17]])
    return s0.astype(np.uint8), s1.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# low-complexity pairs: what reaches the canonical-best bookkeeping (mx >= best_t, r < best_r, the 64-lane reduction)
# ---------------------------------------------------------------------------------------------------------------------
LOW_M, LOW_N, LOW_P = 2100, 300, 97          # 2100 rows: nine strips at R = 4, three at R = 16
LOW_NAMES = ("A^m/A^n", "(AC)^m/(AC)^n", "(ACG)^m/(CGA)^n", "A^m/C^n", "P^k/P", "P/P^k", "P^k/P^k'", "P^k/PxP")


def _breaker(alpha, P):
    """a letter that continues no copy of P at either end"""
    return [x for x in alpha if x != P[0] and x != P[-1]][0]


def low_pair(name, way="generic", three_columns=False):
    """the low-complexity pairs by name, in the way's alphabet (P is drawn from it).  All are LOW_M x LOW_N or smaller, except
    "P/P^k", whose seq0 IS the 97-mer: one strip, the best score at several columns of ONE row.  "P^k/PxP" (added to the issue's
    list): seq1 = P, 53 letters that fit nothing, P -- bridging them costs more than the second copy brings, so the best score
    97 stands at columns 97 and 247 of every row 97 t: ties across strips, across the lanes of a strip and across the columns
    of a row in one pair.  three_columns: what the same generator gives the packed kernel -- seq1, a breaker too long to bridge,
    and seq1 again: a further run of columns that reaches the same best score in the same rows, more chunks for its column
    bookkeeping."""
    alpha = letters(way)
    a, c, g = alpha[0], alpha[1], alpha[2]
    rng = np.random.default_rng([97, len(alpha)])
    P = rng.choice(alpha, size=LOW_P)
    rep = lambda unit, length: np.resize(np.asarray(unit, dtype=np.uint8), length)
    m, n = LOW_M, LOW_N
    if name == "A^m/A^n":
        s0, s1 = rep([a], m), rep([a], n)
    elif name == "(AC)^m/(AC)^n":
        s0, s1 = rep([a, c], m), rep([a, c], n)
    elif name == "(ACG)^m/(CGA)^n":
        s0, s1 = rep([a, c, g], m), rep([c, g, a], n)
    elif name == "A^m/C^n":
        s0, s1 = rep([a], m), rep([c], n)
    elif name == "P^k/P":
        s0, s1 = rep(P, m), P.copy()
    elif name == "P/P^k":
        s0, s1 = P.copy(), rep(P, 3 * LOW_P)
    elif name == "P^k/P^k'":
        s0, s1 = rep(P, m).copy(), rep(P, 3 * LOW_P).copy()
        for k in range(m // LOW_P):                           # one substitution per copy: the same place in seq0 (the copies tie) ...
            q = k * LOW_P + 5
            s0[q] = alpha[(int(np.where(alpha == s0[q])[0][0]) + 1) % len(alpha)]
        for k in range(3):                                    # ... a place of its own in seq1
            q = k * LOW_P + (29 * k + 40) % LOW_P
            s1[q] = alpha[(int(np.where(alpha == s1[q])[0][0]) + 1) % len(alpha)]
    elif name == "P^k/PxP":
        x = rep([_breaker(alpha, P)], 53)                     # a run of one letter: no piece of P fits more than its own runs of it
        s0, s1 = rep(P, m), np.concatenate([P, x, P])
    else:
        raise ValueError(name)
    s0, s1 = np.ascontiguousarray(s0, dtype=np.uint8), np.ascontiguousarray(s1, dtype=np.uint8)
    if three_columns:                                         # (a breaker no gap bridges for less than the second run brings)
        x = _breaker(alpha, P) if "P" in name else alpha[3]
        s1 = np.concatenate([s1, rep([x], len(s1) // 2 + 5), s1]).astype(np.uint8)
    return s0, s1


def with_alphabet(way, s0, s1):
    """the pair inside sequences that carry the way's whole alphabet behind it (the number of common byte values decides the
    kernel): returns the longer sequences; the pair itself is the partition (0, 0, len(s0), len(s1))"""
    alpha = letters(way)
    return np.concatenate([s0, alpha]).astype(np.uint8), np.concatenate([s1, alpha]).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# custom borders
# ---------------------------------------------------------------------------------------------------------------------
def custom_border(length, corner, seed, local=False):
    """length + 1 border cells, the corner first: an irregular, steep walk from the corner's value (test_gpu_batch_stages.py,
    _custom_col) -- local: values in [0, 60) -- whose gap component lies 0 to 6 under H, so that it wins the E / F of the first
    cells wherever it is within the gap-open penalty of H, and is -INF in a tenth of the cells"""
    rng = np.random.RandomState(seed)
    c = np.zeros((length + 1, 2), dtype=np.int32)
    if local:
        c[:, 0] = rng.randint(0, 60, length + 1)
    else:
        c[0, 0] = corner
        c[1:, 0] = corner + np.cumsum(rng.randint(-7, 2, length))
    c[:, 1] = c[:, 0] - rng.randint(0, 7, length + 1)
    c[rng.rand(length + 1) < 0.1, 1] = -INF
    return c


def custom_borders(m, n, corner, seed, local=False):
    """(first row, first column) with one corner cell of its own"""
    row, col = custom_border(n, corner, 2 * seed, local), custom_border(m, corner, 2 * seed + 1, local)
    row[0] = col[0] = (corner, -INF)
    return row, col


# ---------------------------------------------------------------------------------------------------------------------
# one partition, its manager, its oracle run and the comparison
# ---------------------------------------------------------------------------------------------------------------------
class Part:
    """one partition.  start / end: the alignment edge flags (0 anywhere ... 4 both sequences; test_gpu_parity.py, EDGE); quiet: the
    manager refuses scores (TRACK = false); row / col: custom border cells (corner included) or None for the edge form's own;
    interval: special rows; stop_at: the manager says stop once its last column has passed this row"""

    def __init__(self, box, start=0, end=0, quiet=False, interval=0, row=None, col=None, stop_at=None):
        self.box, self.start, self.end, self.quiet, self.interval = tuple(int(x) for x in box), start, end, quiet, interval
        self.row, self.col, self.stop_at = row, col, stop_at

    @property
    def m(self):
        return self.box[2] - self.box[0]

    @property
    def n(self):
        return self.box[3] - self.box[1]

    def sw(self):
        return self.start == 0

    def tracked(self):
        return self.end == 0 and not self.quiet

    def manager(self, pkg, stop=True, **kw):
        from masa_cudalign_amd.manager import ArrayCellsReader
        args = dict(alignment_start=self.start, alignment_end=self.end,      # (the flags are AT_ANYWHERE = 0 ... AT_SEQUENCE_1_AND_2 = 4)
                    keep_last_row=True, keep_last_column=True, special_row_interval=self.interval)
        if self.row is not None:
            args["first_row_reader"] = ArrayCellsReader(self.row)
        if self.col is not None:
            args["first_column_reader"] = ArrayCellsReader(self.col)
        args.update(kw)
        return manager_class(pkg)(pkg.Partition(*self.box), stop_at=self.stop_at if stop else None, no_scores=self.quiet, **args)

    def borders(self, pkg):
        """the cells the manager's readers hand out (corner included), from readers of their own"""
        mg = self.manager(pkg)
        row = np.zeros((self.n + 1, 2), dtype=np.int32)
        col = np.zeros((self.m + 1, 2), dtype=np.int32)
        mg.first_row_reader.read(row, self.n + 1)
        mg.first_column_reader.read(col, self.m + 1)
        return row, col

    def oracle(self, pkg, oracle, s0, s1, block_h, rows=None, threads=0):
        """the oracle on the partition's letters with the manager's own borders as custom data; rows: only the first `rows` rows"""
        i0, j0, i1, j1 = self.box
        row, col = self.borders(pkg)
        if rows is not None:
            i1, col = i0 + rows, col[:rows + 1]
        best = {0: oracle.BEST_ANYWHERE, 1: oracle.BEST_LAST_ROW, 2: oracle.BEST_LAST_COL, 3: oracle.BEST_LAST_ROW_OR_COL, 4: oracle.BEST_LAST_CELL}[self.end]
        return oracle.stage1(s0[i0:i1], s1[j0:j1], recurrence=oracle.SMITH_WATERMAN if self.sw() else oracle.NEEDLEMAN_WUNSCH,
                             first_row_type=oracle.INIT_WITH_CUSTOM_DATA, first_col_type=oracle.INIT_WITH_CUSTOM_DATA,
                             custom_first_row=row, custom_first_col=col, block_h=block_h, block_w=1 << 20,
                             special_row_interval=self.interval, want_last_row=True, want_last_col=True, best_mode=best, threads=threads)


_MGR = {}


def manager_class(pkg):
    if "cls" in _MGR:
        return _MGR["cls"]

    class Mgr(pkg.Stage1Manager):
        """Stage1Manager that counts its first-column stream, notes the order in which special rows arrive, can say stop once its
        last column has passed a row (AlignerManager at a goal) and can refuse scores (TRACK = false for SW as well as NW)"""

        def __init__(self, part, stop_at=None, no_scores=False, **kw):
            pkg.Stage1Manager.__init__(self, part, **kw)
            self.stop_at, self.no_scores = stop_at, no_scores
            self.col_asked = 0
            self.row_order = []

        def receiveFirstColumn(self, buf, length):
            self.col_asked += length
            pkg.Stage1Manager.receiveFirstColumn(self, buf, length)

        def dispatchColumn(self, j, buf, length):
            pkg.Stage1Manager.dispatchColumn(self, j, buf, length)
            if self.stop_at is not None and self.last_column_pos > self.stop_at:
                self.active = False

        def dispatchRow(self, i, buf, length):
            self.row_order.append(i)
            pkg.Stage1Manager.dispatchRow(self, i, buf, length)

        def mustDispatchScores(self):
            return False if self.no_scores else pkg.Stage1Manager.mustDispatchScores(self)
    _MGR["cls"] = Mgr
    return Mgr


def special_rows(case, mg):
    """special rows the manager received ABOVE its last row, relative to the partition: {dp row: [chunks]}"""
    return {i - case.box[0]: v for i, v in mg.special_rows.items() if i < case.box[2]}


def delivered_once(case, mg):
    """every special row in order, none twice, in one delivery (the leading cell + the row)"""
    order = []
    for i in mg.row_order:
        if i < case.box[2] and (not order or order[-1] != i):
            order.append(i)
    assert order == sorted(set(order)), order
    for i, chunks in special_rows(case, mg).items():
        assert len(chunks) == 2, (i, len(chunks))


def expect_oracle(pkg, case, mg, ref, what=""):
    """a manager that ran to its end against the oracle: best cell, last row, last column, every special row once"""
    assert np.array_equal(mg.lastColumn(), ref["last_col"]), ("last column", what)
    assert np.array_equal(mg.lastRow(), ref["last_row"]), ("last row", what)
    bi, bj, bs = ref["best"]
    if case.quiet:
        assert tuple(mg.getBestScore()) == (-1, -1, -INF), (mg.getBestScore(), what)
    elif case.end in (0, 4):
        # the oracle's best cell through a manager of the same kind (its own rules: a minimum score, the last cell only)
        want = case.manager(pkg)
        if bs > -INF:
            want.dispatchScore((case.box[0] + bi - 1, case.box[1] + bj - 1, bs))
        assert tuple(mg.getBestScore()) == tuple(want.getBestScore()), (mg.getBestScore(), want.getBestScore(), ref["best"], what)
    else:
        assert tuple(mg.getBestScore()) == (case.box[0] + bi, case.box[1] + bj, bs), (mg.getBestScore(), ref["best"], what)
    want = {r: ref["special_rows"][k] for k, r in enumerate(ref["special_row_ids"]) if r < case.m}
    got = special_rows(case, mg)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want), what)
    for r in want:
        assert np.array_equal(np.concatenate(got[r]), want[r]), ("special row", r, what)
    delivered_once(case, mg)
    assert mg.col_asked <= case.m + 1, (mg.col_asked, what)            # the first-column stream: read once at the most


# ---------------------------------------------------------------------------------------------------------------------
# which combinations the GPU file runs
# ---------------------------------------------------------------------------------------------------------------------
EDGE_ROWS = lambda R: (R + 1, 64 * R + 1, 64 * R + R + 2, 2 * 64 * R + 1)     # m < strip, one row into the second strip, emit_row 1, three strips
EDGE_COLS = (65, 193, 300)


def instantiation_grid():
    """test 1: [(R, sw, profile, track, way)] -- the 24 unpruned instantiations; PROFILE = false alternates between the three
    byte-compare ways so that each height meets each of them"""
    out = []
    compare = ("coded", "raw15", "generic")
    k = 0
    for R in HEIGHTS:
        for sw in (True, False):
            for profile in (True, False):
                for track in (True, False):
                    way = "profile" if profile else compare[k % 3]
                    k += 0 if profile else 1
                    out.append((R, sw, profile, track, way))
    return out


def census():
    """(way, R, rows, columns, edge form) combinations of tests 1 and 2 of the GPU file, and how many of them are ragged, have
    n < 64 or m < R"""
    combos = []
    for R, sw, profile, track, way in instantiation_grid():
        form = (0, 0) if sw else ((4, 0) if track else (4, 4))
        for kind in ("iid", "foreign"):
            for r in row_counts(R):
                for c in COLS:
                    combos.append((way, R, r, c, form, kind, track))
    for way in WAYS:
        for R in HEIGHTS:
            for form in EDGE_FORMS:
                for r in EDGE_ROWS(R):
                    for c in EDGE_COLS:
                        combos.append((way, R, r, c, form, "iid", form[1] == 0))
    return {"combinations": len(combos), "distinct": len(set(combos)),
            "ragged": sum(1 for x in combos if x[2] % (64 * x[1]) != 0),
            "n<64": sum(1 for x in combos if x[3] < 64), "m<R": sum(1 for x in combos if x[2] < x[1])}
