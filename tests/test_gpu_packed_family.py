"""GPU: the packed 16-bit kernel family (csrc/sw_kernel_pk16.inc, built as sw_kernel_pk16_{a..j}.hip and the wide-alphabet twins
sw_kernel_pk16_w{a..j}.hip) held to the oracle instantiation by instantiation, each named in mi355sw_stats.kernel.  Heights are
R' = rows_per_lane / 2, a strip is SH = 128 R' rows.  Inputs and shape lists: tests/packed_cases.py (shown to be what they claim
by tests/test_packed_case_inputs.py on the CPU).  Integer work: every comparison is bit-exact against oracle.stage1 /
oracle.process_block -- the best cell through a manager of the same kind, the last row, the last column, every special row
delivered once, the first-column stream read at most once.  One aligner per (way, height), many small partitions per test."""
import numpy as np
import pytest

import packed_cases as pc
from helpers import NEEDLEMAN_WUNSCH, SMITH_WATERMAN, assert_pruned_borders, manager_rows, oracle_kwargs

pytestmark = pytest.mark.gpu

TWINS = [(wide, Rh) for wide in (False, True) for Rh in pc.HEIGHTS]
TWIN_IDS = ["%s-%d" % ("wide" if w else "narrow", 128 * Rh) for w, Rh in TWINS]


def _way(wide, k):
    """the ways of a twin in turn"""
    ways = pc.WIDE if wide else pc.NARROW
    return ways[k % len(ways)]


def _aligner(pkg, way, Rh, flags=0, **kw):
    return pkg.MI355Aligner(device=0, rows_per_lane=2 * Rh, flags=pc.flags(way) | flags, **kw)


def _in_twin(st, way, kernel=None, rows=None):
    """the way led into its twin: the packed kernels, no rerun on the int32 family, `_wide<` in the name or not"""
    assert st["profile_kernel"] == 2 and st["restarts"] == 0, (st["profile_kernel"], st["restarts"], st["kernel"], way)
    assert ("_wide<" in st["kernel"]) == pc.is_wide(way), (st["kernel"], way)
    if kernel is not None:
        assert st["kernel"] == kernel, (st["kernel"], kernel)
    if rows is not None:
        assert st["strip_rows"] == rows, (st["strip_rows"], rows)


def _expect_without_last_row(pkg, case, mg, ref, what=""):
    """a run nobody read the last row of: the best cell and the last column are the oracle's, the first column was read once"""
    assert mg.last_row_chunks == [], what
    assert np.array_equal(mg.lastColumn(), ref["last_col"]), ("last column", what)
    bi, bj, bs = ref["best"]
    if case.quiet:
        assert tuple(mg.getBestScore()) == (-1, -1, -pc.INF), (mg.getBestScore(), what)
    elif case.end == 0:
        want = case.manager(pkg)
        if bs > -pc.INF:
            want.dispatchScore((case.box[0] + bi - 1, case.box[1] + bj - 1, bs))
        assert tuple(mg.getBestScore()) == tuple(want.getBestScore()), (mg.getBestScore(), want.getBestScore(), what)
    else:                                                    # the best of the last column: the manager's own argmax over exact cells
        assert case.end == 2 and mg.getBestScore()[2] == int(ref["last_col"][:, 0].max()), (mg.getBestScore(), what)
    assert mg.col_asked <= case.m + 1, (mg.col_asked, what)


def _run(pkg, oracle, al, way, s0, s1, cases, kernel, rows, block_h=None, threads=0):
    """every case through alignPartition on the aligner (its sequences set) and against the oracle in full"""
    for c in cases:
        mg = c.manager(pkg)
        al.alignPartition(pkg.Partition(*c.box), mg)
        st = al.getStatistics()
        _in_twin(st, way, kernel(c) if callable(kernel) else kernel, rows)
        ref = c.oracle(pkg, oracle, s0, s1, block_h or st["strip_rows"], threads=threads)
        pc.expect_oracle(pkg, c, mg, ref, (way, c.box, c.start, c.end, c.quiet, st["kernel"]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the 24 unpruned strip instantiations of each twin, by name
# ---------------------------------------------------------------------------------------------------------------------
_GRID = pc.unpruned_grid()


@pytest.mark.parametrize("kind", ["iid", "foreign"])
@pytest.mark.parametrize("wide,Rh,track,sw,way", _GRID,
                         ids=["%d-%s-%s-%s" % (128 * g[1], "sw" if g[3] else "nw", "track" if g[2] else "quiet", g[4]) for g in _GRID])
def test_every_unpruned_instantiation_by_name(pkg, oracle, wide, Rh, track, sw, way, kind):
    """each instantiation on every row count of packed_cases.row_counts(R') (1 ... four and a half strips: every emit lane, half
    and row of a ragged last strip) times every column count (1 ... 449: the output chunk trails by up to 127 columns, the table
    form reaches three chunks back), on `iid` letters and with foreign bytes facing each other.  TRACK = false: NW to the last
    cell, and SW through a manager that refuses scores; TRACK = true for NW: global start, best anywhere.  Every ragged shape runs
    twice: with the last row read (the emit position moves off the strip's bottom) and with keep_last_row=False (the ragged strip
    takes the ordinary code, the table form included) -- NW to the last cell always reads its last row, so its second run looks
    for the best of the last column instead: the same instantiation, the same first row and column."""
    SH = 128 * Rh
    start, end, quiet = pc.form_of(track, sw)
    name = pc.strip_name(Rh, track, sw, False, wide)
    g = pc.grid_pair(way, pc.row_counts(Rh), kind=kind, seed=Rh)
    al = _aligner(pkg, way, Rh)
    try:
        al.setSequences(g.s0, g.s1)
        for box in g.boxes():
            c = pc.Part(box, start, end, quiet=quiet)
            mg = c.manager(pkg)
            al.alignPartition(pkg.Partition(*box), mg)
            st = al.getStatistics()
            _in_twin(st, way, name, SH)
            ref = c.oracle(pkg, oracle, g.s0, g.s1, SH)
            pc.expect_oracle(pkg, c, mg, ref, (way, kind, box, name))
            if c.m % SH != 0:
                c2 = c if end != 4 else pc.Part(box, 4, 2)
                mg = c2.manager(pkg, keep_last_row=False)
                al.alignPartition(pkg.Partition(*box), mg)
                _in_twin(al.getStatistics(), way, name, SH)
                _expect_without_last_row(pkg, c2, mg, ref, (way, kind, box, name, "no last row"))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. edge forms, custom borders, partitions at an offset, processBlock
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,Rh", TWINS, ids=TWIN_IDS)
def test_edge_forms_and_custom_borders_at_an_offset(pkg, oracle, wide, Rh):
    """every partition sits at (i0, j0) != (0, 0) inside longer sequences.  The engine's own borders for all seven edge forms; then
    custom first rows and first columns -- a corner of its own, values near +-120 000 000 (the wave-uniform bias far from 0, a
    re-centre at the first chunk), gap components 0 to 6 under H that decide the first E / F, -INF in a tenth of them (-32768 in
    the 16-bit domain, and it must stay there) -- for NW to the last cell, NW with the best anywhere (far below zero: rows past the
    end of a ragged strip hold more than any real cell), a goal sweep (last column only), and SW with and without scores"""
    way = _way(wide, pc.HEIGHTS.index(Rh))
    g = pc.grid_pair(way, pc.EDGE_ROWS(Rh), pc.EDGE_COLS, seed=20 + Rh)
    cases = [pc.Part(b, s, e) for s, e in pc.EDGE_FORMS for b in g.boxes()]
    forms = [(4, 4, False, pc.OFFSET), (4, 0, False, -pc.OFFSET), (4, 2, False, -1234), (0, 0, False, None), (0, 0, True, None)]
    for k, b in enumerate(g.boxes()):
        for f, (s, e, quiet, corner) in enumerate(forms):
            row, col = pc.custom_borders(b[2] - b[0], b[3] - b[1], corner or 0, 100 * k + f, local=corner is None)
            cases.append(pc.Part(b, s, e, quiet=quiet, row=row, col=col))
    al = _aligner(pkg, way, Rh)
    try:
        al.setSequences(g.s0, g.s1)
        _run(pkg, oracle, al, way, g.s0, g.s1, cases, lambda c: pc.strip_name(Rh, c.tracked(), c.sw(), False, wide), 128 * Rh)
    finally:
        al.close()


@pytest.mark.parametrize("wide,Rh", TWINS, ids=TWIN_IDS)
def test_process_block_on_the_packed_family(pkg, oracle, wide, Rh):
    """AbstractBlockProcessor::processBlock: random borders with -INF entries, SW and NW, blocks at an offset, one row high, eight
    columns wide, two strips and five rows tall -- and NW once more with the borders 120 000 000 down: every real cell then lies far
    under what the rows past the end of a ragged strip hold"""
    way = _way(wide, pc.HEIGHTS.index(Rh) + 1)
    SH = 128 * Rh
    rng = np.random.default_rng(11 + Rh)
    size = max(3000, 2 * SH + 300)
    s0, s1 = pc.with_alphabet(pc.alphabet(way), *pc.related_pair(pc.alphabet(way), size, 3000, 81))
    al = _aligner(pkg, way, Rh)
    try:
        al.setSequences(s0, s1)
        for rec, deep in ((pkg.SMITH_WATERMAN, 0), (pkg.NEEDLEMAN_WUNSCH, 0), (pkg.NEEDLEMAN_WUNSCH, -pc.OFFSET)):
            for (i0, j0, i1, j1) in [(0, 0, 700, 900), (100, 250, 1124, 314), (1000, 1000, 1001, 2500), (5, 7, 1500, 8), (3, 11, 3 + 2 * SH + 5, 211)]:
                m, n = i1 - i0, j1 - j0
                row = np.stack([deep + rng.integers(0, 50, n), deep + rng.integers(-60, 40, n)], axis=1).astype(np.int32)
                col = np.stack([deep + rng.integers(0, 50, m + 1), deep + rng.integers(-60, 40, m + 1)], axis=1).astype(np.int32)
                row[rng.integers(0, n, max(1, n // 10)), 1] = -pkg.INF
                col[1 + rng.integers(0, m, max(1, m // 10)), 1] = -pkg.INF
                r1, c1 = row.copy(), col.copy()
                b1 = oracle.process_block(s0, s1, r1, c1, i0, j0, i1, j1, rec)
                r2, c2 = row.copy(), col.copy()
                b2 = al.processBlock(r2, c2, i0, j0, i1, j1, rec)
                _in_twin(al.getStatistics(), way, pc.strip_name(Rh, True, rec == pkg.SMITH_WATERMAN, False, wide), SH)
                assert np.array_equal(r1, r2) and np.array_equal(c1, c2), (way, Rh, rec, deep, i0, j0)
                assert tuple(b1) == tuple(b2), (b1, b2, way, Rh, rec, deep, i0, j0)
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. special rows at the first two rows the runtime grants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_per_lane", [4, 8, 16, 32, 12, 24, 0])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_special_rows_at_the_smallest_spacing(pkg, oracle, wide, rows_per_lane):
    """the smallest spacing the runtime grants is 8192 rows rounded up to the grid: 8192 at 256-, 512-, 1024- and 2048-row strips,
    fixed (the strips' own grid) and engine-picked (the 2048-row unit), 8448 at fixed 768-row strips and 9216 at fixed 1536-row
    strips.  g rows give no special row, g + 1 one, 2 g one (the row at m is not special), 2 g + 1 two; the oracle with the same
    block height says where they go.  SW and NW, 193 columns, the partition at an offset."""
    way = "wide15" if wide else "acgt"
    n = 193
    SH = 64 * rows_per_lane
    g = (8192 + SH - 1) // SH * SH if SH else 8192
    s0, s1 = pc.with_alphabet(pc.alphabet(way), *pc.related_pair(pc.alphabet(way), 2 * g + 1 + 3, n + 5, 33))
    want = {g: [], g + 1: [g], 2 * g: [g], 2 * g + 1: [g, 2 * g]}
    al = pkg.MI355Aligner(device=0, rows_per_lane=rows_per_lane, flags=pc.flags(way))
    picked = set()
    try:
        al.setSequences(s0, s1)
        for m in sorted(want):
            for start, end in ((0, 0), (4, 4)):
                c = pc.Part((3, 5, 3 + m, 5 + n), start, end, interval=8192)
                mg = c.manager(pkg)
                al.alignPartition(pkg.Partition(*c.box), mg)
                st = al.getStatistics()
                _in_twin(st, way, pc.strip_name(st["strip_rows"] // 128, start == 0, start == 0, False, wide), SH or None)
                assert st["strip_rows"] in (256, 512, 1024, 2048) or rows_per_lane in (12, 24)
                picked.add(st["strip_rows"])
                assert sorted(pc.special_rows(c, mg)) == want[m], (m, sorted(pc.special_rows(c, mg)))
                ref = c.oracle(pkg, oracle, s0, s1, SH or 2048, threads=pc.THREADS)
                pc.expect_oracle(pkg, c, mg, ref, (way, rows_per_lane, m, start))
    finally:
        al.close()
    print("rows_per_lane %d, %s: strips of %s rows" % (rows_per_lane, way, sorted(picked)))


# ---------------------------------------------------------------------------------------------------------------------
# 4. low-complexity pairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,Rh", TWINS, ids=TWIN_IDS)
def test_low_complexity_pairs_keep_the_canonical_best(pkg, oracle, wide, Rh):
    """periodic sequences with a further run of columns (int32_cases.low_pair(..., three_columns=True)): the same best score in
    many strips, in many lanes of a strip and at several columns of a row -- the fast pass with the chunk maximum on every other
    row and the exact replay that restores the canonical cell.  The best cell is the oracle's (min i, then min j): unpruned; with
    block pruning, the borders held by assert_pruned_borders; and under MI355SW_F_TWO_PHASE (a value-only main pass and the exact
    pass of the winning strip).  The wide twin takes the pair inside a 15-letter alphabet."""
    way = "wide15" if wide else "acgt"
    SH = 128 * Rh
    for two_phase in (False, True):
        al = _aligner(pkg, way, Rh, flags=pc.F_TWO_PHASE if two_phase else 0)
        try:
            for name in pc.LOW_NAMES:
                s0, s1 = pc.low_pair(name, pc.alphabet(way), three_columns=True)
                m, n = len(s0), len(s1)
                q0, q1 = pc.with_alphabet(pc.alphabet(way), s0, s1)
                al.setSequences(q0, q1)
                c = pc.Part((0, 0, m, n))
                ref = c.oracle(pkg, oracle, q0, q1, SH)
                for prune in ((False,) if two_phase else (False, True)):
                    mg = c.manager(pkg, block_pruning=prune)
                    al.alignPartition(pkg.Partition(*c.box), mg)
                    st = al.getStatistics()
                    _in_twin(st, way, pc.strip_name(Rh, not two_phase, True, prune, wide), SH)
                    what = (way, Rh, name, prune, two_phase, st["pruned_cells"])
                    if two_phase:
                        assert st["kernel_launches"] == 2 or ref["best"][2] == 0, what
                    if not prune:
                        assert st["pruned_cells"] == 0
                        pc.expect_oracle(pkg, c, mg, ref, what)
                    else:
                        assert st["pruned_cells"] + st["processed_cells"] == m * n, what
                        assert tuple(mg.getBestScore()) == tuple(ref["best"]), (mg.getBestScore(), ref["best"], what)
                        assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, ref["best"][2], SMITH_WATERMAN,
                                              col0=True, where=str(what))
        finally:
            al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the pruning instantiations, one wavefront
# ---------------------------------------------------------------------------------------------------------------------
# Per R' and twin, related_pair(alphabet, m, m, 700 + R') with m a multiple of the strip height (computed on the CPU, asserted by
# tests/test_packed_case_inputs.py):
#   "sw": (m, blocks pruned, blocks) -- the smallest m at which the oracle's own pruned run, blocks of SH x 64, prunes a tenth
#   "nw": (m, blocks the rule may skip, blocks, H[m][n]) -- the smallest m at which the blocks of SH x 64 that may go WHOLE (every
#         cell of the block is one helpers.assert_pruned_cells does not hold exact, goal = H[m][n]) hold a tenth of the cells.  The
#         reference's rule skips blocks, so that is what "the reference alone" can prune: in a one-strip matrix every block holds
#         cells of the main diagonal and none may go (though 84 to 96 % of the single cells might); at two strips 37 to 48 % go.
PRUNE_SHAPES = {
    ("acgt", 2): {"sw": (1280, 17, 100), "nw": (512, 6, 16, 338)},
    ("acgt", 4): {"sw": (1024, 4, 32), "nw": (1024, 14, 32, 767)},
    ("acgt", 6): {"sw": (1536, 7, 48), "nw": (1536, 22, 48, 1197)},
    ("acgt", 8): {"sw": (2048, 9, 64), "nw": (2048, 30, 64, 1609)},
    ("acgt", 12): {"sw": (3072, 15, 96), "nw": (3072, 46, 96, 2517)},
    ("acgt", 16): {"sw": (4096, 20, 128), "nw": (4096, 60, 128, 3179)},
    ("wide15", 2): {"sw": (1280, 18, 100), "nw": (512, 6, 16, 301)},
    ("wide15", 4): {"sw": (1024, 4, 32), "nw": (1024, 14, 32, 738)},
    ("wide15", 6): {"sw": (1536, 7, 48), "nw": (1536, 22, 48, 1157)},
    ("wide15", 8): {"sw": (2048, 9, 64), "nw": (2048, 28, 64, 1433)},
    ("wide15", 12): {"sw": (3072, 15, 96), "nw": (3072, 44, 96, 2262)},
    ("wide15", 16): {"sw": (4096, 20, 128), "nw": (4096, 60, 128, 3125)},
}
PRUNE_CASES = {"sw-track": (True, True, 0), "sw-two-phase": (False, True, pc.F_TWO_PHASE), "nw": (False, False, 0)}


@pytest.mark.parametrize("case", list(PRUNE_CASES))
@pytest.mark.parametrize("wide,Rh", TWINS, ids=TWIN_IDS)
def test_pruning_instantiations_prune_and_keep_what_matters(pkg, oracle, wide, Rh, case):
    """<R',true,true,true>, <R',false,true,true> (MI355SW_F_TWO_PHASE with pruning: two launches, the canonical cell from the exact
    pass) and <R',false,false,true> (a global alignment, the goal is the last cell) with one wavefront (waves=1: strips one after
    the other, what is pruned is a function of the input): cells are pruned, pruned and processed cells add up to the matrix, the
    best cell is the oracle's and every border value that could still matter is exact.  Should the engine prune nothing at the
    reference's shape, the shape is doubled once; the assertion stays."""
    way = "wide15" if wide else "acgt"
    SH = 128 * Rh
    track, sw, fl = PRUNE_CASES[case]
    size = PRUNE_SHAPES[(way, Rh)]["sw" if sw else "nw"][0]
    start = end = 0 if sw else 4
    results = []
    al = _aligner(pkg, way, Rh, flags=fl, waves=1)
    try:
        for m in (size, 2 * size):
            s0, s1 = pc.related_pair(pc.alphabet(way), m, m, 700 + Rh)
            q0, q1 = pc.with_alphabet(pc.alphabet(way), s0, s1)
            al.setSequences(q0, q1)
            c = pc.Part((0, 0, m, m), start, end)
            mg = c.manager(pkg, block_pruning=True)
            al.alignPartition(pkg.Partition(*c.box), mg)
            st = al.getStatistics()
            _in_twin(st, way, pc.strip_name(Rh, track, sw, True, wide), SH)
            assert st["waves"] == 1
            results.append((m, st["pruned_cells"]))
            print("pruning %s %s R' %d: %d x %d, %d cells pruned of %d" % (case, way, Rh, m, m, st["pruned_cells"], m * m))
            if st["pruned_cells"] > 0:
                break
        assert st["pruned_cells"] > 0, results
        assert st["pruned_cells"] + st["processed_cells"] == m * m
        if fl:
            assert st["kernel_launches"] == 2, st["kernel_launches"]
        ref = c.oracle(pkg, oracle, q0, q1, SH, threads=pc.THREADS)
        assert tuple(mg.getBestScore()) == tuple(ref["best"]), (mg.getBestScore(), ref["best"])
        assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, m, ref["best"][2], SMITH_WATERMAN if sw else NEEDLEMAN_WUNSCH,
                              col0=True, where="%s %s R' %d" % (case, way, Rh))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the mixed kernels, both recurrences
# ---------------------------------------------------------------------------------------------------------------------
# (wavefronts, columns, row counts): the smallest matrices at which the engine's own cost model picks 1536-row strips that leave
# part of the last round idle AND strips of both heights run (packed_cases.mixed_plan restates the rule; the CPU file holds these
# shapes to it).  16 strips for 22 529 to 23 040 rows: the last 1408-row strip is ragged with emit_half 0 (22 529, 22 600) and 1
# (22 611), one row short (22 655) and full (22 656; 23 040 with four 1536-row strips).
MIXED_SHAPES = [(2, 160, (22529, 22600, 22611, 22655, 22656, 23040)), (4, 500, (22611, 22656)), (8, 1160, (33793,))]


@pytest.mark.parametrize("sw", [True, False], ids=["sw", "nw"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_mixed_heights_both_recurrences(pkg, oracle, wide, sw):
    """sw_strip_kernel_pk16_mixed<12,11,true,SW>: R' = 11 exists nowhere else.  The engine picks the launch itself
    (rows_per_lane = 0; a tracked best, a zero first column, no last column) -- the name is asserted, so a drift of the cost
    model fails here and is not skipped.  NW: gap-initialised first row, zero first column, best anywhere.  The best cell and the
    last row are the oracle's."""
    way = "wide15" if wide else "acgt"
    eng = pkg.engine
    for W, n, ms in MIXED_SHAPES:
        s0, s1 = pc.with_alphabet(pc.alphabet(way), *pc.related_pair(pc.alphabet(way), max(ms), n, 60 + W))
        al = pkg.MI355Aligner(device=0, waves=W, flags=pc.flags(way))
        try:
            al.setSequences(s0, s1)
            for m in ms:
                plan = pc.mixed_plan(m, n, W)
                al.streamBegin(pkg.Partition(0, 0, m, n), recurrence_type=eng.SMITH_WATERMAN if sw else eng.NEEDLEMAN_WUNSCH,
                               first_row_init_type=eng.INIT_WITH_ZEROES if sw else eng.INIT_WITH_GAPS, want_last_row=True, track_best=True)
                while not al.streamPoll()[1]:
                    pass
                row = al.streamReadLastRow()
                best, _ = al.streamEnd()
                st = al.getStatistics()
                _in_twin(st, way, pc.mixed_name(sw, wide), 1536)
                assert (st["strips_first"], st["strips"], st["strip_rows_second"]) == (plan[0], plan[1], 1408), (st, plan)
                ref = oracle.stage1(s0[:m], s1[:n], recurrence=oracle.SMITH_WATERMAN if sw else oracle.NEEDLEMAN_WUNSCH,
                                    first_row_type=oracle.INIT_WITH_ZEROES if sw else oracle.INIT_WITH_GAPS, want_last_row=True, threads=pc.THREADS)
                assert tuple(best) == (ref["best"][0] - 1, ref["best"][1] - 1, ref["best"][2]), (best, ref["best"], W, m, n)
                assert np.array_equal(row, ref["last_row"][1:]), (W, m, n)
        finally:
            al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the batch kernels, by name
# ---------------------------------------------------------------------------------------------------------------------
_BATCH = [(wide, Rh, track, sw) for wide in (False, True) for Rh in pc.BATCH_HEIGHTS for track in (True, False) for sw in (True, False)]


@pytest.mark.parametrize("wide,Rh,track,sw", _BATCH,
                         ids=["%s-%d-%s-%s" % ("wide" if b[0] else "narrow", 128 * b[1], "sw" if b[3] else "nw", "track" if b[2] else "quiet") for b in _BATCH])
def test_every_batch_instantiation_by_name(pkg, oracle, wide, Rh, track, sw):
    """sw_batch_kernel_pk16<R',TRACK,SW>: one launch of alignPartitions over twelve ragged partitions of the grid, at offsets -- one
    row into the second strip, the emit positions of lanes 31 / 32 and 63, three strips -- each equal to the oracle"""
    way = _way(wide, _BATCH.index((wide, Rh, track, sw)))
    SH = 128 * Rh
    start, end, quiet = pc.form_of(track, sw)
    rows = (Rh + 1, SH + 1, SH + 63 * Rh + 2, SH + 64 * Rh + 1, SH + 127 * Rh + Rh - 1, 2 * SH + 1)
    g = pc.grid_pair(way, rows, (65, 300), seed=40 + Rh)
    cases = [pc.Part(b, start, end, quiet=quiet) for b in g.boxes()]
    al = _aligner(pkg, way, Rh)
    try:
        al.setSequences(g.s0, g.s1)
        mgs = [c.manager(pkg) for c in cases]
        al.alignPartitions([pkg.Partition(*c.box) for c in cases], mgs, rows_per_lane=2 * Rh)
        st = al.getStatistics()
    finally:
        al.close()
    _in_twin(st, way, pc.batch_name(Rh, track, sw, wide), SH)
    assert st["kernel_launches"] == 1, st["kernel_launches"]
    for c, mg in zip(cases, mgs):
        pc.expect_oracle(pkg, c, mg, c.oracle(pkg, oracle, g.s0, g.s1, SH), (way, c.box, st["kernel"]))


# ---------------------------------------------------------------------------------------------------------------------
# 8. the stage-2-shaped stop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_a_stop_like_stage2_at_its_goal(pkg, oracle, wide):
    """the stop test of tests/test_gpu_int32_family.py at 256-row strips: NW from a crosspoint, custom borders (packed_cases.stop_borders:
    that file's, with a fall a 16-bit window can follow), 1 000 000 x 300, last column dispatched, the manager says stop once its
    last column has passed row 20 000.  What was dispatched before the stop is the oracle's, no special row below the stop is
    handed over, and the first-column stream is read at most once"""
    way = "wide15" if wide else "acgt"
    Rh, m, n, stop_at = 2, 1000000, 300, 20000
    s0, s1 = pc.with_alphabet(pc.alphabet(way), *pc.related_pair(pc.alphabet(way), m + 9, n + 4, 91))
    row, col = pc.stop_borders(m, n, -777, 6)
    c = pc.Part((9, 4, 9 + m, 4 + n), 4, 2, interval=8192, row=row, col=col, stop_at=stop_at)
    al = _aligner(pkg, way, Rh)
    try:
        al.setSequences(s0, s1)
        mg = c.manager(pkg)
        al.alignPartition(pkg.Partition(*c.box), mg)
        st = al.getStatistics()
    finally:
        al.close()
    _in_twin(st, way, pc.strip_name(Rh, False, False, False, wide), 128 * Rh)
    got = mg.lastColumn()                                    # the corner cell + the rows dispatched before the stop
    seen = len(got) - 1
    assert stop_at <= seen < m, seen                         # it did stop
    upto = min(m, seen + 128 * Rh)
    ref = c.oracle(pkg, oracle, s0, s1, 128 * Rh, rows=upto, threads=pc.THREADS)     # rows 0..seen depend on nothing below them
    assert np.array_equal(got, ref["last_col"][:seen + 1])
    want = dict(zip(ref["special_row_ids"], ref["special_rows"]))
    rows = pc.special_rows(c, mg)
    assert rows and all(r <= seen for r in rows), (sorted(rows), seen)
    for r, chunks in rows.items():
        assert np.array_equal(np.concatenate(chunks), want[r]), r
    pc.delivered_once(c, mg)
    assert mg.col_asked <= m + 1, mg.col_asked
    # (1024 wavefronts sweep these 300 columns in about a millisecond: whether rows are left when the stop arrives is a matter of
    #  timing here, unlike on the int32 family.  What holds whatever the timing is the bound of test_gpu_parity.py's stop test:
    #  nothing is computed below the rows the engine had been fed, but for the strips in flight)
    assert st["processed_cells"] <= min(m, mg.col_asked + (st["waves"] + 1) * st["strip_rows"]) * n


# ---------------------------------------------------------------------------------------------------------------------
# 9. goal and edge instantiations no other file names: the wide twin's
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_goal_strip_kernel_at_512_rows(pkg, oracle):
    """sw_strip_kernel_pk16_wide<4,false,false,true,true> (tests/test_gpu_wide_alphabet.py names the 256-row one): one goal sweep
    with B = (largest H of the oracle's last column) - 200, a ragged last strip and a partly filled last chunk"""
    from test_gpu_goal_prune import _check_sweep, _manager, _reference
    m, n = 2049, 1601
    s0, s1 = pc.with_alphabet(pc.alphabet("wide15"), *pc.related_pair(pc.alphabet("wide15"), m, n, 71))
    ref = _reference(oracle, s0[:m], s1[:n], 512, 8192)
    bound = int(ref["last_col"][:, 0].max()) - 200
    al = _aligner(pkg, "wide15", 4)
    try:
        al.setSequences(s0, s1)
        part = pkg.Partition(0, 0, m, n)
        mg = _manager(pkg, part, 8192)
        al.setGoalBounds([bound])
        al.alignPartition(part, mg)
        st = al.getStatistics()
    finally:
        al.close()
    _in_twin(st, "wide15", pc.strip_name(4, False, False, True, True, goal=True), 512)
    assert st["kernel_launches"] == 1
    assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == m * n
    _check_sweep(mg, ref, m, n, bound, "wide goal sweep, 512-row strips")


@pytest.mark.parametrize("Rh", [2, 8])
def test_wide_goal_batch_kernels(pkg, oracle, Rh):
    """sw_batch_kernel_pk16_wide<R',false,false,true,true>: three partitions along the diagonal of a 15-letter related pair in one
    launch, two bounds and a partition without one"""
    from test_gpu_goal_prune import INF, _check_sweep, _reference
    way = "wide15"
    m, n = 2048, 1536
    s0, s1 = pc.with_alphabet(pc.alphabet(way), *pc.related_pair(pc.alphabet(way), 3 * m, 3 * n, 72, rate=0.04))
    parts = [pkg.Partition(k * m, k * n, (k + 1) * m, (k + 1) * n) for k in range(3)]
    refs = [_reference(oracle, s0[p.i0:p.i1], s1[p.j0:p.j1], 128 * Rh, 0) for p in parts]
    tops = [int(r["last_col"][:, 0].max()) for r in refs]
    bounds = [tops[0] - 200, -INF, tops[2] - 60]
    al = pkg.MI355Aligner(device=0, flags=pc.flags(way))
    try:
        al.setSequences(s0, s1)
        mgs = [pkg.Stage1Manager(p, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_OR_2,
                                 keep_last_row=True, keep_last_column=True) for p in parts]
        al.setGoalBounds(bounds)
        al.alignPartitions(parts, mgs, rows_per_lane=2 * Rh)
        st = al.getStatistics()
    finally:
        al.close()
    _in_twin(st, way, pc.batch_name(Rh, False, False, True, goal=True), 128 * Rh)
    assert st["kernel_launches"] == 1
    for k in (0, 2):
        _check_sweep(mgs[k], refs[k], m, n, bounds[k], "partition %d" % k)
    assert np.array_equal(mgs[1].lastColumn(), refs[1]["last_col"]) and np.array_equal(mgs[1].lastRow(), refs[1]["last_row"])
    assert 0 < st["pruned_cells"] <= 2 * m * n and st["pruned_cells"] + st["processed_cells"] == 3 * m * n


_EDGE_REF = {}


@pytest.mark.parametrize("Rh", [2, 4, 8, 16])
def test_wide_edge_kernels_by_height(pkg, oracle, Rh):
    """sw_strip_kernel_pk16_wide<R',false,false,true,false,true> at each of its four heights (tests/test_gpu_edge_prune.py runs the
    wide twin at the engine's own choice of height only): the three edge modes on a 15-letter related pair, held as that file
    holds its runs -- the result cell, last row, last column, the cell count, the kernel"""
    import edge_prune_cases as ec
    from test_gpu_edge_prune import check_pruned_run, edge_run
    way = "wide15"
    m, n = 9000, 7000
    s0, s1 = pc.related_pair(pc.alphabet(way), m, n, 77, rate=0.04)
    if "ref" not in _EDGE_REF:                               # computed once, shared by the four heights, left unchanged
        kw = oracle_kwargs(oracle, dict(start=4, end=3, pruning=False, disk=-1, block=(1024, 1 << 20)), m, n)
        kw.update(want_last_row=True, want_last_col=True, threads=pc.THREADS)
        _EDGE_REF["ref"] = oracle.stage1(s0, s1, **kw)
        for a in (_EDGE_REF["ref"]["last_row"], _EDGE_REF["ref"]["last_col"]):
            a.setflags(write=False)
    ref = _EDGE_REF["ref"]
    al = _aligner(pkg, way, Rh)
    try:
        al.setSequences(s0, s1)
        for mode in ec.MODES:
            mg, st = edge_run(pkg, al, m, n, 4, mode)
            _in_twin(st, way, pc.strip_name(Rh, False, False, True, True, edge=True), 128 * Rh)
            check_pruned_run(mg, st, ref, m, n, mode, where="wide, %d-row strips" % (128 * Rh))
    finally:
        al.close()
