"""GPU: the int32 kernel family (csrc/sw_kernel.hip: sw_strip_kernel<R, SW, PROFILE, TRACK[, PRUNE]>, R in {4, 8, 16}) held to the
oracle at every one of its 30 instantiations.  It runs every pair with 15 or more common byte values, every rerun after
MI355SW_EOVERFLOW16 and whatever MI355SW_F_FORCE_INT32 / MI355SW_F_FORCE_GENERIC_COMPARE send there, and it is the reference other
tests hold the packed kernels to.  Inputs and shape lists: tests/int32_cases.py (shown to be what they claim by
tests/test_int32_case_inputs.py on the CPU).  Integer work: every comparison is bit-exact -- the best cell, the last row, the last
column and, where rows are kept, every special row, delivered once.  One aligner per (way, R), many small partitions per test."""
import numpy as np
import pytest

import int32_cases as ic
from helpers import assert_pruned_borders, manager_rows

pytestmark = pytest.mark.gpu


def _aligner(pkg, way, R, **kw):
    return pkg.MI355Aligner(device=0, rows_per_lane=R, flags=ic.flags(way), **kw)


def _in_family(st, way, kernel=None, rows=None):
    assert st["profile_kernel"] == ic.WAYS[way][2], (st["profile_kernel"], way)
    if kernel is None:
        assert st["kernel"].startswith("sw_strip_kernel<"), st["kernel"]
    else:
        assert st["kernel"] == kernel, (st["kernel"], kernel)
    if rows is not None:
        assert st["strip_rows"] == rows, (st["strip_rows"], rows)
    assert st["restarts"] == 0


def _run(pkg, oracle, al, way, s0, s1, cases, kernel=None, rows=None, block_h=None):
    """every case through alignPartition on the aligner (its sequences set) and against the oracle in full"""
    for c in cases:
        mg = c.manager(pkg)
        al.alignPartition(pkg.Partition(*c.box), mg)
        st = al.getStatistics()
        name = kernel(c) if callable(kernel) else kernel
        _in_family(st, way, name, rows)
        ref = c.oracle(pkg, oracle, s0, s1, block_h or st["strip_rows"])
        ic.expect_oracle(pkg, c, mg, ref, (way, c.box, c.start, c.end, c.quiet, st["kernel"]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. every instantiation, by name
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,sw,profile,track,way", ic.instantiation_grid(),
                         ids=["%d-%s-%s-%s" % (g[0], "sw" if g[1] else "nw", g[4], "track" if g[3] else "quiet") for g in ic.instantiation_grid()])
def test_every_instantiation_by_name(pkg, oracle, R, sw, profile, track, way):
    """the 24 unpruned instantiations, each on every row count of int32_cases.row_counts(R) (1 ... about five strips: every emit
    lane and emit row of a ragged last strip) times every column count (1 ... 300: first chunk masked, last chunk masked, every
    step of the chunk count), on `iid` letters and with foreign bytes facing each other.  TRACK = false: NW to the last cell,
    and SW through a manager that refuses scores.  TRACK = true for NW: global start, best anywhere."""
    start, end = (0, 0) if sw else ((4, 0) if track else (4, 4))
    name = ic.kernel_name(R, sw, profile, track)
    al = _aligner(pkg, way, R)
    try:
        for kind in ("iid", "foreign"):
            g = ic.GridPair(way, ic.row_counts(R), kind=kind, seed=R)
            al.setSequences(g.s0, g.s1)
            _run(pkg, oracle, al, way, g.s0, g.s1, [ic.Part(b, start, end, quiet=sw and not track) for b in g.boxes()], name, 64 * R)
    finally:
        al.close()


@pytest.mark.parametrize("asked,lands", [(12, 8), (24, 16), (32, 16)])
def test_heights_outside_the_family_land_on_it(pkg, oracle, asked, lands):
    """rows_per_lane 12, 24 and 32 are heights of the packed kernels only: the int32 family runs them at 8, 16 and 16"""
    for way in ("profile", "raw15"):
        g = ic.GridPair(way, ic.EDGE_ROWS(lands), ic.EDGE_COLS, seed=asked)
        al = _aligner(pkg, way, asked)
        try:
            al.setSequences(g.s0, g.s1)
            _run(pkg, oracle, al, way, g.s0, g.s1, [ic.Part(b) for b in g.boxes()], ic.kernel_name(lands, True, way == "profile", True), 64 * lands)
        finally:
            al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. edge forms, custom borders, partitions at an offset, processBlock
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ic.HEIGHTS)
@pytest.mark.parametrize("way", list(ic.WAYS))
def test_edge_forms_and_custom_borders_at_an_offset(pkg, oracle, way, R):
    """every partition sits at (i0, j0) != (0, 0) inside longer sequences (seq0 + i0 and the code shift both in play).  The
    engine's own borders for all seven edge forms; then custom first rows and first columns -- a corner of its own, values near
    +-120 000 000, gap components that decide the first E / F, -INF in a tenth of them -- for NW to the last cell, NW with the best
    anywhere (far below zero: rows past the end of a ragged strip hold more than any real cell), a goal sweep (last column
    only), and SW with and without scores"""
    g = ic.GridPair(way, ic.EDGE_ROWS(R), ic.EDGE_COLS, seed=20 + R)
    cases = [ic.Part(b, s, e) for s, e in ic.EDGE_FORMS for b in g.boxes()]
    forms = [(4, 4, False, ic.OFFSET), (4, 0, False, -ic.OFFSET), (4, 2, False, -1234), (0, 0, False, None), (0, 0, True, None)]
    for k, b in enumerate(g.boxes()):
        for f, (s, e, quiet, corner) in enumerate(forms):
            row, col = ic.custom_borders(b[2] - b[0], b[3] - b[1], corner or 0, 100 * k + f, local=corner is None)
            cases.append(ic.Part(b, s, e, quiet=quiet, row=row, col=col))
    profile = ic.WAYS[way][3]
    al = _aligner(pkg, way, R)
    try:
        al.setSequences(g.s0, g.s1)
        _run(pkg, oracle, al, way, g.s0, g.s1, cases, lambda c: ic.kernel_name(R, c.sw(), profile, c.tracked()), 64 * R)
    finally:
        al.close()


@pytest.mark.parametrize("R", ic.HEIGHTS)
@pytest.mark.parametrize("way", list(ic.WAYS))
def test_process_block_on_the_int32_family(pkg, oracle, way, R):
    """AbstractBlockProcessor::processBlock (S3) as test_gpu_parity.py::test_process_block_seam runs it on the packed kernel: random
    borders with -INF entries, SW and NW, blocks at an offset, one row high, eight columns wide -- and NW once more with the borders
    120 000 000 down: every real cell then lies far under what the rows past the end of a ragged strip hold, and the best cell this
    call reports passes no manager's minimum score"""
    rng = np.random.default_rng(11 + R)
    s0, s1 = ic.related_pair(way, 3000, 3000, 81)
    s0, s1 = ic.with_alphabet(way, s0, s1)
    al = _aligner(pkg, way, R)
    try:
        al.setSequences(s0, s1)
        for rec, deep in ((pkg.SMITH_WATERMAN, 0), (pkg.NEEDLEMAN_WUNSCH, 0), (pkg.NEEDLEMAN_WUNSCH, -ic.OFFSET)):
            for (i0, j0, i1, j1) in [(0, 0, 700, 900), (100, 250, 1124, 314), (1000, 1000, 1001, 2500), (5, 7, 1500, 8)]:
                m, n = i1 - i0, j1 - j0
                row = np.stack([deep + rng.integers(0, 50, n), deep + rng.integers(-60, 40, n)], axis=1).astype(np.int32)
                col = np.stack([deep + rng.integers(0, 50, m + 1), deep + rng.integers(-60, 40, m + 1)], axis=1).astype(np.int32)
                row[rng.integers(0, n, max(1, n // 10)), 1] = -pkg.INF
                col[1 + rng.integers(0, m, max(1, m // 10)), 1] = -pkg.INF
                r1, c1 = row.copy(), col.copy()
                b1 = oracle.process_block(s0, s1, r1, c1, i0, j0, i1, j1, rec)
                r2, c2 = row.copy(), col.copy()
                b2 = al.processBlock(r2, c2, i0, j0, i1, j1, rec)
                _in_family(al.getStatistics(), way, ic.kernel_name(R, rec == pkg.SMITH_WATERMAN, ic.WAYS[way][3], True), 64 * R)
                assert np.array_equal(r1, r2) and np.array_equal(c1, c2), (way, R, rec, deep, i0, j0)
                assert tuple(b1) == tuple(b2), (b1, b2, way, R, rec, deep, i0, j0)
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. special rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_per_lane", [4, 8, 16, 0])
@pytest.mark.parametrize("way", list(ic.WAYS))
def test_special_rows_at_the_smallest_spacing(pkg, oracle, way, rows_per_lane):
    """8192 rows is the smallest spacing the runtime grants: 8192 rows give no special row, 8193 one, 16384 one (the row at m is
    not special), 16385 two -- with the strip height fixed (the rows on the strips' own grid) and engine-picked (the 2048-row
    unit), SW and NW, 193 columns, the partition at an offset"""
    n = 193
    s0, s1 = ic.with_alphabet(way, *ic.related_pair(way, 16385 + 3, n + 5, 33))
    want = {8192: [], 8193: [8192], 16384: [8192], 16385: [8192, 16384]}
    al = _aligner(pkg, way, rows_per_lane)
    try:
        al.setSequences(s0, s1)
        for m in sorted(want):
            for start, end in ((0, 0), (4, 4)):
                c = ic.Part((3, 5, 3 + m, 5 + n), start, end, interval=8192)
                mg = c.manager(pkg)
                al.alignPartition(pkg.Partition(*c.box), mg)
                st = al.getStatistics()
                _in_family(st, way, rows=64 * rows_per_lane if rows_per_lane else None)
                assert sorted(ic.special_rows(c, mg)) == want[m], (m, sorted(ic.special_rows(c, mg)))
                ref = c.oracle(pkg, oracle, s0, s1, 64 * rows_per_lane if rows_per_lane else 2048, threads=16)
                ic.expect_oracle(pkg, c, mg, ref, (way, rows_per_lane, m, start))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 16])
@pytest.mark.parametrize("way", list(ic.WAYS) + ["packed"])
def test_low_complexity_pairs_keep_the_canonical_best(pkg, oracle, way, R):
    """periodic sequences, letters of one sequence only, the same best score in many strips, in many lanes of a strip and at
    several columns of a row (test_int32_case_inputs.py shows where): the best cell is the oracle's (min i, then min j), unpruned
    and with block pruning -- a periodic pair has co-optimal paths through every slab corner, what SW_PRUNE_MARGIN and
    SW32_PRUNE_MARGIN are there for; the pruned run's borders are held by assert_pruned_borders.  `packed`: the same pairs, with
    a further run of columns, on the default packed kernel."""
    packed = way == "packed"
    al = pkg.MI355Aligner(device=0, rows_per_lane=R) if packed else _aligner(pkg, way, R)
    try:
        for name in ic.LOW_NAMES:
            s0, s1 = ic.low_pair(name, "generic" if packed else way, three_columns=packed)
            m, n = len(s0), len(s1)
            if name != "P/P^k":
                assert m > 2 * 64 * R                           # at least three strips
            q0, q1 = (s0, s1) if packed else ic.with_alphabet(way, s0, s1)
            al.setSequences(q0, q1)
            c = ic.Part((0, 0, m, n))
            ref = c.oracle(pkg, oracle, q0, q1, 64 * R)
            for prune in (False, True):
                mg = c.manager(pkg, block_pruning=prune)
                al.alignPartition(pkg.Partition(*c.box), mg)
                st = al.getStatistics()
                if packed:
                    assert st["profile_kernel"] == 2 and st["strip_rows"] == 64 * R, st
                else:
                    _in_family(st, way, ic.kernel_name(R, True, ic.WAYS[way][3], True, prune), 64 * R)
                what = (way, R, name, prune, st["pruned_cells"])
                if not prune:
                    assert st["pruned_cells"] == 0
                    ic.expect_oracle(pkg, c, mg, ref, what)
                else:
                    assert st["pruned_cells"] + st["processed_cells"] == m * n, what
                    assert tuple(mg.getBestScore()) == tuple(ref["best"]), (mg.getBestScore(), ref["best"], what)
                    assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, ref["best"][2], oracle.SMITH_WATERMAN,
                                          col0=True, where=str(what))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the six pruning instantiations <R,true,profile,true,true>
# ---------------------------------------------------------------------------------------------------------------------
# Per R the smallest related pair (int32_cases.related_pair(way, m, m, 500 + R), m a multiple of the strip height) at which the
# oracle's own pruned run (pruning=True, blocks of 64 R rows x 64 columns: the kernel's slab) prunes at least a tenth of its
# blocks -- the same shape for the 7-letter and the 15-letter alphabet:
#   R = 4: 1280 x 1280, 17 of 100 blocks;  R = 8: 1024 x 1024, 4 of 32;  R = 16: 2048 x 2048, 9 of 64
# The engine at these shapes, one wavefront (both ways alike): 442 368 of 1 638 400 cells pruned, 98 304 of 1 048 576, 589 824 of
# 4 194 304 -- no shape had to be doubled.
PRUNE_SHAPES = {4: (1280, 17, 100), 8: (1024, 4, 32), 16: (2048, 9, 64)}


@pytest.mark.parametrize("R", ic.HEIGHTS)
@pytest.mark.parametrize("way", ["profile", "raw15"])
def test_pruning_instantiations_prune_and_keep_what_matters(pkg, oracle, way, R):
    """one wavefront (waves=1: strips one after the other, what is pruned is a function of the input): cells are pruned, pruned and
    processed cells add up to the matrix, the best cell is the oracle's and every border value that could still matter is exact.
    Should the engine prune nothing at the oracle's shape, the shape is doubled once; the assertion stays."""
    size, pruned, blocks = PRUNE_SHAPES[R]
    results = []
    al = _aligner(pkg, way, R, waves=1)
    try:
        for m in (size, 2 * size):
            s0, s1 = ic.related_pair(way, m, m, 500 + R)
            if m == size:
                o = oracle.stage1(s0, s1, pruning=True, block_h=64 * R, block_w=64)
                assert (o["blocks_pruned"], o["blocks_total"]) == (pruned, blocks) and 10 * pruned >= blocks
            q0, q1 = ic.with_alphabet(way, s0, s1)
            al.setSequences(q0, q1)
            c = ic.Part((0, 0, m, m))
            mg = c.manager(pkg, block_pruning=True)
            al.alignPartition(pkg.Partition(*c.box), mg)
            st = al.getStatistics()
            _in_family(st, way, ic.kernel_name(R, True, way == "profile", True, True), 64 * R)
            assert st["waves"] == 1
            results.append((m, st["pruned_cells"]))
            print("pruning %s R %d: %d x %d, %d cells pruned of %d" % (way, R, m, m, st["pruned_cells"], m * m))
            if st["pruned_cells"] > 0:
                break
        assert st["pruned_cells"] > 0, results
        assert st["pruned_cells"] + st["processed_cells"] == m * m
        ref = c.oracle(pkg, oracle, q0, q1, 64 * R)
        assert tuple(mg.getBestScore()) == tuple(ref["best"]), (mg.getBestScore(), ref["best"])
        # (no special row at these heights, and on the last row and column nothing can still exceed the best: they are held as
        #  lower bounds that never go under the local floor; a value that could matter would have to be exact)
        assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, m, ref["best"][2], oracle.SMITH_WATERMAN,
                              col0=True, where="%s R %d" % (way, R))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a stop between strips
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["profile", "raw15"])
def test_a_stop_between_strips_like_stage2_at_its_goal(pkg, oracle, way):
    """test_gpu_parity.py::test_stop_like_stage2_goal_found on this family, which has no stop inside a strip: NW from a
    crosspoint, custom borders, tall and narrow, last column dispatched, the manager says stop once its last column has passed
    row 20 000.  What was dispatched before the stop is the oracle's, no special row below the stop is handed over, and the
    first-column stream is read at most once"""
    R, m, n, stop_at = 4, 1000000, 300, 20000
    s0, s1 = ic.with_alphabet(way, *ic.related_pair(way, m + 9, n + 4, 91))
    row, col = ic.custom_borders(m, n, -777, 6)
    c = ic.Part((9, 4, 9 + m, 4 + n), 4, 2, interval=8192, row=row, col=col, stop_at=stop_at)
    al = _aligner(pkg, way, R)
    try:
        al.setSequences(s0, s1)
        mg = c.manager(pkg)
        al.alignPartition(pkg.Partition(*c.box), mg)
        st = al.getStatistics()
    finally:
        al.close()
    _in_family(st, way, ic.kernel_name(R, False, way == "profile", False), 64 * R)
    got = mg.lastColumn()                                    # the corner cell + the rows dispatched before the stop
    seen = len(got) - 1
    assert stop_at <= seen < m, seen                         # it did stop
    upto = min(m, seen + 64 * R)
    ref = c.oracle(pkg, oracle, s0, s1, 64 * R, rows=upto, threads=16)      # rows 0..seen depend on nothing below them
    assert np.array_equal(got, ref["last_col"][:seen + 1])
    want = dict(zip(ref["special_row_ids"], ref["special_rows"]))
    rows = ic.special_rows(c, mg)
    assert rows and all(r <= seen for r in rows), (sorted(rows), seen)
    for r, chunks in rows.items():
        assert np.array_equal(np.concatenate(chunks), want[r]), r
    ic.delivered_once(c, mg)
    assert mg.col_asked <= m + 1, mg.col_asked
    assert st["processed_cells"] < m * n
