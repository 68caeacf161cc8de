"""GPU: per-block scores (config.block_score_columns) -- what CUDAligner::getBlockScores +
AbstractDiagonalAligner::flushBlockScores hand to AlignerManager::dispatchScore(score, bx, by)
(X/CUDAligner.cpp:441-452, AbstractDiagonalAligner.cpp:392-403, AlignerManager.cpp:411-450; consumer: --dump-blocks).
The engine's grid is "strip x W columns"; every block's best cell must be the oracle's for the same grid."""
import numpy as np
import pytest

import block_score_cases as bc

pytestmark = pytest.mark.gpu


def _blocks(oracle, ref):
    return {k: (v[0] + 1, v[1] + 1, v[2]) if v[2] > -oracle.INF else None for k, v in ref["block_scores"].items()}


@pytest.mark.parametrize("kind,m,n,R,W,flags", [
    ("related", 5000, 4321, 4, 700, 0),          # ragged last strip and last column block
    ("unrelated", 3000, 3100, 4, 512, 0),        # low scores: ties everywhere, the canonical cell must win in every block
    ("related", 9000, 7000, 8, 1000, 0),
    ("related", 5000, 4321, 4, 700, 2),          # int32 kernels
    ("semiglobal", 4000, 3500, 4, 600, 0),       # NW recurrence, gap-initialised borders, scores anywhere
])
def test_every_block_best_equals_the_oracles(pkg, oracle, kind, m, n, R, W, flags):
    if kind == "unrelated":
        s0, s1 = pkg.seqgen.unrelated_pair(m, n, cfg=51)
    else:
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=52)
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags, block_score_columns=W)
    try:
        assert al.getCapabilities()["dispatch_block_scores"] == 1
        al.setSequences(s0, s1)
        part = pkg.Partition(0, 0, m, n)
        if kind == "semiglobal":
            mg = pkg.Stage1Manager(part, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_ANYWHERE, keep_last_row=True)
            ref = oracle.stage1(s0, s1, recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=oracle.INIT_WITH_GAPS,
                                first_col_type=oracle.INIT_WITH_GAPS, block_h=64 * R, block_w=W, want_last_row=True)
        else:
            mg = pkg.Stage1Manager(part, keep_last_row=True)
            ref = oracle.stage1(s0, s1, block_h=64 * R, block_w=W, want_last_row=True)
        al.alignPartition(part, mg)
        st = al.getStatistics()
        al.unsetSequences()
    finally:
        al.close()
    assert st["strip_rows"] == 64 * R
    gh, gw = ref["grid"]
    assert (gh, gw) == (-(-m // (64 * R)), -(-n // W))
    want = _blocks(oracle, ref)
    got = {k: (v if v[2] > -pkg.INF else None) for k, v in mg.block_scores.items()}
    assert set(got) == set(want)
    bad = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not bad, bad[:5]
    # the main pass is untouched by the second sweep: best cell and last row as without block scores
    assert tuple(mg.getBestScore()) == tuple(ref["best"])
    assert np.array_equal(mg.lastRow(), ref["last_row"])


# ---------------------------------------------------------------------------------------------------------------------
# Every strip's record, block by block, at the edges of the kernels (tests/block_score_cases.py; the inputs are shown to be
# what they claim by tests/test_block_score_case_inputs.py)
# ---------------------------------------------------------------------------------------------------------------------
def run_blocks(pkg, case):
    """one block-score run of the case: (manager, statistics)"""
    s0, s1 = case.sequences()
    al = pkg.MI355Aligner(device=0, rows_per_lane=case.R, flags=case.flags, block_score_columns=case.W)
    try:
        if case.fault:
            al.configure(fault_overflow_strip_plus1=case.fault)
        al.setSequences(s0, s1)
        part = pkg.Partition(*case.box)
        mg = pkg.Stage1Manager(part, alignment_start=case.start, alignment_end=case.end, keep_last_row=True)
        al.alignPartition(part, mg)
        st = al.getStatistics()
        al.unsetSequences()
    finally:
        al.close()
    return mg, st


def expect_blocks(pkg, oracle, case, mg, ref, strip_rows):
    """grid shape, every block's (i, j, score), best cell and last row against the oracle's run on the partition's letters"""
    i0, j0 = case.origin
    gh, gw = ref["grid"]
    assert (gh, gw) == (-(-case.m // strip_rows), -(-case.n // case.W))
    want = {k: (v[0] + i0 + 1, v[1] + j0 + 1, v[2]) if v[2] > -oracle.INF else None for k, v in ref["block_scores"].items()}
    got = {k: (v if v[2] > -pkg.INF else None) for k, v in mg.block_scores.items()}
    assert set(got) == set(want), (sorted(set(got) ^ set(want))[:5], len(got), len(want))
    bad = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not bad, (len(bad), len(want), bad[:5])
    # the main pass is untouched by the second sweep: the best cell as a manager of the same kind keeps the oracle's, and the last row
    bi, bj, bs = ref["best"]
    keeper = pkg.Stage1Manager(pkg.Partition(*case.box), alignment_start=case.start, alignment_end=case.end)
    if bs > -oracle.INF:
        keeper.dispatchScore((i0 + bi - 1, j0 + bj - 1, bs))
    assert tuple(mg.getBestScore()) == tuple(keeper.getBestScore()), (mg.getBestScore(), ref["best"])
    if case.sw:
        assert tuple(mg.getBestScore()) == (i0 + bi, j0 + bj, bs)
    assert np.array_equal(mg.lastRow(), ref["last_row"])


@pytest.mark.parametrize("case", bc.grid_cases() + [bc.NEGATIVE] + bc.ONE_SIDED + bc.SLICED + bc.LO_HI, ids=repr)
def test_every_strip_record_of_every_band_is_the_oracles(pkg, oracle, case):
    """heights x row counts x band widths x tie pairs on every kernel route; the all-negative global grid (no block may come back
    as "no score"); one-sided starts; a partition inside longer sequences (coordinates compared after the shift); a tie between
    the LO and the HI rows of one lane in one step"""
    mg, st = run_blocks(pkg, case)
    if case.R == 0:
        assert st["strip_rows"] in (256, 512, 1024)                 # the engine's pick: a height both kernel families have
    else:
        assert st["strip_rows"] == 64 * case.R
    assert st["kernel"] == bc.kernel_name(case.route, st["strip_rows"] // 64, case.sw) and st["restarts"] == 0, (st["kernel"], st["restarts"])
    ref = case.reference(oracle, st["strip_rows"])
    if case is bc.NEGATIVE:
        scores = [v[2] for v in mg.block_scores.values()]
        assert len(scores) == 240 and max(scores) < 0 and min(scores) > -pkg.INF, (len(scores), min(scores), max(scores))
    expect_blocks(pkg, oracle, case, mg, ref, st["strip_rows"])


@pytest.mark.parametrize("case", bc.OVERFLOW, ids=repr)
def test_blocks_after_an_overflow_report_keep_their_grid(pkg, oracle, case):
    """an overflow report injected at strip 1 of every packed launch: the main pass and every band restart on the int32 family.
    The grid is the one the caller fixed -- at 768-, 1536- and 2048-row strips, which the int32 family does not have, the bands
    are rerun at 256 or 512 rows and their records merged into each block's -- and blocks, best cell and last row are the oracle's."""
    mg, st = run_blocks(pkg, case)
    assert st["restarts"] == 1 and st["kernel"] == bc.rerun_kernel_name(case.route, case.R, case.sw), (st["restarts"], st["kernel"])
    ref = case.reference(oracle)
    expect_blocks(pkg, oracle, case, mg, ref, 64 * case.R)


# ---------------------------------------------------------------------------------------------------------------------
# mi355sw_stream_strip_scores: what include/mi355sw.h promises of it
# ---------------------------------------------------------------------------------------------------------------------
def run_stream(pkg, s0, s1, m, n, R, waves, sw, flags=0, track=True, al=None):
    """one stream over the partition (0, 0, m, n) to its end: (best, records, statistics)"""
    own = al is None
    if own:
        al = pkg.MI355Aligner(device=0, rows_per_lane=R, waves=waves, flags=flags)
    try:
        al.setSequences(s0, s1)
        gaps = pkg.engine.INIT_WITH_ZEROES if sw else pkg.engine.INIT_WITH_GAPS
        al.streamBegin(pkg.Partition(0, 0, m, n), recurrence_type=pkg.engine.SMITH_WATERMAN if sw else pkg.engine.NEEDLEMAN_WUNSCH,
                       first_row_init_type=gaps, first_column_init_type=gaps, track_best=track)
        best, _ = al.streamEnd()
        st = al.getStatistics()
        rec = [tuple(int(x) for x in r) for r in al.streamStripScores()]
        one = [tuple(int(x) for x in r) for r in al.streamStripScores(max_count=1)]
        al.unsetSequences()
    finally:
        if own:
            al.close()
    return best, rec, one, st


def canonical(cells):
    """score desc, i asc, j asc over (i, j, score) cells"""
    return min(cells, key=lambda c: (-c[2], c[0], c[1]))


def true_score(oracle, s0, s1, i, j, sw):
    """H at the 0-based cell (i, j): the last cell of the oracle's run on the prefixes"""
    kw = {} if sw else dict(recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=oracle.INIT_WITH_GAPS, first_col_type=oracle.INIT_WITH_GAPS)
    return int(oracle.stage1(s0[:i + 1], s1[:j + 1], want_last_row=True, **kw)["last_row"][-1, 0])


def expect_records(oracle, s0, s1, sw, SH, rec, best, cells, ref):
    """what holds in every schedule: at most one record per strip in ascending order, each a true cell of its strip; their
    canonical maximum is the stream's best and the oracle's; every strip whose own best equals the global best has a record,
    and it is that strip's canonical cell"""
    strips = [r[0] // SH for r in rec]                              # (records: i, j, score)
    assert strips == sorted(set(strips)) and all(0 <= s < len(cells) for s in strips), strips
    for i, j, score in rec:
        assert 0 <= j < len(s1) and score == true_score(oracle, s0, s1, i, j, sw), (i, j, score)
    top = canonical(rec)
    assert tuple(best) == top
    assert (top[0] + 1, top[1] + 1, top[2]) == tuple(ref["best"])
    by_strip = {r[0] // SH: r for r in rec}
    for s, cell in enumerate(cells):
        if cell[2] == ref["best"][2]:
            assert by_strip.get(s) == tuple(cell), (s, by_strip.get(s), cell)


@pytest.mark.parametrize("route,R,waves,sw", bc.STRIP_RUNS, ids=lambda v: str(v))
def test_strip_scores_in_any_schedule(pkg, oracle, route, R, waves, sw):
    s0, s1 = bc.strip_pair(route, sw)
    m, n = bc.STRIP_M, bc.STRIP_N
    best, rec, one, st = run_stream(pkg, s0, s1, m, n, R, waves, sw, flags=bc.ROUTES[route][1])
    assert st["kernel"] == bc.kernel_name(route, R, sw) and st["strip_rows"] == 64 * R, st["kernel"]
    cells, ref = bc.strip_bests(oracle, s0[:m], s1[:n], 64 * R, sw)
    assert 1 <= len(rec) <= len(cells)
    expect_records(oracle, s0[:m], s1[:n], sw, 64 * R, rec, best, cells, ref)
    assert one == rec[:1]                                           # max_count is honoured: only the first is written
    if not bc.ROUTES[route][2]:                                     # the int32 kernels never seed a strip from the running best
        assert rec == [tuple(c) for c in cells]


_SERIAL = {}


def serial_reference(pkg, oracle):
    """the waves = 1 pair and its strips' canonical cells: computed once, shared, left unchanged"""
    if not _SERIAL:
        s0, s1 = pkg.seqgen.unrelated_pair(bc.SERIAL_M, bc.SERIAL_N, cfg=bc.SERIAL_CFG)
        _SERIAL["pair"] = (s0, s1)
        _SERIAL["ref"] = bc.strip_bests(oracle, s0, s1, 256)
    return _SERIAL["pair"], _SERIAL["ref"]


@pytest.mark.parametrize("route_flags", [0, bc.F_FORCE_INT32], ids=["packed", "int32"])
def test_strip_scores_of_the_serial_schedule(pkg, oracle, route_flags):
    """waves = 1: only the strips above can have written the running best before a strip looks at it, and a lane takes ties with
    it -- every strip whose best is at least the best of all strips above it holds exactly its canonical cell.  Strip bests
    9 9 9 11 8 9 10 10 10 10 10 9 9 9 11 8: strips 0 and 3 are strict maxima, strips 1, 2 and 14 tie.  (The absence of other
    records is not pinned.)"""
    (s0, s1), (cells, ref) = serial_reference(pkg, oracle)
    best, rec, one, st = run_stream(pkg, s0, s1, bc.SERIAL_M, bc.SERIAL_N, 4, 1, True, flags=route_flags)
    assert st["waves"] == 1 and st["strip_rows"] == 256
    expect_records(oracle, s0, s1, True, 256, rec, best, cells, ref)
    strict, tied = bc.prefix_maxima([c[2] for c in cells])
    assert strict == [0, 3] and tied == [1, 2, 14]
    by_strip = {r[0] // 256: r for r in rec}
    for s in strict + tied:
        assert by_strip.get(s) == tuple(cells[s]), (s, by_strip.get(s), cells[s])


@pytest.mark.parametrize("route", ["onehot", "wide15"])
def test_strip_scores_of_a_two_phase_run_are_the_one_best_cell(pkg, oracle, route):
    s0, s1 = bc.strip_pair(route, True)
    m, n = bc.STRIP_M, bc.STRIP_N
    best, rec, one, st = run_stream(pkg, s0, s1, m, n, 4, 0, True, flags=bc.ROUTES[route][1] | bc.F_TWO_PHASE)
    assert st["kernel_launches"] == 2                               # value-only main pass + the exact pass of the winning strip
    ref = oracle.stage1(s0[:m], s1[:n])
    bi, bj, bs = ref["best"]
    assert rec == [(bi - 1, bj - 1, bs)] and one == rec and tuple(best) == (bi - 1, bj - 1, bs)


@pytest.mark.parametrize("flags", [0, bc.F_FORCE_INT32], ids=["packed", "int32"])
def test_strip_scores_of_an_untracked_stream_are_none(pkg, flags):
    """track_best = 0 on an engine whose stream before it WAS tracked: no record of that stream is handed out again"""
    s0, s1 = bc.strip_pair("onehot", True)
    m, n = bc.STRIP_M, bc.STRIP_N
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=flags)
    try:
        best, rec, one, st = run_stream(pkg, s0, s1, m, n, 4, 0, True, al=al)
        assert len(rec) >= 1 and one == rec[:1]
        best, rec, one, st = run_stream(pkg, s0, s1, m, n, 4, 0, True, track=False, al=al)
        assert rec == [] and one == [] and tuple(best)[2] == -pkg.INF, (rec, best)
    finally:
        al.close()
