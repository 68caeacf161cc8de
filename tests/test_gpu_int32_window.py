"""GPU (-m gpu): the pruning window of the int32 kernel family -- MI355SW_F_INT32_WINDOW, opt-in; csrc/sw_kernel.hip,
process_strip<R, SW, PROFILE, TRACK, true, GOAL, EDGE, true>: a strip reads from its predecessor's last progress word where that
row turns into the skip constant, its trailing chunks go through the slab test, and it retires behind the alignment.

The oracle of every pruned run is the UNPRUNED one (helpers.oracle_full and the references of the files below), with the suite's
own criteria, imported and not restated: helpers.assert_pruned_borders for the local and the last-cell rule,
edge_prune_cases.assert_edge_pruned_borders / edge_optimum for the edge rule, _check_sweep of tests/test_gpu_goal_prune.py for goal
bounds.  The window changes what is WRITTEN, not what is skipped: every windowed run stands next to the same run under
MI355SW_F_NO_WINDOW and with the flag off.  Pairs, shapes and the census: tests/int32_window_cases.py."""
import time

import numpy as np
import pytest

import edge_prune_cases as ec
import int32_window_cases as cases
import test_gpu_int32_edge_goal as eg
from helpers import assert_pruned_borders, assert_pruned_cells, manager_rows, oracle_full
from test_gpu_bound import _stream
from test_gpu_edge_prune import unpruned
from test_gpu_goal_prune import _check_sweep, _reference

pytestmark = pytest.mark.gpu
INF = cases.INF
F_FORCE_INT32, F_NO_WINDOW = cases.F_FORCE_INT32, cases.F_NO_WINDOW
NW, SW = 0, 1
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _flags(pkg, rule):
    """the new flag next to the flag of the rule it acts under"""
    e = pkg.engine
    own = 0 if rule in cases.LOCAL_KINDS or rule == "local" else (e.F_INT32_PRUNE_GLOBAL if rule == "last_cell" else e.F_INT32_PRUNE_EDGE_GOAL)
    return e.F_INT32_WINDOW | own


def _is(st, rule, windowed):
    assert st["profile_kernel"] in (0, 1), st
    R = st["strip_rows"] // 64
    name = (cases.kernel_name if windowed else cases.walking_name)(R, rule, st["profile_kernel"] == 1)
    assert st["kernel"] == name, (st["kernel"], name)
    return True


def _not_below_minus_inf(*arrays):
    for a in arrays:
        if a is not None:
            assert int(np.asarray(a).min()) >= -INF, int(np.asarray(a).min())


def _reference_of(oracle, rule, key, s0, s1, R):
    if rule in cases.LOCAL_KINDS or rule == "local":
        return _once(("local",) + key, lambda: oracle_full(oracle, s0, s1))
    if rule == "last_cell":
        return _once(("last_cell",) + key, lambda: oracle_full(oracle, s0, s1, edge=4))
    if rule == "goal":
        return _once(("goal", R) + key, lambda: _reference(oracle, s0, s1, 64 * R, 8192))
    return unpruned(oracle, ("int32_window",) + key, s0, s1, 4)


def _bound_of(rule, ref):
    if rule in cases.LOCAL_KINDS or rule == "local":
        return int(ref["best"][2])
    if rule == "last_cell":
        return int(ref["last_row"][-1, 0])
    if rule == "goal":
        return int(ref["last_col"][:, 0].max()) - cases.GOAL_SLACK
    return ec.edge_optimum(rule, ref["last_row"], ref["last_col"])


def _run(pkg, al, rule, m, n, bound):
    """one run of the rule over the whole matrix from its bound; everything it handed out, in the form its criterion takes"""
    if rule in cases.LOCAL_KINDS or rule == "local":
        return _stream(pkg, al, m, n, SW, bound)
    if rule == "last_cell":
        return _stream(pkg, al, m, n, NW, bound)
    if rule == "goal":
        mg, st = eg._goal_run(pkg, al, m, n, bound)
        return {"mg": mg, "stats": st, "last_row": mg.lastRow()[1:], "last_col": mg.lastColumn()[1:]}
    return eg._stream(pkg, al, pkg.Partition(0, 0, m, n), rule, bound, edge_best=rule)


def _check(out, rule, ref, m, n, bound, where):
    """the rule's own criterion on every cell handed out; nothing below -INF; the books balance"""
    st = out["stats"]
    assert st["pruned_cells"] + st["processed_cells"] == m * n and st["restarts"] == 0, (where, st)
    if rule in cases.LOCAL_KINDS or rule == "local":
        assert out["best"] == tuple(ref["best"]), (where, out["best"], ref["best"])
        n_must = assert_pruned_borders(out["rows"], out["last_row"], out["last_col"], ref, m, n, bound, SW, col0=False,
                                       must_rows_upto=ref["best"][0], where=where)
        # (on the last row and the last column of a local run nothing can still reach the best: with no special row that the optimal
        #  path crosses there is no value the run owes exactly, and the criterion is the lower bound alone)
        assert n_must > 0 or not any(i <= ref["best"][0] for i in out["rows"]), where
        assert int(out["last_row"][:, 0].min()) >= 0 and int(out["last_col"][:, 0].min()) >= 0
    elif rule == "last_cell":
        assert int(out["last_row"][-1, 0]) == bound == int(out["last_col"][-1, 0]), where
        assert assert_pruned_borders(out["rows"], out["last_row"], out["last_col"], ref, m, n, bound, NW, col0=False, must_rows_upto=m, where=where) > 0
        _not_below_minus_inf(out["last_row"], out["last_col"], *out["rows"].values())
    elif rule == "goal":
        mg = out["mg"]
        _check_sweep(mg, ref, m, n, bound, where)
        _not_below_minus_inf(mg.lastRow(), mg.lastColumn(), *[mg.specialRow(i) for i in mg.special_rows])
    else:
        assert eg._check_stream(out, ref, m, n, rule, where) == bound and out["edge_best"][2] == bound


def _three_runs(pkg, oracle, rule, s0, s1, key, R, waves=None, base=F_FORCE_INT32):
    """window on, window on under MI355SW_F_NO_WINDOW, flag off: each holds the criterion; returns the three statistics"""
    m, n = len(s0), len(s1)
    ref = _reference_of(oracle, rule, key, s0, s1, R)
    bound = _bound_of(rule, ref)
    kw = {} if waves is None else {"waves": waves}
    res = {}
    for name, flags in (("window", _flags(pkg, rule)), ("no_window", _flags(pkg, rule) | F_NO_WINDOW), ("off", _flags(pkg, rule) & ~pkg.engine.F_INT32_WINDOW)):
        al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=base | flags, **kw)
        try:
            al.setSequences(s0, s1)
            out = _run(pkg, al, rule, m, n, bound)
        finally:
            al.close()
        assert _is(out["stats"], rule, name == "window") and out["stats"]["strip_rows"] == 64 * R
        _check(out, rule, ref, m, n, bound, "%s %s R %d %s" % (rule, key, R, name))
        res[name] = out
    p = [res[k]["stats"]["pruned_cells"] for k in ("window", "no_window", "off")]
    print("%s %s %d x %d, %d-row strips: pruned cells window %d, MI355SW_F_NO_WINDOW %d, flag off %d; kernel ms %.2f / %.2f / %.2f" % (
        rule, key, m, n, 64 * R, p[0], p[1], p[2], *[res[k]["stats"]["kernel_ms"] for k in ("window", "no_window", "off")]))
    assert max(p) - min(p) <= cases.CLOSE * m * n, p
    return res


# ---- 1. retire, local ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", cases.HEIGHTS)
@pytest.mark.parametrize("route", ["forced", "iupac"])
def test_strips_below_the_end_of_the_alignment_retire(pkg, oracle, route, R):
    """49 152 x 8192, the alignment ends at row 7682: 161 of 192 256-row strips lie below it.  With the flag, from the optimum and
    on one wavefront: the oracle's canonical best cell, the criterion on every row handed out, at least half the matrix skipped
    (the census leaves 0.73), the windowed kernel -- and every special row at or below row 16 384 and the last row read (0, -INF)
    over their last 63 columns: nobody walked there.  With the flag cleared on the same engine those columns hold a computed cell
    in every one of these rows (a walking strip computes its trailing chunk, whose cells carry a finite F)."""
    m, n = cases.RETIRE_M, cases.RETIRE_N
    s0, s1, flags = cases.retire_pair(pkg, route)
    ref = _once(("retire", route), lambda: oracle_full(oracle, s0, s1))
    if route == "forced":
        assert tuple(ref["best"]) == cases.RETIRE_BEST
        for i, row in zip(ref["special_row_ids"], ref["special_rows"]):
            assert i < cases.RETIRE_QUIET_FROM or int(row[:, 0].max()) <= cases.RETIRE_QUIET_H, i
    opt = int(ref["best"][2])
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags | pkg.engine.F_INT32_WINDOW, waves=1)
    try:
        al.setSequences(s0, s1)
        on = _stream(pkg, al, m, n, SW, opt)
        al.setFlag(pkg.engine.F_INT32_WINDOW, False)
        off = _stream(pkg, al, m, n, SW, opt)
    finally:
        al.close()
    for out, windowed in ((on, True), (off, False)):
        assert _is(out["stats"], "local", windowed) and out["stats"]["strip_rows"] == 64 * R
        _check(out, "local", ref, m, n, opt, "retire %s R %d window %s" % (route, R, windowed))
    st = on["stats"]
    print("%s, %d-row strips: %.3f of the matrix skipped with the window (%.3f without), kernel ms %.2f / %.2f" % (
        route, 64 * R, st["pruned_cells"] / float(m * n), off["stats"]["pruned_cells"] / float(m * n), st["kernel_ms"], off["stats"]["kernel_ms"]))
    assert st["pruned_cells"] >= cases.RETIRE_HALF * m * n
    deep = sorted(i for i in on["rows"] if i >= cases.RETIRE_ROWS_FROM)
    assert len(deep) >= 4 and deep == sorted(i for i in off["rows"] if i >= cases.RETIRE_ROWS_FROM)
    for where, a, b in [(i, on["rows"][i], off["rows"][i]) for i in deep] + [("last row", on["last_row"], off["last_row"])]:
        assert not a[-63:, 0].any() and np.all(a[-63:, 1] == -INF), where                   # retired: the constant the host filled in
        assert b[-63:, 0].any() or np.any(b[-63:, 1] != -INF), where                        # walked: a computed cell


# ---- 2. the window against the oracle and against the walk, every rule ---------------------------------------------------------------
@pytest.mark.parametrize("R", cases.HEIGHTS)
@pytest.mark.parametrize("rule", cases.RULES, ids=[str(r) for r in cases.RULES])
def test_every_rule_with_the_window_against_the_oracle_and_against_the_walk(pkg, oracle, rule, R):
    """24 000 x 20 000 (the last strip is ragged at every height), forced int32, the bound from the optimum: local from the
    corner, with a piece from the middle of seq0 and with a short homology and a long tail; the last cell; edge modes 1 to 3; goal
    with B = the largest last-column H - 200.  Each of the three runs holds its rule's criterion, nothing lies below -INF, and
    the three skip the same cells up to 5 % of the matrix.  pruned_cells > 0: from the optimum every rule skips here -- the
    sweep-grown bound, which is weaker, already did on this shape in tests/test_gpu_int32_prune_global.py (test 1) and
    tests/test_gpu_int32_edge_goal.py (tests 2 and 10); the local pairs leave whole corners that are out of the optimum's reach."""
    s0, s1 = cases.local_pair(pkg, rule if rule in cases.LOCAL_KINDS else "corner")
    res = _three_runs(pkg, oracle, rule, s0, s1, (rule if rule in cases.LOCAL_KINDS else "corner",), R)
    for name, out in res.items():
        assert out["stats"]["pruned_cells"] > 0, (rule, R, name)


# ---- 3. runs of skipped slabs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, None], ids=["one_wave", "default"])
@pytest.mark.parametrize("rule", ["local", "last_cell", 3, "goal"], ids=["local", "last_cell", "edge3", "goal"])
def test_runs_of_skipped_slabs(pkg, oracle, rule, waves):
    """16 384 x 16 384 related from the corner, 256-row strips: the triangle below the diagonal is a run of skipped slabs in every
    strip, and no strip is ragged.  The checks are test 2's.  How a run of skipped slabs is taken has no functional observable
    beyond "the same cells, the same counts": kernel_ms is printed for the window on and off, and no time is asserted."""
    s0, s1 = pkg.seqgen.related_pair(cases.M3, cases.N3, cfg=833)
    res = _three_runs(pkg, oracle, rule, s0, s1, ("square",), 4, waves=waves)
    assert res["window"]["stats"]["pruned_cells"] > 0
    if waves == 1:
        # (a function of the input: one wavefront, the bound fixed from the start -- the window skips exactly what the walk skips
        #  plus the trailing chunks of piece b, which the walk always computes)
        assert res["no_window"]["stats"]["pruned_cells"] == res["off"]["stats"]["pruned_cells"]
        assert res["window"]["stats"]["pruned_cells"] >= res["off"]["stats"]["pruned_cells"]


# ---- 4. ragged and narrow edges of the mechanism ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.EDGE_COLS)
@pytest.mark.parametrize("m", cases.EDGE_ROWS)
def test_ragged_rows_and_trailing_chunks_of_every_width(pkg, oracle, m, n):
    """m = 4096 + {1, 255, 256, 257}, n = 3072 + {0, 1, 63, 64, 65}, 256-row strips, local and last cell from the optimum on one
    wavefront.  Last row and last column hold the criterion cell by cell (helpers.assert_pruned_cells: the oracle's bytes wherever
    the rule could not have skipped the cell) -- a lane that has passed the last column keeps its cells when the trailing chunk
    is skipped.  A ragged strip never retires: its row, the last row, holds a computed cell in its last columns."""
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=840 + m % 5)
    for rule in ("local", "last_cell"):
        res = _three_runs(pkg, oracle, rule, s0, s1, ("edge", m, n), 4, waves=1)
        on = res["window"]
        assert on["stats"]["pruned_cells"] % (64 * 256) == 0
        if m % 256:
            tail = on["last_row"][-63:]
            assert np.any(tail[:, 1] != -INF) or (rule == "last_cell" and np.any(tail[:, 0] > -INF)), (rule, m, n)


# ---- 5. through the manager --------------------------------------------------------------------------------------------------------
def test_the_window_through_the_manager_on_a_pair_of_15_letters(pkg, oracle):
    """alignPartition with Stage1Manager(block_pruning=True, ...) on a 24 000 x 20 000 pair of 15 letters: the family is chosen by
    the alphabet, not forced, and the bound is the one the sweep grows.  The oracle's best cell, and the criterion."""
    m, n = cases.M2, cases.N2
    s0, s1 = cases.iupac_codes(*cases.local_pair(pkg, "corner"), 812)
    ref = _once(("manager",), lambda: oracle_full(oracle, s0, s1))
    al = pkg.MI355Aligner(device=0, flags=pkg.engine.F_INT32_WINDOW)
    try:
        al.setSequences(s0, s1)
        part = pkg.Partition(0, 0, m, n)
        mg = pkg.Stage1Manager(part, block_pruning=True, special_row_interval=8192, keep_last_row=True, keep_last_column=True)
        al.alignPartition(part, mg)
        st = al.getStatistics()
    finally:
        al.close()
    assert _is(st, "local", True), st["kernel"]
    assert tuple(mg.getBestScore()) == tuple(ref["best"])
    assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == m * n
    assert assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, ref["best"][2], SW, col0=True,
                                 must_rows_upto=ref["best"][0], where="manager") > 0


# ---- 6. the overflow rerun ---------------------------------------------------------------------------------------------------------
def test_the_overflow_rerun_runs_windowed(pkg, oracle):
    """a packed local pruning run that reports an overflow at strip 1 (injected, as tests/test_gpu_overflow.py does): one restart
    on the int32 family, which keeps the flag -- the windowed kernel -- and the result is test 2's"""
    m, n = cases.M2, cases.N2
    s0, s1 = cases.local_pair(pkg, "corner")
    ref = _reference_of(oracle, "corner", ("corner",), s0, s1, 4)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=pkg.engine.F_INT32_WINDOW, waves=1)
    try:
        al.setSequences(s0, s1)
        al.configure(fault_overflow_strip_plus1=2)
        part = pkg.Partition(0, 0, m, n)
        mg = pkg.Stage1Manager(part, block_pruning=True, special_row_interval=8192, keep_last_row=True, keep_last_column=True)
        al.alignPartition(part, mg)
        st = al.getStatistics()
    finally:
        al.close()
    assert st["restarts"] == 1 and _is(st, "local", True), (st["restarts"], st["kernel"])
    assert tuple(mg.getBestScore()) == tuple(ref["best"])
    # (what the packed attempt handed out before its report came from a pruning run as well: the criterion either way)
    assert assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, ref["best"][2], SW, col0=True,
                                 must_rows_upto=ref["best"][0], where="rerun") > 0
    assert st["pruned_cells"] > 0


# ---- 7. a two-band chain on one GPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["local", "last_cell"])
def test_two_bands_of_a_chain_are_windowed_each_on_its_own(pkg, oracle, rule):
    """12 000 x 10 000, two column bands in one process (mi355sw_port_attach, share_best), both forced onto the int32 family with
    the flag, the bound from the optimum in both: the chain's result is the single partition's (the oracle's), the boundary column
    and each band's slice of the last row hold the criterion in whole-matrix coordinates"""
    from masa_cudalign_amd.bands import band_limits, canonical_best
    m, n = 12000, 10000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=861)
    sw = rule == "local"
    rec = SW if sw else NW
    ref = _once(("chain", rule), lambda: oracle_full(oracle, s0, s1, edge=0 if sw else 4, special_row_interval=0))
    goal = _bound_of(rule, ref)
    lim = band_limits(n, [1, 1])
    seam = _once(("seam", rule), lambda: oracle_full(oracle, s0, s1[:lim[1]], edge=0 if sw else 4, special_row_interval=0))["last_col"]
    a0, a1 = (pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flags(pkg, rule)) for _ in range(2))
    outs, bests = [], []
    try:
        for al in (a0, a1):
            al.setSequences(s0, s1)
        a1.portCreate(m)
        a0.portAttach(a1)
        for k, al in enumerate((a0, a1)):
            kw = dict(prune_blocks=True, prune_rows=m, prune_cols=n - lim[k], share_best=True, last_column_port=(k == 0), want_last_row=True,
                      want_last_column=(k == 1), first_row_start_offset=lim[k], initial_bound=goal)
            if not sw:
                kw.update(recurrence_type=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=pkg.INIT_WITH_GAPS, first_column_init_type=pkg.INIT_WITH_GAPS, track_best=False)
            if k == 1:
                kw.update(first_column_init_type=pkg.INIT_WITH_CUSTOM_DATA, first_column_port=True, first_column=[[0 if sw else -2 * lim[1] - 3, -INF]])
            al.streamBegin(pkg.Partition(0, lim[k], m, lim[k + 1]), **kw)
            while not al.streamPoll()[1]:
                time.sleep(0.001)
            out = {"last_row": al.streamReadLastRow(), "last_col": al.streamReadColumn(0, m) if k == 1 else None}
            best, _ = al.streamEnd()
            out["stats"] = al.getStatistics()
            outs.append(out)
            bests.append(best)
            assert _is(out["stats"], rule, True), out["stats"]["kernel"]
            assert out["stats"]["pruned_cells"] + out["stats"]["processed_cells"] == m * (lim[k + 1] - lim[k])
        boundary = a1.portRead(0, m)
    finally:
        a0.close()
        a1.close()
    if sw:
        best = canonical_best(bests)
        assert (best[0] + 1, best[1] + 1, best[2]) == tuple(ref["best"])
    else:
        assert int(outs[1]["last_row"][-1, 0]) == goal
    rows = np.arange(1, m + 1)
    assert assert_pruned_cells(boundary, seam[1:], rows, lim[1], m, n, goal, rec, where="boundary column")[0] > 0
    for k in (0, 1):
        cols = np.arange(lim[k] + 1, lim[k + 1] + 1)
        assert_pruned_cells(outs[k]["last_row"], ref["last_row"][cols], m, cols, m, n, goal, rec, where="band %d last row" % k)
    assert_pruned_cells(outs[1]["last_col"], ref["last_col"][1:], rows, n, m, n, goal, rec, where="band 1 last column")
    _not_below_minus_inf(boundary, outs[0]["last_row"], outs[1]["last_row"], outs[1]["last_col"])
    print("%s: bands skipped %d and %d cells" % (rule, outs[0]["stats"]["pruned_cells"], outs[1]["stats"]["pruned_cells"]))
    assert outs[0]["stats"]["pruned_cells"] + outs[1]["stats"]["pruned_cells"] > 0


# ---- 8. flag off on the same engine, and what is not served --------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["local", "last_cell"])
def test_flag_off_is_the_run_under_no_window(pkg, oracle, rule):
    """on one engine, one wavefront, the bound from the optimum: the flag cleared and the flag with MI355SW_F_NO_WINDOW give the
    same pruned_cells, the same (walking) kernel and the same bytes of the last row and the last column"""
    m, n = 4096 + 255, 3072 + 65
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=840 + m % 5)
    ref = _reference_of(oracle, rule, ("edge", m, n), s0, s1, 4)
    bound = _bound_of(rule, ref)
    win = pkg.engine.F_INT32_WINDOW
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flags(pkg, rule), waves=1)
    try:
        al.setSequences(s0, s1)
        al.setFlag(win, False)
        off = _run(pkg, al, rule, m, n, bound)
        al.setFlag(win, True)
        al.setFlag(F_NO_WINDOW, True)
        nowin = _run(pkg, al, rule, m, n, bound)
        al.setFlag(F_NO_WINDOW, False)
        on = _run(pkg, al, rule, m, n, bound)
    finally:
        al.close()
    assert _is(off["stats"], rule, False) and _is(nowin["stats"], rule, False) and _is(on["stats"], rule, True)
    assert off["stats"]["pruned_cells"] == nowin["stats"]["pruned_cells"] > 0
    assert off["last_row"].tobytes() == nowin["last_row"].tobytes() and off["last_col"].tobytes() == nowin["last_col"].tobytes()
    _check(on, rule, ref, m, n, bound, "flag back on")


def test_what_the_window_does_not_serve(pkg, oracle):
    """reproducible pruning and block scores keep the walk: the walking kernel's name, the criterion as before"""
    m, n = 4096 + 255, 3072 + 65
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=840 + m % 5)
    ref = _reference_of(oracle, "local", ("edge", m, n), s0, s1, 4)
    bound = _bound_of("local", ref)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | pkg.engine.F_INT32_WINDOW | cases.F_DET, waves=1)
    try:
        al.setSequences(s0, s1)
        out = _run(pkg, al, "local", m, n, bound)
        assert _is(out["stats"], "local", False)
        _check(out, "local", ref, m, n, bound, "deterministic")
        al.setFlag(cases.F_DET, False)
        al.configure(block_score_columns=1024)
        out = _run(pkg, al, "local", m, n, bound)
        assert _is(out["stats"], "local", False)
        _check(out, "local", ref, m, n, bound, "block_score_columns")
    finally:
        al.close()
