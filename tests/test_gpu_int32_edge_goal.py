"""GPU (-m gpu): the edge rule (mi355sw_set_prune_end) and goal bounds (mi355sw_set_goal_bounds) in the int32 kernel family --
MI355SW_F_INT32_PRUNE_EDGE_GOAL, opt-in; csrc/sw_kernel.hip, process_strip<R, false, PROFILE, false, true, GOAL, EDGE> -- on the
pairs the packed kernels cannot take (15 or more common byte values, 63 or more with MI355SW_F_WIDE_ALPHABET), under
MI355SW_F_FORCE_INT32 and on the rerun after an MI355SW_EOVERFLOW16 report.

The oracle of every pruned run is the UNPRUNED one (oracle.stage1, pruning off) with the suite's own criteria, imported and
not restated: edge_prune_cases.assert_edge_pruned_borders / edge_optimum for the edge rule, assert_goal_pruned / _check_sweep
of tests/test_gpu_goal_prune.py for goal bounds.  waves = 1 wherever a count is asserted: with a first bound equal to the
optimum (edge) or with constant bounds (goal), what is skipped is then a function of the input.  pruned_cells > 0 is demanded
only where tests/int32_edge_goal_cases.py's census allows it (a tenth of the eligible slabs may be skipped whole)."""
import hashlib
import time

import numpy as np
import pytest

import edge_prune_cases as ec
import int32_edge_goal_cases as cases
from helpers import load_golden, make_pair, manager_rows, oracle_kwargs
from test_gpu_edge_prune import check_result, edge_run, unpruned
from test_gpu_goal_prune import _bytes, _check_sweep, _manager, _reference

pytestmark = pytest.mark.gpu
F_FORCE_INT32, F_NO_WINDOW, F_DET, F_WIDE = 2, 1024, 16384, 65536
INF = 999999999
THREADS = 16
_CACHE = {}


def _flag(pkg):
    return pkg.engine.F_INT32_PRUNE_EDGE_GOAL


def _kernel(st, rule):
    """the int32 family's instantiation of the rule: "goal", an edge mode, or None for a kernel that prunes nothing"""
    k = st["kernel"]
    if not k.startswith("sw_strip_kernel<") or st["profile_kernel"] not in (0, 1):
        return False
    R = st["strip_rows"] // 64
    prof = "true" if st["profile_kernel"] == 1 else "false"
    tail = {None: "", "goal": ",true,true"}.get(rule, ",true,false,true")
    return k == "sw_strip_kernel<%d,false,%s,false%s>" % (R, prof, tail)


def _edge_ref(oracle, key, s0, s1, start=4):
    return unpruned(oracle, ("int32_edge_goal",) + tuple(key), s0, s1, start)


def _stream(pkg, al, part, mode, bound=None, edge_best=None, **over):
    """one global stream with the edge named (mode 0: not named) to its end"""
    if mode:
        al.setPruneEnd(mode)
    kw = dict(recurrence_type=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=pkg.INIT_WITH_GAPS, first_column_init_type=pkg.INIT_WITH_GAPS,
              track_best=False, prune_blocks=True, want_last_row=True, want_last_column=True, initial_bound=bound)
    kw.update(over)
    al.streamBegin(part, **kw)
    while not al.streamPoll()[1]:
        time.sleep(0.001)
    out = {"last_row": al.streamReadLastRow() if kw["want_last_row"] else None,
           "last_col": al.streamReadColumn(0, part.getHeight()) if kw["want_last_column"] else None}
    if edge_best:
        out["edge_best"] = al.streamEdgeBest(edge_best)
    al.streamEnd()
    out["stats"] = al.getStatistics()
    return out


def _no_value_below_minus_inf(*arrays):
    for a in arrays:
        if a is not None:
            assert int(np.asarray(a).min()) >= -INF, int(np.asarray(a).min())


def _check_stream(out, ref, m, n, mode, where):
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    assert ec.edge_optimum(mode, np.vstack([ref["last_row"][:1], out["last_row"]]), np.vstack([ref["last_col"][:1], out["last_col"]])) == opt, where
    assert ec.assert_edge_pruned_borders({}, out["last_row"], out["last_col"], ref, m, n, opt, mode, col0=False, where=where) > 0
    _no_value_below_minus_inf(out["last_row"], out["last_col"])
    return opt


# ---- 1. the edge rule: every route, every height, every mode ---------------------------------------------------------------
M1, N1 = 4096, 3072


@pytest.mark.parametrize("R", [4, 8, 16, 0])
@pytest.mark.parametrize("route", cases.ROUTES)
def test_edge_rule_on_every_route_and_height(pkg, oracle, route, R):
    """4096 x 3072 through the streaming form with initial_bound = the oracle's edge optimum, modes 1 to 3.  With the flag: the
    edge instantiation runs, cells are skipped, the books balance, result cell, last row and last column hold the criterion and
    nothing lies below -INF.  Without it, on the same engine: nothing is skipped and every byte is the oracle's."""
    s0, s1, flags = cases.pair(pkg, M1, N1, route)
    ref = _edge_ref(oracle, (route, M1, N1), s0, s1)
    part = pkg.Partition(0, 0, M1, N1)
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        for mode in ec.MODES:
            opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
            out = _stream(pkg, al, part, mode, opt, edge_best=mode)
            st = out["stats"]
            assert _kernel(st, mode), st["kernel"]
            assert R == 0 or st["strip_rows"] == 64 * R
            _check_stream(out, ref, M1, N1, mode, "%s R %d mode %d" % (route, R, mode))
            assert out["edge_best"][2] == opt
            assert st["pruned_cells"] + st["processed_cells"] == M1 * N1 and st["pruned_cells"] % (64 * st["strip_rows"]) == 0
            print("%s R %d mode %d: %d of %d eligible slabs skipped (%s)" % (route, R, mode, st["pruned_cells"] // (64 * st["strip_rows"]),
                                                                              (M1 // st["strip_rows"]) * (N1 // 64 - 2), st["kernel"]))
            if cases.worth_asserting(pkg, M1, N1, mode, st["strip_rows"] // 64, route):
                assert st["pruned_cells"] > 0, (route, R, mode)
        al.setFlag(_flag(pkg), False)
        for mode in ec.MODES:
            out = _stream(pkg, al, part, mode, ec.edge_optimum(mode, ref["last_row"], ref["last_col"]))
            assert out["stats"]["pruned_cells"] == 0 and _kernel(out["stats"], None), out["stats"]
            assert np.array_equal(out["last_row"], ref["last_row"][1:]) and np.array_equal(out["last_col"], ref["last_col"][1:])
    finally:
        al.close()


@pytest.mark.parametrize("mode", ec.MODES)
def test_ebound_is_held_against_the_best_of_the_named_edge(pkg, oracle, mode):
    """initial_bound = optimum + 1 is refused at the end of the stream (MI355SW_EBOUND) and the engine stays usable"""
    s0, s1, flags = cases.pair(pkg, M1, N1, "forced")
    ref = _edge_ref(oracle, ("forced", M1, N1), s0, s1)
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    part = pkg.Partition(0, 0, M1, N1)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=flags | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        with pytest.raises(pkg.AlignerError, match="EBOUND"):
            _stream(pkg, al, part, mode, opt + 1)
        out = _stream(pkg, al, part, mode, opt)
        assert _kernel(out["stats"], mode) and _check_stream(out, ref, M1, N1, mode, "after EBOUND") == opt
    finally:
        al.close()


# ---- 2. the bound the sweep grows ----------------------------------------------------------------------------------------------
M2, N2 = 24000, 20000


@pytest.mark.parametrize("start", [4, 3])
@pytest.mark.parametrize("R", [4, 8])
def test_edge_rule_with_the_bound_the_sweep_grows(pkg, oracle, R, start):
    """24 000 x 20 000 related pair, forced int32, through alignPartition with Stage1Manager(prune_edges=True), no first bound"""
    s0, s1 = pkg.seqgen.related_pair(M2, N2, cfg=812)
    ref = _edge_ref(oracle, ("grown", start), s0, s1, start)
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=F_FORCE_INT32 | _flag(pkg))
    try:
        al.setSequences(s0, s1)
        for mode in ec.MODES:
            mg, st = edge_run(pkg, al, M2, N2, start, mode)
            assert _kernel(st, mode) and st["strip_rows"] == 64 * R, st["kernel"]
            opt = check_result(mg, ref, M2, N2, mode)
            assert ec.assert_edge_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, M2, N2, opt, mode, col0=True, where="grown") > 0
            assert st["pruned_cells"] + st["processed_cells"] == M2 * N2
            print("start %d mode %d, %d-row strips: %.4f of the cells skipped with a sweep-grown bound" % (start, mode, 64 * R, st["pruned_cells"] / float(M2 * N2)))
            assert st["pruned_cells"] > 0, (start, mode, R)
    finally:
        al.close()


# ---- 3. the sign and span of the forced gap ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(9000, 24000), (24000, 9000), (8191, 8257), (8257, 8191)])
def test_the_forced_gap_has_the_right_sign_and_span_on_int32(pkg, oracle, m, n):
    """di - dj changes sign inside the matrix; shapes off the 64-column and strip grids (the pairs and the reference of
    tests/test_gpu_edge_prune.py::test_the_forced_gap_has_the_right_sign_and_span)"""
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9600 + m % 7)
    ref = unpruned(oracle, ("t2", m, n, 4), s0, s1, 4)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg))
    try:
        al.setSequences(s0, s1)
        for mode in ec.MODES:
            mg, st = edge_run(pkg, al, m, n, 4, mode)
            assert _kernel(st, mode), st["kernel"]
            opt = check_result(mg, ref, m, n, mode)
            assert ec.assert_edge_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, opt, mode, col0=True, where="gap") > 0
            assert st["pruned_cells"] + st["processed_cells"] == m * n
            print("%d x %d mode %d: %.4f of the cells skipped" % (m, n, mode, st["pruned_cells"] / float(m * n)))
    finally:
        al.close()


# ---- 4. structural edges -------------------------------------------------------------------------------------------------------
SH = 256


def _goal_run(pkg, al, m, n, cols, rows=None, interval=8192):
    part = pkg.Partition(0, 0, m, n)
    mg = _manager(pkg, part, interval)
    if cols is not None:
        al.setGoalBounds([cols], None if rows is None else [rows])
    al.alignPartition(part, mg)
    return mg, al.getStatistics()


@pytest.mark.parametrize("name", ["n191", "n192", "n193", "n255", "n256", "n257", "m-1", "m0", "m+1"])
def test_structural_edges(pkg, oracle, name):
    """the 2 CHUNK / col0 + CHUNK <= n eligibility edge (1024 rows) and m one row short of, equal to and one row over two
    256-row strips (1536 columns): each mode from its optimum and the goal rule, result and criterion; never more slabs than are
    eligible -- none where no slab is"""
    m, n = (1024, int(name[1:])) if name[0] == "n" else (2 * SH + {"m-1": -1, "m0": 0, "m+1": 1}[name], 1536)
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=881)
    ref = _edge_ref(oracle, ("edge", name), s0, s1)
    limit = (m // SH) * max(0, n // 64 - 2) * 64 * SH
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        for mode in ec.MODES:
            out = _stream(pkg, al, pkg.Partition(0, 0, m, n), mode, ec.edge_optimum(mode, ref["last_row"], ref["last_col"]))
            st = out["stats"]
            assert _kernel(st, mode), st["kernel"]
            _check_stream(out, ref, m, n, mode, "%s mode %d" % (name, mode))
            assert st["pruned_cells"] % (64 * SH) == 0 and st["pruned_cells"] <= limit and st["pruned_cells"] + st["processed_cells"] == m * n, (name, mode, st)
        gref = _reference(oracle, s0, s1, SH, 8192)
        bound = int(gref["last_col"][:, 0].max()) - cases.GOAL_SLACK
        mg, st = _goal_run(pkg, al, m, n, bound)
        assert _kernel(st, "goal"), st["kernel"]
        _check_sweep(mg, gref, m, n, bound, name)
        assert st["pruned_cells"] % (64 * SH) == 0 and st["pruned_cells"] <= limit and st["pruned_cells"] + st["processed_cells"] == m * n, (name, st)
        print("%s: %d x %d, goal rule %d of %d eligible slabs skipped" % (name, m, n, st["pruned_cells"] // (64 * SH), limit // (64 * SH)))
    finally:
        al.close()


# ---- 5. goal bounds ------------------------------------------------------------------------------------------------------------
GOAL_CASES = [(m, n, R) for (m, n) in [(2048, 1536), (2049, 1601), (8209, 4096), (16401, 1536)] for R in (4, 8)] + [(2048, 1536, 16)]


@pytest.mark.parametrize("route", cases.ROUTES)
@pytest.mark.parametrize("m,n,R", GOAL_CASES, ids=["%dx%d_R%d" % c for c in GOAL_CASES])
def test_one_goal_sweep_against_the_oracle(pkg, oracle, m, n, R, route):
    """test_gpu_goal_prune.py::test_one_goal_sweep_against_the_oracle on the int32 family, B = (largest H of the oracle's last
    column) - 200: the goal instantiation, _check_sweep, two runs alike, the bound consumed by its call, a row bound alone, both
    bounds off, and the flag off"""
    interval = 8192
    s0, s1, flags = cases.pair(pkg, m, n, route)
    if ("goal", route, m, n, R) not in _CACHE:
        _CACHE[("goal", route, m, n, R)] = _reference(oracle, s0, s1, 64 * R, interval)
    ref = _CACHE[("goal", route, m, n, R)]
    bound = int(ref["last_col"][:, 0].max()) - cases.GOAL_SLACK
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        runs = [_goal_run(pkg, al, m, n, bound) for _ in range(2)]
        mg, st = runs[0]
        assert _kernel(st, "goal"), st["kernel"]
        assert st["strip_rows"] == 64 * R and st["kernel_launches"] == 1 and st["restarts"] == 0
        assert len([i for i in mg.special_rows if i != m]) == (m - 1) // 8192
        differing = _check_sweep(mg, ref, m, n, bound, "%s %dx%d" % (route, m, n))
        _no_value_below_minus_inf(mg.lastRow(), mg.lastColumn(), *[mg.specialRow(i) for i in mg.special_rows])
        print("%s %d x %d, %d-row strips: bound %d, pruned %d of %d cells, %d handed-out values are lower bounds" % (
            route, m, n, st["strip_rows"], bound, st["pruned_cells"], m * n, differing))
        assert st["pruned_cells"] + st["processed_cells"] == m * n
        if (m, n) in cases.SHAPES and cases.worth_asserting(pkg, m, n, "goal", R, route):
            assert st["pruned_cells"] > 0
        assert _bytes(runs[0][0]) == _bytes(runs[1][0]) and runs[0][1]["pruned_cells"] == runs[1][1]["pruned_cells"]
        # the bound is consumed by the call it was set for: the next one computes every cell
        mg, st = _goal_run(pkg, al, m, n, None)
        assert st["pruned_cells"] == 0 and _kernel(st, None), st
        assert np.array_equal(mg.lastColumn(), ref["last_col"]) and np.array_equal(mg.lastRow(), ref["last_row"])
        # a row bound alone: the last row's criterion is the edge rule's for the last row, held against the bound
        rbound = int(ref["last_row"][:, 0].max()) - cases.GOAL_SLACK
        mg, st = _goal_run(pkg, al, m, n, -INF, rbound)
        assert _kernel(st, "goal") and st["pruned_cells"] + st["processed_cells"] == m * n, st
        assert ec.assert_edge_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, rbound, ec.ROW, col0=True, where="row bound") > 0
        must = ref["last_row"][:, 0] >= rbound
        assert must.any() and np.array_equal(mg.lastRow()[must, 0], ref["last_row"][must, 0])
        # both bounds off: nothing goes
        mg, st = _goal_run(pkg, al, m, n, -INF, -INF)
        assert st["pruned_cells"] == 0 and np.array_equal(mg.lastColumn(), ref["last_col"]) and np.array_equal(mg.lastRow(), ref["last_row"])
        al.setFlag(_flag(pkg), False)
        mg, st = _goal_run(pkg, al, m, n, bound)
        assert st["pruned_cells"] == 0 and _kernel(st, None), st
        assert np.array_equal(mg.lastColumn(), ref["last_col"]) and np.array_equal(mg.lastRow(), ref["last_row"])
        want = dict(zip(ref.get("special_row_ids") or [], ref["special_rows"] if ref.get("special_rows") is not None else []))
        for i in mg.special_rows:
            if i in want:
                assert np.array_equal(mg.specialRow(i), want[i]), i
    finally:
        al.close()


# ---- 6. goal bounds through alignPartitions --------------------------------------------------------------------------------------
def test_goal_bounds_through_align_partitions(pkg, oracle):
    """two stage-2-shaped partitions (4096 x 3072 blocks along the diagonal) of an IUPAC pair, each with its own bound: the pair
    is not batchable, so each runs on a launch of its own and is pruned there against its own bound"""
    from test_gpu_prune32 import _iupac_pair
    m, n = 4096, 3072
    s0, s1 = _iupac_pair(pkg, 2 * m, 2 * n, 891)
    parts = [pkg.Partition(k * m, k * n, (k + 1) * m, (k + 1) * n) for k in range(2)]
    refs = [_reference(oracle, s0[p.i0:p.i1], s1[p.j0:p.j1], 256, 0) for p in parts]
    bounds = [int(r["last_col"][:, 0].max()) - cases.GOAL_SLACK for r in refs]
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=_flag(pkg), waves=1)
    pruned = {}
    try:
        al.setSequences(s0, s1)
        for name, bs in (("first", [bounds[0], -INF]), ("second", [-INF, bounds[1]]), ("both", bounds)):
            mgs = [pkg.Stage1Manager(p, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_OR_2,
                                     keep_last_row=True, keep_last_column=True) for p in parts]
            al.setGoalBounds(bs)
            al.alignPartitions(parts, mgs)
            st = al.getStatistics()
            assert st["kernel"].startswith("sw_strip_kernel<") and st["pruned_cells"] + st["processed_cells"] == 2 * m * n, st
            for k in (0, 1):
                if bs[k] > -INF:
                    _check_sweep(mgs[k], refs[k], m, n, bs[k], "%s partition %d" % (name, k))
                else:
                    assert np.array_equal(mgs[k].lastColumn(), refs[k]["last_col"]) and np.array_equal(mgs[k].lastRow(), refs[k]["last_row"])
            pruned[name] = st["pruned_cells"]
    finally:
        al.close()
    print("pruned cells: first alone %d, second alone %d, both %d" % (pruned["first"], pruned["second"], pruned["both"]))
    assert pruned["both"] == pruned["first"] + pruned["second"]
    for k, name in enumerate(("first", "second")):
        if cases.worth(cases.gotoh_h(s0[parts[k].i0:parts[k].i1], s1[parts[k].j0:parts[k].j1]), "goal", 4):
            assert pruned[name] > 0, name


# ---- 7. overflow reruns -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["flag", "no_flag"])
def test_overflow_reruns_keep_the_edge_and_the_bounds(pkg, oracle, on):
    """an edge run and a goal sweep that start on the packed kernels and report an overflow at strip 1 (injected): one restart
    on the int32 family, which takes the request with the flag and computes every cell without it"""
    m, n = M1, N1
    s0, s1, _ = cases.pair(pkg, m, n, "forced")
    ref = _edge_ref(oracle, ("forced", m, n), s0, s1)
    gref = _reference(oracle, s0, s1, 256, 8192)
    bound = int(gref["last_col"][:, 0].max()) - cases.GOAL_SLACK
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=_flag(pkg) if on else 0, waves=1)
    try:
        al.setSequences(s0, s1)
        al.configure(fault_overflow_strip_plus1=2)
        mg, st = edge_run(pkg, al, m, n, 4, 3)
        assert st["restarts"] == 1 and _kernel(st, 3 if on else None), (st["restarts"], st["kernel"])
        opt = check_result(mg, ref, m, n, 3)
        assert ec.assert_edge_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, opt, 3, col0=True, where="rerun") > 0
        if not on:
            assert st["pruned_cells"] == 0
            assert np.array_equal(mg.lastRow(), ref["last_row"])          # (the last row is the rerun's alone: every cell computed)
        elif cases.worth_asserting(pkg, m, n, 3, 4):
            print("edge rerun: %d cells skipped" % st["pruned_cells"])
        mg, st = _goal_run(pkg, al, m, n, bound)
        assert st["restarts"] == 1 and _kernel(st, "goal" if on else None), (st["restarts"], st["kernel"])
        _check_sweep(mg, gref, m, n, bound, "goal rerun")
        if not on:
            assert st["pruned_cells"] == 0 and np.array_equal(mg.lastRow(), gref["last_row"])
        elif cases.worth_asserting(pkg, m, n, "goal", 4):
            assert st["pruned_cells"] > 0
    finally:
        al.close()


# ---- 8. a chain of two bands ---------------------------------------------------------------------------------------------------
def test_two_bands_of_a_chain_with_the_edge_named(pkg, oracle):
    """12 000 x 10 000, two column bands in one process (mi355sw_port_attach, share_best), both on the int32 family, mode 3,
    initial_bound = optimum in both: the chain's result from the bands' streamEdgeBest is the optimum, the boundary column and
    each band's slice of the last row hold the criterion in whole-matrix coordinates"""
    from masa_cudalign_amd.bands import band_limits
    m, n, mode = 12000, 10000, 3
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=861)
    ref = _edge_ref(oracle, ("chain",), s0, s1)
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    lim = band_limits(n, [1, 1])
    seam = _edge_ref(oracle, ("chain_seam",), s0, s1[:lim[1]])["last_col"]
    a0, a1 = (pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg)) for _ in range(2))
    try:
        for al in (a0, a1):
            al.setSequences(s0, s1)
        a1.portCreate(m)
        a0.portAttach(a1)
        outs = []
        for k, al in enumerate((a0, a1)):
            kw = dict(prune_rows=m, prune_cols=n - lim[k], share_best=True, last_column_port=(k == 0), want_last_column=(k == 1),
                      first_row_start_offset=lim[k])
            if k == 1:
                kw.update(first_column_init_type=pkg.INIT_WITH_CUSTOM_DATA, first_column_port=True, first_column=[[-2 * lim[1] - 3, -INF]])
            outs.append(_stream(pkg, al, pkg.Partition(0, lim[k], m, lim[k + 1]), mode, opt, edge_best=(1 if k == 0 else 3), **kw))
            assert _kernel(outs[k]["stats"], mode), outs[k]["stats"]["kernel"]
        boundary = a1.portRead(0, m)
    finally:
        a0.close()
        a1.close()
    assert max(o["edge_best"][2] for o in outs) == opt
    rows = np.arange(1, m + 1)
    assert ec.assert_edge_pruned_cells(boundary, seam[1:], rows, lim[1], m, n, opt, mode, where="boundary column")[0] > 0
    for k in (0, 1):
        cols = np.arange(lim[k] + 1, lim[k + 1] + 1)
        ec.assert_edge_pruned_cells(outs[k]["last_row"], ref["last_row"][cols], m, cols, m, n, opt, mode, where="band %d last row" % k)
        assert outs[k]["stats"]["pruned_cells"] + outs[k]["stats"]["processed_cells"] == m * (lim[k + 1] - lim[k])
    ec.assert_edge_pruned_cells(outs[1]["last_col"], ref["last_col"][1:], rows, n, m, n, opt, mode, where="band 1 last column")
    _no_value_below_minus_inf(boundary, outs[0]["last_row"], outs[1]["last_row"], outs[1]["last_col"])
    print("bands skipped %d and %d cells" % (outs[0]["stats"]["pruned_cells"], outs[1]["stats"]["pruned_cells"]))
    assert outs[0]["stats"]["pruned_cells"] + outs[1]["stats"]["pruned_cells"] > 0


# ---- 9. what is not served ------------------------------------------------------------------------------------------------------
def test_what_is_not_served(pkg, oracle):
    """with the new flag: a tracking manager, a local recurrence with an edge named and MI355SW_F_DETERMINISTIC_PRUNE compute
    every cell; with MI355SW_F_INT32_PRUNE_GLOBAL alone edge and goal requests stay unpruned; with the new flag alone a
    last-cell request does"""
    m, n = M1, N1
    s0, s1, _ = cases.pair(pkg, m, n, "forced")
    ref = _edge_ref(oracle, ("forced", m, n), s0, s1)
    gref = _reference(oracle, s0, s1, 256, 8192)
    bound = int(gref["last_col"][:, 0].max()) - cases.GOAL_SLACK

    def exact(mg, st, want):
        assert st["pruned_cells"] == 0 and st["processed_cells"] == m * n and _kernel(st, None), st
        assert np.array_equal(mg.lastRow(), want["last_row"]) and np.array_equal(mg.lastColumn(), want["last_col"])

    class Tracking(pkg.Stage1Manager):
        def mustDispatchScores(self):
            return True

    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        mg, st = edge_run(pkg, al, m, n, 4, 3, manager_class=Tracking)
        assert st["pruned_cells"] == 0 and st["kernel"] == "sw_strip_kernel<4,false,true,true>", st
        assert np.array_equal(mg.lastRow(), ref["last_row"]) and np.array_equal(mg.lastColumn(), ref["last_col"])
        kw = oracle_kwargs(oracle, dict(start=0, end=3, pruning=False, disk=-1, block=(1024, 1 << 20)), m, n)
        kw.update(want_last_row=True, want_last_col=True, threads=THREADS)
        ref_sw = oracle.stage1(s0, s1, **kw)
        part = pkg.Partition(0, 0, m, n)
        mg = pkg.Stage1Manager(part, alignment_start=pkg.AT_ANYWHERE, alignment_end=pkg.AT_SEQUENCE_1_OR_2, keep_last_row=True, keep_last_column=True)
        mg.block_pruning = True
        al.setPruneEnd(3)
        al.alignPartition(part, mg)
        st = al.getStatistics()
        assert st["pruned_cells"] == 0 and st["kernel"].startswith("sw_strip_kernel<4,true,"), st
        assert np.array_equal(mg.lastRow(), ref_sw["last_row"]) and np.array_equal(mg.lastColumn(), ref_sw["last_col"])
        al.setFlag(F_DET, True)
        for mode in ec.MODES:
            exact(*edge_run(pkg, al, m, n, 4, mode), ref)
        exact(*_goal_run(pkg, al, m, n, bound), gref)
        al.setFlag(F_DET, False)
        # the last-cell rule has a flag of its own
        mg = pkg.Stage1Manager(part, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_AND_2, keep_last_row=True,
                               keep_last_column=True, block_pruning=True)
        al.alignPartition(part, mg)
        exact(mg, al.getStatistics(), ref)
        al.setFlag(_flag(pkg), False)
        al.setFlag(pkg.engine.F_INT32_PRUNE_GLOBAL, True)
        for mode in ec.MODES:
            exact(*edge_run(pkg, al, m, n, 4, mode), ref)
        exact(*_goal_run(pkg, al, m, n, bound), gref)
    finally:
        al.close()


# ---- 10. how much ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [3, "goal"], ids=["edge3", "goal"])
def test_skips_at_least_half_of_what_the_packed_family_skips_slab_by_slab(pkg, oracle, rule):
    """the yardstick is the packed family under MI355SW_F_NO_WINDOW at the same strip height (512 rows) and on the same pair: the
    same rule, also slab by slab.  The factor 2 and its reason are those of tests/test_gpu_int32_prune_global.py: an int32 lane
    spans R = 8 rows where a packed lane spans 2 (its span makes both bounds weaker), and ragged and masked chunks are never
    skipped here.  Measured figures: CHANGELOG.md."""
    s0, s1 = pkg.seqgen.related_pair(M2, N2, cfg=812)
    res = {}
    for name, flags in (("int32", F_FORCE_INT32 | _flag(pkg)), ("packed", F_NO_WINDOW)):
        al = pkg.MI355Aligner(device=0, rows_per_lane=8, flags=flags, waves=1)
        try:
            al.setSequences(s0, s1)
            if rule == "goal":
                if "yard" not in _CACHE:
                    _CACHE["yard"] = int(_reference(oracle, s0, s1, 512, 0)["last_col"][:, 0].max()) - cases.GOAL_SLACK
                mg, st = _goal_run(pkg, al, M2, N2, _CACHE["yard"], interval=0)
            else:
                mg, st = edge_run(pkg, al, M2, N2, 4, rule)
            res[name] = (st["pruned_cells"], st["kernel"], st["strip_rows"], mg.getBestScore()[2])
        finally:
            al.close()
    print("rule %s, pruned cells of %d: int32 %d (%s), packed without window %d (%s): ratio %.3f" % (
        rule, M2 * N2, res["int32"][0], res["int32"][1], res["packed"][0], res["packed"][1], res["int32"][0] / float(max(1, res["packed"][0]))))
    assert res["int32"][2] == res["packed"][2] == 512 and res["int32"][3] == res["packed"][3]
    assert "pk16" in res["packed"][1] and res["packed"][0] > 0 and res["int32"][1].startswith("sw_strip_kernel<8,false,")
    assert res["int32"][0] >= 0.5 * res["packed"][0]


# ---- 11. the native pipeline -----------------------------------------------------------------------------------------------------
def test_the_pipeline_leaves_the_references_files_with_goal_pruning_on_int32(pkg, tmp_path):
    """the full-pipeline fixture of tests/test_gpu_goal_prune.py::_pipeline_case (global, 60 000 x 50 000) with
    MI355SW_F_FORCE_INT32 | MI355SW_F_INT32_PRUNE_EDGE_GOAL and prune_traceback=True: the reference's crosspoint and alignment
    files, and stage 2 skipped cells"""
    from masa_cudalign_amd import fasta, pipeline
    from masa_cudalign_amd.crosspoints import CrosspointsFile, crosspoint_file
    fixture = "full_pipeline_global_60000x50000_b8192"
    case = [c for c in load_golden()["cases"] if c["name"] == fixture][0]
    s0, s1 = make_pair(pkg, case["seq"])
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    work = str(tmp_path / "work")
    al = pkg.MI355Aligner(device=0, flags=F_FORCE_INT32 | _flag(pkg))
    try:
        out = pipeline.align(al, q0, q1, work, prune_traceback=True, sra_limit=4 * 1024 * 1024, block_pruning=False, alignment_start=4, alignment_end=4)
    finally:
        al.close()
    assert list(out["best"]) == case["best"]
    assert CrosspointsFile(crosspoint_file(work, 2)).load().tuples() == [tuple(p) for p in case["crosspoints_2"]]
    assert CrosspointsFile(crosspoint_file(work, 3)).load().tuples() == [tuple(p) for p in case["crosspoints_3"]]
    assert hashlib.sha256(open(crosspoint_file(work, 4), "rb").read()).hexdigest() == case["crosspoints_4"]["file_sha256"]
    assert hashlib.sha256(out["text"]).hexdigest() == case["alignment_txt_sha256"]
    sweeps = out["stage2"]["sweeps"]
    print("stage 2: pruned %d, processed %d cells; kernels %s" % (out["stage2"]["pruned_cells"], out["stage2"]["processed_cells"], sorted(set(c["kernel"] for c in sweeps))))
    assert out["stage2"]["pruned_cells"] > 0
    assert any(c["kernel"].startswith("sw_strip_kernel<") and c["kernel"].endswith(",false,true,true>") for c in sweeps)


def test_a_semi_global_pipeline_gives_the_same_alignment_with_and_without_the_flag(pkg, tmp_path):
    """pipeline.align(prune_edges=True) on a semi-global pair (+3), forced int32: alignment.00.txt with the flag is the one
    without it, and only the run with the flag skipped cells in stage 1"""
    from masa_cudalign_amd import fasta, pipeline
    m, n = 24000, 20000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9960)
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    texts = {}
    for on in (False, True):
        al = pkg.MI355Aligner(device=0, flags=F_FORCE_INT32 | (_flag(pkg) if on else 0))
        try:
            out = pipeline.align(al, q0, q1, str(tmp_path / ("on" if on else "off")), alignment_start=4, alignment_end=3,
                                 sra_limit=8 * (n + 1) * 8, prune_edges=True)
        finally:
            al.close()
        assert (out["stage1"]["pruned_cells"] > 0) == on, (on, out["stage1"]["pruned_cells"])
        texts[on] = (tuple(out["best"]), bytes(out["text"]))
    assert texts[True] == texts[False] and len(texts[True][1]) > 10000
