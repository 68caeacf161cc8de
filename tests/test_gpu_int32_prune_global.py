"""GPU (-m gpu): block pruning of GLOBAL alignments in the int32 kernel family (MI355SW_F_INT32_PRUNE_GLOBAL, opt-in) -- the
pairs the packed kernels cannot take (15 or more common byte values, 63 or more with MI355SW_F_WIDE_ALPHABET),
MI355SW_F_FORCE_INT32 and the rerun after an MI355SW_EOVERFLOW16 report.  The rule is the packed family's last-cell rule
("Global"; AbstractBlockPruning.cpp:92-109), one 64-step slab of a strip at a time.

The reference is the UNPRUNED oracle (oracle.stage1, start = end = 4, pruning off), as in tests/test_gpu_prune_global.py: H[m][n]
must be the oracle's, every other cell a lower bound of the true one and exact wherever v + min(dI,dJ) - 2 |dJ - dI| >= H[m][n]
(helpers.assert_pruned_cells, the one criterion of the suite).  waves = 1 wherever a figure is asserted: what is skipped is
then a function of the input."""
import time

import numpy as np
import pytest

from helpers import NEEDLEMAN_WUNSCH, assert_pruned_borders, assert_pruned_cells, oracle_kwargs
from test_gpu_prune32 import _iupac_pair
from test_gpu_prune_global import _check_lower_bounds, _global_run
from test_gpu_wide_alphabet import POOL, THREADS, common_letters, wide_pair

pytestmark = pytest.mark.gpu
F_FORCE_INT32, F_NO_WINDOW, F_WIDE = 2, 1024, 65536
INF = 999999999
M1, N1 = 24000, 20000
_CACHE = {}


def _flag(pkg):
    return pkg.engine.F_INT32_PRUNE_GLOBAL


def _route(pkg, route):
    """the pair and the engine flags of one way into the int32 family"""
    if ("pair", route) not in _CACHE:
        if route == "iupac":
            s0, s1 = _iupac_pair(pkg, M1, N1, 811)
            flags = 0
            assert common_letters(s0, s1) == 15
        elif route == "forced":
            s0, s1 = pkg.seqgen.related_pair(M1, N1, cfg=812)
            flags = F_FORCE_INT32
        else:
            s0, s1 = wide_pair(pkg, M1, N1, POOL, cfg=813, ensure=True)
            flags = F_WIDE
            assert common_letters(s0, s1) == 63
        _CACHE[("pair", route)] = (s0, s1, flags)
    return _CACHE[("pair", route)]


def _oracle_nw(oracle, key, s0, s1, interval=0):
    """the unpruned global oracle over the whole of s0 x s1 (computed once per key)"""
    if ("ref", key) not in _CACHE:
        kw = oracle_kwargs(oracle, dict(start=4, end=4, pruning=False, disk=-1, block=(4096 if interval else 1024, 1 << 20)), len(s0), len(s1))
        kw.update(want_last_row=True, want_last_col=True, special_row_interval=interval, threads=THREADS)
        _CACHE[("ref", key)] = oracle.stage1(s0, s1, **kw)
    return _CACHE[("ref", key)]


def _is_nw_prune_kernel(st):
    return st["kernel"].startswith("sw_strip_kernel<") and st["kernel"].endswith(",false,true>") and st["profile_kernel"] in (0, 1)


def _stream_nw(pkg, al, part, interval=0, **over):
    """one global stream to its end: last row, last column, special rows {dp row of the partition: cells}, statistics"""
    kw = dict(recurrence_type=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=pkg.INIT_WITH_GAPS, first_column_init_type=pkg.INIT_WITH_GAPS,
              track_best=False, prune_blocks=True, want_last_row=True, want_last_column=True, special_row_interval=interval)
    kw.update(over)
    al.streamBegin(part, **kw)
    while not al.streamPoll()[1]:
        time.sleep(0.001)
    out = {"last_row": al.streamReadLastRow(), "rows": {},
           "last_col": al.streamReadColumn(0, part.getHeight()) if kw["want_last_column"] else None}
    while True:
        try:
            dp, cells = al.streamReadSpecialRow(len(out["rows"]))
        except pkg.engine.AlignerError:
            break
        out["rows"][int(dp)] = cells
    al.streamEnd()
    out["stats"] = al.getStatistics()
    return out


def _no_value_below_minus_inf(*arrays):
    """every store of the pruning kernel is clamped at -INF (sw_kernel.hip, clamp_void32 and the output chunk): what is handed
    out is never below it, however many computed cells lie downstream of skipped ones.  (In registers a value may sink to
    -INF - 5 - 5 * (64 + 64 R) inside one slab -- 5 per step, 64 columns and the strip's 64 R rows -- before the next clamp.)"""
    for a in arrays:
        if a is not None:
            assert int(np.asarray(a).min()) >= -INF, int(np.asarray(a).min())


# ---- 1. every route, every strip height, against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 8, 16, 0])
@pytest.mark.parametrize("route", ["iupac", "forced", "wide63"])
def test_every_route_into_the_int32_family_prunes_a_global_alignment(pkg, oracle, route, R):
    """24 000 x 20 000 related pair: 15 IUPAC letters, MI355SW_F_FORCE_INT32, 63 letters under MI355SW_F_WIDE_ALPHABET; strips of
    256 / 512 / 1024 rows and the engine's own choice.  With the flag: H[m][n] is the oracle's, cells are skipped, the books
    balance, the kernel is the global pruning instantiation, last row / last column / special rows every 4096 hold the
    criterion.  Without it, on the same engine: nothing is skipped, everything equals the oracle (true of the parent too)."""
    s0, s1, flags = _route(pkg, route)
    ref = _oracle_nw(oracle, route, s0, s1, 4096)
    final = int(ref["last_row"][-1, 0])
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        mg, st = _global_run(pkg, al, M1, N1, True, 4096)
        assert _is_nw_prune_kernel(st), st["kernel"]
        assert tuple(mg.getBestScore()) == tuple(ref["best"]) == (M1, N1, final)
        assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == M1 * N1, st
        assert st["restarts"] == 0 and st["kernel_launches"] == 1
        _check_lower_bounds(mg, ref, M1, N1, final)
        _no_value_below_minus_inf(mg.lastRow(), mg.lastColumn(), *[mg.specialRow(i) for i in mg.special_rows])
        print("%s R %d: %.3f of the matrix skipped (%s)" % (route, R, st["pruned_cells"] / float(M1 * N1), st["kernel"]))
        al.setFlag(_flag(pkg), False)
        mg, st = _global_run(pkg, al, M1, N1, True, 4096)
        assert st["pruned_cells"] == 0 and st["kernel"].startswith("sw_strip_kernel<") and not st["kernel"].endswith(",true>"), st
        assert tuple(mg.getBestScore()) == tuple(ref["best"])
        assert np.array_equal(mg.lastRow(), ref["last_row"]) and np.array_equal(mg.lastColumn(), ref["last_col"])
        want = dict(zip(ref["special_row_ids"], ref["special_rows"]))
        for i in mg.special_rows:
            if i in want:
                assert np.array_equal(mg.specialRow(i), want[i]), i
    finally:
        al.close()


# ---- 2. structural edges ------------------------------------------------------------------------------------------------------
SH = 256            # rows_per_lane 4


def _edge_case(pkg, name):
    rel = pkg.seqgen.related_pair
    if name.startswith("m"):            # strip boundaries: m = 23 SH - 1, 23 SH, 23 SH + 1, and a last strip that ends inside lane 32
        m = {"m-1": 23 * SH - 1, "m0": 23 * SH, "m+1": 23 * SH + 1, "m_in_lane": 23 * SH + 130}[name]
        return rel(m, 5000, cfg=821)
    if name.startswith("n"):            # the 2 CHUNK / col0 + CHUNK <= n eligibility edge
        return rel(23 * SH, int(name[1:]), cfg=822)
    if name == "identical":
        s = pkg.seqgen.related_pair(23 * SH + 1, 23 * SH + 1, cfg=823)[0]
        return s, s.copy()
    assert name == "unrelated"
    return pkg.seqgen.unrelated_pair(23 * SH + 1, 5000, cfg=824)


@pytest.mark.parametrize("name", ["m-1", "m0", "m+1", "m_in_lane", "n255", "n256", "n257", "n320", "identical", "unrelated"])
def test_structural_edges(pkg, oracle, name):
    """about 6 000 rows at 256-row strips, the bound started at H[m][n] (what a band of a chain is handed): every border cell
    holds the criterion, H[m][n] is exact, and no more slabs go than are eligible -- the ragged last strip is never skipped,
    nor is a slab with col0 < 2 CHUNK or col0 + CHUNK > n"""
    s0, s1 = _edge_case(pkg, name)
    m, n = len(s0), len(s1)
    ref = _oracle_nw(oracle, name, s0, s1)
    goal = int(ref["last_row"][-1, 0])
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg), waves=1 if name != "unrelated" else 0)
    try:
        al.setSequences(s0, s1)
        out = _stream_nw(pkg, al, pkg.Partition(0, 0, m, n), initial_bound=goal)
    finally:
        al.close()
    st = out["stats"]
    assert _is_nw_prune_kernel(st), st["kernel"]
    assert int(out["last_row"][-1, 0]) == goal == int(out["last_col"][-1, 0])
    assert assert_pruned_borders({}, out["last_row"], out["last_col"], ref, m, n, goal, NEEDLEMAN_WUNSCH, col0=False, where=name) > 0
    _no_value_below_minus_inf(out["last_row"], out["last_col"])
    full_strips, eligible = m // SH, max(0, n // 64 - 2)
    assert st["pruned_cells"] % (64 * SH) == 0 and st["pruned_cells"] <= full_strips * eligible * 64 * SH, (name, st["pruned_cells"])
    assert st["pruned_cells"] + st["processed_cells"] == m * n
    if name.startswith("m") or name == "identical":        # (5 888 x 320 and narrower: the one gap may lie anywhere, little can go)
        assert st["pruned_cells"] > 0, name
    print("%s: %d x %d, %d of %d eligible slabs skipped" % (name, m, n, st["pruned_cells"] // (64 * SH), full_strips * eligible))


def test_a_partition_inside_longer_sequences_with_borders_from_the_oracle(pkg, oracle):
    """a partition whose origin is no multiple of 64, inside 7 000 x 6 500, with the super-partition's extents (prune_rows /
    prune_cols) and its first row and column taken from the oracle, as a band of a chain receives them: the partition's last row
    and column hold the criterion in whole-matrix coordinates"""
    L0, L1 = 7000, 6500
    i0, j0, i1, j1 = 1037, 521, 6037 + 130, 4521
    s0, s1 = pkg.seqgen.related_pair(L0, L1, cfg=825)
    goal = int(_oracle_nw(oracle, "inside", s0, s1)["last_row"][-1, 0])
    row_i0 = _oracle_nw(oracle, "inside_i0", s0[:i0], s1)["last_row"]            # (H, F) of row i0, columns 0 .. L1
    col_j0 = _oracle_nw(oracle, "inside_j0", s0, s1[:j0])["last_col"]            # (H, E) of column j0, rows 0 .. L0
    row_i1 = _oracle_nw(oracle, "inside_i1", s0[:i1], s1)["last_row"]
    col_j1 = _oracle_nw(oracle, "inside_j1", s0, s1[:j1])["last_col"]
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        out = _stream_nw(pkg, al, pkg.Partition(i0, j0, i1, j1), initial_bound=goal, prune_rows=L0 - i0, prune_cols=L1 - j0,
                         first_row_init_type=pkg.INIT_WITH_CUSTOM_DATA, first_row=row_i0[j0:j1 + 1],
                         first_column_init_type=pkg.INIT_WITH_CUSTOM_DATA, first_column=col_j0[i0:i1 + 1])
    finally:
        al.close()
    st = out["stats"]
    assert _is_nw_prune_kernel(st) and st["pruned_cells"] > 0, st
    cols, rows = np.arange(j0 + 1, j1 + 1), np.arange(i0 + 1, i1 + 1)
    n_must = assert_pruned_cells(out["last_row"], row_i1[cols], i1, cols, L0, L1, goal, NEEDLEMAN_WUNSCH, where="inside, last row")[0]
    n_must += assert_pruned_cells(out["last_col"], col_j1[rows], rows, j1, L0, L1, goal, NEEDLEMAN_WUNSCH, where="inside, last column")[0]
    assert n_must > 0
    _no_value_below_minus_inf(out["last_row"], out["last_col"])


# ---- 3. skipped, then computed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 16])
def test_lanes_that_compute_again_next_to_skipped_cells(pkg, oracle, R):
    """two related halves joined by unrelated filler of unequal length (2 500 rows against 900 columns): the optimal path runs
    down the diagonal, crosses the filler and goes on at another offset, so every strip below skips slabs on the left, computes
    across the path next to them and skips again -- and the strips under the filler compute under rows that were skipped.  The
    criterion holds on every special row and border, and nothing handed out lies below -INF: see _no_value_below_minus_inf for
    the clamp's bound"""
    sg = pkg.seqgen
    a0, a1 = sg.related_pair(5000, 5000, cfg=831)
    b0, b1 = sg.related_pair(5000, 5000, cfg=832)
    x0, x1 = sg.unrelated_pair(2500, 900, cfg=833)
    s0, s1 = np.ascontiguousarray(np.concatenate([a0, x0, b0])), np.ascontiguousarray(np.concatenate([a1, x1, b1]))
    m, n = len(s0), len(s1)
    ref = _oracle_nw(oracle, "filler", s0, s1, 4096)
    goal = int(ref["last_row"][-1, 0])
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=F_FORCE_INT32 | _flag(pkg))
    try:
        al.setSequences(s0, s1)
        out = _stream_nw(pkg, al, pkg.Partition(0, 0, m, n), interval=4096, initial_bound=goal)
    finally:
        al.close()
    st = out["stats"]
    assert _is_nw_prune_kernel(st) and st["pruned_cells"] > 0.25 * m * n, st
    assert int(out["last_row"][-1, 0]) == goal
    assert sorted(out["rows"]) == [8192]             # (the engine keeps the reference's minimum spacing: below the filler)
    assert assert_pruned_borders(out["rows"], out["last_row"], out["last_col"], ref, m, n, goal, NEEDLEMAN_WUNSCH, col0=False,
                                 must_rows_upto=m, where="filler R %d" % R) > 0
    _no_value_below_minus_inf(out["last_row"], out["last_col"], *out["rows"].values())
    void = sum(int((np.asarray(r)[:, 0] <= -INF // 2).sum()) for r in out["rows"].values())
    assert void > 0                                  # skipped cells were handed out as such ...
    # ... and the last row (its strip is ragged at both heights: never skipped) holds cells computed from skipped ones --
    # numbers again, below the true ones
    lr, want = np.asarray(out["last_row"])[:, 0], ref["last_row"][1:, 0]
    low = lr < want
    assert low.any() and (lr[low] > -INF // 2).any()


def test_a_tail_of_mismatches_is_what_the_lower_bound_charges(pkg, oracle):
    """a related 5 000 x 5 000 pair followed by 1 536 'A' against 1 536 'C': the way to the last cell is 1 536 mismatches at -3
    (a gap through either tail costs more), exactly what the lower bound charges per diagonal step -- a bound that charged
    less would stand above H[m][n] and cut the optimal path in the tail.  No initial bound: gbest is what the sweep finds."""
    a0, a1 = pkg.seqgen.related_pair(5000, 5000, cfg=841)
    tail = 1536
    s0 = np.ascontiguousarray(np.concatenate([a0, np.full(tail, ord("A"), dtype=np.uint8)]))
    s1 = np.ascontiguousarray(np.concatenate([a1, np.full(tail, ord("C"), dtype=np.uint8)]))
    m, n = len(s0), len(s1)
    ref = _oracle_nw(oracle, "tail", s0, s1)
    goal = int(ref["last_row"][-1, 0])
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        out = _stream_nw(pkg, al, pkg.Partition(0, 0, m, n))
    finally:
        al.close()
    assert _is_nw_prune_kernel(out["stats"]) and out["stats"]["pruned_cells"] > 0
    assert int(out["last_row"][-1, 0]) == goal
    assert assert_pruned_borders({}, out["last_row"], out["last_col"], ref, m, n, goal, NEEDLEMAN_WUNSCH, col0=False, where="tail") > 0


# ---- 4. the rerun after an overflow report --------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["flag", "no_flag"])
def test_overflow_rerun_keeps_the_pruning_request(pkg, oracle, on):
    """a packed global pruning run that reports an overflow at strip 1 (injected): one restart on the int32 family, which prunes
    with the flag and computes every cell without it (as it always has)"""
    s0, s1, _ = _route(pkg, "forced")
    ref = _oracle_nw(oracle, "forced", s0, s1, 4096)
    final = int(ref["last_row"][-1, 0])
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=_flag(pkg) if on else 0, waves=1)
    try:
        al.setSequences(s0, s1)
        al.configure(fault_overflow_strip_plus1=2)
        mg, st = _global_run(pkg, al, M1, N1, True, 4096)
    finally:
        al.close()
    assert st["restarts"] == 1 and st["kernel"].startswith("sw_strip_kernel<"), (st["restarts"], st["kernel"])
    assert tuple(mg.getBestScore()) == tuple(ref["best"])
    # (what the packed attempt handed out before its report came from a pruning run: lower bounds under the criterion either way)
    _check_lower_bounds(mg, ref, M1, N1, final)
    if on:
        assert _is_nw_prune_kernel(st) and st["pruned_cells"] > 0, st
    else:
        assert st["pruned_cells"] == 0 and not st["kernel"].endswith(",true>"), st
        assert np.array_equal(mg.lastRow(), ref["last_row"])          # (the last row is the rerun's alone: every cell computed)


# ---- 5. the bound -----------------------------------------------------------------------------------------------------------------
def test_initial_bound_and_ebound(pkg, oracle):
    """initial_bound = H[m][n] passes and skips at least as much as no bound; H[m][n] + 1 is refused at the end of the stream
    (MI355SW_EBOUND) and the engine stays usable"""
    s0, s1, flags = _route(pkg, "forced")
    ref = _oracle_nw(oracle, "forced", s0, s1, 4096)
    final = int(ref["last_row"][-1, 0])
    part = pkg.Partition(0, 0, M1, N1)
    al = pkg.MI355Aligner(device=0, rows_per_lane=8, flags=flags | _flag(pkg), waves=1)
    try:
        al.setSequences(s0, s1)
        none = _stream_nw(pkg, al, part, want_last_column=False)
        exact = _stream_nw(pkg, al, part, want_last_column=False, initial_bound=final)
        with pytest.raises(pkg.engine.AlignerError, match="EBOUND"):
            _stream_nw(pkg, al, part, want_last_column=False, initial_bound=final + 1)
        again = _stream_nw(pkg, al, part, want_last_column=False, initial_bound=final)
    finally:
        al.close()
    for out in (none, exact, again):
        assert int(out["last_row"][-1, 0]) == final and _is_nw_prune_kernel(out["stats"])
        assert_pruned_cells(out["last_row"], ref["last_row"][1:], M1, np.arange(1, N1 + 1), M1, N1, final, NEEDLEMAN_WUNSCH, where="bound")
    assert exact["stats"]["pruned_cells"] >= none["stats"]["pruned_cells"] > 0
    assert again["stats"]["pruned_cells"] == exact["stats"]["pruned_cells"]          # (waves = 1: a function of the input)
    print("skipped: %.3f without a bound, %.3f from H[m][n]" % (none["stats"]["pruned_cells"] / float(M1 * N1), exact["stats"]["pruned_cells"] / float(M1 * N1)))


# ---- 6. a chain of two bands ------------------------------------------------------------------------------------------------------
def test_two_bands_of_a_chain_on_the_int32_family(pkg, oracle):
    """12 000 x 10 000, two column bands in one process (mi355sw_port_attach, share_best), both on the int32 family with the
    flag: the boundary column and the second band's borders hold the criterion in whole-matrix coordinates, H[m][n] is exact"""
    from masa_cudalign_amd.bands import band_limits
    m, n = 12000, 10000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=861)
    ref = _oracle_nw(oracle, "chain", s0, s1)
    goal = int(ref["last_row"][-1, 0])
    lim = band_limits(n, [1, 1])
    seam = _oracle_nw(oracle, "chain_seam", s0, s1[:lim[1]])["last_col"]
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
            outs.append(_stream_nw(pkg, al, pkg.Partition(0, lim[k], m, lim[k + 1]), **kw))
            assert _is_nw_prune_kernel(outs[k]["stats"]), outs[k]["stats"]["kernel"]
        boundary = a1.portRead(0, m)
    finally:
        a0.close()
        a1.close()
    assert int(outs[1]["last_row"][-1, 0]) == goal
    rows = np.arange(1, m + 1)
    assert assert_pruned_cells(boundary, seam[1:], rows, lim[1], m, n, goal, NEEDLEMAN_WUNSCH, where="boundary column")[0] > 0
    for k in (0, 1):
        cols = np.arange(lim[k] + 1, lim[k + 1] + 1)
        assert_pruned_cells(outs[k]["last_row"], ref["last_row"][cols], m, cols, m, n, goal, NEEDLEMAN_WUNSCH, where="band %d last row" % k)
        assert outs[k]["stats"]["pruned_cells"] + outs[k]["stats"]["processed_cells"] == m * (lim[k + 1] - lim[k])
    assert assert_pruned_cells(outs[1]["last_col"], ref["last_col"][1:], rows, n, m, n, goal, NEEDLEMAN_WUNSCH, where="band 1 last column")[0] > 0
    _no_value_below_minus_inf(boundary, outs[0]["last_row"], outs[1]["last_row"], outs[1]["last_col"])
    assert outs[1]["stats"]["pruned_cells"] > 0


# ---- 7. what is not served --------------------------------------------------------------------------------------------------------
def test_what_the_flag_does_not_serve(pkg, oracle):
    """with the flag, a tracked global recurrence, a semi-global end, mi355sw_set_prune_end and a batch compute every cell:
    pruned_cells == 0 and the results are the oracle's"""
    m, n = 6000, 5000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=871)
    ref = _oracle_nw(oracle, "not_served", s0, s1)
    part = pkg.Partition(0, 0, m, n)
    edges = {1: pkg.AT_SEQUENCE_1, 2: pkg.AT_SEQUENCE_2, 3: pkg.AT_SEQUENCE_1_OR_2, 4: pkg.AT_SEQUENCE_1_AND_2}
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 | _flag(pkg))
    try:
        al.setSequences(s0, s1)
        out = _stream_nw(pkg, al, part, track_best=True)
        assert out["stats"]["pruned_cells"] == 0, "tracked"
        assert np.array_equal(out["last_row"], ref["last_row"][1:]) and np.array_equal(out["last_col"], ref["last_col"][1:])
        for mode in (1, 2, 3):
            al.setPruneEnd(mode)
            out = _stream_nw(pkg, al, part)
            assert out["stats"]["pruned_cells"] == 0, ("set_prune_end", mode)
            assert np.array_equal(out["last_row"], ref["last_row"][1:]) and np.array_equal(out["last_col"], ref["last_col"][1:])
        for end in (1, 2, 3):
            mg = pkg.Stage1Manager(part, alignment_start=edges[4], alignment_end=edges[end], keep_last_row=True, keep_last_column=True)
            mg.block_pruning = True                 # a manager that asks although its goal is not the last cell
            al.alignPartition(part, mg)
            st = al.getStatistics()
            kw = oracle_kwargs(oracle, dict(start=4, end=end, pruning=False, disk=-1, block=(st["strip_rows"], 1 << 20)), m, n)
            kw.update(want_last_row=True, want_last_col=True)
            semi = oracle.stage1(s0, s1, **kw)
            assert st["pruned_cells"] == 0, ("alignment_end", end)
            assert tuple(mg.getBestScore()) == tuple(semi["best"])
            assert np.array_equal(mg.lastRow(), semi["last_row"]) and np.array_equal(mg.lastColumn(), semi["last_col"])
        mg = pkg.Stage1Manager(part, alignment_start=edges[4], alignment_end=edges[4], keep_last_row=True, keep_last_column=True, block_pruning=True)
        al.alignPartitions([part], [mg])
        st = al.getStatistics()
        assert st["pruned_cells"] == 0, "batch"
        assert tuple(mg.getBestScore()) == tuple(ref["best"])
        assert np.array_equal(mg.lastRow(), ref["last_row"]) and np.array_equal(mg.lastColumn(), ref["last_col"])
        # (and the same manager on its own IS served: the engine above is not one that cannot prune)
        mg = pkg.Stage1Manager(part, alignment_start=edges[4], alignment_end=edges[4], keep_last_row=True, block_pruning=True)
        al.alignPartition(part, mg)
        assert _is_nw_prune_kernel(al.getStatistics())
    finally:
        al.close()


# ---- 8. how much ------------------------------------------------------------------------------------------------------------------
def test_skips_at_least_half_of_what_the_packed_family_skips_slab_by_slab(pkg, oracle):
    """the yardstick is the packed family under MI355SW_F_NO_WINDOW at the same strip height (512 rows): the same rule, also
    slab by slab.  A factor of 2 is allowed because an int32 lane spans R = 8 rows where a packed lane spans 2 (its span makes
    both bounds weaker) and because ragged and masked chunks are never skipped here.  Measured figures: CHANGELOG.md."""
    s0, s1, _ = _route(pkg, "forced")
    res = {}
    for name, flags in (("int32", F_FORCE_INT32 | _flag(pkg)), ("packed", F_NO_WINDOW)):
        al = pkg.MI355Aligner(device=0, rows_per_lane=8, flags=flags, waves=1)
        try:
            al.setSequences(s0, s1)
            mg, st = _global_run(pkg, al, M1, N1, True)
            res[name] = (st["pruned_cells"], st["kernel"], st["strip_rows"], mg.getBestScore()[2])
        finally:
            al.close()
    print("pruned cells of %d: int32 %d (%s), packed without window %d (%s): ratio %.3f" % (
        M1 * N1, res["int32"][0], res["int32"][1], res["packed"][0], res["packed"][1], res["int32"][0] / float(max(1, res["packed"][0]))))
    assert res["int32"][2] == res["packed"][2] == 512 and res["int32"][3] == res["packed"][3]
    assert "pk16" in res["packed"][1] and res["packed"][0] > 0
    assert res["int32"][0] >= 0.5 * res["packed"][0]
