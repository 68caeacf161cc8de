"""GPU (-m gpu): edge results and edge pruning ALONG A CHAIN OF COLUMN BANDS -- mi355sw_stream_edge_best (csrc/edge_best.hip: the
best cell of an edge, reduced where the edge lies), a band of a chain keeping the request of mi355sw_set_prune_end, and the
drivers: InProcessChain.run / BandRunner.run(prune_end=...), BandRunner.reduce_edge_best, band_stage1.

As in tests/test_gpu_edge_prune.py the oracle of every pruned run is the UNPRUNED one: the chain's result is the canonical best
cell of the allowed edge(s) of the oracle's matrix (score desc, i asc, j asc), and whatever cells a run hands out -- last-row
slices, the last band's last column, every boundary column, special rows -- go through edge_prune_cases.assert_edge_pruned_cells:
exact wherever v + reach(mode) >= optimum, the oracle's value or less everywhere else.  One device; 256-row strips
(rows_per_lane=4) and 128 wavefronts per band, so that every band of a chain is resident; band k+1 starts after band k."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import edge_chain_cases as cc
import edge_prune_cases as ec
from helpers import oracle_kwargs
from test_bands_gloo import _free_port
from test_gpu_edge_prune import THREADS, unpruned

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = cc.INF
F_FORCE_INT32 = 2
_COL = {}


def boundary_column(oracle, key, s0, s1, start, j):
    """column j of the whole matrix, (H, E) of rows 0 .. m, from the unpruned oracle: the last column of the matrix cut at j
    (computed once per key, left unchanged)"""
    if (key, j) not in _COL:
        kw = oracle_kwargs(oracle, dict(start=start, end=3, pruning=False, disk=-1, block=(1024, 1 << 20)), len(s0), j)
        kw.update(want_last_row=False, want_last_col=True, threads=THREADS)
        col = oracle.stage1(s0, s1[:j], **kw)["last_col"]
        col.setflags(write=False)
        _COL[(key, j)] = col
    return _COL[(key, j)]


def nw_stream(pkg, al, m, n, *, start=cc.START_PLUS, mode=0, row=True, col=True, bound=None):
    """one NEEDLEMAN_WUNSCH stream over the whole matrix, left open once its kernel is through"""
    import time
    row_t, col_t = cc.START_INIT[start]
    if mode:
        al.setPruneEnd(mode)
    al.streamBegin(pkg.Partition(0, 0, m, n), recurrence_type=pkg.NEEDLEMAN_WUNSCH, track_best=False, first_row_init_type=row_t,
                   first_column_init_type=col_t, want_last_row=row, want_last_column=col, prune_blocks=bool(mode), initial_bound=bound)
    while not al.streamPoll()[1]:
        time.sleep(0.0005)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. streamEdgeBest alone
# ---------------------------------------------------------------------------------------------------------------------------
def _pair(pkg, kind, m, n):
    if kind == "AA":
        return np.full(m, ord("A"), dtype=np.uint8), np.full(n, ord("A"), dtype=np.uint8)
    return pkg.seqgen.related_pair(m, n, cfg=9980 + (m + n) % 13)


# (600 001 cells: more than one pass of the reduction's grid -- 2048 blocks of 256 lanes)
EDGE_SHAPES = [("related", 1, 1), ("related", 300, 1), ("related", 1, 300), ("related", 257, 63), ("related", 256, 64), ("related", 255, 65),
               ("related", 1000, 1025), ("related", 12000, 10000), ("related", 70, 600001),
               ("AA", 1000, 1025), ("AA", 1025, 1000), ("AA", 256, 64)]


@pytest.mark.parametrize("kind,m,n", EDGE_SHAPES)
def test_stream_edge_best_is_the_canonical_argmax_of_the_edge(pkg, kind, m, n):
    """an unpruned stream and one under setPruneEnd, last row and last column handed out: for edges 1 / 2 / 3 the call returns
    numpy's canonical argmax (score desc, i asc, j asc; cells at -INF are no candidates) over what streamReadLastRow and
    streamReadColumn hand out.  A^m / A^n with zero borders: H[m][j] = m for every j >= m -- a run of equal cells the smallest
    index of which must come back, and the corner ties with them."""
    s0, s1 = _pair(pkg, kind, m, n)
    start = cc.START_3 if kind == "AA" else cc.START_PLUS
    al = pkg.MI355Aligner(device=0, rows_per_lane=4)
    try:
        al.setSequences(s0, s1)
        for mode in (0, 3):
            nw_stream(pkg, al, m, n, start=start, mode=mode)
            row, col = al.streamReadLastRow(), al.streamReadColumn(0, m)
            got = {e: tuple(al.streamEdgeBest(e)) for e in (1, 2, 3)}
            again = tuple(al.streamEdgeBest(3))                        # (the call leaves the stream as it was)
            al.streamEnd()
            for e in (1, 2, 3):
                want = cc.edge_cell_of(e, row, col, m, n)
                assert got[e] == want, (mode, e, got[e], want)
            assert again == got[3]
            if kind == "AA" and mode == 0:
                k = min(m, n)
                assert got[1] == (m - 1, k - 1, k) and got[2] == (k - 1, n - 1, k) and got[3] == ((k - 1, n - 1, k) if m > n else (m - 1, k - 1, k))
    finally:
        al.close()


def test_stream_edge_best_refuses_what_it_cannot_read(pkg):
    """edges outside 1..3, an edge whose border is not handed out: EINVAL; no stream: ESTATE; the stream stays usable"""
    m, n = 2000, 1800
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9981)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4)
    try:
        al.setSequences(s0, s1)
        with pytest.raises(pkg.AlignerError, match="ESTATE"):
            al.streamEdgeBest(1)
        for row, col, bad, good in ((True, True, (0, 4, -1, 7), (1, 2, 3)), (True, False, (2, 3), (1,)), (False, True, (1, 3), (2,)), (False, False, (1, 2, 3), ())):
            nw_stream(pkg, al, m, n, row=row, col=col)
            for e in bad:
                with pytest.raises(pkg.AlignerError, match="EINVAL"):
                    al.streamEdgeBest(e)
            r = al.streamReadLastRow() if row else None
            c = al.streamReadColumn(0, m) if col else None
            for e in good:
                assert tuple(al.streamEdgeBest(e)) == cc.edge_cell_of(e, r, c, m, n)
            al.streamEnd()
        with pytest.raises(pkg.AlignerError, match="ESTATE"):
            al.streamEdgeBest(1)
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the in-process chain
# ---------------------------------------------------------------------------------------------------------------------------
CM, CN, CCFG = 30000, 26000, 35            # the pair of test_gpu_edge_prune.py's first test: 16-42 % skipped on the sweep-grown bound
CHAINS = {"2 bands": [0, 13000, 26000], "1:2:1": [0, 6500, 19500, 26000], "odd middle": [0, 6500, 19501, 26000]}


def chain_run(pkg, als, limits, m, *, start, mode, prune=True, seed=True, bound=None):
    """one InProcessChain run; returns best, statistics and every cell it hands out: {"rows": last-row slices per band,
    "col": the last band's last column, "ports": {k: the boundary column band k received}}"""
    from masa_cudalign_amd.bands import InProcessChain
    row_t, col_t = cc.START_INIT[start]
    N = len(limits) - 1
    out = {"rows": {}, "col": None, "ports": {}}
    chain = InProcessChain(als[:N], prune_blocks=prune, seed_bound=seed)

    def before_end(k, al):
        if mode == 0 or (mode & 1):
            if mode or k == N - 1:
                out["rows"][k] = al.streamReadLastRow()
        if (mode & 2) and k == N - 1:
            out["col"] = al.streamReadColumn(0, m)
    chain.before_end = before_end
    best, stats = chain.run(m, limits, recurrence=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=row_t, first_col_init_type=col_t, prune_end=mode,
                            initial_bound=bound)
    for k in range(1, N):                   # (the ports keep their cells until the next run resets them)
        out["ports"][k] = als[k].portRead(0, m)
    out.update(best=tuple(best), stats=stats, restarts=chain.restarts, initial_bound=chain.initial_bound)
    return out


def check_chain_cells(oracle, out, ref, key, s0, s1, start, limits, m, n, mode, *, exact=False, where=""):
    """last-row slices side by side, the last band's last column, every boundary column: held to the rule (or, exact=True, equal
    to the oracle's).  Returns the number of values the run was held to exactly."""
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    N = len(limits) - 1
    n_must = 0
    pieces = []
    if mode & 1:
        row = np.concatenate([out["rows"][k] for k in range(N)])
        pieces.append((row, ref["last_row"][1:], m, np.arange(1, n + 1), "last row"))
    if mode & 2:
        pieces.append((out["col"], ref["last_col"][1:], np.arange(1, m + 1), n, "last column"))
    for k in range(1, N):
        col = boundary_column(oracle, key, s0, s1, start, limits[k])
        pieces.append((out["ports"][k], col[1:], np.arange(1, m + 1), limits[k], "boundary column %d" % limits[k]))
    for got, want, i, j, name in pieces:
        if exact:
            assert np.array_equal(got, want), (where, name)
        else:
            n_must += ec.assert_edge_pruned_cells(got, want, i, j, m, n, opt, mode, where="%s %s" % (where, name))[0]
    return n_must


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_a_chain_prunes_against_the_edge_and_returns_its_best_cell(pkg, oracle, chain, mode):
    """30 000 x 26 000 over 2 bands, 3 bands of weights 1 : 2 : 1 and 3 bands whose middle one is 13 001 columns wide; starts +
    and 3, with and without the seed step (below 8 Mi rows it has nothing to add: the bound is the sweep-grown one): the
    chain's best is the oracle's cell, cells are skipped, every cell handed out that can matter is the oracle's and every band
    ran the edge kernels"""
    limits, m, n = CHAINS[chain], CM, CN
    N = len(limits) - 1
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=CCFG)
    als = [pkg.MI355Aligner(device=0, waves=128, rows_per_lane=4) for _ in range(N)]
    try:
        for a in als:
            a.setSequences(s0, s1)
        for start in (cc.START_PLUS, cc.START_3):
            ref = unpruned(oracle, ("t1", start), s0, s1, start)
            want = cc.edge_cell_of(mode, ref["last_row"][1:], ref["last_col"][1:], m, n)
            assert want[2] == ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
            for seed in (False, True):
                where = "%s start %d mode %d seed %d" % (chain, start, mode, seed)
                out = chain_run(pkg, als, limits, m, start=start, mode=mode, seed=seed)
                assert out["best"] == want, (where, out["best"], want)
                assert out["restarts"] == 0 and out["initial_bound"] is None, where
                n_must = check_chain_cells(oracle, out, ref, ("t1", start), s0, s1, start, limits, m, n, mode, where=where)
                assert n_must > 0, where
                st = out["stats"]
                assert sum(s["pruned_cells"] for s in st) > 0, where
                for k, s in enumerate(st):
                    assert s["kernel"].endswith(",false,true>") and s["profile_kernel"] == 2 and s["strip_rows"] == 256, (where, k, s["kernel"])
                    assert s["pruned_cells"] + s["processed_cells"] == m * (limits[k + 1] - limits[k]), (where, k)
                print("%s: skipped share per band %s, %d values held exact" % (where, " ".join("%.3f" % (s["pruned_cells"] / float(s["cells"])) for s in st), n_must))
    finally:
        for a in als:
            a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. BandRunner: processes on the one GPU
# ---------------------------------------------------------------------------------------------------------------------------
BM, BN, BCFG = 24000, 20000, 9982
B_LIMIT = 480000                     # bytes of special rows: an interval below the engine's minimum spacing, i.e. 8192 rows


def _worker_runner(rank, world, port, m, n, transport, modes, work, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from masa_cudalign_amd import sra as sra_mod
    from masa_cudalign_amd.bands import BandRunner, band_limits, band_stage1
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _runner_runs(rank, world, m, n, transport, modes, work, q, pkg, dist, sra_mod, BandRunner, band_limits, band_stage1)
    except BaseException:
        cc.report_failure(q, rank)
    finally:
        dist.destroy_process_group()


def _runner_runs(rank, world, m, n, transport, modes, work, q, pkg, dist, sra_mod, BandRunner, band_limits, band_stage1):
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=BCFG)
    lim = band_limits(n, [1] * world)
    al = pkg.MI355Aligner(device=0, waves=128, rows_per_lane=4)
    al.setSequences(s0, s1)
    runner = BandRunner(al, dist=dist, rank=rank, world=world, device=None, segment_rows=2048, transport=transport, prune_blocks=True)
    out = {}
    for mode in modes:
        res = band_stage1(runner, m, lim[rank], lim[rank + 1], os.path.join(work, "mode%d" % mode), B_LIMIT, n_total=n,
                          recurrence=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=pkg.INIT_WITH_GAPS, first_col_init_type=pkg.INIT_WITH_GAPS,
                          track_best=False, prune_end=mode)
        st = al.getStatistics()
        part = sra_mod.SpecialRowsArea(sra_mod.special_rows_path(res["work"], 1, 0), disk_limit=B_LIMIT).open_partition(0, lim[rank], m, lim[rank + 1])
        rows = {i: part.read_row(i).copy() for i in res["special_rows"]}
        out[mode] = dict(best=tuple(res["best"]), reduced=tuple(runner.reduce_edge_best()), own=runner.edge_best, rows=rows,
                         restarts=runner.restarts, kernel=st["kernel"], pruned=int(st["pruned_cells"]), cells=int(st["cells"]),
                         special=list(res["special_rows"]))
        dist.barrier()
    al.close()
    q.put((rank, True, out))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,transport,modes", [(2, "p2p", (3, 1)), (2, "host", (3, 2)), (4, "p2p", (3, 2)), (4, "host", (3, 1))])
def test_band_runner_processes_reduce_the_edge_and_keep_special_rows(pkg, oracle, tmp_path, world, transport, modes):
    """24 000 x 20 000, one process per band on cuda:0, through the ports and through the host, band_stage1 with special rows
    every 8 192 rows: the rows of the bands side by side are held to the rule with every row the optimal alignment crosses
    holding must-values; reduce_edge_best() is the oracle's cell on every rank; no band restarted"""
    from masa_cudalign_amd.bands import band_limits
    m, n = BM, BN
    res = cc.run_ranks(mp.get_context("spawn"), _worker_runner, world, (_free_port(), m, n, transport, modes, str(tmp_path)), 500)
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=BCFG)
    ref = unpruned(oracle, "chain-bands", s0, s1, cc.START_PLUS, interval=8192)
    lim = band_limits(n, [1] * world)
    for mode in modes:
        opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
        want = cc.edge_cell_of(mode, ref["last_row"][1:], ref["last_col"][1:], m, n)
        for r in range(world):
            got = res[r][mode]
            assert got["reduced"] == want, (mode, r, got["reduced"], want)
            assert got["best"] == (want[0] + 1, want[1] + 1, want[2]), (mode, r)           # band_stage1: DP coordinates
            assert got["restarts"] == 0 and got["kernel"].endswith(",false,true>"), (mode, r, got["kernel"])
            assert got["special"] == [8192, 16384, m], (mode, r, got["special"])
        assert want in [tuple(res[r][mode]["own"]) for r in range(world) if res[r][mode]["own"] is not None]
        # every special row and the last row: the bands' slices side by side (cell 0 of a slice is the boundary column's)
        rows = {i: np.concatenate([res[r][mode]["rows"][i][1:] for r in range(world)]) for i in (8192, 16384, m)}
        end_row = m if (mode & 1) and int(ref["last_row"][:, 0].max()) == opt else int(np.argmax(ref["last_col"][:, 0] == opt))
        must_rows = [i for i in ref["special_row_ids"] if i <= end_row and i < m]
        assert len(must_rows) >= 1
        last_row = rows.pop(m)
        n_must = ec.assert_edge_pruned_borders(rows, last_row, None, ref, m, n, opt, mode, col0=False, must_rows=must_rows,
                                               where="%d bands %s mode %d" % (world, transport, mode))
        assert n_must > 0
        assert sum(res[r][mode]["pruned"] for r in range(world)) > 0
        print("%d bands %s mode %d: skipped share per band %s, %d values held exact" % (
            world, transport, mode, " ".join("%.3f" % (res[r][mode]["pruned"] / float(res[r][mode]["cells"])) for r in range(world)), n_must))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. what a chain does not serve
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", ["int32", "768 rows", "overflow"])
def test_requests_a_chain_does_not_serve_compute_every_cell(pkg, oracle, monkeypatch, item):
    """the 1 : 2 : 1 chain with MI355SW_F_FORCE_INT32, with 768-row strips, and with the packed kernels reporting an overflow
    (the test knob of the replay path): the request goes together with the pruning, every cell is the oracle's, nothing is
    skipped, the edge result is still right -- and the overflow costs exactly one restart of the chain"""
    limits, m, n, start = CHAINS["1:2:1"], CM, CN, cc.START_PLUS
    N = len(limits) - 1
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=CCFG)
    ref = unpruned(oracle, ("t1", start), s0, s1, start)
    kw = {"int32": dict(flags=F_FORCE_INT32, rows_per_lane=4), "768 rows": dict(rows_per_lane=12), "overflow": dict(rows_per_lane=4)}[item]
    als = [pkg.MI355Aligner(device=0, waves=128, **kw) for _ in range(N)]
    try:
        for a in als:
            a.setSequences(s0, s1)
        if item == "overflow":
            monkeypatch.setenv("MI355SW_FAULT_OVERFLOW_STRIP", "5")
        for mode in (3, 2):
            out = chain_run(pkg, als, limits, m, start=start, mode=mode)
            assert out["best"] == cc.edge_cell_of(mode, ref["last_row"][1:], ref["last_col"][1:], m, n), (item, mode)
            check_chain_cells(oracle, out, ref, ("t1", start), s0, s1, start, limits, m, n, mode, exact=True, where="%s mode %d" % (item, mode))
            for k, s in enumerate(out["stats"]):
                assert s["pruned_cells"] == 0 and s["processed_cells"] == m * (limits[k + 1] - limits[k]), (item, mode, k)
                assert not s["kernel"].endswith(",false,true>"), (item, mode, s["kernel"])
                if item != "768 rows":
                    assert s["kernel"].startswith("sw_strip_kernel<"), (item, mode, s["kernel"])
            assert out["restarts"] == (1 if item == "overflow" else 0), (item, mode, out["restarts"])
    finally:
        for a in als:
            a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the bound
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ec.MODES)
def test_a_chain_is_held_to_the_bound_it_started_from(pkg, oracle, mode):
    """12 000 x 10 000 over two bands: initial_bound = optimum passes and prunes, optimum + 1 -- a score no alignment reaches --
    is EBOUND from check_chain_bound (one band cannot tell: the best may be another band's), and the chain stays usable"""
    m, n, start = 12000, 10000, cc.START_PLUS
    limits = [0, 5000, 10000]
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9700)
    ref = unpruned(oracle, "t3", s0, s1, start)
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    want = cc.edge_cell_of(mode, ref["last_row"][1:], ref["last_col"][1:], m, n)
    als = [pkg.MI355Aligner(device=0, waves=128, rows_per_lane=4) for _ in range(2)]
    try:
        for a in als:
            a.setSequences(s0, s1)
        for rep in range(2):
            out = chain_run(pkg, als, limits, m, start=start, mode=mode, bound=opt)
            assert out["best"] == want and out["initial_bound"] == opt and out["restarts"] == 0
            assert check_chain_cells(oracle, out, ref, "t3", s0, s1, start, limits, m, n, mode, where="from the optimum") > 0
            assert sum(s["pruned_cells"] for s in out["stats"]) > 0
            assert all(s["kernel"].endswith(",false,true>") for s in out["stats"])
            if rep == 0:
                with pytest.raises(pkg.AlignerError, match="EBOUND"):
                    chain_run(pkg, als, limits, m, start=start, mode=mode, bound=opt + 1)
    finally:
        for a in als:
            a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. off means off
# ---------------------------------------------------------------------------------------------------------------------------
def test_without_the_mode_a_chain_is_what_it_was(pkg, oracle):
    """prune_end=0: the global chain -- (m - 1, n - 1, H[m][n]), the last-cell kernels when it prunes and the plain ones when
    it does not, no last row but the last band's, the unpruned last row the oracle's"""
    limits, m, n, start = CHAINS["1:2:1"], CM, CN, cc.START_PLUS
    N = len(limits) - 1
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=CCFG)
    ref = unpruned(oracle, ("t1", start), s0, s1, start)
    final = int(ref["last_row"][-1, 0])
    als = [pkg.MI355Aligner(device=0, waves=128, rows_per_lane=4) for _ in range(N)]
    try:
        for a in als:
            a.setSequences(s0, s1)
        for prune in (False, True):
            out = chain_run(pkg, als, limits, m, start=start, mode=0, prune=prune)
            assert out["best"] == (m - 1, n - 1, final) and out["restarts"] == 0
            assert sorted(out["rows"]) == [N - 1] and out["col"] is None
            for k, s in enumerate(out["stats"]):
                assert s["kernel"] == "sw_strip_kernel_pk16<2,false,false,%s>" % ("true" if prune else "false"), s["kernel"]
                assert s["pruned_cells"] + s["processed_cells"] == m * (limits[k + 1] - limits[k])
                assert prune or s["pruned_cells"] == 0
            if not prune:
                assert np.array_equal(out["rows"][N - 1], ref["last_row"][1 + limits[N - 1]:])
                for k in range(1, N):
                    assert np.array_equal(out["ports"][k], boundary_column(oracle, ("t1", start), s0, s1, start, limits[k])[1:]), k
            else:
                assert int(out["rows"][N - 1][-1, 0]) == final and np.all(out["rows"][N - 1][:, 0] <= ref["last_row"][1 + limits[N - 1]:, 0])
    finally:
        for a in als:
            a.close()
