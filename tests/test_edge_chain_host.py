"""CPU: edge results and edge pruning along a chain of column bands -- the HOST side.  The ABI carries
mi355sw_stream_edge_best; the chain's reduction (BandRunner.reduce_edge_best) orders its candidates as BestScoreList does; and
BandRunner.run(prune_end=...) over gloo tells every band's engine the edge before each streamBegin exactly when it prunes, asks
for the borders the result is read from, and reduces to the cell and score the oracle's full matrix gives.

The compute engine is tests/test_bands_gloo.py's stand-in on the oracle (the product engine needs a GPU; its side of the
feature is tests/test_gpu_edge_chain.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__ as graft
import edge_chain_cases as cc
import edge_prune_cases as ec
from test_bands_gloo import OracleStreamEngine, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = cc.INF


def test_the_abi_carries_the_edge_result(pkg):
    """header, library, prototype list, Python front; still ABI 8"""
    hdr = open(os.path.join(graft.ROOT, "include", "mi355sw.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mi355sw_stream_edge_best\s*\(\s*mi355sw_handle\s*\*\s*h\s*,\s*int32_t\s+edges\s*,\s*mi355sw_score\s*\*\s*best\s*\)\s*;", code)
    eng = pkg.engine
    assert "mi355sw_stream_edge_best" in eng.ABI_SYMBOLS
    pkg.build_library()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "mi355sw_stream_edge_best")
    lib.mi355sw_stream_edge_best.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    s = eng.Score(5, 6, 7)
    assert lib.mi355sw_stream_edge_best(None, 1, ctypes.byref(s)) != 0        # (no handle: MI355SW_EINVAL, nothing touched)
    assert (s.i, s.j, s.score) == (5, 6, 7)
    assert callable(getattr(pkg.MI355Aligner, "streamEdgeBest", None))
    assert lib.mi355sw_abi_version() == 8
    # the reduction is a unit of its own, built into the library and part of the library's identity
    csrc = os.path.join(graft.PKG_DIR, "csrc")
    assert re.search(r"\bedge_best\.hip\b", open(os.path.join(csrc, "Makefile")).read())
    before = eng.source_build_id()
    assert isinstance(before, str) and len(before) == 16


# ---------------------------------------------------------------------------------------------------------------------------
# the tie order of the chain reduction
# ---------------------------------------------------------------------------------------------------------------------------
class GatherOnly:
    """what reduce_best needs of torch.distributed, with the other ranks' contributions given"""

    def __init__(self, rank, cands):
        self.rank, self.cands = rank, cands

    def all_gather(self, out, t):
        assert tuple(int(x) for x in t.tolist()) == tuple(self.cands[self.rank])
        for k, o in enumerate(out):
            o.copy_(torch.tensor(list(self.cands[k]), dtype=t.dtype))


M, N = 900, 700          # the matrix the hand-made candidates lie on the edges of
TIES = {
    "equal scores on the last row in two bands": [(M - 1, 120, 55), (M - 1, 480, 55), (M - 1, 650, 54)],
    "... the band on the right named first": [(M - 1, 480, 55), (M - 1, 120, 55)],
    "a last-row cell against a last-column cell of the same score": [(M - 1, 30, 77), (M - 1, 300, 70), (400, N - 1, 77)],
    "the last-column cell is the band's own candidate": [(M - 1, 30, 77), (M - 1, 300, 77), (M - 2, N - 1, 77)],
    "the corner cell lies on both edges": [(M - 1, 100, 12), (M - 1, 400, 12), (M - 1, N - 1, 12)],
    "the corner cell alone holds the optimum": [(M - 1, 100, 11), (M - 1, 400, 12), (M - 1, N - 1, 13)],
    "a band that holds nothing": [(-1, -1, -INF), (M - 1, 400, -5), (-1, -1, -INF)],
    "all -INF": [(-1, -1, -INF), (-1, -1, -INF), (-1, -1, -INF), (-1, -1, -INF)],
}


@pytest.mark.parametrize("name", sorted(TIES))
def test_the_chain_reduction_orders_like_best_score_list(pkg, name):
    """score descending, then i ascending, then j ascending -- against numpy's lexsort on hand-made candidates, the same on
    every rank"""
    from masa_cudalign_amd.bands import BandRunner
    cands = TIES[name]
    want = cc.canonical_of(cands)
    for rank in range(len(cands)):
        runner = BandRunner(None, dist=GatherOnly(rank, cands), rank=rank, world=len(cands))
        runner.edge_best = cands[rank]
        assert runner.reduce_edge_best() == want, (name, rank)
    if name == "all -INF":
        assert want == (-1, -1, -INF)
    if name.startswith("a last-row cell against"):
        assert want == (400, N - 1, 77)
    if name.startswith("the corner cell lies"):
        assert want == (M - 1, 100, 12)


def test_a_single_band_reduces_to_its_own_edge_best(pkg):
    from masa_cudalign_amd.bands import BandRunner
    runner = BandRunner(None)
    assert runner.reduce_edge_best() == (-1, -1, -INF)
    runner.edge_best = (3, 4, 5)
    assert runner.reduce_edge_best() == (3, 4, 5)


def test_prune_end_is_a_global_run_with_nothing_tracked(pkg):
    from masa_cudalign_amd.bands import BandRunner, InProcessChain
    for kw in (dict(recurrence=pkg.SMITH_WATERMAN, track_best=True), dict(recurrence=pkg.NEEDLEMAN_WUNSCH, track_best=True),
               dict(recurrence=pkg.SMITH_WATERMAN, track_best=False)):
        with pytest.raises(ValueError, match="prune_end"):
            BandRunner(None).run(100, 0, 100, prune_end=3, **kw)
    with pytest.raises(ValueError, match="prune_end"):
        BandRunner(None).run(100, 0, 100, recurrence=pkg.NEEDLEMAN_WUNSCH, track_best=False, prune_end=4)
    with pytest.raises(ValueError, match="prune_end"):
        InProcessChain([]).run(100, [0, 100], prune_end=1)          # (a local chain)


# ---------------------------------------------------------------------------------------------------------------------------
# BandRunner over gloo
# ---------------------------------------------------------------------------------------------------------------------------
class EdgeOracleEngine(OracleStreamEngine):
    """the stand-in with the two calls of the feature: setPruneEnd is recorded, streamEdgeBest answers from the oracle's rows"""

    def __init__(self, *a, **kw):
        OracleStreamEngine.__init__(self, *a, **kw)
        self.log = []

    def setPruneEnd(self, mode):
        self.log.append(("end", int(mode)))

    def streamBegin(self, part, **kw):
        self.log.append(("begin", bool(kw.get("want_last_row")), bool(kw.get("want_last_column")), bool(kw.get("prune_blocks")),
                         bool(kw.get("force_int32"))))
        self._want = (bool(kw.get("want_last_row")), bool(kw.get("want_last_column")))
        OracleStreamEngine.streamBegin(self, part, **kw)

    def streamEdgeBest(self, edges):
        assert self.done >= self.m
        assert (not edges & 1) or self._want[0]
        assert (not edges & 2) or self._want[1]
        self.log.append(("edge", int(edges)))
        return cc.edge_cell_of(edges, self.row[1:], self.last_col, self.m, self.n, self.part.i0, self.part.j0)


def _worker_edge(rank, world, port, m, n, q):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    oracle = graft.load_oracle()
    from masa_cudalign_amd.bands import BandRunner, band_limits
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _edge_runs(rank, world, m, n, q, pkg, oracle, BandRunner, band_limits)
    except BaseException:
        cc.report_failure(q, rank)
    finally:
        dist.destroy_process_group()


def _edge_runs(rank, world, m, n, q, pkg, oracle, BandRunner, band_limits):
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9970)
    lim = band_limits(n, [1] * world)
    out = {}
    for start in (cc.START_PLUS, cc.START_3):
        row_t, col_t = cc.START_INIT[start]
        for mode in ec.MODES:
            for prune in (False, True):
                eng = EdgeOracleEngine(oracle, s0, s1, seg=256)
                runner = BandRunner(eng, dist=dist, rank=rank, world=world, device=None, segment_rows=512, prune_blocks=prune)
                runner.run(m, lim[rank], lim[rank + 1], recurrence=pkg.NEEDLEMAN_WUNSCH, track_best=False,
                           first_row_init_type=row_t, first_col_init_type=col_t, n_total=n, prune_end=mode)
                out[(start, mode, prune)] = dict(log=list(eng.log), edge=runner.edge_best,
                                                 best=tuple(runner.reduce_edge_best()), restarts=runner.restarts)
                dist.barrier()
    q.put((rank, True, out))


_ORACLE = {}


def _full(pkg, oracle, m, n, start):
    if start not in _ORACLE:
        from helpers import oracle_kwargs
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9970)
        kw = oracle_kwargs(oracle, dict(start=start, end=3, pruning=False, disk=-1, block=(512, 512)), m, n)
        kw.update(want_last_row=True, want_last_col=True)
        ref = oracle.stage1(s0, s1, **kw)
        for a in (ref["last_row"], ref["last_col"]):
            a.setflags(write=False)
        _ORACLE[start] = ref
    return _ORACLE[start]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_band_runner_names_the_edge_and_reduces_to_the_oracles_cell(pkg, oracle, world):
    """3 000 x 2 600, starts + and 3, modes 1 / 2 / 3, with and without prune_blocks: setPruneEnd(mode) right before each
    streamBegin exactly when the runner prunes; the last row wanted in every band when bit 1 is set, the last column in the
    last band only when bit 2 is set; streamEdgeBest asked for the edges the band holds; reduce_edge_best() the same on every
    rank, and the cell and score of edge_optimum on the oracle's full matrix"""
    m, n = 3000, 2600
    res = cc.run_ranks(mp.get_context("spawn"), _worker_edge, world, (_free_port(), m, n), 280)
    for start in (cc.START_PLUS, cc.START_3):
        ref = _full(pkg, oracle, m, n, start)
        for mode in ec.MODES:
            opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
            want = cc.edge_cell_of(mode, ref["last_row"][1:], ref["last_col"][1:], m, n)
            assert want[2] == opt
            for prune in (False, True):
                for rank in range(world):
                    r = res[rank][(start, mode, prune)]
                    last = rank == world - 1
                    here = (mode & 1) | ((mode & 2) if last else 0)
                    # (host transport: every band but the last hands its last column to the driver anyway)
                    begin = ("begin", bool(mode & 1), (not last) or bool(mode & 2), prune, False)
                    want_log = ([("end", mode)] if prune else []) + [begin] + ([("edge", here)] if here else [])
                    assert r["log"] == want_log, (start, mode, prune, rank, r["log"])
                    assert r["best"] == want, (start, mode, prune, rank, r["best"], want)
                    assert r["restarts"] == 0
                    assert (r["edge"] is None) == (here == 0)
                # ... and it is one of the bands' own candidates
                assert want in [tuple(res[rank][(start, mode, prune)]["edge"]) for rank in range(world) if res[rank][(start, mode, prune)]["edge"]]
