"""Shared by tests/test_edge_chain_host.py and tests/test_gpu_edge_chain.py: edge results and edge pruning along a chain of
column bands (mi355sw_stream_edge_best, BandRunner.run / InProcessChain.run(prune_end=...), BandRunner.reduce_edge_best).

The result of such a chain is the best H on the allowed edge(s) of the WHOLE matrix with its cell, in BestScoreList's order --
score descending, then i ascending, then j ascending (M/common/BestScoreList.hpp:30-38) -- as a 0-based cell like every best the
engine reports.  Here: that order in numpy, independent of bands.canonical_best, and the start forms the tests run."""
import numpy as np

INF = 999999999
# alignment_start of the two forms every chain test runs: '+' (gap penalties from the corner on both borders), '3' (zeroes)
START_PLUS, START_3 = 4, 3
INIT_WITH_ZEROES, INIT_WITH_GAPS = 0, 1
START_INIT = {START_PLUS: (INIT_WITH_GAPS, INIT_WITH_GAPS), START_3: (INIT_WITH_ZEROES, INIT_WITH_ZEROES)}   # (first row, first column)


def canonical_of(cands):
    """cands: (k, 3) array-like of (i, j, score); (-1, -1, *) and scores at or below -INF are no candidates.  The first in
    (score desc, i asc, j asc), or (-1, -1, -INF)."""
    c = np.asarray(cands, dtype=np.int64).reshape(-1, 3)
    c = c[(c[:, 0] >= 0) & (c[:, 1] >= 0) & (c[:, 2] > -INF)]
    if len(c) == 0:
        return (-1, -1, -INF)
    k = np.lexsort((c[:, 1], c[:, 0], -c[:, 2]))[0]
    return (int(c[k, 0]), int(c[k, 1]), int(c[k, 2]))


def edge_cell_of(edges, last_row, last_col, m, n, i0=0, j0=0):
    """canonical best cell (i, j, score), 0-based in the whole matrix, of the edge(s) of an m x n partition whose first cell is
    (i0, j0): last_row (n, 2) and last_col (m, 2) WITHOUT their coordinate-0 cells (what streamReadLastRow / streamReadColumn
    hand out); either may be None when its bit of `edges` is clear.  The border cells H[m][0] / H[0][n] are not in the arrays,
    hence no candidates."""
    cands = []
    if edges & 1:
        h = np.asarray(last_row)[:, 0].astype(np.int64)
        assert len(h) == n
        cands.append(np.stack([np.full(n, i0 + m - 1, dtype=np.int64), j0 + np.arange(n), h], axis=1))
    if edges & 2:
        h = np.asarray(last_col)[:, 0].astype(np.int64)
        assert len(h) == m
        cands.append(np.stack([i0 + np.arange(m), np.full(m, j0 + n - 1, dtype=np.int64), h], axis=1))
    return canonical_of(np.concatenate(cands))


def run_ranks(ctx, target, world, args, limit_s):
    """One process per rank running target(rank, world, *args, q); every worker reports (rank, True, payload) or, through
    report_failure, (rank, False, traceback).  Returns {rank: payload}.  A rank that fails -- or dies without a word -- fails the
    test AT ONCE and the other ranks are stopped: nobody sits out a time limit waiting for a band that will never report."""
    import queue
    import time
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = {}, time.time() + limit_s
    try:
        while len(res) < world:
            try:
                rank, ok, payload = q.get(timeout=0.2)
            except queue.Empty:
                gone = [k for k, p in enumerate(procs) if k not in res and p.exitcode is not None]
                if gone:                       # (its report may still be in the pipe: one more look before giving up)
                    try:
                        rank, ok, payload = q.get(timeout=2.0)
                    except queue.Empty:
                        raise AssertionError("rank(s) %s ended (exit code %s) without a result" % (gone, [procs[k].exitcode for k in gone]))
                elif time.time() > deadline:
                    raise AssertionError("no result from rank(s) %s within %d s" % ([k for k in range(world) if k not in res], limit_s))
                else:
                    continue
            assert ok, "rank %d failed:\n%s" % (rank, payload)
            res[rank] = payload
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
    return res


def report_failure(q, rank):
    """from a worker's except clause: the traceback goes to run_ranks"""
    import traceback
    q.put((rank, False, traceback.format_exc()))
