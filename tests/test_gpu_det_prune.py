"""GPU (-m gpu): reproducible pruning (MI355SW_F_DETERMINISTIC_PRUNE).  The reference decides which blocks a diagonal may skip
on the host, between two external diagonals (BlockPruningDiagonal::updatePruningWindow, M/libmasa/pruning/BlockPruningDiagonal.cpp:
109-152): its special rows are a function of the input.  The engine's strips test against a device-wide running best, so WHICH
slabs go depends on when a wavefront looked at it -- the best cell never does, the lower bounds left off the optimal paths do.
In this mode a strip tests against the bound as it stood a fixed number of strips above it plus its own finds
(KernelArgs::det_prefix): two runs leave the same bytes."""
import hashlib
from functools import reduce
from math import gcd

import numpy as np
import pytest
from helpers import assert_pruned_borders, engine_ref, oracle_full

from test_gpu_bound import _stream

pytestmark = pytest.mark.gpu


def _digest(res):
    h = hashlib.sha256()
    for dp in sorted(res["rows"]):
        h.update(np.ascontiguousarray(res["rows"][dp], dtype=np.int32).tobytes())
    h.update(np.ascontiguousarray(res["last_row"], dtype=np.int32).tobytes())
    h.update(np.ascontiguousarray(res["last_col"], dtype=np.int32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("kind,m,n,R", [
    ("local", 2600000, 2300000, 0),        # the bound grows with the sweep (no seed below 8 Mi rows): several rounds of wavefronts
    ("local", 400000, 380000, 4),          # 1563 strips of 256 rows
    ("global", 1500000, 1460000, 8),       # a running LOWER bound of H[m][n]
])
def test_two_runs_leave_the_same_special_rows(pkg, oracle, kind, m, n, R):
    from masa_cudalign_amd.engine import SMITH_WATERMAN, NEEDLEMAN_WUNSCH, F_DETERMINISTIC_PRUNE
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=611)
    rec = SMITH_WATERMAN if kind == "local" else NEEDLEMAN_WUNSCH
    interval = max(8192, m // 24)
    runs = []
    for flags in (F_DETERMINISTIC_PRUNE, F_DETERMINISTIC_PRUNE, 0):
        al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags)
        try:
            al.setSequences(s0, s1)
            runs.append(_stream(pkg, al, m, n, rec, None, interval=interval))
        finally:
            al.close()
    al = pkg.MI355Aligner(device=0, rows_per_lane=R)
    try:
        al.setSequences(s0, s1)
        plain = _stream(pkg, al, m, n, rec, None, interval=interval, prune=False)
    finally:
        al.close()
    a, b, free = runs
    assert a["stats"]["pruned_cells"] > 0.2 * m * n                  # it prunes ...
    assert abs(a["stats"]["pruned_cells"] - b["stats"]["pruned_cells"]) < 1e-5 * m * n   # ... the same slabs in both runs (the count is bookkeeping)
    assert _digest(a) == _digest(b)                                   # the same bytes: special rows, last row, last column
    assert sorted(a["rows"]) == sorted(plain["rows"]) and len(a["rows"]) >= 8
    # and they are what a pruning run may leave: the answer exact, everything else a lower bound of the unpruned run
    if kind == "local":
        assert a["best"] == plain["best"] == free["best"]
    else:
        assert int(a["last_row"][-1, 0]) == int(plain["last_row"][-1, 0]) == int(free["last_row"][-1, 0])
    for dp in plain["rows"]:
        assert np.all(a["rows"][dp] <= plain["rows"][dp]), dp
    assert np.all(a["last_row"] <= plain["last_row"]) and np.all(a["last_col"] <= plain["last_col"])
    # ... and exact wherever the reference's rule could not have skipped a cell, H and the gap component, in the reproducible mode
    # and with the running best alike (helpers.assert_pruned_cells).  The 400 000 x 380 000 case against the unpruned ORACLE
    # (1.5 * 10^11 cells); the other two against the engine's own unpruned run -- 6 * 10^12 and 2.2 * 10^12 cells are 20 and 7
    # minutes of the oracle on 16 cores
    if m * n < 2e11:
        step = reduce(gcd, sorted(plain["rows"]))
        want = oracle_full(oracle, s0, s1, special_row_interval=step, block_h=gcd(step, 1024))
        assert plain["best"] == tuple(want["best"])
    else:
        want = engine_ref(plain["rows"], plain["last_row"], plain["last_col"], col0=False)
    goal = plain["best"][2] if kind == "local" else int(plain["last_row"][-1, 0])
    for name, run in (("reproducible", a), ("running best", free)):
        assert assert_pruned_borders(run["rows"], run["last_row"], run["last_col"], want, m, n, goal, rec, col0=False,
                                     must_rows_upto=plain["best"][0] if kind == "local" else m, where=name) > 0
    # the price: the bound reaches a strip one round of wavefronts later than it could
    print("%s %d x %d: pruned %.3f (reproducible) / %.3f (running best), kernel %.1f / %.1f ms" % (
        kind, m, n, a["stats"]["pruned_cells"] / float(m) / n, free["stats"]["pruned_cells"] / float(m) / n,
        a["stats"]["kernel_ms"], free["stats"]["kernel_ms"]))


def test_a_seeded_run_is_reproducible_at_no_cost(pkg):
    """9 M x 8.6 M: the bound starts from the seed (= the answer on this kind of pair) and never moves -- the mode costs nothing"""
    from masa_cudalign_amd.engine import SMITH_WATERMAN, F_DETERMINISTIC_PRUNE
    m, n = 9000000, 8600000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=612)
    out = []
    for flags in (F_DETERMINISTIC_PRUNE, F_DETERMINISTIC_PRUNE, 0):
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            al.setSequences(s0, s1)
            out.append(_stream(pkg, al, m, n, SMITH_WATERMAN, None, interval=1 << 20))
        finally:
            al.close()
    a, b, free = out
    assert _digest(a) == _digest(b) and a["best"] == b["best"] == free["best"]
    # (the COUNT of skipped slabs is bookkeeping, not data: a strip that retires counts the rest of its row at once, one that
    #  walks behind a slower predecessor counts slab by slab and stops at the row's end -- the same cells either way)
    assert abs(a["stats"]["pruned_cells"] - b["stats"]["pruned_cells"]) < 1e-5 * m * n and a["stats"]["pruned_cells"] > 0.5 * m * n
    print("seeded 9 M x 8.6 M: kernel %.0f / %.0f ms reproducible, %.0f ms running best" % (a["stats"]["kernel_ms"], b["stats"]["kernel_ms"], free["stats"]["kernel_ms"]))
    # (alone on the GPU: 3753 / 3753 / 3749 ms -- profiles/r06_det_prune_tests.log; not asserted: next to other processes' kernels
    #  the three runs' times say nothing about each other)
