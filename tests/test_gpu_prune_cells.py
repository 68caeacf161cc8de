"""GPU (-m gpu): pruned LOCAL runs held to the oracle on every cell that can matter, at the places a skip test goes wrong.

The cases elsewhere in the suite were picked to show that pruning bites; these are picked for strip seams and 64-column chunk
seams at every phase, for alignments that start, end and tie in awkward places, for special rows that cut the optimal path
INSIDE a gap (the cell stage 2 matches there is the gap component), and for every way into the engine.  All against the
unpruned oracle (helpers.oracle_full), every output through helpers.assert_pruned_cells -- the reference's own rule
(AbstractBlockPruning::isBlockPrunable, M/libmasa/pruning/AbstractBlockPruning.cpp:70-111) taken down to one cell: a value v
at (i, j) may differ only if v + min(m - i, n - j) * match <= best.  Every run must have skipped cells, must account for all
m * n cells, and must have at least one must-value on every special row above the best cell."""
from functools import reduce
from math import gcd

import numpy as np
import pytest

from helpers import assert_pruned_borders, assert_pruned_cells, oracle_full
from test_gpu_bound import _pairs, _stream
from test_gpu_window import _pair as _window_pair

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SW = 1
_REF = {}


def _oracle(oracle, key, s0, s1, row_ids):
    """the unpruned oracle with the special rows the engine handed out (it rounds the interval to its strip grid: the rows are
    multiples of one step)"""
    step = reduce(gcd, row_ids) if row_ids else 0
    assert step == 0 or step >= 1024, row_ids
    if (key, step) not in _REF:
        _REF[(key, step)] = oracle_full(oracle, s0, s1, special_row_interval=step, block_h=gcd(step, 1024) or 1024)
    assert set(row_ids) <= set(_REF[(key, step)]["special_row_ids"]), (row_ids, _REF[(key, step)]["special_row_ids"])
    return _REF[(key, step)]


def _manager(pkg, al, m, n, interval):
    """mi355sw_align_partition with a manager that asks for pruning: the same dictionary as test_gpu_bound._stream's, column 0 included"""
    part = pkg.Partition(0, 0, m, n)
    mg = pkg.Stage1Manager(part, special_row_interval=interval, keep_last_row=True, keep_last_column=True, block_pruning=True)
    al.alignPartition(part, mg)
    rows = {i: mg.specialRow(i) for i in sorted(mg.special_rows) if i < m}
    return {"best": tuple(mg.getBestScore()), "rows": rows, "last_row": mg.lastRow(), "last_col": mg.lastColumn(), "stats": al.getStatistics()}


def _check(got, ref, m, n, col0, where):
    st = got["stats"]
    assert got["best"] == tuple(ref["best"]), (where, got["best"], ref["best"])
    assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == m * n, (where, st["pruned_cells"], st["processed_cells"], m * n)
    assert len(got["rows"]) >= 2, where
    n_must = assert_pruned_borders(got["rows"], got["last_row"], got["last_col"], ref, m, n, ref["best"][2], SW, col0=col0,
                                   must_rows_upto=ref["best"][0], where=where)
    assert n_must > 0, where
    return n_must


# ---- seams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,m,n", [(0, 70001, 65537), (4, 66000, 70003), (8, 70001, 65537), (12, 66000, 70003), (16, 70001, 65537),
                                   (24, 66000, 70003), (32, 70001, 65537), (4, 70001, 65537), (16, 66000, 70003)])
def test_strip_and_chunk_seams_at_every_strip_height(pkg, oracle, R, m, n):
    """related pairs whose extents are multiples neither of a strip height nor of 64, so that the optimal path (it drifts with
    every indel) crosses strip seams and chunk seams at every phase; every strip height and the engine's own choice; the bound
    from nothing, from the seed, from the optimum and from optimum - 1; special rows every 8192 rows and at an interval the
    engine rounds to its grid (5000)"""
    from masa_cudalign_amd.engine import SMITH_WATERMAN
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=900 + (m % 7))
    al = pkg.MI355Aligner(device=0, rows_per_lane=R)
    try:
        al.setSequences(s0, s1)
        for interval in (8192, 5000):
            got = _stream(pkg, al, m, n, SMITH_WATERMAN, None, interval=interval)
            ids = sorted(got["rows"])
            ref = _oracle(oracle, ("seams", m, n), s0, s1, ids)
            _check(got, ref, m, n, False, "R %d interval %d bound None" % (R, interval))
            if interval != 8192:
                continue
            opt = ref["best"][2]
            seed = al.seedBound(pkg.Partition(0, 0, m, n), SMITH_WATERMAN)
            assert seed is not None and 0 < seed <= opt
            for bound in (seed, opt, opt - 1):
                got = _stream(pkg, al, m, n, SMITH_WATERMAN, bound, interval=interval)
                assert sorted(got["rows"]) == ids
                _check(got, ref, m, n, False, "R %d interval %d bound %d" % (R, interval, bound))
    finally:
        al.close()


# ---- alignment geometry --------------------------------------------------------------------------------------------------

def _two_homologies(pkg):
    """two separate alignments of nearly equal score on different diagonals: a (25 000) at the top right, b (24 500) at the
    bottom left; whichever is the lesser has to survive wherever it could still overtake"""
    sg = pkg.seqgen
    a, b = sg.random_dna(0x9101, 25000), sg.random_dna(0x9102, 24500)
    s0 = np.concatenate([a, sg.random_dna(0x9103, 10000), b])
    s1 = np.concatenate([sg.mutate_dna(b, 0x9104, inversion=0.0), sg.random_dna(0x9105, 9000), sg.mutate_dna(a, 0x9106, inversion=0.0)])
    return np.ascontiguousarray(s0), np.ascontiguousarray(s1)


def _geometry(pkg, kind):
    sg = pkg.seqgen
    if kind.startswith("window"):                  # k = 0: from the corner; 6: a piece from the middle of seq0; 2: short homology, long tail
        return _window_pair(pkg, int(kind[6:]))[:2]
    if kind in ("inversion", "ties"):
        return _pairs(pkg, kind)
    if kind == "two_homologies":
        return _two_homologies(pkg)
    if kind == "ends_in_last_row":
        return sg.related_pair(60000, 75000, cfg=911, inversion=0.0)
    if kind == "ends_in_last_column":
        return sg.related_pair(75000, 60000, cfg=912, inversion=0.0)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["window0", "window6", "window2", "inversion", "two_homologies", "ends_in_last_row",
                                  "ends_in_last_column", "ties"])
def test_alignment_geometry(pkg, oracle, kind):
    """where the alignment lies: from the corner, from the middle of seq0, a short homology with a long unrelated tail, across an
    inversion of 15 %, two separate homologies of nearly equal score, ending in the last row / the last column (reach = 0 at its
    end), three co-optimal copies -- with the running bound from nothing and with the optimum handed in"""
    from masa_cudalign_amd.engine import SMITH_WATERMAN
    s0, s1 = _geometry(pkg, kind)
    m, n = len(s0), len(s1)
    al = pkg.MI355Aligner(device=0, rows_per_lane=8)
    try:
        al.setSequences(s0, s1)
        got = _stream(pkg, al, m, n, SMITH_WATERMAN, None)
        ref = _oracle(oracle, ("geometry", kind), s0, s1, sorted(got["rows"]))
        best = ref["best"]
        if kind == "ends_in_last_row":
            assert best[0] == m
        if kind == "ends_in_last_column":
            assert best[1] == n
        if kind == "two_homologies":                # each homology on its own: the two scores lie within 5 % of each other
            top = oracle_full(oracle, s0[:25000], s1[-26000:], special_row_interval=0)["best"][2]
            bottom = oracle_full(oracle, s0[-24500:], s1[:25500], special_row_interval=0)["best"][2]
            assert best[2] == max(top, bottom) and min(top, bottom) > 0.95 * best[2], (best, top, bottom)
        _check(got, ref, m, n, False, kind + " bound None")
        tight = _stream(pkg, al, m, n, SMITH_WATERMAN, best[2])
        _check(tight, ref, m, n, False, kind + " bound optimum")
        if kind == "ties":
            # values exactly on the bound are exempt by the reference's <=; how many of them the engine kept is reported, not asserted
            on = kept = 0
            want_rows = dict(zip(ref["special_row_ids"], ref["special_rows"]))
            for i, cells in tight["rows"].items():
                w = want_rows[i][1:].astype(np.int64)
                reach = np.minimum(m - i, n - np.arange(1, n + 1))
                eq = w + reach[:, None] == best[2]
                on, kept = on + int(eq.sum()), kept + int((eq & (cells == w)).sum())
            print("ties: %d values with v + reach == best on the special rows, %d of them kept by the engine" % (on, kept))
    finally:
        al.close()


# ---- gap states on the path ----------------------------------------------------------------------------------------------

def _gap_rich(seed=9):
    """one common sequence (1 % substitutions) with eight insertions of 500 ... 3000 random letters, alternately into seq0 and
    into seq1; an insertion into seq0 is placed so that its rows straddle a multiple of 8192 -- a row the engine hands out at
    every strip height.  Returns the pair and, for every insertion into seq0, (rows above it, its length, the column the
    optimal path stands in while it runs down the gap)"""
    rng = np.random.default_rng(seed)

    def rnd(k):
        return ACGT[rng.integers(0, 4, size=k)]
    s0, s1, ins0 = [], [], []
    rows = cols = 0
    for k in range(1, 9):
        ln = int(rng.integers(500, 3001))
        piece = (8192 * k - ln // 2 if k % 2 else 8192 * k - 4096) - rows
        a = rnd(piece)
        b = a.copy()
        hit = rng.random(piece) < 0.01
        b[hit] = rnd(int(hit.sum()))
        s0.append(a)
        s1.append(b)
        rows, cols = rows + piece, cols + piece
        if k % 2:
            ins0.append((rows, ln, cols))
            s0.append(rnd(ln))
            rows += ln
        else:
            s1.append(rnd(ln))
            cols += ln
    a = rnd(3000)
    s0.append(a)
    s1.append(a.copy())
    return np.ascontiguousarray(np.concatenate(s0)), np.ascontiguousarray(np.concatenate(s1)), ins0


def test_special_rows_that_cut_the_optimal_path_inside_a_gap(pkg, oracle):
    """the gap-rich construction of test_gpu_stage4 at 64 440 x 64 937, special rows asked for every 2048 rows (the engine keeps
    the reference's minimum spacing and hands out every 8192nd; the insertions into seq0 lie across those): at least three rows cut
    the optimal path while it runs down an insertion.  There the path's cell holds H = F (the vertical gap), it is a must-value by
    its F, and the row's maximum of H -- all the older tests pinned -- lies somewhere else.  Manager and stream, three strip heights."""
    from masa_cudalign_amd.engine import SMITH_WATERMAN
    s0, s1, ins0 = _gap_rich()
    m, n = len(s0), len(s1)
    assert (m, n) == (64440, 64937)
    for R in (4, 8, 16):
        al = pkg.MI355Aligner(device=0, rows_per_lane=R)
        try:
            al.setSequences(s0, s1)
            got = _stream(pkg, al, m, n, SMITH_WATERMAN, None, interval=2048)
            ids = sorted(got["rows"])
            ref = _oracle(oracle, "gap_rich", s0, s1, ids)
            best = ref["best"]
            want_rows = dict(zip(ref["special_row_ids"], ref["special_rows"]))
            inside = []
            for i in ids:
                for r0, ln, j in ins0:
                    h, f = int(want_rows[i][j, 0]), int(want_rows[i][j, 1])
                    if r0 < i <= r0 + ln and h == f > 0 and f + min(m - i, n - j) > best[2] and int(want_rows[i][:, 0].argmax()) != j:
                        inside.append((i, j))
            assert len(inside) >= 3, inside
            for where, run, col0 in (("stream", got, False), ("manager", _manager(pkg, al, m, n, 2048), True)):
                assert sorted(run["rows"]) == ids
                _check(run, ref, m, n, col0, "gap-rich R %d %s" % (R, where))
                for i, j in inside:                    # (said once more by name: the cell stage 2 would match, both components)
                    assert tuple(run["rows"][i][j - (0 if col0 else 1)]) == tuple(want_rows[i][j]), (R, where, i, j)
        finally:
            al.close()


# ---- every seam of the ABI -----------------------------------------------------------------------------------------------

def _drain(pkg, al):
    """waits for the running stream, reads its special rows and last row and ends it: (rows and last row, best)"""
    import time
    while not al.streamPoll()[1]:
        time.sleep(0.001)
    out = {"last_row": al.streamReadLastRow(), "rows": {}}
    while True:
        try:
            dp, cells = al.streamReadSpecialRow(len(out["rows"]))
        except pkg.engine.AlignerError:
            break
        out["rows"][int(dp)] = cells
    best, nsp = al.streamEnd()
    assert nsp == len(out["rows"]), (nsp, sorted(out["rows"]))      # the loop ended where the rows end, not at some other failure
    return out, best


def test_every_way_into_the_engine(pkg, oracle):
    """one pair, 70 001 x 65 537: mi355sw_align_partition with a pruning manager on the default aligner (probe and seed pass decide
    by themselves), the stream with initial_bound, and the manager again under MI355SW_F_NO_WINDOW, F_TWO_PHASE,
    F_DETERMINISTIC_PRUNE, F_FORCE_INT32 and F_NO_SEED_PASS; then a chain of two bands on one GPU in one process (mi355sw_port_attach)
    that shares its best: each band's slice with its global column offset, and the boundary column the port carried against the
    oracle's column at the seam"""
    from masa_cudalign_amd.engine import (SMITH_WATERMAN, F_NO_WINDOW, F_TWO_PHASE, F_DETERMINISTIC_PRUNE, F_FORCE_INT32, F_NO_SEED_PASS)
    from masa_cudalign_amd.bands import band_limits, canonical_best
    m, n = 70001, 65537
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=921)
    ref = None
    for name, flags in (("default", 0), ("no window", F_NO_WINDOW), ("two phase", F_TWO_PHASE), ("deterministic", F_DETERMINISTIC_PRUNE),
                        ("int32", F_FORCE_INT32), ("no seed pass", F_NO_SEED_PASS)):
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            al.setSequences(s0, s1)
            got = _manager(pkg, al, m, n, 8192)
            ref = _oracle(oracle, "abi", s0, s1, sorted(got["rows"]))
            _check(got, ref, m, n, True, name + " manager")
            if name == "default":
                got = _stream(pkg, al, m, n, SMITH_WATERMAN, ref["best"][2])
                _check(got, _oracle(oracle, "abi", s0, s1, sorted(got["rows"])), m, n, False, "stream with initial_bound")
        finally:
            al.close()
    # two bands, one process, one GPU
    lim = band_limits(n, [1, 1])
    a0, a1 = pkg.MI355Aligner(device=0, rows_per_lane=4), pkg.MI355Aligner(device=0, rows_per_lane=4)
    try:
        for al in (a0, a1):
            al.setSequences(s0, s1)
        a1.portCreate(m)
        a0.portAttach(a1)
        bands, bests = [], []
        for k, al in enumerate((a0, a1)):
            kw = dict(prune_blocks=True, prune_rows=m, prune_cols=n - lim[k], share_best=True, last_column_port=(k == 0),
                      want_last_row=True, special_row_interval=8192, first_row_start_offset=lim[k])
            if k == 1:
                kw.update(first_column_init_type=pkg.INIT_WITH_CUSTOM_DATA, first_column_port=True, first_column=[[0, -pkg.INF]])
            al.streamBegin(pkg.Partition(0, lim[k], m, lim[k + 1]), **kw)
            out, best = _drain(pkg, al)
            bands.append(out)
            bests.append(best)
            st = al.getStatistics()
            assert st["profile_kernel"] == 2 and st["pruned_cells"] > 0, (k, st)
            assert st["pruned_cells"] + st["processed_cells"] == m * (lim[k + 1] - lim[k]), (k, st)
        best = canonical_best(bests)
        assert (best[0] + 1, best[1] + 1, best[2]) == tuple(ref["best"])
        ids = sorted(bands[0]["rows"])
        assert ids == sorted(bands[1]["rows"]) and len(ids) >= 2
        ref = _oracle(oracle, "abi", s0, s1, ids)
        want_rows = dict(zip(ref["special_row_ids"], ref["special_rows"]))
        goal = ref["best"][2]
        must = dict.fromkeys(ids, 0)
        for k in (0, 1):
            cols = np.arange(lim[k] + 1, lim[k + 1] + 1)
            for i in ids:
                must[i] += assert_pruned_cells(bands[k]["rows"][i], want_rows[i][cols], i, cols, m, n, goal, SW, where="band %d row %d" % (k, i))[0]
            assert_pruned_cells(bands[k]["last_row"], ref["last_row"][cols], m, cols, m, n, goal, SW, where="band %d last row" % k)
        assert all(must[i] > 0 for i in ids if i <= ref["best"][0]), must
        col = oracle_full(oracle, s0, s1[:lim[1]], special_row_interval=0)["last_col"]
        n_must, _ = assert_pruned_cells(a1.portRead(0, m), col[1:], np.arange(1, m + 1), lim[1], m, n, goal, SW, where="boundary column")
        assert n_must > 0
    finally:
        a0.close()
        a1.close()


# ---- the unforced path of the largest configurations, in small --------------------------------------------------------------

@pytest.mark.timeout(900)
def test_default_aligner_on_a_pair_the_seed_and_the_probe_plan_for(pkg, oracle):
    """400 000 x 300 000 related pair, default aligner, pruning manager, special rows every 32768: nothing forced -- probe, seed pass,
    strip height and window are the engine's own choices, as in the largest configurations of the benchmark.  The oracle run
    (1.2 * 10^11 cells) is the cost of this test."""
    m, n = 400000, 300000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=931)
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        got = _manager(pkg, al, m, n, 32768)
        st = got["stats"]
        assert st["profile_kernel"] == 2 and st["restarts"] == 0, st
        ref = _oracle(oracle, "c3_small", s0, s1, sorted(got["rows"]))
        n_must = _check(got, ref, m, n, True, "default aligner")
        assert st["pruned_cells"] > 0.3 * m * n
        print("400 000 x 300 000: %.3f skipped, %d must-values on %d rows" % (st["pruned_cells"] / float(m) / n, n_must, len(got["rows"])))
    finally:
        al.close()
