"""GPU (-m gpu): goal pruning (mi355sw_set_goal_bounds; the GOAL instantiations of the packed pruning kernels,
csrc/sw_kernel_pk16.inc) -- a sweep that looks for a goal score on its LAST COLUMN skips every slab of cells from which
that score is out of reach.

The oracle of a pruned sweep is the UNPRUNED one (oracle/sw_oracle.c).  With the column bound B, a value v (H, or the
gap component) of a cell with dj columns left to the last column

    equals the oracle's,  or  is <= it where the oracle's v has  v + dj < B

-- skipped cells read -INF, cells computed next to them are lower bounds -- and on the last column every cell whose true
H is >= B is exact.  No reference counterpart: MASA-Core's stage 2 switches pruning off (sw_stage2.cpp:324)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import oracle_kwargs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = 999999999
NW_SEMI = dict(start=4, end=3)          # gap-initialised borders, global recurrence, last row and last column handed out


def assert_goal_pruned(got, want, dj, bound, where, last_column=False):
    """the criterion above on (k, 2) cells; dj: columns left per cell.  Returns how many values differ."""
    g, w = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert g.shape == w.shape and g.ndim == 2 and g.shape[1] == 2, (where, g.shape, w.shape)
    dj = np.broadcast_to(np.asarray(dj, dtype=np.int64), (g.shape[0],))[:, None]
    ok = (g == w) | ((g <= w) & (w + dj < bound))
    if not ok.all():
        idx = np.argwhere(~ok)
        raise AssertionError("%s: %d offending values of %d; first (cell, component, got, want, dj, bound): %s" % (
            where, len(idx), g.size, [(int(r), "HG"[c], int(g[r, c]), int(w[r, c]), int(dj[r, 0]), int(bound)) for r, c in idx[:8]]))
    if last_column:
        must = w[:, 0] >= bound
        assert must.any() and np.array_equal(g[must, 0], w[must, 0]), where
    return int((g != w).sum())


def _manager(pkg, part, interval):
    return pkg.Stage1Manager(part, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_OR_2,
                             special_row_interval=interval, keep_last_row=True, keep_last_column=True)


def _reference(oracle, s0, s1, strip_rows, interval):
    m, n = len(s0), len(s1)
    kw = oracle_kwargs(oracle, dict(pruning=False, disk=-1, block=(strip_rows, 1 << 20), **NW_SEMI), m, n)
    kw.update(want_last_row=True, want_last_col=True, special_row_interval=interval)
    return oracle.stage1(s0, s1, **kw)


_REFS = {}


def _shared_reference(pkg, oracle, m, n, strip_rows, interval):
    """pair and oracle result per shape and grid, computed once and left unchanged"""
    key = (m, n, strip_rows, interval)
    if key not in _REFS:
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=71)
        ref = _reference(oracle, s0, s1, strip_rows, interval)
        for a in [ref["last_row"], ref["last_col"]] + list(ref["special_rows"] if ref.get("special_rows") is not None else []):
            a.setflags(write=False)
        _REFS[key] = (s0, s1, ref)
    return _REFS[key]


def _check_sweep(mg, ref, m, n, bound, where):
    """last column, special rows and last row of a goal-pruned sweep against the oracle's; returns the values that differ"""
    differing = assert_goal_pruned(mg.lastColumn(), ref["last_col"], 0, bound, where + " last column", last_column=True)
    cols_left = n - np.arange(0, n + 1)
    differing += assert_goal_pruned(mg.lastRow(), ref["last_row"], cols_left, bound, where + " last row")
    want_rows = dict(zip(ref.get("special_row_ids") or [], ref["special_rows"] if ref.get("special_rows") is not None else []))
    for i in sorted(mg.special_rows):
        if i == m:
            continue                                   # (the manager keeps the last row under its row number too)
        differing += assert_goal_pruned(mg.specialRow(i), want_rows[i], cols_left, bound, "%s special row %d" % (where, i))
    return differing


def _bytes(mg):
    return b"".join([mg.lastColumn().tobytes(), mg.lastRow().tobytes()] + [mg.specialRow(i).tobytes() for i in sorted(mg.special_rows)])


# 2048 x 1536: whole strips; 2049 x 1601: a ragged last strip and a partly filled last chunk; 8209 x 4096: a special row inside
# (the engine never puts special rows closer than 8192 rows: 8209 rows hold the row 8192 and, 17 rows on, the last row);
# 16401 x 1536 (added): two special rows inside, 8192 and 16384
SHAPES = [(2048, 1536), (2049, 1601), (8209, 4096), (16401, 1536)]


@pytest.mark.parametrize("rows_per_lane", [4, 8], ids=["256rows", "512rows"])
@pytest.mark.parametrize("m,n", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_one_goal_sweep_against_the_oracle(pkg, oracle, m, n, rows_per_lane):
    """one sweep through mi355sw_align_partition with B = (largest H of the oracle's last column) - 200"""
    interval = 8192
    s0, s1, ref = _shared_reference(pkg, oracle, m, n, 64 * rows_per_lane, interval)
    bound = int(ref["last_col"][:, 0].max()) - 200
    al = pkg.MI355Aligner(device=0, rows_per_lane=rows_per_lane)
    try:
        al.setSequences(s0, s1)
        runs = []
        for _ in range(2):
            part = pkg.Partition(0, 0, m, n)
            mg = _manager(pkg, part, interval)
            al.setGoalBounds([bound])
            al.alignPartition(part, mg)
            runs.append((mg, al.getStatistics()))
        mg, st = runs[0]
        assert st["kernel"] == "sw_strip_kernel_pk16<%d,false,false,true,true>" % (rows_per_lane // 2), st["kernel"]
        assert st["strip_rows"] == 64 * rows_per_lane and st["kernel_launches"] == 1 and st["restarts"] == 0
        n_special = len([i for i in mg.special_rows if i != m])
        assert n_special == (m - 1) // 8192
        differing = _check_sweep(mg, ref, m, n, bound, "%dx%d" % (m, n))
        print("%d x %d, %d-row strips: bound %d, pruned %d of %d cells, %d handed-out values are lower bounds" % (
            m, n, st["strip_rows"], bound, st["pruned_cells"], m * n, differing))
        assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == m * n
        assert _bytes(runs[0][0]) == _bytes(runs[1][0]) and runs[0][1]["pruned_cells"] == runs[1][1]["pruned_cells"]
        # the bound is consumed by the call it was set for: the next one computes every cell
        part = pkg.Partition(0, 0, m, n)
        mg = _manager(pkg, part, interval)
        al.alignPartition(part, mg)
        assert al.getStatistics()["pruned_cells"] == 0 and np.array_equal(mg.lastColumn(), ref["last_col"]) and np.array_equal(mg.lastRow(), ref["last_row"])
    finally:
        al.close()


@pytest.mark.parametrize("how", ["many_letters", "force_int32"])
def test_outside_the_packed_family_nothing_is_pruned(pkg, oracle, how):
    """more than 14 byte values, or MI355SW_F_FORCE_INT32: the bound is dropped, every cell is the oracle's"""
    from masa_cudalign_amd.engine import F_FORCE_INT32
    m, n = 2049, 1601
    if how == "many_letters":
        rng = np.random.RandomState(12)
        letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
        s1 = letters[rng.randint(0, 20, n)]
        s0 = np.concatenate([s1, letters[rng.randint(0, 20, m - n)]])
        mut = rng.rand(m) < 0.1
        s0[mut] = letters[rng.randint(0, 20, int(mut.sum()))]
        s0, s1 = np.ascontiguousarray(s0), np.ascontiguousarray(s1)
    else:
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=71)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_FORCE_INT32 if how == "force_int32" else 0)
    try:
        al.setSequences(s0, s1)
        ref = _reference(oracle, s0, s1, 256, 8192)
        part = pkg.Partition(0, 0, m, n)
        mg = _manager(pkg, part, 8192)
        al.setGoalBounds([int(ref["last_col"][:, 0].max()) - 200])
        al.alignPartition(part, mg)
        st = al.getStatistics()
    finally:
        al.close()
    assert st["kernel"].startswith("sw_strip_kernel<"), st["kernel"]
    assert st["pruned_cells"] == 0
    assert np.array_equal(mg.lastColumn(), ref["last_col"]) and np.array_equal(mg.lastRow(), ref["last_row"])


@pytest.mark.parametrize("batch_rows_per_lane", [4, 16], ids=["256rows", "1024rows"])
def test_a_batch_of_goal_sweeps(pkg, oracle, batch_rows_per_lane):
    """three partitions of 4096 x 3072 in ONE launch of mi355sw_align_partitions: two bounds and a partition without one"""
    m, n = 4096, 3072
    s0, s1 = pkg.seqgen.related_pair(3 * m, 3 * n, cfg=72)
    parts = [pkg.Partition(k * m, k * n, (k + 1) * m, (k + 1) * n) for k in range(3)]      # three blocks along the diagonal of a related pair
    refs = [_reference(oracle, s0[p.i0:p.i1], s1[p.j0:p.j1], 64 * batch_rows_per_lane, 0) for p in parts]
    tops = [int(r["last_col"][:, 0].max()) for r in refs]
    bounds = [tops[0] - 200, -INF, tops[2] - 60]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        mgs = [pkg.Stage1Manager(p, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_OR_2,
                                 keep_last_row=True, keep_last_column=True) for p in parts]
        al.setGoalBounds(bounds)
        al.alignPartitions(parts, mgs, rows_per_lane=batch_rows_per_lane)
        st = al.getStatistics()
    finally:
        al.close()
    assert st["kernel"] == "sw_batch_kernel_pk16<%d,false,false,true,true>" % (batch_rows_per_lane // 2), st["kernel"]
    assert st["kernel_launches"] == 1 and st["restarts"] == 0
    for k in (0, 2):
        _check_sweep(mgs[k], refs[k], m, n, bounds[k], "partition %d" % k)
    assert np.array_equal(mgs[1].lastColumn(), refs[1]["last_col"]) and np.array_equal(mgs[1].lastRow(), refs[1]["last_row"])
    print("batch at %d-row strips: pruned %d of %d cells" % (64 * batch_rows_per_lane, st["pruned_cells"], 3 * m * n))
    assert 0 < st["pruned_cells"] <= 2 * m * n and st["pruned_cells"] + st["processed_cells"] == 3 * m * n


def test_a_stop_under_goal_pruning(pkg, oracle):
    """a manager that stops at the first last-column cell >= B + 100: the call returns, what it handed out up to there
    meets the criterion, and rows below the stop were not handed out"""
    m, n = 16401, 1536
    s0, s1, ref = _shared_reference(pkg, oracle, m, n, 256, 8192)
    bound = int(ref["last_col"][:, 0].max()) - 200
    want_stop = int(np.argmax(ref["last_col"][:, 0] >= bound + 100))
    assert 0 < want_stop < m - 4096

    class Stopping(pkg.Stage1Manager):
        def dispatchColumn(self, j, buf, length):
            pkg.Stage1Manager.dispatchColumn(self, j, buf, length)
            if self.active and (np.asarray(buf[:length])[:, 0] >= bound + 100).any():
                self.active = False

    al = pkg.MI355Aligner(device=0, rows_per_lane=4)
    try:
        al.setSequences(s0, s1)
        part = pkg.Partition(0, 0, m, n)
        mg = Stopping(part, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_OR_2,
                      special_row_interval=8192, keep_last_column=True)
        al.setGoalBounds([bound])
        al.alignPartition(part, mg)
        st = al.getStatistics()
    finally:
        al.close()
    got = mg.lastColumn()
    assert st["kernel"].endswith(",true,true>") and not mg.active
    assert want_stop < len(got) <= want_stop + 16 * 256 + 1 < m         # stopped within the chunk (<= 16 strips) that held the cell
    assert_goal_pruned(got, ref["last_col"][:len(got)], 0, bound, "stopped last column", last_column=True)
    assert int(np.argmax(got[:, 0] >= bound + 100)) == want_stop
    cols_left = n - np.arange(0, n + 1)
    want_rows = dict(zip(ref["special_row_ids"], ref["special_rows"]))
    for i in sorted(mg.special_rows):
        assert i < len(got)
        assert_goal_pruned(mg.specialRow(i), want_rows[i], cols_left, bound, "special row %d" % i)


def _pipeline_case(fixture, speculate, limit_s=300):
    env = dict(os.environ, MI355SW_STAGE2_SPECULATE="1" if speculate else "0")
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "goal_prune_pipeline_case.py"), fixture], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=limit_s, env=env)
        rc, log = p.returncode, p.stdout.decode(errors="replace")
    except subprocess.TimeoutExpired as e:
        rc, log = -1, "timed out after %d s\n%s" % (limit_s, (e.stdout or b"").decode(errors="replace"))
    if rc != 0:
        pytest.fail("goal pruning pipeline case %s: exit code %d\n%s" % (fixture, rc, log[-3000:]))
    return json.loads([ln for ln in log.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("speculate", [True, False], ids=["guessed", "chain"])
@pytest.mark.parametrize("fixture", ["full_pipeline_pruned_60000x50000_b8192", "full_pipeline_global_60000x50000_b8192"])
def test_pipeline_with_prune_traceback(fixture, speculate):
    """pipeline.align(prune_traceback=True) on the engine: best, crosspoint_02 / 03 / 04 and alignment.00.txt are the
    reference's; every goal-column sweep of 1024 columns and more skipped cells, and stage 2 processed fewer cells than the
    same run without the option (the ratio is printed: no pass mark beyond "fewer")"""
    res = _pipeline_case(fixture, speculate)
    assert all(res["checks"].values()), res
    print("%s, %s: stage 2 processed %d cells with goal pruning, %d without: ratio %.3f; sweeps %s" % (
        fixture, "guessed crosspoints" if speculate else "plain chain", res["processed_on"], res["processed_off"],
        res["processed_on"] / float(res["processed_off"]), res["sweeps"]))
    assert res["processed_on"] < res["processed_off"]
