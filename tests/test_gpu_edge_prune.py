"""GPU (-m gpu): block pruning of alignments that END ON A SEQUENCE EDGE -- mi355sw_set_prune_end, the EDGE instantiations of the
packed pruning kernels (csrc/sw_kernel_pk16_j.hip / _wj.hip), Stage1Manager(prune_edges=True), stage1 / pipeline.align(prune_edges=True).

The reference never prunes such a run (sw_stage1.cpp:219-225), so the oracle of every pruned run here is the UNPRUNED one:
the best score of the allowed edge is the oracle's, and last row, last column and special rows go through
edge_prune_cases.assert_edge_pruned_cells -- a value v, H or the gap component, is exact wherever v + reach(mode) >= optimum
and the oracle's value or less everywhere else.  (The threaded oracle computes every cell of the semi-global forms but
reports a best cell for the local and global ones only: the optimum is read off its last row / last column.)"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import edge_prune_cases as ec
from helpers import assert_pruned_borders, manager_rows, oracle_kwargs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEEP = os.path.join(ROOT, "masa-cudalign_amd", "libmi355sw_keepnops.so")
THREADS = min(64, os.cpu_count() or 1)
ROWS_PER_LANE = {256: 4, 512: 8, 1024: 16, 2048: 32}
_REF = {}


def unpruned(oracle, key, s0, s1, start, interval=0):
    """every cell a run hands out, from the unpruned oracle with the borders of `start`: computed once per key, left unchanged"""
    if key not in _REF:
        kw = oracle_kwargs(oracle, dict(start=start, end=3, pruning=False, disk=-1, block=(1024, 1 << 20)), len(s0), len(s1))
        kw.update(want_last_row=True, want_last_col=True, special_row_interval=interval, threads=THREADS)
        ref = oracle.stage1(s0, s1, **kw)
        for a in (ref["last_row"], ref["last_col"]):
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def edge_run(pkg, al, m, n, start, end, *, call="manager", interval=0, prune=True, manager_class=None):
    """one partition over the whole matrix through alignPartition.  call: "manager" hands the aligner what the manager says
    (Stage1Manager.pruneEnd, as stage1() does), None makes no call, an int is handed over as it is."""
    part = pkg.Partition(0, 0, m, n)
    mg = (manager_class or pkg.Stage1Manager)(part, alignment_start=start, alignment_end=end, special_row_interval=interval, keep_last_row=True,
                                              keep_last_column=True, block_pruning=prune, prune_edges=prune)
    if call == "manager":
        if mg.pruneEnd():
            al.setPruneEnd(mg.pruneEnd())
    elif call is not None:
        al.setPruneEnd(call)
    al.alignPartition(part, mg)
    return mg, al.getStatistics()


def check_result(mg, ref, m, n, mode):
    """the result cell: the oracle's optimum of the allowed edge, at a cell of that edge that holds it"""
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    i, j, score = mg.getBestScore()
    assert score == opt, (mode, (i, j, score), opt)
    assert (i == m and (mode & 1) and int(ref["last_row"][j, 0]) == opt) or (j == n and (mode & 2) and int(ref["last_col"][i, 0]) == opt), (mode, i, j)
    return opt


def check_pruned_run(mg, st, ref, m, n, mode, *, must_rows=(), pruned=None, where=""):
    """everything a pruned run is held to: result cell, last row, last column, special rows, the cell count, the kernel"""
    opt = check_result(mg, ref, m, n, mode)
    n_must = ec.assert_edge_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, opt, mode, col0=True, must_rows=must_rows, where=where)
    assert n_must > 0
    assert st["pruned_cells"] + st["processed_cells"] == m * n, (where, st["pruned_cells"], st["processed_cells"])
    assert st["profile_kernel"] == 2 and st["kernel_launches"] == 1 and st["restarts"] == 0, (where, st)
    assert st["kernel"].endswith(",true>") and "<%d,false,false,true,false,true>" % (st["strip_rows"] // 128) in st["kernel"], st["kernel"]
    print("%s mode %d %d x %d, %d-row strips: %.4f of the cells skipped, %d values held exact" % (where, mode, m, n, st["strip_rows"], st["pruned_cells"] / float(m) / n, n_must))
    if pruned is True:
        assert st["pruned_cells"] > 0, where
    return opt


# ---------------------------------------------------------------------------------------------------------------------
# 1. each mode at the shape of the ignored-request test (test_gpu_prune_global.py), sweep-grown bound only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ec.MODES)
def test_each_mode_prunes_with_the_bound_the_sweep_grows(pkg, oracle, mode):
    """30 000 x 26 000 related pair, starts + and 3, 256- and 2048-row strips, no first bound: cells are skipped and every
    cell that can matter is the oracle's"""
    m, n = 30000, 26000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=35)
    for rows in (256, 2048):
        al = pkg.MI355Aligner(device=0, rows_per_lane=ROWS_PER_LANE[rows])
        try:
            al.setSequences(s0, s1)
            for start in (4, 3):
                ref = unpruned(oracle, ("t1", start), s0, s1, start)
                mg, st = edge_run(pkg, al, m, n, start, mode)
                assert st["strip_rows"] == rows
                check_pruned_run(mg, st, ref, m, n, mode, pruned=True, where="start %d" % start)
        finally:
            al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the asymmetric term: di - dj changes sign inside the matrix; shapes off the 64-column and strip grids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(9000, 24000), (24000, 9000), (8191, 8257), (8257, 8191)])
def test_the_forced_gap_has_the_right_sign_and_span(pkg, oracle, m, n):
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9600 + m % 7)
    for start, rows in ((4, 256), (1, 512)):
        ref = unpruned(oracle, ("t2", m, n, start), s0, s1, start)
        al = pkg.MI355Aligner(device=0, rows_per_lane=ROWS_PER_LANE[rows])
        try:
            al.setSequences(s0, s1)
            for mode in ec.MODES:
                mg, st = edge_run(pkg, al, m, n, start, mode)
                check_pruned_run(mg, st, ref, m, n, mode, where="start %d" % start)
        finally:
            al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a first bound from the caller, through the streaming form
# ---------------------------------------------------------------------------------------------------------------------
def stream(pkg, al, m, n, *, mode, bound, local=False, interval=0):
    eng = pkg.engine
    if mode:
        al.setPruneEnd(mode)
    init = eng.INIT_WITH_ZEROES if local else eng.INIT_WITH_GAPS
    al.streamBegin(pkg.Partition(0, 0, m, n), recurrence_type=eng.SMITH_WATERMAN if local else eng.NEEDLEMAN_WUNSCH, track_best=local,
                   first_row_init_type=init, first_column_init_type=init, want_last_row=True, want_last_column=True,
                   special_row_interval=interval, prune_blocks=True, initial_bound=bound)
    while not al.streamPoll()[1]:
        time.sleep(0.001)
    out = {"last_row": al.streamReadLastRow(), "last_col": al.streamReadColumn(0, m)}
    out["best"] = al.streamEnd()[0]
    out["stats"] = al.getStatistics()
    return out


@pytest.mark.parametrize("mode", ec.MODES)
def test_a_run_that_starts_from_its_optimum(pkg, oracle, mode):
    """12 000 x 10 000, streamBegin(initial_bound = optimum): the result is exact and at least half as many cells go as the
    same pair skips as a local alignment from ITS optimum at the same height (the edge bound is higher and the values carry
    no floor: the rule can only skip more; the half is the margin); optimum + 1 is refused with MI355SW_EBOUND"""
    m, n = 12000, 10000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9700)
    ref = unpruned(oracle, "t3", s0, s1, 4)
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    if "t3sw" not in _REF:
        _REF["t3sw"] = oracle.stage1(s0, s1, threads=THREADS)["best"][2]
    al = pkg.MI355Aligner(device=0, rows_per_lane=8)
    try:
        al.setSequences(s0, s1)
        local = stream(pkg, al, m, n, mode=0, bound=_REF["t3sw"], local=True)
        assert local["best"][2] == _REF["t3sw"] and local["stats"]["pruned_cells"] > 0
        got = stream(pkg, al, m, n, mode=mode, bound=opt)
        st = got["stats"]
        assert ec.edge_optimum(mode, got["last_row"], got["last_col"]) == opt
        ec.assert_edge_pruned_cells(got["last_row"], ref["last_row"][1:], m, np.arange(1, n + 1), m, n, opt, mode, where="last row")
        ec.assert_edge_pruned_cells(got["last_col"], ref["last_col"][1:], np.arange(1, m + 1), n, m, n, opt, mode, where="last column")
        assert st["kernel"].endswith(",false,true>") and st["profile_kernel"] == 2 and st["kernel_launches"] == 1
        assert st["pruned_cells"] + st["processed_cells"] == m * n
        print("mode %d: %d cells skipped from the optimum, the local run %d" % (mode, st["pruned_cells"], local["stats"]["pruned_cells"]))
        assert 2 * st["pruned_cells"] >= local["stats"]["pruned_cells"]
        with pytest.raises(pkg.AlignerError, match="EBOUND"):
            stream(pkg, al, m, n, mode=mode, bound=opt + 1)
        again = stream(pkg, al, m, n, mode=mode, bound=opt)              # the engine stays usable
        assert ec.edge_optimum(mode, again["last_row"], again["last_col"]) == opt
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. seeded shapes
# ---------------------------------------------------------------------------------------------------------------------
F_WIDE = 65536          # MI355SW_F_WIDE_ALPHABET


def _shape(k):
    rng = np.random.default_rng(9800 + k)
    m = int(rng.integers(2000, 30001))
    n = int(np.clip(m * rng.uniform(0.6, 1.5), 2000, 30000))
    rows = (0, 256, 512, 1024, 2048)[k % 5]
    kind = k % 4                        # 0: unrelated, 1..3: related of three divergences
    wide = k in (5, 10)
    start = (4, 3, 1, 2)[(k // 2) % 4]
    return m, n, rows, kind, wide, start


@pytest.mark.parametrize("k", range(12))
def test_seeded_shapes(pkg, oracle, k):
    """twelve seeded shapes from 2 000 to 30 000: every height (and the engine's choice), three divergences, unrelated pairs,
    the wide form with a 20-letter pair, every start form -- each mode held to the oracle"""
    m, n, rows, kind, wide, start = _shape(k)
    if wide:
        from test_gpu_wide_alphabet import wide_pair, POOL
        s0, s1 = wide_pair(pkg, m, n, POOL[:20], cfg=9800 + k, ensure=True)
    elif kind == 0:
        s0, s1 = pkg.seqgen.unrelated_pair(m, n, cfg=9800 + k)
    else:
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9800 + k, p_sub=[0.0, 0.01, 0.05, 0.15][kind], p_indel=[0.0, 0.001, 0.004, 0.01][kind])
    ref = unpruned(oracle, ("t4", k), s0, s1, start)
    al = pkg.MI355Aligner(device=0, rows_per_lane=ROWS_PER_LANE.get(rows, 0), flags=F_WIDE if wide else 0)
    try:
        al.setSequences(s0, s1)
        for mode in ec.MODES:
            mg, st = edge_run(pkg, al, m, n, start, mode)
            assert st["strip_rows"] in ROWS_PER_LANE and (rows == 0 or st["strip_rows"] == rows)
            assert ("_wide<" in st["kernel"]) == wide
            check_pruned_run(mg, st, ref, m, n, mode, where="shape %d start %d" % (k, start))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. special rows, and a resume from one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ec.MODES)
def test_special_rows_and_a_resume_from_one(pkg, oracle, tmp_path, mode):
    """40 000 x 36 000, special rows every 8 192 rows: every row above the end of the optimal alignment holds values the run
    is held to.  Then stage1(prune_edges=True) dies inside its third special row and is resumed: the rest of the matrix
    runs as a partition of its own under the whole matrix as super-partition, from a first row that a pruned run wrote --
    the same optimum, and the rows it leaves on disk are held to the oracle like the others"""
    from masa_cudalign_amd import sra as sra_mod
    m, n, start = 40000, 36000, 4
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9900)
    ref = unpruned(oracle, "t5", s0, s1, start, interval=8192)
    opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
    # rows the optimal alignment crosses: all of them when it ends on the last row, else those above its last-column cell
    end_row = m if (mode & 1) and int(ref["last_row"][:, 0].max()) == opt else int(np.argmax(ref["last_col"][:, 0] == opt))
    must_rows = [i for i in ref["special_row_ids"] if i <= end_row and i < m]
    assert len(must_rows) >= 3
    al = pkg.MI355Aligner(device=0, rows_per_lane=16)
    try:
        al.setSequences(s0, s1)
        mg, st = edge_run(pkg, al, m, n, start, mode, interval=8192)
        assert sorted(i for i in mg.special_rows if i < m) == [i for i in ref["special_row_ids"] if i < m]
        check_pruned_run(mg, st, ref, m, n, mode, must_rows=must_rows, where="special rows")
        al.unsetSequences()

        class Killed(Exception):
            pass

        class DyingManager(pkg.Stage1Manager):
            dead = False

            def dispatchRow(self, i, buf, length):
                if DyingManager.dead:
                    return
                pkg.Stage1Manager.dispatchRow(self, i, buf, length)
                if len(self.sra.rows) >= 2 and length > 1:
                    DyingManager.dead = True
                    self.active = False
                    raise Killed()

        work = str(tmp_path / "work")
        limit = 8 * (n + 1) * 8
        with pytest.raises(Killed):
            pkg.stage1(al, s0, s1, work, alignment_start=start, alignment_end=mode, sra_limit=limit, prune_edges=True, manager_class=DyingManager)
        keep = sra_mod.Status(work).last_special_row
        assert keep == 2 * 8192
        res = pkg.stage1(al, s0, s1, work, alignment_start=start, alignment_end=mode, sra_limit=limit, prune_edges=True)
        st = al.getStatistics()
        assert res["resumed_from"] == keep and res["best"][2] == opt
        assert st["kernel"].endswith(",false,true>") and st["pruned_cells"] + st["processed_cells"] == (m - keep) * n
        part = sra_mod.get_area(None, work, 1, 0, disk_limit=limit).create_partition(0, 0, m, n)
        rows = {i: part.read_row(i) for i in (part.i0 + r for r in part.rows) if keep < i < m}
        assert sorted(rows) == [i for i in ref["special_row_ids"] if keep < i < m]
        assert ec.assert_edge_pruned_borders(rows, None, None, ref, m, n, opt, mode, col0=True, must_rows=[i for i in must_rows if i > keep], where="resumed") > 0
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. ignored and refused requests
# ---------------------------------------------------------------------------------------------------------------------
def test_requests_the_edge_kernels_do_not_serve(pkg, oracle):
    """forced int32, a fixed 768-row height, a local recurrence, a tracking manager: every cell is the oracle's and nothing is
    skipped; mode 7 is MI355SW_EINVAL; a manager that asks without anybody naming the edge gets today's answer -- every cell"""
    m, n = 30000, 26000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=35)

    def exact(mg, st, ref, mode=None):
        assert st["pruned_cells"] == 0 and st["processed_cells"] == m * n and not st["kernel"].endswith(",false,true>"), st
        assert np.array_equal(mg.lastRow(), ref["last_row"]) and np.array_equal(mg.lastColumn(), ref["last_col"])
        if mode:
            check_result(mg, ref, m, n, mode)

    ref = unpruned(oracle, ("t1", 4), s0, s1, 4)
    for kw in (dict(flags=2, rows_per_lane=8), dict(rows_per_lane=12)):          # MI355SW_F_FORCE_INT32; 768-row strips
        al = pkg.MI355Aligner(device=0, **kw)
        try:
            al.setSequences(s0, s1)
            for mode in ec.MODES:
                mg, st = edge_run(pkg, al, m, n, 4, mode)
                exact(mg, st, ref, mode)
        finally:
            al.close()
    al = pkg.MI355Aligner(device=0, rows_per_lane=8)
    try:
        al.setSequences(s0, s1)
        # no call: the manager asks, nobody names the edge (test_gpu_prune_global.py's ignored request)
        for mode in ec.MODES:
            mg, st = edge_run(pkg, al, m, n, 4, mode, call=None)
            exact(mg, st, ref, mode)
        # a value outside 0..3
        with pytest.raises(pkg.AlignerError, match="EINVAL"):
            al.setPruneEnd(7)
        with pytest.raises(pkg.AlignerError, match="EINVAL"):
            al.setPruneEnd(-1)
        mg, st = edge_run(pkg, al, m, n, 4, 1, call=None)                       # (a refused value leaves nothing behind)
        exact(mg, st, ref, 1)
        # a local recurrence that ends on an edge (*3) with the edge named: neither the local rule nor the edge rule holds
        kw = oracle_kwargs(oracle, dict(start=0, end=3, pruning=False, disk=-1, block=(1024, 1 << 20)), m, n)
        kw.update(want_last_row=True, want_last_col=True, threads=THREADS)
        ref_sw = oracle.stage1(s0, s1, **kw)
        part = pkg.Partition(0, 0, m, n)
        mg = pkg.Stage1Manager(part, alignment_start=pkg.AT_ANYWHERE, alignment_end=pkg.AT_SEQUENCE_1_OR_2, keep_last_row=True, keep_last_column=True)
        mg.block_pruning = True
        al.setPruneEnd(3)
        al.alignPartition(part, mg)
        exact(mg, al.getStatistics(), ref_sw)
        assert mg.getBestScore()[2] == ec.edge_optimum(3, ref_sw["last_row"], ref_sw["last_col"])

        # a manager that tracks scores next to its edge
        class Tracking(pkg.Stage1Manager):
            def mustDispatchScores(self):
                return True
        mg, st = edge_run(pkg, al, m, n, 4, 3, manager_class=Tracking)
        exact(mg, st, ref)
        # the last-cell rule is untouched by a word about edges: a global manager keeps it
        part = pkg.Partition(0, 0, m, n)
        mg = pkg.Stage1Manager(part, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_AND_2, keep_last_row=True, keep_last_column=True, block_pruning=True)
        al.setPruneEnd(1)
        al.alignPartition(part, mg)
        st = al.getStatistics()
        final = int(ref["last_row"][-1, 0])
        assert tuple(mg.getBestScore()) == (m, n, final) and st["kernel"].endswith("<4,false,false,true>")
        assert assert_pruned_borders({}, mg.lastRow(), mg.lastColumn(), ref, m, n, final, pkg.NEEDLEMAN_WUNSCH, col0=True, where="global") > 0
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the diagonal seed as the first bound
# ---------------------------------------------------------------------------------------------------------------------
def test_the_global_seed_is_a_first_bound_of_every_mode(pkg, oracle):
    """seedBound(whole matrix, NEEDLEMAN_WUNSCH) at 65 536 x 16 384, its smallest size: the score of a corner-to-corner
    alignment is no more than the optimum of any mode, and the run started from it returns that optimum"""
    m, n = 65536, 16384
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9950)
    ref = unpruned(oracle, "t7", s0, s1, 4)
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        seed = al.seedBound(pkg.Partition(0, 0, m, n), pkg.NEEDLEMAN_WUNSCH)
        assert seed is not None and seed <= int(ref["last_row"][-1, 0])
        for mode in ec.MODES:
            opt = ec.edge_optimum(mode, ref["last_row"], ref["last_col"])
            assert seed <= opt
            got = stream(pkg, al, m, n, mode=mode, bound=seed)
            assert ec.edge_optimum(mode, got["last_row"], got["last_col"]) == opt
            ec.assert_edge_pruned_cells(got["last_row"], ref["last_row"][1:], m, np.arange(1, n + 1), m, n, opt, mode, where="last row")
            ec.assert_edge_pruned_cells(got["last_col"], ref["last_col"][1:], np.arange(1, m + 1), n, m, n, opt, mode, where="last column")
            assert got["stats"]["kernel"].endswith(",false,true>") and got["stats"]["strip_rows"] in ROWS_PER_LANE
            print("mode %d: seed %d, optimum %d, %.4f of the cells skipped" % (mode, seed, opt, got["stats"]["pruned_cells"] / float(m) / n))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the whole pipeline
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", ["+3", "33", "13"])
def test_the_pipeline_leaves_the_same_files(pkg, oracle, tmp_path, edges):
    """pipeline.align(prune_edges=True) at 60 000 x 50 000: best, crosspoint_02 / 03 / 04 and alignment.00.txt are those of
    the run with the option off, stage 1's best is the oracle's, and stage 1 ran the edge kernels and skipped cells"""
    from masa_cudalign_amd import fasta, pipeline
    code = {"1": 1, "2": 2, "3": 3, "+": 4}
    start, end = code[edges[0]], code[edges[1]]
    m, n = 60000, 50000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9960)
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    ref = unpruned(oracle, ("t8", start), s0, s1, start)
    opt = ec.edge_optimum(end, ref["last_row"], ref["last_col"])
    files = {}
    for on in (False, True):
        work = str(tmp_path / ("on" if on else "off"))
        al = pkg.MI355Aligner(device=0)
        try:
            out = pipeline.align(al, q0, q1, work, alignment_start=start, alignment_end=end, sra_limit=8 * (n + 1) * 8, prune_edges=on)
        finally:
            al.close()
        assert out["best"][2] == opt
        assert (out["stage1"]["pruned_cells"] > 0) == on
        found = {}
        for root, _, fns in os.walk(work):
            for fn in fns:
                if fn in ("alignment.00.txt", "crosspoint_02.00", "crosspoint_03.00", "crosspoint_04.00"):
                    found[fn] = open(os.path.join(root, fn), "rb").read()
        assert sorted(found) == ["alignment.00.txt", "crosspoint_02.00", "crosspoint_03.00", "crosspoint_04.00"], sorted(found)
        files[on] = (tuple(out["best"]), found)
    assert files[True][0] == files[False][0]
    for fn in files[True][1]:
        assert files[True][1][fn] == files[False][1][fn], fn
    assert len(files[True][1]["alignment.00.txt"]) > 30000


# ---------------------------------------------------------------------------------------------------------------------
# 9. both builds: the library as shipped and the one with the compiler's wait states left in
# ---------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
import __graft_entry__ as graft
import test_gpu_edge_prune as T
pkg = graft.load_package()
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()
out = {"library": pkg.engine.LIB_PATH, "build_id": pkg.engine.library_build_id(), "cases": []}
# the shapes and modes of two of the runs above, with reproducible pruning: which slabs go -- and with it every byte handed out --
# is then a function of the input, and the two builds can be compared output by output.  (16 wavefronts: a reproducible run
# holds a strip against what the strips `waves` and more above it found, and these matrices are 50 to 120 strips tall.)
for (m, n, cfg, rows, start, mode, flags) in ((30000, 26000, 35, 256, 4, 1, 0), (24000, 9000, 9600 + 24000 %% 7, 512, 1, 3, 0)):
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=cfg)
    al = pkg.MI355Aligner(device=0, rows_per_lane=T.ROWS_PER_LANE[rows], waves=16, flags=flags | pkg.engine.F_DETERMINISTIC_PRUNE)
    try:
        al.setSequences(s0, s1)
        mg, st = T.edge_run(pkg, al, m, n, start, mode, interval=8192)
        out["cases"].append({"best": list(mg.getBestScore()), "kernel": st["kernel"], "restarts": st["restarts"], "pruned_cells": st["pruned_cells"],
                             "last_row": sha(mg.lastRow()), "last_col": sha(mg.lastColumn()),
                             "special": {str(i): sha(mg.specialRow(i)) for i in sorted(mg.special_rows)}})
    finally:
        al.close()
print(json.dumps(out))
"""


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["MI355SW_LIB"] = lib
    else:
        env.pop("MI355SW_LIB", None)
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "here": HERE}], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])


def test_both_builds_agree_on_edge_runs():
    """tests/test_gpu_nops.py for the edge kernels, after test_gpu_wide_alphabet.py::test_both_builds_agree_on_wide_pairs: each
    build in a child process of its own, every output equal"""
    if not os.path.exists(KEEP):
        pytest.fail("libmi355sw_keepnops.so is not built (make -C masa-cudalign_amd/csrc keepnops; __graft_entry__.build() does it)")
    a, b = _child(None), _child(KEEP)
    assert a["library"] != b["library"] and b["library"] == KEEP
    assert a["build_id"] == b["build_id"]
    assert len(a["cases"]) == len(b["cases"]) == 2
    for x, y in zip(a["cases"], b["cases"]):
        assert x["pruned_cells"] > 0 and y["pruned_cells"] > 0
        # (the skipped-cell count of a pruned run is bookkeeping that may differ by a few slabs from run to run; every byte
        #  handed out must be equal)
        x.pop("pruned_cells"), y.pop("pruned_cells")
        assert x == y, (x, y)
        assert x["kernel"].endswith(",false,true>") and x["restarts"] == 0
