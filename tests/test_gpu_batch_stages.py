"""GPU: mi355sw_align_partitions the way stages 2 and 3 drive it.  test_gpu_batch.py checks the batch against single calls
on the easy case (engine-made borders, special rows on the 8192-row grid, one small launch); here every partition of a
batch is held against BOTH the C oracle (int32, the same borders handed over as custom data) and a single
alignPartition call on the same aligner, at the settings where the batched path and the single-call path can part:
special-row spacings that round differently on the 256-, 512-, 1024- and 2048-row grids, custom and streamed borders
far from zero, managers that say stop, more partitions than one launch takes, overflow reruns, strip heights that
change between calls, and stage 2's sweeps from guessed crosspoints on the engine itself."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = 16            # oracle threads: a GPU host grants 16 CPUs per command, os.cpu_count() reports the whole machine
ENGINE_GRID = 2048      # special-row unit where the engine picks the strip height (runtime.cpp, plan_geometry)
OFFSET = 120_000_000    # special-row values deep in a C5-sized alignment


def _mgr_class(pkg):
    class Mgr(pkg.Stage1Manager):
        """Stage1Manager that counts its first-column stream, notes the order in which special rows arrive, can say stop
        once its last column has passed a row (AlignerManager at a goal) and can refuse scores (SW without tracking)"""

        def __init__(self, part, stop_at=None, no_scores=False, **kw):
            pkg.Stage1Manager.__init__(self, part, **kw)
            self.stop_at, self.no_scores = stop_at, no_scores
            self.col_asked = 0
            self.row_order = []
            self.pkg = pkg

        def receiveFirstColumn(self, buf, length):
            self.col_asked += length
            pkg.Stage1Manager.receiveFirstColumn(self, buf, length)

        def dispatchColumn(self, j, buf, length):
            pkg.Stage1Manager.dispatchColumn(self, j, buf, length)
            if self.stop_at is not None and self.last_column_pos > self.stop_at:
                self.active = False

        def dispatchRow(self, i, buf, length):
            if i not in self.special_rows:
                self.row_order.append(i)
            pkg.Stage1Manager.dispatchRow(self, i, buf, length)

        def mustDispatchScores(self):
            return False if self.no_scores else pkg.Stage1Manager.mustDispatchScores(self)
    return Mgr


class Case:
    """one partition of a batch.  kind: "goal" (NW from a crosspoint, last column only: what stage 2 and 3 sweep), "nw"
    (global, last cell), "semi" (NW, best anywhere: scores tracked), "sw", "sw_quiet" (SW, no scores).  row / col:
    factories of custom border readers (None: the kind's own gap or zero borders)."""

    def __init__(self, part, kind, interval=0, row=None, col=None, stop_at=None):
        self.part, self.kind, self.interval, self.row, self.col, self.stop_at = part, kind, interval, row, col, stop_at

    @property
    def m(self):
        return self.part.i1 - self.part.i0

    @property
    def n(self):
        return self.part.j1 - self.part.j0

    def empty(self):
        return self.m <= 0 or self.n <= 0

    def nw(self):
        return self.kind in ("goal", "nw", "semi")

    def tracked(self):
        return self.kind in ("semi", "sw")

    def manager(self, pkg, stop=True):
        kw = dict(keep_last_row=True, keep_last_column=True, special_row_interval=self.interval)
        if self.kind == "goal":
            kw.update(alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_2)
        elif self.kind == "nw":
            kw.update(alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_AND_2)
        elif self.kind == "semi":
            kw.update(alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_ANYWHERE)
        if self.row is not None:
            kw["first_row_reader"] = self.row()
        if self.col is not None:
            kw["first_column_reader"] = self.col()
        return _mgr_class(pkg)(self.part, stop_at=self.stop_at if stop else None, no_scores=self.kind == "sw_quiet", **kw)

    def borders(self, pkg):
        """the cells the manager's readers hand out (corner included), from readers of their own"""
        mg = self.manager(pkg)
        row = np.zeros((self.n + 1, 2), dtype=np.int32)
        col = np.zeros((self.m + 1, 2), dtype=np.int32)
        mg.first_row_reader.read(row, self.n + 1)
        mg.first_column_reader.read(col, self.m + 1)
        return row, col


class Refs(dict):
    """oracle results of one test, by partition, kind, spacing and grid"""

    def __init__(self, pkg, oracle, s0, s1):
        dict.__init__(self)
        self.pkg, self.oracle, self.s0, self.s1 = pkg, oracle, s0, s1

    def __call__(self, case, block_h=2048):
        return _oracle(self, case, block_h)


def _oracle(_REF, case, block_h):
    pkg, oracle, s0, s1 = _REF.pkg, _REF.oracle, _REF.s0, _REF.s1
    p = case.part
    key = (p.i0, p.j0, p.i1, p.j1, case.kind, case.interval, block_h, id(case.row), id(case.col))
    if key not in _REF:
        row, col = case.borders(pkg)
        best = oracle.BEST_LAST_CELL if case.kind == "nw" else oracle.BEST_ANYWHERE
        _REF[key] = oracle.stage1(s0[p.i0:p.i1], s1[p.j0:p.j1], recurrence=oracle.NEEDLEMAN_WUNSCH if case.nw() else oracle.SMITH_WATERMAN,
                                  first_row_type=oracle.INIT_WITH_CUSTOM_DATA, first_col_type=oracle.INIT_WITH_CUSTOM_DATA,
                                  custom_first_row=row, custom_first_col=col, block_h=block_h, block_w=1024,
                                  special_row_interval=case.interval, want_last_row=True, want_last_col=True, best_mode=best,
                                  threads=THREADS)
    return _REF[key]


def _special(case, mg):
    """special rows the manager received ABOVE its last row, relative to the partition: {dp row: [chunks]}"""
    return {i - case.part.i0: v for i, v in mg.special_rows.items() if i < case.part.i1}


def _delivered_once(case, mg):
    rows = [i for i in mg.row_order if i < case.part.i1]
    assert rows == sorted(set(rows)), rows                           # in order, none twice
    for i, chunks in _special(case, mg).items():
        assert len(chunks) == 2, (i, len(chunks))                    # the leading cell + the row: ONE delivery


def _expect_oracle(case, mg, ref, what=""):
    """a manager that ran to its end against the oracle, in full"""
    assert np.array_equal(mg.lastColumn(), ref["last_col"]), ("last column", what)
    assert np.array_equal(mg.lastRow(), ref["last_row"]), ("last row", what)
    if case.tracked() or case.kind == "nw":
        # the oracle's best cell through a manager of the same kind (its own rules: a minimum score, the last cell only)
        bi, bj, bs = ref["best"]
        want = case.manager(mg.pkg)
        if bs > -mg.pkg.INF:
            want.dispatchScore((case.part.i0 + bi - 1, case.part.j0 + bj - 1, bs))
        assert tuple(mg.getBestScore()) == tuple(want.getBestScore()), (mg.getBestScore(), want.getBestScore(), ref["best"], what)
    want = {r: ref["special_rows"][k] for k, r in enumerate(ref["special_row_ids"]) if r < case.m}
    got = _special(case, mg)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want), what)
    for r in want:
        assert np.array_equal(np.concatenate(got[r]), want[r]), (r, what)
    _delivered_once(case, mg)
    if mg.getFirstColumnInitType() == mg.pkg.INIT_WITH_CUSTOM_DATA:
        assert mg.col_asked == case.m + 1, (mg.col_asked, case.m + 1, what)    # streamed: read once, corner + every row
    else:
        assert mg.col_asked <= case.m + 1, (mg.col_asked, what)                # a gap run: made on the device


def _expect_stopped(case, mg, ref, what=""):
    """a manager that said stop: what it received is the oracle's, in order, once"""
    got = mg.lastColumn()
    assert case.stop_at < len(got) <= case.m + 1, (len(got), what)
    assert np.array_equal(got, ref["last_col"][:len(got)]), ("last column", what)
    want = {r: ref["special_rows"][k] for k, r in enumerate(ref["special_row_ids"]) if r < case.m}
    for r, chunks in _special(case, mg).items():
        assert r in want, (r, sorted(want), what)
        assert np.array_equal(np.concatenate(chunks), want[r]), (r, what)
    _delivered_once(case, mg)
    assert mg.col_asked <= case.m + 1


def _expect_same(case, a, b, what=""):
    """batched manager a against the single call's manager b"""
    assert tuple(a.getBestScore()) == tuple(b.getBestScore()), (a.getBestScore(), b.getBestScore(), what)
    assert np.array_equal(a.lastRow(), b.lastRow()), ("last row", what)
    assert np.array_equal(a.lastColumn(), b.lastColumn()), ("last column", what)
    assert sorted(a.special_rows) == sorted(b.special_rows), (sorted(a.special_rows), sorted(b.special_rows), what)
    for k in a.special_rows:
        assert np.array_equal(np.concatenate(a.special_rows[k]), np.concatenate(b.special_rows[k])), (k, what)


def _run(pkg, al, cases, R=None, single=True):
    """the cases through single calls (optional) and then through one alignPartitions call at batch height R"""
    singles, stats = None, []
    if single:
        singles = []
        for c in cases:
            mg = c.manager(pkg)
            al.alignPartition(c.part, mg)
            singles.append(mg)
            stats.append(al.getStatistics())
    batch = [c.manager(pkg) for c in cases]
    al.alignPartitions([c.part for c in cases], batch, **({} if R is None else {"rows_per_lane": R}))
    return singles, batch, al.getStatistics(), stats


def _custom_col(m, corner, seed, INF):
    """m + 1 first-column cells: the corner, then an irregular, steep walk (no gap run: streamed from the host)"""
    rng = np.random.RandomState(seed)
    c = np.zeros((m + 1, 2), dtype=np.int32)
    c[0, 0] = corner
    c[1:, 0] = corner + np.cumsum(rng.randint(-7, 2, m))
    c[:, 1] = -INF
    return c


def _jump_cells(length, at, low, high, INF):
    c = np.zeros((length + 1, 2), dtype=np.int32)
    c[:, 0] = low
    c[at:, 0] = high
    c[:, 1] = -INF
    return c


# ---------------------------------------------------------------------------------------------------------------------
# A. the special-row grid
# ---------------------------------------------------------------------------------------------------------------------
INTERVALS = (8192, 8500, 9300, 12000)


def _grid_cases(pkg, intervals=INTERVALS):
    cases = []
    for iv in intervals:
        cases.append(Case(pkg.Partition(0, 1000, 26000, 3500), "goal", iv))       # m >= 4 n, n >= 2048: a goal sweep's shape
        cases.append(Case(pkg.Partition(5000, 8000, 29000, 14000), "nw", iv))
        cases.append(Case(pkg.Partition(30000, 20000, 55000, 25000), "sw", iv))
    return cases


@pytest.mark.parametrize("R", [4, 8, 16])
def test_batched_special_rows_follow_an_engine_picked_height(pkg, oracle, R):
    """aligner at engine-picked heights (the pipeline's setting): whatever the batch's strip height, its special rows sit
    where a single call puts them -- on the 2048-row grid -- for spacings that round differently on 256-, 512-, 1024- and
    2048-row grids (8500: 8704 / 9216 / 10240 rows)"""
    s0, s1 = pkg.seqgen.related_pair(60000, 40000, cfg=81)
    refs = Refs(pkg, oracle, s0, s1)
    cases = _grid_cases(pkg)
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        singles, batch, st, sst = _run(pkg, al, cases, R)
    finally:
        al.close()
    assert st["strip_rows"] == 64 * R and st["kernel"].startswith("sw_batch_kernel_pk16<%d," % (R // 2))
    for c, s in zip(cases, sst):
        if c.kind == "goal":
            assert s["strip_rows"] == 256, s["strip_rows"]       # recognised as a goal sweep: its height is the engine's
    for k, c in enumerate(cases):
        what = (k, c.kind, c.interval)
        ref = refs(c, ENGINE_GRID)
        _expect_oracle(c, singles[k], ref, what)
        _expect_oracle(c, batch[k], ref, what)
        _expect_same(c, batch[k], singles[k], what)
    # the case keeps its point: at least one spacing puts rows where the batch's own grid would not
    assert any(10240 in _special(c, b) for c, b in zip(cases, batch) if c.interval == 8500)


@pytest.mark.parametrize("R", [4, 8, 16])
def test_batched_special_rows_follow_a_fixed_height(pkg, oracle, R):
    """aligner with a fixed strip height equal to the batch's: the rows of both sit on multiples of that height"""
    s0, s1 = pkg.seqgen.related_pair(60000, 40000, cfg=81)
    refs = Refs(pkg, oracle, s0, s1)
    cases = _grid_cases(pkg, (9300,))
    al = pkg.MI355Aligner(device=0, rows_per_lane=R)
    try:
        al.setSequences(s0, s1)
        singles, batch, st, _ = _run(pkg, al, cases, R)
    finally:
        al.close()
    for k, c in enumerate(cases):
        ref = refs(c, 64 * R)
        _expect_oracle(c, batch[k], ref, (k, c.kind))
        _expect_same(c, batch[k], singles[k], (k, c.kind))


# ---------------------------------------------------------------------------------------------------------------------
# B. custom borders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 16])
def test_batched_custom_borders(pkg, oracle, R):
    """custom first rows (a special row of a larger run, lifted to +-1.2e8), streamed irregular first columns, gap borders
    that start deep into their sequence (InitialCellsReader offsets), and a first-row jump no 16-bit window holds"""
    from masa_cudalign_amd.manager import ArrayCellsReader, InitialCellsReader
    INF = pkg.INF
    s0, s1 = pkg.seqgen.related_pair(60000, 40000, cfg=82)
    refs = Refs(pkg, oracle, s0, s1)
    # a real row: special row 8192 of an oracle run over s0[:16384] x s1[4000:9000]
    big = oracle.stage1(s0[:16384], s1[4000:9000], block_h=2048, special_row_interval=8192, threads=THREADS)
    real = big["special_rows"][0]                                         # 5001 cells, corner included
    assert big["special_row_ids"][0] == 8192 and len(np.unique(real[:, 0])) > 50

    def lifted(off):
        r = real.copy()
        r[:, 0] += off
        return r

    rows = {off: lifted(off) for off in (OFFSET, -OFFSET)}
    cols = {off: _custom_col(30000, int(rows[off][0, 0]), 7 + (off > 0), INF) for off in (OFFSET, -OFFSET)}
    sw_col = np.zeros((20001, 2), dtype=np.int32)
    sw_col[1:, 0] = np.random.RandomState(9).randint(0, 60, 20000)
    sw_col[:, 1] = -INF
    jump = _jump_cells(5000, 2500, 0, 90000, INF)
    cases = [
        Case(pkg.Partition(10000, 4000, 40000, 9000), "nw", 9300, row=lambda: ArrayCellsReader(rows[OFFSET]),
             col=lambda: ArrayCellsReader(cols[OFFSET])),
        Case(pkg.Partition(20000, 30000, 50000, 35000), "semi", 8500, row=lambda: ArrayCellsReader(rows[-OFFSET]),
             col=lambda: ArrayCellsReader(cols[-OFFSET])),
        Case(pkg.Partition(30000, 10000, 50000, 16000), "sw", 9300, col=lambda: ArrayCellsReader(sw_col)),
        Case(pkg.Partition(0, 20000, 26000, 26000), "nw", 12000, row=lambda: InitialCellsReader(0, 2, OFFSET // 2),
             col=lambda: InitialCellsReader(0, 2, OFFSET // 2)),                           # INIT_WITH_GAPS_OPENED at -1.2e8
        Case(pkg.Partition(5000, 0, 29000, 5000), "semi", 9300, row=lambda: InitialCellsReader(3, 2, OFFSET // 2 - 999),
             col=lambda: InitialCellsReader(3, 2, OFFSET // 2 - 999)),                     # INIT_WITH_GAPS, same corner
        Case(pkg.Partition(1000, 31000, 24000, 36000), "sw", 8500, row=lambda: InitialCellsReader(0, 2, 777),
             col=lambda: InitialCellsReader(3, 2, 12345)),                                 # SW clips them: every start offset
        Case(pkg.Partition(40000, 34000, 52000, 39000), "sw", 0, row=lambda: ArrayCellsReader(jump)),  # 0 -> 90 000 step
    ]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        singles, batch, st, sst = _run(pkg, al, cases, R)
    finally:
        al.close()
    assert sst[-1]["restarts"] == 1                  # the jump: reported by the packed kernel, repaired by the int32 rerun ...
    assert st["restarts"] >= 1                       # ... in the batch as well
    for k, c in enumerate(cases):
        ref = refs(c, ENGINE_GRID)
        _expect_oracle(c, singles[k], ref, ("single", k))
        _expect_oracle(c, batch[k], ref, ("batch", k))
        _expect_same(c, batch[k], singles[k], k)


# ---------------------------------------------------------------------------------------------------------------------
# C. goal stops
# ---------------------------------------------------------------------------------------------------------------------
def test_batched_goal_stops_and_the_call_after(pkg, oracle):
    """managers that say stop once their last column has passed a row, beside managers that run to the end; then a second
    call on the same aligner (the pool's sub-handles again) in which nobody stops"""
    s0, s1 = pkg.seqgen.related_pair(70000, 40000, cfg=83)
    refs = Refs(pkg, oracle, s0, s1)
    cases = [
        Case(pkg.Partition(0, 0, 40000, 4000), "goal", 9300, stop_at=23000),
        Case(pkg.Partition(5000, 6000, 45000, 9000), "goal", 8500, stop_at=12500),
        Case(pkg.Partition(20000, 10000, 60000, 14000), "goal", 9300),
        Case(pkg.Partition(10000, 15000, 35000, 18000), "nw", 8192, stop_at=3000),
        Case(pkg.Partition(30000, 20000, 60000, 25000), "sw", 12000),
        Case(pkg.Partition(1000, 26000, 70000, 29000), "goal", 9300, stop_at=40000),
        Case(pkg.Partition(2000, 30000, 22000, 35000), "semi", 9300),
    ]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        batch = [c.manager(pkg) for c in cases]
        al.alignPartitions([c.part for c in cases], batch, rows_per_lane=8)
        again = [c.manager(pkg, stop=False) for c in cases]
        al.alignPartitions([c.part for c in cases], again, rows_per_lane=8)
    finally:
        al.close()
    for k, c in enumerate(cases):
        ref = refs(c, ENGINE_GRID)
        if c.stop_at is not None:
            _expect_stopped(c, batch[k], ref, ("stopped", k))
            assert len(batch[k].lastColumn()) < c.m + 1            # it did stop
        else:
            _expect_oracle(c, batch[k], ref, ("running", k))
        _expect_oracle(c, again[k], ref, ("second call", k))


# ---------------------------------------------------------------------------------------------------------------------
# D. more than BATCH_MAX partitions
# ---------------------------------------------------------------------------------------------------------------------
BATCH_MAX = 256


def test_more_partitions_than_one_launch_takes(pkg, oracle):
    """~300 small partitions of all four kernel variants (NW / SW, with and without scores), zero-area and stopped ones
    among them: two chunks of launches, sub-handles reused within the call; every manager exact"""
    s0, s1 = pkg.seqgen.related_pair(20000, 20000, cfg=84)
    refs = Refs(pkg, oracle, s0, s1)
    rng = np.random.RandomState(11)
    kinds = ("nw", "semi", "sw", "sw_quiet")
    cases = []
    for k in range(300):
        if k % 41 == 7:
            i0, j0 = int(rng.randint(0, 19000)), int(rng.randint(0, 19000))
            cases.append(Case(pkg.Partition(i0, j0, i0 + (k % 2) * 50, j0 + (1 - k % 2) * 50), "nw"))   # zero area
            continue
        h, w = int(rng.randint(1, 2600)), int(rng.randint(1, 700))
        i0, j0 = int(rng.randint(0, 20000 - h)), int(rng.randint(0, 20000 - w))
        kind = kinds[k % 4]
        stop = int(h // 3) if (k % 29 == 3 and h > 700) else None
        cases.append(Case(pkg.Partition(i0, j0, i0 + h, j0 + w), kind, stop_at=stop))
    assert sum(c.stop_at is not None for c in cases) >= 3 and sum(c.empty() for c in cases) >= 5
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        _, batch, st, _ = _run(pkg, al, cases, single=False)
    finally:
        al.close()
    groups = 0
    for c0 in range(0, len(cases), BATCH_MAX):
        groups += len({(c.tracked(), not c.nw()) for c in cases[c0:c0 + BATCH_MAX] if not c.empty()})
    assert groups == 8
    assert st["kernel_launches"] == groups, (st["kernel_launches"], groups)
    assert st["restarts"] == 0
    for k, c in enumerate(cases):
        if c.empty():
            assert not batch[k].last_column_chunks and not batch[k].last_row_chunks
            continue
        ref = refs(c, ENGINE_GRID)
        if c.stop_at is not None:
            _expect_stopped(c, batch[k], ref, k)
        else:
            _expect_oracle(c, batch[k], ref, k)


# ---------------------------------------------------------------------------------------------------------------------
# E. overflow rerun with a streamed first column
# ---------------------------------------------------------------------------------------------------------------------
def test_batched_overflow_rerun_replays_a_streamed_first_column(pkg, oracle, monkeypatch):
    """the batch twin of test_gpu_overflow.py::test_first_column_jump_replays_progressive_traffic: partitions with streamed
    custom first columns report an overflow part-way down (fault injection), their neighbours do not; the reruns on the
    int32 kernels see the column cells the batch attempt already took, the stream is read once, every last-column row
    and special row arrives once and in order, all of it equals the oracle"""
    from masa_cudalign_amd.manager import ArrayCellsReader
    INF = pkg.INF
    s0, s1 = pkg.seqgen.related_pair(60000, 40000, cfg=85)
    refs = Refs(pkg, oracle, s0, s1)
    strip = 40                                  # 256-row batch strips: the fault hits rows 10240.. of partitions taller than that
    c1 = _custom_col(30000, 0, 21, INF)
    c2 = np.zeros((28000 + 1, 2), dtype=np.int32)
    c2[1:, 0] = np.random.RandomState(22).randint(0, 40, 28000)
    c2[:, 1] = -INF
    c3 = _custom_col(32000, OFFSET, 23, INF)
    r3 = np.zeros((3001, 2), dtype=np.int32)
    r3[:, 0] = OFFSET - 5 * np.arange(3001)
    r3[:, 1] = -INF
    cases = [
        Case(pkg.Partition(0, 0, 30000, 3000), "nw", 9300, col=lambda: ArrayCellsReader(c1)),
        Case(pkg.Partition(20000, 5000, 48000, 9000), "sw", 9300, col=lambda: ArrayCellsReader(c2)),
        Case(pkg.Partition(25000, 12000, 57000, 15000), "semi", 9300, row=lambda: ArrayCellsReader(r3),
             col=lambda: ArrayCellsReader(c3)),
        Case(pkg.Partition(0, 20000, 9000, 26000), "sw", 9300),                      # 36 strips: no fault
        Case(pkg.Partition(40000, 30000, 50000, 34000), "nw", 9300),                 # 40 strips: no fault
    ]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        singles = []
        for c in cases:
            mg = c.manager(pkg)
            al.alignPartition(c.part, mg)
            singles.append(mg)
        monkeypatch.setenv("MI355SW_FAULT_OVERFLOW_STRIP", str(strip))
        batch = [c.manager(pkg) for c in cases]
        al.alignPartitions([c.part for c in cases], batch, rows_per_lane=4)
        st = al.getStatistics()
        monkeypatch.delenv("MI355SW_FAULT_OVERFLOW_STRIP")
    finally:
        al.close()
    assert st["restarts"] == 3, st["restarts"]               # one int32 rerun per partition that met the fault
    for k, c in enumerate(cases):
        ref = refs(c, ENGINE_GRID)
        _expect_oracle(c, batch[k], ref, ("batch", k))
        _expect_same(c, batch[k], singles[k], k)


def test_batched_overflow_rerun_of_a_device_made_column(pkg, oracle, monkeypatch):
    """partitions whose gap first column the device makes (nothing streamed, yet counted as fed) report an overflow in a
    batch, one of them on a pool slot that streamed a shorter custom column in the call before, on an aligner that never
    streamed one itself: their int32 reruns make the column again and replay nothing of that earlier stream; a streamed
    neighbour that faults too keeps its own cells"""
    from masa_cudalign_amd.manager import ArrayCellsReader
    INF = pkg.INF
    s0, s1 = pkg.seqgen.related_pair(40000, 20000, cfg=88)
    refs = Refs(pkg, oracle, s0, s1)
    short = _custom_col(3000, 0, 31, INF)
    long_col = _custom_col(26000, 0, 32, INF)
    first = [Case(pkg.Partition(0, 0, 3000, 2000), "nw", col=lambda: ArrayCellsReader(short)),
             Case(pkg.Partition(5000, 3000, 8000, 5000), "sw")]
    second = [Case(pkg.Partition(0, 0, 30000, 3000), "nw", 9300),                    # gap borders from 0: made on the device
              Case(pkg.Partition(2000, 5000, 8000, 9000), "sw", 9300),               # 24 strips: no fault
              Case(pkg.Partition(10000, 10000, 36000, 13000), "nw", 9300, col=lambda: ArrayCellsReader(long_col)),
              Case(pkg.Partition(0, 14000, 28000, 17000), "goal", 9300)]             # made on the device as well
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        b1 = [c.manager(pkg) for c in first]
        al.alignPartitions([c.part for c in first], b1, rows_per_lane=4)
        monkeypatch.setenv("MI355SW_FAULT_OVERFLOW_STRIP", "40")
        b2 = [c.manager(pkg) for c in second]
        al.alignPartitions([c.part for c in second], b2, rows_per_lane=4)
        st = al.getStatistics()
        monkeypatch.delenv("MI355SW_FAULT_OVERFLOW_STRIP")
    finally:
        al.close()
    assert st["restarts"] == 3, st["restarts"]
    for k, c in enumerate(first):
        _expect_oracle(c, b1[k], refs(c, ENGINE_GRID), ("first call", k))
    for k, c in enumerate(second):
        _expect_oracle(c, b2[k], refs(c, ENGINE_GRID), ("second call", k))


def test_overflow_rerun_keeps_the_batch_grid_of_a_fixed_height(pkg, oracle, monkeypatch):
    """aligner at a fixed 512-row height, batch at 256 rows: the batch's special rows sit on multiples of 256, and so do
    those of the int32 rerun after an overflow report -- one grid per partition, the oracle's at block height 256"""
    from masa_cudalign_amd.manager import ArrayCellsReader
    INF = pkg.INF
    s0, s1 = pkg.seqgen.related_pair(40000, 20000, cfg=89)
    refs = Refs(pkg, oracle, s0, s1)
    col = _custom_col(30000, 0, 33, INF)
    cases = [Case(pkg.Partition(0, 0, 30000, 3000), "nw", 9300, col=lambda: ArrayCellsReader(col)),
             Case(pkg.Partition(2000, 5000, 32000, 8000), "sw", 9300),
             Case(pkg.Partition(5000, 10000, 12000, 14000), "semi", 9300)]           # 28 strips: no fault
    al = pkg.MI355Aligner(device=0, rows_per_lane=8)
    try:
        al.setSequences(s0, s1)
        monkeypatch.setenv("MI355SW_FAULT_OVERFLOW_STRIP", "40")
        batch = [c.manager(pkg) for c in cases]
        al.alignPartitions([c.part for c in cases], batch, rows_per_lane=4)
        st = al.getStatistics()
        monkeypatch.delenv("MI355SW_FAULT_OVERFLOW_STRIP")
    finally:
        al.close()
    assert st["restarts"] == 2, st["restarts"]
    for k, c in enumerate(cases):
        _expect_oracle(c, batch[k], refs(c, 256), k)
        assert all(r % 256 == 0 for r in _special(c, batch[k]))


# ---------------------------------------------------------------------------------------------------------------------
# F. strip heights that change between calls
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_heights_change_between_calls(pkg, oracle):
    """1024-row batches, then 256, then 512 on one aligner with other partitions each time (stage 2's sweeps, then stage 3's
    walks, in one pipeline run)"""
    s0, s1 = pkg.seqgen.related_pair(60000, 40000, cfg=86)
    refs = Refs(pkg, oracle, s0, s1)
    calls = [
        (16, [Case(pkg.Partition(0, 0, 40000, 5000), "goal", 8500), Case(pkg.Partition(10000, 8000, 36000, 12000), "nw", 9300)]),
        (4, [Case(pkg.Partition(20000, 14000, 50000, 17000), "goal", 9300), Case(pkg.Partition(5000, 20000, 25000, 24000), "sw", 8500),
             Case(pkg.Partition(30000, 26000, 42000, 27000), "goal", 12000)]),
        (8, [Case(pkg.Partition(15000, 28000, 55000, 32000), "goal", 8500), Case(pkg.Partition(0, 33000, 30000, 38000), "semi", 9300)]),
    ]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        for R, cases in calls:
            _, batch, st, _ = _run(pkg, al, cases, R, single=False)
            assert st["strip_rows"] == 64 * R
            for k, c in enumerate(cases):
                _expect_oracle(c, batch[k], refs(c, ENGINE_GRID), (R, k))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# H. partitions the batch cannot take
# ---------------------------------------------------------------------------------------------------------------------
def test_partitions_the_batch_refuses_run_alone(pkg, oracle):
    """block pruning in a batch: that partition goes to a call of its own and equals it; every other one as always"""
    s0, s1 = pkg.seqgen.related_pair(30000, 30000, cfg=87)
    refs = Refs(pkg, oracle, s0, s1)
    cases = [Case(pkg.Partition(0, 0, 20000, 6000), "sw", 9300), Case(pkg.Partition(5000, 8000, 30000, 13000), "goal", 8500),
             Case(pkg.Partition(1000, 15000, 26000, 30000), "sw", 0)]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        part = pkg.Partition(2000, 2000, 28000, 26000)
        pruned_single = pkg.Stage1Manager(part, block_pruning=True, keep_last_column=True, special_row_interval=9300)
        al.alignPartition(part, pruned_single)
        single_pruned = al.getStatistics()["pruned_cells"]
        pruned_batch = pkg.Stage1Manager(part, block_pruning=True, keep_last_column=True, special_row_interval=9300)
        mgs = [c.manager(pkg) for c in cases]
        al.alignPartitions([c.part for c in cases] + [part], mgs + [pruned_batch], rows_per_lane=4)
        st = al.getStatistics()
    finally:
        al.close()
    # the batch kernel never prunes: cells pruned in this call were pruned by the call of its own
    assert single_pruned > 0 and st["pruned_cells"] > 0, (single_pruned, st["pruned_cells"])
    assert tuple(pruned_batch.getBestScore()) == tuple(pruned_single.getBestScore())
    assert np.array_equal(pruned_batch.lastColumn(), pruned_single.lastColumn())
    assert sorted(pruned_batch.special_rows) == sorted(pruned_single.special_rows)
    for k in pruned_single.special_rows:
        assert np.array_equal(np.concatenate(pruned_batch.special_rows[k]), np.concatenate(pruned_single.special_rows[k]))
    ref = oracle.stage1(s0[2000:28000], s1[2000:26000], threads=THREADS)
    assert tuple(pruned_batch.getBestScore()) == (ref["best"][0] + 2000, ref["best"][1] + 2000, ref["best"][2])
    for k, c in enumerate(cases):
        _expect_oracle(c, mgs[k], refs(c, ENGINE_GRID), k)


def test_many_letters_leave_the_batch_for_single_calls(pkg, oracle):
    """more than 14 byte values: no packed kernel, so no batch -- every partition through a call of its own, same results"""
    rng = np.random.RandomState(12)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    s1 = letters[rng.randint(0, 20, 12000)]
    s0 = s1[:10000].copy()
    mut = rng.rand(10000) < 0.1
    s0[mut] = letters[rng.randint(0, 20, int(mut.sum()))]
    refs = Refs(pkg, oracle, s0, s1)
    cases = [Case(pkg.Partition(0, 0, 10000, 2500), "goal", 8500), Case(pkg.Partition(0, 3000, 9500, 7000), "sw"),
             Case(pkg.Partition(500, 8000, 9999, 12000), "semi", 9300)]
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        singles, batch, st, _ = _run(pkg, al, cases, 4)
    finally:
        al.close()
    assert st["kernel"].startswith("sw_strip_kernel<"), st["kernel"]          # the int32 family, one call each
    for k, c in enumerate(cases):
        _expect_oracle(c, batch[k], refs(c, ENGINE_GRID), k)
        _expect_same(c, batch[k], singles[k], k)


# ---------------------------------------------------------------------------------------------------------------------
# G. stage 2's sweeps from guessed crosspoints on the engine
# ---------------------------------------------------------------------------------------------------------------------
STAGE2_INTERVAL = 8500


def test_stage2_from_guessed_crosspoints_on_the_engine_leaves_the_same_files(pkg, tmp_path, monkeypatch):
    """GPU twin of test_native_pipeline.py::test_stage2_from_guessed_crosspoints_leaves_the_same_files: MI355Aligner at
    engine-picked heights, stage 2's special rows 8500 apart -- a spacing the 512-, 1024- and 2048-row grids round to three
    different rows -- so the plain chain (alignPartition) and the accepted batched sweeps (alignPartitions) must save the
    same rows for the files to match"""
    import filecmp
    from masa_cudalign_amd import sra
    from masa_cudalign_amd.stage1 import stage1
    from masa_cudalign_amd.stage2 import stage2
    from masa_cudalign_amd.stage3 import stage3
    grids = {u: -(-STAGE2_INTERVAL // u) * u for u in (512, 1024, 2048)}
    assert STAGE2_INTERVAL > 8192 and len(set(grids.values())) == 3, grids
    real = sra.flush_intervals

    def stage2_at(m, n, limit, max_deep=20):
        out = real(m, n, limit, max_deep)
        out[1] = STAGE2_INTERVAL
        return out
    monkeypatch.setattr(sra, "flush_intervals", stage2_at)
    monkeypatch.delenv("MI355SW_STAGE2_SPECULATE", raising=False)     # stage 1 records the row peaks, as in the pipeline
    s0, s1 = pkg.seqgen.related_pair(90000, 90000, cfg=7)
    limit = 90000 * 90000 * 8 // 20000                  # stage 1: a special row every ~20 000 rows
    batches, chain = [], []
    runs = {}
    for mode in ("plain", "guessed"):
        work = str(tmp_path / mode)
        al = pkg.MI355Aligner(device=0)
        real_batch, real_single = al.alignPartitions, al.alignPartition
        in_stage2 = False

        def counted(partitions, managers, **kw):
            if in_stage2:
                batches.append(len(partitions))
            return real_batch(partitions, managers, **kw)

        def noted(partition, manager):
            real_single(partition, manager)
            if in_stage2 and mode == "plain":
                chain.append((partition.i1 - partition.i0, partition.j1 - partition.j0, al.getStatistics()["strip_rows"]))
        al.alignPartitions, al.alignPartition = counted, noted
        try:
            stage1(al, s0, s1, work, sra_limit=limit, block_pruning=False)
            in_stage2 = True
            r2 = stage2(al, s0, s1, work, sra_limit=limit, speculate=(mode == "guessed"))
            in_stage2 = False
            r3 = stage3(al, s0, s1, work, sra_limit=limit)
        finally:
            al.close()
        runs[mode] = (work, r2, r3)
    (pw, p2, p3), (gw, g2, g3) = runs["plain"], runs["guessed"]
    assert g2["speculation"]["accepted"] >= 1, g2["speculation"]
    assert batches and max(batches) > 1, batches
    # the plain chain at engine-picked heights: stage 2's own partitions (AlignerManager) of a goal sweep's shape get the
    # engine's short strips (AlignJob::begin), the others the cost model's -- every one of them on the 2048-row grid
    goal_shaped = [(m, n, rows) for m, n, rows in chain if m >= 4 * n and n >= 2048]
    assert goal_shaped and all(rows == (512 if n >= 65536 else 256) for m, n, rows in goal_shaped), chain
    assert all(2048 % rows == 0 for m, n, rows in chain), chain
    assert g2["crosspoints"] == p2["crosspoints"] and g3["crosspoints"] == p3["crosspoints"]
    for f in sorted(os.listdir(os.path.join(pw, "crosspoints"))):
        assert filecmp.cmp(os.path.join(pw, "crosspoints", f), os.path.join(gw, "crosspoints", f), shallow=False), f
    a, b = os.path.join(pw, "special_rows", "stage.02.00"), os.path.join(gw, "special_rows", "stage.02.00")
    files = []
    for root, _, names in os.walk(a):
        files += [os.path.relpath(os.path.join(root, x), a) for x in names]
    assert files
    theirs = []
    for root, _, names in os.walk(b):
        theirs += [os.path.relpath(os.path.join(root, x), b) for x in names]
    assert sorted(files) == sorted(theirs)
    for f in files:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
