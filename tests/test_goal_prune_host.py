"""CPU: goal pruning of stage 2's sweeps (stage2(prune_goal=True), pipeline.align(prune_traceback=True)) -- the HOST side:
which bounds the manager derives for a sweep (AlignerManager.goalBounds) and that they reach the aligner.

The aligner is oracle/aligner_double.py's SerialBlockAligner behind a wrapper that takes setGoalBounds and applies the
rule AT CELL LEVEL to everything the sweep hands to its manager: every component v (H, and the gap component) of every
last-column, special-row and last-row cell with

    v + dj < B_col    and, where a row bound is on,    v + min(di, dj) - 2 * max(0, di - dj) < B_row

(dj / di: columns / rows left to the partition's last column / row) is replaced by -INF.  That is the most aggressive
pruning the rule allows -- the engine skips whole slabs, with a margin -- so a bound that is too tight (a forgotten
GAP_OPEN, a peak taken over the wrong cells, a missing row term) loses the goal or moves a crosspoint here, and the files
differ from the reference's."""
import hashlib
import os

import numpy as np
import pytest

from helpers import load_golden, make_pair, parse_args

G = load_golden()
CASES = {c["name"]: c for c in G["cases"] if "crosspoints_4" in c}
INF = 999999999


def _pruning_double(oracle):
    from oracle.aligner_double import SerialBlockAligner

    class _Pruner:
        """the manager of one sweep as the aligner sees it: everything forwarded, dispatched cells pruned first"""

        def __init__(self, mgr, part, b_col, b_row, owner):
            self._mgr, self._part, self._b_col, self._b_row, self._owner = mgr, part, b_col, b_row, owner
            self._col_pos, self._row_pos = 0, {}

        def __getattr__(self, name):
            return getattr(self._mgr, name)

        def _prune(self, cells, di, dj):
            out = np.array(cells, dtype=np.int32, copy=True)
            v = out.astype(np.int64)
            go = v + dj[:, None] < self._b_col if self._b_col > -INF else np.ones(v.shape, dtype=bool)
            if self._b_row > -INF:
                go &= v + np.minimum(di, dj)[:, None] - 2 * np.maximum(0, di - dj)[:, None] < self._b_row
            go &= v > -INF
            self._owner.replaced += int(go.sum())
            out[go] = -INF
            return out

        def dispatchColumn(self, j, buf, length):
            p = self._part
            if j == p.j1:
                i = p.i0 + self._col_pos + np.arange(length, dtype=np.int64)
                buf = self._prune(buf[:length], p.i1 - i, np.zeros(length, dtype=np.int64))
                self._col_pos += length
            self._mgr.dispatchColumn(j, buf, length)

        def dispatchRow(self, i, buf, length):
            p = self._part
            pos = self._row_pos.get(i, 0)
            j = p.j0 + pos + np.arange(length, dtype=np.int64)
            self._row_pos[i] = pos + length
            self._mgr.dispatchRow(i, self._prune(buf[:length], np.full(length, p.i1 - i, dtype=np.int64), p.j1 - j), length)

    class GoalPruningDouble(SerialBlockAligner):
        def __init__(self, bh, bw):
            SerialBlockAligner.__init__(self, bh, bw)
            self.pending, self.replaced, self.bounded_sweeps, self.row_bounds = None, 0, 0, 0

        def setGoalBounds(self, column_bounds, row_bounds=None):
            assert len(column_bounds) == 1
            self.pending = (int(column_bounds[0]), int(row_bounds[0]) if row_bounds is not None else -INF)

        def alignPartition(self, part, mgr):
            b, self.pending = self.pending, None               # consumed by this call
            if b is None or (b[0] <= -INF and b[1] <= -INF):
                return SerialBlockAligner.alignPartition(self, part, mgr)
            self.bounded_sweeps += 1
            self.row_bounds += b[1] > -INF
            return SerialBlockAligner.alignPartition(self, part, _Pruner(mgr, part, b[0], b[1], self))

    return GoalPruningDouble


def _run(pkg, oracle, case, tmp_path, **kw):
    from masa_cudalign_amd import fasta, pipeline
    s0, s1 = make_pair(pkg, case["seq"])
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    bh, bw = [a for a in case["args"] if a.startswith("--block=")][0][8:].split(",")
    v = [a for a in case["args"] if a.startswith("--disk-size=")][0][12:]
    mult = {"K": 1024, "M": 1024 * 1024, "G": 1024 ** 3}.get(v[-1])
    limit = int(float(v[:-1]) * mult) if mult else int(v)
    edges = parse_args(case["args"])
    al = _pruning_double(oracle)(int(bh), int(bw))
    work = str(tmp_path / "work")
    out = pipeline.align(al, q0, q1, work, sra_limit=limit, block_pruning=False, alignment_start=edges["start"],
                         alignment_end=edges["end"], **kw)
    return al, out, work


@pytest.mark.parametrize("name", ["full_pipeline_20000x9000_b8192", "full_pipeline_3000x2700_b8192"])
def test_cell_level_goal_pruning_leaves_the_reference_files(name, pkg, oracle, tmp_path):
    """prune_traceback=True with every dispatched cell the rule allows replaced by -INF: crosspoint_02 / 03 / 04,
    alignment.00.bin and alignment.00.txt are the fixture's, and cells were replaced"""
    from masa_cudalign_amd import alignment_file as af
    from masa_cudalign_amd.crosspoints import CrosspointsFile, crosspoint_file
    case = CASES[name]
    al, out, work = _run(pkg, oracle, case, tmp_path, prune_traceback=True)
    assert list(out["best"]) == case["best"]
    assert CrosspointsFile(crosspoint_file(work, 2)).load().tuples() == [tuple(p) for p in case["crosspoints_2"]]
    assert CrosspointsFile(crosspoint_file(work, 3)).load().tuples() == [tuple(p) for p in case["crosspoints_3"]]
    assert hashlib.sha256(open(crosspoint_file(work, 4), "rb").read()).hexdigest() == case["crosspoints_4"]["file_sha256"]
    assert hashlib.sha256(out["text"]).hexdigest() == case["alignment_txt_sha256"]
    assert open(os.path.join(work, "alignment.00.txt"), "rb").read() == out["text"]
    mine, theirs = open(os.path.join(work, "alignment.00.bin"), "rb").read(), bytes.fromhex(case["alignment_bin_hex"])
    assert af.canonical(af.loads(mine)) == af.canonical(af.loads(theirs))
    twins = any(len({g[0] for g in gaps}) != len(gaps) for gaps in af.loads(theirs)["result"]["gaps"])   # (see test_native_pipeline.py)
    assert twins or mine == theirs
    print("%s: %d sweeps with bounds (%d with a row bound), %d dispatched values replaced" % (name, al.bounded_sweeps, al.row_bounds, al.replaced))
    r2 = out["stage2"]
    assert r2["processed_cells"] == sum(c["processed_cells"] for c in r2["sweeps"]) and r2["pruned_cells"] == 0   # (the double computes every cell)
    if name == "full_pipeline_3000x2700_b8192":
        # no special row of stage 1 fits 3000 rows: the one sweep of stage 2 may hold the alignment's start (AT_ANYWHERE) and
        # is one of those the rule leaves unpruned -- the case holds the option to "nothing changes" there
        assert len(r2["sweeps"]) == 1 and al.bounded_sweeps == 0 and al.replaced == 0
    else:
        assert al.bounded_sweeps > 0 and al.replaced > 0
        assert any(any(c["bounded"]) for c in r2["sweeps"])


def test_option_off_hands_no_bounds(pkg, oracle, tmp_path):
    """default: no bound ever reaches the aligner"""
    case = CASES["full_pipeline_3000x2700_b8192"]
    al, out, work = _run(pkg, oracle, case, tmp_path)
    assert al.bounded_sweeps == 0 and al.replaced == 0 and al.pending is None
    assert hashlib.sha256(out["text"]).hexdigest() == case["alignment_txt_sha256"]


def test_goal_bounds_of_a_manager(pkg):
    """the bound is goal - peak - GAP_OPEN over the cells the reader can still hand out, border cell included; no bounds
    for a goal that may lie inside the partition, without a goal, or behind a border of unknown peak"""
    from masa_cudalign_amd.manager import (AlignerManager, ArrayCellsReader, InitialCellsReader, ReversedCellsReader,
                                           AT_ANYWHERE, AT_SEQUENCE_1_OR_2, AT_SEQUENCE_2, GAP_OPEN, GAP_EXT)

    class Row:                                            # a last-column reader with a known peak
        def __init__(self, peak):
            self.peak = peak

        def peak_h(self):
            return self.peak

    m = AlignerManager(None)
    m.setLastColumnReader(Row(70))
    m.setGoalScore(100, AT_SEQUENCE_1_OR_2)
    assert m.goalBounds() == (100 - 70 - GAP_OPEN, -INF)
    m.setLastRowReader(ReversedCellsReader(InitialCellsReader(GAP_OPEN, GAP_EXT)))
    assert m.goalBounds() == (100 - 70 - GAP_OPEN, 100 - 0 - GAP_OPEN)
    m.setGoalScore(100, AT_SEQUENCE_2)                    # the last row is not matched
    assert m.goalBounds() == (100 - 70 - GAP_OPEN, -INF)
    m.setGoalScore(100, AT_SEQUENCE_1_OR_2)
    m.setLastRowReader(ReversedCellsReader(ArrayCellsReader(np.zeros((4, 2), dtype=np.int32))))
    assert m.goalBounds() is None                         # a border whose peak nobody knows
    m.setLastRowReader(None)
    m.setGoalScore(100, AT_ANYWHERE)
    assert m.goalBounds() is None
    m.unsetGoalScore()
    assert m.goalBounds() is None
    m.setGoalScore(100, AT_SEQUENCE_1_OR_2)
    m.setLastColumnReader(Row(None))
    assert m.goalBounds() is None


def test_special_row_reader_peak_covers_the_border_cell(pkg, tmp_path):
    """SpecialRowReader.peak_h: cells [0, offset) -- the recorded peak of the row when it lies among them, the cells
    themselves otherwise, the border cell (index 0) included"""
    from masa_cudalign_amd import sra
    part = sra.SpecialRowsPartition(str(tmp_path), 0, 0, 100, 9)
    cells = np.zeros((10, 2), dtype=np.int32)
    cells[:, 0] = [50, 1, 2, 3, 40, 5, 6, 90, 8, 9]
    cells[:, 1] = -INF
    part.write(16, cells[:1])
    part.write(16, cells[1:])
    r = sra.SpecialRowReader(part, 16)
    r.seek(10)
    assert r.peak_h() == 90
    r.seek(7)                                             # the recorded peak (cell 7) is out of reach: cells 0..6
    assert r.peak_h() == 50
    r.seek(1)
    assert r.peak_h() == 50
