"""How an alignment traced back through a chain of column bands is judged -- written once, for the CPU tests
(test_band_traceback_host.py) and the GPU tests (test_gpu_band_traceback.py).

The extra crosspoints on the band boundaries move stage 4's split points, so among equally good alignments the chain may pick
another one than the single partition: byte equality with pipeline.align is asked for ONE band only.  For more, judge():

(a) the alignment in alignment.00.bin is rescored by rescore() below -- match +1, mismatch -3, a gap run of length L costs
    3 + 2 L; nothing of stage56 / stage5.cpp is used -- and must score the unpruned oracle's optimum for the edges;
(b) its ends satisfy the edges; a local alignment ends in the oracle's best cell and starts where the score counted back from
    that cell is used up: the global score of exactly the rectangle between its ends is the optimum;
(c) crosspoint_03.00 is strictly ordered and holds a point on every band boundary the alignment meets -- exactly one where
    the path has one cell on that column; a gap run ALONG the column has several cells there and may leave a point on each
    special row it passes, every one of them a cell of the path --, crosspoint_04.00 has no partition above
    max_partition_size, and every crosspoint of both files is a cell of the rescored path, arrived at as its type says, with the
    path's score up to there (a gap crosspoint: the run's 3 + 2 L so far included);
(d) the score in stage 5's totals (the record's alignment, the file's raw score) equals (a)."""
import os

import numpy as np

from helpers import oracle_kwargs
from test_edge_chain_host import EdgeOracleEngine
from oracle.aligner_double import SerialBlockAligner

MATCH, MISMATCH, GAP_OPEN, GAP_EXT = 1, -3, 3, 2
FLAG = {"*": 0, "1": 1, "2": 2, "3": 3, "+": 4}


class HostAligner(EdgeOracleEngine, SerialBlockAligner):
    """ONE aligner for the CPU tests: the streaming surface of the bands' stand-in engine (stage 1 of a chain) and the serial
    block aligner of the traceback stages, both on the oracle"""

    def __init__(self, oracle, block_h=256, block_w=128):
        EdgeOracleEngine.__init__(self, oracle, None, None, seg=block_h)
        SerialBlockAligner.__init__(self, block_h, block_w)

    def setSequences(self, seq0, seq1):
        SerialBlockAligner.setSequences(self, seq0, seq1)
        self.s0, self.s1 = self.seq0, self.seq1

    def unsetSequences(self):
        SerialBlockAligner.unsetSequences(self)
        self.s0 = self.s1 = None

    def getStatistics(self):
        st = SerialBlockAligner.getStatistics(self)
        st["pruned_cells"] = getattr(self, "pruned_blocks", 0) * self.seg * 128
        return st


def fasta_pair(s0, s1):
    from masa_cudalign_amd import fasta
    return (fasta.parse(b">s0\n" + np.asarray(s0, dtype=np.uint8).tobytes() + b"\n"),
            fasta.parse(b">s1\n" + np.asarray(s1, dtype=np.uint8).tobytes() + b"\n"))


def edge_flags(pkg, edges):
    flag = {"*": pkg.AT_ANYWHERE, "1": pkg.AT_SEQUENCE_1, "2": pkg.AT_SEQUENCE_2, "3": pkg.AT_SEQUENCE_1_OR_2, "+": pkg.AT_SEQUENCE_1_AND_2}
    return dict(alignment_start=flag[edges[0]], alignment_end=flag[edges[1]])


def oracle_optimum(oracle, s0, s1, edges, threads=None):
    """(i, j, score): the unpruned oracle's best cell for the edges, 1-based DP coordinates"""
    kw = oracle_kwargs(oracle, dict(start=FLAG[edges[0]], end=FLAG[edges[1]], pruning=False, disk=-1, block=(1024, 1024)), len(s0), len(s1))
    if not threads:
        return tuple(int(x) for x in oracle.stage1(s0, s1, **kw)["best"])
    kw["threads"] = threads
    end = FLAG[edges[1]]
    if end not in (1, 2, 3):
        return tuple(int(x) for x in oracle.stage1(s0, s1, **kw)["best"])
    # (the threaded oracle hands out the borders, not the best cell of an edge: read it from them, in BestScoreList's order)
    from edge_chain_cases import edge_cell_of
    kw.update(want_last_row=True, want_last_col=True)
    ref = oracle.stage1(s0, s1, **kw)
    i, j, sc = edge_cell_of(end, ref["last_row"][1:], ref["last_col"][1:], len(s0), len(s1))
    return (int(i) + 1, int(j) + 1, int(sc))


def read_alignment(work):
    from masa_cudalign_amd import alignment_file
    return alignment_file.loads(open(os.path.join(work, "alignment.00.bin"), "rb").read())["result"]


def rescore(result, s0, s1):
    """the path of the alignment `result` (alignment_file.loads(...)["result"], forward sequences): returns (score, cells) with
    cells = {(i, j): (score of the path up to DP cell (i, j), how the path arrives there: 0 a pair, 1 a gap in sequence 0 --
    along sequence 1 --, 2 a gap in sequence 1)}; the start cell arrives as a pair with 0."""
    gaps = [{}, {}]
    for k in (0, 1):
        for pos, ln in result["gaps"][k]:
            gaps[k][pos] = gaps[k].get(pos, 0) + ln           # (a run stage 5 cut in two is one run)
    i, j = result["start"][0] - 1, result["start"][1] - 1
    ei, ej = result["end"]
    score = 0
    cells = {(i, j): (0, 0)}
    while (i, j) != (ei, ej):
        assert i <= ei and j <= ej, ("the path left the rectangle of its ends", i, j, ei, ej)
        if gaps[0].get(i + 1):
            ln = gaps[0].pop(i + 1)
            for t in range(1, ln + 1):
                cells[(i, j + t)] = (score - GAP_OPEN - GAP_EXT * t, 1)
            score -= GAP_OPEN + GAP_EXT * ln
            j += ln
        elif gaps[1].get(j + 1):
            ln = gaps[1].pop(j + 1)
            for t in range(1, ln + 1):
                cells[(i + t, j)] = (score - GAP_OPEN - GAP_EXT * t, 2)
            score -= GAP_OPEN + GAP_EXT * ln
            i += ln
        else:
            assert i < ei and j < ej, ("a pair beyond the end", i, j, ei, ej)
            score += MATCH if s0[i] == s1[j] else MISMATCH
            i, j = i + 1, j + 1
            cells[(i, j)] = (score, 0)
    assert not gaps[0] and not gaps[1], ("gaps off the path", gaps)
    return score, cells


def load_points(fn):
    from masa_cudalign_amd.crosspoints import CrosspointsFile
    return CrosspointsFile(fn).load().tuples()


def check_points(points, cells, where):
    """every crosspoint (type, i, j, score) is a cell of the path, arrived at as its type says, with the path's score"""
    base = points[0][3]
    for t, i, j, s in points:
        assert (i, j) in cells, "%s: crosspoint %r is no cell of the alignment" % (where, (t, i, j, s))
        sc, arrive = cells[(i, j)]
        assert s - base == sc, "%s: crosspoint %r carries %d, the alignment scores %d up to there" % (where, (t, i, j, s), s - base, sc)
        if t != 0:
            assert arrive == t, "%s: crosspoint %r of type %d, the alignment arrives there as %d" % (where, (t, i, j, s), t, arrive)


def judge(pkg, oracle, work, s0, s1, limits, edges, out, max_partition_size=16, optimum=None, threads=None):
    """(a)-(d) of the module's docstring for the files align_bands / band_traceback left in `work`; `out`: the record returned
    (None: the files only).  optimum: oracle_optimum(...) if the caller has it already; threads: for the oracle's runs.  Returns a dict of what was seen:
    score, start, end (DP cells), the points of crosspoint_03.00, the path's cells."""
    m, n = len(s0), len(s1)
    opt = optimum if optimum is not None else oracle_optimum(oracle, s0, s1, edges, threads)
    res = read_alignment(work)
    score, cells = rescore(res, s0, s1)
    start, end = (res["start"][0] - 1, res["start"][1] - 1), tuple(res["end"])
    # (a)
    assert score == opt[2], ("rescored", score, "oracle", opt)
    # (b)
    ok_start = {"*": True, "+": start == (0, 0), "1": start[0] == 0, "2": start[1] == 0, "3": start[0] == 0 or start[1] == 0}[edges[0]]
    ok_end = {"*": end == opt[:2], "+": end == (m, n), "1": end[0] == m, "2": end[1] == n, "3": end[0] == m or end[1] == n}[edges[1]]
    assert ok_start and ok_end, (edges, start, end, opt)
    if edges == "**":
        kw = oracle_kwargs(oracle, dict(start=4, end=4, pruning=False, disk=-1, block=(1024, 1024)), end[0] - start[0], end[1] - start[1])
        if threads:
            kw["threads"] = threads
        inner = oracle.stage1(s0[start[0]:end[0]], s1[start[1]:end[1]], **kw)["best"]
        assert int(inner[2]) == opt[2], ("the rectangle between the ends scores", tuple(inner), "the optimum is", opt)
    # (c)
    cp3 = load_points(os.path.join(work, "crosspoints", "crosspoint_03.00"))
    cp4 = load_points(os.path.join(work, "crosspoints", "crosspoint_04.00"))
    for a, b in zip(cp3, cp3[1:]):
        assert a[1] <= b[1] and a[2] <= b[2] and (a[1], a[2]) != (b[1], b[2]), ("crosspoint_03.00 out of order", a, b)
    assert (cp3[0][1], cp3[0][2]) == start and (cp3[-1][1], cp3[-1][2]) == end
    assert (cp4[0][1], cp4[0][2]) == start and (cp4[-1][1], cp4[-1][2]) == end
    on_boundary = {}
    for b in limits[1:-1]:
        if start[1] <= b <= end[1]:
            path_cells = sum(1 for (i, j) in cells if j == b)
            points = [p for p in cp3 if p[2] == b]
            assert path_cells >= 1
            if path_cells == 1:
                assert len(points) == 1, ("boundary", b, points)
            else:
                assert 1 <= len(points) <= path_cells, ("boundary", b, points, path_cells)
            on_boundary[b] = points
    for a, b in zip(cp4, cp4[1:]):
        di, dj = b[1] - a[1], b[2] - a[2]
        assert di >= 0 and dj >= 0
        if di and dj:                                   # (a partition that is one gap run is not split: CrosspointsFile.cpp:71-92)
            assert max(di, dj) <= max_partition_size, ("crosspoint_04.00", a, b)
    check_points(cp3, cells, "crosspoint_03.00")
    check_points(cp4, cells, "crosspoint_04.00")
    # (d)
    assert res["raw_score"] == score
    if out is not None:
        assert out["alignment"].raw_score == score
        assert open(os.path.join(work, "alignment.00.txt"), "rb").read() == out["text"]
    return dict(score=score, start=start, end=end, cp3=cp3, cp4=cp4, cells=cells, on_boundary=on_boundary, optimum=opt)


def tree(path):
    """{relative name: bytes} of every file under `path`"""
    out = {}
    for d, _dirs, files in os.walk(path):
        for f in files:
            fn = os.path.join(d, f)
            out[os.path.relpath(fn, path)] = open(fn, "rb").read()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# planted pairs: unrelated flanks around a common core, so that the local optimum is the core and where it lies is the test's
# choice; rng-made, checked by the tests on the result (never assumed)
# ---------------------------------------------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_dna(seed, k):
    return np.random.default_rng(seed).choice(ACGT, size=k)


def planted(seed, core, before0, after0, before1, after1, cut0=None, cut1=None):
    """seq0 = before0 random letters + core + after0, seq1 likewise with ITS OWN flanks; cut0 = (position in the core, length): that
    many letters of the core are missing in seq0 (the alignment has a gap run in sequence 0 there, along sequence 1), cut1 alike"""
    c = random_dna(seed, core)
    c0 = np.concatenate([c[:cut0[0]], c[cut0[0] + cut0[1]:]]) if cut0 else c
    c1 = np.concatenate([c[:cut1[0]], c[cut1[0] + cut1[1]:]]) if cut1 else c
    s0 = np.concatenate([random_dna(seed + 1, before0), c0, random_dna(seed + 2, after0)])
    s1 = np.concatenate([random_dna(seed + 3, before1), c1, random_dna(seed + 4, after1)])
    return np.ascontiguousarray(s0), np.ascontiguousarray(s1)
