"""GPU (-m gpu): a chain of column bands interrupted and resumed on the engine (bands.serial_band_stage1(resume=True),
pipeline.align_bands(resume=True)) -- 40 000 x 13 200 in three uneven bands, 256-row strips (rows_per_lane=4: the special rows
lie on a 256-row grid and the band ends in a ragged strip), column segments of 4096 rows.  Interruptions are exceptions raised
from the chain's `progress` callback; no process is killed.  A resumed chain leaves the trees of an uninterrupted run on the same
engine, byte for byte (pruned: the oracle's best cell, every row and boundary column under the pruned-cell rule), and every
resumed run begins on the SAME engine object the interrupted one left -- a stream left active would refuse it (MI355SW_ESTATE).
The host side, on the stand-in engine: tests/test_band_resume_host.py."""
import json
import os

import pytest

import band_traceback_cases as bc
from helpers import assert_pruned_cells
from test_band_resume_host import (COLUMN, STATE, Interrupt, Stop, at_begin, column_after_special, nth_special, plain, same_trees,
                                   _hold_tree_to_the_rule)

pytestmark = pytest.mark.gpu

M, N, LIMIT, SEG = 40000, 13200, 500 * 1024, 4096
WEIGHTS = [1, 3, 2]
GRID = 8448                       # the special rows: flush_interval(M, N, LIMIT) = 8251, rounded up to whole 256-row strips
THREADS = min(16, os.cpu_count() or 1)
_CACHE = {}


@pytest.fixture(scope="module")
def al4(pkg):
    al = pkg.MI355Aligner(device=0, rows_per_lane=4)
    yield al
    al.close()


def _pair(pkg):
    if "pair" not in _CACHE:
        _CACHE["pair"] = pkg.seqgen.related_pair(M, N, cfg=11, inversion=0.0)
    return _CACHE["pair"]


def _limits():
    from masa_cudalign_amd.bands import band_limits
    return band_limits(N, WEIGHTS)


def _chain(pkg, al, pair, work, edges, resume=False, progress=None, prune=False, **kw):
    from masa_cudalign_amd import pipeline
    from masa_cudalign_amd.bands import serial_band_stage1
    al.setSequences(*pair)
    try:
        return serial_band_stage1(al, M, _limits(), work, LIMIT, prune_blocks=prune, segment_rows=SEG, resume=resume, progress=progress,
                                  **dict(pipeline.chain_form(**bc.edge_flags(pkg, edges)), **kw))
    finally:
        al.unsetSequences()


def _interrupted(pkg, al, pair, work, edges, when, **kw):
    stop = Stop(when)
    with pytest.raises(Interrupt):
        _chain(pkg, al, pair, work, edges, resume=True, progress=stop, **kw)
    return stop


def _whole(pkg, al, edges, tmp_path_factory):
    """(tree, result) of the uninterrupted, unpruned chain on this engine, once per form"""
    if edges not in _CACHE:
        work = str(tmp_path_factory.mktemp("whole"))
        out = _chain(pkg, al, _pair(pkg), work, edges)
        _CACHE[edges] = (bc.tree(work), out)
    return _CACHE[edges]


def test_the_grid(pkg):
    from masa_cudalign_amd import sra
    assert -(-sra.flush_interval(M, N, LIMIT) // 256) * 256 == GRID and M % 256 != 0


def test_interrupted_at_a_band_boundary(pkg, al4, tmp_path, tmp_path_factory):
    tree0, out0 = _whole(pkg, al4, "**", tmp_path_factory)
    work = str(tmp_path / "w")
    _interrupted(pkg, al4, _pair(pkg), work, "**", at_begin(2))
    assert os.path.getsize(os.path.join(work, "FORK.01", COLUMN)) == 8 * (M + 1)
    out = _chain(pkg, al4, _pair(pkg), work, "**", resume=True)
    assert out["resumed"] == {"bands_skipped": 2, "band": 2, "from_row": 0}
    assert [b["skipped"] for b in out["bands"]] == [True, True, False]
    assert tuple(out["best"]) == tuple(out0["best"])
    same_trees(plain(bc.tree(work)), tree0)


def test_interrupted_inside_a_band(pkg, al4, tmp_path, tmp_path_factory):
    """a global chain, band 1 stopped at a column segment after its second special row: it continues below row 0"""
    tree0, out0 = _whole(pkg, al4, "++", tmp_path_factory)
    work = str(tmp_path / "w")
    stop = _interrupted(pkg, al4, _pair(pkg), work, "++", column_after_special(1, 2))
    st = json.load(open(os.path.join(work, "FORK.01", STATE)))
    print("interrupted at", stop.events[-1], "state rows", st["rows"], "column rows", st["column_rows"])
    out = _chain(pkg, al4, _pair(pkg), work, "++", resume=True)
    want = max(r for r in st["rows"] if r <= st["column_rows"])
    assert out["resumed"] == {"bands_skipped": 1, "band": 1, "from_row": want} and want in (GRID, 2 * GRID)
    assert tuple(out["best"]) == tuple(out0["best"])
    assert out["bands"][1]["special_rows"] == out0["bands"][1]["special_rows"]
    same_trees(plain(bc.tree(work)), tree0)


def test_interrupted_inside_the_first_band(pkg, al4, tmp_path, tmp_path_factory):
    """band 0 has no inbound column: the engine generates its first column (gap penalties) counted from the restart row"""
    tree0, out0 = _whole(pkg, al4, "++", tmp_path_factory)
    work = str(tmp_path / "w")
    _interrupted(pkg, al4, _pair(pkg), work, "++", column_after_special(0, 2))
    out = _chain(pkg, al4, _pair(pkg), work, "++", resume=True)
    assert out["resumed"]["bands_skipped"] == 0 and out["resumed"]["band"] == 0 and out["resumed"]["from_row"] in (GRID, 2 * GRID)
    assert tuple(out["best"]) == tuple(out0["best"])
    same_trees(plain(bc.tree(work)), tree0)


def test_the_engine_takes_the_next_run_after_an_interruption_under_a_running_kernel(pkg, al4, tmp_path, tmp_path_factory):
    """the exception leaves run() from inside flush_special, the kernel of band 0 still running: the stream is aborted and
    ended on the way out, so the same engine begins the resumed chain (a local one: band 0 starts over)"""
    tree0, out0 = _whole(pkg, al4, "**", tmp_path_factory)
    work = str(tmp_path / "w")
    _interrupted(pkg, al4, _pair(pkg), work, "**", nth_special(0, 1))
    out = _chain(pkg, al4, _pair(pkg), work, "**", resume=True)          # (MI355SW_ESTATE here if a stream were left behind)
    assert out["resumed"] == {"bands_skipped": 0, "band": 0, "from_row": 0}
    assert tuple(out["best"]) == tuple(out0["best"])
    same_trees(plain(bc.tree(work)), tree0)


def test_a_pruned_local_chain_resumed(pkg, oracle, al4, tmp_path, tmp_path_factory):
    from masa_cudalign_amd.bands import check_chain_bound
    tree0, out0 = _whole(pkg, al4, "**", tmp_path_factory)
    pair = _pair(pkg)
    opt = bc.oracle_optimum(oracle, pair[0], pair[1], "**", threads=THREADS)
    work = str(tmp_path / "w")
    _interrupted(pkg, al4, pair, work, "**", column_after_special(1, 1), prune=True)
    out = _chain(pkg, al4, pair, work, "**", resume=True, prune=True)
    assert tuple(out["best"]) == opt and out["resumed"] == {"bands_skipped": 1, "band": 1, "from_row": 0}
    bounds = [b["initial_bound"] for b in out["bands"]]
    assert bounds[1] == out["bands"][0]["best"][2] and bounds[1] <= bounds[2] <= opt[2]
    check_chain_bound(opt[2], json.load(open(os.path.join(work, "FORK.00", STATE)))["first_bound"])
    got = bc.tree(work)
    assert sorted(plain(got)) == sorted(tree0)
    rule = lambda g, w, i, j, where: assert_pruned_cells(g, w, i, j, M, N, opt[2], oracle.SMITH_WATERMAN, where=where)[0]
    assert _hold_tree_to_the_rule(got, tree0, _limits(), rule, rows=M) > 0
    print("pruned cells per band", [b["pruned_cells"] for b in out["bands"]])


def test_a_resumed_band_that_restarts_on_the_int32_kernels(pkg, al4, tmp_path, tmp_path_factory):
    """the resumed partition (rows r.. of band 1) reports an overflow at its second strip (the test knob) and starts again on the
    int32 kernels, and so does band 2: the same trees"""
    tree0, out0 = _whole(pkg, al4, "++", tmp_path_factory)
    work = str(tmp_path / "w")
    _interrupted(pkg, al4, _pair(pkg), work, "++", column_after_special(1, 2))
    al4.configure(fault_overflow_strip_plus1=2)
    try:
        out = _chain(pkg, al4, _pair(pkg), work, "++", resume=True)
    finally:
        al4.configure(fault_overflow_strip_plus1=0)
    assert out["resumed"]["from_row"] > 0 and [b["restarts"] for b in out["bands"]][1:] == [1, 1]
    assert tuple(out["best"]) == tuple(out0["best"])
    same_trees(plain(bc.tree(work)), tree0)


def test_a_wide_alphabet_pair_resumed_once(pkg, tmp_path):
    from test_gpu_wide_alphabet import ALPHABETS, F_WIDE, wide_pair
    pair = wide_pair(pkg, M, N, ALPHABETS["letters20"], cfg=401, ensure=True)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_WIDE)
    try:
        a, b = str(tmp_path / "a"), str(tmp_path / "b")
        out0 = _chain(pkg, al, pair, a, "++")
        assert "_wide" in al.getStatistics()["kernel"], al.getStatistics()["kernel"]
        _interrupted(pkg, al, pair, b, "++", column_after_special(1, 2))
        out = _chain(pkg, al, pair, b, "++", resume=True)
    finally:
        al.close()
    assert out["resumed"]["band"] == 1 and out["resumed"]["from_row"] > 0
    assert tuple(out["best"]) == tuple(out0["best"])
    same_trees(plain(bc.tree(b)), bc.tree(a))


@pytest.mark.parametrize("edges", ["**", "++"])
def test_align_bands_resumes(pkg, oracle, al4, tmp_path, edges):
    """stage 1 interrupted inside band 1 with exactly the arguments align_bands gives it, then align_bands(resume=True)"""
    from masa_cudalign_amd import pipeline
    pair = _pair(pkg)
    q0, q1 = bc.fasta_pair(*pair)
    work = str(tmp_path / "w")
    pipeline.check_work_directory(work, q0, q1)
    _interrupted(pkg, al4, pair, work, edges, column_after_special(1, 2), extent=(M, N))
    out = pipeline.align_bands(al4, q0, q1, work, WEIGHTS, sra_limit=LIMIT, block_pruning=False, resume=True, segment_rows=SEG,
                               **bc.edge_flags(pkg, edges))
    assert out["resumed"]["bands_skipped"] == 1 and (out["resumed"]["from_row"] > 0) == (edges == "++")
    if (edges, "opt") not in _CACHE:
        _CACHE[(edges, "opt")] = bc.oracle_optimum(oracle, pair[0], pair[1], edges, threads=THREADS)
    assert tuple(out["best"]) == _CACHE[(edges, "opt")]
    bc.judge(pkg, oracle, work, pair[0], pair[1], _limits(), edges, out, optimum=_CACHE[(edges, "opt")], threads=THREADS)
