"""CPU: a chain of column bands that is interrupted and resumed (bands.serial_band_stage1(resume=True), pipeline.align_bands) on
the bands' stand-in engine -- tests/band_traceback_cases.py's HostAligner, taught here to take a partition that starts below
row 0 with a stored first row, and to hand its rows over one strip per poll as a kernel does.

Interruptions are exceptions raised from the `progress` callback.  What a resumed chain is held to: the trees of every FORK.NN
are those of an uninterrupted run, byte for byte (pruned chains: the oracle's optimum, every special row and boundary column
under the pruned-cell rule), and the stand-in's log shows that the bands done before were not run again and that the band that
was interrupted started where the state on disk says.

Every chain uses segment_rows=4096 and a budget that puts the special rows 4096 rows apart, so that a band of 9000 rows holds
two special rows and three column segments and a restart row inside the band exists.  On the GPU: tests/test_gpu_band_resume.py."""
import json
import os

import numpy as np
import pytest

import band_traceback_cases as bc
import edge_prune_cases as ec
from helpers import assert_pruned_cells

SEG = 4096
M, N, LIMIT = 9000, 1800, 32400
WEIGHTS = [1, 3, 2]
STATE, COLUMN = "chain.mi355", "last_column.mi355"


class Interrupt(Exception):
    pass


class _Yield(Exception):
    pass


class ResumeAligner(bc.HostAligner):
    """the stand-in with what a resumed band asks of the stream calls: a partition with i0 > 0, its first row as custom data
    (first_row: n + 1 cells, boundary cell first), a generated first column counted from i0; every streamBegin is logged with
    its partition; streamPoll completes ONE strip per call, so that special rows and column segments leave in the order a
    running kernel gives them"""

    def __init__(self, oracle, block_h=256, block_w=128):
        bc.HostAligner.__init__(self, oracle, block_h, block_w)
        self.begins = []

    def streamBegin(self, part, **kw):
        self.begins.append(dict(part=(part.i0, part.j0, part.i1, part.j1), prune_rows=kw.get("prune_rows"),
                                initial_bound=kw.get("initial_bound"), prune=bool(kw.get("prune_blocks"))))
        first_row = kw.pop("first_row", None)
        if first_row is not None:
            assert kw["first_row_init_type"] == self.o.INIT_WITH_CUSTOM_DATA and part.i0 > 0
            kw["first_row_init_type"] = 0
        else:
            assert part.i0 == 0
        bc.HostAligner.streamBegin(self, part, **kw)
        if first_row is not None:
            assert len(first_row) == self.n + 1
            self.row = np.array(first_row, dtype=np.int32)
            if not self.custom_col:
                assert kw.get("first_column_start_offset", 0) == part.i0
                self.col[:] = self.o.initial_cells(kw.get("first_column_init_type", 0), part.i0, self.m + 1)
            assert int(self.row[0, 0]) == int(self.col[0, 0]), "the stored row's boundary cell is the partition's corner"
            self.row[0] = self.col[0]

    def _segment_done(self, r1):
        bc.HostAligner._segment_done(self, r1)
        raise _Yield

    def streamPoll(self):
        try:
            self._advance()
        except _Yield:
            pass
        return self.done, self.done >= self.m


class Stop:
    """progress callback: records every event with the sizes of the band's files at that moment and raises Interrupt when
    `when(events)` says so"""

    def __init__(self, when=None, work=None):
        self.when, self.work, self.events, self.sizes = when, work, [], []

    def __call__(self, event, band, row):
        self.events.append((event, band, row))
        if self.work is not None:
            d = os.path.join(self.work, "FORK.%02d" % band)
            fn = os.path.join(d, COLUMN)
            st = json.load(open(os.path.join(d, STATE))) if os.path.exists(os.path.join(d, STATE)) else None
            self.sizes.append((os.path.getsize(fn) if os.path.exists(fn) else None, st))
        if self.when is not None and self.when(self.events):
            raise Interrupt(event, band, row)


def at_begin(band):
    return lambda ev: ev[-1][:2] == ("band_begin", band)


def nth_special(band, count):
    return lambda ev: ev[-1][:2] == ("special_row", band) and sum(1 for e in ev if e[:2] == ("special_row", band)) == count


def column_after_special(band, count):
    """the first "column" event of `band` after its count-th special row"""
    return lambda ev: ev[-1][:2] == ("column", band) and sum(1 for e in ev if e[:2] == ("special_row", band)) >= count


def limits_of(pkg):
    from masa_cudalign_amd.bands import band_limits
    return band_limits(N, WEIGHTS)


def form_of(pkg, edges):
    from masa_cudalign_amd import pipeline
    return pipeline.chain_form(**bc.edge_flags(pkg, edges))


def chain(pkg, oracle, pair, work, edges, resume=False, progress=None, prune=False, al=None, limit=LIMIT, limits=None, **kw):
    from masa_cudalign_amd.bands import serial_band_stage1
    al = al if al is not None else ResumeAligner(oracle)
    al.setSequences(*pair)
    try:
        args = dict(form_of(pkg, edges), prune_blocks=prune, segment_rows=SEG, **kw)
        if resume is not None:
            args.update(resume=resume, progress=progress)
        out = serial_band_stage1(al, len(pair[0]), limits or limits_of(pkg), work, limit, **args)
    finally:
        al.unsetSequences()
    return out, al


def interrupted(pkg, oracle, pair, work, edges, when, **kw):
    stop = Stop(when, work)
    al = ResumeAligner(oracle)
    with pytest.raises(Interrupt):
        chain(pkg, oracle, pair, work, edges, resume=True, progress=stop, al=al, **kw)
    return stop, al


def plain(tree):
    """the tree without the states"""
    return {k: v for k, v in tree.items() if os.path.basename(k) != STATE}


def same_trees(a, b):
    assert sorted(a) == sorted(b), (sorted(set(a) ^ set(b))[:8])
    assert all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]][:8]


_PAIRS, _WHOLE = {}, {}


def pair_of(pkg, related=False):
    if related not in _PAIRS:
        _PAIRS[related] = pkg.seqgen.related_pair(M, N, cfg=23) if related else (bc.random_dna(7, M), bc.random_dna(8, N))
    return _PAIRS[related]


@pytest.fixture(scope="module")
def whole(pkg, oracle, tmp_path_factory):
    """edges -> (tree, result) of the uninterrupted chain as the parent runs it (no resume argument at all), computed once"""
    def get(edges, related=False):
        if (edges, related) not in _WHOLE:
            work = str(tmp_path_factory.mktemp("whole"))
            out, _al = chain(pkg, oracle, pair_of(pkg, related), work, edges, resume=None)
            _WHOLE[(edges, related)] = (bc.tree(work), out)
        return _WHOLE[(edges, related)]
    return get


def test_the_test_shape_has_a_restart_row(pkg):
    from masa_cudalign_amd import sra
    assert 3840 < sra.flush_interval(M, N, LIMIT) <= 4096 and 2 * 4096 < M and M % 256 != 0


# ---------------------------------------------------------------------------------------------------------------------------
def test_a_fresh_run_with_resume_leaves_the_tree_plus_one_state_per_band(pkg, oracle, tmp_path, whole):
    tree0, out0 = whole("**")
    work = str(tmp_path / "w")
    stop = Stop(None, work)
    out, al = chain(pkg, oracle, pair_of(pkg), work, "**", resume=True, progress=stop)
    got = bc.tree(work)
    same_trees(plain(got), tree0)
    assert sorted(k for k in got if k.endswith(STATE)) == ["FORK.%02d/%s" % (k, STATE) for k in range(3)]
    assert not any(k.endswith(COLUMN) or k.endswith(".tmp") for k in got)
    assert tuple(out["best"]) == tuple(out0["best"]) and out["resumed"] is None and out["already_done"] is False
    assert [b["skipped"] for b in out["bands"]] == [False] * 3 and len(al.begins) == 3
    for k in range(3):
        st = json.loads(got["FORK.%02d/%s" % (k, STATE)])
        assert st["done"] and st["band"] == k and st["version"] == 1 and st["key"]["limits"] == limits_of(pkg)
        assert st["special_rows"] == [4096, 8192, M] and tuple(st["best"]) == tuple(out["bands"][k]["best"])
    # the order of durability: at every "column" event the file holds at least the rows the state counts, and the state counts
    # the rows the event names; at every "special_row" event the state names the row
    seen = 0
    for (event, band, row), (size, st) in zip(stop.events, stop.sizes):
        if event == "column":
            assert st["column_rows"] == row and size >= 8 * (1 + row) and not st["done"]
            seen += 1
        if event == "special_row":
            assert row in st["rows"] and not st["done"]
            assert os.path.basename(next(k for k in got if k.startswith("FORK.%02d" % band) and k.endswith("%08X" % row)))
    assert seen == 2 * 3                            # bands 0 and 1: segments of 4096, 4096 and 808 rows
    assert [e for e in stop.events if e[0] in ("band_begin", "band_end")] == [
        ("band_begin", 0, 0), ("band_end", 0, M), ("band_begin", 1, 0), ("band_end", 1, M), ("band_begin", 2, 0), ("band_end", 2, M)]


@pytest.mark.parametrize("band", [1, 2])
def test_interrupted_at_a_band_boundary(pkg, oracle, tmp_path, whole, band):
    tree0, out0 = whole("**")
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, "**", at_begin(band))
    left = bc.tree(work)
    assert "FORK.%02d/%s" % (band - 1, COLUMN) in left and len(left["FORK.%02d/%s" % (band - 1, COLUMN)]) == 8 * (M + 1)
    out, al = chain(pkg, oracle, pair_of(pkg), work, "**", resume=True)
    same_trees(plain(bc.tree(work)), tree0)
    assert tuple(out["best"]) == tuple(out0["best"])
    lim = limits_of(pkg)
    assert [b["part"] for b in al.begins] == [(0, lim[k], M, lim[k + 1]) for k in range(band, 3)]
    assert out["resumed"] == {"bands_skipped": band, "band": band, "from_row": 0}
    assert [b["skipped"] for b in out["bands"]] == [k < band for k in range(3)]
    assert [b["best"] for b in out["bands"]] == [b["best"] for b in out0["bands"]]
    assert [b["initial_bound"] for b in out["bands"]] == [b["initial_bound"] for b in out0["bands"]]


@pytest.mark.parametrize("edges", ["**", "++", "3+", "+3"])
def test_interrupted_inside_a_band(pkg, oracle, tmp_path, whole, edges):
    """band 1, at the first column segment after its second special row: rows 4096 and 8192 and 8192 rows of the column are on
    disk.  A chain that tracks nothing continues at row 8192, a local one starts band 1 over"""
    tree0, out0 = whole(edges)
    work = str(tmp_path / "w")
    stop, _al = interrupted(pkg, oracle, pair_of(pkg), work, edges, column_after_special(1, 2))
    assert stop.events[-1] == ("column", 1, 8192)
    st = json.load(open(os.path.join(work, "FORK.01", STATE)))
    assert not st["done"] and st["rows"] == [4096, 8192] and st["column_rows"] == 8192
    out, al = chain(pkg, oracle, pair_of(pkg), work, edges, resume=True)
    lim = limits_of(pkg)
    want_row = 0 if edges == "**" else 8192
    assert [b["part"] for b in al.begins] == [(want_row, lim[1], M, lim[2]), (0, lim[2], M, lim[3])]
    assert out["resumed"] == {"bands_skipped": 1, "band": 1, "from_row": want_row}
    same_trees(plain(bc.tree(work)), tree0)
    assert tuple(out["best"]) == tuple(out0["best"])
    assert out["bands"][1]["special_rows"] == [4096, 8192, M]


@pytest.mark.parametrize("edges", ["++", "3+"])
def test_interrupted_inside_the_first_band(pkg, oracle, tmp_path, whole, edges):
    """band 0 has no inbound column: its first column is generated, counted from the restart row"""
    tree0, out0 = whole(edges)
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, edges, column_after_special(0, 2))
    out, al = chain(pkg, oracle, pair_of(pkg), work, edges, resume=True)
    lim = limits_of(pkg)
    assert [b["part"] for b in al.begins] == [(8192, 0, M, lim[1]), (0, lim[1], M, lim[2]), (0, lim[2], M, lim[3])]
    assert out["resumed"] == {"bands_skipped": 0, "band": 0, "from_row": 8192}
    same_trees(plain(bc.tree(work)), tree0)
    assert tuple(out["best"]) == tuple(out0["best"])


def test_a_special_row_ahead_of_its_column(pkg, oracle, tmp_path, whole):
    """row 8192 is on disk and in the state, the column only up to row 4096: the band continues from the lower row"""
    tree0, out0 = whole("++")
    work = str(tmp_path / "w")
    stop, _al = interrupted(pkg, oracle, pair_of(pkg), work, "++", nth_special(1, 2))
    assert stop.events[-1] == ("special_row", 1, 8192)
    st = json.load(open(os.path.join(work, "FORK.01", STATE)))
    assert st["rows"] == [4096, 8192] and st["column_rows"] == 4096
    assert any(k.startswith("FORK.01") and k.endswith("%08X" % 8192) for k in bc.tree(work))
    out, al = chain(pkg, oracle, pair_of(pkg), work, "++", resume=True)
    assert al.begins[0]["part"][0] == 4096 and out["resumed"]["from_row"] == 4096
    same_trees(plain(bc.tree(work)), tree0)
    assert tuple(out["best"]) == tuple(out0["best"])


def test_two_interruptions(pkg, oracle, tmp_path, whole):
    tree0, out0 = whole("++")
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, "++", column_after_special(1, 1))
    stop, al = interrupted(pkg, oracle, pair_of(pkg), work, "++", at_begin(2))
    assert al.begins[0]["part"][0] == 4096 and len(al.begins) == 1
    out, al = chain(pkg, oracle, pair_of(pkg), work, "++", resume=True)
    assert [b["part"][:2] for b in al.begins] == [(0, limits_of(pkg)[2])]
    assert out["resumed"] == {"bands_skipped": 2, "band": 2, "from_row": 0}
    same_trees(plain(bc.tree(work)), tree0)
    assert tuple(out["best"]) == tuple(out0["best"])


def test_a_finished_chain_begins_no_stream(pkg, oracle, tmp_path, whole):
    tree0, out0 = whole("3+")
    work = str(tmp_path / "w")
    chain(pkg, oracle, pair_of(pkg), work, "3+", resume=True)
    before = bc.tree(work)
    out, al = chain(pkg, oracle, pair_of(pkg), work, "3+", resume=True)
    assert out["already_done"] is True and al.begins == [] and not any(e[0] == "begin" for e in al.log)
    assert out["resumed"] == {"bands_skipped": 3, "band": None, "from_row": 0}
    assert tuple(out["best"]) == tuple(out0["best"]) and all(b["skipped"] for b in out["bands"])
    same_trees(bc.tree(work), before)
    same_trees(plain(before), tree0)


# ---------------------------------------------------------------------------------------------------------------------------
# pruned chains
# ---------------------------------------------------------------------------------------------------------------------------
def _cells(blob):
    return np.frombuffer(blob, dtype=np.int32).reshape(-1, 2)


def _hold_tree_to_the_rule(got, want, lim, check, rows=M):
    """every special row (boundary cell first) and every tee'd boundary column of the pruned tree `got` against the unpruned
    tree `want` through check(got cells, want cells, i, j, where); returns the number of must-values"""
    total = 0
    for name in sorted(want):
        base = os.path.basename(name)
        if not name.startswith("FORK."):
            continue
        k = int(name[5:7])
        if len(base) == 8 and "special_rows" in name:
            row = int(base, 16)
            total += check(_cells(got[name]), _cells(want[name]), row, np.arange(lim[k], lim[k + 1] + 1), name)
        elif base == "C00000000.INIT_WITH_CUSTOM_DATA":
            total += check(_cells(got[name]), _cells(want[name]), np.arange(0, rows + 1), lim[k], name)
    return total


@pytest.mark.parametrize("edges", ["**", "++", "33"])
def test_a_pruned_chain_resumed_mid_chain(pkg, oracle, tmp_path, whole, edges):
    """a related pair, every band pruning against the chain's bound, interrupted inside band 1 and resumed"""
    from masa_cudalign_amd.bands import check_chain_bound
    pair = pair_of(pkg, True)
    tree0, out0 = whole(edges, True)                # the unpruned chain: exact cells
    opt = bc.oracle_optimum(oracle, pair[0], pair[1], edges)
    assert tuple(out0["best"]) == opt
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair, work, edges, column_after_special(1, 2), prune=True)
    out, al = chain(pkg, oracle, pair, work, edges, resume=True, prune=True)
    assert tuple(out["best"]) == opt
    assert out["resumed"] == {"bands_skipped": 1, "band": 1, "from_row": 0 if edges == "**" else 8192}
    got = bc.tree(work)
    assert sorted(plain(got)) == sorted(tree0)
    bounds = [b["initial_bound"] for b in out["bands"]]
    known = [b for b in bounds if b is not None]
    assert known == sorted(known) and all(b <= opt[2] for b in known)
    states = [json.loads(got["FORK.%02d/%s" % (k, STATE)]) for k in range(3)]
    assert [s["initial_bound"] for s in states] == bounds
    after = [s["bound_after"] for s in states if s["bound_after"] is not None]
    assert after == sorted(after)
    check_chain_bound(opt[2], states[0]["first_bound"])
    assert len({s["first_bound"] for s in states}) == 1
    if edges == "**":
        assert bounds[1] == out["bands"][0]["best"][2] and al.begins[0]["initial_bound"] == bounds[1] and al.begins[0]["prune"]
        assert any(b["pruned_cells"] > 0 for b in out["bands"])
        rule = lambda g, w, i, j, where: assert_pruned_cells(g, w, i, j, M, N, opt[2], oracle.SMITH_WATERMAN, where=where)[0]
    elif edges == "++":
        assert al.begins[0]["prune_rows"] == M - 8192 and out["bands"][1]["pruned_after_resume"] is True
        rule = lambda g, w, i, j, where: assert_pruned_cells(g, w, i, j, M, N, opt[2], oracle.NEEDLEMAN_WUNSCH, where=where)[0]
    else:
        assert al.begins[0]["prune_rows"] == M - 8192 and ("end", 3) in al.log
        rule = lambda g, w, i, j, where: ec.assert_edge_pruned_cells(g, w, i, j, M, N, opt[2], ec.EITHER, where=where)[0]
    assert _hold_tree_to_the_rule(got, tree0, limits_of(pkg), rule) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# durability and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_leftovers_of_a_kill_are_harmless(pkg, oracle, tmp_path, whole):
    """a state caught between write and rename, a column file longer than the state counts, a row still under its .tmp name"""
    tree0, out0 = whole("++")
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, "++", column_after_special(1, 1))
    d = os.path.join(work, "FORK.01")
    st = json.load(open(os.path.join(d, STATE)))
    assert st["column_rows"] == 4096
    with open(os.path.join(d, STATE + ".tmp"), "w") as f:
        f.write('{"version": 1, "done": tr')
    with open(os.path.join(d, COLUMN), "ab") as f:
        f.write(np.full((777, 2), 12345, dtype=np.int32).tobytes())
    rows = os.path.dirname(next(k for k in bc.tree(work) if k.startswith("FORK.01") and k.endswith("%08X" % 4096)))
    with open(os.path.join(work, rows, "%08X.tmp" % 8192), "wb") as f:
        f.write(b"\0" * 64)
    out, al = chain(pkg, oracle, pair_of(pkg), work, "++", resume=True)
    assert al.begins[0]["part"][0] == 4096
    got = bc.tree(work)
    assert not any(k.endswith(".tmp") for k in got)
    same_trees(plain(got), tree0)
    assert tuple(out["best"]) == tuple(out0["best"])


def test_a_column_that_is_gone_sends_the_band_on_the_left_back(pkg, oracle, tmp_path, whole):
    tree0, out0 = whole("++")
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, "++", at_begin(2))
    os.remove(os.path.join(work, "FORK.01", COLUMN))
    out, al = chain(pkg, oracle, pair_of(pkg), work, "++", resume=True)
    lim = limits_of(pkg)
    assert [b["part"] for b in al.begins] == [(0, lim[1], M, lim[2]), (0, lim[2], M, lim[3])]
    same_trees(plain(bc.tree(work)), tree0)


REFUSED = {
    "limits": dict(limits=[0, 400, 1100, N]),
    "sra_limit": dict(limit=LIMIT + 4096),
    "prune_blocks": dict(prune=True),
}


@pytest.mark.parametrize("what", sorted(REFUSED) + ["edges"])
def test_a_state_of_another_run_is_refused(pkg, oracle, tmp_path, what):
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, "++", at_begin(2))
    before = bc.tree(work)
    al = ResumeAligner(oracle)
    field = {"edges": "first_col_init_type|first_row_init_type|prune_end|recurrence|track_best", "sra_limit": "special_row_interval|sra_limit"}.get(what, what)
    with pytest.raises(ValueError, match=field):
        chain(pkg, oracle, pair_of(pkg), work, "3+" if what == "edges" else "++", resume=True, al=al, **REFUSED.get(what, {}))
    assert al.begins == [] and bc.tree(work) == before


def test_special_rows_without_a_state_are_refused(pkg, oracle, tmp_path):
    work = str(tmp_path / "w")
    chain(pkg, oracle, pair_of(pkg), work, "++", resume=None)
    al = ResumeAligner(oracle)
    with pytest.raises(RuntimeError, match="holds special rows but no chain.mi355"):
        chain(pkg, oracle, pair_of(pkg), work, "++", resume=True, al=al)
    assert al.begins == []


def test_a_state_of_another_format_version_is_refused(pkg, oracle, tmp_path):
    work = str(tmp_path / "w")
    interrupted(pkg, oracle, pair_of(pkg), work, "++", at_begin(1))
    fn = os.path.join(work, "FORK.00", STATE)
    st = json.load(open(fn))
    st["version"] = 7
    json.dump(st, open(fn, "w"))
    al = ResumeAligner(oracle)
    with pytest.raises(ValueError, match="version"):
        chain(pkg, oracle, pair_of(pkg), work, "++", resume=True, al=al)
    assert al.begins == []


def test_an_interrupted_run_leaves_no_stream_behind(pkg, oracle, tmp_path):
    """the engine's stream is aborted and ended on the way out, whichever callback raised"""
    calls = []

    class Watched(ResumeAligner):
        def streamAbort(self):
            calls.append("abort")

        def streamEnd(self):
            calls.append("end")
            return ResumeAligner.streamEnd(self)

    stop = Stop(nth_special(0, 1))
    with pytest.raises(Interrupt):
        chain(pkg, oracle, pair_of(pkg), str(tmp_path / "w"), "**", resume=True, progress=stop, al=Watched(oracle))
    assert calls == ["abort", "end"]


# ---------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------------------------------------
class FailingOnce(ResumeAligner):
    """raises Interrupt from the streamBegin of the band that starts at column `j0` -- an interruption in stage 1 for a front
    that has no progress callback of the chain's kind"""

    def __init__(self, oracle, j0):
        ResumeAligner.__init__(self, oracle, 256, 128)
        self.fail_j0 = j0

    def streamBegin(self, part, **kw):
        if part.j0 == self.fail_j0:
            raise Interrupt("streamBegin", part.j0)
        ResumeAligner.streamBegin(self, part, **kw)


@pytest.mark.parametrize("edges", ["**", "++"])
def test_align_bands_resumes_stage_1(pkg, oracle, tmp_path, edges):
    from masa_cudalign_amd import pipeline
    from masa_cudalign_amd.bands import band_limits
    s0, s1 = pkg.seqgen.related_pair(4000, 3600, cfg=23, inversion=0.0)
    q0, q1 = bc.fasta_pair(s0, s1)
    weights, limit = [1, 3, 2], 100 * 1024
    lim = band_limits(len(s1), weights)
    work = str(tmp_path / "w")
    kw = dict(sra_limit=limit, block_pruning=False, **bc.edge_flags(pkg, edges))
    with pytest.raises(Interrupt):
        pipeline.align_bands(FailingOnce(oracle, lim[2]), q0, q1, work, weights, resume=True, **kw)
    assert json.load(open(os.path.join(work, "FORK.01", STATE)))["done"] and not os.path.exists(os.path.join(work, "alignment.00.bin"))
    al = ResumeAligner(oracle, 256, 128)
    out = pipeline.align_bands(al, q0, q1, work, weights, resume=True, **kw)
    assert out["resumed"] == {"bands_skipped": 2, "band": 2, "from_row": 0}
    assert [b["part"][1] for b in al.begins if b["part"][0] == 0 and b["part"][2] == 4000][:1] == [lim[2]]
    bc.judge(pkg, oracle, work, s0, s1, lim, edges, out)
    ref = str(tmp_path / "ref")
    one = pipeline.align_bands(ResumeAligner(oracle, 256, 128), q0, q1, ref, weights, **kw)
    assert tuple(out["best"]) == tuple(one["best"]) and "resumed" not in one
    same_trees(plain(bc.tree(work)), bc.tree(ref))


def test_one_weight_is_align_whatever_resume_says(pkg, oracle, tmp_path):
    from masa_cudalign_amd import pipeline
    s0, s1 = pkg.seqgen.related_pair(2000, 1800, cfg=5)
    q0, q1 = bc.fasta_pair(s0, s1)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    one = pipeline.align_bands(bc.HostAligner(oracle, 128, 128), q0, q1, a, [1], sra_limit=60 * 1024, block_pruning=False)
    two = pipeline.align_bands(bc.HostAligner(oracle, 128, 128), q0, q1, b, [1], sra_limit=60 * 1024, block_pruning=False, resume=True)
    same_trees(bc.tree(a), bc.tree(b))
    assert two["text"] == one["text"] and not any(k.endswith(STATE) for k in bc.tree(b))
