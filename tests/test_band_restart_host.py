"""CPU: the restart of a band on the int32 kernels after the engine reports EOVERFLOW16 (bands.BandRunner.run) -- out of
streamPoll in the middle of a band, and out of streamEnd once every row is done.  The oracle stand-in never reports an
overflow, so here it is scripted: tests/band_traceback_cases.py's HostAligner raises AlignerError("... EOVERFLOW16 ...") at a
chosen call, completes one strip per poll as a kernel does, keeps the inbound rows it was fed across a restart
(first_column_resume_rows) and puts the special rows of a force_int32 stream on another grid: every 512 rows instead of 256.

Two bands run in one process, each on a thread of its own with its own engine, through bands.band_stage1 over an in-process
link (queues for send / recv, a barrier for all_gather): both bands are under way at once, as the ranks of a chain are, and
the link can hold a segment back until the band on the right has met its fault.

Shape: 1280 rows, 600 columns in two bands, segments and special rows of 256 rows -- five segments, four special rows (256,
512, 768, 1024) per band, of which 512 and 1024 lie on the grid of the restart.  On the GPU:
tests/test_gpu_overflow.py::test_band_chain_survives_an_overflow_report."""
import queue
import threading

import numpy as np
import pytest

import band_traceback_cases as bc

M, N, SEG, LIMIT = 1280, 600, 256, 32400
LIMITS = [0, 300, 600]
NSEG = M // SEG
GRID, GRID32 = [256, 512, 768, 1024], [512, 1024]
# edges, block pruning: a global chain, a local one, and one that ends on an edge and prunes (the engine hears of the edge
# before every streamBegin; the stand-in prunes nothing of a global recurrence, so every cell is as without)
FORMS = {"++": ("++", False), "**": ("**", False), "+3 pruned": ("+3", True)}


class _Yield(Exception):
    pass


class ScriptedEngine(bc.HostAligner):
    """faults: [(call, when)] with call "poll" / "end" and when(engine) -> bool, taken in order: the first call of that name at
    which `when` holds raises the overflow report.  calls: what the driver asked of the engine, in order."""

    def __init__(self, oracle, faults=()):
        bc.HostAligner.__init__(self, oracle, block_h=SEG)
        self.faults = list(faults)
        self.calls = []
        self.open = False
        self.faulted = threading.Event()
        self.fault_at = []                       # (call, rows done, inbound rows fed, special rows handed over) at each fault

    def _fault(self, call):
        from masa_cudalign_amd.engine import AlignerError
        if self.faults and self.faults[0][0] == call and self.faults[0][1](self):
            self.faults.pop(0)
            self.fault_at.append((call, self.done, self.fed, [c[1] for c in self.calls if c[0] == "special"]))
            self.calls.append(("fault", call))
            self.faulted.set()
            raise AlignerError("stream_%s: EOVERFLOW16 the packed kernel left its exact range (scripted)" % call)

    def setPruneEnd(self, mode):
        self.calls.append(("prune_end", int(mode)))
        bc.HostAligner.setPruneEnd(self, mode)

    def streamBegin(self, part, **kw):
        assert not self.open, "streamBegin on an engine whose stream is still open"
        self.calls.append(("begin", bool(kw.get("force_int32")), kw.get("first_column_resume_rows")))
        kept, resume_rows = getattr(self, "col", None), kw.pop("first_column_resume_rows", None)
        bc.HostAligner.streamBegin(self, part, **kw)
        if kw.get("force_int32"):
            self.sp_k *= 2                       # other strip heights: the special rows lie elsewhere
        if resume_rows is not None:              # the rows received so far are still in the engine's column
            assert kw.get("stream_first_column") and 0 <= resume_rows <= self.m
            self.col[1:1 + resume_rows] = kept[1:1 + resume_rows]
            self.fed = resume_rows
        self.open = True

    def streamFeedColumn(self, row, cells):
        assert self.open
        self.calls.append(("feed", int(row), len(cells)))
        bc.HostAligner.streamFeedColumn(self, row, cells)

    def _segment_done(self, r1):
        bc.HostAligner._segment_done(self, r1)
        raise _Yield

    def streamPoll(self):
        assert self.open
        self._fault("poll")
        try:
            self._advance()
        except _Yield:
            pass
        return self.done, self.done >= self.m

    def streamReadSpecialRow(self, k, col=0, length=None):
        assert self.open
        dp, cells = bc.HostAligner.streamReadSpecialRow(self, k, col, length)
        if length is None:                       # (length 0 only asks where the row lies)
            self.calls.append(("special", int(dp)))
        return dp, cells

    def streamAbort(self):
        self.calls.append(("abort",))

    def streamEnd(self):
        from masa_cudalign_amd.engine import AlignerError
        self.calls.append(("end",))
        if not self.open:
            raise AlignerError("stream_end: EINVAL no stream")
        self.open = False                        # (a stream whose end reports an overflow is over all the same)
        self._fault("end")
        return bc.HostAligner.streamEnd(self)

    def stream_calls(self):
        return [c[0] for c in self.calls if c[0] in ("begin", "abort", "end", "fault")]


class ThreadLink:
    """torch.distributed's send / recv / all_gather between bands that run on threads of one process.  hold = (segments,
    event): the segment with that index and every later one wait for the event before they travel."""

    def __init__(self, world, hold=None):
        self.world, self.hold = world, hold
        self.queues = [queue.Queue() for _ in range(world)]
        self.barrier = threading.Barrier(world, timeout=60.0)
        self.gathered = [None] * world
        self.broken = threading.Event()
        self.segments = []                       # every row segment sent, in order

    def end(self, rank):
        return _LinkEnd(self, rank)


class _LinkEnd:
    def __init__(self, link, rank):
        self.link, self.rank = link, rank

    def send(self, t, dst=None):
        link = self.link
        if t.dim() == 2:                         # (the start token is one row of two int64)
            if link.hold is not None and len(link.segments) >= link.hold[0]:
                assert link.hold[1].wait(timeout=60.0), "the band on the right never met its fault"
            link.segments.append(t.numpy().copy())
        link.queues[dst].put(t.clone())

    def recv(self, t, src=None):
        while True:
            if self.link.broken.is_set():
                raise RuntimeError("the other band failed")
            try:
                t.copy_(self.link.queues[self.rank].get(timeout=0.05))
                return
            except queue.Empty:
                pass

    def all_gather(self, out, t):
        link = self.link
        link.gathered[self.rank] = t.clone()
        link.barrier.wait()
        for k, o in enumerate(out):
            o.copy_(link.gathered[k])
        link.barrier.wait()


def pair_of():
    """a common core of 400 letters that crosses the band boundary, in unrelated flanks"""
    return bc.planted(41, 400, 500, 380, 100, 100)


def run_chain(pkg, work, form, engines, hold=None):
    """both bands through band_stage1, at once; returns per band (band_stage1's record, the runner, how often before_end ran)"""
    from masa_cudalign_amd import pipeline
    from masa_cudalign_amd.bands import BandRunner, band_stage1
    edges, prune = FORMS[form]
    s0, s1 = pair_of()
    assert (len(s0), len(s1)) == (M, N)
    link = ThreadLink(2, hold)
    got, errors = [None, None], []

    def band(k):
        eng = engines[k]
        eng.setSequences(s0, s1)
        ended = []
        try:
            runner = BandRunner(eng, dist=link.end(k), rank=k, world=2, segment_rows=SEG, prune_blocks=prune, transport="host")
            runner.stall_abort_s = 60.0
            out = band_stage1(runner, M, LIMITS[k], LIMITS[k + 1], work, LIMIT, n_total=N, before_end=lambda e: ended.append(e.done),
                              **pipeline.chain_form(**bc.edge_flags(pkg, edges)))
            got[k] = (out, runner, ended)
        except BaseException as e:
            errors.append(e)
            link.broken.set()
            link.barrier.abort()
        finally:
            eng.unsetSequences()

    threads = [threading.Thread(target=band, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return got, link


_PLAIN = {}


@pytest.fixture(scope="module")
def unfaulted(pkg, oracle, tmp_path_factory):
    """form -> (per band results, the link, the tree) of the chain without a fault, computed once"""
    def get(form):
        if form not in _PLAIN:
            work = str(tmp_path_factory.mktemp("plain"))
            engines = [ScriptedEngine(oracle), ScriptedEngine(oracle)]
            got, link = run_chain(pkg, work, form, engines)
            assert [e.stream_calls() for e in engines] == [["begin", "end"]] * 2
            _PLAIN[form] = (got, link, bc.tree(work))
        return _PLAIN[form]
    return get


def test_the_shape_reaches_every_branch(pkg, unfaulted):
    from masa_cudalign_amd import sra
    assert 0 < sra.flush_interval(M, N, LIMIT) <= SEG and NSEG == 5 and M % SEG == 0
    got, link, tree = unfaulted("**")
    assert len(link.segments) == NSEG
    for k in range(2):
        out, runner, ended = got[k]
        assert runner.special_rows == GRID and out["special_rows"] == GRID + [M] and runner.restarts == 0 and ended == [M]
    best = got[0][0]["best"]
    assert best == got[1][0]["best"] and best[2] > 100 and best[1] > LIMITS[1]      # the core, found across the boundary


def same_results(got, link, tree, got0, link0, tree0, special):
    """the faulted chain against the unfaulted one; special[k]: the special rows band k is to have handed over"""
    assert len(link.segments) == NSEG and [len(s) for s in link.segments] == [SEG] * NSEG      # each segment exactly once
    assert np.array_equal(np.concatenate(link.segments), np.concatenate(link0.segments))
    assert np.array_equal(got[1][1].inbound_column[1:], np.concatenate(link.segments))
    for k in range(2):
        (out, runner, _), (out0, runner0, _) = got[k], got0[k]
        assert out["best"] == out0["best"] and out["band_best"] == out0["band_best"]
        assert runner.edge_best == runner0.edge_best
        if k:
            assert np.array_equal(runner.inbound_column, runner0.inbound_column)
        assert runner.special_rows == special[k] and out["special_rows"] == special[k] + [M]
    # the files: those of the unfaulted run, byte for byte, less the special rows the grid of the restart does not hold
    gone = set()
    for k in range(2):
        ends = tuple("/%08X" % r for r in GRID if r not in special[k])
        gone |= {name for name in tree0 if name.startswith("FORK.%02d/" % k) and ends and name.endswith(ends)}
        assert len([name for name in tree0 if name.startswith("FORK.%02d/" % k) and name.endswith(tuple("/%08X" % r for r in GRID))]) == 4
    assert sorted(tree) == sorted(set(tree0) - gone), sorted(set(tree) ^ (set(tree0) - gone))[:8]
    assert all(tree[name] == tree0[name] for name in tree), [name for name in tree if tree[name] != tree0[name]][:8]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_an_overflow_at_stream_poll_restarts_the_band_on_int32(pkg, oracle, tmp_path, unfaulted, form):
    """band 0 meets it with rows 256, 512 and 768 handed over and three of five segments sent; band 1 with one or two of its five
    inbound segments fed (the link holds the third back until then) and, its column not yet whole, no special row handed over"""
    got0, link0, tree0 = unfaulted(form)
    engines = [ScriptedEngine(oracle, [("poll", lambda e: e.done == 768)]),
               ScriptedEngine(oracle, [("poll", lambda e: 0 < e.fed < e.m)])]
    work = str(tmp_path / "w")
    got, link = run_chain(pkg, work, form, engines, hold=(2, engines[1].faulted))
    prune_end = 3 if form == "+3 pruned" else 0
    for k, eng in enumerate(engines):
        assert eng.stream_calls() == ["begin", "fault", "abort", "end", "begin", "end"] and not eng.open
        begins = [c for c in eng.calls if c[0] == "begin"]
        (call, done, fed, handed), = eng.fault_at
        assert begins[0] == ("begin", False, None)
        assert begins[1] == ("begin", True, fed if k else None)          # the rows fed at that moment; band 0 is fed nothing
        assert got[k][1].restarts == 1 and got[k][2] == [M]              # before_end: once, the stream that ended
        # the engine hears of the edge again before the second begin, exactly when the chain prunes towards an edge
        before = [eng.calls[i - 1] for i, c in enumerate(eng.calls) if c[0] == "begin"]
        assert [b == ("prune_end", prune_end) for b in before] == [bool(prune_end)] * 2
        assert sum(1 for c in eng.calls if c[0] == "prune_end") == (2 if prune_end else 0)
        # special rows: each handed over once, ascending; those before the fault stay, the rest lie on the new grid
        rows = [c[1] for c in eng.calls if c[0] == "special"]
        assert rows == sorted(set(rows)) and rows[:len(handed)] == handed and all(r in GRID32 for r in rows[len(handed):])
        if k == 0:
            assert (done, handed) == (768, [256, 512, 768]) and rows == [256, 512, 768, 1024]
        else:
            assert 0 < fed < M and fed % SEG == 0 and handed == [] and rows == GRID32
            feeds = [c for c in eng.calls if c[0] == "feed"]
            assert feeds == [("feed", q * SEG, SEG) for q in range(NSEG)]      # nothing is fed twice, nothing is left out
    same_results(got, link, tree=bc.tree(work), got0=got0, link0=link0, tree0=tree0, special=[[256, 512, 768, 1024], GRID32])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_an_overflow_at_the_first_stream_end_runs_the_band_again_on_int32(pkg, oracle, tmp_path, unfaulted, form):
    """all rows done, every segment sent, every special row handed over: the stream begins again without an abort, nothing is
    sent or handed over twice, and before_end runs once for each stream that reaches its end"""
    got0, link0, tree0 = unfaulted(form)
    engines = [ScriptedEngine(oracle, [("end", lambda e: True)]), ScriptedEngine(oracle, [("end", lambda e: True)])]
    work = str(tmp_path / "w")
    got, link = run_chain(pkg, work, form, engines)
    prune_end = 3 if form == "+3 pruned" else 0
    for k, eng in enumerate(engines):
        assert eng.stream_calls() == ["begin", "end", "fault", "begin", "end"] and not eng.open
        begins = [c for c in eng.calls if c[0] == "begin"]
        assert begins == [("begin", False, None), ("begin", True, M if k else None)]
        assert got[k][1].restarts == 1 and got[k][2] == [M, M]
        assert eng.fault_at == [("end", M, M, GRID)]
        assert [c[1] for c in eng.calls if c[0] == "special"] == GRID
        assert sum(1 for c in eng.calls if c[0] == "prune_end") == (2 if prune_end else 0)
    same_results(got, link, tree=bc.tree(work), got0=got0, link0=link0, tree0=tree0, special=[GRID, GRID])


@pytest.mark.parametrize("call", ["poll", "end"])
@pytest.mark.parametrize("forced", [False, True], ids=["a second overflow", "force_int32 from the start"])
def test_an_overflow_on_the_int32_kernels_is_raised_not_retried(pkg, oracle, call, forced):
    """one band: the report reaches the caller, the stream is closed, and abort / end came after the last begin"""
    from masa_cudalign_amd.bands import BandRunner
    from masa_cudalign_amd.engine import AlignerError
    when = (lambda e: e.done == 512) if call == "poll" else (lambda e: True)
    eng = ScriptedEngine(oracle, [(call, when)] * (1 if forced else 2))
    s0, s1 = pair_of()
    eng.setSequences(s0, s1)
    ended = []
    try:
        runner = BandRunner(eng, segment_rows=SEG)
        with pytest.raises(AlignerError, match="EOVERFLOW16"):
            runner.run(M, 0, N, force_int32=forced, special_row_interval=SEG, before_end=lambda e: ended.append(e.done))
    finally:
        eng.unsetSequences()
    begins = [c for c in eng.calls if c[0] == "begin"]
    assert [b[1] for b in begins] == ([True] if forced else [False, True])
    assert runner.restarts == (0 if forced else 1) and not eng.faults and not eng.open
    after = eng.stream_calls()[len(eng.stream_calls()) - eng.stream_calls()[::-1].index("begin"):]
    if call == "poll":
        assert after == ["fault", "abort", "end"] and ended == []
    else:
        assert after[:2] == ["end", "fault"] and ended == [M] * len(begins)
