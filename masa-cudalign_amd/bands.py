"""Column-band (multi-GPU) Stage-1 driver: one process per GPU, band g owns columns
[n*W_g/sum(W), n*W_{g+1}/sum(W)) of seq1 and every row of seq0; band g streams its LAST column
(H,E per row) to band g+1, which consumes it as its FIRST column (INIT_WITH_CUSTOM_DATA).

Replaces the reference's --fork/--split chain (M/libmasa/libmasa.cpp:497-642): forked processes
joined by TCP sockets carrying cell_t (M/common/io/SocketCells{Reader,Writer}.cpp), best score
relayed through AlignerPool signal files (M/stage1/sw_stage1.cpp:421-464).  Here the boundary
column goes GPU to GPU: band g+1 owns a column PORT in its own HBM, band g's strip kernel stores its
last column straight into it over xGMI (peer-mapped through hipIpc) and publishes the row count with a
system-scope release store that band g+1's kernel polls -- no host, copy queue or PCIe in the loop
(transport "p2p").  The CPU tests' stand-in engine uses the "host" transport instead (row segments sent
with torch.distributed send/recv, gloo).  The best score is an all_gather of one (score,i,j) triple
reduced with BestScoreList's order.

The compute engine is injected (`engine_factory`) so that the N>1 plumbing can be exercised on CPU
with a stand-in; the product engine is MI355Aligner (HIP, no CPU fallback).
"""
import json
import os
import sys
import threading
import time
import zlib

import numpy as np

from . import sra as sra_mod
from .engine import (INF, SMITH_WATERMAN, NEEDLEMAN_WUNSCH, INIT_WITH_ZEROES, INIT_WITH_GAPS, INIT_WITH_CUSTOM_DATA, Partition,
                     AlignerError)


def band_limits(n, weights):
    """split_sequences, libmasa.cpp:497-535: band g = (n*P[g]/sum, n*P[g+1]/sum] in 1-based trim
    coordinates, i.e. 0-based half-open [n*P[g]//sum, n*P[g+1]//sum)."""
    tot = int(sum(weights))
    acc = [0]
    for w in weights:
        acc.append(acc[-1] + int(w))
    return [(n * acc[g]) // tot for g in range(len(weights) + 1)]


def rows_per_lane_for_bands(m, band_cols, world, waves=1024):
    """Strip height for a chain of `world` equal column bands.  Band g+1 can only start once band g has
    swept its first strips across the whole band, and can never finish earlier than one band sweep after
    band g does, so the chain costs (rounds + world - 1) sweeps of band_cols steps; the step time grows
    with the strip height (measured table, same as runtime.cpp step_ns) while taller strips need fewer
    rounds.  Equal widths are optimal for such a chain (a narrower later band is throttled by its
    predecessor's rate, a wider one by its own), so only the height is planned."""
    best, tb = 0, None
    for R in (4, 8, 12, 16, 24, 32):
        step = {4: 97, 8: 138, 12: 181, 16: 222, 24: 291, 32: 368}[R]
        strips = -(-m // (64 * R))
        rounds = -(-strips // waves)
        t = step * ((rounds + world - 1) * band_cols + 280.0 * min(strips, waves))
        if tb is None or t < tb:
            best, tb = R, t
    return best


def canonical_best(cands):
    """BestScoreList order (M/common/BestScoreList.hpp:30-38): score desc, i asc, j asc."""
    best = (-1, -1, -INF)
    for (i, j, s) in cands:
        if j < 0 and i < 0:
            continue
        if s > best[2] or (s == best[2] and (i < best[0] or (i == best[0] and j < best[1]))):
            best = (int(i), int(j), int(s))
    return best


SEED_MIN_EXTENT = 8 << 20            # rows and columns from which the diagonal seed pays (as in mi355sw_stream_begin)
NO_BOUND = -(1 << 40)                # "no bound" in the start token that travels along the chain


def chain_seed_bound(engine, m, n, recurrence, first_row_init_type, first_col_init_type):
    """What the pruning bound of every band of a chain starts from: the diagonal seed pass over the WHOLE m x n matrix
    (mi355sw_seed_bound), run once on `engine`'s GPU before the first band starts.  A single partition gets it from
    mi355sw_stream_begin by itself; a band cannot (it sees its own columns, and its borders are ports), and without it
    each band prunes only against what the chain has found so far -- at 62 M x 57 M, 41 % of the cells instead of 75 %.
    None where the pass does not apply: small matrices, borders other than the recurrence's own (zeroes for a local
    alignment, gap penalties from the origin for a global one), an engine without the entry point, MI355SW_NO_DIAGONAL_SEED."""
    if m < SEED_MIN_EXTENT or n < SEED_MIN_EXTENT or not hasattr(engine, "seedBound") or os.environ.get("MI355SW_NO_DIAGONAL_SEED"):
        return None
    own = INIT_WITH_ZEROES if recurrence == SMITH_WATERMAN else 1          # 1 = INIT_WITH_GAPS
    if first_row_init_type != own or first_col_init_type != own:
        return None
    return engine.seedBound(Partition(0, 0, m, n), recurrence)


def check_chain_bound(score, bound):
    """A pruning chain must end at or above the bound it started from (the diagonal seed's, a caller's): that bound is the score of
    an alignment that exists / a lower bound of H[m][n], and slabs that can still reach it are computed.  A chain that ends below
    was given a bound no alignment reaches -- its optimum may have been pruned away, the result is void.  One stream checks this
    itself (MI355SW_EBOUND, mi355sw_stream_end); a band of a chain cannot (the best may be another band's)."""
    if bound is not None and score is not None and int(score) < int(bound):
        raise AlignerError("EBOUND: the chain ended at %d, below the bound %d its pruning started from -- no alignment reaches that "
                           "bound, the result is void" % (int(score), int(bound)))


def edge_seed_bound(engine, m, n, first_row_init_type, first_col_init_type):
    """chain_seed_bound for a chain whose alignment ends on a sequence edge (prune_end 1..3): the global seed -- the score of a
    corner-to-corner alignment under gap borders -- is admissible under every start and end form whose borders are zeroes or gap
    penalties counted from the corner (a border of zeroes dominates one of gap penalties cell by cell, and the last cell lies
    on both edges), so it is asked for as the global run's.  Any other border form: no seed."""
    own = (INIT_WITH_ZEROES, INIT_WITH_GAPS)
    if first_row_init_type not in own or first_col_init_type not in own:
        return None
    return chain_seed_bound(engine, m, n, NEEDLEMAN_WUNSCH, INIT_WITH_GAPS, INIT_WITH_GAPS)


def check_prune_end(prune_end, recurrence, track_best):
    """prune_end 1..3 (engine.END_LAST_ROW / END_LAST_COLUMN / END_ROW_OR_COLUMN): the alignment ends on an edge of the whole
    matrix and the result is the best H there -- a global recurrence with nothing tracked"""
    if prune_end not in (0, 1, 2, 3):
        raise ValueError("prune_end %r is none of 0 (the last cell / the best cell), 1 (last row), 2 (last column), 3 (either)" % (prune_end,))
    if prune_end and (recurrence != NEEDLEMAN_WUNSCH or track_best):
        raise ValueError("prune_end=%d needs recurrence=NEEDLEMAN_WUNSCH and track_best=False" % prune_end)


def _border_h(init_type, k):
    """H of the cell at distance k from the origin on a generated first row or column: 0 on a border of zeroes and in the
    origin itself, else k gap extensions and, for INIT_WITH_GAPS, the gap's opening"""
    if init_type == INIT_WITH_ZEROES or k == 0:
        return 0
    return -2 * k - (3 if init_type == INIT_WITH_GAPS else 0)


def _corner_cell(first_row_init_type, j):
    """(H, E) of DP cell (0, j) on the first row: the corner of the band that starts at column j.  Zero-initialised rows give
    (0,-INF); custom rows are handled by the caller feeding row 0 of the stream."""
    return np.array([[_border_h(first_row_init_type, j), -INF]], dtype=np.int32)


def _stop_stream(engine, swallow, guard_abort=True):
    """stops an open stream: the kernel is aborted, then the stream ended.  A failure of either that is of the classes `swallow`
    is dropped (there is no stream any more: the path that raised has ended it already) -- with guard_abort=False only
    streamEnd's, streamAbort's reaches the caller and the stream is not ended."""
    for fn, guarded in ((engine.streamAbort, guard_abort), (engine.streamEnd, True)):
        try:
            fn()
        except swallow:
            if not guarded:
                raise


def _edges_held(prune_end, last):
    """the edge cells of the whole matrix that a band holds, as prune_end's bits: its slice of the last row, and -- the last
    band -- the last column"""
    return (prune_end & 1) | ((prune_end & 2) if last else 0)


def _arm_prune_end(engine, prune_end, prune_blocks):
    """with block pruning the engine hears of the edge before EVERY streamBegin (the int32 retry too: the engine then drops it
    together with the pruning)"""
    if prune_end and prune_blocks:
        engine.setPruneEnd(prune_end)


def _seed_bound(engine, m, n, recurrence, prune_end, first_row_init_type, first_col_init_type):
    """the diagonal seed of the whole m x n matrix for a pruning chain: the edge form's where the alignment ends on an edge"""
    if prune_end:
        return edge_seed_bound(engine, m, n, first_row_init_type, first_col_init_type)
    return chain_seed_bound(engine, m, n, recurrence, first_row_init_type, first_col_init_type)


def _stream_keywords(m, j0, n, first, last, port, chain, recurrence, track_best, first_row_init_type, first_col_init_type,
                     prune_end, prune, want_last_row, force_int32):
    """streamBegin's keywords for the band that starts at column j0 of an n-column matrix and runs m rows.  first / last: its
    place in the chain; port: the boundary columns travel through column ports (else through the host, in segments); chain:
    there is more than one band; prune: block pruning is on for this recurrence."""
    kw = dict(recurrence_type=recurrence, track_best=track_best,
              first_row_init_type=first_row_init_type, first_row_start_offset=j0,
              want_last_column=((not last) and not port) or bool(_edges_held(prune_end, last) & 2),
              last_column_port=(not last) and port,
              want_last_row=want_last_row or bool(prune_end & 1), force_int32=force_int32)
    if prune:
        # every band prunes against the best of the whole chain (share_best) and bounds the gain still possible
        # by the extents of the whole matrix, not of its own band
        kw.update(prune_blocks=True, prune_rows=m, prune_cols=n - j0, share_best=chain)
    if first:
        kw.update(first_column_init_type=first_col_init_type)
    else:
        kw.update(first_column_init_type=INIT_WITH_CUSTOM_DATA, first_column=_corner_cell(first_row_init_type, j0),
                  stream_first_column=not port, first_column_port=port)
    return kw


def _start_token(ok, bound):
    import torch
    return torch.tensor([1 if ok else 0, NO_BOUND if bound is None else int(bound)], dtype=torch.int64)


class BandRunner:
    """Runs one band of the chain on this rank.  `dist` is torch.distributed (already initialised) or an object
    with send/recv/all_gather, or None for a single band.  All ranks must call run() with the same m.

    transport = "p2p"  : the boundary column goes GPU to GPU (column ports, include/mi355sw.h): band g+1 owns a
                         port in its own HBM, band g's strip kernel stores its last column straight into it over
                         xGMI and publishes the row count with a system-scope release store; the hosts only
                         exchange the 80-byte port handle before the kernels start.  Default on GPUs.
                "host" : pinned zero-copy columns + send/recv of row segments between the rank processes (the
                         reference's socket chain, libmasa.cpp:540-642); used by the CPU tests' stand-in engine
                         and as a fallback.
    `device` is only the device of the tensors used for collectives (reduce_best)."""

    def __init__(self, engine, dist=None, rank=0, world=1, device=None, segment_rows=1 << 16, prune_blocks=False,
                 transport="host", seed_bound=True):
        self.engine, self.dist, self.rank, self.world = engine, dist, rank, world
        self.prune_blocks = prune_blocks
        self.seed_bound = seed_bound   # pruning chains: band 0 runs the diagonal seed of the whole matrix first (chain_seed_bound)
        self.initial_bound = None      # ... and this is what the last run's bound started from
        self.device = device
        self.segment_rows = segment_rows
        self.transport = transport if world > 1 else "none"
        self._in_port = None         # PortHandle of this band's inbound port, and the rows it was made for
        self._in_rows = 0
        self._out_token = None       # handle bytes of the neighbour's port currently mapped
        self.restarts = 0            # packed-kernel overflow restarts (int32 rerun) of the last run
        self.p2p_error = None        # why probe_p2p() / verify_p2p() failed on this rank
        self.inbound_crc = None      # crc32 of the inbound boundary column of the last run(digest_inbound=True)
        self.special_rows = []       # DP rows of the special rows the last run handed to its sink
        self.hints = 0               # best-score hints this band took from the others in the last run (host transport)
        self.edge_best = None        # prune_end != 0: best (i, j, score) of the edge cells this band holds, of the last run
        self.stall_abort_s = None    # seconds without progress after which run() gives up (None: MI355SW_BAND_STALL_S, default 900)
        # Block pruning over a chain of bands needs the best of the WHOLE matrix (the reference switches pruning off
        # when it forks, libmasa.cpp:1318-1321).  Between GPUs the kernels share it through the column ports; on the
        # host transport a side thread does, with one small all_reduce(MAX) every few milliseconds on its own group.
        self._best_group = None
        if prune_blocks and world > 1 and dist is not None and hasattr(dist, "new_group"):
            self._best_group = dist.new_group(list(range(world)), backend="gloo")

    def _tensor(self, rows):
        import torch
        return torch.empty((rows, 2), dtype=torch.int32, device="cpu")

    # -- p2p: port hand-shake, once per run ------------------------------------------------------------
    def _exchange_ports(self, m):
        """band g (> 0) makes its inbound port ready (created, or its counter reset) and THEN tells band g-1, which
        only then starts its kernel: nothing can be published into a port before its owner has reset it."""
        import torch
        from .engine import PortHandle
        eng, dist = self.engine, self.dist
        first, last = self.rank == 0, self.rank == self.world - 1
        if not first:
            if self._in_port is None or self._in_rows < m:     # a port made for a taller matrix serves a shorter one
                self._in_port, self._in_rows = eng.portCreate(m), m
            else:
                eng.portReset()
            tok = torch.frombuffer(bytearray(self._in_port.tobytes()), dtype=torch.uint8).clone()
            dist.send(tok, dst=self.rank - 1)
        if not last:
            tok = torch.empty(len(PortHandle().tobytes()), dtype=torch.uint8)
            dist.recv(tok, src=self.rank + 1)
            b = bytes(tok.numpy().tobytes())
            if b != self._out_token:
                eng.portOpen(PortHandle.frombytes(b))
                self._out_token = b

    def probe_p2p(self, m):
        """One port hand-shake without a run, errors caught: True if this rank could create its inbound port and map
        its neighbour's.  The caller makes the ranks agree (all_reduce MIN) and falls back to transport="host" for
        everybody if any of them could not -- a rank that finds out in the middle of run() would leave its
        neighbours' kernels waiting."""
        if self.transport != "p2p":
            return True
        import torch
        from .engine import PortHandle
        ok = True
        first, last = self.rank == 0, self.rank == self.world - 1
        size = len(PortHandle().tobytes())
        try:
            if not first:
                try:
                    self._in_port, self._in_rows = self.engine.portCreate(m), m
                    tok = torch.frombuffer(bytearray(self._in_port.tobytes()), dtype=torch.uint8).clone()
                except Exception as e:            # whatever it was: the neighbour must still get its (empty) token
                    self.p2p_error = str(e)
                    ok = False
                    tok = torch.zeros(size, dtype=torch.uint8)
                self.dist.send(tok, dst=self.rank - 1)
            if not last:
                tok = torch.empty(size, dtype=torch.uint8)
                self.dist.recv(tok, src=self.rank + 1)
                b = bytes(tok.numpy().tobytes())
                if not any(b):
                    ok = False
                else:
                    try:
                        self.engine.portOpen(PortHandle.frombytes(b))
                        self._out_token = b
                    except Exception as e:
                        self.p2p_error = str(e)
                        ok = False
        except Exception as e:            # transport of the tokens itself failed
            self.p2p_error = str(e)
            ok = False
        return ok

    def verify_p2p(self, m, j0, j1, all_min, budget_s=60.0):
        """Functional check of the port transport before anything is timed: the same short chain (m rows) once
        through the ports and once through the host.  True only if, on EVERY rank, the port run came through within
        `budget_s` seconds of waiting and gave the band the same inbound column (crc32) and the same best cell as the
        host run -- a peer mapping that opens but does not deliver (a kernel that never sees the neighbour's counter
        move, or sees it move before the cells) shows up here, bounded in time, instead of in the measurement.
        `all_min(int) -> int` is a collective MIN over the ranks (every rank calls it twice).  On False the caller
        switches all ranks to transport="host"."""
        if self.transport != "p2p":
            return True
        # the check's time budget: the engine's in-kernel waits (mi355sw_config.wait_seconds) and this driver's stall limit
        saved_wait, saved_stall, saved_prune = self.engine._opts["wait_seconds"], self.stall_abort_s, self.prune_blocks
        self.engine.configure(wait_seconds=budget_s)
        self.stall_abort_s = budget_s
        # the check compares boundary COLUMNS: with block pruning a skipped slab leaves a lower bound in them and which slabs are
        # skipped depends on when the chain's best score arrives -- two runs of the same chain may then differ cell by cell and
        # still both be right (seen at N = 8: bands 5-7, same best cell, different crc).  The check runs unpruned.
        self.prune_blocks = False
        got = {}
        try:
            for transport in ("p2p", "host"):
                self.transport = transport
                ok = 1
                try:
                    best = self.run(m, j0, j1, digest_inbound=True)
                    got[transport] = (tuple(int(x) for x in best), self.inbound_crc)
                except Exception as e:          # a wait that ran out, a stalled band, a refused mapping
                    self.p2p_error = "%s run of the transport check: %s" % (transport, e)
                    ok = 0
                    _stop_stream(self.engine, (AlignerError, AttributeError))
                if all_min(ok) == 0:
                    return False
            same = 1 if got["p2p"] == got["host"] else 0
            if not same:
                self.p2p_error = "port run and host run of the transport check differ: %r vs %r" % (got["p2p"], got["host"])
            return all_min(same) == 1
        finally:
            self.transport = "p2p"
            self.stall_abort_s = saved_stall
            self.prune_blocks = saved_prune
            try:
                self.engine.configure(wait_seconds=saved_wait)
            except AlignerError:            # (a stream the check left active: the caller closes the engine)
                self.engine._opts["wait_seconds"] = saved_wait

    def run(self, m, j0, j1, recurrence=SMITH_WATERMAN, track_best=True, first_row_init_type=INIT_WITH_ZEROES,
            first_col_init_type=INIT_WITH_ZEROES, poll_sleep=0.0005, want_last_row=False, before_end=None,
            force_int32=False, digest_inbound=False, special_row_interval=0, special_row_sink=None, n_total=None,
            keep_inbound=False, prune_end=0, row0=0, first_row=None, inbound_prefix=None, initial_bound=None):
        """seq1 of the engine must already hold the whole horizontal sequence (or at least [j0,j1)).
        digest_inbound: leave the crc32 of the boundary column this band received in self.inbound_crc (host transport:
        the segments as they arrive; p2p: the port's memory, read back once the band is through).
        special_row_interval > 0: the band keeps its [j0, j1) slice of every special row (the reference: one Special
        Rows Area per forked node, work.tmp/FORK.NN, Job.cpp:123-128); `special_row_sink(dp_row, first_cell, cells)`
        gets each row as soon as its strip is complete -- cells = (H,F) of columns j0..j1-1, first_cell = the boundary
        column's cell of that row with f = -INF (AbstractDiagonalAligner.cpp:290-298).
        n_total: width of the whole matrix (default j1 of the last band = this band's j1): block pruning bounds what an
        alignment can still gain by the rows and columns left in the SUPER-partition (M3).
        keep_inbound: leave the whole boundary column this band received, corner cell first, in self.inbound_column
        ((m+1, 2) cells (H,E)) -- what the reference tees into C00000000.INIT_WITH_CUSTOM_DATA (sw_stage1.cpp:186-191);
        8 bytes of host memory per row (2 GB at C5's 249 M rows), like the file it becomes.
        prune_end 1 / 2 / 3: the alignment ends anywhere on the last row / the last column / either of the WHOLE matrix
        (NEEDLEMAN_WUNSCH, track_best=False).  Every band keeps its slice of the last row (bit 1) and the last band its last
        column (bit 2); after the kernel the best of the edge cells this band holds is read where it lies (streamEdgeBest) into
        self.edge_best, and reduce_edge_best() gives the chain's.  With prune_blocks the engine hears of the edge before
        every streamBegin (setPruneEnd) and skips what cannot reach it; without, every cell is computed and the result is the
        same.  The int32 restart after an overflow computes every cell too.
        row0 = r > 0 (a band that is resumed, serial_band_stage1(resume=True); host transport or a single band): the band runs
        rows (r, m] only, as Partition(r, j0, m, j1).  first_row: the n + 1 cells (H,F) of DP row r, boundary cell first (the
        special row as it lies on disk); inbound_prefix: cells 0..r of the inbound column, corner first (every band but the
        first) -- its cell r is the partition's corner, and the left neighbour sends rows r.. only.  Outbound segments start
        at row r, special rows come on the grid of the whole band and reach the sink with their row of the whole band, and
        pruning counts m - r rows to the end of the matrix.
        initial_bound: the bound the FIRST band's pruning starts from in place of the diagonal seed (the bound a resumed chain
        started from); the other bands hear theirs from the left.
        The stream is cleaned up behind the run: whatever ends it once its stream has begun -- an engine error, an exception
        out of `special_row_sink` or out of the link to the next band, a stalled chain -- the kernel is stopped (streamAbort)
        and the stream ended before the exception travels on, so the engine takes the next streamBegin."""
        job = _BandRun(self, poll_sleep, before_end, digest_inbound, special_row_interval, special_row_sink)
        try:
            job.plan(m, j0, j1, recurrence, track_best, first_row_init_type, first_col_init_type, want_last_row, force_int32,
                     n_total, keep_inbound, prune_end, row0, first_row, inbound_prefix)
            job.start(initial_bound)
            job.find_special_rows()
            job.start_side_threads()
            job.poll()
            return job.finish()
        except BaseException:
            job.stop()
            raise

    def reduce_best(self, best):
        """global best = canonical max over bands (reference: relay through AlignerPool files)."""
        if self.dist is None or self.world == 1:
            return best
        import torch
        t = torch.tensor(list(best), dtype=torch.int64, device=self.device if self.device is not None else "cpu")
        out = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        best = canonical_best([tuple(int(x) for x in o.tolist()) for o in out])
        if self.prune_blocks:
            check_chain_bound(best[2], self.initial_bound)
        return best

    def reduce_edge_best(self):
        """the result of a run(prune_end=1..3) on every rank: the best cell of the allowed edge(s) of the whole matrix, the
        canonical maximum (score desc, i asc, j asc) over the bands' edge_best -- what Stage1Manager.getBestScore() gives for
        the same form on one partition, as a 0-based cell.  Collective.  A pruning chain is held to the bound it started from."""
        return self.reduce_best(self.edge_best if self.edge_best is not None else (-1, -1, -INF))


class _BandRun:
    """One BandRunner.run(): what its steps and its two side threads share, and the steps, in the order run() takes them.
    stop() is run()'s clean-up when one of them raises."""

    def __init__(self, runner, poll_sleep, before_end, digest_inbound, special_row_interval, special_row_sink):
        self.runner, self.eng, self.dist = runner, runner.engine, runner.dist
        self.rank, self.world = runner.rank, runner.world
        self.first, self.last = runner.rank == 0, runner.rank == runner.world - 1
        self.p2p = runner.transport == "p2p"
        self.host_fed = not self.first and not self.p2p      # the inbound column arrives in row segments, through the host
        self.poll_sleep, self.before_end, self.digest_inbound = poll_sleep, before_end, digest_inbound
        self.interval, self.sink = special_row_interval, special_row_sink
        self.lock = threading.Lock()     # the engine handle is driven by one thread at a time
        self.errors = []                 # what ended a side thread; surfaced by the poll loop
        self.fed = 0                     # rows of the inbound column handed to the engine so far (host transport)
        self.special_dp, self.special_next = [], 0       # DP rows of the engine's special rows; the next one to hand over
        self.inbound_h = None
        self.send_q = 0                  # outbound segments sent so far
        self.rx_stop, self.bx_stop = threading.Event(), threading.Event()
        self.rx = self.bx = None
        self.stream_open = False

    # -- validate and plan -------------------------------------------------------------------------------------
    def plan(self, m, j0, j1, recurrence, track_best, first_row_init_type, first_col_init_type, want_last_row, force_int32,
             n_total, keep_inbound, prune_end, row0, first_row, inbound_prefix):
        runner = self.runner
        check_prune_end(prune_end, recurrence, track_best)
        runner.edge_best = None
        runner.inbound_crc = 0 if self.digest_inbound else None
        runner.inbound_column = np.empty((m + 1, 2), dtype=np.int32) if (keep_inbound and not self.first) else None
        row0 = int(row0)
        if row0 and (not 0 < row0 < m or first_row is None or self.p2p or (not self.first and inbound_prefix is None)):
            raise ValueError("run(row0=%d): a row inside the band, its first row, the inbound column above it, no column port" % row0)
        self.part = Partition(row0, j0, m, j1)
        self.row0, self.m_all, self.m = row0, m, m - row0     # m counts the rows of the partition; the engine's rows are relative to row0
        self.seg = runner.segment_rows
        self.nseg = (self.m + self.seg - 1) // self.seg
        # local alignments prune against the chain's running best score; global ones (NEEDLEMAN_WUNSCH with nothing tracked:
        # the answer is the last cell of the last band) against a running lower bound of that cell, AbstractBlockPruning.cpp:92-109
        self.prune = bool(runner.prune_blocks and (track_best if recurrence == SMITH_WATERMAN else not track_best))
        self.prune_end, self.edges_here = prune_end, _edges_held(prune_end, self.last)
        self.recurrence, self.n_total = recurrence, n_total
        self.first_row_init_type, self.first_col_init_type = first_row_init_type, first_col_init_type
        kw = _stream_keywords(self.m, j0, n_total if n_total is not None else j1, self.first, self.last, self.p2p, self.world > 1,
                              recurrence, track_best, first_row_init_type, first_col_init_type, prune_end, self.prune,
                              want_last_row, force_int32)
        if self.interval > 0:
            kw.update(special_row_interval=int(self.interval))
            if self.host_fed:
                # (special rows sit on multiples of the strip height, every strip height is a multiple of 256: the boundary
                #  column's H at every 256th row covers whatever geometry a restart on the int32 kernels picks)
                self.inbound_h = np.zeros(m // 256 + 2, dtype=np.int32)
        if row0:
            # the rest of the band: DP row row0 as it was saved is the first row, its leading cell the boundary column's
            kw.update(first_row_init_type=INIT_WITH_CUSTOM_DATA, first_row=np.ascontiguousarray(first_row, dtype=np.int32))
            if self.first:
                kw.update(first_column_start_offset=row0)
            else:
                prefix = np.asarray(inbound_prefix, dtype=np.int32).reshape(-1, 2)
                if len(prefix) != row0 + 1:
                    raise ValueError("run(row0=%d): inbound_prefix holds %d cells, not %d" % (row0, len(prefix), row0 + 1))
                if runner.inbound_column is not None:
                    runner.inbound_column[:row0 + 1] = prefix
                kw.update(first_column=prefix[row0:row0 + 1].copy())
        elif runner.inbound_column is not None:
            runner.inbound_column[0] = kw["first_column"][0]
        self.kw = kw

    # -- ordered start -----------------------------------------------------------------------------------------
    def start(self, initial_bound):
        """Ordered start: band g+1 launches its kernel only after band g has launched its own.  It could do nothing
        before band g's first strip is through anyway, and where bands SHARE a GPU (tests and rehearsals on a
        one-GPU box) a kernel that sits polling for its neighbour has been seen to keep that neighbour's set-up
        work (fills, the seed pass) off the GPU for tens of seconds.
        The token always travels, whatever happens to this band's own start: 1 = started, 0 = failed (no memory for the
        special rows, a port that is not there) -- a band that never hears from its left neighbour would sit in recv
        with no kernel running and nothing for the stall watchdog to see, and so would every band to its right.
        With the token travels what the pruning bound starts from: band 0 runs the diagonal seed pass of the WHOLE matrix
        before it starts (the bands to its right could not start earlier anyway) and every band begins with that value."""
        runner, dist, first, last = self.runner, self.dist, self.first, self.last
        if self.p2p:
            runner._exchange_ports(self.m)
        bound = None
        if not first and dist is not None:
            go = _start_token(False, None)
            dist.recv(go, src=self.rank - 1)
            if int(go[0]) != 1:
                if not last:
                    dist.send(_start_token(False, None), dst=self.rank + 1)
                raise RuntimeError("band %d/%d: a band to the left failed to start its kernel" % (self.rank, self.world))
            bound = None if int(go[1]) == NO_BOUND else int(go[1])
        try:
            if first and initial_bound is not None:
                bound = int(initial_bound)
            elif first and self.prune and runner.seed_bound and self.world > 1 and self.n_total is not None:
                bound = _seed_bound(self.eng, self.m_all, self.n_total, self.recurrence, self.prune_end,
                                    self.first_row_init_type, self.first_col_init_type)
            if self.prune and bound is not None:
                self.kw.update(initial_bound=bound)
            runner.initial_bound = bound
            self.begin(self.kw)
        except BaseException:
            if not last and dist is not None:
                dist.send(_start_token(False, None), dst=self.rank + 1)
            raise
        if not last and dist is not None:
            dist.send(_start_token(True, bound), dst=self.rank + 1)
        runner.restarts = 0
        runner.special_rows = []

    def begin(self, kw):
        _arm_prune_end(self.eng, self.prune_end, self.runner.prune_blocks)
        self.eng.streamBegin(self.part, **kw)
        self.stream_open = True

    # -- restart on the int32 kernels --------------------------------------------------------------------------
    def may_restart(self, e):
        """an overflow report of the packed kernels, once: not on the int32 kernels, which have no such range"""
        return "EOVERFLOW16" in str(e) and not self.kw.get("force_int32") and self.runner.restarts == 0

    def begin_on_int32(self):
        """the packed kernel left its exact range: everything handed out so far is exact (the engine only
        reports rows below the failing strip), so the band starts again on the int32 kernel and REPLAYS --
        the inbound rows already received are still in the engine's column (pinned, or the port), outbound
        segments already sent are not sent again (a port is simply written again with the same cells).
        Called with the lock held and no stream open."""
        kw = dict(self.kw, force_int32=True)
        if self.host_fed:
            kw["first_column_resume_rows"] = self.fed
        self.begin(kw)
        self.runner.restarts += 1

    # -- inbound receiver (host transport) ---------------------------------------------------------------------
    def receive(self):
        """inbound boundary column: blocking recv of row segments from the left neighbour"""
        runner, row0, inbound_h = self.runner, self.row0, self.inbound_h
        try:
            for q in range(self.nseg):
                r0 = q * self.seg
                ln = min(self.seg, self.m - r0)
                buf = runner._tensor(ln)
                self.dist.recv(buf, src=self.rank - 1)
                if self.rx_stop.is_set():          # the run has ended (stop()): nothing more goes to the engine
                    return
                if self.digest_inbound:
                    runner.inbound_crc = zlib.crc32(buf.numpy().tobytes(), runner.inbound_crc)
                a0 = row0 + r0                     # the segment's first row in the whole band
                if runner.inbound_column is not None:
                    runner.inbound_column[a0 + 1:a0 + ln + 1] = buf.numpy()
                if inbound_h is not None:          # H of the boundary column at every possible special row
                    q0 = a0 // 256 + 1
                    q1 = (a0 + ln) // 256
                    if q1 >= q0:
                        inbound_h[q0:q1 + 1] = buf.numpy()[q0 * 256 - 1 - a0:q1 * 256 - a0:256, 0]
                with self.lock:
                    self.eng.streamFeedColumn(r0, buf.numpy())
                    self.fed = r0 + ln
        except BaseException as e:     # surfaced by the main loop
            self.errors.append(e)

    # -- running-best exchange (host transport) ----------------------------------------------------------------
    def exchange_best(self):
        """the chain's running best travels between the rank processes (p2p: between the kernels); the thread keeps answering
        the other bands until every band is through"""
        import torch
        runner, eng, dist, bx_stop = self.runner, self.eng, self.dist, self.bx_stop
        known = -INF
        try:
            while True:
                mine = eng.streamRunningBest() if not bx_stop.is_set() else -INF
                t = torch.tensor([max(mine, known), -1 if bx_stop.is_set() else 0], dtype=torch.int64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=runner._best_group)
                if int(t[0]) > known:
                    known = int(t[0])
                    if known > mine and not bx_stop.is_set():
                        try:
                            eng.streamBestHint(known)
                            runner.hints += 1
                        except AlignerError:
                            pass
                if int(t[1]) == -1:                  # every band is through
                    return
                time.sleep(0.002)
        except BaseException as e:
            self.errors.append(e)

    def start_side_threads(self):
        self.runner.hints = 0
        if self.prune and self.world > 1 and not self.p2p and self.runner._best_group is not None:
            self.bx = threading.Thread(target=self.exchange_best, daemon=True)
            self.bx.start()
        if self.host_fed:
            self.rx = threading.Thread(target=self.receive, daemon=True)
            self.rx.start()

    # -- special-row hand-over ---------------------------------------------------------------------------------
    def find_special_rows(self):
        """special rows of this band: DP rows (multiples of the strip height, AbstractDiagonalAligner::isSpecialRow), as the
        stream that has just begun places them.  After a restart on the int32 kernels (other strip heights) the rows
        already handed over stay, the rest are where the new geometry puts them."""
        if self.interval <= 0:
            return
        self.special_dp = []
        while True:
            try:
                dp, _ = self.eng.streamReadSpecialRow(len(self.special_dp), 0, 0)
            except (AlignerError, IndexError):
                break
            self.special_dp.append(int(dp))
        done = self.runner.special_rows
        self.special_next = sum(1 for dp in self.special_dp if done and self.row0 + dp <= done[-1])

    def flush_special(self, rows_ok):
        """hands over every special row whose strip is complete; called with the lock held"""
        while self.special_next < len(self.special_dp) and self.special_dp[self.special_next] <= rows_ok:
            k, dp = self.special_next, self.special_dp[self.special_next]
            if self.host_fed and self.fed < dp:
                return                                  # its boundary cell is still on the way
            _, cells = self.eng.streamReadSpecialRow(k)
            dpa = self.row0 + dp                        # the row in the whole band
            if self.first:
                h = _border_h(self.first_col_init_type, dpa)
            elif self.p2p:
                h = int(self.eng.portRead(dp - 1, 1)[0, 0])
            else:
                h = int(self.inbound_h[dpa // 256])
            if self.sink is not None:
                self.sink(dpa, np.array([h, -INF], dtype=np.int32), cells)
            self.runner.special_rows.append(dpa)
            self.special_next += 1

    # -- the poll / send loop ----------------------------------------------------------------------------------
    def send_segments(self, rows_done):
        """outbound boundary column (host transport): every complete segment goes to the right neighbour"""
        import torch
        sent = False
        while not self.last and not self.p2p and self.send_q < self.nseg:
            r0 = self.send_q * self.seg
            ln = min(self.seg, self.m - r0)
            if rows_done < r0 + ln:
                break
            buf = self.runner._tensor(ln)
            with self.lock:
                buf.copy_(torch.from_numpy(self.eng.streamReadColumn(r0, ln)))
            self.dist.send(buf, dst=self.rank + 1)
            self.send_q += 1
            sent = True
        return sent

    def fail(self):
        """a side thread or the watchdog has given up: the stream is stopped and the first error raised"""
        self.bx_stop.set()
        with self.lock:
            _stop_stream(self.eng, AlignerError, guard_abort=False)
            self.stream_open = False
        if self.bx is not None:           # (it leaves its loop at the next all_reduce in which every band has said stop)
            self.bx.join(timeout=5.0)
        raise self.errors[0]

    def poll(self):
        # a chain that stands still says where: one line per 10 s without progress on this band (rows completed,
        # segments sent), one per second with MI355SW_BAND_DEBUG=1; after MI355SW_BAND_STALL_S seconds (default
        # 900) without progress the band gives up instead of hanging its neighbours for ever
        debug = os.environ.get("MI355SW_BAND_DEBUG") == "1"
        stall_abort = self.runner.stall_abort_s if self.runner.stall_abort_s is not None else float(os.environ.get("MI355SW_BAND_STALL_S", "900"))
        t_dbg = t_prog = time.time()
        seen = (-1, -1)
        rows_done, fin = 0, False
        while True:
            now = time.time()
            if now - t_dbg >= (1.0 if debug else 10.0):
                t_dbg = now
                if (rows_done, self.send_q) != seen:
                    seen, t_prog = (rows_done, self.send_q), now
                if debug or now - t_prog >= 10.0:
                    sys.stderr.write("[band %d/%d] rows_done=%d/%d finished=%d segments_sent=%d/%d no progress for %.0f s\n"
                                     % (self.rank, self.world, rows_done, self.m, int(fin), self.send_q, self.nseg, now - t_prog))
                    sys.stderr.flush()
                if now - t_prog >= stall_abort:
                    self.errors.append(RuntimeError("band %d/%d: no progress for %.0f s (rows_done=%d/%d, segments_sent=%d/%d)"
                                                    % (self.rank, self.world, now - t_prog, rows_done, self.m, self.send_q, self.nseg)))
            if self.errors:
                self.fail()
            with self.lock:
                try:
                    rows_done, fin = self.eng.streamPoll()
                except AlignerError as e:
                    if not self.may_restart(e):
                        raise
                    if os.environ.get("MI355SW_VERBOSE"):
                        print("[bands] band %d/%d restarts on the int32 kernels: %s" % (self.rank, self.world, e), file=sys.stderr)
                    _stop_stream(self.eng, AlignerError)
                    self.begin_on_int32()
                    self.find_special_rows()
                    continue
                # (device-resident rows are read through the copy stream: only once nothing more has to be fed, so that
                #  a copy held up behind the running kernel cannot starve that kernel of its first column)
                if self.special_dp and (not self.host_fed or self.fed >= self.m or fin):
                    self.flush_special(rows_done)
            sent = self.send_segments(rows_done)
            if fin and (self.last or self.p2p or self.send_q >= self.nseg):
                return
            if not sent:
                time.sleep(self.poll_sleep)

    # -- finish ------------------------------------------------------------------------------------------------
    def end_stream(self):
        """the end of a stream that has computed every row: the edge best is read, `before_end` called, the stream ended.
        Returns the band's best, or None where streamEnd reported an overflow that a run on the int32 kernels answers."""
        if self.edges_here:
            self.runner.edge_best = tuple(int(x) for x in self.eng.streamEdgeBest(self.edges_here))
        if self.before_end is not None:       # e.g. read this band's slice of the last row while the stream is open
            self.before_end(self.eng)
        self.bx_stop.set()                   # the exchange thread keeps answering the other bands until every band is through
        try:
            return self.eng.streamEnd()[0]
        except AlignerError as e:            # e.g. reported by the exact-position pass of a very tall band
            if not self.may_restart(e):
                raise
            return None

    def finish(self):
        if self.rx is not None:
            self.rx.join()
        if self.special_dp:
            with self.lock:
                self.flush_special(self.m)
        if self.digest_inbound and self.p2p and not self.first:
            self.runner.inbound_crc = zlib.crc32(np.ascontiguousarray(self.eng.portRead(0, self.m), dtype=np.int32).tobytes())
        if self.runner.inbound_column is not None and self.p2p:
            self.runner.inbound_column[1:] = self.eng.portRead(0, self.m)
        best = self.end_stream()
        if best is None:
            with self.lock:              # (the stream is over and every special row handed over: nothing to stop, nothing to probe)
                self.begin_on_int32()
            while not self.eng.streamPoll()[1]:          # (rows done, finished)
                time.sleep(self.poll_sleep)
            best = self.end_stream()
        self.stream_open = False
        if self.bx is not None:
            self.bx.join()
        if self.errors:
            raise self.errors[0]
        return best

    def stop(self):
        self.rx_stop.set()
        self.bx_stop.set()
        if self.rx is not None:            # (a receiver in the middle of a feed finishes it before the stream goes)
            self.rx.join(timeout=5.0)
        if self.stream_open:
            self.stream_open = False
            _stop_stream(self.eng, Exception)


class InProcessChain:
    """The whole band chain driven by ONE host process: handle k runs band k on GPU `devices[k]`, the boundary columns
    travel through column ports attached with mi355sw_port_attach -- hipDeviceEnablePeerAccess between the devices of one
    process, no hipIpc handle and no second process involved.  The streaming calls never block (begin launches the
    persistent kernel, poll reads pinned words), so one thread serves all bands.

    It is the SECOND device-side transport of bench.py: when the ranks' hipIpc mappings fail their check (probe_p2p /
    verify_p2p) rank 0 runs the chain this way ("comm": "p2p-attach") before anybody falls back to pinned host columns +
    gloo; and it is how a single process uses several GPUs (tools, tests).  The reference has no such mode: its bands are
    forked processes chained by sockets (M/libmasa/libmasa.cpp:540-642).
    Score passes only (best cell, or H[m][n] of a global alignment): special rows per band are BandRunner's job."""

    def __init__(self, aligners, prune_blocks=False, seed_bound=True):
        self.aligners = list(aligners)
        self.prune_blocks = prune_blocks
        self.seed_bound = seed_bound       # pruning: the diagonal seed of the whole matrix first (chain_seed_bound)
        self.initial_bound = None
        self.restarts = 0
        self.before_end = None             # before_end(k, aligner): band k is through and its stream still open (tools, tests)
        self._rows = 0

    def attach(self, m):
        """ports of m rows between consecutive bands (made once; a later run of at most m rows resets them)"""
        als = self.aligners
        if self._rows >= m:
            for k in range(1, len(als)):
                als[k].portReset()
            return
        for k in range(1, len(als)):
            als[k].portCreate(m)
            als[k - 1].portAttach(als[k])
        self._rows = m

    def run(self, m, limits, recurrence=SMITH_WATERMAN, first_row_init_type=INIT_WITH_ZEROES, first_col_init_type=INIT_WITH_ZEROES,
            force_int32=False, poll_sleep=0.0005, prune_end=0, initial_bound=None):
        """limits = band_limits(n, weights): band k = columns [limits[k], limits[k+1]).  Returns (best, per-band statistics):
        best = the canonical best cell of the chain (0-based), or for NEEDLEMAN_WUNSCH (m-1, n-1, H[m][n]).
        prune_end 1 / 2 / 3 (NEEDLEMAN_WUNSCH): the alignment ends on the last row / the last column / either, and best is the
        best cell of that edge (BandRunner.run); the int32 retry after an overflow computes every cell.
        initial_bound: a caller's first bound of a pruning chain -- the score of an admissible alignment that exists; the
        larger of it and the seed's is what every band starts from, and what the result is held to (check_chain_bound)."""
        als, N = self.aligners, len(self.aligners)
        n = limits[-1]
        sw = recurrence == SMITH_WATERMAN
        check_prune_end(prune_end, recurrence, sw)
        self.attach(m)
        self.initial_bound = None
        if self.prune_blocks and self.seed_bound and N > 1:
            self.initial_bound = _seed_bound(als[0], m, n, recurrence, prune_end, first_row_init_type, first_col_init_type)
        if self.prune_blocks and initial_bound is not None:
            self.initial_bound = int(initial_bound) if self.initial_bound is None else max(self.initial_bound, int(initial_bound))
        for attempt in (0, 1):
            begun = []
            try:
                for k in range(N):                         # left to right: band k+1's kernel starts after band k's
                    last = k == N - 1
                    # (every column travels through a port; a global run that ends in the last cell reads it from the last row)
                    kw = _stream_keywords(m, limits[k], n, k == 0, last, True, N > 1, recurrence, sw, first_row_init_type,
                                          first_col_init_type, prune_end, self.prune_blocks, not sw and last,
                                          bool(force_int32 or attempt))
                    if self.prune_blocks and self.initial_bound is not None:
                        kw.update(initial_bound=self.initial_bound)
                    _arm_prune_end(als[k], prune_end, self.prune_blocks)
                    als[k].streamBegin(Partition(0, limits[k], m, limits[k + 1]), **kw)
                    begun.append(k)
                open_ = set(range(N))
                while open_:
                    for k in sorted(open_):
                        _rows, fin = als[k].streamPoll()
                        if fin:
                            open_.discard(k)
                    if open_:
                        time.sleep(poll_sleep)
                bests, stats, h_last = [], [], None
                for k in range(N):
                    if prune_end:
                        here = _edges_held(prune_end, k == N - 1)
                        edge = als[k].streamEdgeBest(here) if here else (-1, -1, -INF)
                    elif not sw and k == N - 1:
                        h_last = int(als[k].streamReadLastRow(col=limits[k + 1] - limits[k] - 1, length=1)[0, 0])
                    if self.before_end is not None:
                        self.before_end(k, als[k])
                    b, _ = als[k].streamEnd()
                    bests.append(edge if prune_end else b)
                    stats.append(als[k].getStatistics())
                best = canonical_best(bests) if (sw or prune_end) else (m - 1, n - 1, h_last)
                if self.prune_blocks:
                    check_chain_bound(best[2], self.initial_bound)
                return best, stats
            except AlignerError as e:
                for k in begun:                            # stop whatever is running, then the whole chain again on the int32 kernels
                    _stop_stream(als[k], AlignerError)
                if "EOVERFLOW16" not in str(e) or force_int32 or attempt == 1:
                    raise
                self.restarts += 1
                self.attach(m)


def _special_row_spacing(m, n, sra_limit, extent=None):
    """rows between two special rows of a band's area of `sra_limit` bytes (0: none are kept).  The spacing follows the sizes of
    the whole, untrimmed matrix (Job.cpp:62-67): `extent`, or m x n"""
    em, en = extent if extent is not None else (m, n)
    return sra_mod.flush_interval(em, en, sra_limit) if sra_limit > 0 else 0


def _band_area(runner, m, j0, j1, bwork, sra_limit, n_total, recurrence, first_row_init_type, first_col_init_type, origin, run_kw,
               extent=None, resume=None):
    """one band's stage 1 into the Special Rows Area of `bwork` (band_stage1 and serial_band_stage1 share it): the partition
    directory, the special rows with their boundary cell, the last row, the markers and the tee'd boundary column.  Returns
    (the band's own best as the engine reports it -- for a global run that ends in the last cell, prune_end 0 and nothing
    tracked, the last band's (m-1, j1-1, H[m][j1]) and nothing for the others --, the partition, the DP rows written).
    origin = (i, j): the cell of the whole matrix the chain's (0, 0) is (a --trim: the files keep absolute coordinates)."""
    first, last = runner.rank == 0, runner.rank == runner.world - 1
    oi, oj = origin
    os.makedirs(bwork, exist_ok=True)
    interval = _special_row_spacing(m, n_total if n_total is not None else j1, sra_limit, extent)
    area = sra_mod.SpecialRowsArea(sra_mod.special_rows_path(bwork, 1, 0), disk_limit=max(sra_limit, 1))
    part = area.create_partition(oi, oj + j0, oi + m, oj + j1)
    part.set_border_markers(first_row_init_type, j0, first_col_init_type if first else INIT_WITH_CUSTOM_DATA, 0)
    run_kw = dict(run_kw)
    kept = []
    if resume is not None:           # serial_band_stage1(resume=True): where the band starts, what stays of an earlier run
        kept, restart = resume.begin(part, interval)
        run_kw.update(restart)

    def sink(dp, c0, cells):
        part.write(oi + dp, np.concatenate([np.asarray(c0, dtype=np.int32).reshape(1, 2), cells]))
        if resume is not None:
            resume.special_row(dp)

    got = {}
    prev_end = run_kw.pop("before_end", None)

    def before_end(eng):
        got["row"] = eng.streamReadLastRow()
        if prev_end is not None:
            prev_end(eng)
    band_best = runner.run(m, j0, j1, recurrence=recurrence, first_row_init_type=first_row_init_type,
                           first_col_init_type=first_col_init_type, special_row_interval=interval,
                           special_row_sink=sink if interval > 0 else None, n_total=n_total, want_last_row=True,
                           before_end=before_end, keep_inbound=not first, **run_kw)
    if first:
        lead = _border_h(first_col_init_type, m)
    else:
        lead = int(runner.inbound_column[m, 0])
        runner.inbound_column.tofile(os.path.join(part.path, "C00000000.INIT_WITH_CUSTOM_DATA"))
    if m not in runner.special_rows:              # the partition's last row: sw_stage1.cpp:203-240's completion marker
        part.write(oi + m, np.concatenate([np.array([[lead, -INF]], dtype=np.int32), got["row"]]))
    part.close()
    if recurrence == NEEDLEMAN_WUNSCH and not run_kw.get("prune_end") and not run_kw.get("track_best", True):
        # both ends in the corners: the result is the last cell of the last band, read from the row just written
        band_best = (m - 1, j1 - 1, int(got["row"][-1, 0])) if last else (-1, -1, -INF)
    return band_best, part, kept + list(runner.special_rows) + ([m] if m not in runner.special_rows else [])


def _write_chain_best(bwork, best, origin=(0, 0)):
    """`crosspoints/crosspoint_01.00` of a band: the chain's best, the engine's 0-based cell as DP coordinates of the whole matrix"""
    if best[0] >= 0 or best[1] >= 0:
        best = (best[0] + 1 + origin[0], best[1] + 1 + origin[1], best[2])
        sra_mod.write_crosspoint(sra_mod.crosspoint_path(bwork, 1, 0), best)
    return tuple(best)


def band_stage1(runner, m, j0, j1, work, sra_limit, n_total=None, recurrence=SMITH_WATERMAN,
                first_row_init_type=INIT_WITH_ZEROES, first_col_init_type=INIT_WITH_ZEROES, **run_kw):
    """Stage 1 of one band with its Special Rows Area: what a forked MASA-Core node leaves in its own work directory
    (`work`/FORK.NN, Job::initializeWorkPath, M/common/Job.cpp:118-128) -- partition directory
    `00000000.<j0>.<m>.<j1>` in absolute coordinates, one file per special row with (j1-j0+1) cells whose leading cell
    is the boundary column's, the last row as the completion marker, the border markers (row marker at offset j0), and
    for every band but the first the boundary column it received as `C00000000.INIT_WITH_CUSTOM_DATA` (the tee of
    sw_stage1.cpp:186-191), so that stage 2 can walk back through this band and hand over to the band on its left at
    that column.  The spacing of the rows follows `sra_limit` (the node's --disk-size) and the size of the WHOLE
    matrix, m x n_total -- a split is a trim, and Job.cpp:62-67 computes the interval from the untrimmed sizes --
    rounded up to the engine's strip height.
    Collective: every rank of the chain calls it.  Returns {"best": the chain's best (i, j, score) in 1-based DP
    coordinates as stage1.py's, "band_best": this band's own, as the engine reports it (0-based cell), "work":
    this band's work directory, "special_rows": DP rows written}; `crosspoints/crosspoint_01.00` of every band holds
    the chain's best (the reference: the running best relayed along the chain, sw_stage1.cpp:421-464 -- the last
    node's file is the one that counts there).
    prune_end=1..3 (with recurrence=NEEDLEMAN_WUNSCH, track_best=False; BandRunner.run): "best" is the chain's best cell of the
    allowed edge(s).  With prune_blocks the special rows are lower bounds, exact on every value that can still reach that
    best (include/mi355sw.h, mi355sw_set_prune_end).
    A global run that ends in the last cell (NEEDLEMAN_WUNSCH, track_best=False, prune_end 0): "best" is (m, n, H[m][n]), which
    the last band reads from its last row -- what the traceback through the chain starts from (bands.band_traceback).
    serial_band_stage1 leaves the same files with the bands run one after the other on one engine.
    No resume here: serial_band_stage1(resume=True) continues a killed serial chain; a coordinated restart of the ranks of this
    collective form is a separate piece of work."""
    bwork = os.path.join(work, "FORK.%02d" % runner.rank) if runner.world > 1 else work
    band_best, _part, rows = _band_area(runner, m, j0, j1, bwork, sra_limit, n_total, recurrence, first_row_init_type,
                                        first_col_init_type, (0, 0), run_kw)
    # (prune_end: the result lies on an edge of the whole matrix, nothing is tracked -- the chain's best is the edge's)
    best = runner.reduce_edge_best() if run_kw.get("prune_end") else runner.reduce_best(band_best)
    best = _write_chain_best(bwork, best)
    return {"best": tuple(best), "band_best": tuple(band_best), "work": bwork, "special_rows": rows}


class _SerialLink:
    """torch.distributed's send / recv between a band and the band the same process runs next: what band k sends -- its start
    token, then its last column in row segments -- waits here until band k+1 asks for it"""

    def __init__(self):
        import collections
        self.queue = collections.deque()
        self.on_segment = None           # on_segment(cells): every row segment of a last column, before it is queued

    def send(self, t, dst=None):
        if self.on_segment is not None and t.dim() == 2:     # (the start token is one row of two int64)
            self.on_segment(t.numpy())
        self.queue.append(t.clone())

    def recv(self, t, src=None):
        t.copy_(self.queue.popleft())

    def raise_bound(self, bound):
        """the start token at the head of the queue carries what the next band's pruning starts from: never less than `bound`"""
        if bound is not None and self.queue:
            self.queue[0][1] = max(int(self.queue[0][1]), int(bound))

    def feed(self, column, row0, segment_rows, bound=None):
        """what a band that ran in an earlier process would have sent: its start token (with `bound`) and rows row0.. of its last
        column (`column`: corner cell first) in segments, for the band that is resumed"""
        import torch
        self.queue.clear()
        self.queue.append(torch.tensor([1, NO_BOUND if bound is None else int(bound)], dtype=torch.int64))
        rows = len(column) - 1
        for r in range(row0, rows, segment_rows):
            self.queue.append(torch.from_numpy(np.ascontiguousarray(column[1 + r:1 + min(r + segment_rows, rows)])))


# ---------------------------------------------------------------------------------------------------------------------------
# resume of a serial chain (serial_band_stage1(resume=True)): two files per band next to what band_stage1 leaves
#   chain.mi355        JSON, written as .tmp and renamed, always AFTER the files it speaks of: the key of the run, the band, and
#                      either the finished band's record or how far an unfinished band is known to be on disk
#   last_column.mi355  the band's outbound boundary column, the next band's corner cell first, raw (H, E) int32 pairs, appended
#                      segment by segment; removed once the next band is done (its C00000000.INIT_WITH_CUSTOM_DATA holds the cells)
# ---------------------------------------------------------------------------------------------------------------------------
CHAIN_STATE, CHAIN_COLUMN, CHAIN_STATE_VERSION = "chain.mi355", "last_column.mi355", 1


def _save_chain_state(bwork, state):
    fn = os.path.join(bwork, CHAIN_STATE)
    with open(fn + ".tmp", "w") as f:
        json.dump(state, f, sort_keys=True)
        f.write("\n")
        f.flush()
        os.fsync(f.fileno())
    os.replace(fn + ".tmp", fn)


def _rows_on_disk(bwork):
    """DP rows (ids) of the complete special rows under a band's work directory, without creating anything"""
    rows = []
    for d, _dirs, files in os.walk(os.path.join(bwork, "special_rows", "stage.01.00")):
        rows += [int(f, 16) for f in files if len(f) == 8 and all(c in "0123456789ABCDEF" for c in f)]
    return sorted(rows)


def _load_chain_state(bwork, key, band):
    """the state a band left, checked against this call: None when the band's directory holds nothing to continue"""
    fn = os.path.join(bwork, CHAIN_STATE)
    if not os.path.exists(fn):
        if _rows_on_disk(bwork):
            raise RuntimeError("serial_band_stage1: %s holds special rows but no %s: cannot resume (clean the work directory)"
                               % (bwork, CHAIN_STATE))
        return None
    state = json.load(open(fn))
    if state.get("version") != CHAIN_STATE_VERSION:
        raise ValueError("serial_band_stage1: %s is of format version %r, this is version %d (clean the work directory)"
                         % (fn, state.get("version"), CHAIN_STATE_VERSION))
    theirs = dict(state.get("key", {}), band=state.get("band"))
    for name, mine in sorted(dict(key, band=band).items()):
        if theirs.get(name) != mine:
            raise ValueError("serial_band_stage1: %s was left by a run with %s = %r, this one has %r (clean the work directory)"
                             % (fn, name, theirs.get(name), mine))
    return state


def _inbound_file(works, k, m):
    """where band k's inbound boundary column lies whole ((m + 1) cells, corner first): the last_column.mi355 of the band on
    its left, or -- band k was done once and that file went -- band k's own tee of it; None when neither is there"""
    fn = os.path.join(works[k - 1], CHAIN_COLUMN)
    if os.path.exists(fn) and os.path.getsize(fn) >= 8 * (m + 1):
        return fn
    for d, _dirs, files in os.walk(os.path.join(works[k], "special_rows", "stage.01.00")):
        fn = os.path.join(d, "C00000000.INIT_WITH_CUSTOM_DATA")
        if "C00000000.INIT_WITH_CUSTOM_DATA" in files and os.path.getsize(fn) == 8 * (m + 1):
            return fn
    return None


def _left_by_earlier_runs(works, m, limits, n_total, sra_limit, origin, extent, recurrence, first_row_init_type,
                          first_col_init_type, prune_blocks, prune_end, track_best):
    """serial_band_stage1(resume=True): what the bands left in `works`, checked before anything runs.  Returns (the key of this
    run, the state of every band or None, the first band that has to run)."""
    N = len(works)
    key = {"m": int(m), "limits": [int(x) for x in limits], "origin": [int(x) for x in origin],
           "extent": [int(x) for x in extent] if extent is not None else None, "n_total": int(n_total),
           "recurrence": int(recurrence), "first_row_init_type": int(first_row_init_type),
           "first_col_init_type": int(first_col_init_type), "track_best": bool(track_best),
           "prune_end": int(prune_end), "prune_blocks": bool(prune_blocks), "sra_limit": int(sra_limit),
           "special_row_interval": int(_special_row_spacing(m, n_total, sra_limit, extent))}
    states = [_load_chain_state(works[k], key, k) for k in range(N)]
    for bwork in works:                               # leftovers of a killed run
        for d, _dirs, files in os.walk(bwork):
            for f in files:
                if f.endswith(".tmp"):
                    os.remove(os.path.join(d, f))
    # bands that are done -- the state says so and the completion marker, the last row, is on disk -- are not run again;
    # the first band that is not needs the column of the band on its left, whole
    k_first = 0
    while k_first < N and states[k_first] is not None and states[k_first].get("done") and m in _rows_on_disk(works[k_first]):
        k_first += 1
    while 0 < k_first < N:
        if _inbound_file(works, k_first, m) is not None:
            break
        k_first -= 1                                  # (no column to start from: the band on the left runs again, from row 0)
        states[k_first] = dict(states[k_first], done=False, rows=[], column_rows=0)
    return key, states, k_first


def _kernel_prunes(name):
    """whether the kernel the engine names in its statistics is a pruning instantiation: sw_strip_kernel_pk16<R,track,local,PRUNE..>,
    sw_strip_kernel<R,local,profile,track,PRUNE> -- the engine may drop a pruning request (include/mi355sw.h), the result is
    the same.  An engine that names no kernel is taken at its word."""
    if not name or "<" not in name:
        return True
    args = name[name.index("<") + 1:].rstrip(">").split(",")
    if "pk16_mixed" in name:
        return len(args) > 2 and args[2] == "true"
    if "pk16" in name:
        return len(args) > 3 and args[3] == "true"
    return len(args) > 4 and args[4] == "true"


class _BandResume:
    """What serial_band_stage1(resume=True) keeps of ONE band while it runs, and where a band that was interrupted starts."""

    def __init__(self, band, bands, bwork, key, m, prev, midband, inbound, link, segment_rows, corner_next, progress):
        self.band, self.last, self.bwork, self.key, self.m = band, band == bands - 1, bwork, key, m
        self.prev, self.midband, self.inbound, self.link, self.segment_rows = prev, midband, inbound, link, segment_rows
        self.corner_next, self.progress = corner_next, progress
        self.bound = None                # what the chain's bound stands at when this band begins
        self.runner = None
        self.state = None
        self.column = None               # last_column.mi355, open for appending
        self.row0 = 0
        self.state_writes = self.column_writes = 0

    def _save(self):
        _save_chain_state(self.bwork, self.state)
        self.state_writes += 1

    def _tell(self, event, row):
        if self.progress is not None:
            self.progress(event, self.band, row)

    def begin(self, part, interval):
        """the row the band starts at and everything run() needs for it; the state says so BEFORE anything below that row goes"""
        m, prev, r = self.m, self.prev, 0
        column_fn = os.path.join(self.bwork, CHAIN_COLUMN)
        if self.midband and interval > 0 and prev is not None and not prev.get("done"):
            on_disk = set(part.rows)
            rows = [x for x in sorted(prev.get("rows", [])) if x in on_disk and 0 < x < m]
            if not self.last:            # ... and no further than the outbound column is known to be on disk
                have = (os.path.getsize(column_fn) // 8 - 1) if os.path.exists(column_fn) else 0
                durable = min(int(prev.get("column_rows", 0)), have)
                rows = [x for x in rows if x <= durable]
            r = rows[-1] if rows else 0
        kept = [x for x in sorted(part.rows) if 0 < x <= r and x in prev.get("rows", [])] if r else []
        self.row0 = r
        self.state = {"version": CHAIN_STATE_VERSION, "key": self.key, "band": self.band, "done": False, "rows": list(kept),
                      "column_rows": r, "initial_bound": prev.get("initial_bound") if (r and prev) else None, "from_row": r}
        self._save()
        for rid in list(part.rows):      # rows below r are written again
            if rid not in kept:
                os.remove(os.path.join(part.path, "%08X" % rid))
        part.rows = list(kept)
        part.reload()
        if not self.last:
            if r:
                self.column = open(column_fn, "r+b")
                self.column.truncate(8 * (1 + r))
                self.column.seek(0, 2)
            else:
                self.column = open(column_fn, "wb")
                self.column.write(self.corner_next.tobytes())
            self.column.flush()
            self.link.on_segment = self.segment
        restart = {}
        if r:
            restart = dict(row0=r, first_row=part.read_row(part.i0 + r))
            if self.inbound is not None:
                restart["inbound_prefix"] = self.inbound[:r + 1]
            elif self.state["initial_bound"] is not None:
                restart["initial_bound"] = self.state["initial_bound"]
        if self.inbound is not None:     # the band on the left ran in an earlier process: its column comes from its file
            self.link.feed(self.inbound, r, self.segment_rows, self.bound)
        return kept, restart

    def _bound_seen(self):
        if self.runner is not None and self.state["initial_bound"] is None and self.runner.initial_bound is not None:
            self.state["initial_bound"] = int(self.runner.initial_bound)

    def special_row(self, dp):
        sra_mod.drain()                  # the row's file is in place (written, renamed) before the state names it
        self._bound_seen()
        self.state["rows"].append(int(dp))
        self._save()
        self._tell("special_row", int(dp))

    def segment(self, cells):
        self.column.write(np.ascontiguousarray(cells, dtype=np.int32).tobytes())
        self.column.flush()
        os.fsync(self.column.fileno())
        self.column_writes += 1
        self._bound_seen()
        self.state["column_rows"] += len(cells)
        self._save()
        self._tell("column", self.state["column_rows"])

    def close(self):
        self.link_off()
        if self.column is not None:
            self.column.close()
            self.column = None

    def link_off(self):
        if self.link is not None:
            self.link.on_segment = None

    def finish(self, record):
        sra_mod.drain()
        self.close()
        self.state = dict({"version": CHAIN_STATE_VERSION, "key": self.key, "band": self.band, "done": True}, **record)
        self._save()


def serial_band_stage1(engine, m, limits, work, sra_limit, n_total=None, recurrence=SMITH_WATERMAN,
                       first_row_init_type=INIT_WITH_ZEROES, first_col_init_type=INIT_WITH_ZEROES, prune_blocks=False,
                       seed_bound=True, segment_rows=1 << 16, origin=(0, 0), extent=None, resume=False, progress=None, **run_kw):
    """The chain of band_stage1, band after band on ONE engine by one process -- the reference's `--split=N --part=1..N`
    sequence: band k runs to its end, its last column (streamReadColumn, on the host) becomes band k+1's first column
    (streamFeedColumn).  limits = band_limits(n, weights): band k = columns [limits[k], limits[k+1]).  Every `work`/FORK.NN
    holds exactly what band_stage1 leaves there on rank k (with one band: `work` itself).  So a single GPU takes a matrix in
    parts, each with its own Special Rows Area.
    prune_blocks: every band prunes against the best of the bands before it -- the bound a band starts from is the largest score
    the chain has found so far (a local chain; last-row cells of a prune_end chain) or the bound the chain started from, so it
    only grows from band to band; the result is held to the first bound (check_chain_bound).  prune_end as band_stage1's.
    origin = (i, j): where the chain's cell (0, 0) lies in the whole matrix (a --trim); directory names, rows and crosspoints
    are absolute, `limits` and `m` relative to it; extent = (rows, columns) of the untrimmed matrix, which the spacing of the
    special rows follows (default: m x n_total).
    Returns {"best": the chain's best (i, j, score) in 1-based DP coordinates, "bands": [per band {"best" (its own, 0-based
    cell), "work", "special_rows", "seconds", "pruned_cells", "initial_bound"}], "limits"}.

    resume=True: a chain that was killed continues from what it left on disk, and a chain that runs through leaves the same
    tree plus one `chain.mi355` per band (the state: the key of the run, the band, `done` and the band's record, or for an
    unfinished band the special rows and the rows of its outbound column known to be on disk; written as .tmp and renamed,
    always after the files it speaks of).  While band k runs, `last_column.mi355` in its directory takes its outbound column
    segment by segment (the next band's corner cell first, raw (H, E) pairs); it goes once band k+1 is done, whose
    C00000000.INIT_WITH_CUSTOM_DATA then holds the same cells.  On entry leftover *.tmp files are removed; bands whose state
    says done and whose last row is on disk are skipped, their candidates, bounds and statistics taken from the state, so that
    the next band starts from the bound the uninterrupted chain would have used; the first band that is not done reads its
    inbound column from the file of the band on its left.  A chain that tracks nothing (track_best=False: the global and the
    edge forms) restarts that band at row r, the largest special row complete on disk that the durable part of its outbound
    column has reached (the last band: the largest complete one; none: row 0) -- BandRunner.run(row0=r); rows [0, r] of every
    file stay, what lies below is written again.  A chain that TRACKS A BEST CELL (a local one) restarts the band at row 0:
    the stream hands out exact best cells at streamEnd only, a best seen in the rows above r could not be located -- the gap
    that remains.  So does the last band of a chain that may end on the last column (its edge cells above r would be lost).
    If the engine drops the pruning request of a partition that starts at r, the rest runs unpruned, the band's record says
    "pruned_after_resume": False and the result is the same.
    Refused before anything runs: a state whose key differs from this call's (ValueError naming the field), a state of
    another format version (ValueError), a band directory with special rows and no state (RuntimeError).  An empty work
    directory is a fresh run.  The return value gains "resumed": {"bands_skipped", "band", "from_row"} (None for a fresh
    run), "already_done" (every band was done: no stream is begun), and per band "skipped", "state_writes", "column_writes".
    progress(event, band, row): called at "band_begin", at "special_row" once the row and the state naming it are on disk, at
    "column" once a segment of the outbound column and the state counting it are, and at "band_end"; an exception out of it
    (or out of a sink) ends the run with the stream closed -- what a test interrupts a chain with.
    band_stage1 over ranks has no resume: a coordinated restart of several processes is another piece of work."""
    N = len(limits) - 1
    if N < 1 or any(limits[k] >= limits[k + 1] for k in range(N)) or limits[0] != 0:
        raise ValueError("serial_band_stage1: limits %r are no chain of bands" % (list(limits),))
    n_total = limits[-1] if n_total is None else n_total
    link = _SerialLink() if N > 1 else None
    prune_end = run_kw.get("prune_end", 0)
    works = [os.path.join(work, "FORK.%02d" % k) if N > 1 else work for k in range(N)]
    key, states, k_first = None, [None] * N, 0
    if resume:
        key, states, k_first = _left_by_earlier_runs(works, m, limits, n_total, sra_limit, origin, extent, recurrence,
                                                     first_row_init_type, first_col_init_type, prune_blocks, prune_end,
                                                     run_kw.get("track_best", True))
    midband = not run_kw.get("track_best", True)          # a chain that tracks a best cell restarts its band at row 0
    resumed = None
    if resume and any(s is not None for s in states):
        resumed = {"bands_skipped": k_first, "band": k_first if k_first < N else None, "from_row": 0}
    bands, cands, bound, first_bound = [], [], None, None
    from_row_before = 0
    for k in range(N):
        bwork = works[k]
        if resume and k < k_first:                        # done in an earlier run: its record stands in for it
            st = states[k]
            mine, own_bound = tuple(int(x) for x in st["best"]), st["initial_bound"]
            rec = {"best": mine, "work": bwork, "special_rows": list(st["special_rows"]), "seconds": st["seconds"],
                   "pruned_cells": int(st["pruned_cells"]), "initial_bound": own_bound, "restarts": int(st["restarts"]),
                   "skipped": True}
        else:
            runner = BandRunner(engine, dist=link, rank=k, world=N, segment_rows=segment_rows, prune_blocks=prune_blocks,
                                transport="host", seed_bound=seed_bound)
            keeper = None
            if resume:
                inbound = None
                # (the band on the left ran in an earlier process, or in this one from a row below 0: its column is its file)
                if k > 0 and (k == k_first or from_row_before):
                    inbound = np.fromfile(_inbound_file(works, k, m), dtype=np.int32, count=2 * (m + 1)).reshape(-1, 2)
                # (the last band of a chain that may end on the last column starts over: its edge cells above the row are gone)
                keeper = _BandResume(k, N, bwork, key, m, states[k], midband and k == k_first and not (k == N - 1 and prune_end & 2),
                                     inbound, link, segment_rows, _corner_cell(first_row_init_type, limits[k + 1]), progress)
                keeper.runner, keeper.bound = runner, bound
                os.makedirs(bwork, exist_ok=True)
                if progress is not None:
                    progress("band_begin", k, 0)
            if k > 0 and (keeper is None or keeper.inbound is None):
                link.raise_bound(bound)
            t0 = time.time()
            try:
                band_best, _part, rows = _band_area(runner, m, limits[k], limits[k + 1], bwork, sra_limit, n_total, recurrence,
                                                    first_row_init_type, first_col_init_type, origin, run_kw, extent, keeper)
            finally:
                if keeper is not None:
                    keeper.close()
            mine = runner.edge_best if prune_end else band_best
            mine = tuple(int(x) for x in mine) if mine is not None else (-1, -1, -INF)
            own_bound = runner.initial_bound
            st = engine.getStatistics() if hasattr(engine, "getStatistics") else {}
            rec = {"best": mine, "work": bwork, "special_rows": rows, "seconds": time.time() - t0,
                   "pruned_cells": int(st.get("pruned_cells", 0)), "initial_bound": own_bound, "restarts": runner.restarts}
            if keeper is not None:
                rec.update(skipped=False, state_writes=keeper.state_writes + 1, column_writes=keeper.column_writes)
                from_row_before = keeper.row0
                if keeper.row0:
                    resumed["from_row"] = keeper.row0
                    if runner.prune_blocks and not run_kw.get("track_best", True):
                        rec["pruned_after_resume"] = _kernel_prunes(st.get("kernel"))
        cands.append(mine)
        if k == 0:
            first_bound = own_bound
        if own_bound is not None:
            bound = own_bound if bound is None else max(bound, own_bound)
        # a score some alignment of the asked form reaches: a local best; a last-row cell of a chain that may end on the last row
        if (recurrence == SMITH_WATERMAN or (prune_end & 1 and k < N - 1)) and mine[2] > -INF:
            bound = mine[2] if bound is None else max(bound, mine[2])
        if resume and not rec["skipped"]:
            keeper.finish({"best": list(mine), "initial_bound": own_bound, "bound_after": bound, "first_bound": first_bound,
                           "special_rows": [int(x) for x in rows], "pruned_cells": rec["pruned_cells"],
                           "restarts": int(rec["restarts"]), "seconds": rec["seconds"]})
            if k > 0 and os.path.exists(os.path.join(works[k - 1], CHAIN_COLUMN)):
                os.remove(os.path.join(works[k - 1], CHAIN_COLUMN))      # this band's tee'd first column holds the same cells
            if progress is not None:
                progress("band_end", k, m)
        bands.append(rec)
    best = canonical_best(cands)
    if prune_blocks:
        check_chain_bound(best[2], first_bound)
    for b in bands:
        out = _write_chain_best(b["work"], best, origin)
    ret = {"best": tuple(out), "bands": bands, "limits": list(limits)}
    if resume:
        ret["resumed"] = resumed
        ret["already_done"] = k_first >= N
    return ret


def band_traceback(runner, seq0, seq1, work, limits, **kw):
    """Stages 2-6 over the chain band_stage1 left, collective over the runner's ranks: band_traceback.traceback_ranks."""
    from . import band_traceback as bt
    return bt.traceback_ranks(runner, seq0, seq1, work, limits, **kw)
