"""The traceback through a chain of column bands: stages 2-6 for a matrix whose stage 1 ran band by band
(bands.band_stage1 on the ranks of a chain, bands.serial_band_stage1 on one engine), each band with its own Special Rows
Area in `<work>/FORK.NN` -- MASA-Core's executeTracebackPipelined (M/libmasa/libmasa.cpp:659-696).

The band that holds the alignment's end walks stage 2 back through its own columns; where the walk reaches the band's first
column -- matched against the boundary column stage 1 kept there (C00000000.INIT_WITH_CUSTOM_DATA) -- the crosspoint goes
to the band on the left, which starts its own stage 2 from it (wait_crosspoint / send_crosspoint: stage2_pool_wait and
stage2_pool_send, M/stage2/sw_stage2.cpp:133-235).  Every band that took part refines its piece with stage 3 and with stage 4
down to partitions of 1024, the lists are joined from right to left (join: stage4_pool_wait, M/stage4/sw_stage4.cpp:854-881),
and the band that holds the alignment's start -- the keeper -- finishes: the joined list is `<work>/crosspoints/
crosspoint_03.00`, stage 4 goes down to max_partition_size, stages 5 and 6 leave crosspoint_04.00, alignment.00.bin and
alignment.00.txt in `<work>`.  All coordinates are absolute, as in pipeline._traceback.

Every step is a plain function of one band's work directory, its columns (j0, j1] and an aligner; traceback_serial (one
process, band after band from the right) and traceback_ranks (one rank per band, objects over torch.distributed) call the
same ones.  The extra crosspoints on the band boundaries move stage 4's split points, so among equally good alignments the
chain may pick another one than a single partition does; with ONE band there is no boundary and pipeline.align's own path runs.

Not carried over a chain: several alignments (--max-alignments), and a global alignment that runs along the first row into a
band that is not the first (stage 2's jump to the origin takes the band's own corner there)."""
import os
import time

import numpy as np

from .manager import AT_ANYWHERE, GAP_OPEN
from .crosspoints import Crosspoint, CrosspointsFile, crosspoint_file, TYPE_MATCH
from .stage2 import stage2
from .stage3 import stage3
from . import sra as sra_mod

BAND_PARTITION_SIZE = 1024          # libmasa.cpp:676-680: what a band's own stage 4 refines to before the lists are joined


class ChainFailed(RuntimeError):
    """another band of the chain failed; the text says which"""


def band_work(work, k, count):
    """Job::initializeWorkPath (M/common/Job.cpp:118-128): band k's own work directory"""
    return os.path.join(work, "FORK.%02d" % k) if count > 1 else work


def check_chain(work, limits, rows, max_alignments=1):
    """what a chain cannot do is refused before anything runs: several alignments; FORK.NN areas of stage 1 that are not
    exactly the bands `limits` names (rows = (i0, i1) of the matrix)"""
    if max_alignments != 1:
        raise ValueError("max_alignments=%d: a chain of bands traces one alignment back" % max_alignments)
    count = len(limits) - 1
    if count < 1 or any(limits[k] >= limits[k + 1] for k in range(count)):
        raise ValueError("limits %r are no chain of bands" % (list(limits),))
    if count == 1:
        return
    forks = sorted(d for d in (os.listdir(work) if os.path.isdir(work) else []) if d.startswith("FORK."))
    want = ["FORK.%02d" % k for k in range(count)]
    if forks != want:
        raise ValueError("%s holds the band directories %r, the chain %r needs exactly %r" % (work, forks, list(limits), want))
    for k in range(count):
        area = os.path.join(work, want[k], "special_rows", "stage.01.00")
        name = "%08X.%08X.%08X.%08X" % (rows[0], limits[k], rows[1], limits[k + 1])
        have = sorted(os.listdir(area)) if os.path.isdir(area) else []
        if have != [name]:
            raise ValueError("%s: stage 1 left the partitions %r, band %d of the chain %r is %s -- the areas do not tile the chain"
                             % (area, have, k, list(limits), name))


def wait_crosspoint(bwork, j0, j1, received=None):
    """stage2_pool_wait (sw_stage2.cpp:133-215).  received: the crosspoint (type, i, j, score) the band on the right handed
    over, None for the right-most band, which starts from the chain's best in its own crosspoint_01.00.  Returns (mine,
    crosspoint): a crosspoint left of column j0 or right of j1 is not this band's (:197-204) -- it goes on to the left
    untouched and the band does nothing; otherwise it is the band's crosspoint_01.00 from now on."""
    fn = crosspoint_file(bwork, 1, 0)
    if received is None:
        cps = CrosspointsFile(fn).load()
        if not cps:
            raise RuntimeError("band traceback: no crosspoint_01.00 in %s" % bwork)
        c = cps[0].astuple()
    else:
        c = tuple(int(x) for x in received)
    if c[2] < j0 or c[2] > j1:
        return False, c
    sra_mod.write_crosspoint(fn, (c[1], c[2], c[3]), typ=c[0])
    return True, c


def send_crosspoint(end, j0, first):
    """stage2_pool_send (sw_stage2.cpp:217-235).  end: where the band's stage 2 stopped, (type, i, j, score) as stage2()
    returns it -- a gap crosspoint's score already opened for the next sweep, which is taken back here (:222-234).  Returns
    the crosspoint for the band on the left, or None: only a crosspoint on the band's first column goes on."""
    t, i, j, s = (int(x) for x in end)
    if t != TYPE_MATCH:
        s -= GAP_OPEN
    return (t, i, j, s) if (not first and j == j0) else None


def band_stage2(aligner, d0, d1, bwork, j0, j1, rows, alignment_start=AT_ANYWHERE, sra_limit=0, areas=None, prune_goal=False):
    """stage 2 through this band's columns, from its crosspoint_01.00"""
    return stage2(aligner, d0, d1, bwork, alignment_start=alignment_start, sra_limit=sra_limit,
                             bounds=(rows[0], j0, rows[1], j1), areas=areas, prune_goal=prune_goal)


def band_refine(aligner, d0, d1, bwork, sra_limit=0, max_partition_size=16, areas=None):
    """stage 3, then stage 4 down to max(1024, max_partition_size) (libmasa.cpp:676-680) on the band's own piece; the list is
    the band's crosspoint_04.00.  Returns (stage 3's record, the list as an (N, 4) array of (type, i, j, score), seconds of
    stage 3 and of stage 4)."""
    t = time.time()
    r3 = stage3(aligner, d0, d1, bwork, sra_limit=sra_limit, areas=areas)
    t3 = time.time() - t
    t = time.time()
    pts = r3["crosspoints"]
    if len(pts) > 1:
        aligner.setSequences(d0, d1)
        try:
            pts, _ = aligner.stage4(pts, max(BAND_PARTITION_SIZE, max_partition_size))
        finally:
            aligner.unsetSequences()
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 4)
    _save(crosspoint_file(bwork, 4, 0), pts)
    return r3, pts, (t3, time.time() - t)


def _save(fn, pts):
    f = CrosspointsFile(fn)
    f.extend(Crosspoint(int(i), int(j), int(s), int(t)) for t, i, j, s in pts)
    f.save()


def join(own, received, j0, j1, first, last):
    """stage4_pool_wait (sw_stage4.cpp:854-881).  own: the band's list, from the alignment's start (or the band's first column)
    to its end (or the band's last column); received: the list of the band on its right or None.  A list that touches the
    right boundary drops its last point -- the received list begins with the same cell -- and takes the received list on;
    one that touches the left boundary goes on to the left.  Returns (list, goes on to the left)."""
    if not last and len(own) and own[-1][2] >= j1:
        if received is None:
            raise RuntimeError("band (%d, %d]: its list ends on the boundary and nothing came from the right" % (j0, j1))
        own = np.concatenate([own[:-1], np.asarray(received, dtype=np.int64).reshape(-1, 4)])
    return own, bool(not first and own[0][2] <= j0)


def keep(aligner, seq0, seq1, d0, d1, work, joined, max_partition_size, secs):
    """the keeper's part: the joined list is <work>/crosspoints/crosspoint_03.00, then stage 4 down to max_partition_size
    over the whole sequences, stages 5 and 6 (pipeline._finish)"""
    from . import pipeline
    _save(crosspoint_file(work, 3, 0), joined)
    return pipeline._finish(aligner, seq0, seq1, d0, d1, work, 0, [tuple(int(x) for x in p) for p in joined],
                            max_partition_size, secs)


def _data(seq0, seq1):
    d0, d1 = np.ascontiguousarray(seq0.data()), np.ascontiguousarray(seq1.data())
    return d0, d1, (seq0.offset0 - 1, seq0.offset1)


def _band_record(k, role):
    return {"band": k, "role": role, "crosspoints": {}, "seconds": {}}


@sra_mod.with_async_files
def traceback_serial(aligner, seq0, seq1, work, limits, alignment_start=AT_ANYWHERE, sra_limit=0, max_partition_size=16,
                     prune_traceback=False, max_alignments=1, secs=None):
    """One process, one aligner: the bands from the right, each through wait_crosspoint, stage 2, send_crosspoint, stage 3 and
    stage 4; then the lists joined from the right and the keeper's finish.  limits: absolute columns, band k = (limits[k],
    limits[k+1]].  Returns pipeline.align's traceback record (alignment, text, crosspoints per stage, stage4) plus "keeper"
    and "bands": per band its role ("band", "forward": passed the crosspoint on, "idle": nothing reached it), crosspoint
    counts and seconds per stage."""
    d0, d1, rows = _data(seq0, seq1)
    check_chain(work, limits, rows, max_alignments)
    secs = {} if secs is None else secs
    count = len(limits) - 1
    received, lists, bands = None, {}, [None] * count
    for k in reversed(range(count)):
        j0, j1, bwork = limits[k], limits[k + 1], band_work(work, k, count)
        if k < count - 1 and received is None:
            bands[k] = _band_record(k, "idle")
            continue
        mine, c = wait_crosspoint(bwork, j0, j1, received)
        if not mine:
            received, bands[k] = c, _band_record(k, "forward")
            continue
        rec = bands[k] = _band_record(k, "band")
        areas = {}
        t = time.time()
        r2 = band_stage2(aligner, d0, d1, bwork, j0, j1, rows, alignment_start, sra_limit, areas, prune_traceback)
        rec["seconds"][2] = time.time() - t
        received = send_crosspoint(r2["end"], j0, k == 0)
        r3, lists[k], (rec["seconds"][3], rec["seconds"][4]) = band_refine(aligner, d0, d1, bwork, sra_limit, max_partition_size, areas)
        rec["crosspoints"] = {2: len(r2["crosspoints"]), 3: len(r3["crosspoints"]), 4: len(lists[k])}
        rec["stage2"], rec["stage3"] = r2, r3
    joined, keeper = None, None
    for k in reversed(range(count)):
        if k not in lists:
            continue
        joined, on = join(lists[k], joined, limits[k], limits[k + 1], k == 0, k == count - 1)
        if not on:
            keeper = k
            break
    if keeper is None:
        raise RuntimeError("band traceback: no band holds the alignment's start")
    for st in (2, 3, 4):
        secs[st] = secs.get(st, 0.0) + sum(b["seconds"].get(st, 0.0) for b in bands)
    out = keep(aligner, seq0, seq1, d0, d1, work, joined, max_partition_size, secs)
    out["crosspoints"].update({2: sum(b["crosspoints"].get(2, 0) for b in bands), 3: len(joined)})
    out.update(keeper=keeper, bands=bands)
    return out


def _send(dist, obj, dst):
    dist.send_object_list([obj], dst=dst)


def _recv(dist, src):
    box = [None]
    dist.recv_object_list(box, src=src)
    return box[0]


@sra_mod.with_async_files
def traceback_ranks(runner, seq0, seq1, work, limits, alignment_start=AT_ANYWHERE, sra_limit=0, max_partition_size=16,
                    prune_traceback=False, max_alignments=1):
    """The same over the ranks of a BandRunner chain (rank k = band k, `work` shared), after band_stage1: crosspoints and lists
    travel as objects (send_object_list / recv_object_list).  A rank starts its stage 3 as soon as its crosspoint has gone to the
    left, so the bands refine side by side -- the reference's pipelining.
    Every rank makes the same four exchanges with its neighbours whatever happens to it: the crosspoint and then the list to the
    left, the keeper's rank to the right, the chain's state to the left again.  A rank that fails goes on answering -- with a
    failure marker that travels in both directions -- and raises once nobody waits for it any more; the others raise ChainFailed.
    Returns the record of traceback_serial's band on every rank (role, counts, seconds), with "keeper": the keeper's rank, and on
    the keeper the alignment's record as well."""
    dist, k, count, aligner = runner.dist, runner.rank, runner.world, runner.engine
    first, last = k == 0, k == count - 1
    j0, j1, bwork = limits[k], limits[k + 1], band_work(work, k, count)
    rec, err, own, areas, secs = _band_record(k, "idle"), None, None, {}, {}

    def fail(e):
        return ("fail", "band %d: %s: %s" % (k, type(e).__name__, e))

    # 1. the crosspoint, to the left
    msg = ("cp", None) if last else _recv(dist, k + 1)
    out = ("cp", None)
    try:
        if msg[0] == "fail":
            raise ChainFailed(msg[1])
        d0, d1, rows = _data(seq0, seq1)
        check_chain(work, limits, rows, max_alignments)
        if last or msg[1] is not None:
            mine, c = wait_crosspoint(bwork, j0, j1, msg[1])
            if not mine:
                out, rec["role"] = ("cp", c), "forward"
            else:
                rec["role"] = "band"
                t = time.time()
                r2 = band_stage2(aligner, d0, d1, bwork, j0, j1, rows, alignment_start, sra_limit, areas, prune_traceback)
                rec["seconds"][2] = time.time() - t
                rec["crosspoints"][2] = len(r2["crosspoints"])
                out = ("cp", send_crosspoint(r2["end"], j0, first))
    except BaseException as e:
        err, out = e, (msg if msg[0] == "fail" else fail(e))
    if not first:
        _send(dist, out, k - 1)
    # ... and this band's own refinement, while the bands on the left walk their stage 2
    if err is None and rec["role"] == "band":
        try:
            r3, own, (rec["seconds"][3], rec["seconds"][4]) = band_refine(aligner, d0, d1, bwork, sra_limit, max_partition_size, areas)
            rec["crosspoints"].update({3: len(r3["crosspoints"]), 4: len(own)})
        except BaseException as e:
            err = e
    # 2. the list, to the left; with it what is known of the keeper
    msg = ("list", None, None) if last else _recv(dist, k + 1)
    out, keeper, final = ("list", None, None), None, None
    try:
        if err is not None:
            raise err
        if msg[0] == "fail":
            raise ChainFailed(msg[1])
        keeper = msg[2]
        if rec["role"] == "band":
            joined, on = join(own, msg[1], j0, j1, first, last)
            if on:
                out = ("list", joined, None)
            else:
                keeper, final = k, joined
        if out[1] is None:
            out = ("list", None, keeper)
        if first and keeper is None:
            raise RuntimeError("band traceback: no band holds the alignment's start")
    except BaseException as e:
        if err is None:
            err = e
        out = msg if msg[0] == "fail" else fail(err)
    if not first:
        _send(dist, out, k - 1)
    if err is None and final is not None:           # the keeper finishes; nobody on its left has anything more to do
        try:
            done = keep(aligner, seq0, seq1, d0, d1, work, final, max_partition_size, secs)
            counts = dict(rec["crosspoints"])
            counts.update({3: len(final), 4: done["crosspoints"][4]})
            rec.update(done)
            rec["crosspoints"] = counts
            rec["seconds"].update({st: rec["seconds"].get(st, 0.0) + s for st, s in secs.items()})
        except BaseException as e:
            err = e
    # 3. the keeper's rank, to the right  4. the chain's state, to the left
    msg = None if first else _recv(dist, k - 1)
    if err is not None:
        out = fail(err) if not isinstance(err, ChainFailed) else ("fail", str(err))
    elif first:
        out = ("ok", keeper)
    else:
        out = msg
    if not last:
        _send(dist, out, k + 1)
        back = _recv(dist, k + 1)
    else:
        back = out
    if not first:
        _send(dist, back if err is None else out, k - 1)
    if err is not None:
        raise err
    if back[0] == "fail":
        raise ChainFailed(back[1])
    rec["keeper"] = back[1]
    return rec
