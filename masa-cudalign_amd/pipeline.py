"""The whole pipeline natively: stage 1 (score + special rows), stage 2 (crosspoints on stage 1's special rows),
stage 3 (crosspoints on the rows stages 2 and 3 save), stage 4 (Myers-Miller refinement down to 16 x 16, on the GPU:
mi355sw_stage4), stage 5 (exact alignment of the small partitions), stage 6 (text) -- what MASA-Core's
executeTraceback() runs after stage 1 (M/libmasa/libmasa.cpp:643-657), with the work directory in MASA-Core's layout:

    <work>/crosspoints/crosspoint_01.00 .. crosspoint_04.00 (+ crosspoint_03.00.rNN per round of stage 3)
    <work>/special_rows/stage.01.00, stage.02.00, stage.03.00.rNN
    <work>/info, <work>/status, <work>/alignment.00.bin (alignment_file.py), <work>/alignment.00.txt

The aligner is an MI355Aligner (or anything with its setSequences / alignPartition / matchLastColumn / stage4 /
unsetSequences); every DP cell of every stage is computed by it.  The sequence modifiers of fasta.py (--trim,
--reverse, --complement, --clear-n) are carried through all stages as in MASA-Core."""
import os
import time

import numpy as np

from .manager import AT_ANYWHERE
from .engine import INF
from .crosspoints import Crosspoint, CrosspointsFile, crosspoint_file, save_array
from .stage1 import stage1
from .stage2 import stage2
from .stage3 import stage3
from . import stage56, alignment_file
from . import sra as sra_mod


class WorkDirectoryMismatch(RuntimeError):
    """MASA-Core prints "Sequence mismatch from previous run. Try cleaning work directory (--clean)" and stops"""


def check_work_directory(work, seq0, seq1):
    """Job::initialize (M/common/Job.cpp:68-90): `<work>/info` names the two sequences a work directory belongs to
    ("seq0=<description>", "seq1=<description>"); a run that finds other names there must not continue from its
    special rows, status and crosspoints"""
    os.makedirs(work, exist_ok=True)
    fn = os.path.join(work, "info")
    if os.path.exists(fn):
        prop = {}
        for line in open(fn, encoding="latin-1"):
            line = line[:-1]
            pos = line.find("=")
            if pos > 0:
                prop[line[:pos]] = line[pos + 1:]
        bad = [(k, prop.get(k, ""), s.description) for k, s in (("seq0", seq0), ("seq1", seq1)) if prop.get(k, "") != s.description]
        if bad:
            raise WorkDirectoryMismatch("sequence mismatch from a previous run in %s (clean the work directory): %s"
                                        % (work, "; ".join("%s: %r != %r" % b for b in bad)))
    else:
        with open(fn, "w", encoding="latin-1") as f:
            f.write("seq0=%s\nseq1=%s\n" % (seq0.description, seq1.description))


@sra_mod.with_async_files
def align(aligner, seq0, seq1, work, alignment_start=AT_ANYWHERE, alignment_end=AT_ANYWHERE, sra_limit=0,
          block_pruning=True, max_partition_size=16, progress=None, max_alignments=1, ram_limit=0, prune_global=False,
          prune_traceback=False, prune_edges=False):
    """seq0, seq1: fasta.Sequence.  Returns {"best", "alignment": stage56.Alignment or None, "text": bytes of
    alignment.00.txt or None when nothing scored above the floor, "crosspoints": {2: n, 3: n, 4: n},
    "seconds": {stage: s}}; with max_alignments > 1 also "alignments": one such record per end point stage 1 kept
    (alignment.NN.txt, crosspoint_0S.NN, special_rows/stage.0S.NN: executeTraceback, libmasa.cpp:643-657).
    prune_traceback: stage 2's sweeps skip what cannot meet their goal (stage2(prune_goal=True)); the same files but
    special_rows/stage.02.NN, whose cells off every goal path may be lower bounds
    prune_edges: stage 1 of an alignment that ends on a sequence edge prunes too (stage1(prune_edges=True)); the same files but
    special_rows/stage.01.NN, whose cells off every optimal path may be lower bounds"""
    check_work_directory(work, seq0, seq1)
    # the data the aligner compares: forward or reversed, complemented, N-cleared (fasta.py); --trim only selects the
    # part of the matrix stage 1 sweeps, every coordinate of every stage stays absolute (Sequence.cpp:117-159)
    d0, d1 = np.ascontiguousarray(seq0.data()), np.ascontiguousarray(seq1.data())
    bounds = (seq0.offset0 - 1, seq1.offset0 - 1, seq0.offset1, seq1.offset1)
    secs = {}
    areas = {}                     # Job's cache of special-rows areas: rows kept in memory live here between the stages
    t = time.time()
    r1 = stage1(aligner, d0, d1, work, alignment_start=alignment_start, alignment_end=alignment_end, sra_limit=sra_limit,
                block_pruning=block_pruning, bounds=bounds, progress=progress, max_alignments=max_alignments,
                ram_limit=ram_limit, areas=areas, prune_global=prune_global, prune_edges=prune_edges)
    secs[1] = time.time() - t
    out = {"best": r1["best"], "alignment": None, "text": None, "crosspoints": {}, "seconds": secs, "stage1": r1,
           "alignments": []}
    if r1["best"] is None or r1["best"][2] <= -INF or r1["best"][0] < 0:
        return out                                        # an empty best-score list: MASA-Core runs no traceback either
    for ident in range(max(len(r1.get("bests", [])), 1)):
        rec = _traceback(aligner, seq0, seq1, d0, d1, work, ident, alignment_start, sra_limit, max_partition_size, bounds, secs,
                         ram_limit, areas, prune_traceback)
        out["alignments"].append(rec)
    out.update(out["alignments"][0])
    return out


def _traceback(aligner, seq0, seq1, d0, d1, work, ident, alignment_start, sra_limit, max_partition_size, bounds, secs,
               ram_limit=0, areas=None, prune_traceback=False):
    """stages 2-6 for the alignment that ends in crosspoint_01.<ident>"""
    def clock(stage, t0):
        secs[stage] = secs.get(stage, 0.0) + time.time() - t0
    t = time.time()
    r2 = stage2(aligner, d0, d1, work, alignment_start=alignment_start, sra_limit=sra_limit, ident=ident, bounds=bounds,
                ram_limit=ram_limit, areas=areas, prune_goal=prune_traceback)
    clock(2, t)
    t = time.time()
    r3 = stage3(aligner, d0, d1, work, sra_limit=sra_limit, ident=ident, ram_limit=ram_limit, areas=areas)
    clock(3, t)
    rec = _finish(aligner, seq0, seq1, d0, d1, work, ident, r3["crosspoints"], max_partition_size, secs)
    rec["crosspoints"].update({2: len(r2["crosspoints"]), 3: len(r3["crosspoints"])})
    rec.update(stage2=r2, stage3=r3)
    return rec


def _finish(aligner, seq0, seq1, d0, d1, work, ident, crosspoints3, max_partition_size, secs):
    """stages 4-6 from a list of stage 3: crosspoint_04.NN, alignment.NN.bin, alignment.NN.txt in `work`"""
    def clock(stage, t0):
        secs[stage] = secs.get(stage, 0.0) + time.time() - t0
    t = time.time()
    aligner.setSequences(d0, d1)
    try:
        try:
            cp4, st4 = aligner.stage4(crosspoints3, max_partition_size, as_array=True)
        except TypeError:              # an aligner double without the array form
            cp4, st4 = aligner.stage4(crosspoints3, max_partition_size)
    finally:
        aligner.unsetSequences()
    # crosspoint_04: millions of points at sizes like C3 (130 MB of text, seconds of formatting).  Nothing in this run reads the
    # file back -- stage 5 takes the array -- so it is written by the areas' file thread while stages 5 and 6 run in the library
    # (their calls release the interpreter); in place when align() returns, like every queued file (sra.async_files)
    if isinstance(cp4, np.ndarray):
        sra_mod.queue_file_operation(_finish, save_array, crosspoint_file(work, 4, ident), cp4)
    else:
        save_array(crosspoint_file(work, 4, ident), cp4)
    clock(4, t)
    t = time.time()
    al = stage56.stage5(seq0, seq1, cp4)
    clock(5, t)
    t = time.time()
    with open(os.path.join(work, "alignment.%02d.bin" % ident), "wb") as f:   # what stage 5 leaves for stage 6 and the viewers
        f.write(alignment_file.dumps(al, seq0, seq1))
    text = stage56.stage6_text(al, seq0, seq1)
    with open(os.path.join(work, "alignment.%02d.txt" % ident), "wb") as f:
        f.write(text)
    clock(6, t)
    return dict(alignment=al, text=text, crosspoints={4: len(cp4)}, stage4=st4)


def chain_form(alignment_start, alignment_end):
    """the stage-1 set-up of a chain of bands for the alignment's edges (sw_stage1.cpp:137-161, :318-322, BandRunner.run):
    keywords of bands.serial_band_stage1 / band_stage1"""
    from .manager import AT_SEQUENCE_1, AT_SEQUENCE_2, AT_SEQUENCE_1_OR_2, AT_SEQUENCE_1_AND_2
    from .engine import SMITH_WATERMAN, NEEDLEMAN_WUNSCH, INIT_WITH_ZEROES, INIT_WITH_GAPS
    if alignment_start == AT_ANYWHERE:
        if alignment_end != AT_ANYWHERE:
            raise ValueError("a chain of bands runs a local start (*) with a local end (*) only")
        return dict(recurrence=SMITH_WATERMAN, first_row_init_type=INIT_WITH_ZEROES, first_col_init_type=INIT_WITH_ZEROES)
    Z, G = INIT_WITH_ZEROES, INIT_WITH_GAPS
    rows = {AT_SEQUENCE_1: (Z, G), AT_SEQUENCE_2: (G, Z), AT_SEQUENCE_1_OR_2: (Z, Z), AT_SEQUENCE_1_AND_2: (G, G)}
    ends = {AT_SEQUENCE_1: 1, AT_SEQUENCE_2: 2, AT_SEQUENCE_1_OR_2: 3, AT_SEQUENCE_1_AND_2: 0}
    if alignment_start not in rows or alignment_end not in ends:
        raise ValueError("a chain of bands cannot start at %r and end at %r" % (alignment_start, alignment_end))
    return dict(recurrence=NEEDLEMAN_WUNSCH, first_row_init_type=rows[alignment_start][0], first_col_init_type=rows[alignment_start][1],
                track_best=False, prune_end=ends[alignment_end])


@sra_mod.with_async_files
def align_bands(aligner, seq0, seq1, work, weights, alignment_start=AT_ANYWHERE, alignment_end=AT_ANYWHERE, sra_limit=0,
                block_pruning=True, max_partition_size=16, progress=None, max_alignments=1, ram_limit=0, prune_global=False,
                prune_traceback=False, prune_edges=False, resume=False, segment_rows=1 << 16):
    """align() with stage 1 taken in len(weights) column bands, one after the other on `aligner` (bands.serial_band_stage1:
    band k gets weights[k] / sum(weights) of the columns, its own Special Rows Area in `work`/FORK.NN and `sra_limit` of
    budget, like a --split node), and the alignment traced back through the chain (band_traceback.traceback_serial).  So one
    GPU aligns a matrix whose special rows it could not keep in one piece, and what the ranks of a chain leave is read the
    same way (bands.band_traceback).  Returns align()'s record plus "bands": per band its role, crosspoint counts and
    seconds per stage (stage 1 included), and "keeper".
    Block pruning applies where a band's stage 1 prunes: local alignments (block_pruning), global ones (prune_global),
    alignments that end on an edge (prune_edges).  ram_limit is not split over bands: rows are kept on disk.
    With ONE band this is align() itself: same path, same files.
    resume=True: stage 1 continues a chain that was killed from what it left in `work` (bands.serial_band_stage1(resume=True):
    bands that are done are skipped, the band that was interrupted restarts at its last durable special row where the chain
    tracks nothing, at row 0 where it tracks a best cell) and leaves one chain.mi355 per band; stages 2 to 6 run as always on
    what stage 1 left -- running them again costs seconds.  The record then carries "resumed" (serial_band_stage1's).  With one
    weight it is align(), which resumes by itself.  segment_rows: the rows per segment of the boundary column between two bands."""
    from . import bands as bands_mod
    from . import band_traceback as bt
    from .manager import AT_SEQUENCE_1_AND_2
    if max_alignments != 1:
        raise ValueError("max_alignments=%d: a chain of bands traces one alignment back" % max_alignments)
    weights = [int(w) for w in weights]
    if not weights or min(weights) <= 0:
        raise ValueError("weights %r: one positive weight per band" % (weights,))
    if len(weights) == 1:
        out = align(aligner, seq0, seq1, work, alignment_start=alignment_start, alignment_end=alignment_end, sra_limit=sra_limit,
                    block_pruning=block_pruning, max_partition_size=max_partition_size, progress=progress, ram_limit=ram_limit,
                    prune_global=prune_global, prune_traceback=prune_traceback, prune_edges=prune_edges)
        out["bands"] = [{"band": 0, "role": "band", "crosspoints": dict(out["crosspoints"]), "seconds": dict(out["seconds"])}]
        out["keeper"] = 0
        return out
    form = chain_form(alignment_start, alignment_end)
    check_work_directory(work, seq0, seq1)
    d0, d1 = np.ascontiguousarray(seq0.data()), np.ascontiguousarray(seq1.data())
    bi0, bj0, bi1, bj1 = seq0.offset0 - 1, seq1.offset0 - 1, seq0.offset1, seq1.offset1
    rel = bands_mod.band_limits(bj1 - bj0, weights)
    if any(rel[k] >= rel[k + 1] for k in range(len(weights))):
        raise ValueError("weights %r leave a band of %d columns empty" % (weights, bj1 - bj0))
    if alignment_start == AT_ANYWHERE:
        prune = bool(block_pruning)
    elif form["prune_end"]:
        prune = bool(block_pruning and prune_edges)
    else:
        prune = bool(block_pruning and prune_global and alignment_start == AT_SEQUENCE_1_AND_2)
    secs = {}
    t = time.time()
    aligner.setSequences(d0[bi0:bi1], d1[bj0:bj1])
    try:
        if resume:
            form = dict(form, resume=True)
        r1 = bands_mod.serial_band_stage1(aligner, bi1 - bi0, rel, work, sra_limit, prune_blocks=prune, origin=(bi0, bj0),
                                          extent=(len(d0), len(d1)), segment_rows=segment_rows, **form)
    finally:
        aligner.unsetSequences()
    secs[1] = time.time() - t
    out = {"best": r1["best"], "alignment": None, "text": None, "crosspoints": {}, "seconds": secs, "stage1": r1, "alignments": [],
           "bands": [{"band": k, "role": "idle", "crosspoints": {}, "seconds": {1: b["seconds"]}} for k, b in enumerate(r1["bands"])]}
    if resume:
        out["resumed"] = r1["resumed"]
    if r1["best"][2] <= -INF or r1["best"][0] < 0:
        return out
    limits = [bj0 + x for x in rel]
    rec = bt.traceback_serial(aligner, seq0, seq1, work, limits, alignment_start=alignment_start, sra_limit=sra_limit,
                              max_partition_size=max_partition_size, prune_traceback=prune_traceback, secs=secs)
    for b, b1 in zip(rec["bands"], r1["bands"]):
        b["seconds"][1] = b1["seconds"]
    out["alignments"].append(rec)
    out.update(rec)
    return out
