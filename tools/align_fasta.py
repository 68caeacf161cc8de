"""Two FASTA files in, alignment.00.txt out: the native pipeline (masa-cudalign_amd/pipeline.py, stages 1-6 on one
MI355X) behind the handful of MASA-CUDAlign options that concern the path -- not a re-build of its command line.

    python tools/align_fasta.py [options] seq0.fasta seq1.fasta
      --work-dir=DIR            work directory in MASA-Core's layout (default ./work.tmp); a killed stage 1 resumes from it
      --disk-size=N[KMG]        Special Rows Area budget on disk (default: 8192-row spacing, at most 4 GiB; the traceback needs special rows)
      --ram-size=N[KMG]         part of the special rows kept in memory instead (they alternate with the rows on disk)
      --trim=I0,I1,J0,J1  --reverse=1|2|both  --complement=1|2|both  --reverse-complement=1|2|both  --clear-n
      --alignment-edges=XY      X start, Y end: * anywhere (local), 1 / 2 on that sequence's edge, 3 on either, + on both (global)
      --max-alignments=N        trace back up to N different alignments (alignment.00.txt .. alignment.NN.txt)
      --no-block-pruning  --prune-global (block pruning for a global alignment too)  --gpu=ID  --stage-1 (best score only)
      --prune-traceback         stage 2's sweeps skip what cannot meet their goal (goal pruning; same alignment, off by default)
      --prune-edges             block pruning for an alignment that starts on a sequence edge and ends on the last row, the last
                                column or either (edges X1, X2, X3 with X not *; same alignment, off by default)
      --split=N | --split=W1,W2,...  stage 1 in N column bands of equal width (or of the given weights), one after the other on
                                the GPU, each with its own Special Rows Area of --disk-size in <work>/FORK.NN, and the alignment
                                traced back through the chain (pipeline.align_bands; one alignment, no --ram-size)
      --resume                  with --split: continue a chain that was killed from what it left in the work directory -- bands
                                that are done are skipped, the band that was interrupted restarts at its last durable special
                                row (a local chain: at its row 0); leaves one chain.mi355 per FORK.NN.  Without --split a killed
                                stage 1 resumes by itself
      --wide-alphabet           sequences with 15 to 62 letters in common (all IUPAC codes, ...) run on the packed kernels too
                                (MI355SW_F_WIDE_ALPHABET; same alignment, off by default)
      --int32-prune-global      with --prune-global: sequences that run on the int32 kernels (15 or more letters in common without
                                --wide-alphabet, 63 or more with it, overflow reruns) prune a global alignment too
                                (MI355SW_F_INT32_PRUNE_GLOBAL; same alignment, off by default)
      --int32-prune-edge-goal   with --prune-edges / --prune-traceback: sequences that run on the int32 kernels prune by the edge
                                rule and stage 2's goal bounds too (MI355SW_F_INT32_PRUNE_EDGE_GOAL; same alignment, off by default)
      --int32-window            sequences that run on the int32 kernels prune with the pruning window: strips below the end of the
                                alignment retire instead of walking the width (MI355SW_F_INT32_WINDOW; same alignment, off by default)

Prints one JSON line (best score, crosspoints per stage, seconds per stage) and leaves alignment.00.txt in the work
directory.  The engine has no CPU fallback: without an MI355X this fails with MI355SW_ENOGPU."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def _size(v):
    mult = {"K": 1024, "M": 1024 ** 2, "G": 1024 ** 3}.get(v[-1:].upper())
    return int(float(v[:-1]) * mult) if mult else int(float(v))


def _flags(v):
    return [v in ("1", "both"), v in ("2", "both")]


def main(argv):
    pkg = g.load_package()
    from masa_cudalign_amd import fasta, pipeline, stage1
    edge = {"*": pkg.AT_ANYWHERE, "1": pkg.AT_SEQUENCE_1, "2": pkg.AT_SEQUENCE_2, "3": pkg.AT_SEQUENCE_1_OR_2,
            "+": pkg.AT_SEQUENCE_1_AND_2}
    work, limit, device, prune, only1, edges, count, ram = "./work.tmp", None, 0, True, False, "**", 1, 0
    trim, rev, comp, clear_n = [0, 0, 0, 0], [False, False], [False, False], False
    prune_global = prune_traceback = wide_alphabet = prune_edges = int32_prune_global = int32_prune_edge_goal = int32_window = False
    weights = None
    resume = False
    files = []
    for a in argv:
        if a.startswith("--work-dir="):
            work = a[11:]
        elif a.startswith("--disk-size="):
            limit = _size(a[12:])
        elif a.startswith("--ram-size="):
            ram = _size(a[11:])
        elif a.startswith("--trim="):
            trim = [int(x) for x in a[7:].split(",")]
        elif a.startswith("--reverse="):
            rev = _flags(a[10:])
        elif a.startswith("--complement="):
            comp = _flags(a[13:])
        elif a.startswith("--reverse-complement="):
            rev = comp = _flags(a[21:])
        elif a == "--clear-n":
            clear_n = True
        elif a.startswith("--alignment-edges="):
            edges = a[18:]
        elif a.startswith("--max-alignments="):
            count = int(a[17:])
        elif a == "--no-block-pruning":
            prune = False
        elif a == "--prune-global":
            prune_global = True
        elif a == "--prune-traceback":
            prune_traceback = True
        elif a == "--prune-edges":
            prune_edges = True
        elif a == "--wide-alphabet":
            wide_alphabet = True
        elif a == "--int32-prune-global":
            int32_prune_global = True
        elif a == "--int32-prune-edge-goal":
            int32_prune_edge_goal = True
        elif a == "--int32-window":
            int32_window = True
        elif a.startswith("--split="):
            v = [int(x) for x in a[8:].split(",")]
            weights = [1] * v[0] if len(v) == 1 else v
        elif a == "--resume":
            resume = True
        elif a.startswith("--gpu="):
            device = int(a[6:])
        elif a == "--stage-1":
            only1 = True
        elif a.startswith("-"):
            raise SystemExit("unknown option %s\n\n%s" % (a, __doc__))
        else:
            files.append(a)
    if len(files) != 2 or len(edges) != 2 or edges[0] not in edge or edges[1] not in edge or len(trim) != 4:
        raise SystemExit(__doc__)
    seqs = [fasta.load(files[k], fasta.SequenceModifiers(clear_n=clear_n, reverse=rev[k], complement=comp[k],
                                                         trim_start=trim[2 * k], trim_end=trim[2 * k + 1])) for k in (0, 1)]
    if limit is None:
        limit = min((len(seqs[0]) // 8192 + 2) * (len(seqs[1]) + 1) * 8, 4 << 30)
    al = pkg.MI355Aligner(device=device, flags=(pkg.engine.F_WIDE_ALPHABET if wide_alphabet else 0) |
                          (pkg.engine.F_INT32_PRUNE_GLOBAL if int32_prune_global else 0) |
                          (pkg.engine.F_INT32_PRUNE_EDGE_GOAL if int32_prune_edge_goal else 0) |
                          (pkg.engine.F_INT32_WINDOW if int32_window else 0))
    try:
        if only1:
            bounds = (seqs[0].offset0 - 1, seqs[1].offset0 - 1, seqs[0].offset1, seqs[1].offset1)
            r = stage1.stage1(al, seqs[0].data(), seqs[1].data(), work, alignment_start=edge[edges[0]],
                              alignment_end=edge[edges[1]], sra_limit=limit, block_pruning=prune, bounds=bounds,
                              progress=sys.stderr, max_alignments=count, ram_limit=ram, prune_global=prune_global,
                              prune_edges=prune_edges)
            res = {"best": list(r["best"]), "seconds": {"1": r["seconds"]}, "gcups": r["gcups"]}
        elif weights is not None and len(weights) > 1:
            out = pipeline.align_bands(al, seqs[0], seqs[1], work, weights, alignment_start=edge[edges[0]], alignment_end=edge[edges[1]],
                                       sra_limit=limit, block_pruning=prune, max_alignments=count, prune_global=prune_global,
                                       prune_traceback=prune_traceback, prune_edges=prune_edges, **({"resume": True} if resume else {}))
            res = {"best": list(out["best"]), "seconds": {str(k): v for k, v in out["seconds"].items()},
                   "crosspoints": {str(k): v for k, v in out["crosspoints"].items()}, "keeper": out.get("keeper"),
                   **({"resumed": out.get("resumed")} if resume else {}),
                   "bands": [{"band": b["band"], "role": b["role"], "crosspoints": {str(k): v for k, v in b["crosspoints"].items()},
                              "seconds": {str(k): v for k, v in b["seconds"].items()}} for b in out["bands"]],
                   "alignments": [os.path.join(work, "alignment.00.txt")] if out["text"] is not None else []}
        else:
            out = pipeline.align(al, seqs[0], seqs[1], work, alignment_start=edge[edges[0]], alignment_end=edge[edges[1]],
                                 sra_limit=limit, block_pruning=prune, progress=sys.stderr, max_alignments=count, ram_limit=ram,
                                 prune_global=prune_global, prune_traceback=prune_traceback, prune_edges=prune_edges)
            res = {"best": list(out["best"]), "seconds": {str(k): v for k, v in out["seconds"].items()},
                   "crosspoints": {str(k): v for k, v in out["crosspoints"].items()},
                   "alignments": [os.path.join(work, "alignment.%02d.txt" % k) for k in range(len(out["alignments"]))]}
    finally:
        al.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
