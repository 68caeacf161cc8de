"""Stage 1 of one related pair as a semi-global alignment (edges XY, default 33), block pruning for edge ends off and on
(Stage1Manager(prune_edges=...), MI355Aligner.setPruneEnd), next to the same pair as a global alignment with prune_global --
`runs` times each, alternating, the score of every run held against the first.

    python tools/edge_prune_measure.py M N [edges] [runs] [out.json] [cfg] [--bands B]

--bands B: instead, the edge form on ONE partition with pruning on next to an in-process chain of B equal column bands on the same
GPU (bands.InProcessChain, prune_end = the form's end) with pruning on and off -- the chain shares the device among its bands
(1024 / B wavefronts each), so its seconds say what the chain costs and skips on one GPU, not what B GPUs would take.

The pair is tools/native_pipeline_run.py's (seqgen cfg 2).  Prints one JSON line per run and a summary line; out.json gets all."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def chain_runs(pkg, m, n, edges, runs, cfg, bands):
    """one partition with edge pruning on / the chain of `bands` bands with it on / the same chain with it off, alternating"""
    from masa_cudalign_amd.bands import InProcessChain, band_limits
    code = {"1": pkg.AT_SEQUENCE_1, "2": pkg.AT_SEQUENCE_2, "3": pkg.AT_SEQUENCE_1_OR_2, "+": pkg.AT_SEQUENCE_1_AND_2}
    start, end = code[edges[0]], code[edges[1]]
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=cfg)
    part = pkg.Partition(0, 0, m, n)
    form = pkg.Stage1Manager(part, alignment_start=start, alignment_end=end, block_pruning=True, prune_edges=True)     # borders and edge of the form
    row_t, col_t, mode = form.getFirstRowInitType(), form.getFirstColumnInitType(), form.pruneEnd()
    assert mode in (1, 2, 3), "edges %s: the alignment does not end on a sequence edge" % edges
    one = pkg.MI355Aligner(device=0)
    als = [pkg.MI355Aligner(device=0, waves=1024 // bands) for _ in range(bands)]
    limits = band_limits(n, [1] * bands)
    out, first = [], None
    try:
        for a in [one] + als:
            a.setSequences(s0, s1)
        for k in range(runs):
            for name in ("one partition on", "%d bands on" % bands, "%d bands off" % bands):
                t0 = time.time()
                if name.startswith("one"):
                    mg = pkg.Stage1Manager(part, alignment_start=start, alignment_end=end, block_pruning=True, prune_edges=True)
                    one.setPruneEnd(mg.pruneEnd())
                    one.alignPartition(part, mg)
                    dt = time.time() - t0
                    best = list(mg.getBestScore())
                    stats = [one.getStatistics()]
                    bound = None
                else:
                    chain = InProcessChain(als, prune_blocks=name.endswith("on"))
                    cell, stats = chain.run(m, limits, recurrence=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=row_t, first_col_init_type=col_t,
                                            prune_end=mode)
                    dt = time.time() - t0
                    best = [cell[0] + 1, cell[1] + 1, cell[2]]          # (the chain reports the 0-based cell, a manager DP coordinates)
                    bound = chain.initial_bound
                first = first or best
                assert best == first, (name, best, first)
                rec = {"run": name, "k": k, "best": best, "seconds": dt, "kernel_ms": [st["kernel_ms"] for st in stats], "seed_ms": stats[0]["seed_ms"],
                       "kernel": [st["kernel"] for st in stats], "strip_rows": [st["strip_rows"] for st in stats], "initial_bound": bound,
                       "pruned_fraction_per_band": [st["pruned_cells"] / float(st["cells"]) for st in stats],
                       "pruned_fraction": sum(st["pruned_cells"] for st in stats) / float(m) / n, "tcups": float(m) * n / dt / 1e12}
                out.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        for a in [one] + als:
            a.close()
    return out


def main():
    pkg = g.load_package()
    bands = 0
    if "--bands" in sys.argv:
        k = sys.argv.index("--bands")
        bands = int(sys.argv[k + 1])
        del sys.argv[k:k + 2]
    m, n = int(sys.argv[1]), int(sys.argv[2])
    edges = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else "33"
    runs = int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[4] != "-" else 3
    outfn = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
    cfg = int(sys.argv[6]) if len(sys.argv) > 6 else 2
    code = {"1": pkg.AT_SEQUENCE_1, "2": pkg.AT_SEQUENCE_2, "3": pkg.AT_SEQUENCE_1_OR_2, "+": pkg.AT_SEQUENCE_1_AND_2}
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=cfg)
    part = pkg.Partition(0, 0, m, n)
    if bands > 0:
        return summarise(pkg, m, n, cfg, chain_runs(pkg, m, n, edges, runs, cfg, bands), outfn,
                         note="the chain runs in one process on ONE GPU, its bands share the device: not a multi-GPU time")
    al = pkg.MI355Aligner(device=0)
    out, first = [], {}
    try:
        al.setSequences(s0, s1)
        for k in range(runs):
            for name, start, end, kw in ((edges + " off", code[edges[0]], code[edges[1]], dict(block_pruning=True)),
                                         (edges + " on", code[edges[0]], code[edges[1]], dict(block_pruning=True, prune_edges=True)),
                                         ("++ prune_global", code["+"], code["+"], dict(block_pruning=True, prune_global=True))):
                mg = pkg.Stage1Manager(part, alignment_start=start, alignment_end=end, **kw)
                if mg.pruneEnd():
                    al.setPruneEnd(mg.pruneEnd())
                t0 = time.time()
                al.alignPartition(part, mg)
                dt = time.time() - t0
                st = al.getStatistics()
                best = list(mg.getBestScore())
                if name.split()[0] not in first:
                    first[name.split()[0]] = best[2]
                assert best[2] == first[name.split()[0]], (name, best, first)
                rec = {"run": name, "k": k, "best": best, "seconds": dt, "kernel_ms": st["kernel_ms"], "seed_ms": st["seed_ms"], "kernel": st["kernel"],
                       "strip_rows": st["strip_rows"], "pruned_fraction": st["pruned_cells"] / float(m) / n, "tcups": float(m) * n / dt / 1e12}
                out.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        al.close()
    return summarise(pkg, m, n, cfg, out, outfn)


def summarise(pkg, m, n, cfg, out, outfn, note=None):
    summary = {"workload": "%d x %d related pair (seqgen cfg=%d), stage 1 only, no special rows" % (m, n, cfg), "build_id": pkg.engine.library_build_id(), "runs": out}
    if note:
        summary["note"] = note
    for name in sorted({r["run"] for r in out}):
        secs = sorted(r["seconds"] for r in out if r["run"] == name)
        summary[name] = {"seconds_median": secs[len(secs) // 2], "seconds_all": secs, "pruned_fraction": [r["pruned_fraction"] for r in out if r["run"] == name]}
    print(json.dumps({k: v for k, v in summary.items() if k != "runs"}))
    if outfn:
        with open(outfn, "w") as f:
            json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
