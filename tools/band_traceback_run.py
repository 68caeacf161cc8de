"""One pair, twice on one MI355X: pipeline.align (one partition) and pipeline.align_bands (stage 1 in B column bands one after
the other, the alignment traced back through the chain) -- seconds per stage, and for the chain per band as well.

    python tools/band_traceback_run.py M N [bands] [sra_bytes] [out.json] [cfg]

Related pair from seqgen (tools/native_pipeline_run.py's), local alignment, block pruning on.  Checks: both runs end on the same
best cell and score, and each alignment re-scores to it (stage 5 refuses anything else).  The two alignments may differ among
equally good ones (the crosspoints on the band boundaries move stage 4's split points); "same_text" records whether they do."""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
from masa_cudalign_amd import fasta, pipeline  # noqa: E402


def main():
    m, n = int(sys.argv[1]), int(sys.argv[2])
    bands = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3] != "-" else 4
    limit = int(float(sys.argv[4])) if len(sys.argv) > 4 and sys.argv[4] != "-" else min(max(200 * 1024, (m // 8192 + 1) * n * 8), 4 << 30)
    outfn = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
    cfg = int(sys.argv[6]) if len(sys.argv) > 6 else 2
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=cfg)
    q0 = fasta.Sequence(">s0", s0, fasta.SequenceModifiers())
    q1 = fasta.Sequence(">s1", s1, fasta.SequenceModifiers())
    res = {"workload": "%dx%d related pair (seqgen cfg=%d), local, stages 1-6 natively" % (m, n, cfg), "sra_bytes": limit,
           "bands": bands, "build_id": pkg.engine.library_build_id(), "runs": {}}
    texts = {}
    for name in ("one partition", "%d serial bands" % bands):
        work = tempfile.mkdtemp(prefix="mi355_bands_")
        al = pkg.MI355Aligner(device=0)
        t0 = time.time()
        try:
            if name == "one partition":
                out = pipeline.align(al, q0, q1, work, sra_limit=limit)
            else:
                out = pipeline.align_bands(al, q0, q1, work, [1] * bands, sra_limit=limit)
        finally:
            al.close()
        run = {"best": list(out["best"]), "seconds": {str(k): v for k, v in out["seconds"].items()}, "total_seconds": time.time() - t0,
               "crosspoints": {str(k): v for k, v in out["crosspoints"].items()},
               "alignment_score": out["alignment"].raw_score if out["alignment"] else None,
               "text_bytes": len(out["text"]) if out["text"] else 0}
        if "keeper" in out:
            run["keeper"] = out["keeper"]
            run["per_band"] = [{"band": b["band"], "role": b["role"], "seconds": {str(k): v for k, v in b["seconds"].items()},
                                "crosspoints": {str(k): v for k, v in b["crosspoints"].items()}} for b in out["bands"]]
            run["stage1_per_band"] = [{"seconds": b["seconds"], "pruned_cells": b["pruned_cells"], "initial_bound": b["initial_bound"],
                                       "special_rows": len(b["special_rows"])} for b in out["stage1"]["bands"]]
        else:
            run["stage1_kernel_ms"] = out["stage1"].get("kernel_ms")
            run["stage1_pruned_fraction"] = out["stage1"].get("pruned_cells", 0) / float(m) / n
        res["runs"][name] = run
        texts[name] = out["text"]
        print(json.dumps({name: run}), flush=True)
        shutil.rmtree(work, ignore_errors=True)
    a, b = res["runs"].values()
    res["same_text"] = len(set(texts.values())) == 1
    res["ok"] = a["best"] == b["best"] and a["alignment_score"] == b["alignment_score"] == a["best"][2]
    print(json.dumps({"ok": res["ok"], "same_text": res["same_text"]}), flush=True)
    if outfn:
        json.dump(res, open(outfn, "w"), indent=1)
    assert res["ok"], res
    return 0


if __name__ == "__main__":
    sys.exit(main())
