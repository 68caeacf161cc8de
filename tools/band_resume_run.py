"""One related pair on one MI355X, local, block pruning on, stage 1 in B serial column bands (tools/band_traceback_run.py's shape):
once straight through (pipeline.align_bands), once interrupted when band 1 is done -- the exception a progress callback raises at
band 2's begin -- and resumed by pipeline.align_bands(resume=True).  Both must end on the same best cell with an alignment that
re-scores to it, and the resumed run must skip the two bands that were done.

    python tools/band_resume_run.py M N [bands] [out.json]"""
import json, os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402
pkg = g.load_package()
from masa_cudalign_amd import fasta, pipeline
from masa_cudalign_amd.bands import serial_band_stage1, band_limits
m, n = int(sys.argv[1]), int(sys.argv[2])
bands = int(sys.argv[3]) if len(sys.argv) > 3 else 4
outfn = sys.argv[4] if len(sys.argv) > 4 else None
limit = min(max(200 * 1024, (m // 8192 + 1) * n * 8), 4 << 30)
s0, s1 = pkg.seqgen.related_pair(m, n, cfg=2)
q0 = fasta.Sequence(">s0", s0, fasta.SequenceModifiers())
q1 = fasta.Sequence(">s1", s1, fasta.SequenceModifiers())
res = {"workload": "%dx%d related pair (seqgen cfg=2), local, block pruning on, %d serial bands" % (m, n, bands), "sra_bytes": limit,
       "build_id": pkg.engine.library_build_id()}
base = os.environ.get("TMPDIR") or tempfile.gettempdir()
al = pkg.MI355Aligner(device=0)
class Kill(Exception):
    pass
try:
    work = tempfile.mkdtemp(prefix="mi355_resume_a_", dir=base)
    t = time.time()
    out = pipeline.align_bands(al, q0, q1, work, [1] * bands, sra_limit=limit)
    res["straight"] = {"best": list(out["best"]), "seconds": {str(k): v for k, v in out["seconds"].items()}, "total_seconds": time.time() - t,
                       "stage1_per_band": [b["seconds"] for b in out["stage1"]["bands"]], "alignment_score": out["alignment"].raw_score}
    print(json.dumps(res["straight"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    work = tempfile.mkdtemp(prefix="mi355_resume_b_", dir=base)
    pipeline.check_work_directory(work, q0, q1)
    def progress(event, band, row):
        if (event, band) == ("band_begin", 2):
            raise Kill()
    al.setSequences(s0, s1)
    t = time.time()
    try:
        serial_band_stage1(al, m, band_limits(n, [1] * bands), work, limit, prune_blocks=True, origin=(0, 0), extent=(m, n), resume=True,
                           progress=progress, **pipeline.chain_form(pkg.AT_ANYWHERE, pkg.AT_ANYWHERE))
        raise SystemExit("the chain was not interrupted")
    except Kill:
        pass
    finally:
        al.unsetSequences()
    first = time.time() - t
    left = sorted(os.path.relpath(os.path.join(d, f), work) for d, _s, fs in os.walk(work) for f in fs if f.endswith(".mi355"))
    t = time.time()
    out = pipeline.align_bands(al, q0, q1, work, [1] * bands, sra_limit=limit, resume=True)
    res["interrupted_after_band_1"] = {"seconds_until_the_interruption": first, "files_left": left, "resumed": out["resumed"],
        "best": list(out["best"]), "seconds": {str(k): v for k, v in out["seconds"].items()}, "total_seconds": time.time() - t,
        "stage1_per_band": [{"seconds": b["seconds"], "skipped": b["skipped"], "state_writes": b.get("state_writes"), "column_writes": b.get("column_writes")}
                            for b in out["stage1"]["bands"]], "alignment_score": out["alignment"].raw_score}
    print(json.dumps(res["interrupted_after_band_1"]), flush=True)
    shutil.rmtree(work, ignore_errors=True)
finally:
    al.close()
a, b = res["straight"], res["interrupted_after_band_1"]
res["ok"] = a["best"] == b["best"] and a["alignment_score"] == b["alignment_score"] == a["best"][2] and b["resumed"]["bands_skipped"] == 2
if outfn:
    json.dump(res, open(outfn, "w"), indent=1)
print(json.dumps({"ok": res["ok"]}))
assert res["ok"]
