"""Body of tests/test_gpu_goal_prune.py::test_pipeline_with_prune_traceback, runnable on its own:

    python tests/goal_prune_pipeline_case.py <fixture>        -> one JSON line, exit code 0 = every check held

The native pipeline on the ENGINE (cuda:0) twice on one full-pipeline fixture -- without and with prune_traceback -- at
engine-picked strip heights (the goal kernels are built for the heights the engine gives a goal sweep).  The run with the
option must leave the reference's best score, crosspoint_02 / 03 / 04 and alignment.00.txt; every goal-column sweep of 1024
columns and more must report skipped cells; the cells stage 2 processed are reported for both runs.
MI355SW_STAGE2_SPECULATE=0 walks the plain chain (one sweep per call), the default batches the sweeps from guessed crosspoints."""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

PIPELINE = {
    "full_pipeline_pruned_60000x50000_b8192": dict(sra_limit=4 * 1024 * 1024, block_pruning=True),
    "full_pipeline_global_60000x50000_b8192": dict(sra_limit=4 * 1024 * 1024, block_pruning=False, alignment_start=4, alignment_end=4),
}


def run(fixture):
    import __graft_entry__ as graft
    from helpers import load_golden, make_pair
    pkg = graft.load_package()
    from masa_cudalign_amd import fasta, pipeline
    from masa_cudalign_amd.crosspoints import CrosspointsFile, crosspoint_file
    case = [c for c in load_golden()["cases"] if c["name"] == fixture][0]
    s0, s1 = make_pair(pkg, case["seq"])
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    outs, works = {}, {}
    al = pkg.MI355Aligner(device=0)
    try:
        for mode in ("off", "on"):
            works[mode] = tempfile.mkdtemp(prefix="mi355_goal_prune_")
            outs[mode] = pipeline.align(al, q0, q1, works[mode], prune_traceback=(mode == "on"), **PIPELINE[fixture])
    finally:
        al.close()
    on, off, work = outs["on"], outs["off"], works["on"]
    checks = {"best": list(on["best"]) == case["best"],
              "crosspoints_2": CrosspointsFile(crosspoint_file(work, 2)).load().tuples() == [tuple(p) for p in case["crosspoints_2"]],
              "crosspoints_3": CrosspointsFile(crosspoint_file(work, 3)).load().tuples() == [tuple(p) for p in case["crosspoints_3"]],
              "crosspoints_4": hashlib.sha256(open(crosspoint_file(work, 4), "rb").read()).hexdigest() == case["crosspoints_4"]["file_sha256"],
              "alignment_txt": hashlib.sha256(on["text"]).hexdigest() == case["alignment_txt_sha256"],
              "off_alignment_txt": hashlib.sha256(off["text"]).hexdigest() == case["alignment_txt_sha256"],
              "off_prunes_nothing": off["stage2"]["pruned_cells"] == 0 and not any(any(c["bounded"]) for c in off["stage2"]["sweeps"])}
    sweeps = on["stage2"]["sweeps"]
    wide = [c for c in sweeps if any(b and w >= 1024 for b, w in zip(c["bounded"], c["widths"]))]
    checks["bounded_sweeps"] = len(wide) > 0
    checks["every_wide_goal_sweep_pruned"] = all(c["pruned_cells"] > 0 for c in wide)
    checks["goal_kernels"] = all(c["kernel"].endswith(",true,true>") for c in wide)
    res = {"fixture": fixture, "checks": checks, "ok": all(checks.values()), "processed_on": on["stage2"]["processed_cells"],
           "processed_off": off["stage2"]["processed_cells"], "pruned_on": on["stage2"]["pruned_cells"],
           "sweeps": [{"widths": c["widths"], "bounded": sum(c["bounded"]), "processed": c["processed_cells"], "pruned": c["pruned_cells"]} for c in sweeps],
           "seconds": {"off": off["seconds"], "on": on["seconds"]}}
    for w in works.values():
        shutil.rmtree(w, ignore_errors=True)
    print(json.dumps(res), flush=True)
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
