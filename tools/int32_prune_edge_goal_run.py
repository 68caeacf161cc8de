"""What MI355SW_F_INT32_PRUNE_EDGE_GOAL buys on the int32 kernel family: one related pair under MI355SW_F_FORCE_INT32,
gap-initialised borders, each case once with the flag off (every cell computed) and once with it on.

  * the edge rule, mode 3 (the alignment ends on the last row or the last column), over the whole M x N matrix, both runs
    handed the same initial_bound, which a packed engine's diagonal seed makes (mi355sw_seed_bound: the int32 family has no
    seed of its own);
  * one stage-2-shaped goal sweep: the partition of all M rows by the first W columns, last column handed out, with the
    column bound B = (largest H of the last column, from an unpruned sweep on the packed kernels) - 200.

    python tools/int32_prune_edge_goal_run.py M N [W] [OUT.json]        (the profile under profiles/: 16000000 14650000 1000000)

The best H of the edge (mode 3) and every last-column cell at or above B (goal) must be equal between the two runs; the result
is one JSON record keyed by the library's build id: seconds (wall and device-event kernel time), pruned_fraction and the
kernel's name per run."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    pkg = g.load_package()
    eng = pkg.engine
    m, n = int(argv[0]), int(argv[1])
    w = int(argv[2]) if len(argv) > 2 and argv[2].isdigit() else min(n, 1000000)
    out_path = argv[-1] if argv[-1].endswith(".json") else None
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=5)
    part = pkg.Partition(0, 0, m, n)
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        t0 = time.time()
        bound = al.seedBound(part, pkg.NEEDLEMAN_WUNSCH)
        seed_s = time.time() - t0
    finally:
        al.close()
    cases = (("flag off", eng.F_FORCE_INT32), ("flag on", eng.F_FORCE_INT32 | eng.F_INT32_PRUNE_EDGE_GOAL))
    runs = []

    def record(rule, name, cells, wall, st, **more):
        rec = {"rule": rule, "case": name, "wall_s": wall, "kernel_ms": st["kernel_ms"], "kernel": st["kernel"], "strip_rows": st["strip_rows"],
               "pruned_fraction": st["pruned_cells"] / float(cells), "tcups_mn_kernel": cells / st["kernel_ms"] / 1e9}
        rec.update(more)
        runs.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    # ---- the edge rule, mode 3 ----
    for name, flags in cases:
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            al.setSequences(s0, s1)
            t0 = time.time()
            al.setPruneEnd(3)
            al.streamBegin(part, recurrence_type=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=pkg.INIT_WITH_GAPS,
                           first_column_init_type=pkg.INIT_WITH_GAPS, track_best=False, prune_blocks=True, want_last_row=True,
                           want_last_column=True, initial_bound=bound)
            while not al.streamPoll()[1]:
                time.sleep(0.005)
            best = al.streamEdgeBest(3)
            al.streamEnd()
            wall = time.time() - t0
            st = al.getStatistics()
        finally:
            al.close()
        record("edge, mode 3", name, float(m) * n, wall, st, edge_best=list(best))
    assert runs[0]["edge_best"] == runs[1]["edge_best"], "flag on and flag off disagree on the best cell of the edge"
    assert runs[0]["pruned_fraction"] == 0 and runs[1]["kernel"].endswith(",false,true,false,true>"), runs

    # ---- one goal sweep ----
    gpart = pkg.Partition(0, 0, m, w)
    goal, columns = None, []
    # (the bound comes from an unpruned sweep on the packed kernels, so that both int32 runs bring it and get the same strip height)
    for name, flags in (("packed, no bound", 0),) + cases:
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            al.setSequences(s0, s1)
            mg = pkg.Stage1Manager(gpart, alignment_start=pkg.AT_SEQUENCE_1_AND_2, alignment_end=pkg.AT_SEQUENCE_1_OR_2, keep_last_row=True,
                                   keep_last_column=True)
            t0 = time.time()
            if goal is not None:
                al.setGoalBounds([goal])
            al.alignPartition(gpart, mg)
            wall = time.time() - t0
            st = al.getStatistics()
        finally:
            al.close()
        col = np.asarray(mg.lastColumn())[:, 0].copy()
        columns.append(col)
        if goal is None:
            goal = int(col.max()) - 200
            continue
        record("goal, column bound", name, float(m) * w, wall, st, bound=goal, cells_at_or_above_bound=int((col >= goal).sum()))
    must = columns[0] >= goal
    assert must.any() and all(np.array_equal(columns[0][must], c[must]) for c in columns[1:]), "a last-column cell at or above the bound differs"
    assert runs[2]["pruned_fraction"] == 0 and runs[3]["kernel"].endswith(",false,true,true>"), runs
    out = {"workload": "%dx%d related pair (seqgen cfg=5), gap-initialised borders, MI355SW_F_FORCE_INT32; edge rule mode 3 over the whole matrix, "
                       "goal sweep over %d rows x the first %d columns" % (m, n, m, w),
           "initial_bound": bound, "seed_bound_s": seed_s, "library_build_id": eng.library_build_id(), "source_build_id": eng.source_build_id(),
           "runs": runs}
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
