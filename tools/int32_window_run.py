"""What MI355SW_F_INT32_WINDOW buys on the int32 kernel family: tools/int32_prune_edge_goal_run.py's two cases -- one related pair
under MI355SW_F_FORCE_INT32 | MI355SW_F_INT32_PRUNE_EDGE_GOAL, gap-initialised borders -- each REPEATS times with the window flag
off ("walk": every strip walks the whole width) and on ("window"), taking turns:

  * the edge rule, mode 3, over the whole M x N matrix, initial_bound from a packed engine's mi355sw_seed_bound;
  * one stage-2-shaped goal sweep: all M rows by the first W columns, B = (largest H of the last column, from an unpruned
    sweep on the packed kernels) - 200;
  * as reference points, the packed family on the same edge run with its window and under MI355SW_F_NO_WINDOW, once each.

    python tools/int32_window_run.py M N [W] [REPEATS] [--walk-only] [OUT.json]      (the profile: 16000000 14650000 1000000 3)

--walk-only leaves the flag out altogether: with MI355SW_LIB pointing at another build's library (the parent commit's) this is
that build's yardstick on the same pair.  The best cell of the edge and every last-column cell at or above B must be equal in
all runs.  The result is one JSON record keyed by the library's build id."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def main(argv):
    walk_only = "--walk-only" in argv
    argv = [a for a in argv if a != "--walk-only"]
    if len(argv) < 2:
        raise SystemExit(__doc__)
    pkg = g.load_package()
    eng = pkg.engine
    m, n = int(argv[0]), int(argv[1])
    nums = [int(a) for a in argv[2:] if a.isdigit()]
    w = nums[0] if nums else min(n, 1000000)
    repeats = nums[1] if len(nums) > 1 else 3
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
    base = eng.F_FORCE_INT32 | eng.F_INT32_PRUNE_EDGE_GOAL
    cases = [("walk", base)] + ([] if walk_only else [("window", base | eng.F_INT32_WINDOW)])
    runs = []

    def record(rule, name, cells, wall, st, **more):
        rec = {"rule": rule, "case": name, "wall_s": wall, "kernel_ms": st["kernel_ms"], "kernel": st["kernel"], "strip_rows": st["strip_rows"],
               "pruned_fraction": st["pruned_cells"] / float(cells), "tcups_mn_kernel": cells / st["kernel_ms"] / 1e9}
        rec.update(more)
        runs.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    def edge_run(rule, name, flags):
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
        return record(rule, name, float(m) * n, wall, st, edge_best=list(best))

    # ---- the edge rule, mode 3 ----
    for _ in range(repeats):
        for name, flags in cases:
            rec = edge_run("edge, mode 3", name, flags)
            assert rec["kernel"].endswith(",false,true,true>" if name == "window" else ",false,true,false,true>"), rec
    assert all(r["edge_best"] == runs[0]["edge_best"] for r in runs), "the runs disagree on the best cell of the edge"
    if not walk_only:
        for name, flags in (("packed, window", 0), ("packed, MI355SW_F_NO_WINDOW", eng.F_NO_WINDOW)):
            rec = edge_run("edge, mode 3, packed family", name, flags)
            assert rec["edge_best"] == runs[0]["edge_best"] and "pk16" in rec["kernel"], rec

    # ---- one goal sweep ----
    gpart = pkg.Partition(0, 0, m, w)
    goal, columns = None, []
    # (the bound comes from an unpruned sweep on the packed kernels, so that every int32 run brings it and gets the same strip height)
    for name, flags in [("packed, no bound", 0)] + cases * repeats:
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
        if goal is None:
            goal = int(col.max()) - 200
            columns.append(col)
            continue
        must = columns[0] >= goal
        assert must.any() and np.array_equal(columns[0][must], col[must]), "a last-column cell at or above the bound differs"
        rec = record("goal, column bound", name, float(m) * w, wall, st, bound=goal, cells_at_or_above_bound=int((col >= goal).sum()))
        assert rec["kernel"].endswith(",true,true,false,true>" if name == "window" else ",false,true,true>"), rec
    out = {"workload": "%dx%d related pair (seqgen cfg=5), gap-initialised borders, MI355SW_F_FORCE_INT32 | MI355SW_F_INT32_PRUNE_EDGE_GOAL; edge rule mode 3 over "
                       "the whole matrix, goal sweep over %d rows x the first %d columns; %d runs each, walk and window taking turns" % (m, n, m, w, repeats),
           "initial_bound": bound, "seed_bound_s": seed_s, "library_build_id": eng.library_build_id(), "source_build_id": eng.source_build_id(),
           "library": "another build's (MI355SW_LIB)" if os.environ.get("MI355SW_LIB") else "this tree's", "runs": runs}
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
