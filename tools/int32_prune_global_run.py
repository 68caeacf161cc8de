"""What MI355SW_F_INT32_PRUNE_GLOBAL buys on the int32 kernel family: one related pair, global recurrence, gap-initialised
borders, MI355SW_F_FORCE_INT32 -- once with the flag off (every cell computed) and once with it on, both asked to prune and
both handed the same initial_bound, which a packed engine's diagonal seed makes (mi355sw_seed_bound: the int32 family has
no seed of its own).

    python tools/int32_prune_global_run.py M N [OUT.json]        (the profile under profiles/: 16000000 14650000)

H[m][n] must be equal between the two runs; the result is one JSON record keyed by the library's build id: seconds (wall and
device-event kernel time), pruned_fraction, H[m][n] and the kernel's name per run."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    pkg = g.load_package()
    eng = pkg.engine
    m, n = int(argv[0]), int(argv[1])
    out_path = argv[2] if len(argv) > 2 else None
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
    runs = []
    for name, flags in (("flag off", eng.F_FORCE_INT32), ("flag on", eng.F_FORCE_INT32 | eng.F_INT32_PRUNE_GLOBAL)):
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            al.setSequences(s0, s1)
            t0 = time.time()
            al.streamBegin(part, recurrence_type=pkg.NEEDLEMAN_WUNSCH, first_row_init_type=pkg.INIT_WITH_GAPS,
                           first_column_init_type=pkg.INIT_WITH_GAPS, track_best=False, prune_blocks=True, want_last_row=True,
                           initial_bound=bound)
            while not al.streamPoll()[1]:
                time.sleep(0.005)
            h = int(al.streamReadLastRow(n - 1, 1)[0, 0])
            al.streamEnd()
            wall = time.time() - t0
            st = al.getStatistics()
        finally:
            al.close()
        rec = {"case": name, "wall_s": wall, "kernel_ms": st["kernel_ms"], "kernel": st["kernel"], "strip_rows": st["strip_rows"],
               "pruned_fraction": st["pruned_cells"] / float(m) / n, "tcups_mn_kernel": m * n / st["kernel_ms"] / 1e9, "h_m_n": h}
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    assert runs[0]["h_m_n"] == runs[1]["h_m_n"], "flag on and flag off disagree on H[m][n]"
    assert runs[0]["pruned_fraction"] == 0 and runs[1]["kernel"].endswith(",false,true>")
    out = {"workload": "%dx%d related pair (seqgen cfg=5), global, gap-initialised borders, MI355SW_F_FORCE_INT32, prune_blocks" % (m, n),
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
