"""What MI355SW_F_WIDE_ALPHABET buys: one pair with 15 letters common to both sequences timed with the flag off (raw bytes,
the int32 kernels), with the flag on (the packed kernels' wide-alphabet twins) and, for scale, the same pair without the
extra letters (the packed kernels as they are) -- alternating, REPEAT times each; device-event kernel time and wall time.

    python tools/wide_alphabet_perf.py c2 DENSITY [REPEAT] [OUT.json]      BASELINE config C2: 3 M x 3 M unrelated, local, score only
    python tools/wide_alphabet_perf.py global DENSITY [REPEAT] [OUT.json]  16 M x 14.65 M related, global, block pruning asked for

The eleven IUPAC ambiguity codes NRYKMSWBDHV are written into both sequences at one position in DENSITY (1000: the table
form of the packed kernels is taken in most chunks; 40: the equality form in most).  The best cell (c2) / H[m][n] (global)
must be equal between flag on and flag off; the result is one JSON record keyed by the library's build id."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

EXTRA = np.frombuffer(b"NRYKMSWBDHV", dtype=np.uint8)


def sprinkle(seq, density, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    pos = rng.integers(0, len(out), len(out) // density)
    out[pos] = EXTRA[rng.integers(0, len(EXTRA), len(pos))]
    out[:len(EXTRA)] = EXTRA                     # every letter in both sequences, whatever the density
    return out


def main(argv):
    pkg = g.load_package()
    eng = pkg.engine
    mode, density = argv[0], int(argv[1])
    repeat = int(argv[2]) if len(argv) > 2 else 3
    out_path = argv[3] if len(argv) > 3 else None
    if mode == "c2":
        m = n = 3000000
        p0, p1 = pkg.seqgen.unrelated_pair(m, n, cfg=2)
        edge, prune = pkg.AT_ANYWHERE, False
        what = "3000000x3000000 unrelated pair (seqgen cfg=2, BASELINE C2), local, score only"
    elif mode == "global":
        m, n = 16000000, 14650000
        p0, p1 = pkg.seqgen.related_pair(m, n, cfg=5)
        edge, prune = pkg.AT_SEQUENCE_1_AND_2, True
        what = "16000000x14650000 related pair (seqgen cfg=5), global, block pruning asked for (--prune-global)"
    else:
        raise SystemExit(__doc__)
    w0, w1 = sprinkle(p0, density, 1), sprinkle(p1, density, 2)
    k = len(np.intersect1d(np.unique(w0), np.unique(w1)))
    cases = (("flag off", w0, w1, 0), ("flag on", w0, w1, eng.F_WIDE_ALPHABET), ("plain pair", p0, p1, 0))
    part = pkg.Partition(0, 0, m, n)
    runs = []
    for rep in range(repeat):
        for name, s0, s1, flags in cases:
            al = pkg.MI355Aligner(device=0, flags=flags)
            try:
                al.setSequences(s0, s1)
                mg = pkg.Stage1Manager(part, alignment_start=edge, alignment_end=edge, block_pruning=prune)
                t0 = time.time()
                al.alignPartition(part, mg)
                wall = time.time() - t0
                st = al.getStatistics()
            finally:
                al.close()
            rec = {"case": name, "repeat": rep, "kernel_ms": st["kernel_ms"], "seed_ms": st["seed_ms"], "wall_s": wall, "kernel": st["kernel"],
                   "profile_kernel": st["profile_kernel"], "restarts": st["restarts"], "pruned_fraction": st["pruned_cells"] / float(m) / n,
                   "tcups_mn_kernel": m * n / (st["kernel_ms"] + st["seed_ms"]) / 1e9, "best": [int(x) for x in mg.getBestScore()]}
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    on = [r for r in runs if r["case"] == "flag on"]
    off = [r for r in runs if r["case"] == "flag off"]
    assert all(r["best"] == off[0]["best"] for r in on + off), "flag on and flag off disagree on the result"
    assert all("_wide<" in r["kernel"] for r in on) and all(r["profile_kernel"] == 0 for r in off)

    def med(rs, key):
        return float(np.median([r[key] for r in rs]))
    out = {"workload": what, "letters": "NRYKMSWBDHV at one position in %d of both sequences" % density, "common_byte_values": k,
           "library_build_id": eng.library_build_id(), "source_build_id": eng.source_build_id(), "repeat": repeat,
           "median_kernel_ms": {c[0]: med([r for r in runs if r["case"] == c[0]], "kernel_ms") for c in cases},
           "median_wall_s": {c[0]: med([r for r in runs if r["case"] == c[0]], "wall_s") for c in cases}, "runs": runs}
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k2: out[k2] for k2 in ("workload", "letters", "common_byte_values", "library_build_id", "median_kernel_ms", "median_wall_s")}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
