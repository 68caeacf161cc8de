#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  tests/golden/stage4_edges.json: two pairs of the input classes tests/stage4_edge_cases.py adds --
letters that occur in one sequence only at aligned positions (at most 7 common letters), and low complexity -- once through
the REFERENCE's own pipeline (oracle/_ref/ref_driver): its crosspoint_03 list and the sha256 of its crosspoint_04 text.
tests/test_stage4_edge_inputs.py holds the oracle's stage 4 to these digests wherever it runs, and to the live reference
where that is built.

    python oracle/make_golden_stage4_edges.py                  (needs oracle/_ref: oracle/build_ref.sh)
    python oracle/make_golden_stage4_edges.py --search-gapped  (no reference needed: prints seeds for GAPPED_SEEDS)
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import stage4_edge_cases as E  # noqa: E402

REF_ARGS = ["--disk-size=500K", "--block=8192,8192"]
OUT = os.path.join(ROOT, "tests", "golden", "stage4_edges.json")
COLUMNS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def golden_pairs(pkg):
    """name -> (seq0, seq1).  The reference's FASTA reader is only known to pass letters: the foreign bytes are IUPAC letters"""
    return {"foreign_5_common": E.foreign_pair(pkg.seqgen, 5, only0=b"RK", only1=b"YM"), "low_complexity": E.low_complexity_single()}


def search_gapped(oracle, seeds, budget):
    """a greedy cover, cheapest pair first, of: the oriented corner type 0, 1, 2 x side x orientation at more than 256 rows, and
    every column count of COLUMNS with a gapped corner"""
    targets = set((t, side, inv) for t in (0, 1, 2) for side in "fr" for inv in (False, True)) | set(("cols", c) for c in COLUMNS)
    found = []
    for seed in range(seeds):
        x, y = E.gapped_pair(seed)
        if len(x) * len(y) > budget:
            continue
        hits = set()
        for limit, given, _, _ in E.ladder(oracle, x, y, [(0, 0, 0, 0), (0, len(x), len(y), E.nw_score(oracle, x, y))]):
            for rows, cols, t, side, inv in E.first_step_halves(given, limit):
                if rows > 256:
                    hits.add((t, side, inv))
                if t != 0 and cols in COLUMNS:
                    hits.add(("cols", cols))
        found.append((len(x) * len(y), seed, hits))
    chosen = []
    while targets:
        best = max(found, key=lambda f: (len(f[2] & targets) / (f[0] + 1e6)))
        if not best[2] & targets:
            break
        chosen.append(best[1])
        targets -= best[2]
    print("GAPPED_SEEDS =", tuple(sorted(chosen)), " cells", sum(f[0] for f in found if f[1] in chosen), " uncovered:", sorted(targets, key=str))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search-gapped", action="store_true")
    ap.add_argument("--seeds", type=int, default=400)
    ap.add_argument("--budget", type=int, default=6000000, help="largest pair (cells) the search may choose")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    pkg = graft.load_package()
    oracle = graft.load_oracle()
    if args.search_gapped:
        return search_gapped(oracle, args.seeds, args.budget)
    assert oracle.have_ref(), "build oracle/_ref first (oracle/build_ref.sh)"
    rec = {"generator": "oracle/make_golden_stage4_edges.py", "args": REF_ARGS, "cases": {}}
    for name, (s0, s1) in golden_pairs(pkg).items():
        ref = oracle.run_ref(s0, s1, REF_ARGS)
        got, _ = oracle.stage4(s0, s1, ref["crosspoints_3"], 16)
        assert got == ref["crosspoints_4"], name
        rec["cases"][name] = {"m": len(s0), "n": len(s1), "seq0_sha256": hashlib.sha256(s0.tobytes()).hexdigest(),
                              "seq1_sha256": hashlib.sha256(s1.tobytes()).hexdigest(), "best": list(ref["best"]),
                              "crosspoints_3": [list(p) for p in ref["crosspoints_3"]], "crosspoints_4_count": len(ref["crosspoints_4"]),
                              "crosspoints_4_sha256": hashlib.sha256(ref["crosspoints_4_txt"]).hexdigest()}
        print(name, len(s0), len(s1), "best", ref["best"], "points", len(ref["crosspoints_3"]), "->", len(ref["crosspoints_4"]))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
