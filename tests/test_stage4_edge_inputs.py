"""CPU: the inputs of tests/test_gpu_stage4_edges.py (tests/stage4_edge_cases.py) held to their conditions with the oracle
alone -- nobody has to trust that file's coverage claims -- and the oracle's stage 4 (oracle/stage4_oracle.c) pinned on the
two input classes that are new here: letters of one sequence only at aligned positions, and low complexity.

The census walks the ladder of limits the GPU test walks (each rung fed the oracle's list of the rung before) and records, for
every partition stage 4 splits FIRST at a rung, the two half-matrices mm_half_kernel would sweep: rows, columns, the type of
the crosspoint at the half's corner as the split's orientation sees it, the side, the orientation.  What it must contain are
conditions on the inputs, checked here; they are not measurements."""
import collections
import hashlib
import json
import os

import pytest

import stage4_edge_cases as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage4_edges.json")
ROW_RESIDUES = (255, 0, 1, 3, 4, 5)
COLUMNS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def _text(points):
    return ("START\n" + "".join("%d,%d,%d,%d\n" % tuple(p) for p in points) + "END\n").encode()


def _halves(rungs):
    return [h for limit, given, _, _ in rungs for h in E.first_step_halves(given, limit)]


def _winners(oracle, seq0, seq1, rungs):
    """(q, column, lenB) of every first-step split of the rungs down to limit 16 (no candidate beyond the first ballot below)"""
    out = []
    for limit, given, _, _ in rungs:
        if limit < 16:
            continue
        for k in E.first_step_partitions(given, limit):
            s, e = given[k - 1], given[k]
            p = E.first_step_point(oracle, seq0, seq1, s, e)
            col, lenB = E.split_column(s, e, p)
            out.append((E.winning_candidate(s, e, p), col, lenB))
    return out


def test_census_of_the_edge_inputs(pkg, oracle):
    s0, s1, cp = E.geometry_and_gapped(pkg.seqgen, oracle)
    g0, g1, gcp = E.gapped(oracle)
    l0, l1, lcp = E.low_complexity(oracle)
    main = E.ladder(oracle, s0, s1, cp, key="geometry+gapped")
    gap = E.ladder(oracle, g0, g1, gcp, key="gapped")
    low = E.ladder(oracle, l0, l1, lcp, key="low_complexity")
    halves = _halves(main) + _halves(low)
    print("\nstage-4 edge inputs: geometry + gapped %d partitions, %d x %d letters, %d cells; low complexity %d partitions; "
          "%d first-step halves over the ladder %s; final lists of %d and %d points"
          % (len(cp) - 1, len(s0), len(s1), sum((cp[k][1] - cp[k - 1][1]) * (cp[k][2] - cp[k - 1][2]) for k in range(1, len(cp))),
             len(lcp) - 1, len(halves), list(E.LADDER), len(main[-1][2]), len(low[-1][2])))

    # rows = 255, 0, 1, 3, 4, 5 (mod 256) at 255 rows and more: each side, each orientation
    by_rows = collections.Counter((rows % 256, side, inv) for rows, _, _, side, inv in halves if rows >= 255)
    print("rows mod 256 (>= 255 rows)   " + "  ".join("%s/%s" % (side, "inv" if inv else "dir") for side in "fr" for inv in (False, True)))
    for r in ROW_RESIDUES:
        counts = [by_rows[(r, side, inv)] for side in "fr" for inv in (False, True)]
        print("  %3d                        " % r + "  ".join("%5d" % c for c in counts))
        assert min(counts) > 0, (r, counts)
    small = collections.Counter(rows for rows, _, _, _, _ in halves if rows <= 4)
    print("rows 1, 2, 3, 4:", [small[r] for r in (1, 2, 3, 4)])
    assert all(small[r] > 0 for r in (1, 2, 3, 4))

    # columns at the chunk edges, each with a type-0 corner and with a gapped one
    by_cols = collections.Counter((cols, t != 0) for _, cols, t, _, _ in halves)
    print("columns   type-0 corner   gapped corner")
    for c in COLUMNS:
        print("  %5d   %8d   %12d" % (c, by_cols[(c, False)], by_cols[(c, True)]))
        assert by_cols[(c, False)] > 0 and by_cols[(c, True)] > 0, c

    # every oriented corner type on both sides, at more than one pass; the forward side's type 1 is row_open = 0
    by_type = collections.Counter((t, side, rows > 256) for rows, _, t, side, _ in halves)
    print("oriented type / side   all   rows > 256")
    for side in "fr":
        for t in (0, 1, 2):
            print("  %d %s              %7d   %7d" % (t, side, by_type[(t, side, False)] + by_type[(t, side, True)], by_type[(t, side, True)]))
            assert by_type[(t, side, True)] > 0, (t, side)

    # tie-breaks: winners beyond the first and the second ballot of 64 candidates, and at the extreme columns
    wins = _winners(oracle, l0, l1, low)
    wins_gap = _winners(oracle, g0, g1, gap)
    for name, w in (("low complexity", wins), ("gapped", wins_gap)):
        print("%s: %d splits at limits >= 16; q >= 64: %d, q >= 128: %d, column 0: %d, column lenB: %d"
              % (name, len(w), sum(q >= 64 for q, _, _ in w), sum(q >= 128 for q, _, _ in w), sum(c == 0 for _, c, _ in w),
                 sum(c == n for _, c, n in w)))
    both = wins + wins_gap
    assert any(q >= 64 for q, _, _ in both) and any(q >= 128 for q, _, _ in both)
    assert any(c == 0 for _, c, _ in both) and any(c == n for _, c, n in both)
    # all three crosspoint types come out of it
    assert {p[0] for p in main[-1][2]} == {0, 1, 2}


def test_first_step_halves_and_winning_candidate():
    """the census helpers on a list small enough to check by hand"""
    pts = [(0, 0, 0, 0), (1, 10, 4, 0), (2, 10, 4, 0), (0, 13, 24, 0), (0, 20, 24, 0)]
    # 10 x 4 direct; a zero-sided one; 3 x 20 inverse (seq1 split; start type 2 is seen as 1); 7 x 0
    assert E.first_step_halves(pts, 5) == [(5, 4, 0, "f", False), (5, 4, 1, "r", False), (10, 3, 1, "f", True), (10, 3, 0, "r", True)]
    assert E.first_step_halves(pts, 10) == [(10, 3, 1, "f", True), (10, 3, 0, "r", True)]
    assert E.first_step_halves(pts, 20) == []
    # lenB = 4: jmid1 = 2; the kernel's order of columns is 2, 2, 3, 1, 4, 0
    s, e = pts[0], pts[1]
    assert [E.winning_candidate(s, e, (0, 5, c, 0)) for c in (2, 3, 1, 4, 0)] == [0, 2, 3, 4, 5]
    # lenB = 3: jmid1 = 2; columns 2, 1, 3, 0; inverse: the column is an i
    s, e = pts[2], pts[3]
    assert [E.winning_candidate(s, e, (0, 10 + c, 14, 0)) for c in (2, 1, 3, 0)] == [0, 1, 2, 3]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _golden_pairs(pkg):
    return {"foreign_5_common": E.foreign_pair(pkg.seqgen, 5, only0=b"RK", only1=b"YM"), "low_complexity": E.low_complexity_single()}


@pytest.mark.parametrize("name", ["foreign_5_common", "low_complexity"])
def test_oracle_against_the_recorded_reference(pkg, oracle, name):
    """the reference's crosspoint_04 text of the two pairs (sha256, recorded by oracle/make_golden_stage4_edges.py) from its
    crosspoint_03 list: the oracle's stage 4 writes the same bytes.  Needs no reference."""
    case = _golden()["cases"][name]
    s0, s1 = _golden_pairs(pkg)[name]
    assert hashlib.sha256(s0.tobytes()).hexdigest() == case["seq0_sha256"] and hashlib.sha256(s1.tobytes()).hexdigest() == case["seq1_sha256"]
    got, _ = oracle.stage4(s0, s1, [tuple(p) for p in case["crosspoints_3"]], 16)
    assert len(got) == case["crosspoints_4_count"]
    assert hashlib.sha256(_text(got)).hexdigest() == case["crosspoints_4_sha256"]


@pytest.mark.parametrize("name", ["foreign_5_common", "low_complexity"])
def test_oracle_against_the_live_reference(pkg, oracle, name, tmp_path):
    """MASA-Core itself on a pair with 5 common letters and letters of one sequence only at aligned positions (R, K in seq0
    only; Y, M in seq1 only), and on a low-complexity pair: its crosspoint_04 is the oracle's stage 4 of its crosspoint_03,
    and its digest is the committed one"""
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference's sources)")
    g = _golden()
    s0, s1 = _golden_pairs(pkg)[name]
    ref = oracle.run_ref(s0, s1, g["args"], workdir=str(tmp_path))
    got, _ = oracle.stage4(s0, s1, ref["crosspoints_3"], 16)
    assert got == ref["crosspoints_4"]
    assert hashlib.sha256(ref["crosspoints_4_txt"]).hexdigest() == g["cases"][name]["crosspoints_4_sha256"]
    assert [list(p) for p in ref["crosspoints_3"]] == g["cases"][name]["crosspoints_3"]
    if name == "foreign_5_common":
        # the foreign letters are in the aligned region, so the refinement walked over them
        assert ref["crosspoints_4"][0][1] < 60 and ref["crosspoints_4"][-1][1] > 2800
