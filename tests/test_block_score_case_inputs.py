"""CPU: the inputs of the per-strip record tests (tests/block_score_cases.py) are what they claim -- with the oracle only.
A case that loses the property it exists for fails here instead of passing quietly on the GPU."""
import numpy as np
import pytest

import block_score_cases as bc

GRID = bc.grid_cases()
ALL = bc.all_block_cases()


def test_names_are_unique_and_sizes_within_the_limits():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    for c in ALL:
        assert c.m * c.n <= bc.MAX_CELLS and c.bands() <= bc.MAX_BANDS, c
        assert c.R in (0, 4, 8, 16) or (bc.ROUTES[c.route][2] and c.R in (12, 24, 32)), c


def test_every_value_meets_every_route():
    """heights, row counts, band widths and tie pairs of the issue's lists: each with each kernel route at least once"""
    for route, (_, _, packed) in bc.ROUTES.items():
        mine = [c for c in GRID if c.route == route]
        assert {c.R for c in mine} == set((0, 4, 8, 16) + ((12, 24, 32) if packed else ())), route
        assert {c.row_kind for c in mine if c.R} == set(bc.ROW_KINDS), route
        assert {c.width_kind for c in mine} == set(bc.WIDTH_KINDS), route
        assert set(bc.TIE_PAIRS) <= {c.pair for c in mine}, route


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_alphabet_decides_the_route(pkg, case):
    """the number of byte values common to both sequences is the route's K, and the coding form the one the route names
    (mi355sw_describe_coding's rule: include/mi355sw.h)"""
    s0, s1 = case.sequences()
    K = len(np.intersect1d(np.unique(s0), np.unique(s1)))
    assert K == len(bc.ROUTES[case.route][0])
    want = {"onehot": K <= 14, "wide15": K == 15, "wide62": K == 62, "int32flag": K == 8, "int32alpha": K == 15, "profile7": K == 7}
    assert want[case.route]
    assert len(s0) >= case.box[2] and len(s1) >= case.box[3]


@pytest.mark.parametrize("case", [c for c in ALL if c.R], ids=repr)
def test_row_counts_are_the_edges_they_name(case):
    SH = 64 * case.R
    ragged, lane, half, used = bc.last_row_place(case.R, case.m)
    kind = case.row_kind
    if case.fault:
        assert case.m > SH                                          # strip 1, where the overflow report is injected, exists
    if kind == "below":
        assert case.m < SH and ragged
    elif kind == "exact":
        assert case.m == SH and not ragged
    elif kind == "plus1":
        assert case.m == SH + 1 and (lane, half, used) == (0, "LO", 1)
    elif kind == "km1":
        assert (case.m + 1) % SH == 0 and case.m > SH and (lane, half, used) == (63, "HI", case.R // 2 - 1)
    elif kind == "ragged_lo":
        assert ragged and half == "LO" and 0 < lane < 63 and used < case.R // 2      # ends INSIDE the LO half: the HI rows of that lane are void
    elif kind == "ragged_hi":
        assert ragged and half == "HI" and 0 < lane < 63 and used < case.R // 2      # ends inside the HI half


@pytest.mark.parametrize("case", GRID, ids=repr)
def test_band_widths_are_the_edges_they_name(case):
    n, W, kind = case.n, case.W, case.width_kind
    if kind in ("63", "64", "65", "127"):
        assert W == int(kind) and n > 2 * W
    elif kind == "one_band":
        assert W >= n
    elif kind == "last1":
        assert n % W == 1 and n > W                                 # the one-column last band exists
    elif kind == "wide":
        assert W > 2048 and W % 64 != 0 and n > W


@pytest.mark.parametrize("case", [c for c in GRID if c.pair in bc.TIE_PAIRS and c.R], ids=repr)
def test_tie_pairs_have_ties_that_decide(oracle, case):
    """blocks whose best score stands in more than one cell, counted on the dense matrix (numpy) -- whose canonical cell is the
    oracle's in EVERY block, so the count is of the oracle's own grid.  The two constructed pairs tie in every block by their
    arithmetic; of the random ones no more is asked than that a tied block exists."""
    s0, s1 = case.slices()
    H = bc.local_matrix(s0, s1)
    ref = case.reference(oracle)
    SH, W = 64 * case.R, case.W
    tied = by_row = by_col = 0
    for (bx, by), (i, j, s) in ref["block_scores"].items():
        r0, r1, c0, c1 = 1 + by * SH, min(1 + (by + 1) * SH, case.m + 1), 1 + bx * W, min(1 + (bx + 1) * W, case.n + 1)
        cell, count = bc.canonical_cell(H, r0, r1, c0, c1)
        assert cell == (i + 1, j + 1, s), (bx, by)
        if count > 1:
            tied += 1
            ii, jj = np.nonzero(H[r0:r1, c0:c1] == s)
            by_row += int(len(set(ii.tolist())) > 1)
            by_col += int(np.count_nonzero(ii == ii[0]) > 1)
    blocks = len(ref["block_scores"])
    assert tied >= 1 and by_row + by_col >= tied, (tied, blocks)
    if case.pair in ("ones", "periodic"):
        assert tied == blocks, (tied, blocks)
    if case.pair == "ones":
        # H = min(i, j): above the diagonal a block's best fills its last ROW from column i on, below it its last COLUMN
        k = min(case.m, case.n)
        assert ref["best"] == (k, k, k)


def test_negative_case_has_only_negative_finite_block_bests(oracle):
    c = bc.NEGATIVE
    ref = c.reference(oracle)
    assert ref["grid"] == (8, 30)
    scores = [v[2] for v in ref["block_scores"].values()]
    assert len(scores) == 240 and max(scores) < 0 and min(scores) == -3442 and min(scores) > -oracle.INF


@pytest.mark.parametrize("case", bc.ONE_SIDED, ids=repr)
def test_one_sided_starts_have_one_border_of_each_kind(oracle, case):
    """one border of zeroes, the other of gap penalties -- and the blocks differ from those of the local and of the global form"""
    kw = case.oracle_kwargs(oracle)
    assert kw["recurrence"] == oracle.NEEDLEMAN_WUNSCH
    assert {kw["first_row_type"], kw["first_col_type"]} == {oracle.INIT_WITH_ZEROES, oracle.INIT_WITH_GAPS}
    s0, s1 = case.slices()
    mine = case.reference(oracle)["block_scores"]
    both = oracle.stage1(s0, s1, recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=oracle.INIT_WITH_GAPS, first_col_type=oracle.INIT_WITH_GAPS,
                         block_h=64 * case.R, block_w=case.W)["block_scores"]
    swapped = oracle.stage1(s0, s1, recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=kw["first_col_type"], first_col_type=kw["first_row_type"],
                            block_h=64 * case.R, block_w=case.W)["block_scores"]
    assert mine != both and mine != swapped


@pytest.mark.parametrize("case", bc.SLICED, ids=repr)
def test_sliced_partition_differs_from_the_same_box_at_the_origin(oracle, case):
    i0, j0, i1, j1 = case.box
    assert i0 % 64 and j0 % 64
    s0, s1 = case.sequences()
    at_origin = oracle.stage1(s0[:case.m], s1[:case.n], block_h=64 * case.R, block_w=case.W, **case.oracle_kwargs(oracle))
    sliced = case.reference(oracle)
    assert sliced["grid"] == at_origin["grid"]
    differ = sum(1 for k in sliced["block_scores"] if sliced["block_scores"][k] != at_origin["block_scores"][k])
    assert 2 * differ >= len(sliced["block_scores"]), differ        # a wrong offset cannot go unseen


@pytest.mark.parametrize("case", bc.LO_HI, ids=repr)
def test_planted_tie_stands_in_both_halves_of_one_lane(oracle, case):
    """H = T at (r, j) in the LO rows and at (r', j - 1) in the HI rows of one fully valid lane, nowhere else in rows up to r':
    the block's canonical cell is (r, j), and a lane that prefers its HI half on a tie reports (r', j - 1)"""
    R = case.R
    r, r2, j, T = bc.lo_hi_place(R)
    assert r // (64 * R) == r2 // (64 * R) == 1 and case.m == 2 * 64 * R          # strip 1, every row of it valid
    assert (r % (64 * R)) // R == (r2 % (64 * R)) // R == bc.LO_HI_LANE
    assert r % R == R // 2 - 1 and r2 % R == R - 1                                # the last LO row and the last HI row
    assert j < case.W
    s0, s1 = case.slices()
    H = bc.local_matrix(s0, s1)
    assert H.max() == T and H[r + 1, j + 1] == T and H[r2 + 1, j] == T
    ii, jj = np.nonzero(H == T)
    assert sorted(zip(ii.tolist(), jj.tolist())) == [(r + 1, j + 1), (r2 + 1, j)]
    assert case.reference(oracle)["block_scores"][(0, 1)] == (r, j, T)


def test_overflow_cases_cover_the_heights_of_both_packed_forms():
    got = {(c.route.rstrip("1562"), c.R) for c in bc.OVERFLOW}
    assert {("onehot", 4), ("onehot", 8), ("onehot", 16), ("wide", 4), ("wide", 8), ("wide", 16), ("onehot", 12)} <= got
    assert all(c.fault == 2 for c in bc.OVERFLOW)


def test_serial_pair_has_strict_and_tied_prefix_maxima(pkg, oracle):
    """the waves = 1 pair of the strip-score test: strips that beat everything above them and strips that only tie it"""
    s0, s1 = pkg.seqgen.unrelated_pair(bc.SERIAL_M, bc.SERIAL_N, cfg=bc.SERIAL_CFG)
    cells, _ = bc.strip_bests(oracle, s0, s1, 256)
    scores = [c[2] for c in cells]
    assert scores == [9, 9, 9, 11, 8, 9, 10, 10, 10, 10, 10, 9, 9, 9, 11, 8]
    strict, tied = bc.prefix_maxima(scores)
    assert strict == [0, 3] and tied == [1, 2, 14]


@pytest.mark.parametrize("route,sw", sorted({(r, sw) for r, _, _, sw in bc.STRIP_RUNS}))
def test_strip_pairs_have_several_strips_at_the_global_best_or_one(oracle, route, sw):
    """local runs: the low-scoring four-letter pair -- more than one strip holds the global best, so the rule "every strip whose
    best equals the global best has a record" speaks of several strips; global runs: strip bests differ"""
    s0, s1 = bc.strip_pair(route, sw)
    m, n = bc.STRIP_M, bc.STRIP_N
    assert n < 16384
    cells, ref = bc.strip_bests(oracle, s0[:m], s1[:n], 256, sw)
    scores = [c[2] for c in cells]
    assert len(scores) == 8
    top = max(scores)
    assert (ref["best"][2] == top) if sw else (top > 0)
    if sw:
        assert scores.count(top) >= 2, scores
