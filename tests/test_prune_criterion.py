"""CPU: the criterion every pruned-run test goes through (helpers.assert_pruned_cells), held against the reference's rule.

Reference: AbstractBlockPruning::isBlockPrunable, M/libmasa/pruning/AbstractBlockPruning.cpp:70-111 -- a block is skipped
when score + min(rows left, columns left) * match <= bestScore.  Per cell of a local alignment, with the final best score:
a value v (H or a gap component) at (i, j) may differ from the unpruned one only if v + min(m - i, n - j) * match <= best.
Three checks: the oracle's own pruned run stays inside the criterion (and the criterion is far from empty there); the helper
rejects what it has to reject; and on a small matrix, computed here by a plain Gotoh sweep that shares nothing with the
oracle, a simulated skipper that obeys the rule breaks no non-exempt value while one that is a single point too eager does."""
import numpy as np
import pytest

from helpers import INF, NEEDLEMAN_WUNSCH, SMITH_WATERMAN, assert_pruned_cells, oracle_full

MATCH, MISMATCH, GAP_FIRST, GAP_EXT = 1, -3, 5, 2         # the reference's DNA scores: opening a gap costs 3 + 2, extending it 2


def _h_only(cells):
    """the same cells with the gap component voided: the helper then counts H values alone"""
    c = np.array(cells, dtype=np.int32)
    c[:, 1] = -INF
    return c


def test_oracle_pruned_run_stays_inside_the_criterion(pkg, oracle):
    """related_pair(60000, 50000, cfg=31): the oracle's pruned run (1024 x 1024 blocks, the restatement of the reference's
    pruning) against its unpruned run -- special rows every 8192 rows, last row, last column, H and F.  Hundreds of thousands
    of values differ, none of those the criterion says must be equal; the count of must-H-cells per row is pinned so that
    the criterion cannot silently become vacuous.  (The reference leaves stale, sometimes higher values in skipped blocks:
    lower_bound=False.)"""
    m, n = 60000, 50000
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=31)
    full = oracle_full(oracle, s0, s1)
    pruned = oracle.stage1(s0, s1, pruning=True, block_h=1024, block_w=1024, special_row_interval=8192,
                           want_last_row=True, want_last_col=True)
    best = full["best"]
    assert tuple(pruned["best"]) == tuple(best) and best[2] == 37990
    assert (pruned["blocks_pruned"], pruned["blocks_total"]) == (1420, 2891)
    assert pruned["special_row_ids"] == full["special_row_ids"] == [8192 * k for k in range(1, 8)]
    cols = np.arange(0, n + 1)
    must = differ = 0
    per_row_h = []
    for i, got, want in zip(full["special_row_ids"], pruned["special_rows"], full["special_rows"]):
        a, b = assert_pruned_cells(got, want, i, cols, m, n, best[2], SMITH_WATERMAN, lower_bound=False, where="row %d" % i)
        must, differ = must + a, differ + b
        per_row_h.append(assert_pruned_cells(_h_only(got), _h_only(want), i, cols, m, n, best[2], SMITH_WATERMAN, lower_bound=False)[0])
    a, b = assert_pruned_cells(pruned["last_row"], full["last_row"], m, cols, m, n, best[2], SMITH_WATERMAN, lower_bound=False, where="last row")
    must, differ = must + a, differ + b
    a, b = assert_pruned_cells(pruned["last_col"], full["last_col"], np.arange(0, m + 1), n, m, n, best[2], SMITH_WATERMAN, lower_bound=False, where="last column")
    must, differ = must + a, differ + b
    print("values that differ: %d, values that must be equal: %d, H cells per row: %s" % (differ, must, per_row_h))
    assert per_row_h[:6] == [12010, 19802, 8227, 7418, 6240, 69]
    assert 100000 < must < 115000 and 350000 < differ < 385000


def _cells(h, f):
    return np.stack([np.asarray(h, dtype=np.int32), np.asarray(f, dtype=np.int32)], axis=1)


def test_helper_rejects_and_accepts_what_it_should():
    """m = n = 100, best 60, one row at i = 50 (reach = min(50, 100 - j)): a must-cell lowered by 1 is rejected in H and in the
    gap component; an exempt cell raised by 1 is rejected under lower_bound=True only; a local H of -1 is rejected; an
    exempt cell lowered to 0 is accepted; the void F of column 0 is never a must"""
    m = n = 100
    j = np.arange(0, n + 1)
    h = np.where((j >= 30) & (j <= 50), 40, 3)            # 40 + 50 > 60: must; 3 + 50 <= 60: exempt
    f = np.where((j >= 30) & (j <= 50), 35, 2)
    f[0] = -INF
    want = _cells(h, f)
    args = (50, j, m, n, 60, SMITH_WATERMAN)
    assert assert_pruned_cells(want.copy(), want, *args) == (42, 0)
    for comp in (0, 1):
        got = want.copy()
        got[40, comp] -= 1
        with pytest.raises(AssertionError, match=r"1 offending.*\(50, 40, '%s', %d, %d, %d, 60\)" % ("HG"[comp], want[40, comp] - 1, want[40, comp], want[40, comp] + 50)):
            assert_pruned_cells(got, want, *args, where="row 50")
        with pytest.raises(AssertionError):
            assert_pruned_cells(got, want, *args, lower_bound=False)
    got = want.copy()
    got[70, 0] += 1                                       # exempt, but no lower bound any more
    with pytest.raises(AssertionError):
        assert_pruned_cells(got, want, *args)
    assert assert_pruned_cells(got, want, *args, lower_bound=False) == (42, 1)
    got = want.copy()
    got[70, 0] = -1
    with pytest.raises(AssertionError):
        assert_pruned_cells(got, want, *args)
    got = want.copy()
    got[70] = (0, -INF)
    assert assert_pruned_cells(got, want, *args) == (42, 2)
    # a value exactly on the bound is exempt (the reference's <=): 10 + 50 == 60
    want2 = want.copy()
    want2[20] = (10, 10)
    got = want2.copy()
    got[20] = (0, 0)
    assert assert_pruned_cells(got, want2, *args) == (42, 2)
    want2[20, 0] = 11
    with pytest.raises(AssertionError):
        assert_pruned_cells(got, want2, *args)
    # scalar i and scalar j both broadcast; coordinates outside the matrix are a mistake of the caller
    with pytest.raises(AssertionError):
        assert_pruned_cells(want, want, 101, j, m, n, 60, SMITH_WATERMAN)
    # global: v + min(di, dj) - 2 |dj - di| >= goal, equality included
    want = _cells([0, 10, 9], [0, 10, 9])
    got = _cells([0, 10, 0], [0, 10, -INF])
    assert assert_pruned_cells(got, want, 90, np.array([90, 90, 90]), m, n, 20, NEEDLEMAN_WUNSCH) == (2, 2)
    got[1, 1] = 9
    with pytest.raises(AssertionError):
        assert_pruned_cells(got, want, 90, 90, m, n, 20, NEEDLEMAN_WUNSCH)


def _gotoh(s0, s1, skip_below=None, best=None):
    """local Gotoh over the whole matrix in Python integers, every cell kept: H, E (gap along the row), F (gap along the
    column).  skip_below = t simulates a skipper: a cell whose freshly computed H has H + reach <= best - t is written as
    H = 0, E = F = -INF, and its successors are computed from that."""
    m, n = len(s0), len(s1)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), -INF, dtype=np.int64)
    F = np.full((m + 1, n + 1), -INF, dtype=np.int64)
    a, b = s0.tolist(), s1.tolist()
    for i in range(1, m + 1):
        hp, fp = H[i - 1].tolist(), F[i - 1].tolist()
        hr, er, fr = [0] * (n + 1), [-INF] * (n + 1), [-INF] * (n + 1)
        ai = a[i - 1]
        for j in range(1, n + 1):
            e = max(er[j - 1] - GAP_EXT, hr[j - 1] - GAP_FIRST)
            f = max(fp[j] - GAP_EXT, hp[j] - GAP_FIRST)
            h = max(0, hp[j - 1] + (MATCH if ai == b[j - 1] else MISMATCH), e, f)
            if skip_below is not None and h + min(m - i, n - j) * MATCH <= best - skip_below:
                h, e, f = 0, -INF, -INF
            hr[j], er[j], fr[j] = h, max(e, -INF), max(f, -INF)
        H[i], E[i], F[i] = hr, er, fr
    return H, E, F


def test_criterion_is_closed_under_dependence_by_brute_force(pkg, oracle):
    """related_pair(400, 300, cfg=5), all 120 000 cells, H / E / F: a skipper that obeys the rule with t = 50, 5, 0 to spare
    changes tens of thousands of values and not one the criterion calls non-exempt; a skipper one point too eager (t = -1)
    does break non-exempt values, and the helper says so -- the smallest demonstration that the check can fail."""
    m, n = 400, 300
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=5)
    H, E, F = _gotoh(s0, s1)
    best = int(H.max())
    ref = oracle.stage1(s0, s1, want_last_row=True, want_last_col=True)      # the two restatements agree where the oracle hands out cells
    assert ref["best"][2] == best == 268
    assert np.array_equal(ref["last_row"][1:, 0], H[m, 1:]) and np.array_equal(ref["last_row"][1:, 1], F[m, 1:])
    assert np.array_equal(ref["last_col"][1:, 0], H[1:, n]) and np.array_equal(ref["last_col"][1:, 1], E[1:, n])
    ii, jj = np.meshgrid(np.arange(1, m + 1), np.arange(1, n + 1), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()

    def check(Hs, Es, Fs):
        out = []
        for G, Gs in ((E, Es), (F, Fs)):
            want = _cells(H[1:, 1:].ravel(), G[1:, 1:].ravel())
            got = _cells(Hs[1:, 1:].ravel(), Gs[1:, 1:].ravel())
            out.append(assert_pruned_cells(got, want, ii, jj, m, n, best, SMITH_WATERMAN, where="H and %s" % ("E" if G is E else "F")))
        return out

    for t in (50, 5, 0):
        Hs, Es, Fs = _gotoh(s0, s1, skip_below=t, best=best)
        (must_e, diff_e), (must_f, diff_f) = check(Hs, Es, Fs)
        assert int((Hs != H).sum()) > 30000 and must_e > 10000 and must_f > 10000, (t, must_e, must_f)
        print("t = %d: %d H values differ; must (H + E) %d, (H + F) %d" % (t, int((Hs != H).sum()), must_e, must_f))
    Hs, Es, Fs = _gotoh(s0, s1, skip_below=-1, best=best)
    with pytest.raises(AssertionError, match="offending"):
        check(Hs, Es, Fs)
