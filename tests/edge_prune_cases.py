"""Shared by tests/test_edge_prune_host.py and tests/test_gpu_edge_prune.py: block pruning of alignments that END ON A
SEQUENCE EDGE (mi355sw_set_prune_end, Stage1Manager(prune_edges=True)).

The recurrence is NEEDLEMAN_WUNSCH, nothing is tracked, and the result is the best H on the allowed edge:

    mode 1 (ROW,    alignment_end AT_SEQUENCE_1)       last row              forced gap g = max(0, di - dj)
    mode 2 (COLUMN, alignment_end AT_SEQUENCE_2)       last column           forced gap g = max(0, dj - di)
    mode 3 (EITHER, alignment_end AT_SEQUENCE_1_OR_2)  last row or column    forced gap g = 0

with di / dj the rows / columns left to the end of the matrix.  A path through a cell that holds t ends with at most
t + min(di, dj) - 2 g (every diagonal step a match, the forced gap at its extension price) and an admissible alignment of at
least t - 3 min(di, dj) - (g > 0 ? 3 + 2 g : 0) exists (mismatches down the diagonal, then one gap along the edge reached).

Here: the statement every pruned edge run is held to (assert_edge_pruned_cells, the shape of helpers.assert_pruned_cells), a
full DP and a CELL-LEVEL pruned DP in numpy -- the most aggressive form of the rule, where the engine skips 64-column slabs
of whole strips."""
import numpy as np

INF = 999999999
MATCH, MISMATCH, GAP_OPEN, GAP_EXT = 1, -3, 3, 2
GAP_FIRST = GAP_OPEN + GAP_EXT
NW_PRUNE_MARGIN = 16          # csrc/sw_kernel_pk16.inc
ROW, COLUMN, EITHER = 1, 2, 3
MODES = (ROW, COLUMN, EITHER)
NEG = -(1 << 40)              # "no value" inside the numpy DPs (int64: never wraps)


def forced_gap(mode, di, dj):
    di, dj = np.asarray(di, dtype=np.int64), np.asarray(dj, dtype=np.int64)
    if mode == ROW:
        return np.maximum(0, di - dj)
    if mode == COLUMN:
        return np.maximum(0, dj - di)
    if mode == EITHER:
        return np.zeros(np.broadcast(di, dj).shape, dtype=np.int64)
    raise ValueError(mode)


def reach(mode, di, dj):
    """the most a path can still gain from a cell with di rows and dj columns to go"""
    return np.minimum(di, dj) * MATCH - GAP_EXT * forced_gap(mode, di, dj)


def lower_drop(mode, di, dj):
    """the most an admissible alignment through the cell can still lose"""
    g = forced_gap(mode, di, dj)
    return -MISMATCH * np.minimum(di, dj) + np.where(g > 0, GAP_OPEN + GAP_EXT * g, 0)


def assert_edge_pruned_cells(got, want, i, j, m, n, optimum, mode, *, lower_bound=True, where=""):
    """Which cells a run pruned under `mode` owes exactly.  got, want: (k, 2) int32 cells (H and the gap component) of the
    pruned run and of the unpruned reference; i, j: their 1-based DP coordinates in the whole m x n matrix (scalars
    broadcast; row 0 / column 0 are coordinate 0); optimum: the best H on the allowed edge.  A value v -- H or the gap
    component -- must be exact if v + reach(mode) >= optimum; lower_bound=True also asks got <= want everywhere.  Values at
    or below -INF / 2 are never "must".  Returns (n_must, n_differing)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.ndim == 2 and got.shape[1] == 2, (where, got.shape, want.shape)
    k = got.shape[0]
    i = np.broadcast_to(np.asarray(i, dtype=np.int64), (k,))
    j = np.broadcast_to(np.asarray(j, dtype=np.int64), (k,))
    assert np.all((0 <= i) & (i <= m) & (0 <= j) & (j <= n)), where
    g, w = got.astype(np.int64), want.astype(np.int64)
    r = reach(mode, m - i, n - j)
    must = w + r[:, None] >= optimum
    must &= w > -INF // 2
    bad = must & (g != w)
    if lower_bound:
        bad |= g > w
    if bad.any():
        idx = np.argwhere(bad)
        first = [(int(i[a]), int(j[a]), "HG"[c], int(g[a, c]), int(w[a, c]), int(w[a, c] + r[a]), int(optimum)) for a, c in idx[:8]]
        raise AssertionError("%s (mode %d): %d offending values of %d (%d must be equal); first (i, j, component, got, want, want + reach, optimum): %s"
                             % (where, mode, len(idx), 2 * k, int(must.sum()), first))
    return int(must.sum()), int((g != w).sum())


def assert_edge_pruned_borders(rows, last_row, last_col, ref, m, n, optimum, mode, *, col0, must_rows=(), where=""):
    """special rows {dp row: cells}, last row and last column of a pruned run against the unpruned oracle result `ref`;
    col0: the arrays start at coordinate 0 (a manager's) or 1 (the stream's).  Every row in must_rows must hold a must-value.
    Returns the number of must-values."""
    off = 0 if col0 else 1
    want_rows = dict(zip(ref.get("special_row_ids") or [], ref["special_rows"] if ref.get("special_rows") is not None else []))
    total = 0
    for i in sorted(rows):
        if i not in want_rows:                  # (a manager keeps the last row under its row number too)
            assert i == m and last_row is not None, (where, i)
            continue
        n_must, _ = assert_edge_pruned_cells(rows[i], want_rows[i][off:], i, np.arange(off, n + 1), m, n, optimum, mode, where="%s row %d" % (where, i))
        if i in must_rows:
            assert n_must > 0, "%s row %d: nothing to hold the run to" % (where, i)
        total += n_must
    if last_row is not None:
        total += assert_edge_pruned_cells(last_row, ref["last_row"][off:], m, np.arange(off, n + 1), m, n, optimum, mode, where=where + " last row")[0]
    if last_col is not None:
        total += assert_edge_pruned_cells(last_col, ref["last_col"][off:], np.arange(off, m + 1), n, m, n, optimum, mode, where=where + " last column")[0]
    return total


def edge_optimum(mode, last_row, last_col):
    """best H on the allowed edge(s); last_row / last_col with their coordinate-0 cell"""
    best = -INF
    if mode & 1:
        best = max(best, int(np.asarray(last_row)[:, 0].max()))
    if mode & 2:
        best = max(best, int(np.asarray(last_col)[:, 0].max()))
    return best


# ---------------------------------------------------------------------------------------------------------------------------
# numpy DPs, swept by anti-diagonals (a cell needs its left, upper and upper-left neighbours: the two diagonals before its own)
# ---------------------------------------------------------------------------------------------------------------------------
def borders(m, n, row_gaps, col_gaps):
    """first row / first column (H) of the start forms: zeroes, or gap penalties counted from the corner"""
    r = np.zeros(n + 1, dtype=np.int64)
    c = np.zeros(m + 1, dtype=np.int64)
    if row_gaps:
        r[1:] = -GAP_OPEN - GAP_EXT * np.arange(1, n + 1)
    if col_gaps:
        c[1:] = -GAP_OPEN - GAP_EXT * np.arange(1, m + 1)
    return r, c


START_BORDERS = {1: (False, True), 2: (True, False), 3: (False, False), 4: (True, True)}    # alignment_start -> (row_gaps, col_gaps)


def nw_dp(s0, s1, row_gaps, col_gaps, mode=0, bound=None):
    """H, E (horizontal gap), F (vertical gap) of the whole matrix, (m + 1) x (n + 1) int64, -INF where there is no value.
    mode 0: every cell.  mode 1..3: the cell-level pruned DP -- a cell is VOID (H = E = F = -INF) when every value that
    enters it (H of the three neighbours, E of the left one, F of the upper one) has v + reach + NW_PRUNE_MARGIN < bound, with
    reach taken at the neighbour; after every anti-diagonal the bound is raised to the best H - lower_drop of its cells.
    Returns (H, E, F, void share of the inner cells, final bound)."""
    s0, s1 = np.asarray(s0), np.asarray(s1)
    m, n = len(s0), len(s1)
    H = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    H[0, :], H[:, 0] = borders(m, n, row_gaps, col_gaps)
    lb = NEG if bound is None else int(bound)
    void = 0
    if mode:
        ii, jj = np.arange(m + 1)[:, None], np.arange(n + 1)[None, :]
        R = reach(mode, m - ii, n - jj) + NW_PRUNE_MARGIN        # per source cell
        D = lower_drop(mode, m - ii, n - jj)
        lb = max(lb, int((H[0, :] - D[0, :]).max()), int((H[:, 0] - D[:, 0]).max()))     # (the borders are cells too)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        sc = np.where(s0[i - 1] == s1[j - 1], MATCH, MISMATCH)
        hd, hu, hl, fu, el = H[i - 1, j - 1], H[i - 1, j], H[i, j - 1], F[i - 1, j], E[i, j - 1]
        e = np.maximum(el - GAP_EXT, hl - GAP_FIRST)
        f = np.maximum(fu - GAP_EXT, hu - GAP_FIRST)
        h = np.maximum(hd + sc, np.maximum(e, f))
        if mode:
            live = (hd + R[i - 1, j - 1] >= lb) | (np.maximum(hu, fu) + R[i - 1, j] >= lb) | (np.maximum(hl, el) + R[i, j - 1] >= lb)
            h, e, f = np.where(live, h, NEG), np.where(live, e, NEG), np.where(live, f, NEG)
            void += int((~live).sum())
        h, e, f = np.maximum(h, NEG), np.maximum(e, NEG), np.maximum(f, NEG)
        H[i, j], E[i, j], F[i, j] = h, e, f
        if mode:
            ok = h > NEG // 2
            if ok.any():
                lb = max(lb, int((h[ok] - D[i, j][ok]).max()))
    for a in (H, E, F):
        a[a <= NEG // 2] = -INF
    return H, E, F, void / float(m * n), lb


def seeded_pair(k, pkg):
    """pair k of the host cases: related and unrelated, m >> n and n >> m, up to 400 x 400"""
    rng = np.random.default_rng(9100 + k)
    shape = k % 4
    if shape == 0:
        m, n = int(rng.integers(150, 401)), int(rng.integers(150, 401))
    elif shape == 1:
        m, n = int(rng.integers(300, 401)), int(rng.integers(40, 120))
    elif shape == 2:
        m, n = int(rng.integers(40, 120)), int(rng.integers(300, 401))
    else:
        m = int(rng.integers(200, 401))
        n = int(np.clip(m + rng.integers(-60, 61), 100, 400))
    if k % 5 == 4:
        s0, s1 = pkg.seqgen.unrelated_pair(m, n, cfg=9100 + k)
    else:
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9100 + k, p_sub=[0.0, 0.02, 0.08, 0.15][k % 4], p_indel=[0.0, 0.002, 0.01, 0.02][(k // 4) % 4])
    start = (1, 2, 3, 4)[(k // 2) % 4]          # zero and gap borders
    return s0, s1, start
