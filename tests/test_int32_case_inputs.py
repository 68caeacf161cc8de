"""CPU: the inputs of tests/test_gpu_int32_family.py (tests/int32_cases.py) are what they claim -- shown with a plain numpy Gotoh
DP written here (X/CUDAligner.cu:276-289: E = max(Hleft - 3, Eleft) - 2, F = max(Hup - 3, Fup) - 2, H = max(0, Hdiag + (+1 / -3), E, F))
and, for the best cells, with the oracle itself.  No GPU: what the engine makes of these inputs is the GPU file's business."""
import numpy as np
import pytest

import int32_cases as ic

NEG = -10 ** 9


def gotoh_local(s0, s1):
    """H, E, F of the local alignment, (m + 1) x (n + 1), zero borders.  Row by row: E[i][j] = max over k < j of H[i][k] - 3 - 2 (j - k),
    and a cell whose H comes from E never opens a better gap than the one it continues, so the running maximum may be taken over
    max(0, diagonal, F) alone"""
    m, n = len(s0), len(s1)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    two_j = 2 * np.arange(n + 1, dtype=np.int64)
    s1 = np.asarray(s1)
    for i in range(1, m + 1):
        F[i, 1:] = np.maximum(H[i - 1, 1:] - 3, F[i - 1, 1:]) - 2
        sub = np.where(s1 == s0[i - 1], 1, -3)
        h = np.zeros(n + 1, dtype=np.int64)
        h[1:] = np.maximum(np.maximum(H[i - 1, :-1] + sub, F[i, 1:]), 0)
        run = np.maximum.accumulate(h + two_j)
        E[i, 1:] = run[:-1] - 3 - two_j[1:]
        H[i] = np.maximum(h, E[i])
        H[i, 0] = 0
    return H, E, F


def traceback(H, E, F, s0, s1, i, j):
    """the cells (i, j) the optimal path that ends in (i, j) crosses diagonally (diagonal first, then E, then F)"""
    pairs, state = [], "H"
    while i > 0 and j > 0:
        if state == "H":
            if H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + (1 if s0[i - 1] == s1[j - 1] else -3):
                pairs.append((i, j))
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                assert H[i, j] == F[i, j]
                state = "F"
        elif state == "E":
            if E[i, j] == H[i, j - 1] - 5:
                state = "H"
            j -= 1
        else:
            if F[i, j] == H[i - 1, j] - 5:
                state = "H"
            i -= 1
    return pairs


def test_gotoh_written_here_is_the_oracles(oracle):
    """the DP above against the oracle on a related pair with gaps: every cell of the last row and of the last column, and the best"""
    s0, s1 = ic.related_pair("raw15", 700, 300, 3)
    H, E, F = gotoh_local(s0, s1)
    ref = oracle.stage1(s0, s1, want_last_row=True, want_last_col=True)
    assert np.array_equal(H[-1], ref["last_row"][:, 0]) and np.array_equal(H[:, -1], ref["last_col"][:, 0])
    assert np.array_equal(F[-1, 1:], ref["last_row"][1:, 1]) and np.array_equal(E[1:, -1], ref["last_col"][1:, 1])
    i, j = [int(x) for x in np.argwhere(H == H.max())[0]]
    assert ref["best"] == (i, j, int(H.max()))


@pytest.mark.parametrize("way", list(ic.WAYS))
def test_the_ways_code_their_pairs_as_claimed(pkg, way):
    """mi355sw_sequence_codes (host code) on the grid pairs: the number of common byte values is the way's K with and without
    foreign bytes, the form is 1 (coded: seq0_shift = 2) for `profile` and `coded` and 0 (raw bytes, no shift) for the other two,
    and with K = 7 both sequences' foreign bytes share code 7"""
    from masa_cudalign_amd.engine import sequence_codes
    alpha, fl, _, profile, coded = ic.WAYS[way]
    for kind in ("iid", "foreign"):
        g = ic.GridPair(way, ic.row_counts(4), kind=kind)
        lut0, lut1, common, form = sequence_codes(g.s0, g.s1, fl)
        assert common == len(alpha), (way, kind, common)
        assert form == (1 if coded else 0)
        assert (form == 1 and common <= 7) == profile          # runtime.cpp, mi355sw_set_sequences: h->profile
        have0, have1 = set(g.s0.tolist()), set(g.s1.tolist())
        assert (have0 & have1) == set(alpha)
        if kind == "foreign":
            assert set(ic.FOREIGN0) <= have0 - have1 and set(ic.FOREIGN1) <= have1 - have0
            if way == "profile":
                assert {int(lut0[b]) for b in ic.FOREIGN0} == {7} == {int(lut1[b]) for b in ic.FOREIGN1}
            if way == "coded":
                assert {int(lut0[b]) for b in ic.FOREIGN0} == {14} and {int(lut1[b]) for b in ic.FOREIGN1} == {15}
    for name in ic.LOW_NAMES:
        s0, s1 = ic.with_alphabet(way, *ic.low_pair(name, way))
        assert sequence_codes(s0, s1, fl)[2:] == (len(alpha), 1 if coded else 0), name


def test_row_counts_reach_every_emit_position():
    """per height: ragged last strips whose emit lane is 0, 1 and 62 and whose emit row is 0, 1, R - 2 and R - 1; full strips; fewer
    rows than a lane holds; rows_per_lane 12, 24 and 32 are no height of this family (runtime.cpp, plan_geometry: 8, 16, 16)"""
    for R in ic.HEIGHTS:
        SH = 64 * R
        rows = ic.row_counts(R)
        assert {1, 2, R - 1, R, R + 1, SH - 1, SH, SH + 1, 2 * SH - 1, 2 * SH + 1} <= set(rows)
        assert {SH + R * k + d for k in (0, 1, 62) for d in (0, 1, R - 1)} <= set(rows)
        assert any(4 * SH < r <= 5 * SH for r in rows) and max(rows) <= 5 * SH
        emits = {ic.emit_position(R, r)[1:] for r in rows if r > SH and ic.emit_position(R, r)[0]}
        for lane in (0, 1, 62):
            assert {(lane, 0), (lane, 1), (lane, R - 2), (lane, R - 1)} <= emits, (R, lane, sorted(emits))


@pytest.mark.parametrize("way", list(ic.WAYS))
def test_low_complexity_pairs_tie_where_the_bookkeeping_looks(oracle, way):
    """Per low-complexity pair: every cell that holds the best score, from the DP above; the oracle's best is the (min i, then
    min j) cell among them -- the tie rule of the oracle itself on these inputs.

    Which ties a pair CAN show follows from its shape, not from any engine: with m > n and the best score equal to the length of
    seq1 (A^m/A^n, (AC)^m/(AC)^n, (ACG)^m/(CGA)^n, P^k/P; P^k/P^k' likewise) only the last column reaches it, so the ties lie in many strips and many lanes but never at
    two columns of one row; with seq0 = P (97 rows: one strip at every height) they lie at the columns 97 t of row 97 alone.  So
    the three kinds of tie -- two strips at R = 4, two lanes of one strip, two columns of one row -- are asserted where the shape
    allows them: strips and lanes for the tall periodic pairs, columns for P/P^k, and all three for P^k/PxP, the pair added
    for exactly that.  Every pair is printed."""
    SH, R = 256, 4
    shown = {}
    for three in (False, True):
        if three and way != "generic":
            continue                                     # the third run of columns goes to the packed kernel: ACGT, default flags
        for name in ic.LOW_NAMES:
            s0, s1 = ic.low_pair(name, way, three_columns=three)
            assert len(s0) <= 2100 and len(s1) <= (800 if three else 300)
            H = gotoh_local(s0, s1)[0]
            best = int(H[1:, 1:].max())
            cells = np.argwhere(H[1:, 1:] == best) + 1
            ref = oracle.stage1(s0, s1)
            assert ref["best"] == (int(cells[0][0]), int(cells[0][1]), best), (name, ref["best"], cells[:3])   # (A^m/C^n: (1, 1, 0))
            strip_of, lane_of = (cells[:, 0] - 1) // SH, ((cells[:, 0] - 1) % SH) // R
            strips = np.unique(strip_of)
            lanes = int(np.unique(np.unique(strip_of * 64 + lane_of) // 64, return_counts=True)[1].max())
            rows, counts = np.unique(cells[:, 0], return_counts=True)
            kinds = (len(strips) >= 2, lanes >= 2, int(counts.max()) >= 2)
            shown[(name, three)] = kinds
            print("%-8s %-18s%s best %4d at %5d cells: %d strips, %d lanes of one strip, %d columns of one row" %
                  (way, name, " x2" if three else "", best, len(cells), len(strips), lanes, int(counts.max())))
    for name in ("A^m/A^n", "(AC)^m/(AC)^n", "(ACG)^m/(CGA)^n", "P^k/P", "P^k/P^k'"):
        assert shown[(name, False)][:2] == (True, True), (name, shown[(name, False)])
    assert shown[("P/P^k", False)][2]
    assert shown[("P^k/PxP", False)] == (True, True, True), shown[("P^k/PxP", False)]
    assert shown[("A^m/C^n", False)] == (True, True, True)             # every cell holds the floor
    if way == "generic":
        for name in ("A^m/A^n", "(AC)^m/(AC)^n", "(ACG)^m/(CGA)^n", "P^k/P", "P^k/PxP"):  # the packed kernel's further run of columns: all three kinds
            assert shown[(name, True)] == (True, True, True), (name, shown[(name, True)])


@pytest.mark.parametrize("way", list(ic.WAYS))
def test_foreign_bytes_face_each_other_on_the_optimal_path(oracle, way):
    """For partitions of the `foreign` grid pair: the optimal path crosses at least one cell where a foreign byte of seq0 faces a
    foreign byte of seq1, and the oracle's best is lower than the best of the same letters with both foreign bytes replaced by
    one common letter -- a kernel that lets the two match (both carry code 7 with K = 7) scores higher, and is caught"""
    R = 4
    SH = 64 * R
    g = ic.GridPair(way, ic.row_counts(R), kind="foreign")
    a = ic.letters(way)[0]
    f0, f1 = set(ic.FOREIGN0), set(ic.FOREIGN1)
    checked = 0
    for r in (SH + 1, 2 * SH + 1, 4 * SH + SH // 2 + 3):
        for c in (65, 193, 300):
            i0, j0, i1, j1 = g.box(r, c)
            s0, s1 = g.s0[i0:i1], g.s1[j0:j1]
            H, E, F = gotoh_local(s0, s1)
            bi, bj, bs = oracle.stage1(s0, s1)["best"]
            assert H[bi, bj] == bs == H.max()
            path = traceback(H, E, F, s0, s1, bi, bj)
            facing = [(i, j) for i, j in path if int(s0[i - 1]) in f0 and int(s1[j - 1]) in f1]
            assert facing, (way, r, c)
            t0, t1 = s0.copy(), s1.copy()
            t0[np.isin(t0, list(f0))] = a
            t1[np.isin(t1, list(f1))] = a
            assert oracle.stage1(t0, t1)["best"][2] >= bs + 4 * len(facing) > bs, (way, r, c)
            checked += 1
    assert checked == 9


def test_custom_borders_carry_what_they_claim():
    """a corner of its own, values near OFFSET, -INF gap components in about a tenth of the cells and gap components within the
    gap-open penalty of H (they decide the first E / F) in the rest"""
    for corner in (ic.OFFSET, -ic.OFFSET):
        row, col = ic.custom_borders(700, 300, corner, 5)
        assert tuple(row[0]) == tuple(col[0]) == (corner, -ic.INF)
        for b in (row, col):
            void = b[1:, 1] == -ic.INF
            assert 0.05 < void.mean() < 0.2
            assert np.all(np.abs(b[:, 0] - corner) < 8 * len(b))
            near = (b[1:, 0] - b[1:, 1] < 3) & ~void
            assert near.mean() > 0.3
    row, col = ic.custom_borders(700, 300, 0, 6, local=True)
    assert row[:, 0].min() >= 0 and col[:, 0].max() < 60


def test_census_of_the_int32_inputs():
    """how many (way, R, rows, columns, edge form) combinations tests 1 and 2 of the GPU file run, and how many of them are ragged,
    narrower than a chunk or shorter than a lane (printed; the figures are in the CHANGELOG)"""
    c = ic.census()
    print("int32 family census:", c)
    grid = ic.instantiation_grid()
    assert len(grid) == 24 and len({g[:4] for g in grid}) == 24
    for R in ic.HEIGHTS:                                 # every byte-compare way at every height
        assert {g[4] for g in grid if g[0] == R and not g[2]} == {"coded", "raw15", "generic"}
    assert c["combinations"] >= c["distinct"] > 10000       # (tests 1 and 2 share the local form on a few shapes)
    assert c["ragged"] > 0.8 * c["combinations"] and c["n<64"] > 0.2 * c["combinations"] and c["m<R"] > 0
