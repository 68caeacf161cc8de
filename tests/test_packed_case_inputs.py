"""CPU: the inputs of tests/test_gpu_packed_family.py (tests/packed_cases.py) are what they claim.  No GPU: what the engine makes of
these inputs is the GPU file's business.  The plain numpy Gotoh DP of tests/test_int32_case_inputs.py is reused for the local
recurrence; the global one (gap-initialised borders) is written here for the pruning shapes."""
import numpy as np
import pytest

import int32_cases as ic
import packed_cases as pc
from helpers import MATCH
from test_int32_case_inputs import gotoh_local, traceback

NEG = -10 ** 9


def gotoh_global(s0, s1):
    """H of the global alignment, (m + 1) x (n + 1), gap-initialised borders: H[0][j] = -(3 + 2 j), H[i][0] = -(3 + 2 i), H[0][0] = 0
    (X/CUDAligner.cu:276-289 without the floor; a cell whose H comes from E never opens a better gap than the one it continues)"""
    m, n = len(s0), len(s1)
    two_j = 2 * np.arange(n + 1, dtype=np.int64)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    H[0, 1:] = -3 - two_j[1:]
    F = np.full(n + 1, NEG, dtype=np.int64)
    s1 = np.asarray(s1)
    for i in range(1, m + 1):
        F[1:] = np.maximum(H[i - 1, 1:] - 3, F[1:]) - 2
        sub = np.where(s1 == s0[i - 1], 1, -3)
        h = np.full(n + 1, NEG, dtype=np.int64)
        h[0] = -3 - 2 * i
        h[1:] = np.maximum(H[i - 1, :-1] + sub, F[1:])
        run = np.maximum.accumulate(h + two_j)
        E = np.full(n + 1, NEG, dtype=np.int64)
        E[1:] = run[:-1] - 3 - two_j[1:]
        H[i] = np.maximum(h, E)
    return H


def test_global_gotoh_written_here_is_the_oracles(oracle):
    s0, s1 = ic.related_pair(b"ACGT", 700, 300, 3)
    H = gotoh_global(s0, s1)
    ref = oracle.stage1(s0, s1, recurrence=oracle.NEEDLEMAN_WUNSCH, first_row_type=oracle.INIT_WITH_GAPS, first_col_type=oracle.INIT_WITH_GAPS,
                        want_last_row=True, want_last_col=True, best_mode=oracle.BEST_LAST_CELL)
    assert np.array_equal(H[-1], ref["last_row"][:, 0]) and np.array_equal(H[:, -1], ref["last_col"][:, 0])
    assert ref["best"] == (700, 300, int(H[-1, -1]))


# ---------------------------------------------------------------------------------------------------------------------
# the instantiations
# ---------------------------------------------------------------------------------------------------------------------
def test_the_instantiation_list_is_the_130_of_the_two_builds():
    """24 + 18 + 2 + 12 + 4 + 4 + 1 per twin, no name twice; the names test 1 of the GPU file asserts are the 24 unpruned ones"""
    names = []
    for wide in (False, True):
        groups = pc.instantiations(wide)
        assert [len(groups[g]) for g in ("strip", "prune", "mixed", "batch", "goal", "edge", "band")] == [24, 18, 2, 12, 4, 4, 1]
        assert all(("_wide<" in x) == wide for g in groups.values() for x in g)
        names += [x for g in groups.values() for x in g]
    assert len(names) == len(set(names)) == 130
    grid = pc.unpruned_grid()
    assert len(grid) == 48
    for wide in (False, True):
        got = {pc.strip_name(Rh, track, sw, False, wide) for w, Rh, track, sw, way in grid if w == wide}
        assert got == set(pc.instantiations(wide)["strip"])
        for Rh in pc.HEIGHTS:                                # every way of the twin at every height
            assert {g[4] for g in grid if g[0] == wide and g[1] == Rh} == set(pc.WIDE if wide else pc.NARROW)


# ---------------------------------------------------------------------------------------------------------------------
# the alphabets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", list(pc.WAYS))
def test_the_ways_code_their_pairs_as_claimed(pkg, way):
    """mi355sw_sequence_codes (host code) on the grid pairs: K common byte values with and without foreign bytes, form 1 (one-hot)
    for the narrow ways and 2 (code words) for the wide ones; A, C, G, T carry the codes below 4 wherever the table form is
    expected (acgt, switch -- whose fifth letter is code 4); the foreign codes are 7 / 7 up to K = 7, 14 / 15 at K = 14 and
    K / K + 1 in the wide form: 63 = the largest code (byte 252) at K = 62"""
    from masa_cudalign_amd.engine import sequence_codes
    alpha, fl, wide, K = pc.WAYS[way]
    for kind in ("iid", "foreign"):
        for Rh in (2, 16):
            g = pc.grid_pair(way, pc.row_counts(Rh), kind=kind, seed=Rh)
            lut0, lut1, common, form = sequence_codes(g.s0, g.s1, fl)
            assert (common, form) == (K, 2 if wide else 1), (way, kind, common, form)
            have0, have1 = set(g.s0.tolist()), set(g.s1.tolist())
            assert (have0 & have1) == set(pc.alphabet(way))
            if way in ("acgt", "switch"):
                assert sorted(int(lut1[b]) for b in b"ACGT") == [0, 1, 2, 3]
            if way == "switch":
                assert int(lut0[pc.SWITCH_LETTER]) == int(lut1[pc.SWITCH_LETTER]) == 4
            if kind == "foreign":
                assert set(pc.FOREIGN0) <= have0 - have1 and set(pc.FOREIGN1) <= have1 - have0
                f0, f1 = {int(lut0[b]) for b in pc.FOREIGN0}, {int(lut1[b]) for b in pc.FOREIGN1}
                want = ({K}, {K + 1}) if wide else (({7}, {7}) if K <= 7 else ({14}, {15}))
                assert (f0, f1) == want, (way, f0, f1)
                if way == "wide62":
                    assert max(f1) * 4 == 252
    for name in pc.LOW_NAMES:                                 # the low-complexity pairs inside the alphabets tests 4 runs them in
        s0, s1 = pc.with_alphabet(pc.alphabet(way), *pc.low_pair(name, pc.alphabet(way), three_columns=True))
        assert sequence_codes(s0, s1, fl)[2:] == (K, 2 if wide else 1), (way, name)


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------
def test_emit_census():
    """over the row counts of every R': every combination of emit_half in {0, 1} and emit_row in {0, 1, R'-2, R'-1} occurs in a ragged
    second strip, and emit_lane takes 0, 1, 31, 32 and 63; full strips, fewer rows than a block and than a lane are there too"""
    cen = pc.census()
    for Rh in pc.HEIGHTS:
        SH = 128 * Rh
        rows = pc.row_counts(Rh)
        assert {1, 2, Rh, Rh + 1, 2 * Rh - 1, 2 * Rh, 2 * Rh + 1, SH - 1, SH, SH + 1, 2 * SH - 1, 2 * SH + 1} <= set(rows) and min(rows) == 1
        assert {SH + Rh * v + d for v in pc.EMIT_V for d in (0, 1, 2, Rh - 1, Rh)} <= set(rows)
        assert any(4 * SH < r <= 5 * SH for r in rows) and max(rows) <= 5 * SH
        pos, lanes = cen[Rh]
        for half in (0, 1):
            for row in (0, 1, Rh - 2, Rh - 1):
                assert pos.get((half, row), 0) > 0, (Rh, half, row, pos)
        assert {0, 1, 31, 32, 63} <= set(lanes), (Rh, sorted(lanes))
        print("R' %2d: %2d row counts, (emit_half, emit_row): %s, emit_lane: %s" % (Rh, len(rows), sorted(pos.items()), sorted(lanes.items())))
    assert pc.emit_position(4, 512) == (False, 63, 1, 3) and pc.emit_position(4, 513) == (True, 0, 0, 0)
    assert pc.emit_position(4, 512 + 4 * 63 + 3) == (True, 31, 1, 2)
    assert pc.emit_position(11, 1000, row0=0) == (True, 45, 0, 9)


def test_column_counts_cover_the_chunk_edges():
    """every step of nchunks = (n + 127 + 63) / 64 from 2 to 7, and 9 at 449 columns; the counts around every multiple of 64; widths
    at which 0, 1, 2 and 5 chunks are unmasked"""
    assert pc.COLS == tuple(sorted(pc.COLS)) and set(ic.COLS) <= set(pc.COLS)
    assert {(n + 127 + 63) // 64 for n in pc.COLS} == set(range(2, 8)) | {9}
    for k in (64, 128, 192, 256):
        assert {k - 1, k, k + 1} <= set(pc.COLS)
    unmasked = {n: sum(f != "masked" for f in pc.chunk_forms(np.zeros(n, dtype=np.uint8))) for n in pc.COLS}
    assert unmasked[191] == 0 and unmasked[192] == 1 and unmasked[256] == 2 and unmasked[449] == 5, unmasked


# ---------------------------------------------------------------------------------------------------------------------
# the `switch` kind
# ---------------------------------------------------------------------------------------------------------------------
def test_switch_pairs_change_form_inside_a_strip(pkg):
    """the per-chunk rule of the kernel restated (packed_cases.chunk_forms: `masked`, `simple0..2` and `use_perm` of process_strip16):
    in the 449-column region chunk 2 takes the table form, chunks 3, 4 and 5 -- 'N' at column 200 is in their reach -- the
    general form and chunk 6 the table form again; 257 and 300 columns: table, general; with the last row read in a ragged
    strip (emit_any) no chunk takes the table form.  The ACGT pair takes the table form in every unmasked chunk, the 14-letter
    pair in none."""
    from masa_cudalign_amd.engine import sequence_codes
    for kind in ("iid", "foreign"):
        g = pc.grid_pair("switch", pc.row_counts(2), kind=kind)
        lut1 = sequence_codes(g.s0, g.s1, 0)[1]
        forms = {}
        for c in g.cols:
            j0 = g.j0[c]
            assert (c > pc.SWITCH_COL) == (pc.SWITCH_LETTER in g.s1[j0: j0 + c].tolist())
            if c > pc.SWITCH_COL:
                assert int(g.s1[j0 + pc.SWITCH_COL]) == pc.SWITCH_LETTER and list(g.s1[j0: j0 + c]).count(pc.SWITCH_LETTER) == 1
            forms[c] = pc.chunk_forms(lut1[g.s1[j0: j0 + c]])
        if kind == "iid":
            assert forms[449] == ["masked", "masked", "table", "general", "general", "general", "table", "masked", "masked"], forms[449]
            assert forms[300][2:4] == forms[257][2:4] == ["table", "general"]
            assert forms[256][2] == forms[192][2] == "table"
        else:                                                 # foreign bytes of seq1 every 37 / 41 columns: the general form
            assert "table" not in forms[449] and forms[449].count("general") == 5
        assert "table" not in pc.chunk_forms(lut1[g.s1[g.j0[449]: g.j0[449] + 449]], emit_any=True)
        for r in g.rows:                                      # seq0 carries the letter where the tiles of seq1's base string do
            i0 = g.i0[r]
            assert (r > pc.SWITCH_COL) == (pc.SWITCH_LETTER in g.s0[i0: i0 + r].tolist())
    g = pc.grid_pair("acgt", pc.row_counts(2))
    lut1 = sequence_codes(g.s0, g.s1, 0)[1]
    assert pc.chunk_forms(lut1[g.s1[g.j0[449]: g.j0[449] + 449]])[2:7] == ["table"] * 5
    g = pc.grid_pair("onehot14", pc.row_counts(2))
    lut1 = sequence_codes(g.s0, g.s1, 0)[1]
    assert pc.chunk_forms(lut1[g.s1[g.j0[449]: g.j0[449] + 449]])[2:7] == ["general"] * 5


# ---------------------------------------------------------------------------------------------------------------------
# the `foreign` kind
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", list(pc.WAYS))
def test_foreign_bytes_face_each_other_on_the_optimal_path(oracle, way):
    """the argument of tests/test_int32_case_inputs.py on the packed ways: in partitions of the `foreign` grid pair the optimal
    path crosses a cell where a foreign byte of seq0 faces one of seq1, and the same letters with both replaced by one common
    letter score at least 4 more per such cell -- a kernel that lets the two match (both carry code 7 up to K = 7) is caught"""
    Rh = 2
    SH = 128 * Rh
    g = pc.grid_pair(way, pc.row_counts(Rh), kind="foreign")
    a = np.frombuffer(pc.alphabet(way), dtype=np.uint8)[0]
    f0, f1 = set(pc.FOREIGN0), set(pc.FOREIGN1)
    checked = 0
    for r in (SH + 1, 2 * SH + 1, 4 * SH + SH // 2 + 3):
        for c in (129, 193, 300):                            # (65 columns of 62 letters: the best local path is too short to cross one)
            i0, j0, i1, j1 = g.box(r, c)
            s0, s1 = g.s0[i0:i1], g.s1[j0:j1]
            H, E, F = gotoh_local(s0, s1)
            bi, bj, bs = oracle.stage1(s0, s1)["best"]
            assert H[bi, bj] == bs == H.max()
            facing = [(i, j) for i, j in traceback(H, E, F, s0, s1, bi, bj) if int(s0[i - 1]) in f0 and int(s1[j - 1]) in f1]
            assert facing, (way, r, c)
            t0, t1 = s0.copy(), s1.copy()
            t0[np.isin(t0, list(f0))] = a
            t1[np.isin(t1, list(f1))] = a
            assert oracle.stage1(t0, t1)["best"][2] >= bs + 4 * len(facing) > bs, (way, r, c)
            checked += 1
    assert checked == 9


# ---------------------------------------------------------------------------------------------------------------------
# pruning shapes
# ---------------------------------------------------------------------------------------------------------------------
def nw_skippable_blocks(s0, s1, block_h, block_w=64):
    """(blocks the global rule may skip, blocks, cells in them, H[m][n]).  helpers.assert_pruned_cells holds a value v at (i, j) exact
    when v + min(di, dj) * MATCH - 2 |dj - di| >= H[m][n]; the gap components of a cell never exceed its H, so a cell may go when
    its H fails that test, and a block -- the reference's rule skips blocks, AbstractBlockPruning::isBlockPrunable -- when every
    cell in it may"""
    m, n = len(s0), len(s1)
    H = gotoh_global(s0, s1)
    di = (m - np.arange(m + 1))[:, None]
    dj = (n - np.arange(n + 1))[None, :]
    may = (H + np.minimum(di, dj) * MATCH - 2 * np.abs(dj - di) < H[m, n])[1:, 1:]
    skip = total = cells = 0
    for r in range(0, m, block_h):
        for c in range(0, n, block_w):
            b = may[r: r + block_h, c: c + block_w]
            total += 1
            if b.all():
                skip += 1
                cells += b.size
    return skip, total, cells, int(H[m, n])


@pytest.mark.parametrize("Rh", pc.HEIGHTS)
def test_pruning_shapes_are_the_smallest_the_reference_prunes_a_tenth_of(oracle, Rh):
    """PRUNE_SHAPES of the GPU file, per R' and twin (related_pair(alphabet, m, m, 700 + R'), m a multiple of the strip height).
    local: the smallest m at which the oracle's own pruned run, blocks of SH x 64, prunes at least a tenth of its blocks.
    global (the reference never prunes one, so there is no run to ask): the smallest m at which the blocks of SH x 64 the rule may
    skip whole hold at least a tenth of the cells -- none at one strip, where every block holds cells of the main diagonal; two
    strips at every height."""
    from test_gpu_packed_family import PRUNE_SHAPES
    SH = 128 * Rh
    for way in ("acgt", "wide15"):
        m_sw, pruned, blocks = PRUNE_SHAPES[(way, Rh)]["sw"]
        assert m_sw % SH == 0
        for m in range(SH, m_sw + 1, SH):
            s0, s1 = ic.related_pair(pc.alphabet(way), m, m, 700 + Rh)
            o = oracle.stage1(s0, s1, pruning=True, block_h=SH, block_w=64)
            if m < m_sw:
                assert 10 * o["blocks_pruned"] < o["blocks_total"], (way, Rh, m, o["blocks_pruned"], o["blocks_total"])
            else:
                assert (o["blocks_pruned"], o["blocks_total"]) == (pruned, blocks) and 10 * pruned >= blocks
        m_nw, skip, total, goal = PRUNE_SHAPES[(way, Rh)]["nw"]
        assert m_nw % SH == 0
        for m in range(SH, m_nw + 1, SH):
            s0, s1 = ic.related_pair(pc.alphabet(way), m, m, 700 + Rh)
            got = nw_skippable_blocks(s0, s1, SH)
            print("%s R' %d global %d x %d: %d of %d blocks may go, %d of %d cells, H[m][n] = %d" % (way, Rh, m, m, got[0], got[1], got[2], m * m, got[3]))
            if m < m_nw:
                assert 10 * got[2] < m * m, (way, Rh, m, got)
            else:
                assert (got[0], got[1], got[3]) == (skip, total, goal) and 10 * got[2] >= m * m, (way, Rh, m, got)


# ---------------------------------------------------------------------------------------------------------------------
# the mixed launch
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_shapes_are_what_the_cost_model_picks():
    """MIXED_SHAPES of the GPU file against the restated cost model (packed_cases.mixed_plan: step_ns, estimate_ns,
    pick_rows_per_lane and plan_geometry of runtime.cpp): every shape is a mixed launch with strips of both heights, the last
    1408-row strip is full, one row short, and ragged with emit_half 0 and 1; no smaller matrix with 2, 4 or 8 wavefronts is
    one.  (The GPU file asserts the kernel's name: a drift of the model fails there, loudly.)"""
    from test_gpu_packed_family import MIXED_SHAPES
    seen = set()
    for W, n, ms in MIXED_SHAPES:
        for m in ms:
            plan = pc.mixed_plan(m, n, W)
            assert plan is not None and 1 <= plan[0] < plan[1], (W, n, m, plan)
            row0, held = pc.mixed_last_strip(m, n, W)
            assert 0 < held <= 1408
            ragged, lane, half, row = pc.emit_position(11, m, row0=row0)
            seen.add("full" if held == 1408 else ("short" if held == 1407 else "ragged%d" % half))
            print("mixed W %d: %d x %d: %d + %d strips, the last holds %d rows: emit_lane %d half %d row %d" % (
                W, m, n, plan[0], plan[1] - plan[0], held, lane, half, row))
    assert seen == {"full", "short", "ragged0", "ragged1"}, seen
    smallest = min(m * n for W, n, ms in MIXED_SHAPES for m in ms)
    for W in (2, 4, 8):
        for n in range(100, 3000, 10):
            for m in range(1537, 60000, 64):
                plan = pc.mixed_plan(m, n, W)
                if plan and plan[0] >= 1:
                    assert m * n >= smallest - 64 * n, (W, m, n, smallest)
                    break


def test_custom_borders_of_a_tall_strip_stay_inside_the_spread_guard():
    """the custom first columns of test 2 move by at most 7 per row: over the tallest strip (2048 rows) the spread of H stays under
    the 24 000 the packed kernel accepts from border data (OVF16_SPREAD), so restarts == 0 can be asserted"""
    for corner in (pc.OFFSET, -pc.OFFSET):
        row, col = pc.custom_borders(2 * 2048 + 1, 300, corner, 5)
        h = col[:, 0].astype(np.int64)
        for r0 in range(0, len(h) - 1, 2048):
            seg = h[r0: r0 + 2049]
            assert seg.max() - seg.min() < 24000
