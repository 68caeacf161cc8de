"""GPU (-m gpu): MI355SW_F_WIDE_ALPHABET -- pairs with 15 to 62 byte values common to both sequences on the packed kernels'
wide-alphabet twins (csrc/sw_kernel_pk16.inc built with PK16_WIDE: a match is the equality of two code words instead of a
one-hot bit per letter).  The oracle compares raw bytes, so it is the reference for every alphabet as it stands; every
capability the packed family has is exercised once on a wide pair: parity at every strip height, pruning of global and
local alignments with the window, batches, goal pruning, mixed strip heights, the two-phase best, the overflow rerun,
stage 4, the whole pipeline, and the build with the compiler's wait states left in.

Without the flag (and on a library that does not know it) a pair with 15 or more common byte values ends on the int32
kernels (`sw_strip_kernel<`), unpruned and unbatched: the `_wide<` assertions are what these tests add."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import NEEDLEMAN_WUNSCH, SMITH_WATERMAN, assert_pruned_borders, manager_rows, oracle_kwargs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEEP = os.path.join(ROOT, "masa-cudalign_amd", "libmi355sw_keepnops.so")
THREADS = 16            # oracle threads: a GPU host grants 16 CPUs per command, os.cpu_count() reports the whole machine
F_WIDE = 65536          # MI355SW_F_WIDE_ALPHABET (pinned against the header and engine.py by tests/test_wide_alphabet_host.py)

# ACGT first (they are the commonest by construction and get the codes below 4), then N, then whatever fills the alphabet
POOL = b"ACGTN" + bytes(b for b in b"RYKMSWBDHVEFIJLOPQUXZ" b"abcdefghijklmnopqrstuvwxyz" b"0123456789?" )
assert len(POOL) == 63 and len(set(POOL)) == 63 and b"@" not in POOL and b"#" not in POOL
IUPAC = POOL[:15]
assert sorted(IUPAC) == sorted(b"ACGTNRYKMSWBDHV")
ALPHABETS = {"iupac15": IUPAC, "letters20": POOL[:20], "letters40": POOL[:40]}
EDGE = {0: "AT_ANYWHERE", 1: "AT_SEQUENCE_1", 2: "AT_SEQUENCE_2", 3: "AT_SEQUENCE_1_OR_2", 4: "AT_SEQUENCE_1_AND_2"}
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def wide_pair(pkg, m, n, letters, cfg, density=40, ensure=False, foreign=True, n_run=None, clean=None):
    """A related pair over `letters` (ACGT + extras).  seqgen.random_dna, the extra letters written in at about one position
    in `density`, one run of 90 'N', then seqgen.mutate_dna -- so seq1 carries the letters and the pair stays related.
    (mutate_dna knows four letters: it is run on ACGT stand-ins, once for the sequence and once per base-4 digit of the
    letter's index with the stand-in rotated by that digit.  Its substitutions, indels and inversion depend on the seed and
    the length alone, so the runs differ exactly where a letter position ends up, by that digit.)
    ensure: every extra letter written at least once into the stretch both sequences share.  foreign: '@' in seq0 only, '#' in
    seq1 only.  n_run: where the run of 'N' starts (default: the middle).  clean: (a, b), a stretch left without letters -- at one
    letter in 40 next to no chunk of seq1 has 192 plain columns in reach, which is what the table form needs; this is where the
    kernel takes it."""
    sg = pkg.seqgen
    assert letters[:4] == b"ACGT" and b"N" in letters and len(letters) - 4 < 63
    extras = np.frombuffer(letters[4:], dtype=np.uint8)
    length = max(m, n) + n // 8 + 64
    base = sg.random_dna(sg.SEED0 + cfg, length)
    rng = np.random.default_rng(cfg)
    idx = np.zeros(length, dtype=np.int64)               # 0: a plain base, k + 1: extras[k]
    pos = rng.integers(0, length, length // density)
    idx[pos] = 1 + rng.integers(0, len(extras), len(pos))
    common = min(m, n)
    free = np.ones(common - common // 8, dtype=bool)     # where `ensure` may write: not into the run, not into the clean stretch
    if common > 400:
        at = common // 2 if n_run is None else n_run
        idx[at: at + 90] = 1 + letters.index(b"N") - 4
        free[at: at + 90] = False
    if clean is not None:
        idx[clean[0]: clean[1]] = 0
        free[clean[0]: clean[1]] = False
    free = np.nonzero(free)[0]
    if ensure and len(free) >= 4 * len(extras):          # (three copies where there is room: a deletion or a '#' may take one)
        copies = 3 if len(free) >= 12 * len(extras) else 1
        idx[rng.choice(free, copies * len(extras), replace=False)] = 1 + np.tile(np.arange(len(extras)), copies)
    codes = np.searchsorted(_ACGT, base)
    seed = sg.SEED1 + cfg
    plain = sg.mutate_dna(base, seed)
    c1 = np.searchsorted(_ACGT, plain)
    idx1 = np.zeros(len(plain), dtype=np.int64)
    for k in range(3):
        digit = (idx >> (2 * k)) & 3
        if not digit.any():
            continue
        marked = sg.mutate_dna(_ACGT[(codes + digit) % 4], seed)
        assert len(marked) == len(plain)
        idx1 |= ((np.searchsorted(_ACGT, marked) - c1) % 4) << (2 * k)
    s0 = np.where(idx > 0, extras[np.maximum(idx, 1) - 1], base)[:m].astype(np.uint8)
    s1 = np.where(idx1 > 0, extras[np.maximum(idx1, 1) - 1], plain).astype(np.uint8)
    if len(s1) < n:
        s1 = np.concatenate([s1, sg.random_dna(sg.SEED1 + cfg + 77, n - len(s1))])
    s1 = s1[:n]
    if foreign:
        s0[5::211] = ord("@")
        at = np.arange(7, n, 199)
        if clean is not None:
            at = at[(at < clean[0] - 40) | (at >= clean[1] + 40)]
        s1[at] = ord("#")
    return np.ascontiguousarray(s0), np.ascontiguousarray(s1)


def common_letters(s0, s1):
    return len(np.intersect1d(np.unique(s0), np.unique(s1)))


def assert_wide(st, restarts=0):
    assert st["profile_kernel"] == 2 and "_wide<" in st["kernel"] and st["restarts"] == restarts, (st["profile_kernel"], st["kernel"], st["restarts"])


def run_stage1(pkg, al, s0, s1, start=0, end=0, interval=0, prune=False, keep=True):
    al.setSequences(s0, s1)
    part = pkg.Partition(0, 0, len(s0), len(s1))
    mg = pkg.Stage1Manager(part, alignment_start=getattr(pkg, EDGE[start]), alignment_end=getattr(pkg, EDGE[end]),
                           special_row_interval=interval, keep_last_row=keep, keep_last_column=keep, block_pruning=prune)
    al.alignPartition(part, mg)
    return mg, al.getStatistics()


def reference(oracle, s0, s1, start, end, strip_rows, interval=0):
    kw = oracle_kwargs(oracle, dict(start=start, end=end, pruning=False, disk=-1, block=(strip_rows, 1 << 20)), len(s0), len(s1))
    # (the threaded oracle reports a best cell for "anywhere" and "last cell" only: the semi-global forms take the serial one)
    kw.update(want_last_row=True, want_last_col=True, special_row_interval=interval, threads=THREADS if start == end and start in (0, 4) else 0)
    return oracle.stage1(s0, s1, **kw)


def assert_equals_oracle(mg, ref, what=""):
    assert tuple(mg.getBestScore()) == tuple(ref["best"]), (what, mg.getBestScore(), ref["best"])
    assert np.array_equal(mg.lastRow(), ref["last_row"]), what
    assert np.array_equal(mg.lastColumn(), ref["last_col"]), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity at every strip height
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 8, 12, 16, 24, 32])
@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_parity_at_every_height(pkg, oracle, alphabet, R):
    """m = one strip + 70 rows (a full strip and a ragged one), n = 700 (the 128-column window of column codes shifts
    several times; chunks of plain ACGT take the table form, chunks with another letter the equality form): local and
    global, at 512-row strips one semi-global form as well -- best cell, last row and last column are the oracle's"""
    m, n = 64 * R + 70, 700
    s0, s1 = wide_pair(pkg, m, n, ALPHABETS[alphabet], cfg=100 + R, ensure=True, n_run=100, clean=(330, 680))
    assert not np.isin(s1[384:640], np.frombuffer(POOL[4:] + b"#", dtype=np.uint8)).any()      # chunks 6 to 9: plain
    assert common_letters(s0, s1) >= 15
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=F_WIDE)
    try:
        for start, end in [(0, 0), (4, 4)] + ([(1, 3)] if R == 8 else []):
            mg, st = run_stage1(pkg, al, s0, s1, start, end)
            assert_wide(st)
            assert st["strip_rows"] == 64 * R
            assert_equals_oracle(mg, reference(oracle, s0, s1, start, end, 64 * R), (alphabet, R, start, end))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. fuzz
# ---------------------------------------------------------------------------------------------------------------------
def _fuzz_case(k):
    rng = np.random.default_rng(7000 + k)
    m = int(rng.choice([257, 300, 511, 512, 513, 777, 1024, 1500, 2049, 2600, 4097, 6000]))
    n = int(rng.choice([255, 256, 257, 300, 383, 384, 385, 511, 900, 1300, 2500, 6000]))
    K = int(rng.integers(15, 63))
    R = int(rng.choice([0, 4, 8, 12, 16, 24, 32]))
    start, end = [(0, 0), (4, 4)][int(rng.integers(0, 2))]
    track = bool(rng.integers(0, 2))
    return m, n, K, R, start, end, track


@pytest.mark.parametrize("k", range(60))
def test_randomised_differential_against_oracle(pkg, oracle, k):
    """60 seeded cases in the manner of test_gpu_parity.py's fuzz: sizes around lane, chunk and strip edges up to 6000 (from
    255: below that a sequence cannot hold 15 letters next to its bases at one letter in 20), alphabets of 15 to 62 letters,
    every strip height and the engine's own choice, local and global, best cell tracked and not"""
    m, n, K, R, start, end, track = _fuzz_case(k)
    clean = (n - 450, n - 50) if n >= 1300 else None          # (room for the table form in the longer rows)
    s0, s1 = wide_pair(pkg, m, n, POOL[:K], cfg=7000 + k, density=20, ensure=True, n_run=min(m, n) // 8, clean=clean)
    have = common_letters(s0, s1)
    assert 15 <= have <= K, (have, K)        # (a deletion may cost seq1 a rare letter; the '@' / '#' are not common)

    class Quiet(pkg.Stage1Manager):
        def mustDispatchScores(self):
            return track

    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=F_WIDE)
    try:
        al.setSequences(s0, s1)
        part = pkg.Partition(0, 0, m, n)
        mg = Quiet(part, alignment_start=getattr(pkg, EDGE[start]), alignment_end=getattr(pkg, EDGE[end]), keep_last_row=True,
                   keep_last_column=True)
        al.alignPartition(part, mg)
        st = al.getStatistics()
        assert_wide(st)
        ref = reference(oracle, s0, s1, start, end, st["strip_rows"])
        assert np.array_equal(mg.lastRow(), ref["last_row"]) and np.array_equal(mg.lastColumn(), ref["last_col"])
        if track:
            assert tuple(mg.getBestScore()) == tuple(ref["best"])
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the edges of the range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags,kernel", [(14, F_WIDE, "packed"), (15, F_WIDE, "wide"), (62, F_WIDE, "wide"), (63, F_WIDE, "int32"), (15, 0, "int32")])
def test_edges_of_the_range(pkg, oracle, K, flags, kernel):
    """14 common letters with the flag on: today's kernel; 15 and 62: the wide twins; 63, or 15 with the flag off: raw
    bytes on the int32 kernel.  All of them: the oracle's bytes"""
    m, n = 3000, 3500
    s0, s1 = wide_pair(pkg, m, n, POOL[:K], cfg=300 + K, density=10, ensure=True)
    assert common_letters(s0, s1) == K
    al = pkg.MI355Aligner(device=0, flags=flags)
    try:
        mg, st = run_stage1(pkg, al, s0, s1)
        if kernel == "wide":
            assert_wide(st)
        elif kernel == "packed":
            assert st["profile_kernel"] == 2 and "_wide" not in st["kernel"] and "_pk16" in st["kernel"], st["kernel"]
        else:
            assert st["profile_kernel"] == 0 and st["kernel"].startswith("sw_strip_kernel<"), st["kernel"]
        assert st["restarts"] == 0
        assert_equals_oracle(mg, reference(oracle, s0, s1, 0, 0, st["strip_rows"]), (K, flags))
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. overflow rerun
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [False, True], ids=["sw", "nw"])
def test_overflow_rerun_runs_the_int32_kernel_on_the_codes(pkg, oracle, nw):
    """an overflow report of a wide kernel (injected at strip 1): one restart on the int32 byte-compare kernel over the SAME
    coded sequences; last column (its first cells were handed out before the report), last row, special rows and best cell
    are the oracle's, every special row delivered once"""
    m, n = 20000, 3000
    s0, s1 = wide_pair(pkg, m, n, ALPHABETS["letters20"], cfg=401, ensure=True)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_WIDE)
    try:
        edge = 4 if nw else 0
        mg, st = run_stage1(pkg, al, s0, s1, edge, edge, interval=8192)
        assert_wide(st)                                   # (without the fault: the wide kernel, no restart)
        al.configure(fault_overflow_strip_plus1=2)
        mg, st = run_stage1(pkg, al, s0, s1, edge, edge, interval=8192)
    finally:
        al.close()
    assert st["restarts"] == 1 and st["profile_kernel"] == 0 and st["kernel"].startswith("sw_strip_kernel<"), (st["restarts"], st["kernel"])
    ref = reference(oracle, s0, s1, edge, edge, 8192, interval=8192)
    assert_equals_oracle(mg, ref, "rerun")
    want = dict(zip(ref["special_row_ids"], ref["special_rows"]))
    rows = sorted(r for r in mg.special_rows if r < m)
    assert rows == [8192, 16384]
    for r in rows:
        assert len(mg.special_rows[r]) == 2               # the leading cell + the row: ONE delivery
        assert np.array_equal(mg.specialRow(r), want[r]), r


# ---------------------------------------------------------------------------------------------------------------------
# 5. / 6. block pruning of a global and of a local alignment
# ---------------------------------------------------------------------------------------------------------------------
PRUNE_M, PRUNE_N, PRUNE_K = 30000, 26000, 16
_PRUNE = {}


def prune_pair(pkg):
    if "pair" not in _PRUNE:
        _PRUNE["pair"] = wide_pair(pkg, PRUNE_M, PRUNE_N, POOL[:PRUNE_K], cfg=501, ensure=True)
    return _PRUNE["pair"]


def prune_reference(pkg, oracle, edge):
    """the unpruned oracle of the pruning pair per edge type: computed once, shared, left unchanged"""
    if edge not in _PRUNE:
        s0, s1 = prune_pair(pkg)
        ref = reference(oracle, s0, s1, edge, edge, 8192, interval=8192)
        for a in [ref["last_row"], ref["last_col"]] + list(ref["special_rows"]):
            a.setflags(write=False)
        _PRUNE[edge] = ref
    return _PRUNE[edge]


def test_global_pruning(pkg, oracle):
    """30 000 x 26 000 related pair with 16 common letters, gap-initialised borders, 256-row strips: H[m][n] is the unpruned
    oracle's, every border cell handed out is held by helpers.assert_pruned_borders, skipped + computed = m * n -- and the
    wide kernel skips what today's kernel skips on the same pair with its two rarest letters rewritten to N (14 letters):
    at least 0.9 of it (the margin: the few positions where a rewritten letter now matches an N)"""
    m, n = PRUNE_M, PRUNE_N
    s0, s1 = prune_pair(pkg)
    assert common_letters(s0, s1) == PRUNE_K
    ref = prune_reference(pkg, oracle, 4)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_WIDE)
    try:
        mg, st = run_stage1(pkg, al, s0, s1, 4, 4, interval=8192, prune=True)
        assert_wide(st)
        assert st["kernel_launches"] == 1
        assert tuple(mg.getBestScore()) == tuple(ref["best"]) == (m, n, int(ref["last_row"][-1, 0]))
        assert st["pruned_cells"] + st["processed_cells"] == m * n
        assert assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, ref["best"][2], NEEDLEMAN_WUNSCH, col0=True,
                                     must_rows_upto=m, where="wide global") > 0
        # the same pair at 14 letters, on today's kernel
        both = np.concatenate([s0, s1])
        counts = sorted((int((both == b).sum()), b) for b in np.intersect1d(np.unique(s0), np.unique(s1)))
        rare = [b for _, b in counts[:2]]
        t0, t1 = s0.copy(), s1.copy()
        for t in (t0, t1):
            t[np.isin(t, rare)] = ord("N")
        assert common_letters(t0, t1) == 14
        mg14, st14 = run_stage1(pkg, al, t0, t1, 4, 4, interval=8192, prune=True)
        assert st14["profile_kernel"] == 2 and "_wide" not in st14["kernel"] and st14["restarts"] == 0, st14["kernel"]
        print("global 30000 x 26000: wide kernel skipped %d cells, the 14-letter pair on today's kernel %d" % (st["pruned_cells"], st14["pruned_cells"]))
        assert st["pruned_cells"] > 0 and st["pruned_cells"] >= 0.9 * st14["pruned_cells"]
    finally:
        al.close()


def test_local_pruning_with_the_window(pkg, oracle):
    """the same pair, local: the best cell is the oracle's, every cell handed out (special rows, last row, last column) is held
    by helpers.assert_pruned_borders / assert_pruned_cells, and cells were skipped"""
    m, n = PRUNE_M, PRUNE_N
    s0, s1 = prune_pair(pkg)
    ref = prune_reference(pkg, oracle, 0)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_WIDE)
    try:
        mg, st = run_stage1(pkg, al, s0, s1, 0, 0, interval=8192, prune=True)
        assert_wide(st)
        assert st["kernel"].startswith("sw_strip_kernel_pk16_wide<2,"), st["kernel"]
        assert tuple(mg.getBestScore()) == tuple(ref["best"])
        assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == m * n
        assert assert_pruned_borders(manager_rows(mg), mg.lastRow(), mg.lastColumn(), ref, m, n, ref["best"][2], SMITH_WATERMAN, col0=True,
                                     must_rows_upto=ref["best"][0], where="wide local") > 0
    finally:
        al.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch, 8. goal pruning: the many-letter cases of test_gpu_batch_stages.py / test_gpu_goal_prune.py with the flag on
# ---------------------------------------------------------------------------------------------------------------------
def test_many_letters_run_in_the_batch(pkg, oracle):
    """the three partitions of test_many_letters_leave_the_batch_for_single_calls on its 20-letter pair: with the flag they
    run in ONE launch of the wide batch kernel; each equals the oracle and its own single call"""
    from test_gpu_batch_stages import Case, Refs, ENGINE_GRID, _expect_oracle, _expect_same, _run
    rng = np.random.RandomState(12)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    s1 = letters[rng.randint(0, 20, 12000)]
    s0 = s1[:10000].copy()
    mut = rng.rand(10000) < 0.1
    s0[mut] = letters[rng.randint(0, 20, int(mut.sum()))]
    refs = Refs(pkg, oracle, s0, s1)
    cases = [Case(pkg.Partition(0, 0, 10000, 2500), "goal", 8500), Case(pkg.Partition(0, 3000, 9500, 7000), "sw"),
             Case(pkg.Partition(500, 8000, 9999, 12000), "semi", 9300)]
    al = pkg.MI355Aligner(device=0, flags=F_WIDE)
    try:
        al.setSequences(s0, s1)
        singles, batch, st, single_stats = _run(pkg, al, cases, 4)
    finally:
        al.close()
    assert st["kernel"].startswith("sw_batch_kernel_pk16_wide<"), st["kernel"]
    assert st["restarts"] == 0 and st["profile_kernel"] == 2
    for s in single_stats:
        assert_wide(s)
    for k, c in enumerate(cases):
        _expect_oracle(c, batch[k], refs(c, ENGINE_GRID), k)
        _expect_same(c, batch[k], singles[k], k)


def test_many_letters_are_goal_pruned(pkg, oracle):
    """the "many_letters" case of test_gpu_goal_prune.py with the flag on: the goal instantiation of the wide pruning kernel
    skips cells, the goal is where the unpruned run finds it, every last-column cell at or above its bound is exact"""
    from test_gpu_goal_prune import _check_sweep, _manager, _reference
    m, n = 2049, 1601
    rng = np.random.RandomState(12)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    s1 = letters[rng.randint(0, 20, n)]
    s0 = np.concatenate([s1, letters[rng.randint(0, 20, m - n)]])
    mut = rng.rand(m) < 0.1
    s0[mut] = letters[rng.randint(0, 20, int(mut.sum()))]
    s0, s1 = np.ascontiguousarray(s0), np.ascontiguousarray(s1)
    ref = _reference(oracle, s0, s1, 256, 8192)
    bound = int(ref["last_col"][:, 0].max()) - 200
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_WIDE)
    try:
        al.setSequences(s0, s1)
        part = pkg.Partition(0, 0, m, n)
        plain = _manager(pkg, part, 8192)
        al.alignPartition(part, plain)
        st0 = al.getStatistics()
        mg = _manager(pkg, part, 8192)
        al.setGoalBounds([bound])
        al.alignPartition(part, mg)
        st = al.getStatistics()
    finally:
        al.close()
    assert_wide(st0)
    assert st0["pruned_cells"] == 0 and np.array_equal(plain.lastColumn(), ref["last_col"]) and np.array_equal(plain.lastRow(), ref["last_row"])
    assert st["kernel"] == "sw_strip_kernel_pk16_wide<2,false,false,true,true>", st["kernel"]
    assert st["restarts"] == 0 and st["kernel_launches"] == 1
    assert st["pruned_cells"] > 0 and st["pruned_cells"] + st["processed_cells"] == m * n
    _check_sweep(mg, ref, m, n, bound, "wide goal sweep")      # (last column: every cell with H >= bound exact)
    goal = int(np.argmax(plain.lastColumn()[:, 0]))
    assert int(np.argmax(mg.lastColumn()[:, 0])) == goal and mg.lastColumn()[goal, 0] == plain.lastColumn()[goal, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 9. mixed strip heights, the two-phase best
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_heights(pkg, oracle):
    """the (21 300 x 12 000, 8 wavefronts) shape of test_gpu_mixed.py with 15 common letters: the mixed wide kernel"""
    m, n = 21300, 12000
    s0, s1 = wide_pair(pkg, m, n, IUPAC, cfg=601, ensure=True)
    ref = oracle.stage1(s0, s1, want_last_row=True, threads=THREADS)
    al = pkg.MI355Aligner(device=0, waves=8, flags=F_WIDE)
    try:
        al.setSequences(s0, s1)
        al.streamBegin(pkg.Partition(0, 0, m, n), want_last_row=True)
        while not al.streamPoll()[1]:
            pass
        row = al.streamReadLastRow()
        best, _ = al.streamEnd()
        st = al.getStatistics()
    finally:
        al.close()
    assert st["kernel"] == "sw_strip_kernel_pk16_mixed_wide<12,11,true,true>", st["kernel"]
    assert_wide(st)
    assert st["strips"] % 8 == 0 and st["strip_rows"] == 1536 and st["strip_rows_second"] == 1408
    assert tuple(best) == (ref["best"][0] - 1, ref["best"][1] - 1, ref["best"][2])
    assert np.array_equal(row, ref["last_row"][1:])


def test_two_phase_best(pkg, oracle):
    """value-only main pass + exact pass of the winning strip (MI355SW_F_TWO_PHASE): two launches, the canonical cell"""
    m, n = 9000, 7000
    s0, s1 = wide_pair(pkg, m, n, IUPAC, cfg=602, ensure=True)
    al = pkg.MI355Aligner(device=0, rows_per_lane=4, flags=F_WIDE | pkg.engine.F_TWO_PHASE)
    try:
        mg, st = run_stage1(pkg, al, s0, s1, keep=False)
    finally:
        al.close()
    assert_wide(st)
    assert st["kernel_launches"] == 2
    assert tuple(mg.getBestScore()) == tuple(oracle.stage1(s0, s1, threads=THREADS)["best"])


# ---------------------------------------------------------------------------------------------------------------------
# 10. stage 4 and the pipeline
# ---------------------------------------------------------------------------------------------------------------------
def test_stage4_on_wide_codes(pkg, oracle):
    """test_gpu_stage4.py::test_coded_and_raw_sequences' 15-letter case: the refinement runs on the coded sequences and leaves
    the crosspoints it leaves on the raw bytes (flag off) -- the oracle's"""
    from test_gpu_stage4 import _global_endpoints
    letters = b"ACGTNRYKMSWBDHV"
    rng = np.random.default_rng(len(letters))
    alpha = np.frombuffer(letters, dtype=np.uint8)
    s0 = alpha[rng.integers(0, 4, 3000)].copy()
    s1 = s0.copy()
    for s in (s0, s1):
        idx = rng.integers(0, len(s), 150)
        s[idx] = alpha[rng.integers(0, len(alpha), len(idx))]
    s1 = np.concatenate([s1[:1000], s1[1040:]])
    assert common_letters(s0, s1) == 15
    cp = _global_endpoints(oracle, s0, s1)
    want = oracle.stage4(s0, s1, cp, 16)[0]
    got = {}
    for flags in (F_WIDE, 0):
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            mg, st = run_stage1(pkg, al, s0, s1, keep=False)     # (which sequences the handle holds: coded wide / raw)
            assert ("_wide<" in st["kernel"]) == (flags != 0) and st["profile_kernel"] == (2 if flags else 0)
            got[flags] = al.stage4(cp, 16)[0]
        finally:
            al.close()
    assert got[F_WIDE] == got[0] == want


def test_pipeline_leaves_the_same_files(pkg, tmp_path):
    """all six stages on a 40 000 x 36 000 pair with 16 common letters, flag on and flag off: alignment.00.txt and the crosspoint
    files of stages 2, 3 and 4 are byte-identical"""
    from masa_cudalign_amd import fasta, pipeline
    m, n = 40000, 36000
    s0, s1 = wide_pair(pkg, m, n, POOL[:16], cfg=701, ensure=True, foreign=False)
    assert common_letters(s0, s1) == 16
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    files = {}
    for name, flags in (("on", F_WIDE), ("off", 0)):
        work = str(tmp_path / name)
        os.makedirs(work)
        al = pkg.MI355Aligner(device=0, flags=flags)
        try:
            out = pipeline.align(al, q0, q1, work, sra_limit=4 * 1024 * 1024, block_pruning=True)
        finally:
            al.close()
        assert out["best"][2] > 10000
        found = {}
        for root, _, fns in os.walk(work):
            for fn in fns:
                if fn in ("alignment.00.txt", "crosspoint_02.00", "crosspoint_03.00", "crosspoint_04.00"):
                    found[fn] = open(os.path.join(root, fn), "rb").read()
        assert sorted(found) == ["alignment.00.txt", "crosspoint_02.00", "crosspoint_03.00", "crosspoint_04.00"], sorted(found)
        files[name] = (found, tuple(out["best"]))
    assert files["on"][1] == files["off"][1]
    for fn in files["on"][0]:
        assert files["on"][0][fn] == files["off"][0][fn], fn
    assert len(files["on"][0]["alignment.00.txt"]) > 30000


# ---------------------------------------------------------------------------------------------------------------------
# 11. both builds: the library as shipped and the one with the compiler's wait states left in
# ---------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
import __graft_entry__ as graft
import test_gpu_wide_alphabet as T
pkg = graft.load_package()
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()
out = {"library": pkg.engine.LIB_PATH, "build_id": pkg.engine.library_build_id(), "cases": []}
def one(s0, s1, R, edge, prune, interval, flags):
    al = pkg.MI355Aligner(device=0, rows_per_lane=R, flags=flags)
    try:
        mg, st = T.run_stage1(pkg, al, s0, s1, edge, edge, interval=interval, prune=prune)
        out["cases"].append({"best": list(mg.getBestScore()), "kernel": st["kernel"], "restarts": st["restarts"],
                             "pruned_cells": st["pruned_cells"], "last_row": sha(mg.lastRow()), "last_col": sha(mg.lastColumn()),
                             "special": {str(i): sha(mg.specialRow(i)) for i in sorted(mg.special_rows)}})
    finally:
        al.close()
# one case of the parity test: 1024-row strips + 70 rows, local and global
s0, s1 = T.wide_pair(pkg, 64 * 16 + 70, 700, T.IUPAC, cfg=116, ensure=True)
one(s0, s1, 16, 0, False, 0, T.F_WIDE)
one(s0, s1, 16, 4, False, 0, T.F_WIDE)
# the global pruning case; reproducible pruning, so that which slabs go -- and with it every byte handed out -- is a function
# of the input and the two builds can be compared output by output
s0, s1 = T.prune_pair(pkg)
one(s0, s1, 4, 4, True, 8192, T.F_WIDE | pkg.engine.F_DETERMINISTIC_PRUNE)
print(json.dumps(out))
"""


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["MI355SW_LIB"] = lib
    else:
        env.pop("MI355SW_LIB", None)
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "here": HERE}], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])


def test_both_builds_agree_on_wide_pairs():
    """tests/test_gpu_nops.py for the wide kernels (their v_pk_min_u16 -> v_pk_sub_i16 -> v_pk_add_u16 chain is one of the
    pairs csrc/strip_pk_nops.py takes the wait state out of): each build in a child process of its own, every output equal"""
    if not os.path.exists(KEEP):
        pytest.fail("libmi355sw_keepnops.so is not built (make -C masa-cudalign_amd/csrc keepnops; __graft_entry__.build() does it)")
    a, b = _child(None), _child(KEEP)
    assert a["library"] != b["library"] and b["library"] == KEEP
    assert a["build_id"] == b["build_id"]
    assert len(a["cases"]) == len(b["cases"]) == 3
    assert a["cases"][2]["pruned_cells"] > 0 and b["cases"][2]["pruned_cells"] > 0
    for x, y in zip(a["cases"], b["cases"]):
        # (the skipped-cell count of a pruned run is bookkeeping that may differ by a few slabs from run to run, of one library
        #  as well -- tests/test_gpu_det_prune.py allows it 1e-5 of the matrix, less than one slab here; every byte handed out
        #  must be equal)
        x.pop("pruned_cells"), y.pop("pruned_cells")
        assert x == y, (x, y)
        assert "_wide<" in x["kernel"] and x["restarts"] == 0
    assert a["cases"][2]["best"][:2] == [PRUNE_M, PRUNE_N]
