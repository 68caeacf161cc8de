"""GPU (-m gpu): stage 4 (csrc/stage4.hip: mm_half_kernel, mm_match_kernel, s4_make_comparable, stage4_refine) at its
structural edges, through MI355Aligner.stage4 against the oracle's restatement of sw_stage4.cpp.  Every check is exact:
lists of integers equal the oracle's.

The inputs are those of tests/stage4_edge_cases.py; tests/test_stage4_edge_inputs.py (CPU) holds them to what they claim to
cover -- rows and columns on every pass / lane / chunk edge, every oriented corner type on both sides at more than 256 rows
(row_open = 0 among them), winners beyond the first and second ballot, the extreme columns -- and pins the oracle to the
reference on the two new input classes.

  1. letters that occur in one sequence only, in every coding form
  2. the geometry ladder (+ the gapped pairs)      3. the same ladder on low-complexity sequences
  4. errors and degenerate lists, each compared with what the oracle does"""
import os

import numpy as np
import pytest

import stage4_edge_cases as E
from test_gpu_stage4 import _global_endpoints

pytestmark = pytest.mark.gpu

F_WIDE = 65536                       # MI355SW_F_WIDE_ALPHABET
F_FORCE_GENERIC_COMPARE = 1          # MI355SW_F_FORCE_GENERIC_COMPARE


def _oracle_stage4(oracle, s0, s1, cp, limit):
    """(list, steps) or the oracle's negative return code"""
    try:
        return oracle.stage4(s0, s1, cp, limit)
    except RuntimeError as e:
        assert "oc_stage4 failed" in str(e)
        return int(str(e).rsplit(" ", 1)[1])


def _same(got, want, given, limit):
    got = [tuple(p) for p in got]
    want = [tuple(p) for p in want]
    assert got == want, E.first_difference(got, want, given, limit)


# ---------------------------------------------------------------------------------------------------------------------
# 1. foreign bytes
# ---------------------------------------------------------------------------------------------------------------------
FORMS = [(4, 0, 1, "profile"), (7, 0, 1, "profile"), (8, 0, 1, "one-hot"), (14, 0, 1, "one-hot"), (15, 0, 0, "raw"),
         (15, F_WIDE, 2, "wide"), (40, F_WIDE, 2, "wide"), (5, F_FORCE_GENERIC_COMPARE, 0, "generic")]


@pytest.mark.parametrize("n_common,flags,form,name", FORMS, ids=["%d-%s" % (f[0], f[3]) for f in FORMS])
def test_foreign_bytes_in_every_coding_form(pkg, oracle, n_common, flags, form, name):
    """A 3000 x 2960 pair with two different bytes that occur in seq0 only and two that occur in seq1 only, at aligned
    positions (mismatches of the true alignment) and on both sides of the gap: the reference compares raw bytes, so a byte
    of one sequence only never equals anything.  With at most 7 common letters both sequences carry the code 7 for such
    bytes (mi355sw_sequence_codes: the int32 nibble-profile kernel's convention); a stage 4 that compares the codes scores
    '@' against '#' as a match, finds column sums above the partition's score difference and ends with ETRACEBACK -- the
    two profile cases (4 and 7 common letters) fail that way on the commit before s4_make_comparable learnt the number of
    matching codes; the other forms have two different foreign codes and passed before."""
    s0, s1 = E.foreign_pair(pkg.seqgen, n_common)
    _, _, k, f = pkg.engine.sequence_codes(s0, s1, flags)
    assert (k, f) == (n_common, form)
    cp = _global_endpoints(oracle, s0, s1)
    al = pkg.MI355Aligner(device=0, flags=flags)
    try:
        al.setSequences(s0, s1)
        for limit in (16, 1):
            want, steps = oracle.stage4(s0, s1, cp, limit)
            got, st = al.stage4(cp, limit)
            _same(got, want, cp, limit)
            assert st["steps"] == steps
    finally:
        al.close()


def test_pipeline_on_foreign_letters(pkg, oracle, tmp_path):
    """all six stages on a pair with 7 common letters (A C G T N R Y), K and M in seq0 only, S and W in seq1 only: stage 4 is
    handed stage 3's list and leaves what the oracle's stage 4 leaves; alignment.00.txt is the text stages 5 and 6 make of the
    oracle's list.  (Before the fix: stages 1-3 succeed and stage 4 ends the pipeline with ETRACEBACK.)"""
    from masa_cudalign_amd import fasta, pipeline, stage56
    from masa_cudalign_amd.crosspoints import CrosspointsFile, crosspoint_file
    s0, s1 = E.foreign_pair(pkg.seqgen, 7, only0=b"KM", only1=b"SW")
    assert pkg.engine.sequence_codes(s0, s1, 0)[2:] == (7, 1)
    q0, q1 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n"), fasta.parse(b">s1\n" + s1.tobytes() + b"\n")
    work = str(tmp_path / "work")
    os.makedirs(work)
    al = pkg.MI355Aligner(device=0)
    try:
        out = pipeline.align(al, q0, q1, work, sra_limit=500 * 1024)
    finally:
        al.close()
    cp3 = CrosspointsFile(crosspoint_file(work, 3)).load().tuples()
    cp4 = CrosspointsFile(crosspoint_file(work, 4)).load().tuples()
    want, _ = oracle.stage4(s0, s1, cp3, 16)
    _same(cp4, want, cp3, 16)
    assert cp4[0][1] < 60 and cp4[-1][1] > 2800            # the alignment runs over the foreign letters
    text = stage56.stage6_text(stage56.stage5(q0, q1, want), q0, q1)
    assert out["text"] == text and open(os.path.join(work, "alignment.00.txt"), "rb").read() == text


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the ladders
# ---------------------------------------------------------------------------------------------------------------------
def _walk_ladder(pkg, oracle, s0, s1, cp, key):
    rungs = E.ladder(oracle, s0, s1, cp, key=key)
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        for limit, given, want, steps in rungs:
            got, st = al.stage4(np.array(given, dtype=np.int32), limit, as_array=True)
            if not np.array_equal(got, np.array(want, dtype=np.int32)):
                pytest.fail(E.first_difference(got.tolist(), want, given, limit))
            assert st["steps"] == steps, (limit, st["steps"], steps)
        # uninterrupted, from the first list to the last: every error would cascade here, and the steps are the oracle's
        want, steps = E.cached(("whole", key), lambda: oracle.stage4(s0, s1, cp, 1))
        got, st = al.stage4(cp, 1)
        _same(got, want, cp, 1)
        assert st["steps"] == steps and want == list(rungs[-1][2])
    finally:
        al.close()


def test_geometry_ladder(pkg, oracle):
    """geometry() + gapped() as one list of 666 independent partitions, down the limits 2000 .. 1: at every rung the engine is
    handed the ORACLE's list of the rung before (one error does not cascade) and leaves the oracle's list in the oracle's
    number of steps.  A mismatch names the first differing partition."""
    s0, s1, cp = E.geometry_and_gapped(pkg.seqgen, oracle)
    _walk_ladder(pkg, oracle, s0, s1, cp, "geometry+gapped")


def test_low_complexity_ladder(pkg, oracle):
    """A^m / A^n, (AC)^m / (AC)^n, (ACG)^m / (CGA)^n, A^m / C^n, (AACAG)^m / (AACAGT)^n and a substituted, deleted (ACGT)^900:
    nearly every column ties, so the order of mm_match_kernel's candidates decides -- from the middle outwards, forward side
    first, aligned before gapped, 64 per ballot, an "Error Match" before a later match"""
    s0, s1, cp = E.low_complexity(oracle)
    _walk_ladder(pkg, oracle, s0, s1, cp, "low_complexity")


# ---------------------------------------------------------------------------------------------------------------------
# 4. errors and degenerate lists
# ---------------------------------------------------------------------------------------------------------------------
def _expect_like_oracle(pkg, oracle, al, s0, s1, cp, limit):
    """ETRACEBACK exactly when oc_stage4 returns -3 or -4, ETOOLARGE exactly when it returns -2, its list otherwise"""
    want = _oracle_stage4(oracle, s0, s1, cp, limit)
    if isinstance(want, int):
        assert want in (-2, -3, -4), want
        with pytest.raises(pkg.AlignerError, match="ETOOLARGE" if want == -2 else "ETRACEBACK"):
            al.stage4(cp, limit)
    else:
        got, st = al.stage4(cp, limit)
        _same(got, want[0], cp, limit)
        assert st["steps"] == want[1]
    return want


def test_a_score_lowered_by_7(pkg, oracle, aligner):
    """tests/test_gpu_stage4.py raises the end score by 7 (no column reaches it: -3); lowered by 7 some column's scores EXCEED
    the difference (-4, "Error Match") unless an earlier candidate happens to add up to it.  Whatever the oracle does with the
    list -- at the first split, or further down a partly refined list -- the engine does, and the handle is fine afterwards"""
    s0, s1 = pkg.seqgen.related_pair(900, 800, cfg=77)
    cp = _global_endpoints(oracle, s0, s1)
    partly, _ = oracle.stage4(s0, s1, cp, 200)
    assert len(partly) > 3
    lowered = [cp[0], (0, cp[1][1], cp[1][2], cp[1][3] - 7)]
    deep = partly[:-1] + [(partly[-1][0], partly[-1][1], partly[-1][2], partly[-1][3] - 7)]
    aligner.setSequences(s0, s1)
    try:
        seen = []
        for bad in (lowered, deep):
            for limit in (16, 1):
                seen.append(_expect_like_oracle(pkg, oracle, aligner, s0, s1, bad, limit))
                _expect_like_oracle(pkg, oracle, aligner, s0, s1, cp, 16)          # the same handle, a valid list
        assert any(isinstance(w, int) and w in (-3, -4) for w in seen), seen    # (the error path did run)
    finally:
        aligner.unsetSequences()


@pytest.mark.parametrize("m,n", [(131072, 131072), (262142, 20)])
def test_partitions_beyond_the_reference_s_limit(pkg, oracle, aligner, m, n):
    """lenB >= 131072, and lenA / 2 + 1 >= 131072: ETOOLARGE like the oracle's -2 (the reference falls back to another
    strategy there, which neither restates), decided on the host before any half is launched; then a valid list"""
    s0, s1 = pkg.seqgen.random_dna(31, m), pkg.seqgen.random_dna(32, n)
    big = [(0, 0, 0, 0), (0, m, n, 0)]
    assert _oracle_stage4(oracle, s0, s1, big, 16) == -2
    k = min(m, n, 600)
    ok = [(0, 0, 0, 0), (0, k, k, E.nw_score(oracle, s0[:k], s1[:k]))]
    aligner.setSequences(s0, s1)
    try:
        assert _expect_like_oracle(pkg, oracle, aligner, s0, s1, big, 16) == -2
        assert not isinstance(_expect_like_oracle(pkg, oracle, aligner, s0, s1, ok, 4), int)
    finally:
        aligner.unsetSequences()


def test_lists_with_nothing_to_refine(pkg, oracle, aligner):
    """returned unchanged with steps == 0: a list of one point, two identical consecutive points, a list already within the
    limit.  A zero-sided partition of 5000 (di == 0, and dj == 0) between normal ones is left alone while its neighbours are
    refined -- and alone it is nothing to refine either"""
    sg = pkg.seqgen
    a1, b1 = sg.related_pair(300, 290, cfg=41)
    a2, b2 = sg.related_pair(280, 300, cfg=42)
    a3, b3 = sg.related_pair(310, 305, cfg=43)
    only0, only1 = sg.random_dna(44, 5000), sg.random_dna(45, 5000)
    s0 = np.concatenate([a1, only0, a2, a3])
    s1 = np.concatenate([b1, b2, only1, b3])
    gap = -(3 + 2 * 5000)
    cp, i, j, sc = [(0, 0, 0, 0)], 0, 0, 0
    for da, db in ((a1, b1), (only0, None), (a2, b2), (None, only1), (a3, b3)):
        i += 0 if da is None else len(da)
        j += 0 if db is None else len(db)
        sc += gap if da is None or db is None else E.nw_score(oracle, da, db)
        cp.append((0, i, j, sc))
    aligner.setSequences(s0, s1)
    try:
        for unchanged, limit in (([cp[1]], 16), ([cp[1], cp[1]], 16), ([cp[0], cp[1]], 300), ([cp[1], cp[2]], 16), ([cp[3], cp[4]], 16)):
            want, steps = oracle.stage4(s0, s1, unchanged, limit)
            got, st = aligner.stage4(unchanged, limit)
            assert got == want == [tuple(p) for p in unchanged] and st["steps"] == steps == 0 and st["partitions"] == 0, (unchanged, limit)
        for limit in (16, 1):
            want, steps = oracle.stage4(s0, s1, cp, limit)
            got, st = aligner.stage4(cp, limit)
            _same(got, want, cp, limit)
            assert st["steps"] == steps > 0
            for z in (cp[1:3], cp[3:5]):                       # the zero-sided partitions: still one piece
                k = got.index(z[0])
                assert got[k + 1] == z[1]
            assert len(got) > len(cp) + 30
    finally:
        aligner.unsetSequences()
