"""CPU: how a pair of sequences is coded for the kernels (mi355sw_sequence_codes, the rule mi355sw_set_sequences applies) with
and without MI355SW_F_WIDE_ALPHABET, and the flag's way through the fronts."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft

# 63 printable bytes; which four are the commonest is decided by the counts pair_with gives them, not by their order here
LETTERS = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz?", dtype=np.uint8)


def pair_with(k, extra0=b"@", extra1=b"#"):
    """two sequences with exactly k byte values in common.  Counts: the letters 'T', 'G', 'C', 'A' (in this order) are the four
    commonest, with distinct totals; every other common letter appears three times in all (a tie over the whole rest); extra0 /
    extra1 appear in one sequence only."""
    assert 4 <= k <= len(LETTERS)
    top = [ord(c) for c in "TGCA"]
    rest = [int(b) for b in LETTERS if int(b) not in top][:k - 4]
    s0, s1 = [], []
    for rank, b in enumerate(top):
        s0 += [b] * (40 - 5 * rank)
        s1 += [b] * (30 - 3 * rank)
    for b in rest:
        s0 += [b, b]
        s1 += [b]
    s0 += list(extra0)
    s1 += list(extra1)
    rng = np.random.default_rng(k)
    s0, s1 = np.array(s0, dtype=np.uint8), np.array(s1, dtype=np.uint8)
    rng.shuffle(s0)
    rng.shuffle(s1)
    return s0, s1, top, sorted(rest)


def expected_tables(top, rest, foreign0, foreign1):
    lut0, lut1 = np.full(256, foreign0, dtype=np.uint8), np.full(256, foreign1, dtype=np.uint8)
    for code, b in enumerate(top + rest):       # by frequency; the tie among `rest` keeps byte order (stable sort)
        lut0[b] = lut1[b] = code
    return lut0, lut1


@pytest.mark.parametrize("k", [5, 14, 15, 20])
def test_flag_off_codes_as_before(pkg, k):
    s0, s1, top, rest = pair_with(k)
    lut0, lut1, common, form = pkg.engine.sequence_codes(s0, s1, 0)
    assert common == k
    if k <= 14:
        assert form == 1
        want0, want1 = expected_tables(top, rest, 7 if k <= 7 else 14, 7 if k <= 7 else 15)
        assert np.array_equal(lut0, want0) and np.array_equal(lut1, want1)
    else:
        assert form == 0
        assert np.array_equal(lut0, np.arange(256)) and np.array_equal(lut1, np.arange(256))


@pytest.mark.parametrize("k", [15, 20, 62])
def test_flag_on_codes_wide(pkg, k):
    eng = pkg.engine
    s0, s1, top, rest = pair_with(k)
    lut0, lut1, common, form = eng.sequence_codes(s0, s1, eng.F_WIDE_ALPHABET)
    assert (common, form) == (k, 2)
    assert [int(lut0[b]) for b in top] == [0, 1, 2, 3]
    want0, want1 = expected_tables(top, rest, k, k + 1)
    assert np.array_equal(lut0, want0) and np.array_equal(lut1, want1)
    for b in top + rest:
        assert lut0[b] == lut1[b] < k
    assert lut0[ord("@")] == k and lut1[ord("#")] == k + 1
    assert int(lut1.max()) * 4 <= 255            # seq1 is stored as code * 4 in a byte


def test_the_flag_leaves_up_to_14_letters_alone(pkg):
    eng = pkg.engine
    for k in (5, 14):
        s0, s1, _, _ = pair_with(k)
        off, on = eng.sequence_codes(s0, s1, 0), eng.sequence_codes(s0, s1, eng.F_WIDE_ALPHABET)
        assert on[2:] == off[2:] == (k, 1)
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])


def test_63_letters_and_the_generic_compare_stay_raw(pkg):
    eng = pkg.engine
    s0, s1, _, _ = pair_with(63)
    lut0, lut1, common, form = eng.sequence_codes(s0, s1, eng.F_WIDE_ALPHABET)
    assert (common, form) == (63, 0)
    assert np.array_equal(lut0, np.arange(256)) and np.array_equal(lut1, np.arange(256))
    s0, s1, _, _ = pair_with(20)
    assert eng.sequence_codes(s0, s1, eng.F_WIDE_ALPHABET | eng.F_FORCE_GENERIC_COMPARE)[2:] == (20, 0)
    assert eng.sequence_codes(s0, s1, eng.F_WIDE_ALPHABET | eng.F_FORCE_INT32)[2:] == (20, 2)     # int32 kernel, on the codes
    s0, s1, _, _ = pair_with(5)
    assert eng.sequence_codes(s0, s1, eng.F_FORCE_GENERIC_COMPARE)[2:] == (5, 0)


def test_empty_sequences_and_bad_arguments(pkg):
    eng = pkg.engine
    empty = np.zeros(0, dtype=np.uint8)
    assert eng.sequence_codes(empty, empty, eng.F_WIDE_ALPHABET)[2:] == (0, 1)
    lib = pkg.load_library()
    k, form = ctypes.c_int32(), ctypes.c_int32()
    lut = (ctypes.c_uint8 * 256)()
    assert lib.mi355sw_sequence_codes(None, 3, None, 0, 0, lut, lut, ctypes.byref(k), ctypes.byref(form)) == -1
    assert lib.mi355sw_sequence_codes(None, 0, None, 0, 0, None, lut, ctypes.byref(k), ctypes.byref(form)) == -1


def test_the_flag_in_the_header_and_the_fronts(pkg, monkeypatch):
    eng = pkg.engine
    hdr = open(os.path.join(graft.ROOT, "include", "mi355sw.h")).read()
    m = re.search(r"#define\s+MI355SW_F_WIDE_ALPHABET\s+(\d+)", hdr)
    assert m and int(m.group(1)) == eng.F_WIDE_ALPHABET == 65536
    bits = [int(v) for v in re.findall(r"#define\s+MI355SW_F_[A-Z0-9_]+\s+(\d+)", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)      # one bit each, none shared
    assert "mi355sw_sequence_codes" in eng.ABI_SYMBOLS
    lib = pkg.load_library()
    assert hasattr(lib, "mi355sw_sequence_codes") and lib.mi355sw_sequence_codes.argtypes is not None
    for name in list(eng._ENV_FLAGS):
        monkeypatch.delenv(name, raising=False)
    assert eng.env_switches()[0] == 0
    monkeypatch.setenv("MI355SW_WIDE_ALPHABET", "1")
    assert eng.env_switches()[0] == eng.F_WIDE_ALPHABET
    # the command-line fronts
    src = open(os.path.join(graft.PKG_DIR, "host", "Mi355AlignerParameters.cpp")).read()
    assert '"wide-alphabet"' in src
    assert "MI355SW_F_WIDE_ALPHABET" in open(os.path.join(graft.PKG_DIR, "host", "Mi355Aligner.cpp")).read()
    assert "--wide-alphabet" in open(os.path.join(graft.ROOT, "tools", "align_fasta.py")).read()
