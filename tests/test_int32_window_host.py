"""CPU: MI355SW_F_INT32_WINDOW (the pruning window of the int32 kernel family, opt-in) in the header, in engine.py, behind its
environment switch and in tools/align_fasta.py; what the header says about it; and the census of tests/int32_window_cases.py,
which says why the GPU file may demand that half of the retire pair's matrix is skipped.  What the flag does is
tests/test_gpu_int32_window.py's."""
import os
import re
import subprocess
import sys

import __graft_entry__ as graft
import int32_window_cases as cases
from helpers import oracle_full


def _read(*path):
    return open(os.path.join(*path), errors="replace").read()


def test_the_flags_value_in_the_header_and_in_the_engine(pkg):
    eng = pkg.engine
    hdr = _read(graft.ROOT, "include", "mi355sw.h")
    m = re.search(r"#define\s+MI355SW_F_INT32_WINDOW\s+(\d+)", hdr)
    assert m and int(m.group(1)) == eng.F_INT32_WINDOW == 524288
    bits = [int(v) for v in re.findall(r"#define\s+MI355SW_F_[A-Z0-9_]+\s+(\d+)", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)      # one bit each, none shared
    assert max(bits) == 524288                                                       # the next free bit
    assert re.search(r"#define\s+MI355SW_ABI_VERSION\s+8\b", hdr)                    # additive: the ABI version stays
    assert eng.F_INT32_WINDOW not in (eng.F_INT32_PRUNE_GLOBAL, eng.F_INT32_PRUNE_EDGE_GOAL, eng.F_NO_WINDOW)


def test_the_header_says_what_is_served_and_what_is_not():
    hdr = _read(graft.ROOT, "include", "mi355sw.h")
    text = hdr[hdr.index("#define MI355SW_F_INT32_WINDOW"):hdr.index("#define MI355SW_F_NO_HOST_COUNTER")]
    for word in ("off by default", "additive in ABI 8", "MI355SW_F_INT32_PRUNE_GLOBAL", "MI355SW_F_INT32_PRUNE_EDGE_GOAL", "MI355SW_F_NO_WINDOW",
                 "MI355SW_F_DETERMINISTIC_PRUNE", "block_score_columns", "batch", "MI355SW_EOVERFLOW16", "RETIRES", "pruned_cells",
                 "mi355sw_stats.kernel", "No gap words", "no mid-strip stop"):
        assert word in text, word
    # the two older flags no longer say that this family has no window: they point here
    older = hdr[hdr.index("#define MI355SW_F_INT32_PRUNE_GLOBAL"):hdr.index("#define MI355SW_F_INT32_WINDOW")]
    assert "No pruning window" not in older and older.count("MI355SW_F_INT32_WINDOW") == 2


def test_the_environment_switch(pkg, monkeypatch):
    eng = pkg.engine
    assert eng._ENV_FLAGS["MI355SW_INT32_WINDOW"] == eng.F_INT32_WINDOW
    for name in list(eng._ENV_FLAGS):
        monkeypatch.delenv(name, raising=False)
    assert eng.env_switches()[0] == 0                     # off by default
    monkeypatch.setenv("MI355SW_INT32_WINDOW", "1")
    assert eng.env_switches()[0] == eng.F_INT32_WINDOW


def test_align_fasta_parses_the_option(tmp_path):
    """the option is taken like its neighbours: with it and no input files the tool ends at its usage text, not at "unknown option"
    (no engine is made before the files are read)"""
    tool = os.path.join(graft.ROOT, "tools", "align_fasta.py")
    text = _read(tool)
    assert "--int32-window" in text and "F_INT32_WINDOW" in text
    runs = {}
    for opt in ("--int32-window", "--int32-prune-global", "--no-such-option"):
        p = subprocess.run([sys.executable, tool, opt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
        runs[opt] = (p.returncode, p.stdout.decode(errors="replace"))
    assert runs["--int32-window"] == runs["--int32-prune-global"], runs
    assert runs["--no-such-option"] != runs["--int32-window"], runs


def test_the_runtime_and_the_kernel_select_it_by_the_flag_and_by_a_template_parameter():
    csrc = os.path.join(graft.PKG_DIR, "csrc")
    rt = _read(csrc, "runtime.cpp")
    assert "flag(h, MI355SW_F_INT32_WINDOW)" in rt and "windowed32" in rt
    kern = _read(csrc, "sw_kernel.hip")
    assert kern.count("bool EDGE = false, bool WINDOW = false>") == 2           # process_strip and sw_strip_kernel, the last parameter
    assert 'static_assert(!WINDOW || PRUNE' in kern
    # both families read the progress word the same way: the define lives in the shared header, once
    assert "#define WIN_RETIRED 0x40000000" in _read(csrc, "sw_kernel.h")
    assert "#define WIN_RETIRED" not in _read(csrc, "sw_kernel_pk16.inc") and "#define WIN_RETIRED" not in kern
    # the adapter under host/ gets nothing
    for name in os.listdir(os.path.join(graft.PKG_DIR, "host")):
        assert "INT32_WINDOW" not in _read(graft.PKG_DIR, "host", name), name


def test_kernel_names_spell_out_all_eight_arguments():
    for rule in cases.RULES:
        for R in cases.HEIGHTS:
            for prof in (False, True):
                k = cases.kernel_name(R, rule, prof)
                assert k.count(",") == 7 and k.endswith(",true>") and k.startswith("sw_strip_kernel<%d," % R), k
                assert cases.walking_name(R, rule, prof) != k
    assert len({cases.kernel_name(R, rule, p) for rule in ("local", "last_cell", 3, "goal") for R in cases.HEIGHTS for p in (False, True)}) == 24


def test_the_retire_pair_and_its_census(pkg, oracle):
    """the oracle's best cell, the quiet rows below the alignment, and how much the local rule may skip in the strips below it:
    161 of 192 strips, 24 192 eligible slabs; the ceiling of what those strips alone may skip is well above the half of the
    matrix that the GPU file demands"""
    m, n = cases.RETIRE_M, cases.RETIRE_N
    s0, s1, flags = cases.retire_pair(pkg)
    assert (len(s0), len(s1), flags) == (m, n, cases.F_FORCE_INT32)
    ref = oracle_full(oracle, s0, s1, special_row_interval=cases.RETIRE_SH, block_h=cases.RETIRE_SH)
    assert tuple(ref["best"]) == cases.RETIRE_BEST == (7682, 7680, 6959)
    rows = dict(zip(ref["special_row_ids"], ref["special_rows"]))
    for i in rows:
        if i >= cases.RETIRE_QUIET_FROM and i % 8192 == 0:
            assert int(rows[i][:, 0].max()) <= cases.RETIRE_QUIET_H == 8, i
    below, strips, skippable, eligible = cases.retire_census(rows, ref["best"], m, n)
    print("%d of %d strips lie below the alignment; of %d eligible slabs those strips alone may skip %d (%.3f)" % (
        below, strips, eligible, skippable, skippable / float(eligible)))
    assert (below, strips, eligible) == (161, 192, 24192)
    assert skippable == 17733                               # 0.733 of the eligible slabs
    assert skippable * cases.CHUNK * cases.RETIRE_SH > (cases.RETIRE_HALF + 0.2) * m * n
    # the 15-letter pair: the same shape of alignment, a lower score (every 50th base is an ambiguity code), the same condition
    t0, t1, tflags = cases.retire_pair(pkg, "iupac")
    assert tflags == 0 and len(t0) == m and len(t1) == n
    tref = oracle_full(oracle, t0, t1, special_row_interval=cases.RETIRE_SH, block_h=cases.RETIRE_SH)
    assert tuple(tref["best"][:2]) == cases.RETIRE_BEST[:2] and 5000 < tref["best"][2] < cases.RETIRE_BEST[2]
    tb, _, tk, te = cases.retire_census(dict(zip(tref["special_row_ids"], tref["special_rows"])), tref["best"], m, n)
    print("15 letters: best %s, %d of %d" % (tuple(tref["best"]), tk, te))
    assert tb == 161 and tk * cases.CHUNK * cases.RETIRE_SH > (cases.RETIRE_HALF + 0.1) * m * n


def test_shapes_of_the_gpu_file_take_every_path():
    """the edge shapes: ragged by 1 row, by all but one row, a whole strip more and one row over it; trailing chunks of every
    width -- none, 1, 63, a whole chunk, a whole chunk and 1"""
    assert [m % 256 for m in cases.EDGE_ROWS] == [1, 255, 0, 1] and [m // 256 for m in cases.EDGE_ROWS] == [16, 16, 17, 17]
    assert [n % 64 for n in cases.EDGE_COLS] == [0, 1, 63, 0, 1]
    assert cases.M2 % 1024 and cases.M2 % 512 and cases.M2 % 256 and cases.N2 % 64           # the last strip is ragged at every height
    assert cases.M3 % 1024 == 0 and cases.RETIRE_M % 1024 == 0                               # ... and never here: every strip may retire
