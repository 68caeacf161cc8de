"""CPU: MI355SW_F_INT32_PRUNE_EDGE_GOAL (the edge rule and goal bounds in the int32 kernel family, opt-in) in the header, in
engine.py, behind its environment switch and in tools/align_fasta.py; and the census of tests/int32_edge_goal_cases.py, which
says at which shapes the GPU file may demand pruned_cells > 0.  What the flag does is tests/test_gpu_int32_edge_goal.py's."""
import os
import re
import subprocess
import sys

import pytest

import __graft_entry__ as graft
import int32_edge_goal_cases as cases


def _read(*path):
    return open(os.path.join(*path), errors="replace").read()


def test_the_flags_value_in_the_header_and_in_the_engine(pkg):
    eng = pkg.engine
    hdr = _read(graft.ROOT, "include", "mi355sw.h")
    m = re.search(r"#define\s+MI355SW_F_INT32_PRUNE_EDGE_GOAL\s+(\d+)", hdr)
    assert m and int(m.group(1)) == eng.F_INT32_PRUNE_EDGE_GOAL == 262144
    bits = [int(v) for v in re.findall(r"#define\s+MI355SW_F_[A-Z0-9_]+\s+(\d+)", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)      # one bit each, none shared
    assert re.search(r"#define\s+MI355SW_ABI_VERSION\s+8\b", hdr)                    # additive: the ABI version stays
    assert eng.F_INT32_PRUNE_EDGE_GOAL != eng.F_INT32_PRUNE_GLOBAL                   # a flag of its own


def test_the_header_says_what_is_served_and_what_is_not():
    hdr = _read(graft.ROOT, "include", "mi355sw.h")
    text = hdr[hdr.index("#define MI355SW_F_INT32_PRUNE_EDGE_GOAL"):hdr.index("#define MI355SW_F_NO_HOST_COUNTER")]
    for word in ("mi355sw_set_prune_end", "mi355sw_set_goal_bounds", "MI355SW_F_DETERMINISTIC_PRUNE", "mi355sw_align_partitions",
                 "block_score_columns", "initial_bound", "MI355SW_EBOUND", "off by default", "MI355SW_F_INT32_PRUNE_GLOBAL"):
        assert word in text, word
    older = hdr[hdr.index("#define MI355SW_F_INT32_PRUNE_GLOBAL"):hdr.index("#define MI355SW_F_INT32_PRUNE_EDGE_GOAL")]
    assert "MI355SW_F_INT32_PRUNE_EDGE_GOAL" in older                                # the older flag points to this one


def test_the_environment_switch(pkg, monkeypatch):
    eng = pkg.engine
    assert eng._ENV_FLAGS["MI355SW_INT32_PRUNE_EDGE_GOAL"] == eng.F_INT32_PRUNE_EDGE_GOAL
    for name in list(eng._ENV_FLAGS):
        monkeypatch.delenv(name, raising=False)
    assert eng.env_switches()[0] == 0                     # off by default
    monkeypatch.setenv("MI355SW_INT32_PRUNE_EDGE_GOAL", "1")
    assert eng.env_switches()[0] == eng.F_INT32_PRUNE_EDGE_GOAL


def test_align_fasta_parses_the_option(tmp_path):
    """the option is taken like its neighbours: with it and no input files the tool ends at its usage text, not at "unknown option"
    (no engine is made before the files are read)"""
    tool = os.path.join(graft.ROOT, "tools", "align_fasta.py")
    text = _read(tool)
    assert "--int32-prune-edge-goal" in text and "F_INT32_PRUNE_EDGE_GOAL" in text
    runs = {}
    for opt in ("--int32-prune-edge-goal", "--int32-prune-global", "--no-such-option"):
        p = subprocess.run([sys.executable, tool, opt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
        runs[opt] = (p.returncode, p.stdout.decode(errors="replace"))
    assert runs["--int32-prune-edge-goal"] == runs["--int32-prune-global"], runs
    assert runs["--no-such-option"] != runs["--int32-prune-global"], runs


def test_the_runtime_and_the_kernel_select_it_by_the_flag_and_by_template_parameters():
    csrc = os.path.join(graft.PKG_DIR, "csrc")
    rt = _read(csrc, "runtime.cpp")
    assert "flag(h, MI355SW_F_INT32_PRUNE_EDGE_GOAL)" in rt
    kern = _read(csrc, "sw_kernel.hip")
    for prof in ("true", "false"):
        assert "sw_strip_kernel<R, false, %s, false, true, true>" % prof in kern            # goal
        assert "sw_strip_kernel<R, false, %s, false, true, false, true>" % prof in kern     # edge
    assert "bool PRUNE = false, bool GOAL = false, bool EDGE = false>" in kern


@pytest.mark.parametrize("m,n", cases.SHAPES, ids=["%dx%d" % s for s in cases.SHAPES])
def test_the_census_runs_and_every_shape_meets_the_one_tenth_condition(pkg, m, n):
    """eligible slabs are whole strips x full chunks from column 128 on; at every shape, rule and height the case module names,
    at least a tenth of them may be skipped whole -- the condition under which the GPU file demands pruned_cells > 0"""
    H = cases.matrix(pkg, m, n)
    assert H.shape == (m + 1, n + 1) and int(H[0, 0]) == 0 and int(H[0, n]) == -3 - 2 * n and int(H[m, 0]) == -3 - 2 * m
    for rule in cases.RULES:
        last = None
        for R in cases.HEIGHTS:
            k, e = cases.census(H, rule, R)
            print("%d x %d, rule %s, %d-row strips: %d of %d eligible slabs may be skipped whole" % (m, n, rule, 64 * R, k, e))
            assert e == (m // (64 * R)) * (n // 64 - 2)
            assert 0 < k <= e and k >= cases.WORTH * e, (rule, R, k, e)
            assert cases.worth_asserting(pkg, m, n, rule, R)
            # (a taller strip's slab is the union of shorter ones: what it may skip, they may)
            assert last is None or k * (e_last // e) <= last, (rule, R, k, last)
            last, e_last = k, e
    # mode 3 ("either") can skip no more than a single-edge mode: its optimum is the larger one, but it forces no gap
    assert cases.bound_of(H, 3) == max(cases.bound_of(H, 1), cases.bound_of(H, 2))


@pytest.mark.parametrize("route", [r for r in cases.ROUTES if r != "forced"])
def test_the_other_routes_pairs_meet_the_condition_too(pkg, route):
    """the 15-letter and the 63-letter pair carry every letter in both sequences at both shapes, and what may be skipped on
    them is at least a tenth as well"""
    for m, n in cases.SHAPES:
        H = cases.matrix(pkg, m, n, route)
        for rule in cases.RULES:
            for R in cases.HEIGHTS:
                k, e = cases.census(H, rule, R)
                assert k >= cases.WORTH * e > 0, (route, m, n, rule, R, k, e)
