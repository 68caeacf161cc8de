"""CPU: MI355SW_F_INT32_PRUNE_GLOBAL (block pruning of global alignments in the int32 kernel family, opt-in) in the header, in
engine.py, behind its environment switch and in the three fronts.  What it does is tests/test_gpu_int32_prune_global.py's."""
import os
import re

import __graft_entry__ as graft


def _read(*path):
    return open(os.path.join(*path), errors="replace").read()


def test_the_flags_value_in_the_header_and_in_the_engine(pkg):
    eng = pkg.engine
    hdr = _read(graft.ROOT, "include", "mi355sw.h")
    m = re.search(r"#define\s+MI355SW_F_INT32_PRUNE_GLOBAL\s+(\d+)", hdr)
    assert m and int(m.group(1)) == eng.F_INT32_PRUNE_GLOBAL == 131072
    bits = [int(v) for v in re.findall(r"#define\s+MI355SW_F_[A-Z0-9_]+\s+(\d+)", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)      # one bit each, none shared
    assert re.search(r"#define\s+MI355SW_ABI_VERSION\s+8\b", hdr)                    # additive: the ABI version stays


def test_the_header_says_what_is_not_served():
    hdr = _read(graft.ROOT, "include", "mi355sw.h")
    text = hdr[hdr.index("#define MI355SW_F_INT32_PRUNE_GLOBAL"):hdr.index("#define MI355SW_F_NO_HOST_COUNTER")]
    for word in ("mi355sw_set_prune_end", "mi355sw_set_goal_bounds", "MI355SW_F_DETERMINISTIC_PRUNE", "mi355sw_align_partitions",
                 "diagonal seed", "initial_bound", "MI355SW_EBOUND", "off by default"):
        assert word in text, word


def test_the_environment_switch(pkg, monkeypatch):
    eng = pkg.engine
    assert eng._ENV_FLAGS["MI355SW_INT32_PRUNE_GLOBAL"] == eng.F_INT32_PRUNE_GLOBAL
    for name in list(eng._ENV_FLAGS):
        monkeypatch.delenv(name, raising=False)
    assert eng.env_switches()[0] == 0                     # off by default
    monkeypatch.setenv("MI355SW_INT32_PRUNE_GLOBAL", "1")
    assert eng.env_switches()[0] == eng.F_INT32_PRUNE_GLOBAL


def test_the_three_fronts_name_it():
    host = os.path.join(graft.PKG_DIR, "host")
    assert '"int32-prune-global"' in _read(host, "Mi355AlignerParameters.cpp")
    assert "getInt32PruneGlobal" in _read(host, "Mi355AlignerParameters.hpp")
    assert "MI355SW_F_INT32_PRUNE_GLOBAL" in _read(host, "Mi355Aligner.cpp")
    tool = _read(graft.ROOT, "tools", "align_fasta.py")
    assert "--int32-prune-global" in tool and "F_INT32_PRUNE_GLOBAL" in tool


def test_the_runtime_and_the_kernel_select_it_by_the_flag_and_by_template_parameters():
    csrc = os.path.join(graft.PKG_DIR, "csrc")
    rt = _read(csrc, "runtime.cpp")
    assert "flag(h, MI355SW_F_INT32_PRUNE_GLOBAL)" in rt
    kern = _read(csrc, "sw_kernel.hip")
    for prof in ("true", "false"):
        assert "sw_strip_kernel<R, false, %s, false, true>" % prof in kern
    assert "constexpr bool NWP = PRUNE && !SW;" in kern
