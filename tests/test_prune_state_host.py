"""CPU: the host side of a reproducibly pruned stage 1 that is resumed (F_DETERMINISTIC_PRUNE): the pruning state of the last
special row travels in `status.mi355` next to the row number, and the run that continues from that row hands exactly those
words to the aligner before it starts -- and only then.  The aligner here is the oracle's block aligner with the two calls
recorded (the engine's side of it runs in tests/test_gpu_prune_resume.py)."""
import ctypes
import os
import re

import pytest

import __graft_entry__ as graft
from helpers import make_pair
from test_sra import _check_against_reference, CASE

LIMIT = 200 * 1024                       # the fixture's --disk-size: special rows 8192 and 16384 of 20000
KEY = (0, 0, 20000, 9000, 0, 0)          # (i0, j0, i1, j1, alignment start, alignment end) of the fixture's run


def _state_of(row):
    """what the recording aligner says the state of `row` is: lag 3, words that name the row"""
    return {"row": row, "words": [row - 3, row - 2, row - 2, row + 5], "strip_rows": 256, "lag": 3}


@pytest.fixture()
def doubles(pkg, oracle):
    from oracle.aligner_double import SerialBlockAligner

    class Plain(SerialBlockAligner):
        """the block aligner as the fixture's run used it (--block=8192,1000), with its calls written down"""

        def __init__(self):
            SerialBlockAligner.__init__(self, 8192, 1000)
            self.events = []

        def alignPartition(self, part, mgr):
            self.events.append(("align", part.i0))
            SerialBlockAligner.alignPartition(self, part, mgr)

    class Recording(Plain):
        refuse = False

        def pruneState(self, row):
            self.events.append(("get", row))
            return _state_of(row)

        def setPruneState(self, words, strip_rows, lag):
            self.events.append(("set", list(words), strip_rows, lag))
            if self.refuse:
                raise pkg.AlignerError("setPruneState: EINVAL rows_per_lane is fixed to another strip height")

    return Plain, Recording


class Killed(Exception):
    pass


def _dying_manager(pkg, rows):
    class DyingManager(pkg.Stage1Manager):
        """dies in the middle of the row after `rows` complete ones"""

        def dispatchRow(self, i, buf, length):
            pkg.Stage1Manager.dispatchRow(self, i, buf, length)
            if len(self.sra.rows) >= rows and length > 1:
                raise Killed()
    return DyingManager


def _cut_run(pkg, aligner, work, rows=1):
    s0, s1 = make_pair(pkg, CASE["seq"])
    with pytest.raises(Killed):
        pkg.stage1(aligner, s0, s1, work, sra_limit=LIMIT, manager_class=_dying_manager(pkg, rows))
    return s0, s1


# ---- Status ----------------------------------------------------------------------------------------------------------------

def test_status_round_trips_a_state(pkg, tmp_path):
    work = str(tmp_path)
    st = pkg.sra.Status(work)
    st.claim(KEY, False)
    st.last_special_row = 16384
    st.prune_state = {"row": 16384, "strip_rows": 1024, "lag": 4, "words": [-999999999, -999999999, 7, 7, 4000]}
    st.value_best = (4100, 8192, 9216)
    st.save((9004, 9000, 8091))
    back = pkg.sra.Status(work)
    assert back.loaded and back.last_special_row == 16384 and back.best == (9004, 9000, 8091)
    assert back.prune_state == st.prune_state and back.value_best == (4100, 8192, 9216) and back.value_key == KEY
    assert back.prune_state_for(16384) == st.prune_state and back.prune_state_for(8192) is None
    # the state alone, without a two-phase value
    st.value_best = None
    st.save()
    back = pkg.sra.Status(work)
    assert back.prune_state == st.prune_state and back.value_best is None and back.value_key == KEY
    # a state of another row than the one the status names is not written
    st.last_special_row = 24576
    st.save()
    assert pkg.sra.Status(work).prune_state_for(24576) is None


def test_status_loads_a_side_file_without_a_state(pkg, tmp_path):
    work = str(tmp_path)
    open(os.path.join(work, "status"), "w").write("1\n8192\n9004 9000 8091\n")
    open(os.path.join(work, "status.mi355"), "w").write("4100 0 8192 0 0 20000 9000 0 0\n")      # value_best and its key only
    st = pkg.sra.Status(work)
    assert st.loaded and st.value_best == (4100, 0, 8192) and st.value_key == KEY and st.prune_state is None
    open(os.path.join(work, "status.mi355"), "w").write("4100 0 8192\n")                          # ... and the oldest form
    st = pkg.sra.Status(work)
    assert st.value_best == (4100, 0, 8192) and st.value_key is None and st.prune_state is None
    # a kill between the two renames (side file first): the status file names the row before, whose line is still there
    both = "prune_state 8192 256 1 0 0 20000 9000 0 0 2 5 6\nprune_state 16384 256 1 0 0 20000 9000 0 0 2 7 8\n"
    open(os.path.join(work, "status.mi355"), "w").write(both)
    assert pkg.sra.Status(work).prune_state == {"row": 8192, "strip_rows": 256, "lag": 1, "words": [5, 6]}
    open(os.path.join(work, "status"), "w").write("1\n16384\n9004 9000 8091\n")
    assert pkg.sra.Status(work).prune_state == {"row": 16384, "strip_rows": 256, "lag": 1, "words": [7, 8]}
    open(os.path.join(work, "status"), "w").write("1\n8192\n9004 9000 8091\n")
    # a state line cut short is no state
    open(os.path.join(work, "status.mi355"), "w").write("prune_state 8192 256 3 0 0 20000 9000 0 0 4 1 2 3\n")
    assert pkg.sra.Status(work).prune_state is None


def test_status_drops_the_state_of_another_partition(pkg, tmp_path):
    work = str(tmp_path)
    st = pkg.sra.Status(work)
    st.claim(KEY, False)
    st.last_special_row = 8192
    st.prune_state = _state_of(8192)
    st.save()
    same = pkg.sra.Status(work)
    same.claim(KEY, True)
    assert same.prune_state_for(8192) == _state_of(8192)
    other = pkg.sra.Status(work)
    other.claim((0, 0, 20000, 8000, 0, 0), True)
    assert other.prune_state is None and other.value_key == (0, 0, 20000, 8000, 0, 0)
    fresh = pkg.sra.Status(work)
    fresh.claim(KEY, False)                         # a run that starts from the first row has nothing to continue
    assert fresh.prune_state is None


# ---- stage1() <-> aligner --------------------------------------------------------------------------------------------------

def test_state_is_saved_with_the_row_and_handed_over_on_resume(pkg, tmp_path, doubles):
    _, Recording = doubles
    work = str(tmp_path / "work")
    first = Recording()
    s0, s1 = _cut_run(pkg, first, work)
    assert first.events == [("align", 0), ("get", 8192)]            # asked once, for the row it saved; nothing handed over
    st = pkg.sra.Status(work)
    assert st.last_special_row == 8192 and st.prune_state == _state_of(8192) and st.value_key == KEY
    second = Recording()
    res = pkg.stage1(second, s0, s1, work, sra_limit=LIMIT)
    assert res["resumed_from"] == 8192 and res["reproducible_resume"] is True
    w = _state_of(8192)
    assert second.events[:2] == [("set", w["words"], w["strip_rows"], w["lag"]), ("align", 8192)]      # before alignPartition
    assert [e for e in second.events if e[0] == "set"] == second.events[:1]
    assert ("get", 16384) in second.events                          # rows relative to the sequences the aligner was given
    _check_against_reference(work, res)
    assert not os.path.exists(os.path.join(work, "status.mi355"))   # stage 1 complete: nothing left to continue


def test_a_run_resumed_twice_hands_over_the_state_of_its_own_last_row(pkg, tmp_path, doubles):
    _, Recording = doubles
    work = str(tmp_path / "work")
    s0, s1 = _cut_run(pkg, Recording(), work, rows=1)
    second = Recording()
    with pytest.raises(Killed):
        pkg.stage1(second, s0, s1, work, sra_limit=LIMIT, manager_class=_dying_manager(pkg, 2))   # (rows 8192 and 16384 complete)
    assert pkg.sra.Status(work).prune_state == _state_of(16384)
    third = Recording()
    res = pkg.stage1(third, s0, s1, work, sra_limit=LIMIT)
    w = _state_of(16384)
    assert third.events[:2] == [("set", w["words"], w["strip_rows"], w["lag"]), ("align", 16384)]
    assert res["reproducible_resume"] is True and res["resumed_from"] == 16384
    # (no look at the files here: the block aligner hands out its scores after the whole grid, so the best cell of the rows
    #  the second run swept died with it -- the engine dispatches them before each special row, tests/test_gpu_prune_resume.py)


def test_nothing_is_handed_over_on_a_fresh_run(pkg, tmp_path, doubles):
    _, Recording = doubles
    s0, s1 = make_pair(pkg, CASE["seq"])
    al = Recording()
    res = pkg.stage1(al, s0, s1, str(tmp_path / "work"), sra_limit=LIMIT)
    assert res["resumed_from"] is None and res["reproducible_resume"] is False
    assert not [e for e in al.events if e[0] == "set"]
    assert [e for e in al.events if e[0] == "get"] == [("get", 8192), ("get", 16384), ("get", 20000)]
    _check_against_reference(str(tmp_path / "work"), res)


def test_nothing_is_handed_over_for_another_key_or_another_row(pkg, tmp_path, doubles):
    _, Recording = doubles
    work = str(tmp_path / "work")
    s0, s1 = _cut_run(pkg, Recording(), work)
    side = os.path.join(work, "status.mi355")
    text = open(side).read()
    assert text.startswith("prune_state 8192 256 3 0 0 20000 9000 0 0 4 ")
    # the state of another partition (key), then of another row of this one
    for changed in (text.replace(" 0 0 20000 9000 0 0 ", " 0 0 20000 9000 0 1 "), text.replace("prune_state 8192 ", "prune_state 16384 ")):
        open(side, "w").write(changed)
        al = Recording()
        with pytest.raises(Killed):
            pkg.stage1(al, s0, s1, work, sra_limit=LIMIT, manager_class=_dying_manager(pkg, 1))     # (dies inside its first row)
        assert al.events == [("align", 8192)], changed
    # a run that does not prune has no use for it
    open(side, "w").write(text)
    al = Recording()
    res = pkg.stage1(al, s0, s1, work, sra_limit=LIMIT, block_pruning=False)
    assert res["resumed_from"] == 8192 and res["reproducible_resume"] is False and not [e for e in al.events if e[0] == "set"]


def test_an_aligner_without_the_calls_resumes_as_before(pkg, tmp_path, doubles):
    Plain, _ = doubles
    work = str(tmp_path / "work")
    s0, s1 = _cut_run(pkg, Plain(), work)
    st = pkg.sra.Status(work)
    assert st.last_special_row == 8192 and st.prune_state is None and not os.path.exists(os.path.join(work, "status.mi355"))
    al = Plain()
    res = pkg.stage1(al, s0, s1, work, sra_limit=LIMIT)
    assert res["resumed_from"] == 8192 and res["reproducible_resume"] is False and al.events == [("align", 8192)]
    _check_against_reference(work, res)


def test_an_aligner_that_refuses_the_state_resumes_as_before(pkg, tmp_path, doubles):
    Plain, Recording = doubles
    work = str(tmp_path / "work")
    s0, s1 = _cut_run(pkg, Recording(), work)
    al = Recording()
    al.refuse = True
    res = pkg.stage1(al, s0, s1, work, sra_limit=LIMIT)
    assert [e[0] for e in al.events[:2]] == ["set", "align"]
    assert res["resumed_from"] == 8192 and res["reproducible_resume"] is False
    _check_against_reference(work, res)
    # ... and a state saved by a run whose aligner had none is not there to hand over
    work2 = str(tmp_path / "work2")
    _cut_run(pkg, Plain(), work2)
    al = Recording()
    res = pkg.stage1(al, s0, s1, work2, sra_limit=LIMIT)
    assert res["reproducible_resume"] is False and not [e for e in al.events if e[0] == "set"]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------

def test_the_two_calls_are_declared_exported_and_prototyped(pkg):
    names = ["mi355sw_get_prune_state", "mi355sw_set_prune_state"]
    src = open(os.path.join(graft.ROOT, "include", "mi355sw.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mi355sw_[a-z_0-9]+)\s*\(", src))
    pkg.build_library()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for name in names:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pkg.engine.ABI_SYMBOLS, name
    loaded = pkg.load_library()
    assert len(loaded.mi355sw_get_prune_state.argtypes) == 7 and len(loaded.mi355sw_set_prune_state.argtypes) == 5
    lib.mi355sw_abi_version.restype = ctypes.c_int
    assert lib.mi355sw_abi_version() == 8                           # additive, like mi355sw_set_goal_bounds
    assert hasattr(pkg.MI355Aligner, "pruneState") and hasattr(pkg.MI355Aligner, "setPruneState")
    # the flag's comment names the calls that make its promise about resumed runs true
    flag = re.search(r"#define MI355SW_F_DETERMINISTIC_PRUNE.*?\*/", open(os.path.join(graft.ROOT, "include", "mi355sw.h")).read(), flags=re.S).group(0)
    assert "mi355sw_get_prune_state" in flag and "mi355sw_set_prune_state" in flag
    # a null handle is refused, not dereferenced
    cnt = ctypes.c_int32(5)
    assert lib.mi355sw_set_prune_state(None, None, 0, 0, 0) != 0
    assert lib.mi355sw_get_prune_state(None, 0, None, 0, ctypes.byref(cnt), None, None) != 0
