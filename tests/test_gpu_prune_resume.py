"""GPU (-m gpu): a reproducibly pruned stage 1 (F_DETERMINISTIC_PRUNE) that is cut off and resumed ends with the BYTES of the
uninterrupted run -- every special row, the status file, the crosspoint -- because the resumed run starts from the pruning
state saved with the row it continues from (mi355sw_get_prune_state / mi355sw_set_prune_state): the words its first strips
read are the ones the strips of the uninterrupted run read at those rows, it runs no probe, seed or warm-up pass of its own,
and never has more strips in flight than the lag the state was saved with.  Without the state (a strip height the state was
not saved at, the int32 family, a state of another row) the run resumes as it always did: same best cell, other lower bounds.

40960 x 30000, special rows every 8192 rows (four, and the last row); the cut is a manager that raises inside dispatchRow."""
import hashlib
import os
import signal
import subprocess
import sys
import time

import pytest

from helpers import assert_pruned_borders, oracle_full, SMITH_WATERMAN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M, N = 40960, 30000
LIMIT = 1250000                 # Job::calculateFlushIntervals: 40960 * 30000 * 8 // 1250000 + 1 = 7865 rows -> the 8192-row minimum
ROW = 8192


class Killed(Exception):
    pass


def _flags(pkg, grow=True):
    """grow: no diagonal seed, no seed pass -- the bound starts at nothing and grows with the sweep"""
    e = pkg.engine
    return e.F_DETERMINISTIC_PRUNE | ((e.F_NO_DIAGONAL_SEED | e.F_NO_SEED_PASS) if grow else 0)


def _cutter(pkg, rows):
    class DyingManager(pkg.Stage1Manager):
        """raises inside the special row after `rows` complete ones (rows of the runs before count: they are on disk)"""
        dead = False

        def dispatchRow(self, i, buf, length):
            if self.dead:
                return
            pkg.Stage1Manager.dispatchRow(self, i, buf, length)
            if len(self.sra.rows) >= rows and length > 1:
                self.dead = True
                self.active = False
                raise Killed()
    return DyingManager


def _tree(work):
    out = {}
    for root, _, files in os.walk(work):
        for fn in files:
            p = os.path.join(root, fn)
            out[os.path.relpath(p, work)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


_PAIR = {}


def _pair(pkg):
    if "p" not in _PAIR:
        _PAIR["p"] = pkg.seqgen.related_pair(M, N)
    return _PAIR["p"]


def _cut_and_resume(pkg, tmp_path, cuts, *, first=None, resume=None, flags=None, stage_kw=None, tamper=None):
    """one run cut after cuts[0], cuts[1], ... complete special rows and resumed each time, and the uninterrupted run of the
    same aligner next to it.  first / resume: MI355Aligner arguments of the run(s) that are cut and of the last one.
    Returns (result of the last run, result of the uninterrupted run, the two work directories, the aligner's kernel name)."""
    s0, s1 = _pair(pkg)
    flags = _flags(pkg) if flags is None else flags
    first = dict(first or {})
    resume = dict(first if resume is None else resume)
    kw = dict(sra_limit=LIMIT, block_pruning=True)
    kw.update(stage_kw or {})
    work, ref_work = str(tmp_path / "cut"), str(tmp_path / "straight")
    al = pkg.MI355Aligner(device=0, **dict(dict(flags=flags), **first))
    try:
        ref = pkg.stage1(al, s0, s1, ref_work, **kw)
        for k, rows in enumerate(cuts):
            with pytest.raises(Killed):
                pkg.stage1(al, s0, s1, work, manager_class=_cutter(pkg, rows), **kw)
            st = pkg.sra.Status(work)
            assert st.stage == 1 and st.last_special_row == rows * ROW
            if k == 0:
                assert st.prune_state is not None and st.prune_state["row"] == rows * ROW, "no pruning state saved with row %d" % (rows * ROW)
                assert len(st.prune_state["words"]) == st.prune_state["lag"] + 1
    finally:
        al.close()
    if tamper is not None:
        tamper(work)
    al = pkg.MI355Aligner(device=0, **dict(dict(flags=flags), **resume))
    try:
        res = pkg.stage1(al, s0, s1, work, **kw)
        kernel = al.getStatistics()["kernel"]
    finally:
        al.close()
    assert ref["resumed_from"] is None and res["resumed_from"] == cuts[-1] * ROW
    return res, ref, work, ref_work, kernel


def _same_bytes(res, ref, work, ref_work, where):
    a, b = _tree(work), _tree(ref_work)
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("%s: reproducible_resume %r, best %r / %r, pruned cells %d (resumed part) / %d, files that differ: %s" % (
        where, res.get("reproducible_resume"), tuple(res["best"]), tuple(ref["best"]), res["pruned_cells"], ref["pruned_cells"], differ or "none"))
    assert res["reproducible_resume"] is True, where
    assert tuple(res["best"]) == tuple(ref["best"]), where
    assert sorted(a) == sorted(b) and len([k for k in a if k.startswith("special_rows")]) == M // ROW + 2, where   # 4 rows + last row + 2 markers
    assert not differ, "%s: %s" % (where, differ)          # every special row, status, crosspoint: the same bytes
    assert ref["pruned_cells"] > 0 and res["pruned_cells"] > 0, where


def test_history_above_the_lag(pkg, oracle, tmp_path):
    """256-row strips (160 of them), 4 wavefronts, cut at strip 64: the lag + 1 words are five different prefixes.  The resumed
    tree is also held to the unpruned oracle, by the criterion every pruned run is held to."""
    res, ref, work, ref_work, kernel = _cut_and_resume(pkg, tmp_path, [2], first=dict(rows_per_lane=4, waves=4))
    assert res["strip_rows"] == 256 and "pk16<2," in kernel and kernel.endswith("true>")
    _same_bytes(res, ref, work, ref_work, "160 strips, lag 4, cut at strip 64")
    s0, s1 = _pair(pkg)
    want = oracle_full(oracle, s0, s1, special_row_interval=ROW)
    assert tuple(res["best"]) == tuple(want["best"])
    part = pkg.sra.SpecialRowsArea(os.path.join(work, "special_rows", "stage.01.00")).create_partition(0, 0, M, N)
    try:
        rows = {i: part.read_row(i) for i in range(ROW, M, ROW)}
        last = part.read_row(M)
    finally:
        part.close()
    assert sorted(rows) == [ROW, 2 * ROW, 3 * ROW, 4 * ROW]
    n_must = assert_pruned_borders(rows, last, None, want, M, N, want["best"][2], SMITH_WATERMAN, col0=True,
                                   must_rows_upto=min(want["best"][0], M - 1), where="resumed tree")
    assert n_must > 0


def test_history_clamped_inside_the_lag(pkg, tmp_path):
    """48 wavefronts, cut at strip 32: the first 17 of the 49 words are prefix[0], strips 32 .. 47 of the uninterrupted run
    read it and so must strips 0 .. 15 of the resumed one"""
    res, ref, work, ref_work, _ = _cut_and_resume(pkg, tmp_path, [1], first=dict(rows_per_lane=4, waves=48))
    _same_bytes(res, ref, work, ref_work, "160 strips, lag 48, cut at strip 32")


def test_default_waves_every_strip_reads_the_start(pkg, tmp_path):
    """1024-row strips, a wavefront for every strip: the lag is the number of strips and every strip reads prefix[0] -- the
    resumed run's strips too, not the best of everything above their first row"""
    res, ref, work, ref_work, _ = _cut_and_resume(pkg, tmp_path, [2], first=dict(rows_per_lane=16))
    assert res["strip_rows"] == 1024
    _same_bytes(res, ref, work, ref_work, "40 strips of 1024 rows, default waves")


def test_default_flags_no_seed_of_its_own(pkg, tmp_path):
    """the warm-up pass of the first run is part of what its strips start from; the resumed run must not run another"""
    res, ref, work, ref_work, _ = _cut_and_resume(pkg, tmp_path, [2], first=dict(rows_per_lane=4, waves=4), flags=_flags(pkg, grow=False))
    _same_bytes(res, ref, work, ref_work, "default flags")


def test_global_alignment(pkg, tmp_path):
    """both ends in the corners, pruned against a running lower bound of the last cell"""
    e = pkg.manager
    kw = dict(alignment_start=e.AT_SEQUENCE_1_AND_2, alignment_end=e.AT_SEQUENCE_1_AND_2, prune_global=True)
    res, ref, work, ref_work, _ = _cut_and_resume(pkg, tmp_path, [2], first=dict(rows_per_lane=4, waves=4), flags=_flags(pkg, grow=False), stage_kw=kw)
    assert tuple(res["best"])[:2] == (M, N)
    _same_bytes(res, ref, work, ref_work, "global")


def test_resumed_twice(pkg, tmp_path):
    """cut after the first row, resumed, cut after the third, resumed: the second state is one a resumed run saved"""
    res, ref, work, ref_work, _ = _cut_and_resume(pkg, tmp_path, [1, 3], first=dict(rows_per_lane=4, waves=4))
    _same_bytes(res, ref, work, ref_work, "resumed twice")


@pytest.mark.parametrize("why", ["another strip height", "int32 family", "state of another row"])
def test_a_state_that_cannot_be_used_falls_back(pkg, tmp_path, why):
    """the resuming engine refuses the state (rows_per_lane fixed to 768-row strips; F_FORCE_INT32), or the side file holds the
    state of a row the run does not continue from: a resume as before this state existed -- not reproducible, same best cell"""
    first = dict(rows_per_lane=4, waves=4)
    resume, tamper, flags = first, None, _flags(pkg)
    if why == "another strip height":
        resume = dict(rows_per_lane=12, waves=4)
    elif why == "int32 family":
        resume = dict(rows_per_lane=4, waves=4, flags=flags | pkg.engine.F_FORCE_INT32)
    else:
        def tamper(work):
            side = os.path.join(work, "status.mi355")
            text = open(side).read()
            assert "prune_state %d " % (2 * ROW) in text
            open(side, "w").write(text.replace("prune_state %d " % (2 * ROW), "prune_state %d " % ROW))
    res, ref, work, ref_work, _ = _cut_and_resume(pkg, tmp_path, [2], first=first, resume=resume, flags=flags, tamper=tamper)
    print("%s: reproducible_resume %r, best %r / %r" % (why, res.get("reproducible_resume"), tuple(res["best"]), tuple(ref["best"])))
    assert res["reproducible_resume"] is False
    assert tuple(res["best"]) == tuple(ref["best"])
    assert open(os.path.join(work, "status")).read() == open(os.path.join(ref_work, "status")).read()


def test_the_engine_refuses_what_it_cannot_honour(pkg):
    """mi355sw_set_prune_state: EINVAL with the reason kept on the handle"""
    e = pkg.engine
    words = [-e.INF, 5, 9]
    for kw, msg in ((dict(flags=0), "DETERMINISTIC_PRUNE is off"),
                    (dict(flags=_flags(pkg) | e.F_FORCE_INT32), "FORCE_INT32"),
                    (dict(flags=_flags(pkg), rows_per_lane=12), "another strip height")):
        al = pkg.MI355Aligner(device=0, **kw)
        try:
            with pytest.raises(pkg.AlignerError, match="EINVAL.*" + msg):
                al.setPruneState(words, 256, 2)
        finally:
            al.close()
    al = pkg.MI355Aligner(device=0, flags=_flags(pkg))
    try:
        al.setPruneState(words, 256, 2)
        with pytest.raises(pkg.AlignerError, match="EINVAL"):
            al.setPruneState(words, 256, 3)                 # lag + 1 words
        with pytest.raises(pkg.AlignerError, match="EINVAL"):
            al.setPruneState(words, 320, 2)                 # no such strip height
        with pytest.raises(pkg.AlignerError, match="EINVAL"):
            al.setPruneState([9, 5, 9], 256, 2)             # not a running maximum
        assert al.pruneState(8192) is None                  # nothing ran: no state
    finally:
        al.close()


CHILD = r"""
import sys, time
sys.path.insert(0, %(root)r)
import __graft_entry__ as g
pkg = g.load_package()
class Slow(pkg.Stage1Manager):
    def dispatchRow(self, i, buf, length):
        pkg.Stage1Manager.dispatchRow(self, i, buf, length)
        if length > 1:
            time.sleep(0.05)
s0, s1 = pkg.seqgen.related_pair(%(m)d, %(n)d, cfg=77)
al = pkg.MI355Aligner(device=0, rows_per_lane=16, flags=pkg.engine.F_DETERMINISTIC_PRUNE)
pkg.stage1(al, s0, s1, %(work)r, sra_limit=%(limit)d, manager_class=Slow, block_pruning=True)
print("child finished", flush=True)
"""


def test_sigkill_then_resume_leaves_the_same_bytes(pkg, tmp_path):
    """200 000 x 30 000, default flags (the probe runs in the first run only), one child process killed once while it writes its
    special rows: the resumed run's whole tree is the uninterrupted run's"""
    m, n, limit = 200000, 30000, 8 << 20
    work = str(tmp_path / "killed")
    child = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, m=m, n=n, work=work, limit=limit)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    d = os.path.join(work, "special_rows", "stage.01.00", "%08X.%08X.%08X.%08X" % (0, 0, m, n))
    try:
        t0 = time.time()
        while time.time() - t0 < 120:
            done = [fn for fn in (os.listdir(d) if os.path.isdir(d) else []) if len(fn) == 8]
            if len(done) >= 4 or child.poll() is not None:
                break
            time.sleep(0.01)
        assert child.poll() is None, child.stdout.read().decode(errors="replace")[-2000:]
    finally:
        if child.poll() is None:
            child.send_signal(signal.SIGKILL)
        child.wait(timeout=60)
    rows_before = sorted(int(fn, 16) for fn in os.listdir(d) if len(fn) == 8)
    assert 4 <= len(rows_before) < m // 8192                       # killed in the middle
    st = pkg.sra.Status(work)
    assert st.stage == 1 and st.last_special_row in rows_before
    assert st.prune_state is not None and st.prune_state["row"] == st.last_special_row and st.prune_state["strip_rows"] == 1024
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=77)
    al = pkg.MI355Aligner(device=0, rows_per_lane=16, flags=pkg.engine.F_DETERMINISTIC_PRUNE)
    try:
        res = pkg.stage1(al, s0, s1, work, sra_limit=limit, block_pruning=True)
        ref_work = str(tmp_path / "straight")
        ref = pkg.stage1(al, s0, s1, ref_work, sra_limit=limit, block_pruning=True)
    finally:
        al.close()
    assert ref["resumed_from"] is None and res["resumed_from"] == st.last_special_row
    a, b = _tree(work), _tree(ref_work)
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("SIGKILL at row %d of %d: reproducible_resume %r, best %r / %r, pruned %d / %d, files that differ: %s" % (
        res["resumed_from"], m, res.get("reproducible_resume"), tuple(res["best"]), tuple(ref["best"]), res["pruned_cells"], ref["pruned_cells"], differ or "none"))
    assert res["reproducible_resume"] is True
    assert tuple(res["best"]) == tuple(ref["best"])
    assert not differ, differ
    assert ref["pruned_cells"] > 0 and res["pruned_cells"] > 0
