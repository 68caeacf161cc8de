"""CPU: block pruning of alignments that end on a sequence edge (mi355sw_set_prune_end, Stage1Manager(prune_edges=True),
stage1(prune_edges=True)) -- the RULE, at cell level in numpy (tests/edge_prune_cases.py), and the HOST side: the mode reaches
the aligner exactly when it should, and the ABI carries the call.

The rule is the global one (AbstractBlockPruning.cpp:92-109) with the forced gap of the edge the alignment may end on; the
reference's stage 1 never prunes such a run (sw_stage1.cpp:219-225), so the oracle of a pruned run is the unpruned one."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft
import edge_prune_cases as ec

N_PAIRS = 44
_full = {}


def _pair(k, pkg):
    """pair k with its full DP under its own borders and the global DP (gap borders), computed once"""
    if k not in _full:
        s0, s1, start = ec.seeded_pair(k, pkg)
        rg, cg = ec.START_BORDERS[start]
        H, E, F, _, _ = ec.nw_dp(s0, s1, rg, cg)
        Hg = H if (rg and cg) else ec.nw_dp(s0, s1, True, True)[0]
        for a in (H, E, F):
            a.setflags(write=False)
        _full[k] = (s0, s1, start, H, E, F, int(Hg[-1, -1]))
    return _full[k]


@pytest.mark.parametrize("k", range(N_PAIRS))
def test_cell_level_pruned_dp_keeps_the_optimum_and_every_must_cell(k, pkg):
    """44 seeded pairs up to 400 x 400 (related of four divergences and unrelated, square, m >> n, n >> m, zero and gap
    borders), every mode: the pruned DP's optimum is the full DP's, every value with v + reach >= optimum -- H, E and F of
    every cell of the matrix -- is the full DP's, every other value is it or lies below it; the global score with gap
    borders is no more than the optimum of any mode (the seed's first bound)"""
    s0, s1, start, H, E, F, h_global = _pair(k, pkg)
    m, n = len(s0), len(s1)
    rg, cg = ec.START_BORDERS[start]
    ii, jj = np.meshgrid(np.arange(m + 1), np.arange(n + 1), indexing="ij")
    shares = []
    for mode in ec.MODES:
        opt = ec.edge_optimum(mode, H[m, :, None], H[:, n, None])
        assert h_global <= opt, (mode, h_global, opt)
        for bound in (None, h_global):
            Hp, Ep, Fp, share, lb = ec.nw_dp(s0, s1, rg, cg, mode=mode, bound=bound)
            assert lb <= opt, (mode, lb, opt)                      # the running bound never passes what exists
            assert ec.edge_optimum(mode, Hp[m, :, None], Hp[:, n, None]) == opt, mode
            for name, got, want in (("E", Ep, E), ("F", Fp, F)):
                cells_got = np.stack([Hp.ravel(), got.ravel()], axis=1)
                cells_want = np.stack([H.ravel(), want.ravel()], axis=1)
                n_must, _ = ec.assert_edge_pruned_cells(cells_got, cells_want, ii.ravel(), jj.ravel(), m, n, opt, mode,
                                                        where="pair %d H/%s bound %s" % (k, name, bound))
                assert n_must > 0
            shares.append(share)
    print("pair %d (%d x %d, start %d): void share row/column/either, sweep-grown and seeded: %s" % (k, m, n, start, " ".join("%.3f" % s for s in shares)))


@pytest.mark.parametrize("start", [1, 2, 3, 4])
@pytest.mark.parametrize("end", [1, 2, 3])
def test_full_dp_is_the_oracles(start, end, pkg, oracle):
    """the numpy DP the rule is tested on, pinned on oracle.stage1 for each of the twelve start x end forms: best score of the
    allowed edge, last row and last column with their gap components"""
    from helpers import oracle_kwargs
    for k in (start + 4 * end, 20 + start):
        s0, s1 = pkg.seqgen.related_pair(230 + 17 * k, 310 - 11 * k, cfg=9300 + k, p_sub=0.05, p_indel=0.01)
        m, n = len(s0), len(s1)
        rg, cg = ec.START_BORDERS[start]
        H, E, F, _, _ = ec.nw_dp(s0, s1, rg, cg)
        kw = oracle_kwargs(oracle, dict(start=start, end=end, pruning=False, disk=-1, block=(64, 64)), m, n)
        kw.update(want_last_row=True, want_last_col=True)
        ref = oracle.stage1(s0, s1, **kw)
        assert ref["best"][2] == ec.edge_optimum(end, H[m, :, None], H[:, n, None])
        assert np.array_equal(ref["last_row"][:, 0], H[m, :]) and np.array_equal(ref["last_col"][:, 0], H[:, n])
        assert np.array_equal(ref["last_row"][1:, 1], F[m, 1:]) and np.array_equal(ref["last_col"][1:, 1], E[1:, n])


def _recording_double():
    from oracle.aligner_double import SerialBlockAligner

    class Plain(SerialBlockAligner):
        """an aligner without the call"""
        def __init__(self):
            SerialBlockAligner.__init__(self, 512, 512)
            self.log = []

        def alignPartition(self, part, mgr):
            self.log.append(("align", part.i0, bool(mgr.mustPruneBlocks())))
            return SerialBlockAligner.alignPartition(self, part, mgr)

    class Recording(Plain):
        def setPruneEnd(self, mode):
            self.log.append(("end", int(mode)))

    return Plain, Recording


@pytest.mark.parametrize("start,end,mode", [(4, 1, 1), (3, 2, 2), (1, 3, 3), (2, 1, 1)])
def test_stage1_hands_the_mode_to_the_aligner_exactly_when_it_should(start, end, mode, pkg, oracle, tmp_path):
    """fresh run, resumed run, flag off, aligner without the method -- and edges the option does not cover"""
    from masa_cudalign_amd.stage1 import stage1
    from masa_cudalign_amd import sra as sra_mod
    Plain, Recording = _recording_double()
    m, n = 2600, 2500
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=9400 + start)
    from helpers import oracle_kwargs
    want = oracle.stage1(s0, s1, **oracle_kwargs(oracle, dict(start=start, end=end, pruning=False, disk=-1, block=(512, 512)), m, n))["best"]
    limit = 4 * (n + 1) * 8
    # fresh run: one call with the mode, right before the partition
    al = Recording()
    r = stage1(al, s0, s1, str(tmp_path / "on"), alignment_start=start, alignment_end=end, sra_limit=limit, prune_edges=True)
    assert al.log == [("end", mode), ("align", 0, True)] and tuple(r["best"]) == tuple(want)
    # resumed run: a run that died inside its second special row continues from the first -- with the mode
    assert len([x for x in r["special_rows"] if x < m]) >= 2

    class Killed(Exception):
        pass

    class DyingManager(pkg.Stage1Manager):
        dead = False

        def dispatchRow(self, i, buf, length):
            if DyingManager.dead:
                return
            pkg.Stage1Manager.dispatchRow(self, i, buf, length)
            if len(self.sra.rows) >= 1 and length > 1:
                DyingManager.dead = True
                self.active = False
                raise Killed()

    work = str(tmp_path / "resume")
    with pytest.raises(Killed):
        stage1(Recording(), s0, s1, work, alignment_start=start, alignment_end=end, sra_limit=limit, prune_edges=True, manager_class=DyingManager)
    keep = sra_mod.Status(work).last_special_row
    assert 0 < keep < m
    al = Recording()
    r2 = stage1(al, s0, s1, work, alignment_start=start, alignment_end=end, sra_limit=limit, prune_edges=True)
    assert r2["resumed_from"] == keep and al.log == [("end", mode), ("align", keep, True)] and tuple(r2["best"]) == tuple(want)
    # flag off: no call, no pruning request
    al = Recording()
    r = stage1(al, s0, s1, str(tmp_path / "off"), alignment_start=start, alignment_end=end, sra_limit=limit)
    assert al.log == [("align", 0, False)] and tuple(r["best"]) == tuple(want)
    # an aligner without the method: nobody can tell it the edge, so nothing asks it to prune
    al = Plain()
    r = stage1(al, s0, s1, str(tmp_path / "plain"), alignment_start=start, alignment_end=end, sra_limit=limit, prune_edges=True)
    assert al.log == [("align", 0, False)] and tuple(r["best"]) == tuple(want)


@pytest.mark.parametrize("start,end", [(0, 0), (4, 4), (0, 1), (0, 3)])
def test_edges_the_option_does_not_cover_hear_nothing(start, end, pkg, tmp_path):
    """local, global and floor-plus-edge forms: prune_edges changes nothing about what the manager asks for"""
    from masa_cudalign_amd.stage1 import stage1
    _, Recording = _recording_double()
    s0, s1 = pkg.seqgen.related_pair(700, 650, cfg=9500)
    logs = []
    for flag in (False, True):
        al = Recording()
        stage1(al, s0, s1, str(tmp_path / ("w%d" % flag)), alignment_start=start, alignment_end=end, prune_edges=flag)
        logs.append(al.log)
    assert logs[0] == logs[1] and all(e[0] == "align" for e in logs[0])
    for s in (1, 2, 3, 4):
        for e in (1, 2, 3):
            part = pkg.Partition(0, 0, 700, 650)
            on = pkg.Stage1Manager(part, alignment_start=s, alignment_end=e, block_pruning=True, prune_edges=True)
            off = pkg.Stage1Manager(part, alignment_start=s, alignment_end=e, block_pruning=True)
            never = pkg.Stage1Manager(part, alignment_start=s, alignment_end=e, block_pruning=False, prune_edges=True)
            assert on.mustPruneBlocks() and on.pruneEnd() == e and on.getRecurrenceType() == pkg.NEEDLEMAN_WUNSCH
            assert (e & 1) == 0 or on.mustDispatchLastRow()
            assert (e & 2) == 0 or on.mustDispatchLastColumn()
            assert not on.mustDispatchLastCell() and not on.mustDispatchScores()
            assert not off.mustPruneBlocks() and off.pruneEnd() == 0
            assert not never.mustPruneBlocks() and never.pruneEnd() == 0


def test_the_abi_carries_the_call(pkg):
    """the symbol and the four constants: header, library, prototype list, Python front"""
    hdr = open(os.path.join(graft.ROOT, "include", "mi355sw.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mi355sw_set_prune_end\s*\(\s*mi355sw_handle\s*\*\s*h\s*,\s*int32_t\s+end\s*\)\s*;", code)
    consts = dict(re.findall(r"#define\s+(MI355SW_END_[A-Z_]+)\s+(\d+)", code))
    assert consts == {"MI355SW_END_LAST_CELL": "0", "MI355SW_END_LAST_ROW": "1", "MI355SW_END_LAST_COLUMN": "2", "MI355SW_END_ROW_OR_COLUMN": "3"}
    eng = pkg.engine
    assert (eng.END_LAST_CELL, eng.END_LAST_ROW, eng.END_LAST_COLUMN, eng.END_ROW_OR_COLUMN) == (0, 1, 2, 3)
    assert "mi355sw_set_prune_end" in eng.ABI_SYMBOLS
    pkg.build_library()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "mi355sw_set_prune_end")
    assert lib.mi355sw_set_prune_end(None, 1) != 0                  # (no handle: MI355SW_EINVAL, nothing touched)
    assert callable(getattr(pkg.MI355Aligner, "setPruneEnd", None))
    assert lib.mi355sw_abi_version() == 8
