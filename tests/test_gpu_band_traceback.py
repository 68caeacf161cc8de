"""GPU (-m gpu): the traceback through a chain of column bands on the engine -- pipeline.align_bands on one MI355Aligner
(bands.serial_band_stage1, then band_traceback.traceback_serial), and bands.band_traceback over three gloo ranks that share
device 0.  Every alignment over more than one band goes through band_traceback_cases.judge (rescored independently against the
oracle's optimum, ends, joined list, stage 5's total); one band leaves pipeline.align's files.  The host side, on the oracle's
doubles: tests/test_band_traceback_host.py."""
import os
import socket
import sys

import pytest

import band_traceback_cases as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (40000, 13200, 500 * 1024)
WEIGHTS = {2: [1, 3], 3: [1, 3, 2], 4: [1, 3, 2, 1]}
THREADS = min(16, os.cpu_count() or 1)
_CACHE = {}


def _pair(pkg):
    if "pair" not in _CACHE:
        s0, s1 = pkg.seqgen.related_pair(SHAPE[0], SHAPE[1], cfg=11, inversion=0.0)
        for a in (s0, s1):
            a.setflags(write=False)
        _CACHE["pair"] = (s0, s1)
    return _CACHE["pair"]


def _optimum(pkg, oracle, edges):
    """the oracle's answer for the sweep's pair: once per form, shared by the band counts"""
    if edges not in _CACHE:
        _CACHE[edges] = bc.oracle_optimum(oracle, *_pair(pkg), edges, threads=THREADS)
    return _CACHE[edges]


def _run(pkg, aligner, s0, s1, work, weights, edges, limit, **kw):
    from masa_cudalign_amd import pipeline
    from masa_cudalign_amd.bands import band_limits
    q0, q1 = bc.fasta_pair(s0, s1)
    kw.setdefault("block_pruning", False)
    out = pipeline.align_bands(aligner, q0, q1, work, weights, sra_limit=limit, **dict(bc.edge_flags(pkg, edges), **kw))
    return out, band_limits(len(s1), weights)


@pytest.mark.parametrize("edges", ["**", "++", "3+", "+3"])
@pytest.mark.parametrize("count", [2, 3, 4])
def test_bands_sweep(pkg, oracle, aligner, tmp_path, count, edges):
    """40 000 x 13 200 in 2, 3 and 4 bands of uneven width on one aligner: local, global and the two half-free forms"""
    s0, s1 = _pair(pkg)
    opt = _optimum(pkg, oracle, edges)
    work = str(tmp_path / "w")
    out, limits = _run(pkg, aligner, s0, s1, work, WEIGHTS[count], edges, SHAPE[2])
    assert tuple(out["best"]) == opt
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, edges, out, optimum=opt, threads=THREADS)
    assert len(out["bands"]) == count and len(seen["on_boundary"]) >= 1
    assert out["bands"][out["keeper"]]["role"] == "band"
    print("bands %d edges %s: seconds %s" % (count, edges, {k: round(v, 3) for k, v in out["seconds"].items()}))


def test_one_band_is_pipeline_align(pkg, aligner, tmp_path):
    from masa_cudalign_amd import pipeline
    s0, s1 = _pair(pkg)
    q0, q1 = bc.fasta_pair(s0, s1)
    a, b = str(tmp_path / "align"), str(tmp_path / "bands")
    one = pipeline.align(aligner, q0, q1, a, sra_limit=SHAPE[2])
    out = pipeline.align_bands(aligner, q0, q1, b, [5], sra_limit=SHAPE[2])
    ta, tb = bc.tree(a), bc.tree(b)
    assert sorted(ta) == sorted(tb) and all(ta[k] == tb[k] for k in ta), [k for k in ta if ta.get(k) != tb.get(k)][:5]
    assert "alignment.00.bin" in ta and "crosspoints/crosspoint_04.00" in ta and not any(k.startswith("FORK") for k in tb)
    assert out["text"] == one["text"] and len(out["bands"]) == 1


@pytest.mark.parametrize("which", [1, 2])
def test_a_gap_run_on_the_boundary(pkg, oracle, aligner, tmp_path, which):
    """24 000 rows: the boundary column cuts a gap run in sequence 0 (handed over as TYPE_GAP_1), or a gap run in sequence 1
    stands on it (handed over at its lower end, where H is the gap component: test_band_traceback_host.py says why)"""
    n, core, cut = 20000, 16000, 41
    b = n // 2
    if which == 1:
        s0, s1 = bc.planted(300, core, 4000, 4000, b - 8000, n - (b - 8000) - core, cut0=(7980, cut))
    else:
        s0, s1 = bc.planted(300, core, 4000, 4000, b - 8000, n - (b - 8000) - (core - cut), cut1=(8000, cut))
    assert len(s1) == n and len(s0) <= 30000
    work = str(tmp_path / "w")
    out, limits = _run(pkg, aligner, s0, s1, work, [1, 1], "**", 2 * 1024 * 1024)
    assert limits[1] == b
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out, threads=THREADS)
    on = sorted(c for c in seen["cells"] if c[1] == b)
    handed = bc.load_points(os.path.join(work, "FORK.00", "crosspoints", "crosspoint_01.00"))
    assert len(handed) == 1 and handed[0][2] == b and handed[0] in seen["cp3"], handed
    if which == 1:
        assert [seen["cells"][c][1] for c in on] == [1] and handed[0][0] == 1, (on, handed)
    else:
        assert [seen["cells"][c][1] for c in on] == [0] + [2] * cut
        assert handed[0][:2] == (0, on[-1][0]) and seen["cells"][on[-1]] == (handed[0][3], 2), handed
    assert len(out["stage1"]["bands"][0]["special_rows"]) >= 2


def test_a_band_of_63_columns(pkg, oracle, aligner, tmp_path):
    from masa_cudalign_amd.bands import band_limits
    n, weights = 20000, [9937, 63, 10000]
    assert band_limits(n, weights) == [0, 9937, 10000, 20000]
    s0, s1 = bc.planted(500, 16000, 4000, 4000, 2000, 2000)
    work = str(tmp_path / "w")
    out, limits = _run(pkg, aligner, s0, s1, work, weights, "**", 2 * 1024 * 1024)
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out, threads=THREADS)
    assert set(seen["on_boundary"]) == {9937, 10000}
    assert out["bands"][1]["role"] == "band" and out["bands"][1]["crosspoints"][2] >= 2


def test_a_pruned_chain(pkg, oracle, aligner, tmp_path):
    """block pruning in every band's stage 1, the bound growing along the chain: the same optimum, judged like the others"""
    s0, s1 = _pair(pkg)
    opt = _optimum(pkg, oracle, "**")
    work = str(tmp_path / "w")
    out, limits = _run(pkg, aligner, s0, s1, work, WEIGHTS[3], "**", SHAPE[2], block_pruning=True)
    assert tuple(out["best"]) == opt
    bc.judge(pkg, oracle, work, s0, s1, limits, "**", out, optimum=opt, threads=THREADS)
    pruned = [b["pruned_cells"] for b in out["stage1"]["bands"]]
    bounds = [b["initial_bound"] for b in out["stage1"]["bands"]]
    print("pruned cells per band", pruned, "bounds", bounds)
    assert max(pruned) > 0
    assert bounds[1] is not None and bounds[1] <= bounds[2] <= opt[2]


def test_a_wide_alphabet_pair(pkg, oracle, tmp_path):
    """16 letters in common, MI355SW_F_WIDE_ALPHABET: the chain on the packed kernels' wide twins"""
    from test_gpu_wide_alphabet import wide_pair, common_letters, POOL, F_WIDE
    s0, s1 = wide_pair(pkg, 30000, 26000, POOL[:16], cfg=703, ensure=True, foreign=False)
    assert common_letters(s0, s1) == 16
    work = str(tmp_path / "w")
    al = pkg.MI355Aligner(device=0, flags=F_WIDE)
    try:
        out, limits = _run(pkg, al, s0, s1, work, [1, 3, 2], "**", 2 * 1024 * 1024)
    finally:
        al.close()
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out, threads=THREADS)
    assert seen["score"] > 5000 and len(seen["on_boundary"]) == 2


# ---------------------------------------------------------------------------------------------------------------------------
# three ranks on device 0
# ---------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys, json
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch.distributed as dist
import __graft_entry__ as graft
pkg = graft.load_package()
import band_traceback_cases as cases
from masa_cudalign_amd import bands
rank, world, port, work, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = port
dist.init_process_group("gloo", rank=rank, world_size=world)
try:
    m, n, limit = %(shape)r
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=11, inversion=0.0)
    q0, q1 = cases.fasta_pair(s0, s1)
    lim = bands.band_limits(n, %(weights)r)
    al = pkg.MI355Aligner(device=0)
    try:
        al.setSequences(s0, s1)
        runner = bands.BandRunner(al, dist=dist, rank=rank, world=world, device=None, segment_rows=4096, transport="host")
        r1 = bands.band_stage1(runner, m, lim[rank], lim[rank + 1], work, limit, n_total=n)
        al.unsetSequences()
        rec = bands.band_traceback(runner, q0, q1, work, lim, sra_limit=limit)
    finally:
        al.close()
    json.dump({"role": rec["role"], "keeper": rec["keeper"], "best": list(r1["best"]),
               "seconds": {str(k): v for k, v in rec["seconds"].items()}}, open(out, "w"))
finally:
    dist.destroy_process_group()
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(240)
def test_three_ranks_share_the_device(pkg, oracle, tmp_path):
    """band_stage1 and bands.band_traceback on three gloo ranks, one aligner each on device 0: judged, and the keeper's rank on
    every rank.  Each child has its own time limit; the parent stops at the first child that dies."""
    import json
    import subprocess
    s0, s1 = _pair(pkg)
    opt = _optimum(pkg, oracle, "**")
    work = str(tmp_path / "w")
    script = str(tmp_path / "child.py")
    with open(script, "w") as f:
        f.write(CHILD % dict(root=ROOT, shape=SHAPE, weights=WEIGHTS[3]))
    port = str(_free_port())
    outs = [str(tmp_path / ("rank%d.json" % r)) for r in range(3)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, script, str(r), "3", port, work, outs[r]])
             for r in range(3)]
    try:
        from concurrent.futures import ThreadPoolExecutor, as_completed
        with ThreadPoolExecutor(3) as pool:
            waits = {pool.submit(p.wait): r for r, p in enumerate(procs)}
            for done in as_completed(waits):
                if done.result() != 0:                 # the others are ended at once, not waited for
                    for p in procs:
                        if p.poll() is None:
                            p.kill()
                    raise AssertionError("rank %d ended with %d" % (waits[done], done.result()))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    res = [json.load(open(fn)) for fn in outs]
    assert len({r["keeper"] for r in res}) == 1 and res[res[0]["keeper"]]["role"] == "band"
    assert all(tuple(r["best"]) == opt for r in res)
    from masa_cudalign_amd.bands import band_limits
    bc.judge(pkg, oracle, work, s0, s1, band_limits(SHAPE[1], WEIGHTS[3]), "**", None, optimum=opt, threads=THREADS)
    print("seconds per rank", [r["seconds"] for r in res])
