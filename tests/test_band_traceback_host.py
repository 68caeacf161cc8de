"""CPU: the traceback through a chain of column bands (masa-cudalign_amd/band_traceback.py, bands.serial_band_stage1,
pipeline.align_bands, bands.band_traceback) on the oracle's aligner doubles -- one aligner with the bands' streaming surface
(tests/test_bands_gloo.py's stand-in) for stage 1 and the serial block aligner (oracle/aligner_double.py) for stages 2-4.

What an alignment over more than one band is held to is written once, in band_traceback_cases.judge: rescored independently it
scores the oracle's optimum, its ends satisfy the edges, the joined crosspoint list is ordered, meets every boundary and carries
the path's scores, and stage 5's total agrees.  One band: the files of pipeline.align, byte for byte.  On the GPU:
tests/test_gpu_band_traceback.py."""
import os
import sys

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import band_traceback_cases as bc
from test_bands_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = (40000, 13200, 500 * 1024)            # the shape and budget of check_area_against_split_reference on the engine


# ---------------------------------------------------------------------------------------------------------------------------
# stage 1: the serial chain leaves what the ranks leave
# ---------------------------------------------------------------------------------------------------------------------------
def _worker_area(rank, world, port, m, n, limit, work, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as graft
    pkg = graft.load_package()
    oracle = graft.load_oracle()
    from masa_cudalign_amd.bands import BandRunner, band_limits, band_stage1
    from test_bands_gloo import OracleStreamEngine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        s0, s1 = pkg.seqgen.related_pair(m, n, cfg=11)
        lim = band_limits(n, [1] * world)
        eng = OracleStreamEngine(oracle, s0, s1, seg=256)
        runner = BandRunner(eng, dist=dist, rank=rank, world=world, device=None, segment_rows=4096, transport="host")
        res = band_stage1(runner, m, lim[rank], lim[rank + 1], work, limit, n_total=n)
        dist.barrier()
        q.put((rank, res["best"]))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def parity_areas(pkg, oracle, tmp_path_factory):
    """the producer-parity pair once: band_stage1 over gloo (world 3) and serial_band_stage1 on one engine, 40 000 x 13 200"""
    from masa_cudalign_amd.bands import band_limits, serial_band_stage1
    m, n, limit = PARITY
    base = tmp_path_factory.mktemp("parity")
    ranks, serial = str(base / "ranks"), str(base / "serial")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_area, args=(r, 3, port, m, n, limit, ranks, q)) for r in range(3)]
    for p in procs:
        p.start()
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=11)
    al = bc.HostAligner(oracle, 256, 128)
    al.setSequences(s0, s1)
    got = serial_band_stage1(al, m, band_limits(n, [1, 1, 1]), serial, limit)
    al.unsetSequences()
    bests = dict(q.get(timeout=280) for _ in range(3))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return dict(ranks=ranks, serial=serial, best=got["best"], rank_bests=bests, s0=s0, s1=s1, result=got)


@pytest.mark.timeout(600)
def test_the_serial_chain_leaves_the_areas_of_the_ranks(parity_areas):
    """producer parity: FORK.00 .. FORK.02 of serial_band_stage1 and of band_stage1 over gloo are the same trees, byte for byte
    -- partition directories, rows with their boundary cell, markers, the tee'd boundary column, crosspoint_01.00"""
    a, b = bc.tree(parity_areas["ranks"]), bc.tree(parity_areas["serial"])
    assert sorted(a) == sorted(b)
    assert all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]][:5]
    names = sorted(a)
    for k in range(3):
        assert "FORK.%02d/crosspoints/crosspoint_01.00" % k in names
    assert sum(1 for x in names if x.endswith("C00000000.INIT_WITH_CUSTOM_DATA")) == 2
    assert sum(1 for x in names if len(os.path.basename(x)) == 8) >= 12          # special rows (and the last row) of three bands
    assert all(tuple(v) == tuple(parity_areas["best"]) for v in parity_areas["rank_bests"].values())


def test_a_pruning_serial_chain_starts_every_band_from_a_bound_that_only_grows(pkg, oracle, tmp_path):
    from masa_cudalign_amd.bands import band_limits, serial_band_stage1
    m, n = 3000, 3300
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=41)
    want = oracle.stage1(s0, s1)["best"]
    al = bc.HostAligner(oracle, 256, 128)
    al.setSequences(s0, s1)
    got = serial_band_stage1(al, m, band_limits(n, [1, 3, 2]), str(tmp_path / "w"), 100 * 1024, prune_blocks=True)
    assert tuple(got["best"]) == tuple(want)
    bounds = [b["initial_bound"] for b in got["bands"]]
    assert bounds[0] is None and bounds[1] is not None and bounds[1] <= bounds[2] <= want[2]
    assert bounds[1] == got["bands"][0]["best"][2]
    assert any(b["pruned_cells"] > 0 for b in got["bands"])


# ---------------------------------------------------------------------------------------------------------------------------
# one band: pipeline.align's files
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_band_is_pipeline_align(pkg, oracle, tmp_path):
    from masa_cudalign_amd import pipeline
    s0, s1 = pkg.seqgen.related_pair(4000, 3600, cfg=5)
    q0, q1 = bc.fasta_pair(s0, s1)
    a, b = str(tmp_path / "align"), str(tmp_path / "bands")
    one = pipeline.align(bc.HostAligner(oracle, 128, 128), q0, q1, a, sra_limit=100 * 1024, block_pruning=False)
    out = pipeline.align_bands(bc.HostAligner(oracle, 128, 128), q0, q1, b, [7], sra_limit=100 * 1024, block_pruning=False)
    ta, tb = bc.tree(a), bc.tree(b)
    assert sorted(ta) == sorted(tb) and all(ta[k] == tb[k] for k in ta)
    assert "alignment.00.txt" in ta and "crosspoints/crosspoint_04.00" in ta and not any(k.startswith("FORK") for k in tb)
    assert out["text"] == one["text"] and tuple(out["best"]) == tuple(one["best"])
    assert len(out["bands"]) == 1 and out["bands"][0]["crosspoints"] == one["crosspoints"] and out["keeper"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# more bands: judged
# ---------------------------------------------------------------------------------------------------------------------------
SWEEP = (4000, 3600, 100 * 1024)
WEIGHTS = {2: [1, 3], 3: [1, 3, 2], 4: [1, 3, 2, 1]}
_OPT = {}


def _sweep_pair(pkg):
    return pkg.seqgen.related_pair(SWEEP[0], SWEEP[1], cfg=23, inversion=0.0)


def _run(pkg, oracle, s0, s1, work, weights, edges, limit, block=(128, 128), **kw):
    from masa_cudalign_amd import pipeline
    from masa_cudalign_amd.bands import band_limits
    q0, q1 = bc.fasta_pair(s0, s1)
    out = pipeline.align_bands(bc.HostAligner(oracle, *block), q0, q1, work, weights, sra_limit=limit, block_pruning=False,
                               **dict(bc.edge_flags(pkg, edges), **kw))
    return out, band_limits(len(s1), weights)


@pytest.mark.parametrize("edges", ["**", "++", "3+", "+3"])
@pytest.mark.parametrize("count", [2, 3, 4])
def test_bands_sweep(pkg, oracle, tmp_path, count, edges):
    """2, 3 and 4 bands of uneven width, local, global and the two half-free forms, each under (a)-(d)"""
    s0, s1 = _sweep_pair(pkg)
    if edges not in _OPT:
        _OPT[edges] = bc.oracle_optimum(oracle, s0, s1, edges)
    work = str(tmp_path / "w")
    out, limits = _run(pkg, oracle, s0, s1, work, WEIGHTS[count], edges, SWEEP[2])
    assert tuple(out["best"]) == _OPT[edges]
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, edges, out, optimum=_OPT[edges])
    assert len(out["bands"]) == count and len(seen["on_boundary"]) >= 1
    assert out["bands"][out["keeper"]]["role"] == "band"
    assert all(b["seconds"].get(1, 0) > 0 for b in out["bands"])


def _special_row(m, n, limit, bh):
    """the spacing of the special rows the double's stage 1 keeps (Job.cpp:231-241, rounded up to whole blocks)"""
    interval = m * n * 8 // max(limit, n * 16) + 1
    return -(-interval // bh) * bh


def test_an_alignment_inside_a_middle_band(pkg, oracle, tmp_path):
    """ends and starts inside band 1 of 3: band 2 only passes the crosspoint on, band 0 hears nothing, band 1 keeps"""
    s0, s1 = bc.planted(100, 600, 700, 700, 1200, 1200)
    out, limits = _run(pkg, oracle, s0, s1, str(tmp_path / "w"), [1, 1, 1], "**", 60 * 1024)
    seen = bc.judge(pkg, oracle, str(tmp_path / "w"), s0, s1, limits, "**", out)
    assert limits[1] < seen["start"][1] and seen["end"][1] < limits[2]
    assert [b["role"] for b in out["bands"]] == ["idle", "band", "forward"] and out["keeper"] == 1
    assert seen["on_boundary"] == {} and seen["score"] >= 590


def test_a_crossing_on_the_corner_of_a_special_row(pkg, oracle, tmp_path):
    """the path meets the boundary column exactly on a special row: the crosspoint handed over is that corner, an aligned pair"""
    m, n, limit, bh = 3000, 3000, 64 * 1024, 128
    r, b = _special_row(m, n, limit, bh), 1500
    assert 0 < r < 2000
    before1 = 900
    before0 = before1 + r - b
    assert before0 > 0
    s0, s1 = bc.planted(200, 1200, before0, m - 1200 - before0, before1, n - 1200 - before1)
    work = str(tmp_path / "w")
    out, limits = _run(pkg, oracle, s0, s1, work, [1, 1], "**", limit)
    assert limits == [0, b, n]
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out)
    assert all(r in band["special_rows"] for band in out["stage1"]["bands"])
    assert (r, b) in seen["cells"]
    assert [p[:3] for p in seen["on_boundary"][b]] == [(0, r, b)]
    first = bc.load_points(os.path.join(work, "FORK.00", "crosspoints", "crosspoint_01.00"))
    assert first == seen["on_boundary"][b]


@pytest.mark.parametrize("which", [1, 2])
def test_a_crossing_inside_a_gap_run(pkg, oracle, tmp_path, which):
    """the boundary column meets a gap run.  In sequence 0 the run lies along sequence 1 and crosses the column: the crosspoint
    handed over is TYPE_GAP_1 with the run's score so far.  In sequence 1 the run lies ALONG the column and cannot cross it; the
    band on the right meets it at its lower end, where H equals the gap component (a larger H there would be a better alignment),
    and stage 2 matches H first: what is handed over is that cell as TYPE_MATCH, carrying the whole run's cost, and the band on
    the left walks up the run.  A hand-over of TYPE_GAP_2 does not exist -- TYPE_GAP_2 crosspoints on the boundary column do,
    where the run passes special rows of the left band: test_a_gap_run_along_the_boundary_..."""
    b, core, cut = 1500, 1600, 41
    if which == 1:          # columns before1 + 780 + 1 .. + 41 of the run: the boundary inside
        s0, s1 = bc.planted(300, core, 500, 900, b - 800, 3000 - (b - 800) - core, cut0=(780, cut))
    else:                   # the run stands on column before1 + 800 = b
        s0, s1 = bc.planted(300, core, 500, 900, b - 800, 3000 - (b - 800) - (core - cut), cut1=(800, cut))
    assert len(s1) == 3000
    work = str(tmp_path / "w")
    out, limits = _run(pkg, oracle, s0, s1, work, [1, 1], "**", 64 * 1024)
    assert limits[1] == b
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out)
    on = sorted(c for c in seen["cells"] if c[1] == b)
    if which == 1:          # one cell of the path on the column, inside the run
        assert [seen["cells"][c][1] for c in on] == [1], "the run does not lie where it was planted"
    else:                   # the pair the run starts from, then the run
        assert [seen["cells"][c][1] for c in on] == [0] + [2] * cut, "the run does not lie where it was planted"
    handed = bc.load_points(os.path.join(work, "FORK.00", "crosspoints", "crosspoint_01.00"))
    assert len(handed) == 1 and handed[0][2] == b and handed[0] in seen["cp3"], handed
    if which == 1:
        assert handed[0][0] == 1 and seen["cells"][(handed[0][1], b)][1] == 1, handed
    else:
        assert handed[0][:2] == (0, on[-1][0]) and seen["cells"][on[-1]] == (handed[0][3], 2), handed


def test_a_gap_run_along_the_boundary_for_more_than_one_special_row_spacing(pkg, oracle, tmp_path):
    m_core, cut, b, bh = 4400, 600, 2500, 128
    s0, s1 = bc.planted(400, m_core, 300, 300, b - 2200, 2100, cut1=(2200, cut))
    m, n = len(s0), len(s1)
    limit = m * n * 8 // 250
    r = _special_row(m, n, limit, bh)
    assert r <= 256 and cut > 2 * r
    work = str(tmp_path / "w")
    out, limits = _run(pkg, oracle, s0, s1, work, [b, n - b], "**", limit)
    assert limits[1] == b
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out)
    run = sorted(c[0] for c in seen["cells"] if c[1] == b)
    assert len(run) == cut + 1 or len(run) == cut, len(run)
    rows = [x for x in out["stage1"]["bands"][0]["special_rows"] if run[0] < x < run[-1]]
    assert len(rows) >= 2                         # special rows of the left band cross the run ...
    crossed = [p for p in seen["on_boundary"][b] if p[0] == 2]
    assert len(crossed) >= 2 and all(run[0] < p[1] < run[-1] for p in crossed)      # ... and leave TYPE_GAP_2 crosspoints on the column
    assert seen["score"] > 2200 + 300             # more than the longer arm of the core alone: the run is part of the alignment


def test_a_narrow_band_crossed_between_two_special_rows(pkg, oracle, tmp_path):
    """a band 63 columns wide, crossed by the alignment without meeting a special row inside it"""
    from masa_cudalign_amd.bands import band_limits
    n, weights = 3000, [1437, 63, 1500]
    assert band_limits(n, weights) == [0, 1437, 1500, 3000]
    s0, s1 = bc.planted(500, 2000, 400, 600, 500, 500)
    work = str(tmp_path / "w")
    out, limits = _run(pkg, oracle, s0, s1, work, weights, "**", 64 * 1024)
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out)
    assert limits[2] - limits[1] == 63
    lo = min(c[0] for c in seen["cells"] if c[1] == limits[1])
    hi = max(c[0] for c in seen["cells"] if c[1] == limits[2])
    inside = [x for x in out["stage1"]["bands"][1]["special_rows"] if lo <= x <= hi]
    assert inside == [] and hi - lo >= 63
    band = out["bands"][1]
    assert band["role"] == "band" and band["crosspoints"][2] == 2          # where it came in and where it went out
    assert set(seen["on_boundary"]) == {1437, 1500}


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, oracle, tmp_path):
    from masa_cudalign_amd import pipeline, band_traceback as bt
    s0, s1 = bc.planted(100, 600, 700, 700, 1200, 1200)
    q0, q1 = bc.fasta_pair(s0, s1)
    with pytest.raises(ValueError, match="max_alignments"):
        pipeline.align_bands(bc.HostAligner(oracle, 128, 128), q0, q1, str(tmp_path / "a"), [1, 1], sra_limit=60 * 1024, max_alignments=2)
    work = str(tmp_path / "w")
    out, limits = _run(pkg, oracle, s0, s1, work, [1, 1, 1], "**", 60 * 1024)
    al = bc.HostAligner(oracle, 128, 128)
    with pytest.raises(ValueError, match="max_alignments"):
        bt.traceback_serial(al, q0, q1, work, limits, sra_limit=60 * 1024, max_alignments=3)
    with pytest.raises(ValueError, match="tile"):
        bt.traceback_serial(al, q0, q1, work, [0, 900, 2000, 3000], sra_limit=60 * 1024)
    with pytest.raises(ValueError, match="FORK"):
        bt.traceback_serial(al, q0, q1, work, [0, 1500, 3000], sra_limit=60 * 1024)
    with pytest.raises(ValueError, match="local"):
        pipeline.align_bands(al, q0, q1, str(tmp_path / "b"), [1, 1], alignment_end=pkg.AT_SEQUENCE_1)
    bt.traceback_serial(al, q0, q1, work, limits, sra_limit=60 * 1024)          # ... and the right chain is traced again


# ---------------------------------------------------------------------------------------------------------------------------
# the collective form
# ---------------------------------------------------------------------------------------------------------------------------
def _worker_trace(rank, world, port, work, weights, limit, fail_rank, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as graft
    pkg = graft.load_package()
    oracle = graft.load_oracle()
    import band_traceback_cases as cases
    from masa_cudalign_amd import bands, band_traceback as bt
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        s0, s1 = pkg.seqgen.related_pair(SWEEP[0], SWEEP[1], cfg=23, inversion=0.0)
        q0, q1 = cases.fasta_pair(s0, s1)
        lim = bands.band_limits(len(s1), weights)
        al = cases.HostAligner(oracle, 128, 128)
        al.setSequences(s0, s1)
        runner = bands.BandRunner(al, dist=dist, rank=rank, world=world, device=None, segment_rows=1024, transport="host")
        r1 = bands.band_stage1(runner, len(s0), lim[rank], lim[rank + 1], work, limit, n_total=len(s1))
        al.unsetSequences()
        if rank == fail_rank:
            def broken(*a, **kw):
                raise OSError("this band's disk is gone")
            bt.stage3 = broken
        try:
            rec = bands.band_traceback(runner, q0, q1, work, lim, sra_limit=limit)
            q.put((rank, "ok", dict(role=rec["role"], keeper=rec["keeper"], counts=rec["crosspoints"], best=r1["best"],
                                    text=rec.get("text"))))
        except BaseException as e:
            q.put((rank, "raised", "%s: %s" % (type(e).__name__, e)))
    finally:
        dist.destroy_process_group()


def _ranks(work, fail_rank, timeout):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_trace, args=(r, 3, port, work, WEIGHTS[3], SWEEP[2], fail_rank, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(3):
        rank, state, val = q.get(timeout=timeout)
        res[rank] = (state, val)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(300)
def test_the_ranks_leave_the_files_of_the_serial_driver(pkg, oracle, tmp_path):
    """bands.band_traceback over gloo (world 3) after band_stage1: the same areas, so the same files as align_bands' -- every
    crosspoint file of every band, the joined list, crosspoint_04.00, alignment.00.bin and .txt -- and the same keeper on every rank"""
    s0, s1 = _sweep_pair(pkg)
    serial, ranks = str(tmp_path / "serial"), str(tmp_path / "ranks")
    out, limits = _run(pkg, oracle, s0, s1, serial, WEIGHTS[3], "**", SWEEP[2])
    res = _ranks(ranks, None, 240)
    assert all(res[r][0] == "ok" for r in range(3)), res
    assert {res[r][1]["keeper"] for r in range(3)} == {out["keeper"]}
    assert [res[r][1]["role"] for r in range(3)] == [b["role"] for b in out["bands"]]
    assert res[out["keeper"]][1]["text"] == out["text"]
    a, b = bc.tree(serial), bc.tree(ranks)
    a.pop("info")
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    assert all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]][:5]
    bc.judge(pkg, oracle, ranks, s0, s1, limits, "**", None)


@pytest.mark.timeout(120)
def test_a_rank_that_raises_ends_all_ranks(pkg, oracle, tmp_path):
    """band 1's stage 3 fails: it raises its own error, its neighbours on both sides raise ChainFailed naming it, nobody waits"""
    res = _ranks(str(tmp_path / "ranks"), 1, 100)
    assert res[1][0] == "raised" and "OSError" in res[1][1] and "disk is gone" in res[1][1]
    for r in (0, 2):
        assert res[r][0] == "raised" and "ChainFailed" in res[r][1] and "band 1" in res[r][1], res[r]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference, where it is built
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_the_right_most_band_walks_like_the_reference_part(pkg, oracle, tmp_path):
    """MASA-Core as --split=3 --part=1..3 on a global pair of the producer-parity shape, the last part with its traceback: the
    right-most band's crosspoint_02.00 and crosspoint_03.00 are the reference's for part 3, byte for byte"""
    from oracle import binding as ob
    if not ob.have_ref():
        pytest.skip("oracle/_ref/ref_driver not built")
    from masa_cudalign_amd.bands import band_limits, serial_band_stage1
    from masa_cudalign_amd import band_traceback as bt, pipeline
    m, n, limit = PARITY
    s0, s1 = pkg.seqgen.related_pair(m, n, cfg=11, inversion=0.0)
    refdir = str(tmp_path / "ref")
    os.makedirs(refdir)
    args = ["--disk-size=500K", "--no-block-pruning", "--block=256,128", "--edges=++", "--split=3"]
    for k in (1, 2):
        ob.run_ref(s0, s1, args + ["--part=%d" % k, "--stage-1"], workdir=refdir, timeout=300)
    # Part 3 gets a work directory of its own, like a node's: in the one parts 1 and 2 used its stage 2 would walk on into
    # their areas.  The boundary columns travel through files next to the work directories either way; the chain's signal files
    # (the running best of the parts before, <work>/shared) are what a node's stage 1 waits for, so they are copied over.
    import shutil
    shutil.copytree(os.path.join(refdir, "work", "shared"), os.path.join(refdir, "work3", "shared"))
    ob.run_ref(s0, s1, args + ["--part=3", "--work-dir=" + os.path.join(refdir, "work3")], workdir=refdir, timeout=300)
    work = str(tmp_path / "native")
    q0, q1 = bc.fasta_pair(s0, s1)
    al = bc.HostAligner(oracle, 256, 128)
    lim = band_limits(n, [1, 1, 1])
    al.setSequences(s0, s1)
    serial_band_stage1(al, m, lim, work, limit, **pipeline.chain_form(pkg.AT_SEQUENCE_1_AND_2, pkg.AT_SEQUENCE_1_AND_2))
    al.unsetSequences()
    bwork = bt.band_work(work, 2, 3)
    mine, _c = bt.wait_crosspoint(bwork, lim[2], lim[3])
    assert mine
    bt.band_stage2(al, s0, s1, bwork, lim[2], lim[3], (0, m), pkg.AT_SEQUENCE_1_AND_2, limit)
    bt.band_refine(al, s0, s1, bwork, limit)
    for name in ("crosspoint_02.00", "crosspoint_03.00"):
        got = bc.load_points(os.path.join(bwork, "crosspoints", name))
        want = bc.load_points(os.path.join(refdir, "work3", "crosspoints", name))
        diff = [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not diff and len(got) == len(want), (name, "first differing crosspoint", diff[:1], len(got), len(want))
        assert open(os.path.join(bwork, "crosspoints", name), "rb").read() == open(os.path.join(refdir, "work3", "crosspoints", name), "rb").read()


# ---------------------------------------------------------------------------------------------------------------------------
# --trim: the chain covers the selected part of the matrix, every coordinate stays absolute
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_trimmed_chain_keeps_absolute_coordinates(pkg, oracle, tmp_path):
    from masa_cudalign_amd import fasta, pipeline
    from masa_cudalign_amd.bands import band_limits
    s0, s1 = _sweep_pair(pkg)
    t0, t1 = (301, 3700), (201, 3400)                       # --trim=301,3700,201,3400: 1-based, inclusive
    q0 = fasta.parse(b">s0\n" + s0.tobytes() + b"\n", fasta.SequenceModifiers(trim_start=t0[0], trim_end=t0[1]))
    q1 = fasta.parse(b">s1\n" + s1.tobytes() + b"\n", fasta.SequenceModifiers(trim_start=t1[0], trim_end=t1[1]))
    work = str(tmp_path / "w")
    out = pipeline.align_bands(bc.HostAligner(oracle, 128, 128), q0, q1, work, [1, 3, 2], sra_limit=SWEEP[2], block_pruning=False)
    i, j, sc = bc.oracle_optimum(oracle, s0[t0[0] - 1:t0[1]], s1[t1[0] - 1:t1[1]], "**")
    opt = (i + t0[0] - 1, j + t1[0] - 1, sc)
    assert tuple(out["best"]) == opt
    limits = [t1[0] - 1 + x for x in band_limits(t1[1] - t1[0] + 1, [1, 3, 2])]
    seen = bc.judge(pkg, oracle, work, s0, s1, limits, "**", out, optimum=opt)
    assert len(seen["on_boundary"]) == 2
    names = sorted(os.listdir(os.path.join(work, "FORK.01", "special_rows", "stage.01.00")))
    assert names == ["%08X.%08X.%08X.%08X" % (t0[0] - 1, limits[1], t0[1], limits[2])]
