"""Shared helpers for the parity tests."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage1_cases.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def make_pair(pkg, spec):
    """Must stay identical to oracle/make_golden.py:make_pair (the fixtures pin the sha256 of both)."""
    sg = pkg.seqgen
    kind = spec["kind"]
    if kind == "related":
        return sg.related_pair(spec["m"], spec["n"], cfg=spec["cfg"])
    if kind == "unrelated":
        return sg.unrelated_pair(spec["m"], spec["n"], cfg=spec["cfg"])
    if kind == "with_n":
        s0, s1 = sg.related_pair(spec["m"], spec["n"], cfg=spec["cfg"])
        s0, s1 = s0.copy(), s1.copy()
        s0[spec["m"] // 3: spec["m"] // 3 + 50] = ord("N")
        s1[spec["n"] // 3 + 10: spec["n"] // 3 + 70] = ord("N")
        s1[5::97] = ord("R")
        return s0, s1
    if kind == "literal":
        return (np.frombuffer(spec["s0"].encode(), dtype=np.uint8), np.frombuffer(spec["s1"].encode(), dtype=np.uint8))
    raise ValueError(kind)


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return {"len": int(a.shape[0]), "sha256": hashlib.sha256(a.tobytes()).hexdigest(),
            "head": a[:4].tolist(), "tail": a[-4:].tolist()}


def parse_args(args):
    """Reference CLI flags of a fixture -> stage-1 parameters (libmasa.cpp:1054-1103, sw_stage1.cpp:137-161)."""
    edges = "**"
    out = dict(pruning=True, disk=0, block=(1024, 1024), stage1_only=False)
    for a in args:
        if a.startswith("--edges="):
            edges = a[8:10]
        elif a == "--no-block-pruning":
            out["pruning"] = False
        elif a == "--no-flush":
            out["disk"] = -1
        elif a.startswith("--disk-size=") and out["disk"] != -1:
            v = a[12:]
            mult = {"K": 1024, "M": 1024 ** 2, "G": 1024 ** 3}[v[-1]]
            out["disk"] = int(float(v[:-1]) * mult)
        elif a.startswith("--block="):
            h, w = a[8:].split(",")
            out["block"] = (int(h), int(w))
        elif a == "--stage-1":
            out["stage1_only"] = True
    flag = {"*": 0, "1": 1, "2": 2, "3": 3, "+": 4}
    out["start"], out["end"] = flag[edges[0]], flag[edges[1]]
    return out


def flush_interval(m, n, limit):
    """Job::calculateFlushIntervals, M/common/Job.cpp:231-241 (first interval only)."""
    if limit <= 0:
        return 0
    if limit < n * 8 * 2:
        limit = n * 8 * 2
    return int(m * n * 8 // limit + 1)


def oracle_kwargs(oracle, p, m, n):
    """stage-1 set-up of sw_stage1.cpp:137-161/:318-322/:219-225 expressed as oracle.stage1 arguments."""
    start, end = p["start"], p["end"]
    kw = dict(block_h=p["block"][0], block_w=p["block"][1])
    kw["recurrence"] = oracle.SMITH_WATERMAN if start == 0 else oracle.NEEDLEMAN_WUNSCH
    Z, G = oracle.INIT_WITH_ZEROES, oracle.INIT_WITH_GAPS
    kw["first_row_type"], kw["first_col_type"] = {0: (Z, Z), 1: (Z, G), 2: (G, Z), 3: (Z, Z), 4: (G, G)}[start]
    kw["best_mode"] = {0: oracle.BEST_ANYWHERE, 1: oracle.BEST_LAST_ROW, 2: oracle.BEST_LAST_COL,
                       3: oracle.BEST_LAST_ROW_OR_COL, 4: oracle.BEST_LAST_CELL}[end]
    kw["want_last_row"] = end in (1, 3)
    kw["want_last_col"] = end in (2, 3)
    kw["pruning"] = p["pruning"] and end == 0
    kw["special_row_interval"] = flush_interval(m, n, p["disk"])
    if kw["special_row_interval"]:
        kw["want_last_row"] = True     # SpecialRowsPartition always hands out a last-row writer
    return kw


def oracle_full(oracle, seq0, seq1, edge=0, special_row_interval=8192, block_h=1024):
    """the oracle's whole-matrix answer for the larger GPU parity cases -- best cell, last row, last column, special rows every
    `special_row_interval` rows -- on every host core (oracle_stage1_mt: the same cells as the serial schedule, pinned on it by
    tests/test_oracle_golden.py::test_threaded_oracle_equals_the_serial_one).  edge: 0 = local (**), 4 = global (++).
    block_h: the oracle hands out special rows at block boundaries -- an interval that is no multiple of 1024 needs a block
    height that divides it."""
    m, n = len(seq0), len(seq1)
    kw = oracle_kwargs(oracle, dict(start=edge, end=edge, pruning=False, disk=-1, block=(block_h, 1024)), m, n)
    kw.update(want_last_row=True, want_last_col=True, special_row_interval=special_row_interval, threads=min(64, os.cpu_count() or 1))
    return oracle.stage1(seq0, seq1, **kw)


MATCH = 1                       # the reference's score of a matching pair (DNA_MATCH; oracle/sw_oracle.h: OC_MATCH)
INF = 999999999
NEEDLEMAN_WUNSCH, SMITH_WATERMAN = 0, 1


def assert_pruned_cells(got, want, i, j, m, n, goal, recurrence, *, lower_bound=True, where=""):
    """Which cells a block-pruned run owes exactly -- the one statement every pruned-run test goes through.

    got, want: (k, 2) int32 cells (H and the gap component) of the pruned run and of the unpruned oracle; i, j: their
    1-based DP coordinates in the WHOLE m x n matrix (scalars broadcast; column 0 / row 0 are coordinate 0).

    local (SMITH_WATERMAN), goal = the final best score: AbstractBlockPruning::isBlockPrunable
    (M/libmasa/pruning/AbstractBlockPruning.cpp:70-111) skips when score + min(rows left, columns left) * match <= best.
    Per cell: reach = min(m - i, n - j) * MATCH; a true value v -- H or a gap component -- may differ only if
    v + reach <= goal; every other value must equal the oracle's.  The rule is closed under dependence (a value that can
    only be derived through a legally skipped cell is itself exempt), so it needs no knowledge of what the engine skipped.

    global (NEEDLEMAN_WUNSCH), goal = H[m][n]: a value must be exact if v + min(di, dj) - 2 |dj - di| >= goal (every
    diagonal step a match, the forced gap at its extension price), on H and with the same bound on the gap component.

    Values at or below -INF / 2 (the void F of a first-column cell) are never "must".  lower_bound=True (the engine: skipped
    cells hold lower bounds) also asks got <= want everywhere and, for local runs, got.h >= 0.
    Returns (n_must, n_differing): how many values had to be equal, and how many values differ at all."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.ndim == 2 and got.shape[1] == 2, (where, got.shape, want.shape)
    k = got.shape[0]
    i = np.broadcast_to(np.asarray(i, dtype=np.int64), (k,))
    j = np.broadcast_to(np.asarray(j, dtype=np.int64), (k,))
    assert np.all((0 <= i) & (i <= m) & (0 <= j) & (j <= n)), where
    g, w = got.astype(np.int64), want.astype(np.int64)
    di, dj = m - i, n - j
    if recurrence == SMITH_WATERMAN:
        reach = np.minimum(di, dj) * MATCH
        must = w + reach[:, None] > goal
    elif recurrence == NEEDLEMAN_WUNSCH:
        reach = np.minimum(di, dj) * MATCH - 2 * np.abs(dj - di)
        must = w + reach[:, None] >= goal
    else:
        raise ValueError(recurrence)
    must &= w > -INF // 2
    bad = must & (g != w)
    if lower_bound:
        bad |= g > w
        if recurrence == SMITH_WATERMAN:
            bad[:, 0] |= g[:, 0] < 0
    if bad.any():
        idx = np.argwhere(bad)
        first = [(int(i[r]), int(j[r]), "HG"[c], int(g[r, c]), int(w[r, c]), int(w[r, c] + reach[r]), int(goal)) for r, c in idx[:8]]
        raise AssertionError("%s: %d offending values of %d (%d must be equal); first (i, j, component, got, want, want + reach, goal): %s"
                             % (where, len(idx), 2 * k, int(must.sum()), first))
    return int(must.sum()), int((g != w).sum())


def assert_pruned_borders(rows, last_row, last_col, ref, m, n, goal, recurrence, *, col0, must_rows_upto=0, lower_bound=True, where=""):
    """everything a pruned run over the whole m x n matrix handed out, through assert_pruned_cells against the unpruned
    oracle result `ref`: rows = {dp row: cells}, last_row, last_col (None = not kept).  col0: the arrays start at coordinate 0
    (Stage1Manager: n + 1 / m + 1 cells) or at 1 (the stream: n / m cells).  Every special row with 0 < i <= must_rows_upto
    (local: the best cell's row -- the optimal path crosses it; global: m) must have at least one must-value.
    Returns the number of must-values over all of it."""
    off = 0 if col0 else 1
    want_rows = dict(zip(ref.get("special_row_ids") or [], ref["special_rows"] if ref.get("special_rows") is not None else []))
    total = 0
    for i in sorted(rows):
        if i not in want_rows:                  # (a manager keeps the last row under its row number too)
            assert i == m and last_row is not None, (where, i)
            continue
        n_must, _ = assert_pruned_cells(rows[i], want_rows[i][off:], i, np.arange(off, n + 1), m, n, goal, recurrence,
                                        lower_bound=lower_bound, where="%s row %d" % (where, i))
        if i <= must_rows_upto:
            assert n_must > 0, "%s row %d: nothing to hold the run to" % (where, i)
        total += n_must
    if last_row is not None:
        total += assert_pruned_cells(last_row, ref["last_row"][off:], m, np.arange(off, n + 1), m, n, goal, recurrence,
                                     lower_bound=lower_bound, where=where + " last row")[0]
    if last_col is not None:
        total += assert_pruned_cells(last_col, ref["last_col"][off:], np.arange(off, m + 1), n, m, n, goal, recurrence,
                                     lower_bound=lower_bound, where=where + " last column")[0]
    return total


def manager_rows(mg):
    return {i: mg.specialRow(i) for i in sorted(mg.special_rows)}


def engine_ref(rows, last_row, last_col, *, col0):
    """an UNPRUNED engine run in the shape of an oracle result, for the sizes no oracle run is affordable at (the check is then
    engine against engine: it pins what pruning changed, not the recurrence)"""
    def pad(a):
        return None if a is None else (a if col0 else np.concatenate([np.zeros((1, 2), dtype=np.int32), a]))
    ids = sorted(rows)
    return {"special_row_ids": ids, "special_rows": [pad(rows[i]) for i in ids], "last_row": pad(last_row), "last_col": pad(last_col)}
