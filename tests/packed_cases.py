"""Inputs and shape lists of tests/test_gpu_packed_family.py (GPU) and tests/test_packed_case_inputs.py (CPU: shows that the
inputs are what they claim).  No GPU here.

The packed 16-bit kernel family (csrc/sw_kernel_pk16.inc, built twenty times: sw_kernel_pk16_{a..j}.hip and the wide-alphabet twins
sw_kernel_pk16_w{a..j}.hip) runs every pair with at most 14 common byte values and, with MI355SW_F_WIDE_ALPHABET, 15 to 62.  Heights
are named by R' = rows_per_lane / 2 (the template argument: rows per 16-bit half), a strip is SH = 128 R' rows.  What is not
packed-specific comes from tests/int32_cases.py."""
import numpy as np

import int32_cases as ic
from int32_cases import (INF, OFFSET, EDGE_FORMS, FOREIGN0, FOREIGN1, LOW_NAMES, GridPair, Part, custom_borders,     # noqa: F401
                         delivered_once, expect_oracle, low_pair, manager_class, related_pair, special_rows, with_alphabet)

F_TWO_PHASE, F_WIDE = 32, 65536                            # MI355SW_F_TWO_PHASE, MI355SW_F_WIDE_ALPHABET (include/mi355sw.h, engine.py)
HEIGHTS = (2, 4, 6, 8, 12, 16)                             # R': 256, 512, 768, 1024, 1536 and 2048-row strips
BATCH_HEIGHTS = (2, 4, 8)                                  # alignPartitions(rows_per_lane = 4, 8, 16)
COLS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 449)
CHUNK = 64
THREADS = 16                                               # oracle threads: never os.cpu_count()

# ACGT first, then what fills the alphabet; '@', '$', '#', '%' (int32_cases.FOREIGN0 / FOREIGN1) are in none of them
POOL = b"ACGTN" + bytes(b for b in b"RYKMSWBDHVEFIJLOPQUXZ" b"abcdefghijklmnopqrstuvwxyz" b"0123456789?")
assert len(POOL) == 63 and len(set(POOL)) == 63 and not set(POOL) & set(FOREIGN0 + FOREIGN1)

# way: (alphabet, flags, wide twin, K = byte values common to both sequences)
#   acgt:     every unmasked chunk is eligible for the table form (one byte permute: all codes in reach < 4)
#   onehot14: all bits 2..15 of the one-hot half-word in use, the foreign codes are 14 / 15; iid letters: the general form everywhere
#   switch:   ACGT and one more common letter, 'N', at column 200 of every seq1 region: the chunks of one strip change between the
#             table form and the general form (SwitchPair)
#   wide15 / wide62: the two ends of the wide range; with K = 62 the seq1-only code is 63, code * 4 = 252 the largest byte of the form
WAYS = {
    "acgt": (b"ACGT", 0, False, 4),
    "onehot14": (POOL[:14], 0, False, 14),
    "switch": (b"ACGT", 0, False, 5),
    "wide15": (POOL[:15], F_WIDE, True, 15),
    "wide62": (POOL[:62], F_WIDE, True, 62),
}
NARROW, WIDE = ("acgt", "onehot14", "switch"), ("wide15", "wide62")
SWITCH_LETTER, SWITCH_COL = ord("N"), 200


def alphabet(way):
    """what the int32_cases generators take in place of one of their own ways"""
    return WAYS[way][0] + (b"N" if way == "switch" else b"")


def flags(way):
    return WAYS[way][1]


def is_wide(way):
    return WAYS[way][2]


# ---------------------------------------------------------------------------------------------------------------------
# the instantiations and the mi355sw_stats.kernel string of each (runtime.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def _b(x):
    return "true" if x else "false"


def strip_name(Rh, track, sw, prune=False, wide=False, goal=False, edge=False):
    return "sw_strip_kernel_pk16%s<%d,%s,%s,%s%s>" % ("_wide" if wide else "", Rh, _b(track), _b(sw), _b(prune),
                                                      ",true" if goal else (",false,true" if edge else ""))


def mixed_name(sw, wide=False):
    return "sw_strip_kernel_pk16_mixed%s<12,11,true,%s>" % ("_wide" if wide else "", _b(sw))


def batch_name(Rh, track, sw, wide=False, goal=False):
    if goal:
        return "sw_batch_kernel_pk16%s<%d,false,false,true,true>" % ("_wide" if wide else "", Rh)
    return "sw_batch_kernel_pk16%s<%d,%s,%s>" % ("_wide" if wide else "", Rh, _b(track), _b(sw))


BAND_NAME = "sw_batch_kernel_pk16%s<4,false,false,true> (the seed's band kernel: reports no name)"


def instantiations(wide):
    """every instantiation one twin's ten translation units contain (the PK16_PART sections at the end of sw_kernel_pk16.inc):
    {group: [names]} -- 24 + 18 + 2 + 12 + 4 + 4 + 1 = 65"""
    out = {
        "strip": [strip_name(R, t, s, False, wide) for R in HEIGHTS for t in (True, False) for s in (True, False)],          # launch16_r<R', false>
        "prune": [strip_name(R, t, s, True, wide) for R in HEIGHTS for t, s in ((True, True), (False, True), (False, False))],  # launch16_r<R', true>
        "mixed": [mixed_name(True, wide), mixed_name(False, wide)],                                                          # part 6
        "batch": [batch_name(R, t, s, wide) for R in BATCH_HEIGHTS for t in (True, False) for s in (True, False)],           # parts 0 and 7
        "goal": [strip_name(2, False, False, True, wide, goal=True), strip_name(4, False, False, True, wide, goal=True),
                 batch_name(2, False, False, wide, goal=True), batch_name(8, False, False, wide, goal=True)],                # part 8
        "edge": [strip_name(R, False, False, True, wide, edge=True) for R in (2, 4, 8, 16)],                                 # part 9
        "band": [BAND_NAME % ("_wide" if wide else "")],                                                                     # part 0
    }
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rows: the emit geometry of a ragged last strip (sw_kernel_pk16.inc, process_strip16: "emitting virtual lane / row")
# ---------------------------------------------------------------------------------------------------------------------
EMIT_V = (0, 1, 2, 63, 64, 126, 127)                       # virtual lanes: lane 0 LO and HI, lane 1, lanes 31 / 32, lane 63 LO and HI


def row_counts(Rh):
    """1, 2, R'-1, R', R'+1, 2R'-1, 2R', 2R'+1 (the LO and the HI block of lane 0); SH-1, SH, SH+1, 2SH-1, 2SH+1; SH + R' v + d for
    v in EMIT_V and d in {0, 1, 2, R'-1, R'}: a ragged second strip whose last valid row is R' v + d - 1 -- row R'-1 of the
    virtual lane above, rows 0, 1, R'-2 and R'-1 of virtual lane v itself; about four and a half strips"""
    SH = 128 * Rh
    rows = [1, 2, Rh - 1, Rh, Rh + 1, 2 * Rh - 1, 2 * Rh, 2 * Rh + 1, SH - 1, SH, SH + 1, 2 * SH - 1, 2 * SH + 1]
    rows += [SH + Rh * v + d for v in EMIT_V for d in (0, 1, 2, Rh - 1, Rh)]
    rows.append(4 * SH + SH // 2 + 3)
    return sorted(set(r for r in rows if r > 0))


def emit_position(Rh, m, row0=None):
    """(ragged, emit_lane, emit_half, emit_row) of the last strip of an m-row partition when its last row is read -- the strip
    starts at row0 (default: strips of one height)"""
    SH = 128 * Rh
    if row0 is None:
        row0 = (m - 1) // SH * SH
    ragged = row0 + SH > m
    emit_v, emit_row = 127, Rh - 1
    if ragged:
        last = m - 1 - row0
        emit_v = last // Rh
        emit_row = last - emit_v * Rh
    return ragged, emit_v >> 1, emit_v & 1, emit_row


# ---------------------------------------------------------------------------------------------------------------------
# columns: which form a chunk takes (sw_kernel_pk16.inc: `masked`, `simple0` .. `simple2`, `use_perm`)
# ---------------------------------------------------------------------------------------------------------------------
def chunk_forms(codes, emit_any=False):
    """per chunk c of a strip over n = len(codes) columns (codes: seq1's codes of the partition's columns): "masked", "table" or
    "general".  The strip takes nchunks = (n + 127 + 63) / 64 chunks; chunk c loads columns 64 c .. 64 c + 63.  It is masked when
    64 c < 127 or 64 c + 63 >= n; simple0 of a chunk: all 64 columns exist and carry codes < 4; the table form needs the chunk
    unmasked, no moved emit position, and simple0 of this chunk and of the two before it -- the columns 64 (c - 2) .. 64 c + 63.
    (The hot loop, c > 256, is not restated: no shape here is that wide.)"""
    n = len(codes)
    nchunks = (n + 127 + CHUNK - 1) // CHUNK
    simple = [64 * c + 64 <= n and bool(np.all(np.asarray(codes[64 * c: 64 * c + 64]) < 4)) for c in range(nchunks)]
    out = []
    for c in range(nchunks):
        if 64 * c - 127 < 0 or 64 * c + 63 >= n:
            out.append("masked")
        elif not emit_any and simple[c] and simple[c - 1] and simple[c - 2]:
            out.append("table")
        else:
            out.append("general")
    return out


class SwitchPair(GridPair):
    """the ACGT grid pair with one more common letter: 'N' at column SWITCH_COL of every seq1 region that is wide enough -- chunk 3
    of a strip, in reach of chunks 3, 4 and 5 -- at the same place of every 300-letter tile of seq0 (the pair stays related
    there), and once behind both sequences: K = 5, 'N' the rarest, so its code is 4"""

    def __init__(self, rows, cols=COLS, kind="iid", seed=0):
        GridPair.__init__(self, b"ACGT", rows, cols, kind, seed)
        self.way = "switch"
        for c in self.cols:
            if c > SWITCH_COL:
                self.s1[self.j0[c] + SWITCH_COL] = SWITCH_LETTER
        for r in self.rows:
            self.s0[self.i0[r] + SWITCH_COL: self.i0[r] + r: ic.BASE] = SWITCH_LETTER
        n = np.array([SWITCH_LETTER], dtype=np.uint8)
        self.s0, self.s1 = np.concatenate([self.s0, n]), np.concatenate([self.s1, n])


def grid_pair(way, rows, cols=COLS, kind="iid", seed=0):
    return SwitchPair(rows, cols, kind, seed) if way == "switch" else GridPair(alphabet(way), rows, cols, kind, seed)


# ---------------------------------------------------------------------------------------------------------------------
# which combinations the GPU file runs
# ---------------------------------------------------------------------------------------------------------------------
def unpruned_grid():
    """test 1: [(wide, R', track, sw, way)] -- the 24 unpruned strip instantiations of each twin; the narrow twin goes round
    acgt / onehot14 / switch and the wide twin round wide15 / wide62, so that each height meets each of them"""
    out = []
    for wide, ways in ((False, NARROW), (True, WIDE)):
        k = 0
        for Rh in HEIGHTS:
            for sw in (True, False):
                for track in (True, False):
                    out.append((wide, Rh, track, sw, ways[k % len(ways)]))
                    k += 1
    return out


def form_of(track, sw):
    """(start, end, quiet): SW tracked; SW through a manager that refuses scores; NW with a global start and the best anywhere; NW to the last cell"""
    if sw:
        return 0, 0, not track
    return (4, 0, False) if track else (4, 4, False)


EDGE_ROWS = lambda Rh: (Rh + 1, 128 * Rh + 1, 128 * Rh + 3 * Rh + 2, 2 * 128 * Rh + 1)   # m < lane, one row into strip two, emit_v 3 (HI) row 1, three strips
EDGE_COLS = (65, 193, 300)


# ---------------------------------------------------------------------------------------------------------------------
# the engine's choice of strip heights, restated (runtime.cpp: step_ns, estimate_ns, pick_rows_per_lane, plan_geometry)
# ---------------------------------------------------------------------------------------------------------------------
STEP_NS = {4: 97, 8: 138, 12: 181, 16: 222, 24: 291, 32: 368}


def estimate_ns(m, n, R, W):
    strips = (m + 64 * R - 1) // (64 * R)
    rounds = (strips + W - 1) // W
    return STEP_NS[R] * (rounds * n + 280.0 * min(strips, W))


def pick_rows_per_lane(m, n, W):
    """unpruned, no special rows, no block scores: the first of the six heights with the smallest estimate"""
    best = 4
    for R in (8, 12, 16, 24, 32):
        if estimate_ns(m, n, R, W) < estimate_ns(m, n, best, W):
            best = R
    return best


def mixed_plan(m, n, W):
    """None, or (strips of 1536 rows, strips in all) of the mixed launch plan_geometry sets up for a tracked run with a zero
    first column, no last column, no special rows, no pruning, rows_per_lane = 0 and waves = W"""
    if pick_rows_per_lane(m, n, W) != 24:
        return None
    strips = (m + 1535) // 1536
    if strips < W:                                         # pick_waves: never more wavefronts than strips
        return None
    rounds = (strips + W - 1) // W
    total = rounds * W
    if rounds > 8 or (total - strips) * 50 < total:
        return None
    na = max(0, -(-(m - total * 1408) // 128))
    if na <= total and na * 1536 + (total - 1 - na) * 1408 < m:
        return na, total
    return None


def mixed_last_strip(m, n, W):
    """(row0, rows it holds) of the last strip of the mixed launch"""
    na, total = mixed_plan(m, n, W)
    row0 = na * 1536 + (total - 1 - na) * 1408
    return row0, m - row0


def stop_borders(m, n, corner, seed):
    """(first row, first column) of the stop test: int32_cases.custom_borders with a walk the packed kernels can follow.  The
    int32 file's borders fall by 3 a cell on average, faster than a gap extends (2): 20 000 rows down, the first column lies
    20 000 under the cells next to it, no 16-bit window holds both, and the packed kernel hands the partition to the int32
    family (restarts = 1 -- seen on the first run of this file).  Here the steps are -4 .. +1, 1.5 down on average: the cells
    beside the column stay within a few hundred of it.  Everything else as there: a corner of its own, gap components 0 to 6
    under H, -INF in a tenth of them."""
    out = []
    for length, sd in ((n, 2 * seed), (m, 2 * seed + 1)):
        rng = np.random.RandomState(sd)
        c = np.zeros((length + 1, 2), dtype=np.int32)
        c[0, 0] = corner
        c[1:, 0] = corner + np.cumsum(rng.randint(-4, 2, length))
        c[:, 1] = c[:, 0] - rng.randint(0, 7, length + 1)
        c[rng.rand(length + 1) < 0.1, 1] = -INF
        c[0] = (corner, -INF)
        out.append(c)
    return out[0], out[1]


def census():
    """per R': how often each (emit_half, emit_row) and each emit_lane occurs over the ragged row counts of more than a strip"""
    out = {}
    for Rh in HEIGHTS:
        pos, lanes = {}, {}
        for m in row_counts(Rh):
            ragged, lane, half, row = emit_position(Rh, m)
            if ragged and m > 128 * Rh:
                pos[(half, row)] = pos.get((half, row), 0) + 1
                lanes[lane] = lanes.get(lane, 0) + 1
        out[Rh] = (pos, lanes)
    return out
