// MI355X (gfx950 / CDNA4) Stage-1 affine-gap SW/NW strip-wavefront kernel.
//
// Replaces the reference's device code (X/CUDAligner.cu: kernel_long_phase :941-1007,
// kernel_short_phase :745-824, kernel_single_phase :1100-1156, kernel_sw :276-289,
// kernel_check_max4 :396-410, kernel_load :441-459, kernel_flush :502-540) with a
// from-scratch design for 64-lane wavefronts:
//
//   * one wavefront owns a STRIP of 64*R consecutive DP rows (lane k: rows k*R..k*R+R-1, all
//     state in VGPRs) and sweeps it left->right over the whole partition width; lane k is k
//     columns behind lane k-1 (systolic skew), so every step each lane computes R cells of one
//     column and hands its bottom (H,F) to lane k+1 with a single DPP wave_shr:1 move;
//   * the horizontal bus row (H,F per column, HBM) is read in coalesced 64-column chunks,
//     staged through LDS and fed to lane 0; lane 63's outputs are collected in LDS and written
//     back in coalesced chunks (in place: a strip overwrites the bus row it consumed);
//   * strips are claimed dynamically (atomic ticket) by persistent wavefronts; strip s+1
//     follows strip s through a per-strip progress counter (write-through sc1 stores + drained
//     flag, MI355X_MICROARCH.md "Valid forms") -- no kernel launch per external diagonal;
//   * arithmetic is kept in the "t = H - (open+ext)" domain so that one subtraction per cell
//     feeds both E of the right neighbour and F of the lower neighbour, the substitution score
//     is one v_bfe_i32 from a per-row 8x4-bit profile register, H is v_max3 + v_max, and the
//     running best is folded with v_max3 -- ~9.5 int32 VALU ops per SW cell.
//
// Recurrence (bit-identical to CPUBlockProcessor.cpp:66-93 and CUDAligner.cu:276-289):
//   E = max(Hleft-3, Eleft)-2 ; F = max(Hup-3, Fup)-2 ; v = Hdiag + (c0!=c1 ? -3 : +1)
//   H = SW ? max(0,v,E,F) : max(v,E,F)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_kernel.h"

namespace mi355sw {

#define DBG(k, v) do { if (a->dbg != nullptr && lane == 0) st_agent(&a->dbg[k], (v)); } while (0)

#define GAP_FIRST 5   // DNA_GAP_OPEN + DNA_GAP_EXT (CUDAligner.hpp:92-98)
#define GAP_EXT 2
#define NEG_INF (-999999999)   // libmasaTypes.hpp:46

typedef unsigned int u32;
typedef __attribute__((address_space(1))) int gint;
typedef __attribute__((address_space(1))) unsigned long long gu64;

__device__ __forceinline__ int wave_shr1(int old, int src) {
    // lane k <- src of lane k-1 ; lane 0 keeps `old` (DPP wave_shr:1, bound_ctrl off)
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int max3(int a, int b, int c) {
    return max(max(a, b), c);   // folds to v_max3_i32
}
__device__ __forceinline__ int ld_agent(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int2 ld_agent2(const int2* p) {
    unsigned long long x = __hip_atomic_load((const unsigned long long*) p, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
    return make_int2((int) (u32) x, (int) (u32) (x >> 32));
}
__device__ __forceinline__ void st_agent2(int2* p, int2 v) {
    unsigned long long x = ((unsigned long long) (u32) v.y << 32) | (u32) v.x;
    __hip_atomic_store((unsigned long long*) p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave-uniform polls: the loaded word is the same in every lane; readfirstlane tells the compiler so
// (scalar branches instead of EXEC-masked loops)
__device__ __forceinline__ int poll_agent(const int* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int poll_sys(const int* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
__device__ __forceinline__ int ld_sys(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ int2 ld_sys2(const int2* p) {
    unsigned long long x = __hip_atomic_load((const unsigned long long*) p, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM);
    return make_int2((int) (u32) x, (int) (u32) (x >> 32));
}

// Per-wave LDS staging area (all values in the t = H-5 domain).
struct __attribute__((aligned(16))) WaveLds {
    int2 in_tf[CHUNK + 1];    // (t,F) of the row above, columns [64c, 64c+64) (+1: prefetch slot)
    int2 out_tf[CHUNK];       // (t,F) of the emit row, written by the emit lane at step u
    unsigned char c1[2 * CHUNK + 8];   // seq1 shift codes: [0,64) previous chunk, [64,128) current
    int red[3 * 64];          // strip-end best reduction
};

template <int R>
struct LaneState {
    int tl[R];      // t (= H-5) of the cell to the left, per row
    int e[R];       // E of the cell to the left, per row
    int prof[R];    // PROFILE: 8 nibbles (c1 code -> score+5) ; else raw seq0 byte
    int tup_prev;   // t of (row above, previous column)
    int tbot, fbot; // bottom (t,F) produced at the previous step
    int best_t, best_r, best_j;
};

// One systolic step: every lane advances one column.  `u` is the step index inside the chunk.
template <int R, bool SW, bool PROFILE, bool MASKED, bool TRACK, bool EMIT_ANY, bool CMAX = false>
__device__ __forceinline__ void wave_step(LaneState<R>& st, WaveLds* lds, const int u, const int lane,
                                          const int jl /* column of this lane at u=0 */, const int n,
                                          const int nvalid, const int emit_lane, const int emit_row,
                                          int2& feed_io, int& c1_io, int* cmax = nullptr) {
    // ---- hand-off from the lane above (full EXEC); LDS reads are software-pipelined by one step ----
    const int2 feed = feed_io;                             // (t,F) of the row above: lane 0 only
    const int c1 = c1_io;
    feed_io = lds->in_tf[u + 1];                           // broadcast read for the next step
    c1_io = lds->c1[CHUNK + u + 1 - lane];
    const int tup = wave_shr1(feed.x, st.tbot);
    const int fup = wave_shr1(feed.y, st.fbot);

    bool active = true;
    if (MASKED) active = (u32) (jl + u) < (u32) n;
    if (active) {
        int diag = st.tup_prev;
        int upt = tup, upf = fup;
        int t_emit = 0, f_emit = 0;
        int mx = NEG_INF, tprev = NEG_INF;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int E = max(st.tl[r], st.e[r] - GAP_EXT);
            const int F = max(upt, upf - GAP_EXT);
            int v;
            if (PROFILE) {
                v = diag + __builtin_amdgcn_sbfe(st.prof[r], c1, 4);   // score+5 in {2,6}
            } else {
                v = diag + ((st.prof[r] != c1) ? 2 : 6);
            }
            int h = max3(v, E, F);
            if (SW) h = max(h, 0);
            const int t = h - GAP_FIRST;
            diag = st.tl[r];
            st.tl[r] = t;
            st.e[r] = E;
            upt = t;
            upf = F;
            if (TRACK || CMAX) { if (r & 1) mx = max3(mx, tprev, t); tprev = t; }
            if (EMIT_ANY) {
                t_emit = (r == emit_row) ? t : t_emit;
                f_emit = (r == emit_row) ? F : f_emit;
            }
        }
        if ((TRACK || CMAX) && (R & 1)) mx = max(mx, tprev);
        if (CMAX) *cmax = max(*cmax, mx);                   // the lane's maximum over the chunk (block pruning: what it can hand on)
        st.tup_prev = tup;
        st.tbot = upt;
        st.fbot = upf;
        if (!EMIT_ANY) { t_emit = upt; f_emit = upf; }
        if (lane == emit_lane) lds->out_tf[u] = make_int2(t_emit, f_emit);

        if (TRACK) {
            // rare path: exact canonical (max score, min i, min j) bookkeeping
            if (__any(mx >= st.best_t)) {
                const int j = jl + u;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int t = st.tl[r];
                    const bool upd = (r < nvalid) && ((t > st.best_t) || (t == st.best_t && r < st.best_r));
                    st.best_t = upd ? t : st.best_t;
                    st.best_r = upd ? r : st.best_r;
                    st.best_j = upd ? j : st.best_j;
                }
            }
        }
    }
}

// PRUNE (round 5; local alignments): block pruning in the int32 family too -- the reference prunes in every instantiation of
// its kernels (X/CUDAligner.cu:950-960); here a 64-step slab of the strip is skipped when nothing that enters it (the lanes'
// chunk maxima, the bus cells above it) can still reach the running best, exactly the packed kernel's local test
// (sw_kernel_pk16.inc, SW_PRUNE_MARGIN included).  Skipped cells read H = 0, E = F = -INF.  This family takes the pairs the
// packed kernel cannot (more than 14 common byte values) and its reruns.  By itself a strip walks the whole width slab by slab;
// window, retire and fast-forward are the WINDOW instantiations' (opt-in, MI355SW_F_INT32_WINDOW: see process_strip).
#define SW32_PRUNE_MARGIN 8
// PRUNE && !SW (global alignments; opt-in, MI355SW_F_INT32_PRUNE_GLOBAL): the packed family's last-cell rule (DESIGN.md
// section 4, "Global"; AbstractBlockPruning.cpp:92-109) on int32 values, slab by slab.  gbest holds a running LOWER bound of
// H[m][n] - GAP_FIRST of the super-partition; dI / dJ below are a cell's rows / columns to that cell.
//   * every computed slab of full rows and columns contributes nw_lower32 of each lane's chunk maximum;
//   * a slab goes when nw_upper32 of everything that enters it -- each lane's lane_entry, the bus cells above -- is below it
//     (strict: ties are kept);
//   * skipped cells read H = E = F = -INF; a lane that holds nothing (t <= NEG_INF / 2) enters nothing;
//   * what a lane carries over a chunk boundary and every cell stored is clamped at -INF (clamp_void32): next to skipped
//     cells a computed cell sinks by up to 5 per step, and the clamp bounds that to one slab ("No wrap").
// The margin is the packed family's NW_PRUNE_MARGIN, not SW32_PRUNE_MARGIN: what enters a slab through its corner -- the bus
// cell diagonally above its first cell, the bottom cell of the lane above one column back -- is within one step (5) of a
// value the test does look at, and one cell of position moves this bound by up to 3 where the local bound moves by 1; 16
// covers 5 + 2 * 3 with room, and with the same margin the two families' skip counts can be held against each other.
#define NW32_PRUNE_MARGIN 16
// Upper bound (t domain) of the last cell's score over every path through a cell that holds at most `t` and has between
// di - si and di rows and between dj - sj and dj columns to go: every diagonal step a match, the gap that the imbalance
// forces at its extension price (the cell may sit inside an open gap).  The position terms are the most favourable of the span.
__device__ __forceinline__ int nw_upper32(const int t, const int di, const int dj, const int si, const int sj) {
    if (t <= NEG_INF / 2) return NEG_INF - 1;             // nothing enters here: below every lower bound, known or not
    const int dlo = dj - sj - di, dhi = dj - di + si;      // range of (columns left - rows left) over the cells
    const int dmin = min(max(0, max(dlo, -dhi)), 400000000);   // (int32 headroom; a weaker bound, never a wrong one)
    return t + min(di, dj) - 2 * dmin + NW32_PRUNE_MARGIN;
}
// Lower bound (t domain) of the last cell's score from a cell that holds `t`, a score some path really reaches, wherever it
// lies among cells with at most `kmax` diagonal steps to go and an imbalance of at most `dmax`: mismatches down the diagonal,
// then one gap (dec = distMin * -mismatch + gap_open + gaps * gap_ext).  The position terms are the least favourable of the span.
__device__ __forceinline__ int nw_lower32(const int t, const long long kmax, const long long dmax) {
    const long long lb = (long long) t - 3 * kmax - 3 - 2 * dmax;
    return lb > (long long) NEG_INF ? (int) lb : NEG_INF;
}
// EDGE (opt-in, MI355SW_F_INT32_PRUNE_EDGE_GOAL; KernelArgs::prune_end 1: the alignment ends anywhere on the last row, 2: anywhere
// on the last column, 3: on either): edge_upper16 / edge_lower16 of sw_kernel_pk16.inc on int32 values with this family's spans.
// Everything is the global rule's -- gbest a running lower bound, here of the best H on the named edge(s) minus GAP_FIRST; where
// the bounds are folded; -INF for skipped cells; the clamps -- except the gap the rest of a path is forced to hold: to end on the
// last row it only has to get DOWN, g = max(0, di - dj); on the last column ACROSS, g = max(0, dj - di); on either, none.
__device__ __forceinline__ int edge_upper32(const int end, const int t, const int di, const int dj, const int si, const int sj) {
    if (t <= NEG_INF / 2) return NEG_INF - 1;             // nothing enters here: below every lower bound, known or not
    const int dlo = dj - sj - di, dhi = dj - di + si;      // range of (columns left - rows left) over the cells
    const int gmin = min(end == 1 ? max(0, -dhi) : (end == 2 ? max(0, dlo) : 0), 400000000);   // the least forced gap among them
    return t + min(di, dj) - 2 * gmin + NW32_PRUNE_MARGIN;
}
// mismatches down the diagonal to the nearer edge, at most `kmax` steps, and -- only where that edge is not one the alignment may
// end on -- one gap along it; dlo .. dhi: range of (columns left - rows left) over the cells the maximum may lie in
__device__ __forceinline__ int edge_lower32(const int end, const int t, const long long kmax, const long long dlo, const long long dhi) {
    const long long gmax = end == 1 ? -dlo : (end == 2 ? dhi : 0);   // the largest forced gap among them
    const long long lb = (long long) t - 3 * kmax - (gmax > 0 ? 3 + 2 * gmax : 0);
    return lb > (long long) NEG_INF ? (int) lb : NEG_INF;
}
// GOAL (the same flag; KernelArgs::goal_bound_col / _row, t domain, constants of the sweep): goal_keep16 on int32 values.  A cell
// that holds t with dj columns left reaches the last column with at most t + dj, and the last row with at most
// t + min(di, dj) - 2 * (di - dj) when it has more rows left than columns.  `t` bounds cells whose rows-left lie in [di - si, di]
// and whose columns-left are at most dj; a term that is off sits out of every value's reach.  (64-bit: t + dj need not fit.)
__device__ __forceinline__ bool goal_keep32(const int t, const int di, const int dj, const int si, const long long gcol, const long long grow) {
    if (t <= NEG_INF / 2) return false;                   // nothing enters here
    const long long ucol = (long long) t + dj + NW32_PRUNE_MARGIN;
    const long long surplus = (long long) di - si - dj;   // the least (rows left - columns left) among the cells
    const long long urow = (long long) t + min(di, dj) - 2 * (surplus > 0 ? surplus : 0) + NW32_PRUNE_MARGIN;
    return ucol >= gcol || urow >= grow;
}
// a lane's state at a chunk boundary, -INF images pulled back up to -INF (t domain: -INF - GAP_FIRST)
template <int R>
__device__ __forceinline__ void clamp_void32(LaneState<R>& st) {
#pragma unroll
    for (int r = 0; r < R; r++) { st.tl[r] = max(st.tl[r], NEG_INF - GAP_FIRST); st.e[r] = max(st.e[r], NEG_INF); }
    st.tup_prev = max(st.tup_prev, NEG_INF - GAP_FIRST);
    st.tbot = max(st.tbot, NEG_INF - GAP_FIRST);
    st.fbot = max(st.fbot, NEG_INF);
}
// WINDOW (opt-in, MI355SW_F_INT32_WINDOW; every pruning instantiation has a windowed twin): the packed family's pruning window
// (sw_kernel_pk16.inc, "the pruning WINDOW") without gap words -- this family has no band mode, so nothing ever jumps.
//   a. the predecessor's last progress word is WIN_RETIRED + X (sw_kernel.h): from output column X on its row is the skip
//      constant, written or not, and the chunk head substitutes the constant for whatever bus[col >= X] holds;
//   b. the trailing chunks of a non-ragged strip (col0 + CHUNK > n) go through the slab test too, with the same entries: bus
//      cells at col >= n enter nothing, and a lane that has passed column n - 1 (jl >= n) is no entry and keeps its state --
//      tl / e are its final last-column cells, which the epilogue hands out;
//   c. void_from is the first output column from which everything the strip has left is the constant (a computed chunk resets
//      it).  The strip RETIRES at a chunk whose test says skip when the slab before was skipped (its state is the skip state) and
//      the predecessor's X <= col0 (nothing but the constant enters from above, for good): the local test is monotone in the
//      column and gbest only grows, a global strip in that state holds nothing and nothing enters.  It leaves the chunk loop,
//      counts the slabs it did not walk as pruned, writes its last column from its state and publishes WIN_RETIRED + void_from.
//      A strip that walks to the end publishes WIN_RETIRED + min(void_from, n) with its last chunk; a ragged strip never retires.
//   d. FAST-FORWARD: after a skipped slab the strip's state is a constant, so the test of the slabs that follow depends on the bus
//      cells above them alone (after substitution a).  From chunk 3 on, up to SW32_FF full slabs the predecessor has ALREADY
//      published (one look at its word, no wait) are fetched and tested in one go, with gseen as it stood at the first; the
//      leading run that can go is written out together -- the bus cells, with the emit lag; special rows and the last row hold the
//      constant already -- with one drain and one progress flag, pruned_slabs rises by the run, and the seq1 codes of the last
//      slab of the run are staged for the chunk that follows.  Decisions, cells and counts are those of slab by slab.
// No new wait: the poll is the existing one with its spin_limit, and a retired predecessor's word satisfies it.  Rows that leave
// the device (special rows, the last row) are pre-filled with the constant by the host (mi355sw_stream_begin).
// WINDOW is the last parameter and defaults to false: every instantiation named without it is the kernel it was under
//   template <int R, bool SW, bool PROFILE, bool TRACK, bool PRUNE = false, bool GOAL = false, bool EDGE = false>
// (every `if (WINDOW)` below folds away; the parent's register, scratch and instruction counts per kernel are kept: CHANGELOG.md).
#define SW32_FF 16     // slabs per fast-forward batch
#define SW32_FFB 4     // ... fetched SW32_FFB at a time
// the slab test of a strip in the skip state (fast-forward): what enters is the bus cell above alone -- `top_h` its H, column `col`
// of the slab that starts at `col0`; the lane itself holds the constant (local: t = -GAP_FIRST) or nothing (global)
template <bool SW, bool GOAL, bool EDGE>
__device__ __forceinline__ bool void_slab_goes32(const int top_h, const int col0, const int col, const int pr_rows, const int pr_cols, const int gseen,
                                                 const int prune_end, const long long gcol, const long long grow, const bool goal_any) {
    if (SW) {
        const int left = min(pr_rows + 2, pr_cols + 1 - (col0 - CHUNK));
        const int e = max(-GAP_FIRST, top_h - GAP_FIRST);
        return !__any(e + left + SW32_PRUNE_MARGIN >= gseen);
    }
    if (GOAL) return goal_any && !__any(goal_keep32(top_h - GAP_FIRST, pr_rows + 1, pr_cols - col + 1, 0, gcol, grow));
    const int top = EDGE ? edge_upper32(prune_end, top_h - GAP_FIRST, pr_rows + 1, pr_cols - col + 1, 0, 1)
                         : nw_upper32(top_h - GAP_FIRST, pr_rows + 1, pr_cols - col + 1, 0, 1);
    return !__any(top >= gseen);
}
template <int R, bool SW, bool PROFILE, bool TRACK, bool PRUNE = false, bool GOAL = false, bool EDGE = false, bool WINDOW = false>
__device__ __attribute__((noinline)) void process_strip(const KernelArgs* ap, const int s_in, WaveLds* lds, const int lane) {
    constexpr bool NWP = PRUNE && !SW;                  // the global (last-cell) rule, and its two variants:
    static_assert(!GOAL || (PRUNE && !SW && !TRACK), "goal mode: global recurrence, pruning kernels, nothing tracked");
    static_assert(!EDGE || (PRUNE && !SW && !TRACK && !GOAL), "edge mode: global recurrence, pruning kernels, nothing tracked, no goal");
    static_assert(!WINDOW || PRUNE, "the window: pruning kernels only");
    const UniformArgs a = uniform_args(ap);
    const int s = __builtin_amdgcn_readfirstlane(s_in);
    const int n = a->n;
    const int SH = 64 * R;
    const int nchunks = (n + 63 + CHUNK - 1) / CHUNK;
    const int row0 = a->strip_row0 + s * SH;          // first DP row of this strip (0-based)
    const int lrow0 = row0 + lane * R;                // first row of this lane
    const int rows_left = a->m - lrow0;
    const int nvalid = rows_left < 0 ? 0 : (rows_left > R ? R : rows_left);
    const int* prog_in = &a->progress[s];              // progress of the strip above
    // wait budget of the in-kernel polls: a band fed by another GPU may legitimately stand still for as long as
    // its first column takes to arrive (the first strip waits on the host counter, all others on that strip)
    const int spin_limit = a->first_col_ready != nullptr ? (1 << 30) : (1 << 24);
    int* prog_out = &a->progress[s + 1];

    // which (lane,row) is the row handed to the next strip / flushed as special row
    int emit_lane = 63, emit_row = R - 1;
    const bool ragged = (row0 + SH > a->m);
    if (ragged) {
        const int last = a->m - 1 - row0;              // last valid row inside the strip
        emit_lane = last / R;
        emit_row = last - emit_lane * R;
    }
    const bool last_strip = (row0 + SH >= a->m);
    int2* special = nullptr;
    if (a->special_interval_strips > 0 && a->special_rows != nullptr) {
        const int sg = a->strip_index0 + s + 1;       // strips completed once this one ends
        if (sg % a->special_interval_strips == 0 && (long long) sg * SH < a->m)
            special = a->special_rows + (long long) (sg / a->special_interval_strips - 1) * a->special_pitch;
    }
    int2* lastrow = (last_strip && a->last_row != nullptr) ? a->last_row : nullptr;

    // ---- per-lane state from the first column (InitialCellsReader semantics on device) ----
    // (a column delivered from outside has been awaited in claim_strip_common)
    LaneState<R> st;
#pragma unroll
    for (int r = 0; r < R; r++) {
        int h = 0, e = NEG_INF;
        if (a->first_col != nullptr) {
            const int g = lrow0 + r;
            if (g < a->m) {
                const int2 c = ld_sys2(&a->first_col[g + 1]);
                h = c.x; e = c.y;
            }
        }
        st.tl[r] = h - GAP_FIRST;
        st.e[r] = e;
        const int g = lrow0 + r;
        const int c0 = (g < a->m) ? (int) a->seq0[g] : a->pad_code;
        if (PROFILE) {
            // nibble k = score(c0, code k) + 5 : 6 on match, 2 otherwise; pad/foreign codes never match
            u32 p = 0x22222222u;
            if (c0 < a->n_match_codes) p += (4u << (4 * c0));
            st.prof[r] = (int) p;
        } else {
            st.prof[r] = c0 << a->seq0_shift;
        }
    }
    {
        int hd = 0;
        if (a->first_col != nullptr && lrow0 <= a->m) hd = ld_sys2(&a->first_col[lrow0]).x;
        st.tup_prev = hd - GAP_FIRST;
    }
    st.tbot = NEG_INF; st.fbot = NEG_INF;
    st.best_t = NEG_INF; st.best_r = R; st.best_j = -1;
    // block pruning: what the lane holds, bounded from above (t domain); the running best as of the last look
    int lane_entry = NEG_INF, gseen = NEG_INF, pruned_slabs = 0;
    if (PRUNE) {
#pragma unroll
        for (int r = 0; r < R; r++) lane_entry = max(lane_entry, st.tl[r]);
    }
    const int pr_rows = PRUNE ? a->prune_rows - 1 - row0 : 0, pr_cols = PRUNE ? a->prune_cols - 1 : 0;
    // goal mode: the two bounds, a term that is off (-INF in the argument block) out of every value's reach; edge mode: which edge(s)
    const int goal_c = GOAL ? a->goal_bound_col : NEG_INF, goal_r = GOAL ? a->goal_bound_row : NEG_INF;
    const long long gcol = goal_c <= NEG_INF / 2 ? 0x7fffffffffffffffll : (long long) goal_c;
    const long long grow = goal_r <= NEG_INF / 2 ? 0x7fffffffffffffffll : (long long) goal_r;
    const bool goal_any = goal_c > NEG_INF / 2 || goal_r > NEG_INF / 2;
    const int prune_end = EDGE ? a->prune_end : 0;
    // the window: the predecessor's X once its last word has been seen, this strip's own void_from, whether the slab before went
    int pred_x = 0x7fffffff, void_from = 0x7fffffff;
    bool prev_skip = false, retired = false;
    int ff_block = -1;                 // the chunk a fast-forward ended in front of: it takes the ordinary path

    DBG(1, 1);
    // ---- sweep the strip ----
    for (int c = 0; c < nchunks; c++) {
        const int col0 = c * CHUNK;
        bool skip = false;
        DBG(2, c); DBG(3, 10);
        // (0) window, fast-forward: the state is the skip state -- a run of slabs the strip above has already published goes in one step
        if (WINDOW && prev_skip && !ragged && c >= 3 && c != ff_block && pred_x > col0) {
            const int pv = poll_agent(prog_in);
            if (pv >= WIN_RETIRED) pred_x = pv - WIN_RETIRED;
            const int avail = min(pv >= WIN_RETIRED ? n : pv, n);
            const int K = min((avail - col0) / CHUNK, (int) SW32_FF);       // full slabs ready above
            if (K >= 2) {
                if (!GOAL) gseen = max(gseen, poll_agent(a->gbest_in));
                int run = 0;
                // (SW32_FFB loads in flight at a time: the registers of R = 4 / 8 leave room for no more next to a strip's state)
#pragma unroll 1
                for (int g = 0; g < K && run == g; g += SW32_FFB) {
                    int tops[SW32_FFB];
#pragma unroll
                    for (int k = 0; k < SW32_FFB; k++) {
                        tops[k] = 0;
                        if (g + k < K) tops[k] = ld_agent((const int*) &a->bus[col0 + (g + k) * CHUNK + lane]);
                    }
#pragma unroll
                    for (int k = 0; k < SW32_FFB; k++) {
                        if (g + k == run && g + k < K) {
                            const int colk = col0 + (g + k) * CHUNK + lane;
                            const int top_h = colk >= pred_x ? (NWP ? NEG_INF : 0) : tops[k];
                            if (void_slab_goes32<SW, GOAL, EDGE>(top_h, col0 + (g + k) * CHUNK, colk, pr_rows, pr_cols, gseen, prune_end, gcol, grow, goal_any)) run = g + k + 1;
                        }
                    }
                }
                run = __builtin_amdgcn_readfirstlane(run);
                if (run > 0) {
                    const int2 cell = NWP ? make_int2(NEG_INF, NEG_INF) : make_int2(0, NEG_INF);
#pragma unroll 1
                    for (int k = 0; k < run; k++) st_agent2(&a->bus[col0 + k * CHUNK - 63 + lane], cell);
                    const int last0 = col0 + (run - 1) * CHUNK;
                    lds->c1[CHUNK + lane] = a->seq1[last0 + lane];      // what the next chunk shifts down as "the chunk before"
                    pruned_slabs += run;
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (drain, then flag: as below)
                    if (lane == 0) st_agent(prog_out, last0 + 1);
                    c += run - 1;
                    ff_block = c + 1;
                    continue;
                }
            }
            ff_block = c;
        }
        // (1) input chunk: wait for the strip above, then stage bus + seq1 codes into LDS
        {
            int need = col0 + CHUNK;
            if (need > n) need = n;
            if (col0 < n) {
                int spins = 0;
                if (WINDOW) {
                    // (the same wait; the word it ends on says whether the strip above is done, and from where its row is void)
                    int pv = poll_agent(prog_in);
                    while (pv < need && spins < spin_limit) {
                        __builtin_amdgcn_s_sleep(2);
                        spins++;
                        pv = poll_agent(prog_in);
                    }
                    if (pv >= WIN_RETIRED) pred_x = pv - WIN_RETIRED;
                } else
                while (poll_agent(prog_in) < need && spins < spin_limit) {
                    __builtin_amdgcn_s_sleep(2);
                    spins++;
                }
                if (spins >= spin_limit && lane == 0) atomicExch(a->error_flag, 1);
            }
            const int col = col0 + lane;
            int2 hf = make_int2(0, NEG_INF);
            unsigned char code = 0;
            if (col < n) {
                hf = ld_agent2(&a->bus[col]);
                code = a->seq1[col];
            }
            // window: what the strip above left from its X on is the skip constant, whatever the memory holds; a lane that has
            // passed the last column and a bus cell behind it enter no slab
            if (WINDOW && col >= pred_x) hf = NWP ? make_int2(NEG_INF, NEG_INF) : make_int2(0, NEG_INF);
            const bool passed = WINDOW && col0 - lane >= n, beyond = WINDOW && col >= n;
            if (PRUNE) {
                if (!GOAL) gseen = max(gseen, poll_agent(a->gbest_in));     // (goal mode: the bounds are fixed, nothing is read)
                if (GOAL) {
                    if (!ragged && col0 >= 2 * CHUNK && (WINDOW || col0 + CHUNK <= n)) {
                        // (the same two entries as below, held against the sweep's own bounds: see goal_keep32)
                        const bool own = !passed && goal_keep32(lane_entry, pr_rows - lane * R, pr_cols - col0 + lane + 2, R - 1, gcol, grow);
                        const bool top = !beyond && goal_keep32(hf.x - GAP_FIRST, pr_rows + 1, pr_cols - col + 1, 0, gcol, grow);
                        skip = goal_any && !__any(own || top);
                    }
                } else if (EDGE) {
                    if (!ragged && col0 >= 2 * CHUNK && (WINDOW || col0 + CHUNK <= n)) {
                        // (the same two entries and spans as below: see edge_upper32)
                        const int own = passed ? NEG_INF - 1 : edge_upper32(prune_end, lane_entry, pr_rows - lane * R, pr_cols - col0 + lane + 2, R - 1, 2);
                        const int top = beyond ? NEG_INF - 1 : edge_upper32(prune_end, hf.x - GAP_FIRST, pr_rows + 1, pr_cols - col + 1, 0, 1);
                        skip = !__any(max(own, top) >= gseen);
                    }
                } else if (NWP) {
                    if (!ragged && col0 >= 2 * CHUNK && (WINDOW || col0 + CHUNK <= n)) {
                        // what enters the slab: the lane's own last column (its R rows, column col0 - lane - 1, one column
                        // of room on either side) and the bus cell of its column (the row above the strip; its left
                        // neighbour is the slab's corner)
                        const int own = passed ? NEG_INF - 1 : nw_upper32(lane_entry, pr_rows - lane * R, pr_cols - col0 + lane + 2, R - 1, 2);
                        const int top = beyond ? NEG_INF - 1 : nw_upper32(hf.x - GAP_FIRST, pr_rows + 1, pr_cols - col + 1, 0, 1);
                        skip = !__any(max(own, top) >= gseen);
                    }
                } else
                if (!ragged && col0 >= 2 * CHUNK && (WINDOW || col0 + CHUNK <= n)) {
                    // (lane k is k columns behind lane 0: the slab touches columns col0 - 63 .. col0 + 63)
                    const int left = min(pr_rows + 2, pr_cols + 1 - (col0 - CHUNK));
                    const int e = max(passed ? NEG_INF : lane_entry, beyond ? NEG_INF : hf.x - GAP_FIRST);
                    skip = !__any(e + left + SW32_PRUNE_MARGIN >= gseen);
                }
                // retire: the state is the skip state, nothing but the constant enters from above from here on, and the rule
                // lets this slab go -- as it will every slab to the right (see WINDOW above)
                if (WINDOW && skip && prev_skip && pred_x <= col0) { retired = true; pruned_slabs += nchunks - c; break; }
            }
            // shift the seq1 window: [64,128) -> [0,64), then the new chunk
            const unsigned char prev = lds->c1[CHUNK + lane];
            lds->c1[lane] = prev;
            lds->c1[CHUNK + lane] = code;
            lds->in_tf[lane] = make_int2(hf.x - GAP_FIRST, hf.y);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        DBG(3, 20);
        // (2) 64 systolic steps
        const int jl = col0 - lane;
        const bool masked = (c == 0) || (col0 + CHUNK - 1 >= n);
        int2 feed = lds->in_tf[0];
        int c1 = lds->c1[CHUNK - lane];
        int cm = NEG_INF;
        if (PRUNE && skip) {
            // the slab is not computed: every cell in it counts as H = 0 (t = -5), E = F = -INF
            // (global rule: H = -INF as well, and the lane then holds nothing -- cm stays at -INF)
            const int t_skip = NWP ? NEG_INF - GAP_FIRST : -GAP_FIRST;
            // (window, trailing chunks: a lane that has passed column n - 1 holds its final last-column cells -- they stay)
            const bool keep = WINDOW && jl >= n;
#pragma unroll
            for (int r = 0; r < R; r++) { st.tl[r] = keep ? st.tl[r] : t_skip; st.e[r] = keep ? st.e[r] : NEG_INF; }
            st.tup_prev = t_skip; st.tbot = t_skip; st.fbot = NEG_INF;
            lds->out_tf[lane] = make_int2(t_skip, NEG_INF);
            if (!NWP) cm = -GAP_FIRST;
            pruned_slabs++;
            if (WINDOW) {
                if (!prev_skip) void_from = max(0, col0 - 63);      // (the emit lag: this slab's output columns start there)
                prev_skip = true;
            }
        } else if (ragged) {
#pragma unroll 2
            for (int u = 0; u < CHUNK; u++)
                wave_step<R, SW, PROFILE, true, TRACK, true, PRUNE>(st, lds, u, lane, jl, n, nvalid, emit_lane, emit_row, feed, c1, &cm);
        } else if (masked) {
#pragma unroll 2
            for (int u = 0; u < CHUNK; u++)
                wave_step<R, SW, PROFILE, true, TRACK, false, PRUNE>(st, lds, u, lane, jl, n, nvalid, 63, R - 1, feed, c1, &cm);
        } else {
#pragma unroll 4
            for (int u = 0; u < CHUNK; u++)
                wave_step<R, SW, PROFILE, false, TRACK, false, PRUNE>(st, lds, u, lane, jl, n, nvalid, 63, R - 1, feed, c1, &cm);
        }
        if (WINDOW && !skip) { prev_skip = false; void_from = 0x7fffffff; }   // a computed chunk: its output is no constant
        if (NWP) {
            // what the lane can hand on, as below; after a skipped slab it holds nothing
            lane_entry = skip ? NEG_INF : max(cm, masked ? lane_entry : NEG_INF);
            if (!skip) {
                clamp_void32<R>(st);
                // what this slab's cells say about H[m][n] from below.  The lane's maximum is the score of one of its cells --
                // its R rows, columns col0 - lane .. + 63 -- wherever it is: only slabs of full rows and columns are asked
                // (edge mode: about the best H on the named edge(s); goal mode: the bounds are fixed, nothing is folded or published)
                int lbv = NEG_INF;
                if (!GOAL && !masked && !ragged) {
                    const long long ki = (long long) pr_rows - lane * R, dj = (long long) pr_cols - col0 + lane;
                    const long long dhi = dj - (ki - (R - 1)), dlo = (dj - 63) - ki;
                    lbv = EDGE ? edge_lower32(prune_end, cm, ki < dj ? ki : dj, dlo, dhi) : nw_lower32(cm, ki < dj ? ki : dj, dhi > -dlo ? dhi : -dlo);
                }
                if (!GOAL && __any(lbv > gseen)) {
                    int w = lbv;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) w = max(w, __shfl_xor(w, d));
                    w = __builtin_amdgcn_readfirstlane(w);
                    if (lane == 0) atomicMax(a->gbest, w);
                    gseen = max(gseen, w);
                }
            }
        } else if (PRUNE) {
            // what the lane can hand on (a chunk it sat out entirely -- masked steps -- keeps what it held), and what the others learn
            lane_entry = max(cm, skip ? -GAP_FIRST : (masked ? lane_entry : NEG_INF));
            if (!skip && __any(cm > gseen)) {
                int w = cm;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) w = max(w, __shfl_xor(w, d));
                w = __builtin_amdgcn_readfirstlane(w);
                if (lane == 0) atomicMax(a->gbest, w);
                gseen = max(gseen, w);
            }
        }
        DBG(3, 30);
        // (3) output chunk: columns col0-emit_lane .. col0-emit_lane+63
        {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int2 tf = lds->out_tf[lane];
            const int col = col0 - emit_lane + lane;
            if (col >= 0 && col < n) {
                int2 hf = make_int2(tf.x + GAP_FIRST, tf.y);
                if (NWP) hf = make_int2(max(hf.x, NEG_INF), max(hf.y, NEG_INF));   // (-INF images stay at -INF: see clamp_void32)
                st_agent2(&a->bus[col], hf);
                if (special != nullptr) special[col] = hf;
                if (lastrow != nullptr) lastrow[col] = hf;
            }
            // every store of this wave must have left before the flag (R1: drain, then flag)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int done = col0 - emit_lane + CHUNK;
            if (done > n) done = n;
            if (done < 0) done = 0;
            // (window: the last word of a strip that walked to the end -- done, and void from there on)
            if (WINDOW && c == nchunks - 1) done = WIN_RETIRED + min(void_from, n);
            if (lane == 0) st_agent(prog_out, done);
        }
    }
    // (window: a retired strip's last word.  Every store of the chunks before it was drained ahead of their own flag, and
    //  nothing has been stored since; the columns from its first unwritten one on -- col0 - 63 >= void_from -- stay as they are)
    if (WINDOW && retired && lane == 0) st_agent(prog_out, WIN_RETIRED + void_from);

    if (PRUNE && pruned_slabs > 0 && lane == 0 && a->pruned_slabs != nullptr) atomicAdd(a->pruned_slabs, (unsigned long long) pruned_slabs);
    DBG(3, 40);
    // ---- strip epilogue: last column, best score ----
    if (a->last_col != nullptr) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int g = lrow0 + r;
            if (g < a->m) a->last_col[g + 1] = make_int2(st.tl[r] + GAP_FIRST, st.e[r]);
        }
    }
    if (TRACK) {
        // canonical reduction over lanes: max t, then min row, then min j
        lds->red[lane] = st.best_t;
        lds->red[64 + lane] = (st.best_j >= 0) ? (lrow0 + st.best_r) : 0x7fffffff;
        lds->red[128 + lane] = st.best_j;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            int bt = NEG_INF, bi = 0x7fffffff, bj = -1;
            for (int k = 0; k < 64; k++) {
                const int t = lds->red[k], i = lds->red[64 + k], j = lds->red[128 + k];
                if (j >= 0 && (t > bt || (t == bt && (i < bi || (i == bi && j < bj))))) {
                    bt = t; bi = i; bj = j;
                }
            }
            int4 rec;
            rec.x = (bj >= 0) ? bt + GAP_FIRST : NEG_INF;
            rec.y = bi; rec.z = bj; rec.w = 1;
            a->strip_best[s] = rec;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// TWO wavefronts per SIMD for this family (the packed kernels keep one): its inner loop is v_max_i32 / v_add_u32 /
// v_bfe, and a non-packed "slow" instruction of one wavefront co-issues with a "fast" one of another
// (profiles/r02_valu_issue_rate.md, result 2: v_max_i32 next to v_add_u32 = full overlap) -- which no single wavefront
// can do for itself.  The register allocation is held between a third and a half of the SIMD's 512-entry file, so that
// exactly two of these wavefronts fit a SIMD wherever the dispatcher puts them (launch = 2 x SIMDs wavefronts): the
// strip chain runs at the speed of its slowest member, a SIMD with three would hold everybody up.
// Measured (tools/int32_perf.py, 4 M x 3 M SW, GCUPS one / two wavefronts per SIMD): 256-row strips 1543 / 2244 (related),
// 512-row 1779 / 2060 (related), 2023(1024-row) / 2468 (unrelated); 1024-row strips need 248 registers and LOSE with two
// (1718 / 1486): they keep a SIMD to themselves, and the runtime prefers the short strips for this family.
#ifndef SW32_WAVES_PER_SIMD
#define SW32_WAVES_PER_SIMD 2
#endif
template <int R, bool SW, bool PROFILE, bool TRACK, bool PRUNE = false, bool GOAL = false, bool EDGE = false, bool WINDOW = false>
__global__ void __launch_bounds__(64)
#if SW32_WAVES_PER_SIMD == 2
__attribute__((amdgpu_waves_per_eu(R == 16 ? 1 : 2, R == 16 ? 1 : 2)))
#endif
sw_strip_kernel(const KernelArgs* __restrict__ ap) {
    __shared__ WaveLds lds_store;
    WaveLds* lds = &lds_store;
    const int lane = threadIdx.x;
    const UniformArgs a = uniform_args(ap);
    const int num_strips = a->num_strips;
#if SW32_WAVES_PER_SIMD == 2
    // vector + accumulation registers together in (170, 256]: R = 4 uses ~85 vector registers, R = 8 ~135, R = 16 ~250
    if (R == 4) asm volatile("" ::: "a127");
    else if (R == 8) asm volatile("" ::: "a63");
    else asm volatile("" ::: "a255");               // 1024-row strips: one wavefront per SIMD, as the packed kernels
#else
    // one wavefront per SIMD, enforced: see sw_kernel_pk16.inc
    asm volatile("" ::: "a255");
#endif
    for (;;) {
        const int s = __builtin_amdgcn_readfirstlane(claim_strip_common(ap, lane, 64 * R));
        if (s >= num_strips) break;
        if (poll_agent(a->abort_flag) != 0 || (a->host_abort != nullptr && poll_sys(a->host_abort) != 0)) {
            // stopped: this wavefront is done (every strip still in flight holds an earlier ticket; see sw_kernel_pk16.inc)
            if (lane == 0) st_agent(&a->progress[s + 1], a->n);
            __builtin_amdgcn_wave_barrier();
            break;
        } else {
            process_strip<R, SW, PROFILE, TRACK, PRUNE, GOAL, EDGE, WINDOW>(ap, s, lds, lane);
        }
        complete_strip_common(ap, s, lane, 64 * R, true);
    }
}

// Device-side border initialisation: InitialCellsReader::read (InitialCellsReader.cpp:84-108)
__global__ void fill_bus_kernel(int2* bus, int n, int init_type, int start_offset) {
    const int stride = gridDim.x * blockDim.x;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        int h = 0;
        if (init_type == INIT_WITH_GAPS) h = -GAP_EXT * (start_offset + j + 1) - 3;
        else if (init_type == INIT_WITH_GAPS_OPENED) h = -GAP_EXT * (start_offset + j + 1);
        bus[j] = make_int2(h, NEG_INF);
    }
}

__global__ void fill_int_kernel(int* p, long long count, int value) {
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) p[k] = value;
}

__global__ void fill_cells_kernel(int2* p, long long count, int2 value) {
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) p[k] = value;
}

template <int R>
static hipError_t launch_r(const KernelArgs* a, int grid, hipStream_t stream, bool sw, bool profile, bool track, bool prune, bool goal, bool edge, bool window) {
    if (prune && window) {    // the windowed twin of every pruning instantiation below (MI355SW_F_INT32_WINDOW)
#define LAUNCH_W(SWV, TRV, GOV, EDV) do { \
        if (profile) hipLaunchKernelGGL((sw_strip_kernel<R, SWV, true, TRV, true, GOV, EDV, true>), dim3(grid), dim3(64), 0, stream, a); \
        else hipLaunchKernelGGL((sw_strip_kernel<R, SWV, false, TRV, true, GOV, EDV, true>), dim3(grid), dim3(64), 0, stream, a); } while (0)
        if (sw) LAUNCH_W(true, true, false, false);
        else if (goal) LAUNCH_W(false, false, true, false);
        else if (edge) LAUNCH_W(false, false, false, true);
        else LAUNCH_W(false, false, false, false);
#undef LAUNCH_W
        return hipGetLastError();
    }
#define LAUNCH(SWV, PRV, TRV) \
    hipLaunchKernelGGL((sw_strip_kernel<R, SWV, PRV, TRV>), dim3(grid), dim3(64), 0, stream, a)
    if (sw && prune) {        // block pruning: local alignments with their best score tracked
        if (profile) hipLaunchKernelGGL((sw_strip_kernel<R, true, true, true, true>), dim3(grid), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((sw_strip_kernel<R, true, false, true, true>), dim3(grid), dim3(64), 0, stream, a);
    } else if (prune && goal) {   // ... global ones that look for a goal on their last column / row (MI355SW_F_INT32_PRUNE_EDGE_GOAL)
        if (profile) hipLaunchKernelGGL((sw_strip_kernel<R, false, true, false, true, true>), dim3(grid), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((sw_strip_kernel<R, false, false, false, true, true>), dim3(grid), dim3(64), 0, stream, a);
    } else if (prune && edge) {   // ... global ones that end on an edge of the super-partition (the same flag)
        if (profile) hipLaunchKernelGGL((sw_strip_kernel<R, false, true, false, true, false, true>), dim3(grid), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((sw_strip_kernel<R, false, false, false, true, false, true>), dim3(grid), dim3(64), 0, stream, a);
    } else if (prune) {       // ... and global ones whose goal is the last cell, nothing tracked (MI355SW_F_INT32_PRUNE_GLOBAL)
        if (profile) hipLaunchKernelGGL((sw_strip_kernel<R, false, true, false, true>), dim3(grid), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((sw_strip_kernel<R, false, false, false, true>), dim3(grid), dim3(64), 0, stream, a);
    } else if (sw) {
        if (profile) { if (track) LAUNCH(true, true, true); else LAUNCH(true, true, false); }
        else         { if (track) LAUNCH(true, false, true); else LAUNCH(true, false, false); }
    } else {
        if (profile) { if (track) LAUNCH(false, true, true); else LAUNCH(false, true, false); }
        else         { if (track) LAUNCH(false, false, true); else LAUNCH(false, false, false); }
    }
#undef LAUNCH
    return hipGetLastError();
}

hipError_t launch_strip_kernel(const KernelArgs& a, KernelArgs* dargs, int rows_per_lane, int grid, hipStream_t stream,
                               bool sw, bool profile, bool track, bool window) {
    hipError_t e = hipMemcpyAsync(dargs, &a, sizeof(KernelArgs), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);      // `a` is a host temporary
    if (e != hipSuccess) return e;
    // (the runtime sets a.prune for this family where an instantiation exists: local and tracked, or global and not tracked)
    const bool prune = a.prune != 0 && (sw ? track : !track);
    // goal and edge mode, under the packed dispatch's conditions (launch_strip_kernel_pk16)
    const bool goal = prune && (a.goal_bound_col > NEG_INF / 2 || a.goal_bound_row > NEG_INF / 2);
    const bool edge = prune && !goal && a.prune_end != 0;
    if ((goal || edge) && (track || sw)) return hipErrorInvalidValue;
    if (window && !prune) return hipErrorInvalidValue;    // (the window is the pruning kernels': a missing kernel is an error)
    switch (rows_per_lane) {
    case 4: return launch_r<4>(dargs, grid, stream, sw, profile, track, prune, goal, edge, window);
    case 8: return launch_r<8>(dargs, grid, stream, sw, profile, track, prune, goal, edge, window);
    case 16: return launch_r<16>(dargs, grid, stream, sw, profile, track, prune, goal, edge, window);
    default: return hipErrorInvalidValue;
    }
}

int strip_kernel_waves_per_simd(int rows_per_lane) { return (SW32_WAVES_PER_SIMD == 2 && rows_per_lane < 16) ? 2 : 1; }

hipError_t launch_fill_bus(int2* bus, int n, int init_type, int start_offset, hipStream_t stream) {
    int blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(fill_bus_kernel, dim3(blocks), dim3(256), 0, stream, bus, n, init_type, start_offset);
    return hipGetLastError();
}

hipError_t launch_fill_int(int* p, long long count, int value, hipStream_t stream) {
    long long b = (count + 255) / 256;
    int blocks = (int) (b > 2048 ? 2048 : (b < 1 ? 1 : b));
    hipLaunchKernelGGL(fill_int_kernel, dim3(blocks), dim3(256), 0, stream, p, count, value);
    return hipGetLastError();
}

hipError_t launch_fill_cells(int2* p, long long count, int h, int f, hipStream_t stream) {
    long long b = (count + 255) / 256;
    int blocks = (int) (b > 8192 ? 8192 : (b < 1 ? 1 : b));
    hipLaunchKernelGGL(fill_cells_kernel, dim3(blocks), dim3(256), 0, stream, p, count, make_int2(h, f));
    return hipGetLastError();
}

}  // namespace mi355sw
