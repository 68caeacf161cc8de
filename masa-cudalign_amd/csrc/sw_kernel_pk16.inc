// MI355X (gfx950) Stage-1 SW strip kernel, PACKED 16-BIT form: two DP cells per VALU instruction.
//
// Why: a wave64 int32 VALU op issues once per 4 cycles per SIMD on this chip whatever the occupancy
// (tools/micro_valu.hip), so the int32 kernel (sw_kernel.hip, ~10.8 ops/cell) is pinned at its VALU
// ceiling.  v_pk_{add,max}_i16 / v_pk_min_u16 issue at the same rate and carry two cells.
//
// Geometry: every lane owns TWO row blocks of R rows, packed lo/hi in each 32-bit register: the LO
// block (rows 2kR..2kR+R-1 of the strip) and the HI block (the next R rows), HI running ONE column behind
// LO.  The wave is a 128-stage systolic array ("virtual lane" v = 2*lane+half is v columns behind virtual
// lane 0): the LO block receives the bottom (T,F) of the previous lane's HI block by DPP wave_shr:1, the HI
// block receives its own lane's LO bottom of the previous step; one v_alignbit_b32 merges the two.
// Strip height = 128*R rows.
//
// Arithmetic (exact restatement of CPUBlockProcessor.cpp:66-93 for SW).  Row r of a block is kept in the
// domain X^ = X + 2r - bias ("row-shifted"): stepping DOWN one row then costs nothing for the gap extension
// (F^[r] = max(T^[r-1], F^[r-1]) is max(Hu-5, Fu-2) in that domain), the SW floor becomes a per-row
// constant Z^[r] = 2r - bias, and the diagonal score absorbs the shift:
//   x = mask0[r] & mask1        one-hot base masks (bit 2+code) | bit 1, both halves at once
//   y = pk_min_u16(x, 6)        = 6 on match, 2 otherwise        (score + 3 + 2)
//   (PK16_WIDE, the wide-alphabet twins: x = word0[r] ^ word1 on code words (code * 4), y = 6 - pk_min_u16(x, 4) -- see below)
//   E = sat(pk_max(TL,E) - 2)                                    (max(Hl-5,E-2) = max(Tl,E)-2, same row)
//   g = pk_max(pk_max(diag+y, E), Z^[r])                         off the row-to-row dependency chain
//   F = pk_max(upT, upF) ; H = pk_max(g, F) ; T = H - 3          the chain: 3 dependent ops per row
// 10 packed ops per 2 cells (+1 for the running maximum).  Bottoms are handed to the next block converted
// to its "row -1" domain (-2R).  Values are 16-bit RELATIVE to a wave-uniform
// int32 bias that is re-centred at chunk boundaries (every 64 columns) on the wavefront's running maximum:
// H is Lipschitz (|dH| <= 5 per row/column step), so everything a wavefront touches in one chunk lies
// within a few thousand of that maximum while the 16-bit window is 65536 wide.  A per-chunk guard on the
// chunk maximum still reports an overflow (the host then re-runs with the int32 kernel) long before a wrap
// is possible.  -INF borders saturate at -32768 and stay there (saturating adds).
//
// Two scoring forms per kernel, picked per chunk: the TABLE form (one v_perm_b32 per row, wave_step16<PERM>) when every
// column in reach carries one of the four commonest codes, else the GENERAL form above.  The one-hot general form has
// room for 14 matchable codes (bits 2..15 of a half).  PK16_WIDE builds the same file with an EQUALITY general form
// instead: a row's half-word is code * 4 (the pad / seq0-only code for rows that match nothing), a column's is code * 4
// (1020 for a column outside the matrix, which no row carries), x = row ^ column is 0 exactly on equal codes and >= 4
// otherwise, and y = 6 - pk_min_u16(x, 4) is the same 6 / 2 -- v_xor_b32, v_pk_min_u16, v_pk_sub_i16, one packed
// instruction more than the one-hot form, for up to 62 matchable codes (code * 4 of the seq1-only code K + 1 must fit a
// byte of seq1).  Everything else -- the table form and the test that picks it, the chunk loop, the exact replay, HALF
// tracking, re-basing, pruning, the window, goal mode, the stop -- does not depend on how a match is recognised and is
// shared.  The wide units (sw_kernel_pk16_w{a..j}.hip) give their kernels and launchers names of their own
// (sw_strip_kernel_pk16_wide<...>, launch_strip_kernel_pk16_wide, ...); the units {a..j} compile this file with
// PK16_WIDE unset and are untouched by it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_kernel.h"

#ifndef PK16_WIDE
#define PK16_WIDE 0
#endif
#if PK16_WIDE
// the wide twins' names: every kernel and every launcher of this file
#define sw_strip_kernel_pk16 sw_strip_kernel_pk16_wide
#define sw_strip_kernel_pk16_mixed sw_strip_kernel_pk16_mixed_wide
#define sw_batch_kernel_pk16 sw_batch_kernel_pk16_wide
#define launch16_r launch16_wide_r
#define launch_strip_kernel_pk16 launch_strip_kernel_pk16_wide
#define launch_strip_kernel_pk16_goal launch_strip_kernel_pk16_goal_wide
#define launch_strip_kernel_pk16_edge launch_strip_kernel_pk16_edge_wide
#define launch_strip_kernel_pk16_mixed launch_strip_kernel_pk16_mixed_wide
#define launch_batch_kernel_pk16 launch_batch_kernel_pk16_wide
#define launch_batch_kernel_pk16_r8 launch_batch_kernel_pk16_r8_wide
#define launch_batch_kernel_pk16_band launch_batch_kernel_pk16_band_wide
#define launch_batch_kernel_pk16_goal launch_batch_kernel_pk16_goal_wide
// half-word of a code in the equality form (rows: code <= pad_code <= 62; columns: code <= 63, or 255 outside the matrix)
#define WORD16(code) ((code) << 2)
#endif

namespace mi355sw {

#define DBG16(k, v) do { if (a->dbg != nullptr && lane == 0) __hip_atomic_store(&a->dbg[k], (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (0)

#define NEG_INF (-999999999)
// branch weights for the block placement: with ONE wavefront per SIMD a taken branch costs ~55 ns (the instruction fetch
// restarts with nobody to hide it), so the bulk path of a chunk -- fast pass, permute scoring, prefetched inputs,
// nothing to replay or re-centre -- should be the fall-through one
#ifndef PK16_NO_HINTS
#define LIKELY16(x) __builtin_expect(!!(x), 1)
#define UNLIKELY16(x) __builtin_expect(!!(x), 0)
#else
#define LIKELY16(x) (x)
#define UNLIKELY16(x) (x)
#endif
#define T_OFF 3            // T = H - 3
#define PRIO_CHUNKS 4       // chunks of every strip that run at raised wave priority
#define REBASE_HI 20000     // chunk maximum (relative) above which the window is moved up ...
#define REBASE_TO 8000      // ... so that the maximum sits here
#ifndef PK16_LDS_AHEAD
#define PK16_LDS_AHEAD 1   // steps between the request of a step's LDS operands and their use
#endif
#ifndef PK16_PRUNE
#define PK16_PRUNE 1
#endif
#ifndef PK16_OUT2D
#define PK16_OUT2D 1       // output staging as out2[step][lane] (see WaveLds16)
#endif
#ifndef PK16_LDS_PAIR
#define PK16_LDS_PAIR 1    // LDS operands of two steps per ds_read (see run_chunk16)
#endif
#define REBASE_LO (-8000)   // NW only: chunk maximum below which the window is moved down
#ifndef PK16_HALFTRACK
#define PK16_HALFTRACK 1  // fast pass accumulates the chunk maximum on odd rows only (even rows: bound +5)
#endif
#ifndef PK16_SVC_A
#define PK16_SVC_A 16     // step of a chunk at which the previous chunk's stores are published and the next inputs requested
#define PK16_SVC_B 0      // second chance for the input prefetch (0: none)
#endif
#ifndef PK16_START_SLACK
#define PK16_START_SLACK 0   // extra chunks of distance a strip keeps from its predecessor when it starts (measured on C2:
                             // 0: 1641 ms, 1: 1647, 2: 1668, 4: 1699 -- strips do not lose ground to their predecessors,
                             // so the distance is pure start-up cost)
#endif
#ifndef PK16_FF
#define PK16_FF 16         // pruned slabs tested and written out per round trip once a run of them has begun (0: one by one)
#endif
#ifndef PK16_HOTLOOP
#define PK16_HOTLOOP 1     // the usual chunks run in a loop of their own (see "the chunk loop" in process_strip16)
#endif
#ifndef PK16_EXACT_MODE
#define PK16_EXACT_MODE 1  // after a replayed chunk, run the following chunks in the exact code directly
#endif
// Steps per loop body of the 64-step chunk loop.  With the aligned build (csrc/align8.py) 8 and 16 are within 1 %
// of each other on 2 rounds x 1 M columns (ms, unroll 8 / 16):
//   R'=2: 218.9/226.8   4: 312.5/318.0   6: 401.4/397.7   8: 478.0/480.9   12: 660.0/662.9   16: 832.5/839.7
// but on C2 itself (3 M columns, R'=12) 16 wins by 2 % (1640 vs 1672 ms), so the rule stays as it was tuned on the
// long sweeps: 8 for R'=4 and 16, else 16.
#ifdef PK16_UNROLL
#define PK16_UNROLL_FOR(R) (PK16_UNROLL)
#else
#define PK16_UNROLL_FOR(R) (((R) == 4 || (R) == 16) ? 8 : 16)
#endif
#define GUARD16 30000      // chunk maximum above this => overflow report (wrap needs 32767)
// causes of an overflow report (device word error_flag[1], quoted in the host's message)
#define OVF16_SPREAD 1      // the strip's first column spreads over more than 24000 (no DP column does: <= 5 per row)
#define OVF16_BUS_ABOVE 2   // a bus cell from the strip above lies more than GUARD16 above this strip's window
#define OVF16_BUS_BELOW 4   // ... below it (NW / semi-global only: SW has its floor)
#define OVF16_CHUNK_MAX 8   // a chunk's maximum left the window upwards
#define OVF16_INJECTED 16   // MI355SW_FAULT_OVERFLOW_STRIP (test knob)

typedef unsigned int u32;
typedef short s2 __attribute__((ext_vector_type(2)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s2 as_s2(int x) { return __builtin_bit_cast(s2, x); }
__device__ __forceinline__ int as_i(s2 x) { return __builtin_bit_cast(int, x); }
__device__ __forceinline__ s2 pmax(s2 a, s2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ s2 padd_sat(s2 a, s2 b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ s2 splat(int v) { s2 r = {(short) v, (short) v}; return r; }
__device__ __forceinline__ int pack(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }
__device__ __forceinline__ int clamp16(int x) { return x < -32768 ? -32768 : (x > 32767 ? 32767 : x); }
__device__ __forceinline__ int lo16(int x) { return __builtin_amdgcn_sbfe(x, 0, 16); }
__device__ __forceinline__ int hi16(int x) { return x >> 16; }

__device__ __forceinline__ int wave_shr1_16(int old, int src) {
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int poll_agent16(const int* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int poll_sys16(const int* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
__device__ __forceinline__ void st_agent16(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sys16(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ int2 ld_agent2_16(const int2* p) {
    unsigned long long x = __hip_atomic_load((const unsigned long long*) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_int2((int) (u32) x, (int) (u32) (x >> 32));
}
__device__ __forceinline__ int2 ld_sys2_16(const int2* p) {
    unsigned long long x = __hip_atomic_load((const unsigned long long*) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return make_int2((int) (u32) x, (int) (u32) (x >> 32));
}
__device__ __forceinline__ int ld_u8_16(const unsigned char* p) {
    return (int) __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Asynchronous loads whose results are not needed for thousands of cycles.  They are issued from inline
// assembly straight into FIXED accumulation registers (a240..a245, far above anything the compiler spills
// into): the compiler neither tracks them with s_waitcnt nor has to keep a VGPR for them across the hot
// loop, and it never sees the value before the consumer -- after its own s_waitcnt vmcnt(0) -- reads the
// register back.  (Tracked loads into VGPRs were spilled to AGPRs whenever the loop ran out of registers,
// and the spill copy forced a vmcnt(0): a full memory latency, every chunk, right where it was meant to be
// hidden.  Which build did that was a matter of luck: 1.72 s vs 1.95 s on C2.)
//   a[240:241] next chunk's bus cell   a242 / a243 seq1 bytes (column, column-1)
//   a244 predecessor's progress         a245 running global best
#define ASYNC_SET(REG, VAL) asm volatile("v_accvgpr_write_b32 " REG ", %0" ::"v"(VAL) : "memory", REG)
#define ASYNC_LD32(REG, PTR) asm volatile("global_load_dword " REG ", %0, off sc1" ::"v"(PTR) : "memory", REG)
#define ASYNC_LD32_SYS(REG, PTR) asm volatile("global_load_dword " REG ", %0, off sc0 sc1" ::"v"(PTR) : "memory", REG)
#define ASYNC_LD8(REG, PTR) asm volatile("global_load_ubyte " REG ", %0, off sc1" ::"v"(PTR) : "memory", REG)
#define ASYNC_LD64_240(PTR) asm volatile("global_load_dwordx2 a[240:241], %0, off sc1" ::"v"(PTR) : "memory", "a240", "a241")
//   a[246:247] the predecessor's unwritten gap (pruning kernels with a window, see WIN_RETIRED)
//   a248 the stream's stop word (KernelArgs::stop_word)
#define ASYNC_LD64_246(PTR) asm volatile("global_load_dwordx2 a[246:247], %0, off sc1" ::"v"(PTR) : "memory", "a246", "a247")
#define ASYNC_GET(REG, OUT) asm volatile("v_accvgpr_read_b32 %0, " REG : "=v"(OUT) : : "memory")
#define ASYNC_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
__device__ __forceinline__ void st_agent2_16(int2* p, int2 v) {
    unsigned long long x = ((unsigned long long) (u32) v.y << 32) | (u32) v.x;
    __hip_atomic_store((unsigned long long*) p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

enum { WIN = 128 };   // seq1 window: 128 columns of history in front of the 64-column chunk

// ---- the pruning WINDOW (reference: BlockPruningDiagonal::updatePruningWindow, BlockPruningDiagonal.cpp:109-152, hands
//      [windowStart, windowEnd] to processDiagonal and blocks outside it cost a branch, X/CUDAligner.cu:950-960) ----
// A strip of a pruning run computes a band of columns and skips what lies left and right of it.  Skipped bus cells are a
// constant -- (0, -INF) for a local alignment, (-INF, -INF) for a global one -- so a strip need not WRITE them if the strip
// below knows where they are: per strip two words `win[2(s+1)], win[2(s+1)+1]` = [gap_lo, gap_hi), output columns it jumped
// over without writing, published BEFORE the progress value that covers them; and its LAST progress value is
// WIN_RETIRED + X: "done, and from column X on everything I left is the constant (written or not)".  The strip below
// substitutes the constant for whatever the bus memory holds there (stale cells of strips further up), jumps over the
// predecessor's gap in one step when its own state is void, and retires at once when it is void behind the
// predecessor's X: strips below the end of the alignment end after three chunks instead of walking the whole width.
// Rows that must exist in memory (special rows, checkpoint rows, the last row) are pre-filled with the constant by the host.
// (WIN_RETIRED itself: sw_kernel.h -- the int32 family's window reads the progress word the same way)

struct __attribute__((aligned(16))) WaveLds16 {
    int2 in_tf[CHUNK + (PK16_LDS_AHEAD > 2 ? PK16_LDS_AHEAD : 2)];      // (T16<<16, F16<<16) of the row above (value in the HIGH half: DPP `old` of lane 0)
#if PK16_OUT2D
    int2 out2[CHUNK][64];       // [step][lane]: EVERY lane stores its bottom (T,F) words at its own column of the step's
                                // row -- one ds_write_b64 with an immediate offset and no address arithmetic at all
                                // (the form before cost s_or + v_mov + v_cndmask + v_lshl_add per step, 3 % of the
                                // hot loop); the emitting lane's column is picked when the chunk is written out.
                                // 32 KB per wavefront: four one-wavefront workgroups per CU fit the 160 KB of LDS
#else
    int2 out_tf[CHUNK];         // packed (T,F) words of the emit lane, one per step
    int2 dump[64];              // write-only slots of the non-emitting lanes (no EXEC toggling per step)
#endif
    int c1w[WIN + CHUNK + 8];   // per column j: mask(j) | mask(j-1)<<16 (PK16_WIDE: the code words, same layout)
    int c1s[WIN + CHUNK + 8];   // per column j: v_perm_b32 selector {code(j), zero, 4+code(j-1), zero} (table form)
    int red[3 * 64];
};

template <int R>
struct Lane16 {
    s2 TL[R];       // T of the cell to the left      (lo: LO block row r, hi: HI block row r)
    s2 E[R];        // E of the cell to the left
    int M0[R];      // one-hot base masks of the two rows (PK16_WIDE: their code words)
    int TLO[R], THI[R];   // table form of the same: byte c = score of the row against column code c (c < 4)
    s2 tup_prev;    // T of (row above the block, previous column)
    s2 tbot, fbot;  // bottoms produced at the previous step
    int best_t, best_r, best_j;   // best T (true, 32-bit), row index inside the lane (0..2R-1), column
};

template <int R, bool MASKED, bool TRACK, bool EMIT_ANY, bool HALF, bool PERM, bool SWF, bool SATT>
__device__ __forceinline__ void wave_step16(Lane16<R>& st, WaveLds16* lds, const int u, const int lane,
                                            const int jl /* LO column of this lane at u=0 */, const int n,
                                            const int nvalid_lo, const int nvalid_hi, const int emit_lane,
                                            const int emit_row, const s2 (&Z)[R], const int bias, const int2 feed, const int c1p,
                                            s2 (&cm)[R], int2* out_base, const int out_stride, const bool all_rows_valid) {
    // (feed = the bus cell of this step for lane 0, c1p = this lane's column codes: staged in LDS, fetched by the caller
    //  ahead of their use)
    // hand-off: LO <- previous lane's HI bottom (DPP), HI <- own LO bottom; lane 0 LO <- bus feed
    const int dT = wave_shr1_16(feed.x, as_i(st.tbot));
    const int dF = wave_shr1_16(feed.y, as_i(st.fbot));
    const s2 tup = as_s2(__builtin_amdgcn_alignbit(as_i(st.tbot), dT, 16));
    s2 upT = tup;
    s2 upF = as_s2(__builtin_amdgcn_alignbit(as_i(st.fbot), dF, 16));
    s2 diag = st.tup_prev;

    int vmask = -1;
    if (MASKED) {
        const int j = jl + u;                                  // LO column; HI is at j-1
        const bool vlo = (u32) j < (u32) n;
        const bool vhi = (u32) (j - 1) < (u32) n;
        vmask = (vlo ? 0xffff : 0) | (vhi ? 0xffff0000 : 0);
    }
    const s2 m2 = splat(-2), m3 = splat(-T_OFF);
    const us2 six = {6, 6};
#if PK16_WIDE
    const us2 four = {4, 4};
#endif
    s2 t_emit = splat(0), f_emit = splat(0);
    s2 ms = splat(-32768);                                   // TRACK only: true (unshifted) maximum of the step
    s2 newT[R];
    s2 Hbot = splat(0);
#pragma unroll
    for (int r = 0; r < R; r++) {
        // score + 5 of the two cells: one byte permute when every column in reach is one of <= 4 plain
        // codes (table form), else one-hot AND + min (PK16_WIDE: XOR of the code words, 0 exactly on a match)
        us2 y;
        if (PERM) {
            y = __builtin_bit_cast(us2, __builtin_amdgcn_perm((u32) st.THI[r], (u32) st.TLO[r], (u32) c1p));
        } else {
#if PK16_WIDE
            const int x = st.M0[r] ^ c1p;
            y = six - __builtin_elementwise_min(__builtin_bit_cast(us2, x), four);
#else
            const int x = st.M0[r] & c1p;
            y = __builtin_elementwise_min(__builtin_bit_cast(us2, x), six);
#endif
        }
        s2 Ev = padd_sat(pmax(st.TL[r], st.E[r]), m2);
        const s2 v = diag + __builtin_bit_cast(s2, y);
        const s2 g = SWF ? pmax(pmax(v, Ev), Z[r]) : pmax(v, Ev);   // off the row-to-row critical chain (Z: SW floor)
        const s2 Fv = pmax(upT, upF);                      // chain: max, max, add per row
        const s2 H = pmax(g, Fv);
        // (SATT: kernels in which whole slabs can be -INF -- block pruning without a floor -- keep the image of -INF at
        //  -32768 through this subtraction as well; everywhere else H is a real score well inside the window)
        s2 T = SATT ? padd_sat(H, m3) : H + m3;
        diag = st.TL[r];
        if (MASKED) {
            T = as_s2((as_i(T) & vmask) | (as_i(st.TL[r]) & ~vmask));
            Ev = as_s2((as_i(Ev) & vmask) | (as_i(st.E[r]) & ~vmask));
        }
        st.TL[r] = T;
        st.E[r] = Ev;
        newT[r] = T;
        upT = T;
        upF = Fv;
        Hbot = H;
        // HALF: H(i,j) <= H(i+1,j) + 5 (the row below can always open a gap), so the odd rows bound the
        // even ones; the chunk test adds the 5 and an exact replay decides
        // (an odd block height leaves its last, even row without an odd row below it in the block: it is tracked too)
        if (!HALF || (r & 1) || r == R - 1) {
            if (MASKED) cm[r] = pmax(cm[r], as_s2((as_i(T) & vmask) | (0x80008000 & ~vmask)));
            else cm[r] = pmax(cm[r], T);
        }
        if (TRACK) {
            // (SATT: a cell at the window's bottom stays there, see T above)
            const s2 tt = SATT ? padd_sat(T, splat(-2 * r)) : T + splat(-2 * r);
            if (MASKED) ms = pmax(ms, as_s2((as_i(tt) & vmask) | (0x80008000 & ~vmask)));
            else ms = pmax(ms, tt);
        }
        if (EMIT_ANY) {
            t_emit = (r == emit_row) ? T : t_emit;
            f_emit = (r == emit_row) ? Fv : f_emit;
        }
    }
    // bottoms for the next block, converted to its "row -1" domain (2(R-1) -> -2); saturating, so the
    // -INF image stays put.  tbot comes straight from H (parallel to T = H - 3, not behind it).
    const s2 tb = MASKED ? padd_sat(upT, splat(-2 * R)) : padd_sat(Hbot, splat(-T_OFF - 2 * R));
    const s2 fb = padd_sat(upF, splat(-2 * R));
    if (MASKED) {
        st.tup_prev = as_s2((as_i(tup) & vmask) | (as_i(st.tup_prev) & ~vmask));
        st.tbot = as_s2((as_i(tb) & vmask) | (as_i(st.tbot) & ~vmask));
        st.fbot = as_s2((as_i(fb) & vmask) | (as_i(st.fbot) & ~vmask));
    } else {
        st.tup_prev = tup;
        st.tbot = tb;
        st.fbot = fb;
    }
    if (!EMIT_ANY) { t_emit = upT; f_emit = upF; }
#if PK16_OUT2D
    out_base[64 * u] = make_int2(as_i(t_emit), as_i(f_emit));      // out2[u][lane]
#else
    // all lanes store (no s_and_saveexec / s_or per step): lane `emit_lane` into out_tf[u], the others into dump[lane]
    out_base[out_stride * u] = make_int2(as_i(t_emit), as_i(f_emit));
#endif

    if (TRACK) {
        // cheap per-step test on max(lo,hi); rare exact path keeps the canonical (max, min i, min j) cell
        const int mi = as_i(ms);
        const int m = max(lo16(mi), hi16(mi)) + bias;
        if (__any(m >= st.best_t)) {
            const int j = jl + u;
            if (all_rows_valid) {
                // Only the step's best cell of the lane can displace the running best: the larger half
                // maximum (LO on a tie: smaller row), at the FIRST row that reaches it.  Packed search for
                // that row: (ms - tt) is 0 exactly there.
                us2 fr = {0x7fff, 0x7fff};
                const us2 one = {1, 1}, big = {0x4000, 0x4000};
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const s2 tt = SATT ? padd_sat(newT[r], splat(-2 * r)) : newT[r] + splat(-2 * r);
                    const us2 d = __builtin_bit_cast(us2, ms - tt);
                    const us2 z = __builtin_elementwise_min(d, one);
                    const us2 rv = {(unsigned short) r, (unsigned short) r};
                    fr = __builtin_elementwise_min(fr, (us2) (z * big + rv));
                }
                const int fi = __builtin_bit_cast(int, fr);
                const int mlo = lo16(mi), mhi = hi16(mi);
                const bool vlo = MASKED ? ((vmask & 1) != 0) : true;
                const bool vhi = MASKED ? (((vmask >> 16) & 1) != 0) : true;
                const bool use_hi = vhi && (!vlo || mhi > mlo);
                const int t = (use_hi ? mhi : mlo) + bias;
                const int rr = use_hi ? (R + (int) ((u32) fi >> 16)) : (fi & 0xffff);
                const bool upd = (use_hi ? vhi : vlo) && ((t > st.best_t) || (t == st.best_t && rr < st.best_r));
                st.best_t = upd ? t : st.best_t;
                st.best_r = upd ? rr : st.best_r;
                st.best_j = upd ? (j - (use_hi ? 1 : 0)) : st.best_j;
            } else
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int nv = half ? nvalid_hi : nvalid_lo;
                const bool hv = MASKED ? (((vmask >> (16 * half)) & 1) != 0) : true;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int w = as_i(newT[r]);
                    const int t = (half ? hi16(w) : lo16(w)) + bias - 2 * r;
                    const int rr = half * R + r;
                    const bool upd = hv && (r < nv) && ((t > st.best_t) || (t == st.best_t && rr < st.best_r));
                    st.best_t = upd ? t : st.best_t;
                    st.best_r = upd ? rr : st.best_r;
                    st.best_j = upd ? (j - half) : st.best_j;
                }
            }
        }
    }
}

// true (unshifted) maximum T of a chunk from the per-row accumulators
template <int R, bool HALF>
__device__ __forceinline__ int chunk_max16(const s2 (&cm)[R]) {
    int v = -32768 - 2 * R;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (HALF && !(r & 1) && r != R - 1) continue;      // the rows wave_step16 accumulates
        const int w = as_i(cm[r]);
        v = max(v, max(lo16(w), hi16(w)) - 2 * r);
    }
    return v;
}

// a wave-uniform value the compiler can neither re-derive nor re-load: it went through an opaque register once
__device__ __forceinline__ int pin32_16(int v) {
    asm volatile("" : "+v"(v));
    return __builtin_amdgcn_readfirstlane(v);
}
template <typename T>
__device__ __forceinline__ T* pin_ptr16(T* p) {
    const unsigned long long v = (unsigned long long) p;
    const unsigned lo = (unsigned) pin32_16((int) (unsigned) v), hi = (unsigned) pin32_16((int) (unsigned) (v >> 32));
    // (a pointer rebuilt from an integer is a flat pointer to the compiler -- flat accesses count on both memory counters and
    //  make every LDS wait a wait for global memory too -- so it is told that this one points to global memory)
    typedef __attribute__((address_space(1))) T* GlobalPtr;
    return (T*) (GlobalPtr) (((unsigned long long) hi << 32) | lo);
}

template <bool B> struct BoolC16 { static constexpr bool value = B; };

// 64 systolic steps of one chunk (reads the staged inputs from LDS, leaves the emit row in out_tf)
struct NoService16 { __device__ __forceinline__ void operator()(int) const {} };

template <int R, bool MASKED, bool TRACKSTEP, bool EMIT_ANY, bool HALF, bool PERM, bool SWF, bool SATT, typename Svc>
__device__ __forceinline__ void run_chunk16(Lane16<R>& st, WaveLds16* lds, const int lane, const int jl, const int n,
                                            const int nvalid_lo, const int nvalid_hi, const int emit_lane,
                                            const int emit_row, const s2 (&Z)[R], const int bias, s2 (&cmax)[R],
                                            Svc&& service, const bool all_rows_valid = true) {
#if PK16_OUT2D
    int2* out_base = &lds->out2[0][lane];
    const int out_stride = 0;
#else
    int2* out_base = (lane == emit_lane) ? &lds->out_tf[0] : &lds->dump[lane];
    const int out_stride = (lane == emit_lane) ? 1 : 0;
#endif
    constexpr int UNR = PK16_UNROLL_FOR(R);
    // the service point is a loop-body boundary: a body that steps over it would never publish a chunk (deadlock)
    static_assert(PK16_SVC_A % UNR == 0 && CHUNK % UNR == 0 && (PK16_SVC_B == 0 || PK16_SVC_B % UNR == 0),
                  "PK16_UNROLL must divide the service points and the chunk");
    const int* c1arr = PERM ? lds->c1s : lds->c1w;
#if PK16_LDS_PAIR
    // LDS operands of TWO steps per instruction (ds_read_b128 for the bus cells, ds_read_b64 for the column codes),
    // requested one pair of steps before they are used: half the LDS instructions and half the s_waitcnt of the
    // one-step form, each of which costs the lone wavefront an issue slot
    static_assert(UNR % 2 == 0, "steps are processed in pairs");
    int4 feed2 = *reinterpret_cast<const int4*>(&lds->in_tf[0]);
    int2 c2 = *reinterpret_cast<const int2*>(&c1arr[WIN - 2 * lane]);
#pragma unroll 1
    for (int ub = 0; ub < CHUNK; ub += UNR) {
        if (ub == PK16_SVC_A) service(0);
        if (PK16_SVC_B > 0 && ub == PK16_SVC_B) service(1);
#pragma unroll
        for (int k = 0; k < UNR; k += 2) {
            const int u = ub + k;
            const int4 nfeed = *reinterpret_cast<const int4*>(&lds->in_tf[u + 2]);
            const int2 nc = *reinterpret_cast<const int2*>(&c1arr[WIN + u + 2 - 2 * lane]);
            wave_step16<R, MASKED, TRACKSTEP, EMIT_ANY, HALF, PERM, SWF, SATT>(st, lds, u, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, make_int2(feed2.x, feed2.y), c2.x, cmax, out_base, out_stride, all_rows_valid);
            wave_step16<R, MASKED, TRACKSTEP, EMIT_ANY, HALF, PERM, SWF, SATT>(st, lds, u + 1, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, make_int2(feed2.z, feed2.w), c2.y, cmax, out_base, out_stride, all_rows_valid);
            feed2 = nfeed;
            c2 = nc;
        }
    }
#else
    // LDS operands are requested PK16_LDS_AHEAD steps before they are used
    int2 feed[PK16_LDS_AHEAD];
    int c1[PK16_LDS_AHEAD];
#pragma unroll
    for (int k = 0; k < PK16_LDS_AHEAD; k++) {
        feed[k] = lds->in_tf[k];
        c1[k] = c1arr[WIN + k - 2 * lane];
    }
#pragma unroll 1
    for (int ub = 0; ub < CHUNK; ub += UNR) {
        // in-chunk service points: wave-uniform branches at a loop-body boundary, where the schedule is cut anyway
        if (ub == PK16_SVC_A) service(0);
        if (PK16_SVC_B > 0 && ub == PK16_SVC_B) service(1);
#pragma unroll
        for (int k = 0; k < UNR; k++) {
            const int u = ub + k;
            const int2 f = feed[0];
            const int c = c1[0];
#pragma unroll
            for (int q = 0; q + 1 < PK16_LDS_AHEAD; q++) { feed[q] = feed[q + 1]; c1[q] = c1[q + 1]; }
            feed[PK16_LDS_AHEAD - 1] = lds->in_tf[u + PK16_LDS_AHEAD];
            c1[PK16_LDS_AHEAD - 1] = c1arr[WIN + u + PK16_LDS_AHEAD - 2 * lane];
            wave_step16<R, MASKED, TRACKSTEP, EMIT_ANY, HALF, PERM, SWF, SATT>(st, lds, u, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, f, c, cmax, out_base, out_stride, all_rows_valid);
        }
    }
#endif
}

// ---- block pruning of GLOBAL alignments (AbstractBlockPruning::isBlockPrunable, NEEDLEMAN_WUNSCH branch,
//      M/libmasa/pruning/AbstractBlockPruning.cpp:92-109): the alignment ends in the last cell of the super-partition ----
// Upper bound (T = H - 3 domain) of the score in that last cell of any path through a cell that holds `t`, when the
// cell has between di - si and di rows and between dj - sj and dj columns still to go: every one of the min(di, dj)
// diagonal steps a match, and the gap that the imbalance |dj - di| forces at its extension price only (the cell may sit
// inside a gap that is already open).  The reference takes the block's best score and the block's corner; here the
// cells are a lane's last column or a bus cell, and the spans make the bound hold for every cell of them.
// The local test needs the same kind of room (round 5): what enters a slab through its CORNER -- the bus cell diagonally above
// the strip's first cell of the slab, carried in from the slab before -- is not among the values the test looks at (the
// lanes' chunk maxima, the bus cells above the slab's own columns), only within one step (<= 5) of one of them.  Without the
// margin a path that can only TIE what is already known -- a second co-optimal alignment, or the optimal one itself behind a
// bound that starts at the optimum -- and crosses a strip boundary exactly at a slab corner on its last cells was cut there.
#define SW_PRUNE_MARGIN 8
#define NW_PRUNE_MARGIN 16   // entering values the test does not look at one by one (the diagonal neighbour of the slab's
                             // corner, a gap state next to the cell) are within this of one it does look at
__device__ __forceinline__ int nw_upper16(const int t, const int di, const int dj, const int si, const int sj) {
    if (t <= NEG_INF / 2) return NEG_INF - 1;             // nothing enters here: below every lower bound, known or not
    const int inc = min(di, dj);
    const int dlo = dj - sj - di, dhi = dj - di + si;      // range of (columns left - rows left) over the cells
    int dmin = max(0, max(dlo, -dhi));
    dmin = min(dmin, 400000000);                          // (int32 headroom; a weaker bound, never a wrong one)
    return t + inc - 2 * dmin + NW_PRUNE_MARGIN;
}
// Lower bound (T domain) of the last cell's score from a cell that holds `t` (a score some path really reaches):
// mismatches down the diagonal for at most `kmax` steps, then one gap of at most `dmax` (AbstractBlockPruning.cpp:100-104:
// dec = distMin * -mismatch + gap_open + gaps * gap_ext)
__device__ __forceinline__ int nw_lower16(const int t, const long long kmax, const long long dmax) {
    const long long lb = (long long) t - 3 * kmax - 3 - 2 * dmax;
    return lb > (long long) NEG_INF ? (int) lb : NEG_INF;
}

// GOAL mode of the global pruning kernels (round 7): the sweep looks for a goal score met somewhere on its LAST COLUMN -- a
// stage-2 sweep from a crosspoint, matched there against a special row of stage 1 -- and, when its partition runs to the
// matrix's border, on its last row.  The bounds are constants of the sweep (KernelArgs::goal_bound_col / _row, T domain):
// a cell that holds t with dj columns left reaches the last column with at most t + dj (every step a match), and the last
// row with at most t + min(di, dj) - 2 * (di - dj) when it has more rows left than columns (the surplus is a gap).  A slab
// goes when nothing that enters it stays at or above a bound that is on; the test is strict and keeps NW_PRUNE_MARGIN.
// `t` bounds cells whose rows-left lie in [di - si, di] and whose columns-left are at most dj.  (64-bit: t + dj need not fit.)
__device__ __forceinline__ bool goal_keep16(const int t, const int di, const int dj, const int si, const long long gcol, const long long grow) {
    if (t <= NEG_INF / 2) return false;                   // nothing enters here
    const long long ucol = (long long) t + dj + NW_PRUNE_MARGIN;
    const long long surplus = (long long) di - si - dj;   // the least (rows left - columns left) among the cells
    const long long urow = (long long) t + min(di, dj) - 2 * (surplus > 0 ? surplus : 0) + NW_PRUNE_MARGIN;
    return ucol >= gcol || urow >= grow;
}

// EDGE mode of the global pruning kernels: the alignment ends on an EDGE of the super-partition instead of in its last cell --
// KernelArgs::prune_end 1: anywhere on the last row, 2: anywhere on the last column, 3: on either -- and the result is the best
// H there.  Everything is the global mode's (the running lower bound in gbest, det_prefix, the window, -INF for skipped cells)
// except the gap that the rest of a path is forced to hold, g: the global mode must reach the corner, |dj - di| cells of gap;
// a path that may end anywhere on the last row only has to get DOWN, g = max(0, di - dj); one that may end anywhere on the last
// column only has to get ACROSS, g = max(0, dj - di); one that may do either is never forced into a gap.
// Upper bound, as nw_upper16: every one of the min(di, dj) diagonal steps a match, the forced gap at its extension price.
__device__ __forceinline__ int edge_upper16(const int end, const int t, const int di, const int dj, const int si, const int sj) {
    if (t <= NEG_INF / 2) return NEG_INF - 1;             // nothing enters here: below every lower bound, known or not
    const int inc = min(di, dj);
    const int dlo = dj - sj - di, dhi = dj - di + si;      // range of (columns left - rows left) over the cells
    int gmin = end == 1 ? max(0, -dhi) : (end == 2 ? max(0, dlo) : 0);   // the least forced gap among them
    gmin = min(gmin, 400000000);                          // (int32 headroom; a weaker bound, never a wrong one)
    return t + inc - 2 * gmin + NW_PRUNE_MARGIN;
}
// Lower bound, as nw_lower16: mismatches down the diagonal to the nearer edge, at most `kmax` steps, and -- only where that
// edge is not one the alignment may end on -- one gap along it; dlo .. dhi: range of (columns left - rows left) over the cells.
__device__ __forceinline__ int edge_lower16(const int end, const int t, const long long kmax, const long long dlo, const long long dhi) {
    const long long gmax = end == 1 ? -dlo : (end == 2 ? dhi : 0);   // the largest forced gap among them
    const long long lb = (long long) t - 3 * kmax - (gmax > 0 ? 3 + 2 * gmax : 0);
    return lb > (long long) NEG_INF ? (int) lb : NEG_INF;
}

template <int R, bool TRACK, bool SWF, bool PRUNE, bool GOAL = false, bool EDGE = false>
__device__ __attribute__((noinline)) void process_strip16(const KernelArgs* ap, const int s_in, WaveLds16* lds, const int lane) {
    const UniformArgs a = uniform_args(ap);
    const int s = __builtin_amdgcn_readfirstlane(s_in);
    const int n = a->n;
    const int SH = 128 * R;
    const int nchunks = (n + 127 + CHUNK - 1) / CHUNK;
    int bias = 0;                                         // wave-uniform int32 bias of the 16-bit window

    const int row0 = (s >= a->mix_first ? a->strip_row0_b : a->strip_row0) + s * SH;   // (mixed-height launches: see sw_strip_kernel_pk16_mixed)
    const int lrow_lo = row0 + (2 * lane) * R;            // first row of the LO block
    const int lrow_hi = lrow_lo + R;                      // first row of the HI block
    int nvalid_lo = a->m - lrow_lo; nvalid_lo = nvalid_lo < 0 ? 0 : (nvalid_lo > R ? R : nvalid_lo);
    int nvalid_hi = a->m - lrow_hi; nvalid_hi = nvalid_hi < 0 ? 0 : (nvalid_hi > R ? R : nvalid_hi);
    const int* prog_in = &a->progress[s];
    // wait budget of the in-kernel polls: a band fed by another GPU may legitimately stand still for as long as
    // its first column takes to arrive (the first strip waits on the host counter, all others on that strip)
    const int spin_limit = a->first_col_ready != nullptr ? (1 << 30) : (1 << 24);
    int* prog_out = &a->progress[a->independent ? a->num_strips + 1 + s : s + 1];

    // emitting virtual lane / row: the strip's bottom row, or DP row m-1 for the ragged last strip
    int emit_v = 127, emit_row = R - 1;
    const bool ragged = (row0 + SH > a->m);
    const bool emit_any = ragged && a->last_row != nullptr;   // otherwise nobody reads a ragged strip's bus row
    if (emit_any) {
        const int last = a->m - 1 - row0;
        emit_v = last / R;
        emit_row = last - emit_v * R;
    }
    const int emit_lane = emit_v >> 1, emit_half = emit_v & 1;
    const bool last_strip = (row0 + SH >= a->m);
    int2* special = nullptr;
    if (a->special_interval_strips > 0 && a->special_rows != nullptr) {
        const int sg = a->strip_index0 + s + 1;
        if (sg % a->special_interval_strips == 0 && (long long) sg * SH < a->m)
            special = a->special_rows + (long long) (sg / a->special_interval_strips - 1) * a->special_pitch;
    }
    int2* lastrow = (last_strip && a->last_row != nullptr) ? a->last_row : nullptr;
    int2* ckpt = nullptr;
    if (a->ckpt_rows != nullptr && a->ckpt_interval_strips > 0) {
        const int sg = a->strip_index0 + s + 1;
        if (sg % a->ckpt_interval_strips == 0 && !last_strip)
            ckpt = a->ckpt_rows + (long long) (sg / a->ckpt_interval_strips) * a->ckpt_pitch;
    }

    int overflow = 0;                                     // why the 16-bit window cannot hold this strip (OVF16_*), 0 = it can
    // ---- first column (a column delivered from outside has been awaited in claim_strip_common) ----
#ifdef PK16_LEGACY_FCWAIT
    if (a->first_col != nullptr && a->first_col_ready != nullptr) {
        int need = row0 + SH;
        if (need > a->m) need = a->m;
        int spins = 0;
        while (poll_sys16(a->first_col_ready) < need && poll_agent16(a->abort_flag) == 0 && spins < (1 << 26)) {
            __builtin_amdgcn_s_sleep(32);
            spins++;
        }
        if (spins >= (1 << 26) && lane == 0) atomicExch(a->error_flag, 2);
    }
#endif
    Lane16<R> st;
    int h0[2 * R], e0[2 * R];
    int hmax = SWF ? 0 : NEG_INF;
    int hmin = -NEG_INF;        // over the cells the column really holds (not the SW floor: a strip deep inside a long
                                // alignment has a first column of large scores only, which the window follows)
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int g = (half ? lrow_hi : lrow_lo) + r;
            // rows past m: 0 is a harmless start under the SW floor; without a floor it could sit far above
            // the window, so they start at the -INF image instead
            int h = (SWF || a->first_col == nullptr) ? 0 : NEG_INF, ee = NEG_INF;
            if (a->first_col != nullptr && g < a->m) {
                const int2 c = ld_sys2_16(&a->first_col[g + 1]);
                h = c.x; ee = c.y;
#ifndef PK16_NO_SPREAD_GUARD
                hmin = min(hmin, h);
#endif
            }
            h0[2 * r + half] = h; e0[2 * r + half] = ee;
            if (SWF || g < a->m) hmax = max(hmax, h);
        }
    }
    const int hmax_lane = hmax;
    // (pruning without a floor: "the column holds nothing" must include the cell diagonally above the strip's first row)
    if (PRUNE && !SWF && lane == 0 && a->first_col != nullptr) hmax = max(hmax, ld_sys2_16(&a->first_col[row0]).x);
    // initial window: centred on the largest first-column score of the strip (0 for zero borders)
#pragma unroll
#ifndef PK16_NO_SPREAD_GUARD
    for (int d = 32; d >= 1; d >>= 1) { hmax = max(hmax, __shfl_xor(hmax, d)); hmin = min(hmin, __shfl_xor(hmin, d)); }
#else
    for (int d = 32; d >= 1; d >>= 1) hmax = max(hmax, __shfl_xor(hmax, d));
#endif
    // A first column taken from a DP matrix moves by at most 5 per row, 10 240 over the tallest strip.  Border data
    // that spreads over more than the window can hold next to a chunk's growth is reported like any other overflow
    // (the int32 kernel takes over) instead of being saturated silently.
    // (Pruning kernels: a boundary column that crosses the edge of a pruned region holds skipped cells -- H = 0, or -INF
    //  without a floor -- next to scores of millions.  Those are lower bounds, and so is what saturation makes of them:
    //  the window's bottom lies 40 000 below the column's maximum, the TRUE value of every cell of the strip within
    //  6 * 2048 of it.)
#ifndef PK16_NO_SPREAD_GUARD
    if (!PRUNE && a->first_col != nullptr && hmax - hmin > 24000) overflow |= OVF16_SPREAD;
#endif
    // SW: the window never goes below the floor (bias >= 0); NW/semi-global: it follows the scores down too
    if (SWF) bias = __builtin_amdgcn_readfirstlane(hmax > REBASE_HI ? hmax - REBASE_TO : 0);
    else if (PRUNE && hmax <= NEG_INF / 2) bias = 0;      // nothing but skipped cells in the first column: see state_void
    else bias = __builtin_amdgcn_readfirstlane((hmax > REBASE_HI || hmax < REBASE_LO) ? hmax - REBASE_TO : 0);
    s2 Z[R];                                              // SW floor (H = 0) of every row in its shifted domain
#pragma unroll
    for (int r = 0; r < R; r++) Z[r] = splat(clamp16(2 * r - bias));
#pragma unroll
    for (int r = 0; r < R; r++) {
        int mk[2], tb[2];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int g = (half ? lrow_hi : lrow_lo) + r;
            const int c0 = (g < a->m) ? (int) a->seq0[g] : a->pad_code;
#if PK16_WIDE
            mk[half] = WORD16(c0);                                     // (pad_code: the word no column carries)
#else
            mk[half] = ((c0 < a->n_match_codes) ? (4 << c0) : 0) | 2;   // bit 1: the constant part of the score
#endif
            tb[half] = 0x02020202 | ((c0 < a->n_match_codes && c0 < 4) ? (4 << (8 * c0)) : 0);
        }
        st.TL[r] = as_s2(pack(clamp16(h0[2 * r] - T_OFF - bias + 2 * r), clamp16(h0[2 * r + 1] - T_OFF - bias + 2 * r)));
        st.E[r] = as_s2(pack(clamp16(e0[2 * r] - bias + 2 * r), clamp16(e0[2 * r + 1] - bias + 2 * r)));
        st.M0[r] = pack(mk[0], mk[1]);
        st.TLO[r] = tb[0];
        st.THI[r] = tb[1];
    }
    {
        int hd[2];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int g0 = half ? lrow_hi : lrow_lo;
            int h = (SWF || a->first_col == nullptr) ? 0 : NEG_INF;
            if (a->first_col != nullptr && g0 <= a->m) h = ld_sys2_16(&a->first_col[g0]).x;
            hd[half] = clamp16(h - T_OFF - bias - 2);        // "row -1" of the block
        }
        st.tup_prev = as_s2(pack(hd[0], hd[1]));
    }
    st.tbot = splat(-32768);
    st.fbot = splat(-32768);
    st.best_t = NEG_INF; st.best_r = 2 * R; st.best_j = -1;
    int lane_max = NEG_INF;                               // best H-3 of this lane, true 32-bit
    int gseen = NEG_INF;
    // Block pruning (AbstractBlockPruning::isBlockPrunable, M3): a 64-step slab of the strip is skipped when
    // nothing that enters it -- the lanes' own state, bounded by their last chunk maximum, and the bus
    // chunk from the strip above -- can reach the running best even if every remaining row/column matched.
    // Skipped cells count as H = 0, a lower bound of every SW cell, so later cells are never overestimated;
    // the test is strict, so cells that could TIE the best are still computed and the canonical position is
    // the unpruned one.  Only while the window sits at the floor (bias == 0): the reset must be
    // representable next to its neighbours.
    // a template parameter, not a run-time flag: the mere presence of the skip path changes the register
    // allocation of the hot loops (measured: -13 % on C2), so unpruned runs use a kernel without it
    // Round 4: (1) the same for GLOBAL alignments (no floor: skipped cells count as -INF, the bound is nw_upper16 against a
    // running LOWER bound of H[m][n] that every computed chunk raises, nw_lower16; gbest holds that bound instead of a
    // best score and travels along a chain of bands the same way).  (2) Neither recurrence needs the window at the floor
    // any more: while slabs are skipped the strip holds no score at all ("state_void"), and the first computed chunk
    // after them sets the window by what the bus brings and re-creates the skipped state under it.  Skipped cells that
    // the new window cannot hold saturate at its bottom -- still lower bounds of their true values, which lie within
    // 6 * (rows + columns in reach) of the bus cells the window was set by.
    constexpr bool prune_on = PRUNE;
    constexpr bool prune_nw = PRUNE && !SWF;
    // every pruning kernel subtracts with saturation where it turns H into T (SATT of wave_step16): skipped cells under a
    // window that has moved on sit at its bottom -- the floor of a local alignment as much as the -INF of a global one --
    // and H - 3 must not wrap around there
    constexpr bool PNW = PRUNE;
    int lane_entry = hmax_lane - T_OFF;                   // upper bound (T domain, true) of what this lane holds
    bool state_void = prune_nw && hmax <= NEG_INF / 2;    // wave-uniform: every lane holds skipped cells only
    const int pr_rows = pin32_16(a->prune_rows - 1 - row0);   // rows of the super-partition below the strip's first row
    const int pr_cols = pin32_16(a->prune_cols - 1);
    int pruned_slabs = 0;
    static_assert(!GOAL || (PRUNE && !SWF && !TRACK), "goal mode: global recurrence, pruning kernels, nothing tracked");
    // goal mode: the two bounds, a term that is off (-INF in the argument block) out of every value's reach
    const int goal_c = GOAL ? pin32_16(a->goal_bound_col) : NEG_INF, goal_r = GOAL ? pin32_16(a->goal_bound_row) : NEG_INF;
    const long long gcol = goal_c <= NEG_INF / 2 ? 0x7fffffffffffffffll : (long long) goal_c;
    const long long grow = goal_r <= NEG_INF / 2 ? 0x7fffffffffffffffll : (long long) goal_r;
    const bool goal_any = goal_c > NEG_INF / 2 || goal_r > NEG_INF / 2;    // (a partition of a batch that brought no bound: nothing goes)
    static_assert(!EDGE || (PRUNE && !SWF && !TRACK && !GOAL), "edge mode: global recurrence, pruning kernels, nothing tracked, no goal");
    const int prune_end = EDGE ? pin32_16(a->prune_end) : 0;   // edge mode: which edge(s) the alignment may end on (see edge_upper16)

    // seq1 window starts empty
#if PK16_WIDE
    constexpr int c1w_none = WORD16(255) | (WORD16(255) << 16);      // columns outside the matrix
#else
    constexpr int c1w_none = 0x00020002;
#endif
    lds->c1w[lane] = c1w_none; lds->c1w[64 + lane] = c1w_none; lds->c1w[128 + lane] = c1w_none;
    if (lane < 8) lds->c1w[192 + lane] = c1w_none;
    lds->c1s[lane] = 0x0c040c00; lds->c1s[64 + lane] = 0x0c040c00; lds->c1s[128 + lane] = 0x0c040c00;
    if (lane < 8) lds->c1s[192 + lane] = 0x0c040c00;
    bool simple1 = false, simple2 = false;                // the previous two chunks held only plain codes (< 4)

    DBG16(1, 1);
    long long tr_start = 0, tr_first = 0; int tr_spins = 0;
    if (a->trace != nullptr) tr_start = __builtin_amdgcn_s_memrealtime();
    // The first chunks of a strip are the critical path of the pipeline's start-up: the next strip cannot
    // begin before they are published.  Run them at raised priority so that they proceed at single-wave
    // speed instead of a quarter of the SIMD (measured: hop 250 us -> ~50 us with 4 waves per SIMD).
    __builtin_amdgcn_s_setprio(3);
    bool simple0 = false;
    bool exact_mode = false;                              // wave-uniform: run the exact-tracking code without a fast pass first
    bool pf_valid = false;                                // next chunk's inputs are in pf_* (wave-uniform)
    // (the prefetched inputs of the next chunk stay in a240..a243 until that chunk's head reads them: carried in
    //  ordinary registers across the chunk boundary they were spilled to scratch and reloaded with a wait, every chunk)
    bool nx_plain = false;                                // ... and only plain codes (< 4, < n_match_codes) are among them
    // Arguments the chunk loop uses, pinned in registers: left to itself the compiler re-reads them from the argument
    // block (s_load + s_waitcnt, a round trip to the scalar cache that the lone wavefront sits through) several times per chunk
    const int nmc = pin32_16(a->n_match_codes);
    int2* const busp = pin_ptr16(a->bus);
    const unsigned char* const seq1p = pin_ptr16(a->seq1);
    // reproducible pruning (KernelArgs::det_prefix): the bound this strip tests against is a word that is final before the strip
    // starts -- what the run began with and what the strips det_lag and more above found -- plus what the strip itself finds
    const bool det = prune_on && !GOAL && a->det_prefix != nullptr;
    // (det_floor: 0, or -det_lag in a stream that continues from a saved state, whose history lies in front of det_prefix[0])
    const int* const gbest_inp = pin_ptr16(det ? (const int*) &a->det_prefix[max(a->det_floor, s - a->det_lag)] : a->gbest_in);
    if (det) {
        int spins = 0;
        while (poll_agent16(gbest_inp) == DET_UNSET && spins < spin_limit) { __builtin_amdgcn_s_sleep(8); spins++; }
        if (spins >= spin_limit && lane == 0) atomicExch(a->error_flag, 1);
    }
    int det_found = NEG_INF;                              // det: what this strip has published so far (wave-uniform)
    const int poll_host = pin32_16(a->host_abort != nullptr ? 1 : 0);
    int* const stopp = pin_ptr16(a->stop_word);
    // the window (pruning kernels, a->win != nullptr): what of the predecessor's bus row is the skip constant without having
    // been written -- its gap [pf_glo, pf_ghi) and everything from pf_hi on -- as read together with the inputs of the chunk
    int* const winp = prune_on ? pin_ptr16(a->win) : nullptr;
    const bool windowed = prune_on && winp != nullptr;
    const int write_bus = pin32_16((prune_on && a->independent) ? 0 : 1);    // (the seed pass's strips share one bus row: they leave it alone)
    int pf_hi = 0x7fffffff, pf_glo = 0, pf_ghi = 0;
    int void_from = 0x7fffffff;                           // output column from which everything this strip has left is the constant
    bool my_gap_used = false, retired = false;
    const int2 skipcell = make_int2(SWF ? 0 : NEG_INF, NEG_INF);
    // BAND mode (the seed's segments, runtime.cpp::anchored_seed): the strip computes only the columns within band_w of a
    // straight line through the partition -- column band_c0 + row * band_slope / 65536 -- and treats everything else as skipped,
    // whatever the bound says: it starts void at the band's first chunk (as after a jump) and retires behind its last.  Every
    // path inside the band is a path of the matrix, so every score in it is the score of an alignment that exists.
    const bool band_mode = windowed && a->band_w > 0;
    int band_lo = 0, band_hi = 0x7fffffff;
    if (band_mode) {
        // (the line may leave the matrix -- sequences of unequal length: the path then runs along the last column / the first
        //  column, which stay inside the band)
        long long top = (long long) a->band_c0 + (((long long) row0 * a->band_slope_q16) >> 16);
        long long bot = top + (((long long) SH * a->band_slope_q16) >> 16);
        top = top < 0 ? 0 : (top > n ? n : top);
        bot = bot < 0 ? 0 : (bot > n ? n : bot);
        long long lo = (top - a->band_w) / CHUNK * CHUNK, hi = (bot + a->band_w + 2 * CHUNK - 1) / CHUNK * CHUNK;
        band_lo = pin32_16((int) (lo < 0 ? 0 : (lo > n ? n : lo)));
        band_hi = pin32_16((int) (hi > n ? n : (hi < 0 ? 0 : hi)));
    }
    int gb_next = NEG_INF;                                // running global best as of the previous chunk
    bool chain_asked = false;                             // this chunk's request went to a neighbouring band's word
    if (TRACK || prune_on) gb_next = poll_agent16(gbest_inp);
    int flag_pending = -1;                                // progress value whose bus stores are still in flight
    bool host_stop = false;
    bool last_skipped = false;                            // the chunk before this one was a pruned slab (pruning kernels)
    // ---- the chunk loop: ONE body, instantiated twice ----
    // The HOT instance takes the chunks in which nothing unusual can happen -- inputs prefetched, plain codes, full
    // width, no exact-mode stretch, nothing but the bus to write -- and holds only the code those need; whatever else
    // turns up in such a chunk (a candidate for the best score, a new maximum, a window shift) ends the hot loop, and
    // the GENERAL instance finishes that chunk from where the hot one stopped (resume_at) and takes every chunk the hot
    // loop may not.  The point is code layout, not arithmetic: the blocks of a loop are laid out together, so the hot
    // path no longer threads through the rare code of a 480 KB function with a far jump at every turn -- with one
    // wavefront per SIMD each taken branch costs tens of nanoseconds of refetch, and the old chunk boundary had ~15.
    int c = 0;
    s2 cmax_over[R];                                      // chunk maxima of a chunk handed over mid-way (kept apart: registers that
                                                          // both instances shared were spilled in one and waited for in the other)
    int rebias_to = bias;
    auto body = [&](auto hot_c, const int resume_at) __attribute__((always_inline)) -> int {
        // returns 0: chunk c is complete; 1 / 2 (hot only): continue it in the general body at the exact replay / at
        // the tail; 3: the host said stop
        constexpr bool HOT = decltype(hot_c)::value;
        const int col0 = c * CHUNK;
        if (!HOT && resume_at == 0) {
            // mustContinue() == false (stage-2/3 goal found): strips in flight give up at the next 64-chunk mark instead
            // of finishing their sweep; what they have produced is void, the host dispatches nothing after its stop
            // (... and tell every other strip of the stream: they look at the device word once per chunk, so all of them end
            //  within a chunk of the first that saw the host's word -- AbstractDiagonalAligner::alignPartition tests
            //  mustContinue() once per external diagonal and all its blocks end together, :64)
            if (UNLIKELY16((c & 63) == 63) && poll_host != 0 && poll_sys16(a->host_abort) != 0) {
                if (lane == 0) st_agent16(stopp, 1);
                host_stop = true;
                return 3;
            }
            // graded: the younger the strip, the closer it is to the start-up front of the pipeline
            if (UNLIKELY16(c == 8)) __builtin_amdgcn_s_setprio(2);
            else if (UNLIKELY16(c == 48)) __builtin_amdgcn_s_setprio(1);
            else if (UNLIKELY16(c == 256)) __builtin_amdgcn_s_setprio(0);
        }
        if (!HOT) { DBG16(2, c); DBG16(3, 10); }
        const bool trc = !HOT && resume_at == 0 && UNLIKELY16((a->trace != nullptr) && (c == 1000 || c == 1));
        long long q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0;
        if (UNLIKELY16(trc)) q0 = __builtin_amdgcn_s_memrealtime();
        bool skip = false;
        // (1) stage the input chunk: prefetched during the previous chunk when the predecessor was far enough
        //     ahead (the usual case), otherwise wait for it here
        if (HOT || resume_at == 0) {
            const int col = col0 + lane;
            int2 hf = make_int2(0, NEG_INF);
            int code = 255, codep = 255;
            if (HOT || LIKELY16(pf_valid)) {
                int b0, b1;
                ASYNC_GET("a240", hf.x); ASYNC_GET("a241", hf.y);
                ASYNC_GET("a242", b0); ASYNC_GET("a243", b1);
                code = b0 >> 2;
                codep = b1 >> 2;
                if (prune_on && windowed) {
                    int g0, g1;
                    ASYNC_GET("a246", g0); ASYNC_GET("a247", g1);
                    pf_glo = __builtin_amdgcn_readfirstlane(g0); pf_ghi = __builtin_amdgcn_readfirstlane(g1);
                }
            } else {
                // (experiment knob, see PK16_START_SLACK)
                int need = col0 + CHUNK + (c == 0 ? PK16_START_SLACK * CHUNK : 0);
                if (need > n) need = n;
                if (col0 < n) {
                    int spins = 0, pv;
                    while ((pv = poll_agent16(prog_in)) < need && spins < spin_limit) {
                        __builtin_amdgcn_s_sleep(2);
                        spins++;
                        // (a strip that waits for the strip above sees a stop here: nothing more will come)
                        if ((spins & 7) == 0 && poll_agent16(stopp) != 0) { host_stop = true; break; }
                    }
                    if (host_stop) return 3;
                    tr_spins += spins;
                    if (spins >= spin_limit && lane == 0) atomicExch(a->error_flag, 1);
                    if (prune_on && windowed) {             // (the gap is read AFTER the progress value that covers it)
                        pf_hi = pv >= WIN_RETIRED ? pv - WIN_RETIRED : 0x7fffffff;
                        const int2 g = ld_agent2_16((const int2*) &winp[2 * s]);
                        pf_glo = __builtin_amdgcn_readfirstlane(g.x); pf_ghi = __builtin_amdgcn_readfirstlane(g.y);
                    }
                }
                if (col < n) {
                    hf = ld_agent2_16(&busp[col]);
                    code = ld_u8_16(&seq1p[col]) >> 2;        // seq1 holds code*4 (shift form of the int32 kernel)
                }
                if (col >= 1 && col - 1 < n) codep = ld_u8_16(&seq1p[col - 1]) >> 2;
            }
            pf_valid = false;
            // the window: cells the strip above left unwritten are the skip constant, whatever the bus memory holds
            if (prune_on && windowed && (col >= pf_hi || (col >= pf_glo && col < pf_ghi))) hf = skipcell;
            if (TRACK || prune_on) {
                // Seed: a cell below the best score already found anywhere can never be the answer, so every
                // lane starts from the global running best (ties are still taken: the test below is >=).
                // Without it each strip spends its first chunks in the exact path and the start-up delay of
                // every hop of the strip pipeline triples.  The value was requested one chunk ago.
                gseen = gb_next;                           // requested one chunk ago, settled at that chunk's end
                if (TRACK && gseen > st.best_t) { st.best_t = gseen; st.best_r = 2 * R; st.best_j = -1; }
                // a chain of column bands shares its running best (pruning kernels only): every 16th chunk asks a
                // neighbour's word instead of this GPU's own -- the band on the left stores into this band's port, the
                // band on the right is read over the link; the answer is folded in at the end of the chunk
                chain_asked = false;
                if (prune_on && (c & 15) == 5 && a->chain_down_in != nullptr) { ASYNC_LD32_SYS("a245", a->chain_down_in); chain_asked = true; }
                else if (prune_on && (c & 15) == 13 && a->chain_up_in != nullptr) { ASYNC_LD32_SYS("a245", a->chain_up_in); chain_asked = true; }
                else ASYNC_LD32("a245", gbest_inp);
            }
            if (UNLIKELY16(trc)) q1 = __builtin_amdgcn_s_memrealtime();
#if PK16_WIDE
            const int mk = WORD16(code), mkp = WORD16(codep);
#else
            const int mk = ((code < nmc) ? (4 << code) : 0) | 2;
            const int mkp = ((codep < nmc) ? (4 << codep) : 0) | 2;
#endif
            // (local alignments: the chunks at the END of the row -- the last, partly filled one and the two in which only the
            //  trailing lanes still hold columns -- are asked too.  A strip that RETIRES (fast_forward) never computes them; one
            //  that walks the same skipped region because the strip above had not yet said "retired" used to: cells with H = 0,
            //  E = -5 instead of the skip constant's E = -INF in its last column -- a difference that depended on timing alone
            //  (found by tools/det_prune_stress.py).  The test is monotone in the column: where the one passes, so does the other.)
            if (prune_on && col0 >= 128 && (SWF || col0 + CHUNK <= n)) {
                if (SWF) {
                    const int left = min(pr_rows + 2, pr_cols + 1 - (col0 - 128));
                    int e = lane_entry;
                    if (col < n) e = max(e, hf.x - T_OFF);
                    skip = !__any(e + left + SW_PRUNE_MARGIN >= gseen);
                } else if (GOAL) {
                    // (the same two entries as below, held against the sweep's own bounds: see goal_keep16)
                    const bool own = goal_keep16(lane_entry, pr_rows - 2 * lane * R, pr_cols - col0 + 2 * lane + 4, 2 * R - 1, gcol, grow);
                    const bool top = goal_keep16(col < n ? hf.x - T_OFF : NEG_INF, pr_rows + 1, pr_cols - col + 1, 0, gcol, grow);
                    skip = goal_any && !__any(own || top);
                } else {
                    // what enters the slab: the lane's own last column (rows of its two blocks, columns col0 - 2 lane - 4 ..
                    // + 1 with room to spare) and the bus cell of its column (row above the strip)
                    const int own = EDGE ? edge_upper16(prune_end, lane_entry, pr_rows - 2 * lane * R, pr_cols - col0 + 2 * lane + 4, 2 * R - 1, 5)
                                         : nw_upper16(lane_entry, pr_rows - 2 * lane * R, pr_cols - col0 + 2 * lane + 4, 2 * R - 1, 5);
                    const int top = EDGE ? edge_upper16(prune_end, col < n ? hf.x - T_OFF : NEG_INF, pr_rows + 1, pr_cols - col + 1, 0, 1)
                                         : nw_upper16(col < n ? hf.x - T_OFF : NEG_INF, pr_rows + 1, pr_cols - col + 1, 0, 1);
                    skip = !__any(max(own, top) >= gseen);
                }
            }
            // Pruning kernels: the bus row is not smooth any more.  Where the strip above went from skipping to computing, its
            // bottom row jumps from the skipped value to scores that may lie far above this strip's window -- whose own cells,
            // computed next to skipped ones, are lower bounds and may be low.  The window then follows the bus: cells it
            // leaves behind saturate at its bottom, which is still below their true values (those lie within 6 * (rows +
            // columns in reach) of the bus cells the window is set by).  The hot loop has no code for this: it hands the
            // chunk over untouched (the prefetched inputs stay in their registers).
            const bool bus_above = prune_on && !skip && __any(col < n && hf.x - T_OFF - bias > REBASE_HI);
            if (HOT && prune_on && bus_above) { pf_valid = true; return 4; }
            if (prune_on && !HOT && !skip && (state_void || bus_above)) {
                int xr = (col < n && hf.x > NEG_INF / 2) ? hf.x : NEG_INF;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) xr = max(xr, __shfl_xor(xr, d));
                xr = __builtin_amdgcn_readfirstlane(xr);
                if (xr <= NEG_INF / 2 && state_void) {
                    // the strip holds nothing and the bus brings nothing: every cell of the slab is -INF whatever the
                    // bound says (chunks at the ends of a row, which the bound is not asked about, and the time before the
                    // first lower bound is known).  Computing them would turn images of -INF into numbers.
                    skip = true;
                } else if (xr > NEG_INF / 2 && state_void) {
                    // first computed chunk after skipped ones: the strip holds no score, so the window is set by what the
                    // bus brings and the skipped state is created again under it
                    if (SWF) bias = xr > REBASE_HI ? xr - REBASE_TO : 0;
                    else bias = (xr > REBASE_HI || xr < REBASE_LO) ? xr - REBASE_TO : 0;
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        Z[r] = splat(clamp16(2 * r - bias));
                        st.TL[r] = SWF ? splat(clamp16(-T_OFF + 2 * r - bias)) : splat(-32768);
                        st.E[r] = splat(-32768);
                    }
                    st.tup_prev = SWF ? splat(clamp16(-T_OFF - 2 - bias)) : splat(-32768);
                    st.tbot = st.tup_prev;
                    st.fbot = splat(-32768);
                    state_void = false;
                } else if (xr > NEG_INF / 2 && xr - REBASE_TO > bias) {
                    // (a shift of more than 16 bits leaves nothing above the window's bottom: three saturating steps)
                    int rem = xr - REBASE_TO - bias;
#pragma unroll 1
                    for (int k3 = 0; k3 < 3 && rem > 0; k3++) {
                        const s2 dlt = splat(min(rem, 32767));
                        rem -= min(rem, 32767);
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            st.TL[r] = __builtin_elementwise_sub_sat(st.TL[r], dlt);
                            st.E[r] = __builtin_elementwise_sub_sat(st.E[r], dlt);
                        }
                        st.tup_prev = __builtin_elementwise_sub_sat(st.tup_prev, dlt);
                        st.tbot = __builtin_elementwise_sub_sat(st.tbot, dlt);
                        st.fbot = __builtin_elementwise_sub_sat(st.fbot, dlt);
                    }
                    bias = xr - REBASE_TO;
#pragma unroll
                    for (int r = 0; r < R; r++) Z[r] = splat(clamp16(2 * r - bias));
                }
            }
            if (!skip) {
                if (col < n && hf.x - T_OFF - bias > GUARD16) overflow |= OVF16_BUS_ABOVE;
                // (no floor to hide behind -- but in a pruning kernel a cell far below the window is a skipped cell or a
                //  lower bound computed next to one, and saturates like them)
                if (!SWF && !PRUNE && col < n && hf.x - T_OFF - bias < -GUARD16) overflow |= OVF16_BUS_BELOW;
            }
            // shift the window by one chunk, then append
            const int w0 = lds->c1w[64 + lane];
            const int w1 = lds->c1w[128 + lane];
            lds->c1w[lane] = w0;
            lds->c1w[64 + lane] = w1;
            lds->c1w[128 + lane] = mk | (mkp << 16);
            const int v0 = lds->c1s[64 + lane];
            const int v1 = lds->c1s[128 + lane];
            lds->c1s[lane] = v0;
            lds->c1s[64 + lane] = v1;
            lds->c1s[128 + lane] = (code & 3) | 0x0c000c00 | ((4 + (codep & 3)) << 16);
            simple2 = simple1; simple1 = simple0;
            simple0 = HOT || ((col0 + CHUNK <= n) && !__any(code >= 4 || code >= nmc));   // (hot: tested before the chunk was taken)
            lds->in_tf[lane] = make_int2(clamp16(hf.x - T_OFF - bias - 2) << 16, clamp16(hf.y - bias - 2) << 16);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ask for the predecessor's progress now, look at the answer in the middle of the chunk
            ASYNC_LD32("a244", prog_in);
            ASYNC_LD32("a248", stopp);                     // ... and for the stop word, looked at when the chunk ends
        }
        if (UNLIKELY16(trc)) q2 = __builtin_amdgcn_s_memrealtime();
        if (!HOT) DBG16(3, 20);
        // (2) 64 systolic steps
        const int jl = col0 - 2 * lane;
        const bool masked = !HOT && ((col0 - 127 < 0) || (col0 + CHUNK - 1 >= n));
        s2 cmax[R];
#pragma unroll
        for (int r = 0; r < R; r++) cmax[r] = (HOT || resume_at == 0) ? splat(-32768) : cmax_over[r];
        rebias_to = bias;
        // Fast pass: no position bookkeeping at all.  Only if some lane's chunk maximum reaches its
        // (globally seeded) threshold is the chunk replayed from a register snapshot with the exact
        // per-step bookkeeping -- a rare event once the running best is above the background level.
        // While chunks keep producing new candidates (start of the run, a ridge of a real alignment) the
        // fast pass would be thrown away every time: such stretches run the exact code directly
        // (exact_mode), one pass per chunk, and return to the fast pass after a chunk without any update.
        Lane16<R> snap;
        if (TRACK && (HOT || resume_at == 0) && !exact_mode && !skip) {
#pragma unroll
            for (int r = 0; r < R; r++) { snap.TL[r] = st.TL[r]; snap.E[r] = st.E[r]; }
            snap.tup_prev = st.tup_prev; snap.tbot = st.tbot; snap.fbot = st.fbot;
        }
        constexpr bool HALF = TRACK && (PK16_HALFTRACK != 0);
        constexpr int SLACK = HALF ? 5 : 0;                // what an untracked (even) row can exceed its neighbour by
        // The ragged last strip runs the ordinary code (rows past m are ordinary cells that never match);
        // only when its DP row m-1 is wanted (last row) does the emit position have to move off the bottom.
        // ---- mid-chunk service: everything that needs a memory round trip happens here, half a chunk after
        //      it was requested, so that no latency is exposed at the chunk boundary ----
        auto service = [&](const int second) {
            // (a) the previous chunk's bus stores have landed by now: publish them
            if (!second) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (flag_pending >= 0) {
                    if (lane == 0) st_agent16(prog_out, flag_pending);
                    flag_pending = -1;
                }
            }
            // (b) is the next input chunk already there?  Then fetch it now (the loads are issued after the
            //     progress value was observed, so they see the published data); otherwise ask again for the
            //     second service point
            const int ncol0 = col0 + CHUNK;
            if (c + 1 < nchunks && !pf_valid) {
                int need = ncol0 + CHUNK;
                if (need > n) need = n;
                int avail_v;
                ASYNC_GET("a244", avail_v);
                const int avail = __builtin_amdgcn_readfirstlane(avail_v);
                if (ncol0 >= n || avail >= need) {
                    const int col = ncol0 + lane;
                    if (prune_on && windowed) {             // what of the predecessor's row is unwritten, as of this progress value
                        pf_hi = avail >= WIN_RETIRED ? avail - WIN_RETIRED : 0x7fffffff;
                        ASYNC_LD64_246((const int2*) &winp[2 * s]);
                    }
                    ASYNC_SET("a240", 0); ASYNC_SET("a241", NEG_INF);          // (H,F) = (0,-INF) past the end
                    ASYNC_SET("a242", 255 << 2); ASYNC_SET("a243", 255 << 2);
                    if (col < n) {
                        ASYNC_LD64_240(&busp[col]);
                        ASYNC_LD8("a242", &seq1p[col]);
                    }
                    if (col >= 1 && col - 1 < n) ASYNC_LD8("a243", &seq1p[col - 1]);
                    pf_valid = true;
                } else if (!second) {
                    ASYNC_LD32("a244", prog_in);
                }
            }
        };
        const bool use_perm = !masked && !emit_any && simple0 && simple1 && simple2;
        auto skip_slab = [&]() {
            // the slab is not computed: every cell in it counts as H = 0 (T = -3), E = F = -INF -- as everything -INF where
            // there is no floor.  The window goes back to the floor with it (nothing is left that it would have to hold).
            if (SWF && bias != 0) {
                bias = 0;
#pragma unroll
                for (int r = 0; r < R; r++) Z[r] = splat(clamp16(2 * r));
            }
            rebias_to = bias;
#pragma unroll
            for (int r = 0; r < R; r++) {
                st.TL[r] = SWF ? splat(-T_OFF + 2 * r) : splat(-32768);
                st.E[r] = splat(-32768);
                cmax[r] = st.TL[r];
            }
            st.tup_prev = SWF ? splat(-T_OFF - 2) : splat(-32768);
            st.tbot = st.tup_prev;
            st.fbot = splat(-32768);
            const int t_skip = SWF ? pack(-T_OFF + 2 * emit_row, -T_OFF + 2 * emit_row) : (int) 0x80008000;
#if PK16_OUT2D
            lds->out2[lane][emit_lane] = make_int2(t_skip, 0x80008000);
#else
            lds->out_tf[lane] = make_int2(t_skip, 0x80008000);
#endif
            exact_mode = false;
            pruned_slabs++;
            last_skipped = true;
            state_void = true;
            if (void_from == 0x7fffffff) void_from = max(0, col0 - 127);
            service(0);
        };
        bool replay = !HOT && resume_at == 1;
        if (prune_on && !skip) { last_skipped = false; void_from = 0x7fffffff; }     // (state_void stays until a computed chunk has set the window)
        if (HOT && prune_on && skip) {         // (pruned slabs come in long runs: they belong to the hot loop)
            skip_slab();
        } else if (HOT) {
            run_chunk16<R, false, false, false, HALF, true, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax, service);
            if (TRACK && UNLIKELY16(__any(chunk_max16<R, HALF>(cmax) + SLACK + bias >= st.best_t))) {
                // back to the snapshot here, so that it does not have to outlive the hot loop
#pragma unroll
                for (int r = 0; r < R; r++) { st.TL[r] = snap.TL[r]; st.E[r] = snap.E[r]; }
                st.tup_prev = snap.tup_prev; st.tbot = snap.tbot; st.fbot = snap.fbot;
#pragma unroll
                for (int r = 0; r < R; r++) cmax_over[r] = cmax[r];
                return 1;
            }
        } else if (resume_at == 0) {
        if (UNLIKELY16(skip)) {
            skip_slab();
        } else
        if (TRACK && UNLIKELY16(exact_mode)) {
            const int bt0 = st.best_t, bj0 = st.best_j, br0 = st.best_r;
            if (emit_any) run_chunk16<R, true, true, true, false, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, cmax, service, !ragged);
            else if (masked) run_chunk16<R, true, true, false, false, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax, service, !ragged);
            else run_chunk16<R, false, true, false, false, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax, service, !ragged);
            exact_mode = __any(st.best_t != bt0 || st.best_j != bj0 || st.best_r != br0);
        } else {
        if (LIKELY16(use_perm)) run_chunk16<R, false, false, false, HALF, true, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax, service);
        else if (emit_any && masked) run_chunk16<R, true, false, true, HALF, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, cmax, service);
        else if (emit_any) run_chunk16<R, false, false, true, HALF, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, cmax, service);
        else if (masked) run_chunk16<R, true, false, false, HALF, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax, service);
        else run_chunk16<R, false, false, false, HALF, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax, service);
        if (TRACK) replay = UNLIKELY16(__any(chunk_max16<R, HALF>(cmax) + SLACK + bias >= st.best_t));
        }
        }
        if (!HOT && TRACK) {
            if (UNLIKELY16(replay)) {
                if (resume_at == 0) {
#pragma unroll
                    for (int r = 0; r < R; r++) { st.TL[r] = snap.TL[r]; st.E[r] = snap.E[r]; }
                    st.tup_prev = snap.tup_prev; st.tbot = snap.tbot; st.fbot = snap.fbot;
                }
                s2 cmax2[R];
#pragma unroll
                for (int r = 0; r < R; r++) cmax2[r] = splat(-32768);
                if (emit_any) run_chunk16<R, true, true, true, false, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, emit_lane, emit_row, Z, bias, cmax2, NoService16(), !ragged);
                else if (masked) run_chunk16<R, true, true, false, false, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax2, NoService16(), !ragged);
                else run_chunk16<R, false, true, false, false, false, SWF, PNW>(st, lds, lane, jl, n, nvalid_lo, nvalid_hi, 63, R - 1, Z, bias, cmax2, NoService16(), !ragged);
                exact_mode = (PK16_EXACT_MODE != 0);
            }
        }
        if (UNLIKELY16(trc)) q3 = __builtin_amdgcn_s_memrealtime();
        if (!HOT) DBG16(3, 30);
        // chunk maximum: range guard, publication of a new global best, re-centring of the 16-bit window
        {
            const int cmv = chunk_max16<R, HALF>(cmax);    // exact, or a lower bound within SLACK of it
            if (cmv + SLACK > GUARD16) {
                if (!(overflow & OVF16_CHUNK_MAX) && atomicCAS(a->error_flag + 7, 0, 1) == 0) {   // diagnostics of the first report (quoted by the host)
                    a->error_flag[3] = c; a->error_flag[4] = bias; a->error_flag[5] = cmv;
                    a->error_flag[6] = (HOT ? 1 : 0) | (skip ? 2 : 0) | ((prune_on && state_void) ? 4 : 0) | (resume_at << 4) | (lane << 8) | (s << 16);
                }
                overflow |= OVF16_CHUNK_MAX;
            }
            lane_max = max(lane_max, cmv + bias);
            lane_entry = (prune_nw && skip) ? NEG_INF : cmv + SLACK + bias;
            // global alignments with pruning: what this chunk's cells say about H[m][n] from below.  The lane's maximum is
            // the score of one of its cells -- rows of its two blocks, columns col0 - 2 lane - 1 .. + 63 -- wherever it is.
            int lbv = NEG_INF;
            if (prune_nw && !GOAL && !skip && !masked && nvalid_lo == R && nvalid_hi == R) {   // (goal mode: the bound is fixed)
                const long long ki = (long long) pr_rows - 2 * lane * R, dj = (long long) pr_cols - col0 + 2 * lane + 1;
                const long long dhi = dj - (ki - (2 * R - 1)), dlo = (dj - 64) - ki;
                lbv = EDGE ? edge_lower16(prune_end, cmv + bias, ki < dj ? ki : dj, dlo, dhi) : nw_lower16(cmv + bias, ki < dj ? ki : dj, dhi > -dlo ? dhi : -dlo);
            }
            // the wave-wide maximum (six cross-lane steps) is only needed when one of its three consumers
            // can fire; three ballots decide that
            const bool need_wmax = !(prune_on && skip) &&
                                   (__any(cmv + SLACK > REBASE_HI) || ((TRACK || (prune_on && SWF)) && __any(cmv + bias > gseen)) ||
                                    (prune_nw && __any(lbv > gseen)) ||
                                    (SWF ? (bias > 0 && !__any(cmv >= 0)) : !__any(cmv >= REBASE_LO)));
            if (HOT && UNLIKELY16(need_wmax)) {
#pragma unroll
                for (int r = 0; r < R; r++) cmax_over[r] = cmax[r];
                return 2;
            }
            if (!HOT && UNLIKELY16(need_wmax)) {
                int w = cmv;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) w = max(w, __shfl_xor(w, d));
                const int wmax = __builtin_amdgcn_readfirstlane(w);
                int news = wmax + bias;                    // what the running best may learn from this chunk
                if (prune_nw) {
                    int wl = lbv;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) wl = max(wl, __shfl_xor(wl, d));
                    news = __builtin_amdgcn_readfirstlane(wl);
                }
                if (prune_on && det && news > gseen) {      // (the strip's own finds count for its later chunks: left to right, no timing in it)
                    det_found = max(det_found, news);
                    gb_next = max(gb_next, news);
                }
                if ((TRACK || prune_on) && !GOAL && news > gseen) {
                    if (lane == 0) {
                        atomicMax(a->gbest, news);
                        if (prune_on) {     // tell the neighbouring bands at once (they fold it into their own gbest)
                            if (a->chain_up_pub != nullptr) st_sys16(a->chain_up_pub, news);
                            if (a->chain_down_pub != nullptr) st_sys16(a->chain_down_pub, news);
                        }
                    }
                }
                int nb = bias;
                if (wmax + SLACK > REBASE_HI) nb = bias + (wmax - REBASE_TO);
                else if (SWF && wmax < 0 && bias > 0 && wmax > -32768) nb = max(0, bias + max(wmax - REBASE_TO, -30000));
                else if (!SWF && wmax < REBASE_LO && wmax > -32768) nb = bias + max(wmax - REBASE_TO, -30000);
                if (nb != bias) {
                    // shift every live 16-bit value by the same amount (saturating: the -INF image stays put
                    // when the window moves up); outputs of this chunk were produced with the old bias
                    rebias_to = nb;
                }
            }
        }
        // everything requested asynchronously during this chunk has long arrived: wait for it BEFORE this chunk's bus
        // stores are issued (the wait must not wait for those); the next chunk's inputs stay where they landed
        ASYNC_WAIT();
        {
            // somebody saw the host's stop (see the poll at the head of the general body): what this strip has is void
            int sw_;
            ASYNC_GET("a248", sw_);
            if (UNLIKELY16(__builtin_amdgcn_readfirstlane(sw_) != 0)) { host_stop = true; return 3; }
        }
        if (pf_valid) {
            int b0;
            ASYNC_GET("a242", b0);
            nx_plain = !__any((b0 >> 2) >= 4 || (b0 >> 2) >= nmc);
        }
        if (TRACK || prune_on) {
            int g;
            ASYNC_GET("a245", g);
            g = __builtin_amdgcn_readfirstlane(g);
            if (prune_on && chain_asked && g > gb_next) {
                // news from a neighbouring band: into this GPU's gbest, and onwards in both directions
                if (lane == 0) {
                    atomicMax(a->gbest, g);
                    if (a->chain_up_pub != nullptr) st_sys16(a->chain_up_pub, g);
                    if (a->chain_down_pub != nullptr) st_sys16(a->chain_down_pub, g);
                }
            }
            gb_next = prune_on ? max(gb_next, g) : g;
        }
        // (3) output chunk: columns col0-emit_v .. col0-emit_v+63
        {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#if PK16_OUT2D
            const int2 tf = lds->out2[lane][emit_lane];    // step `lane` of the chunk, the emitting lane's column
#else
            const int2 tf = lds->out_tf[lane];
#endif
            const int col = col0 - emit_v + lane;
            if (col >= 0 && col < n) {
                const int t16 = emit_half ? hi16(tf.x) : lo16(tf.x);
                const int f16 = emit_half ? hi16(tf.y) : lo16(tf.y);
                // -32768 is the sticky image of -INF (only border rows can carry it)
                // (pruning without a floor: skipped cells are -INF in H as well)
                const int2 hf = make_int2((prune_nw && t16 == -32768) ? NEG_INF : t16 + T_OFF + bias - 2 * emit_row,
                                          f16 == -32768 ? NEG_INF : f16 + bias - 2 * emit_row);
                if (!prune_on || write_bus) st_agent2_16(&busp[col], hf);
                if (!HOT && UNLIKELY16(special != nullptr)) special[col] = hf;
                if (!HOT && UNLIKELY16(lastrow != nullptr)) lastrow[col] = hf;
                if (!HOT && UNLIKELY16(ckpt != nullptr)) ckpt[col] = hf;
            }
            // the progress flag follows at the next mid-chunk service (or after the last chunk), when the
            // stores have drained without anybody waiting for them
            int done = col0 - emit_v + CHUNK;
            if (done > n) done = n;
            if (done < 0) done = 0;
            flag_pending = done;
        }
        if (!HOT && UNLIKELY16(rebias_to != bias)) {
            const s2 dlt = splat(rebias_to - bias);
#pragma unroll
            for (int r = 0; r < R; r++) {
                st.TL[r] = __builtin_elementwise_sub_sat(st.TL[r], dlt);
                st.E[r] = __builtin_elementwise_sub_sat(st.E[r], dlt);
            }
            st.tup_prev = __builtin_elementwise_sub_sat(st.tup_prev, dlt);
            st.tbot = __builtin_elementwise_sub_sat(st.tbot, dlt);
            st.fbot = __builtin_elementwise_sub_sat(st.fbot, dlt);
            bias = rebias_to;
#pragma unroll
            for (int r = 0; r < R; r++) Z[r] = splat(clamp16(2 * r - bias));
        }
        if (UNLIKELY16(trc) && lane == 0) {
            q4 = __builtin_amdgcn_s_memrealtime();
            long long* tr = a->trace + 4 * s;
            const long long v = ((q1 - q0) & 0xffff) | (((q2 - q1) & 0xffff) << 16) | (((q3 - q2) & 0xffff) << 32) | (((q4 - q3) & 0xffff) << 48);
#ifdef PK16_TRACE_ABS   // absolute times (after the input wait) of chunk 1 and chunk 1000 instead of the phase split
            if (c == 1) tr[2] = q1; else tr[3] = q1;
#else
#ifndef PK16_TRACE_BAND
            if (c == 1) tr[2] = v; else tr[3] = v;
#endif
#endif
        }
        return 0;
    };
    // Pruned slabs come in long runs (everything left of the frontier in the lower part of the matrix), and taken one by
    // one each of them is three memory round trips of a microsecond with nothing to hide them behind (the predecessor's
    // progress, the bus chunk for the test, the prefetch of the next one): 3.5 us per slab against 15-20 for a computed
    // one, 12 % of a run that prunes 45 %.  After a skipped slab the state of the strip is a constant (every cell H = 0),
    // so the test of the FOLLOWING slabs depends on nothing but the bus cells above them: up to PK16_FF of them are
    // fetched and tested in one go, and those that can go are written out together -- their bus cells (0, -INF), the two
    // chunks of column codes the window must hold afterwards, one progress flag.  Same decisions as slab by slab (the
    // running best is only as fresh as at the first of them: a weaker bound, never a wrong one), same cells, same counts.
    auto set_prio_for = [&](const int cc) {                // the graded start-up priority of the chunk loop, for a strip that jumps
        if (cc >= 256) __builtin_amdgcn_s_setprio(0);
        else if (cc >= 48) __builtin_amdgcn_s_setprio(1);
        else if (cc >= 8) __builtin_amdgcn_s_setprio(2);
    };
    auto fast_forward = [&]() -> int {
        constexpr int FF = PK16_FF;
        const int col0 = c * CHUNK;
        if (FF == 0 || emit_any || (SWF && bias != 0)) { last_skipped = false; return 0; }
        if (poll_agent16(stopp) != 0) { host_stop = true; return 0; }
        int avail = poll_agent16(prog_in);
        int hi_p = 0x7fffffff, glo_p = 0, ghi_p = 0;
        int count = 0, kmax = 0;
        bool jumped = false;
        if (windowed) {
            hi_p = avail >= WIN_RETIRED ? avail - WIN_RETIRED : 0x7fffffff;
            const int2 g = ld_agent2_16((const int2*) &winp[2 * s]);       // (after the progress value: it covers what the gap says)
            glo_p = __builtin_amdgcn_readfirstlane(g.x); ghi_p = __builtin_amdgcn_readfirstlane(g.y);
            if (c >= 3 && col0 + CHUNK <= n) {
                // With nothing but skipped cells above it -- and nothing but skipped cells in the strip itself: this is the
                // state after a skipped slab -- can the slab at col0 go?  Then every later slab over skipped cells goes too:
                // the same rows left, fewer columns (local); nothing enters at all (global).
                bool go = true;
                if (SWF) {
                    const int left = min(pr_rows + 2, pr_cols + 1 - (col0 - 128));
                    go = !__any(max(lane_entry, -T_OFF) + left + SW_PRUNE_MARGIN >= gb_next);
                }
                if (go && hi_p <= col0) {
                    // the strip above left nothing but skipped cells from here on, and so does this one: done
                    retired = true;
                    pruned_slabs += (n - col0) / CHUNK;
                    return 0;
                }
                if (go && !my_gap_used && glo_p <= col0 && ghi_p >= col0 + CHUNK) {
                    // the strip above jumped over these columns: jump with it, in one step, nothing written
                    count = (min(ghi_p, n) - col0) / CHUNK;
                    jumped = true;
                }
            }
        }
        if (avail > n) avail = n;
        if (!jumped) {
            if (c <= 256) { last_skipped = false; return 0; }
            kmax = (avail - col0) / CHUNK;                  // whole chunks the strip above has published from here on
            if (kmax > FF) kmax = FF;
            if (poll_host != 0 && kmax > 63 - (c & 63)) kmax = 63 - (c & 63);    // the stop poll keeps its chunk
            if (kmax <= 0) { last_skipped = false; return 0; }
            int h[FF];
#pragma unroll
            for (int k = 0; k < FF; k++) {
                h[k] = NEG_INF;
                if (k < kmax) {
                    const int colk = col0 + k * CHUNK + lane;
                    h[k] = __hip_atomic_load(&busp[colk].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (windowed && (colk >= hi_p || (colk >= glo_p && colk < ghi_p))) h[k] = skipcell.x;
                }
            }
            const int gs = gb_next;
#pragma unroll
            for (int k = 0; k < FF; k++) {
                if (k < kmax && count == k) {
                    if (SWF) {
                        const int left = min(pr_rows + 2, pr_cols + 1 - (col0 + k * CHUNK - 128));
                        const int e = max(lane_entry, h[k] - T_OFF);
                        if (!__any(e + left + SW_PRUNE_MARGIN >= gs)) count = k + 1;
                    } else if (GOAL) {
                        if (goal_any && !__any(goal_keep16(h[k] - T_OFF, pr_rows + 1, pr_cols - (col0 + k * CHUNK + lane) + 1, 0, gcol, grow))) count = k + 1;
                    } else {
                        // (the strip holds nothing: only the bus cells can bring a path in)
                        const int top = EDGE ? edge_upper16(prune_end, h[k] - T_OFF, pr_rows + 1, pr_cols - (col0 + k * CHUNK + lane) + 1, 0, 1)
                                             : nw_upper16(h[k] - T_OFF, pr_rows + 1, pr_cols - (col0 + k * CHUNK + lane) + 1, 0, 1);
                        if (!__any(top >= gs)) count = k + 1;
                    }
                }
            }
            if (count == 0) { last_skipped = false; return 0; }
            // bus cells of the skipped slabs: the emit row trails the chunk by emit_v = 127 columns
            const int2 hf0 = skipcell;
#pragma unroll
            for (int k = 0; k < FF; k++) {
                const int col = col0 + k * CHUNK - emit_v + lane;
                if (k < count && col >= 0 && col < n) {
                    if (write_bus) st_agent2_16(&busp[col], hf0);
                    if (UNLIKELY16(special != nullptr)) special[col] = hf0;
                    if (UNLIKELY16(lastrow != nullptr)) lastrow[col] = hf0;
                    if (UNLIKELY16(ckpt != nullptr)) ckpt[col] = hf0;
                }
            }
        } else {
            // this strip's own gap: output columns [col0 - 127, col0 + 64 count - 127) stay unwritten (rows that must exist in
            // memory were pre-filled with the constant by the host); published before the progress value below covers them
            if (lane == 0) st_agent2_16((int2*) &winp[2 * (s + 1)], make_int2(max(0, col0 - emit_v), col0 + count * CHUNK - emit_v));
            my_gap_used = true;
            if (poll_host != 0 && poll_sys16(a->host_abort) != 0) {    // (the stop polls of the chunks jumped over)
                if (lane == 0) st_agent16(stopp, 1);
                host_stop = true;
            }
            set_prio_for(c + count);
        }
        // the window of column codes as the chunk after the run expects it: its two predecessors in slots 1 and 2
        {
            const int cb = col0 + (count - 1) * CHUNK + lane, ca = cb - CHUNK;
            const int codeA = ld_u8_16(&seq1p[ca]) >> 2, codepA = ld_u8_16(&seq1p[ca - 1]) >> 2;
            const int codeB = ld_u8_16(&seq1p[cb]) >> 2, codepB = ld_u8_16(&seq1p[cb - 1]) >> 2;
#if PK16_WIDE
            const int mkA = WORD16(codeA), mkpA = WORD16(codepA), mkB = WORD16(codeB), mkpB = WORD16(codepB);
#else
            const int mkA = ((codeA < nmc) ? (4 << codeA) : 0) | 2, mkpA = ((codepA < nmc) ? (4 << codepA) : 0) | 2;
            const int mkB = ((codeB < nmc) ? (4 << codeB) : 0) | 2, mkpB = ((codepB < nmc) ? (4 << codepB) : 0) | 2;
#endif
            lds->c1w[64 + lane] = mkA | (mkpA << 16);
            lds->c1w[128 + lane] = mkB | (mkpB << 16);
            lds->c1s[64 + lane] = (codeA & 3) | 0x0c000c00 | ((4 + (codepA & 3)) << 16);
            lds->c1s[128 + lane] = (codeB & 3) | 0x0c000c00 | ((4 + (codepB & 3)) << 16);
            simple1 = !__any(codeA >= 4 || codeA >= nmc);
            simple0 = !__any(codeB >= 4 || codeB >= nmc);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int done = col0 + count * CHUNK - emit_v;
        if (done > n) done = n;
        if (done < 0) done = 0;
        if (lane == 0) st_agent16(prog_out, done);
        flag_pending = -1;
        pruned_slabs += count;
        pf_valid = false;
        nx_plain = false;
        last_skipped = jumped || (count == kmax);          // everything that was there went: look again
        return count;
    };
    // band mode: everything left of the band is skipped -- start void at the band's first chunk, as if a run of skipped slabs
    // had just ended there (the state skip_slab leaves, the gap and the progress word fast_forward's jump publishes)
    if (band_mode && band_lo / CHUNK >= 3) {
        c = band_lo / CHUNK;
        if (SWF) bias = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            Z[r] = splat(clamp16(2 * r - bias));
            st.TL[r] = SWF ? splat(-T_OFF + 2 * r) : splat(-32768);
            st.E[r] = splat(-32768);
        }
        st.tup_prev = SWF ? splat(-T_OFF - 2) : splat(-32768);
        st.tbot = st.tup_prev;
        st.fbot = splat(-32768);
        lane_entry = SWF ? -T_OFF + 5 : NEG_INF;
        lane_max = NEG_INF;
        state_void = true;
        {
            const int cb = (c - 1) * CHUNK + lane, ca = cb - CHUNK;
            const int codeA = ld_u8_16(&seq1p[ca]) >> 2, codepA = ld_u8_16(&seq1p[ca - 1]) >> 2;
            const int codeB = ld_u8_16(&seq1p[cb]) >> 2, codepB = ld_u8_16(&seq1p[cb - 1]) >> 2;
#if PK16_WIDE
            const int mkA = WORD16(codeA), mkpA = WORD16(codepA), mkB = WORD16(codeB), mkpB = WORD16(codepB);
#else
            const int mkA = ((codeA < nmc) ? (4 << codeA) : 0) | 2, mkpA = ((codepA < nmc) ? (4 << codepA) : 0) | 2;
            const int mkB = ((codeB < nmc) ? (4 << codeB) : 0) | 2, mkpB = ((codepB < nmc) ? (4 << codepB) : 0) | 2;
#endif
            lds->c1w[64 + lane] = mkA | (mkpA << 16);
            lds->c1w[128 + lane] = mkB | (mkpB << 16);
            lds->c1s[64 + lane] = (codeA & 3) | 0x0c000c00 | ((4 + (codepA & 3)) << 16);
            lds->c1s[128 + lane] = (codeB & 3) | 0x0c000c00 | ((4 + (codepB & 3)) << 16);
            simple1 = !__any(codeA >= 4 || codeA >= nmc);
            simple0 = !__any(codeB >= 4 || codeB >= nmc);
        }
        const int done0 = max(0, c * CHUNK - emit_v);
        if (lane == 0) st_agent2_16((int2*) &winp[2 * (s + 1)], make_int2(0, done0));
        my_gap_used = true;
        void_from = 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) st_agent16(prog_out, done0);
        set_prio_for(c);
    }
    // what a whole strip must be for its chunks to qualify (wave-uniform, fixed per strip): only the bus to write, nothing watching
    const bool hot_strip = (PK16_HOTLOOP != 0) && !emit_any && a->trace == nullptr && a->dbg == nullptr &&
                           special == nullptr && lastrow == nullptr && ckpt == nullptr;
    int resume_at = 0;
    const int hot_end = band_mode ? min(n, band_hi) : n;
#ifdef PK16_TRACE_BAND      // tools/trace_band_split.py: where a strip's lifetime goes in a pruned run (a build of its own, -DPK16_TRACE_BAND)
    long long tb_ff = 0, tb_bodyskip = 0, tb_comp = 0; int nb_bodyskip = 0;
#endif
    while (c < nchunks) {
        // band mode: everything this strip had to write lies behind it -- the rest of the row is skipped
        if (band_mode && c * CHUNK - emit_v >= band_hi) { retired = true; break; }
        if (hot_strip) {
            // per chunk: inputs already prefetched, past the graded-priority start, full width with a chunk to follow,
            // plain codes in the window and in the chunk that enters it, no exact-mode stretch, no stop poll due
            while (pf_valid && !exact_mode && c > 256 && (c + 1) * CHUNK <= hot_end && simple0 && simple1 &&
                   ((c & 63) != 63 || poll_host == 0) && nx_plain && !(prune_on && (last_skipped || state_void))) {
                resume_at = body(BoolC16<true>(), 0);
                if (resume_at == 4) { resume_at = 0; break; }      // untouched: the general body takes the whole chunk
                if (resume_at != 0) break;
                c++;
            }
            if (host_stop) break;
        }
#ifdef PK16_TRACE_BAND
        long long tb_a = 0, tb_b = 0;
        if (a->trace != nullptr) tb_a = __builtin_amdgcn_s_memrealtime();
#endif
        if (prune_on && last_skipped && resume_at == 0) {
            c += fast_forward();                           // (leaves at least the chunk it stopped at)
#ifdef PK16_TRACE_BAND
            if (a->trace != nullptr) tb_ff += __builtin_amdgcn_s_memrealtime() - tb_a;
#endif
            if (retired || host_stop) break;
        }
#ifdef PK16_TRACE_BAND
        if (a->trace != nullptr) tb_b = __builtin_amdgcn_s_memrealtime();
#endif
        const int rc = body(BoolC16<false>(), resume_at);
#ifdef PK16_TRACE_BAND
        if (a->trace != nullptr) {
            const long long tb_c = __builtin_amdgcn_s_memrealtime();
            if (prune_on && last_skipped) { tb_bodyskip += tb_c - tb_b; nb_bodyskip++; }
            else tb_comp += tb_c - tb_b;
        }
#endif
        resume_at = 0;
        if (rc == 3) break;
        c++;
    }

#ifdef PK16_TRACE_BAND
    if (a->trace != nullptr && lane == 0) {
        // [2]: ticks in fast-forward runs (low 32) | ticks in skipped chunks taken by the body (high 32)
        // [3]: ticks in computed chunks (low 32) | number of body-skipped chunks (high 32)
        a->trace[4 * s + 2] = (tb_ff & 0xffffffffll) | (tb_bodyskip << 32);
        a->trace[4 * s + 3] = (tb_comp & 0xffffffffll) | ((long long) nb_bodyskip << 32);
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (host_stop) flag_pending = n;                      // followers must not wait for columns that will never come
    else if (windowed) {
        // the last word of a strip with a window: done, and from this column on everything it left is the skip constant
        // (a strip that retired never wrote those cells; one that walked to the end wrote the same value)
        const int x = retired ? max(0, c * CHUNK - emit_v) : (void_from < n ? void_from : n);
        flag_pending = WIN_RETIRED + x;
    }
    if (flag_pending >= 0 && lane == 0) st_agent16(prog_out, flag_pending);
    if (pruned_slabs > 0 && lane == 0 && a->pruned_slabs != nullptr) atomicAdd(a->pruned_slabs, (unsigned long long) pruned_slabs);
    if (det && lane == 0) st_agent16(&a->det_news[s], det_found);
    __builtin_amdgcn_s_setprio(0);
#ifndef PK16_NO_FAULT
    if (__any(overflow != 0) || s == a->fault_strip) {
#else
    if (__any(overflow != 0)) {
#endif
        int why = overflow;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) why |= __shfl_xor(why, d);
        if (lane == 0) {
            // error_flag[1]: causes (OR over the strips that reported), error_flag[2]: 1 + the first strip that did
            atomicOr(a->error_flag + 1, why != 0 ? why : OVF16_INJECTED);
            atomicCAS(a->error_flag + 2, 0, s + 1);
            atomicExch(a->error_flag, 16);
            st_agent16(a->abort_flag, 1);
        }
    }
    if (a->trace != nullptr && lane == 0) {
        a->trace[4 * s + 0] = tr_start; a->trace[4 * s + 1] = __builtin_amdgcn_s_memrealtime();
    }
    DBG16(3, 40);
    // ---- strip epilogue ----
    if (a->last_col != nullptr) {
#pragma unroll
        for (int half = 0; half < 2; half++) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int g = (half ? lrow_hi : lrow_lo) + r;
                if (g < a->m) {
                    const int t16 = half ? hi16(as_i(st.TL[r])) : lo16(as_i(st.TL[r]));
                    const int e16 = half ? hi16(as_i(st.E[r])) : lo16(as_i(st.E[r]));
                    a->last_col[g + 1] = make_int2((prune_nw && t16 == -32768) ? NEG_INF : t16 + T_OFF + bias - 2 * r,
                                                   e16 == -32768 ? NEG_INF : e16 + bias - 2 * r);
                }
            }
        }
    }
    if (TRACK) {
        lds->red[lane] = st.best_t;
        lds->red[64 + lane] = (st.best_j >= 0) ? (lrow_lo + st.best_r) : 0x7fffffff;   // LO rows then HI rows are consecutive
        lds->red[128 + lane] = st.best_j;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            int bt = NEG_INF, bi = 0x7fffffff, bj = -1;
            for (int k = 0; k < 64; k++) {
                const int t = lds->red[k], i = lds->red[64 + k], j = lds->red[128 + k];
                if (j >= 0 && (t > bt || (t == bt && (i < bi || (i == bi && j < bj))))) { bt = t; bi = i; bj = j; }
            }
            int4 rec;
            rec.x = (bj >= 0) ? bt + T_OFF : NEG_INF;
            rec.y = bi; rec.z = bj; rec.w = 1;
            a->strip_best[s] = rec;
        }
        __builtin_amdgcn_wave_barrier();
    } else {
        // value-only record: the strip's best score; the exact canonical cell of the winning strip is
        // recomputed afterwards from the nearest checkpoint row by the exact-tracking kernel (runtime.cpp)
        lds->red[lane] = lane_max;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            int bt = NEG_INF;
            for (int k = 0; k < 64; k++) bt = max(bt, lds->red[k]);
            int4 rec;
            rec.x = (bt > NEG_INF) ? bt + T_OFF : NEG_INF;
            rec.y = -1; rec.z = -1; rec.w = 2;
            a->strip_best[s] = rec;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int R, bool TRACK, bool SWF, bool PRUNE, bool GOAL = false, bool EDGE = false>
__global__ void __launch_bounds__(64) sw_strip_kernel_pk16(const KernelArgs* __restrict__ ap) {
    __shared__ WaveLds16 lds_store;
    WaveLds16* lds = &lds_store;
    const int lane = threadIdx.x;
    const UniformArgs a = uniform_args(ap);
    const int num_strips = a->num_strips;
    // One wavefront per SIMD is the design point (DESIGN.md §4 "Scheduling"; measurements: docs/NOTEBOOK_r1-r3.md 4.1) and the strip chain runs at the speed of its
    // slowest member, so placement must not be left to the dispatcher: claiming the top accumulation
    // register makes the wavefront's register allocation exceed half of the SIMD's 512-entry file, and the
    // hardware then cannot co-schedule two of them on one SIMD.
    asm volatile("" ::: "a255");
    for (;;) {
        const int s = __builtin_amdgcn_readfirstlane(claim_strip_common(ap, lane, 128 * R));
        if (s >= num_strips) break;
        if (poll_agent16(a->abort_flag) != 0 || poll_agent16(a->stop_word) != 0 || (a->host_abort != nullptr && poll_sys16(a->host_abort) != 0)) {
            // Stopped (mustContinue() == 0, or an error): this wavefront is done.  Every strip still in flight holds an
            // earlier ticket, so nobody waits for this one; taking the strips that are left through the ORDERED
            // completion one by one cost a stage-2 partition of 5 M rows 10-40 ms after its goal had been found
            // (19 000 skipped strips at ~1.5 us each: tools/stage2_probe2.py).  The host learns the end from the launch.
            if (lane == 0) st_agent16(&a->progress[s + 1], a->n);
            __builtin_amdgcn_wave_barrier();
            break;
        } else {
            process_strip16<R, TRACK, SWF, PRUNE, GOAL, EDGE>(ap, s, lds, lane);
        }
        complete_strip_common(ap, s, lane, 128 * R, true);
    }
}

// Two strip heights in ONE launch.  The W wavefronts sweep a partition in ceil(strips / W) rounds and a partly filled last
// round costs a full one (C2: 1954 strips of 1536 rows on 1024 wavefronts = 1.9 rounds, 4.6 % of the chip idle in the
// second).  With the first `mix_first` strips RA half-rows tall and the rest RB = RA - 1, the strip count becomes a whole
// number of rounds (C2: 910 x 1536 + 1138 x 1408 rows = 2048 strips) and the second kind's shorter steps are the gain.
// Two launches could not do it: the second would wait for the first to end and pay the pipeline's ramp again.
template <int RA, int RB, bool TRACK, bool SWF>
__global__ void __launch_bounds__(64) sw_strip_kernel_pk16_mixed(const KernelArgs* __restrict__ ap) {
    __shared__ WaveLds16 lds_store;
    WaveLds16* lds = &lds_store;
    const int lane = threadIdx.x;
    const UniformArgs a = uniform_args(ap);
    const int num_strips = a->num_strips, mix_first = a->mix_first;
    asm volatile("" ::: "a255");                          // one wavefront per SIMD (see sw_strip_kernel_pk16)
    for (;;) {
        const int s = __builtin_amdgcn_readfirstlane(claim_strip_common(ap, lane, 128 * RA));   // (no outside column in this mode)
        if (s >= num_strips) break;
        if (poll_agent16(a->abort_flag) != 0 || poll_agent16(a->stop_word) != 0 || (a->host_abort != nullptr && poll_sys16(a->host_abort) != 0)) {
            if (lane == 0) st_agent16(&a->progress[s + 1], a->n);
            __builtin_amdgcn_wave_barrier();
            break;                                        // stopped: see sw_strip_kernel_pk16
        } else if (s < mix_first) {
            process_strip16<RA, TRACK, SWF, false>(ap, s, lds, lane);
        } else {
            process_strip16<RB, TRACK, SWF, false>(ap, s, lds, lane);
        }
        complete_strip_common(ap, s, lane, 128 * RA, true);
    }
}

// Several partitions in one launch (BatchArgs, sw_kernel.h): the same strip function, the argument block of the
// partition the ticket belongs to.  256- and 512-row strips only: the partitions that come in batches (stage 3's walks
// between two special rows) are tall, narrow and stopped early -- what they need is many of them in flight.
template <int R, bool TRACK, bool SWF, bool PRUNE = false, bool GOAL = false>
__global__ void __launch_bounds__(64) sw_batch_kernel_pk16(const BatchArgs* __restrict__ bp) {
    __shared__ WaveLds16 lds_store;
    WaveLds16* lds = &lds_store;
    const int lane = threadIdx.x;
    const unsigned long long bv = (unsigned long long) bp;
    const BatchArgs* b = (const BatchArgs*) (((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((unsigned) (bv >> 32)) << 32) |
                                             (unsigned) __builtin_amdgcn_readfirstlane((unsigned) bv));
    const int total = __builtin_amdgcn_readfirstlane(b->total);
    asm volatile("" ::: "a255");                          // one wavefront per SIMD (see sw_strip_kernel_pk16)
    for (;;) {
        int t = 0;
        if (lane == 0) t = atomicAdd(b->ticket, 1);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t >= total) break;
        const int2 ps = b->map[t];
        const int p = __builtin_amdgcn_readfirstlane(ps.x), s = __builtin_amdgcn_readfirstlane(ps.y);
        const unsigned long long av = (unsigned long long) b->args[p];
        const KernelArgs* ap = (const KernelArgs*) (((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((unsigned) (av >> 32)) << 32) |
                                                    (unsigned) __builtin_amdgcn_readfirstlane((unsigned) av));
        wait_first_column_common(ap, s, lane, 128 * R);
        const UniformArgs a = uniform_args(ap);
        if (poll_agent16(a->abort_flag) != 0 || poll_agent16(a->stop_word) != 0 || (a->host_abort != nullptr && poll_sys16(a->host_abort) != 0)) {
            if (lane == 0) st_agent16(&a->progress[s + 1], a->n);
            __builtin_amdgcn_wave_barrier();
        } else {
            process_strip16<R, TRACK, SWF, PRUNE, GOAL>(ap, s, lds, lane);
        }
        complete_strip_common(ap, s, lane, 128 * R, false);     // (every ticket of a batch goes through here in order)
    }
}

// One launcher per strip height and pruning mode; they are spread over six translation units
// (sw_kernel_pk16_{a..j}.hip define PK16_PART, sw_kernel_pk16_w{a..j}.hip PK16_WIDE as well) so that the instantiations
// compile in parallel.
template <int RV, bool PRUNE>
hipError_t launch16_r(const KernelArgs* dargs, int grid, hipStream_t stream, bool track, bool sw) {
#define LAUNCH16(TRV, SWV) hipLaunchKernelGGL((sw_strip_kernel_pk16<RV, TRV, SWV, PRUNE>), dim3(grid), dim3(64), 0, stream, dargs)
    if (sw) { if (track) LAUNCH16(true, true); else LAUNCH16(false, true); }
    else if constexpr (!PRUNE) { if (track) LAUNCH16(true, false); else LAUNCH16(false, false); }
    else if (!track) LAUNCH16(false, false);               // global alignment with pruning: the goal is the last cell, nothing to track
    else return hipErrorInvalidValue;
#undef LAUNCH16
    return hipGetLastError();
}

#define PK16_DECL(RV, PR, KW) KW template hipError_t launch16_r<RV, PR>(const KernelArgs*, int, hipStream_t, bool, bool);
#if PK16_PART == 0
PK16_DECL(2, false, ) PK16_DECL(4, false, ) PK16_DECL(6, false, ) PK16_DECL(8, false, )
PK16_DECL(12, false, extern) PK16_DECL(16, false, extern)
PK16_DECL(2, true, extern) PK16_DECL(4, true, extern) PK16_DECL(6, true, extern) PK16_DECL(8, true, extern)
PK16_DECL(12, true, extern) PK16_DECL(16, true, extern)

hipError_t launch_strip_kernel_pk16_goal(const KernelArgs* dargs, int rows_per_half, int grid, hipStream_t stream);   // (unit i)
hipError_t launch_strip_kernel_pk16_edge(const KernelArgs* dargs, int rows_per_half, int grid, hipStream_t stream);   // (unit j)
hipError_t launch_strip_kernel_pk16(const KernelArgs& a, KernelArgs* dargs, int rows_per_half, int grid, hipStream_t stream, bool track, bool sw) {
    hipError_t e = hipMemcpyAsync(dargs, &a, sizeof(KernelArgs), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    const bool pr = a.prune != 0;
    // goal mode (unit i): the heights a goal sweep runs at
    if (pr && (a.goal_bound_col > NEG_INF / 2 || a.goal_bound_row > NEG_INF / 2)) {
        if (track || sw) return hipErrorInvalidValue;
        return launch_strip_kernel_pk16_goal(dargs, rows_per_half, grid, stream);
    }
    // edge mode (unit j): the alignment ends on an edge of the super-partition, KernelArgs::prune_end says which
    if (pr && a.prune_end != 0) {
        if (track || sw) return hipErrorInvalidValue;
        return launch_strip_kernel_pk16_edge(dargs, rows_per_half, grid, stream);
    }
#define PK16_CASE(RV) case RV: return pr ? launch16_r<RV, true>(dargs, grid, stream, track, sw) : launch16_r<RV, false>(dargs, grid, stream, track, sw);
    switch (rows_per_half) {
    PK16_CASE(2) PK16_CASE(4) PK16_CASE(6) PK16_CASE(8) PK16_CASE(12) PK16_CASE(16)
    default: return hipErrorInvalidValue;
    }
#undef PK16_CASE
}

#define BATCH16(RV) do { \
        if (sw) { if (track) hipLaunchKernelGGL((sw_batch_kernel_pk16<RV, true, true>), dim3(grid), dim3(64), 0, stream, dbatch); \
                  else hipLaunchKernelGGL((sw_batch_kernel_pk16<RV, false, true>), dim3(grid), dim3(64), 0, stream, dbatch); } \
        else { if (track) hipLaunchKernelGGL((sw_batch_kernel_pk16<RV, true, false>), dim3(grid), dim3(64), 0, stream, dbatch); \
               else hipLaunchKernelGGL((sw_batch_kernel_pk16<RV, false, false>), dim3(grid), dim3(64), 0, stream, dbatch); } } while (0)
hipError_t launch_batch_kernel_pk16_r8(const BatchArgs* dbatch, int grid, hipStream_t stream, bool track, bool sw);   // (unit h)
hipError_t launch_batch_kernel_pk16(const BatchArgs* dbatch, int rows_per_half, int grid, hipStream_t stream, bool track, bool sw) {
    if (rows_per_half == 2) BATCH16(2);
    else if (rows_per_half == 4) BATCH16(4);
    else if (rows_per_half == 8) return launch_batch_kernel_pk16_r8(dbatch, grid, stream, track, sw);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
#undef BATCH16

// the seed's segments (runtime.cpp::anchored_seed): global-type partitions in band mode, value-only records, pruning kernels
hipError_t launch_batch_kernel_pk16_band(const BatchArgs* dbatch, int grid, hipStream_t stream) {
    hipLaunchKernelGGL((sw_batch_kernel_pk16<4, false, false, true>), dim3(grid), dim3(64), 0, stream, dbatch);
    return hipGetLastError();
}
#elif PK16_PART == 6
hipError_t launch_strip_kernel_pk16_mixed(const KernelArgs& a, KernelArgs* dargs, int rows_per_half_a, int rows_per_half_b, int grid,
                                          hipStream_t stream, bool track, bool sw) {
    if (rows_per_half_a != 12 || rows_per_half_b != 11 || !track) return hipErrorInvalidValue;     // the pair that is built
    hipError_t e = hipMemcpyAsync(dargs, &a, sizeof(KernelArgs), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if (sw) hipLaunchKernelGGL((sw_strip_kernel_pk16_mixed<12, 11, true, true>), dim3(grid), dim3(64), 0, stream, dargs);
    else hipLaunchKernelGGL((sw_strip_kernel_pk16_mixed<12, 11, true, false>), dim3(grid), dim3(64), 0, stream, dargs);
    return hipGetLastError();
}
#elif PK16_PART == 7
// 1024-row strips for batches of tall partitions (mi355sw_config.batch_rows_per_lane = 16: stage 2's sweeps from guessed crosspoints)
hipError_t launch_batch_kernel_pk16_r8(const BatchArgs* dbatch, int grid, hipStream_t stream, bool track, bool sw) {
    if (sw) { if (track) hipLaunchKernelGGL((sw_batch_kernel_pk16<8, true, true>), dim3(grid), dim3(64), 0, stream, dbatch);
              else hipLaunchKernelGGL((sw_batch_kernel_pk16<8, false, true>), dim3(grid), dim3(64), 0, stream, dbatch); }
    else { if (track) hipLaunchKernelGGL((sw_batch_kernel_pk16<8, true, false>), dim3(grid), dim3(64), 0, stream, dbatch);
           else hipLaunchKernelGGL((sw_batch_kernel_pk16<8, false, false>), dim3(grid), dim3(64), 0, stream, dbatch); }
    return hipGetLastError();
}
#elif PK16_PART == 8
// goal mode (process_strip16<.., GOAL>): what a goal sweep gets from AlignJob::begin -- 256- and 512-row strips -- and the batches
// of stage 2's sweeps from guessed crosspoints, 256- and 1024-row strips; global recurrence, nothing tracked, pruning kernels
hipError_t launch_strip_kernel_pk16_goal(const KernelArgs* dargs, int rows_per_half, int grid, hipStream_t stream) {
    if (rows_per_half == 2) hipLaunchKernelGGL((sw_strip_kernel_pk16<2, false, false, true, true>), dim3(grid), dim3(64), 0, stream, dargs);
    else if (rows_per_half == 4) hipLaunchKernelGGL((sw_strip_kernel_pk16<4, false, false, true, true>), dim3(grid), dim3(64), 0, stream, dargs);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_batch_kernel_pk16_goal(const BatchArgs* dbatch, int rows_per_half, int grid, hipStream_t stream) {
    if (rows_per_half == 2) hipLaunchKernelGGL((sw_batch_kernel_pk16<2, false, false, true, true>), dim3(grid), dim3(64), 0, stream, dbatch);
    else if (rows_per_half == 8) hipLaunchKernelGGL((sw_batch_kernel_pk16<8, false, false, true, true>), dim3(grid), dim3(64), 0, stream, dbatch);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
#elif PK16_PART == 9
// edge mode (process_strip16<.., EDGE>): 256-, 512-, 1024- and 2048-row strips; global recurrence, nothing tracked, pruning kernels
hipError_t launch_strip_kernel_pk16_edge(const KernelArgs* dargs, int rows_per_half, int grid, hipStream_t stream) {
#define EDGE16(RV) hipLaunchKernelGGL((sw_strip_kernel_pk16<RV, false, false, true, false, true>), dim3(grid), dim3(64), 0, stream, dargs)
    if (rows_per_half == 2) EDGE16(2);
    else if (rows_per_half == 4) EDGE16(4);
    else if (rows_per_half == 8) EDGE16(8);
    else if (rows_per_half == 16) EDGE16(16);
    else return hipErrorInvalidValue;
#undef EDGE16
    return hipGetLastError();
}
#elif PK16_PART == 1
PK16_DECL(12, false, )
#elif PK16_PART == 2
PK16_DECL(16, false, )
#elif PK16_PART == 3
PK16_DECL(2, true, ) PK16_DECL(4, true, ) PK16_DECL(6, true, ) PK16_DECL(8, true, )
#elif PK16_PART == 4
PK16_DECL(12, true, )
#elif PK16_PART == 5
PK16_DECL(16, true, )
#endif
#undef PK16_DECL

}  // namespace mi355sw
