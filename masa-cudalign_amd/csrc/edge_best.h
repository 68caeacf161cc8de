// The best cell of an edge, found where the edge lies (edge_best.hip): the maximum H of a run of (H, gap component) cells in
// device memory and the SMALLEST index that holds it -- what mi355sw_stream_edge_best reads off a stream's last row, and what
// mi355sw_stream_end holds an edge-pruned run's bound against, without the row ever leaving the GPU.
#pragma once
#include <hip/hip_runtime.h>

// One 64-bit word carries the result: (H + 2^31) in the upper half, 0xFFFFFFFF - index in the lower one, so that the larger
// word is the higher score and, among equal scores, the smaller index.  0 is "nothing yet" (no cell encodes to it: that would
// be H = INT32_MIN at index 0xFFFFFFFF, and a run has at most INT32_MAX cells).
#define EDGE_BEST_NONE 0ull
__host__ __device__ static inline unsigned long long edge_best_key(int h, unsigned index) {
    return ((unsigned long long) ((unsigned) h ^ 0x80000000u) << 32) | (unsigned long long) (0xFFFFFFFFu - index);
}
__host__ __device__ static inline int edge_best_score(unsigned long long key) { return (int) ((unsigned) (key >> 32) ^ 0x80000000u); }
__host__ __device__ static inline unsigned edge_best_index(unsigned long long key) { return 0xFFFFFFFFu - (unsigned) (key & 0xFFFFFFFFull); }

// *d_key (a device word the caller owns) = max(*d_key, key of the best of cells[0 .. len)), 1 <= len <= INT32_MAX.  The launch
// sets *d_key to EDGE_BEST_NONE first (same stream) when `reset`; several runs of cells may be folded into one word otherwise.
hipError_t launch_edge_best(const int2* cells, int len, unsigned long long* d_key, bool reset, hipStream_t stream);
