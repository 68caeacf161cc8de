// The best cell of an edge (edge_best.h): one launch, grid-stride over the cells, a 64-lane reduction per wavefront, and one
// 64-bit atomicMax per wavefront on a word that orders (score, -index) -- no LDS, no second pass, nothing merged on the host.
// A translation unit of its own: the strip kernels' units are assembled from the same text whether this file changes or not.
#include "edge_best.h"

#define EDGE_BEST_BLOCK 256
#define EDGE_BEST_MAX_BLOCKS 2048      // 8 wavefronts per CU on 256 CUs: enough loads in flight to stream a row at HBM speed

__global__ void __launch_bounds__(EDGE_BEST_BLOCK) edge_best_kernel(const int2* __restrict__ cells, const int len, unsigned long long* __restrict__ d_key) {
    const long long stride = (long long) gridDim.x * EDGE_BEST_BLOCK;
    unsigned long long best = EDGE_BEST_NONE;
    // (64-bit index arithmetic: len may be INT32_MAX, and index + stride must not wrap)
    for (long long k = (long long) blockIdx.x * EDGE_BEST_BLOCK + threadIdx.x; k < (long long) len; k += stride) {
        const unsigned long long key = edge_best_key(cells[k].x, (unsigned) k);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long other = __shfl_xor(best, d);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0 && best != EDGE_BEST_NONE) atomicMax(d_key, best);
}

hipError_t launch_edge_best(const int2* cells, int len, unsigned long long* d_key, bool reset, hipStream_t stream) {
    if (cells == nullptr || d_key == nullptr || len < 1) return hipErrorInvalidValue;
    if (reset) {
        const hipError_t e = hipMemsetAsync(d_key, 0, sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    long long blocks = ((long long) len + EDGE_BEST_BLOCK - 1) / EDGE_BEST_BLOCK;
    if (blocks > EDGE_BEST_MAX_BLOCKS) blocks = EDGE_BEST_MAX_BLOCKS;
    hipLaunchKernelGGL(edge_best_kernel, dim3((unsigned) blocks), dim3(EDGE_BEST_BLOCK), 0, stream, cells, len, d_key);
    return hipGetLastError();
}
