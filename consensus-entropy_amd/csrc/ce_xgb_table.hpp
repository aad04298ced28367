// ce_xgb_table.hpp -- the XGB member's two plain (non-template) kernels: the
// lane-table builder and the expf check.  Included by ce_xgb.hip alone, so that
// other objects can include ce_xgb_walk.hpp without defining them again.
#pragma once
#include "ce_xgb_walk.hpp"

namespace ce {

// ce_xgb_lane_table: one wave per tree, lane j writes heap entry j
__global__ __launch_bounds__(256) void k_xgb_lane_table(const uint2* __restrict__ nodes, const float* __restrict__ leaves,
                                                        int T, int depth, int D, uint2* __restrict__ table) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = threadIdx.x & 63, NI = (1 << depth) - 1;
    if (t >= T) return;
    uint2 e = make_uint2(0u, 0u);
    uint32_t dl = 0u;
    if (j >= 1 && j <= NI) {
        const uint2 nd = nodes[t * NI + (j - 1)];
        const uint32_t ft = min(nd.x & 0x7fffffffu, (uint32_t)(D - 1));
        e = make_uint2(xs_fbase(ft), nd.y);
        dl = nd.x & 0x80000000u;
    } else if (j >= NI + 1 && j <= 2 * NI + 1) {
        e = make_uint2(0u, __float_as_uint(leaves[t * (NI + 1) + (j - NI - 1)]));
    }
    table[t * 64 + j] = make_uint2(e.x | dl, e.y);  // half 0: with default_left
    table[((int64_t)T + t) * 64 + j] = e;           // half 1: without
}

__global__ void k_expf(const float* __restrict__ x, int64_t n, float* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        y[i] = glibc_expf(x[i]);
}

}  // namespace ce
