// The two picks the decode, its counts (graph_decode.hip) and the score histograms (calibration.hip) must agree on, stated once:
//   gd_pick   the arg-max predicate of an edge row held one value per lane by a 32-lane group, lowest index among equals
//   gd_top1   the arg-max class of a node row read by one wave, lowest index among equals, and its value
// Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlsat {

// lane k (< 32) of the group holds r = rel[e, k] (any value for k >= R); all 32 lanes call; every lane gets the row's pick
__device__ __forceinline__ int gd_pick(float r, int k, int R) {
    float bv = k < R ? r : -INFINITY;
    int bi = k;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 32);
        const int oi = __shfl_xor(bi, o, 32);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    return bi;
}

// the whole wave calls with its node's row (C >= 1 values); every lane gets the class, bv its value
__device__ __forceinline__ int gd_top1(const float* __restrict__ row, int C, int lane, float& bv) {
    bv = -INFINITY;
    int bi = INT32_MAX;                            // INT32_MAX: this lane holds no class
    for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        if (bi == INT32_MAX || v > bv) {
            bv = v;
            bi = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != INT32_MAX && (bi == INT32_MAX || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    return bi;
}

}  // namespace vlsat
