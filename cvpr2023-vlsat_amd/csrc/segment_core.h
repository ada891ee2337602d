// The arithmetic of the mesh segmenter (include/vlsat_segment.h), for the kernels of mesh_segment.hip and for the host
// (tests/segment_core_check.cpp): the edge weight, the packing of a choice into one 64-bit key, the number of absorb rounds and the
// layout of the scratch block, each stated once so that both sides cannot drift apart.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VLSAT_SEG_HD __host__ __device__ __forceinline__
#else
#define VLSAT_SEG_HD inline
#endif

namespace vlsat {

constexpr int64_t SEG_MAX_VERTS = (int64_t)1 << 24;
constexpr int64_t SEG_MAX_EDGES = ((int64_t)1 << 31) - 1;
constexpr int SEG_NUMBER_TILE = 1024;                     // vertices per block of the dense numbering (flag counts, then apply)
constexpr unsigned long long SEG_NO_KEY = ~0ull;          // never a key: a weight's bits are at most those of 2.0f

VLSAT_SEG_HD uint32_t seg_f32_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
#endif
}

// w = 1 - d clamped to [0, 2], d = fl(fl(fl(ax bx) + fl(ay by)) + fl(az bz)); a NaN d gives 2.  Every product and sum is rounded on
// its own (the device spells the operations out and the file is built with -ffp-contract=off; a host compiler must not contract
// either).  Products commute, so w(a, b) == w(b, a) bit for bit.  The result is never -0: 1 - d is +0 when d == 1.
VLSAT_SEG_HD float seg_weight(float ax, float ay, float az, float bx, float by, float bz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
    const float w = __fsub_rn(1.0f, d);
#else
    volatile float xx = ax * bx, yy = ay * by, zz = az * bz;          // (volatile: no contraction across the statements)
    volatile float s = xx + yy;
    const float d = s + zz;
    const float w = 1.0f - d;
#endif
    if (d != d) return 2.0f;
    return w < 0.0f ? 0.0f : (w > 2.0f ? 2.0f : w);
}

// (weight, target root) as one unsigned number: w >= 0, so the order of its bits is the order of its values, and the minimum key is
// the lowest weight and, on a tie, the lower root.
VLSAT_SEG_HD unsigned long long seg_key(float w, int32_t root) {
    return ((unsigned long long)seg_f32_bits(w) << 32) | (unsigned long long)(uint32_t)root;
}
VLSAT_SEG_HD int32_t seg_key_root(unsigned long long key) { return (int32_t)(uint32_t)(key & 0xffffffffull); }

// ceil(log2(min_verts)); 0 for min_verts <= 1.  After r rounds a component that is still small and still has a neighbour holds at
// least 2^r former components, so this many rounds reach the fixed point.
VLSAT_SEG_HD int seg_rounds(int64_t min_verts) {
    int r = 0;
    while (((int64_t)1 << r) < min_verts) ++r;
    return r;
}

VLSAT_SEG_HD bool seg_edge_ok(int64_t a, int64_t b, int64_t n_verts) { return a >= 0 && b >= 0 && a < n_verts && b < n_verts && a != b; }

VLSAT_SEG_HD bool seg_sizes_ok(int64_t n_verts, int64_t n_edges) {
    return n_verts >= 1 && n_verts <= SEG_MAX_VERTS && n_edges >= 0 && n_edges <= SEG_MAX_EDGES;
}

// scratch: key u64 [V] | parent i32 [V] | root i32 [V] | size i32 [V] | num i32 [V] | block_count i32 [T] | block_first i32 [T + 1],
// T = ceil(V / SEG_NUMBER_TILE); every part starts on a 16-byte boundary.  The edges need none: a weight is recomputed where it is used.
struct SegScratch {
    size_t key, parent, root, size, num, block_count, block_first, bytes;
    int64_t tiles;
};
VLSAT_SEG_HD size_t seg_align16(size_t n) { return (n + 15) & ~(size_t)15; }
VLSAT_SEG_HD SegScratch seg_scratch_layout(int64_t n_verts) {
    SegScratch s;
    const size_t v = (size_t)n_verts;
    s.tiles = (n_verts + SEG_NUMBER_TILE - 1) / SEG_NUMBER_TILE;
    size_t at = 0;
    s.key = at;          at += seg_align16(v * 8);
    s.parent = at;       at += seg_align16(v * 4);
    s.root = at;         at += seg_align16(v * 4);
    s.size = at;         at += seg_align16(v * 4);
    s.num = at;          at += seg_align16(v * 4);
    s.block_count = at;  at += seg_align16((size_t)s.tiles * 4);
    s.block_first = at;  at += seg_align16((size_t)(s.tiles + 1) * 4);
    s.bytes = at;
    return s;
}

}  // namespace vlsat
