// The arithmetic of the voxel-grid filter (include/vlsat_voxel.h), for the kernels of voxel.hip and for the host
// (tests/voxel_core_check.cpp): the cell of a point and its key, the quantised coordinate, the mean of a sum, the normal of three sums,
// the rounded colour mean and the scratch layout, each stated once so that both sides cannot drift apart.  The device side spells every
// rounded operation out (__fsub_rn, __fmul_rn, __dmul_rn, __ddiv_rn, __dsqrt_rn: IEEE, round to nearest even); the host side relies on
// -ffp-contract=off and on volatile temporaries, and a host compiler must not contract.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VLSAT_VOXEL_HD __host__ __device__ __forceinline__
#else
#define VLSAT_VOXEL_HD inline
#endif

namespace vlsat {

constexpr int64_t VOXEL_MAX_POINTS = (int64_t)1 << 24;
constexpr int32_t VOXEL_CELL_BIAS = 1 << 20;                  // a cell coordinate t has |t| < 2^20: t + 2^20 fits 21 bits
constexpr float VOXEL_CELL_LIMIT = 1048576.0f;                // 2^20
constexpr float VOXEL_COORD_LIMIT = 32768.0f;                 // |x| < 2^15, so |llrint(x 2^24)| < 2^39 and 2^24 of them fit int64
constexpr double VOXEL_POINT_SCALE = 16777216.0;              // 2^24
constexpr double VOXEL_NORMAL_SCALE = 1048576.0;              // 2^20
constexpr unsigned long long VOXEL_EMPTY = ~0ull;             // never a key: a key is below 2^63

// inv = fl(1 / voxel) in fp32, once, on the host; false when it is not finite and positive (voxel <= 0, NaN, +inf, or so small that
// the quotient overflows)
inline bool voxel_inverse(float voxel, float& inv) {
    if (!(voxel > 0.0f)) return false;
    volatile float q = 1.0f / voxel;
    inv = q;
    return inv > 0.0f && inv < INFINITY;
}

// t = floor(fl(fl(x - o) inv)) of one axis; false when |x| < 32768 or |t| < 2^20 fails (a NaN fails both)
VLSAT_VOXEL_HD bool voxel_axis(float x, float o, float inv, int32_t& t) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float f = floorf(__fmul_rn(__fsub_rn(x, o), inv));
#else
    volatile float d = x - o;
    volatile float p = d * inv;
    const float f = floorf(p);
#endif
    if (!(fabsf(x) < VOXEL_COORD_LIMIT) || !(fabsf(f) < VOXEL_CELL_LIMIT)) return false;
    t = (int32_t)f;
    return true;
}

VLSAT_VOXEL_HD unsigned long long voxel_pack(int32_t tx, int32_t ty, int32_t tz) {
    return ((unsigned long long)(uint32_t)(tz + VOXEL_CELL_BIAS) << 42) | ((unsigned long long)(uint32_t)(ty + VOXEL_CELL_BIAS) << 21) |
           (unsigned long long)(uint32_t)(tx + VOXEL_CELL_BIAS);
}

// the key of a point, or VOXEL_EMPTY for a point out of range
VLSAT_VOXEL_HD unsigned long long voxel_key(float x, float y, float z, float ox, float oy, float oz, float inv) {
    int32_t tx = 0, ty = 0, tz = 0;
    const bool okx = voxel_axis(x, ox, inv, tx), oky = voxel_axis(y, oy, inv, ty), okz = voxel_axis(z, oz, inv, tz);
    return okx && oky && okz ? voxel_pack(tx, ty, tz) : VOXEL_EMPTY;
}

// q = llrint((double)x scale), half to even; the product is exact (scale is a power of two).  A position has |x| < 32768.
VLSAT_VOXEL_HD long long voxel_quantise(float x, double scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(__dmul_rn((double)x, scale));
#else
    return llrint((double)x * scale);
#endif
}
// a normal's component: one that is not finite or has |n| >= 32768 adds 0
VLSAT_VOXEL_HD long long voxel_quantise_normal(float n) {
    return fabsf(n) < VOXEL_COORD_LIMIT ? voxel_quantise(n, VOXEL_NORMAL_SCALE) : 0ll;
}

// (float)((double)S / (double)count 2^-24)
VLSAT_VOXEL_HD float voxel_mean(long long sum, int32_t count) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2float_rn(__dmul_rn(__ddiv_rn(__ll2double_rn(sum), (double)count), 1.0 / VOXEL_POINT_SCALE));
#else
    volatile double q = (double)sum / (double)count;
    volatile double m = q * (1.0 / VOXEL_POINT_SCALE);
    return (float)m;
#endif
}

// the three sums as fp64, l = sqrt((x x + y y) + z z), (x / l, y / l, z / l) as f32, or zeros when l == 0
VLSAT_VOXEL_HD void voxel_normal(long long sx, long long sy, long long sz, float& nx, float& ny, float& nz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double x = __ll2double_rn(sx), y = __ll2double_rn(sy), z = __ll2double_rn(sz);
    const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
    const bool some = l != 0.0;
    nx = some ? __double2float_rn(__ddiv_rn(x, l)) : 0.0f;
    ny = some ? __double2float_rn(__ddiv_rn(y, l)) : 0.0f;
    nz = some ? __double2float_rn(__ddiv_rn(z, l)) : 0.0f;
#else
    const double x = (double)sx, y = (double)sy, z = (double)sz;
    volatile double xx = x * x, yy = y * y, zz = z * z;
    volatile double s = xx + yy;
    volatile double t = s + zz;
    volatile double l = sqrt(t);
    if (l == 0.0) {
        nx = ny = nz = 0.0f;
        return;
    }
    volatile double qx = x / l, qy = y / l, qz = z / l;
    nx = (float)qx;
    ny = (float)qy;
    nz = (float)qz;
#endif
}

// (2 sum + count) / (2 count) in integers: the mean of a channel rounded half up; sum <= 255 count, so the result is <= 255
VLSAT_VOXEL_HD uint8_t voxel_color(uint32_t sum, int32_t count) {
    const unsigned long long c = (unsigned long long)count;
    return (uint8_t)((2ull * sum + c) / (2ull * c));
}

VLSAT_VOXEL_HD bool voxel_sizes_ok(int64_t n_points) { return n_points >= 1 && n_points <= VOXEL_MAX_POINTS; }

// the table: the least power of two >= 2 V slots (so at most half of them are ever taken), and log2 of it
inline int voxel_log2_slots(int64_t n_points) {
    int b = 1;
    while (((int64_t)1 << b) < 2 * n_points) ++b;
    return b;
}
// where a key's probe starts: the top bits of a multiplicative hash
VLSAT_VOXEL_HD uint32_t voxel_hash(unsigned long long key, int log2_slots) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots));
}

// ---- the scratch block of vlsat_voxel_assign / vlsat_voxel_reduce: byte offsets, every part 256-byte aligned ------------------------------
constexpr int VOXEL_THREADS = 256;
struct VoxelLayout {
    size_t table;          // 16 bytes per slot: key u64, first i32, count i32
    size_t slot_of_point;  // i32 [V]
    size_t head_number;    // i32 [V]: the number of the voxel a head point opens
    size_t block_heads;    // i32 [blocks + 1]: heads per block of VOXEL_THREADS points, then their exclusive scan
    size_t point_sum;      // i64 [V,3] (the first M rows are used)
    size_t normal_sum;     // i64 [V,3]
    size_t color_sum;      // u32 [V,3]
    size_t bytes;
};
inline size_t voxel_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline VoxelLayout voxel_layout(int64_t n_points) {
    const size_t v = (size_t)n_points, blocks = (v + VOXEL_THREADS - 1) / VOXEL_THREADS;
    VoxelLayout l;
    l.table = 0;
    l.slot_of_point = voxel_align(l.table + ((size_t)16 << voxel_log2_slots(n_points)));
    l.head_number = voxel_align(l.slot_of_point + 4 * v);
    l.block_heads = voxel_align(l.head_number + 4 * v);
    l.point_sum = voxel_align(l.block_heads + 4 * (blocks + 1));
    l.normal_sum = voxel_align(l.point_sum + 24 * v);
    l.color_sum = voxel_align(l.normal_sum + 24 * v);
    l.bytes = voxel_align(l.color_sum + 12 * v);
    return l;
}

}  // namespace vlsat
