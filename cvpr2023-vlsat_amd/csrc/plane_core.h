// The arithmetic of the structural-plane search (include/vlsat_objects.h), for the kernels of objects.hip and for the host
// (tests/plane_core_check.cpp): the draw of a rank, the plane through three points, the score of a point and its class, the eligibility
// of a hypothesis, its key and the scratch layouts, each stated once so that both sides cannot drift apart.  The device side spells every
// rounded operation out (__dsub_rn, __dmul_rn, __ddiv_rn, __dsqrt_rn, __fmul_rn, __fadd_rn: IEEE, round to nearest even); the host side
// relies on -ffp-contract=off and on volatile temporaries, and a host compiler must not contract.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VLSAT_PLANE_HD __host__ __device__ __forceinline__
#else
#define VLSAT_PLANE_HD inline
#endif

namespace vlsat {

constexpr int64_t PLANE_MAX_POINTS = (int64_t)1 << 24;
constexpr int PLANE_MAX_HYP = 4096;
constexpr int PLANE_MAX_PLANES = 32;
constexpr int PLANE_MIN_INLIERS = 3;
constexpr int PLANE_MAX_PPM = 500000;
constexpr int CLUSTER_MAX_K = 32;

// draw(k, n): splitmix64 of (seed, k), the top 32 bits scaled to n -- the generator of vlsat_sample_objects and vlsat_split_seeds
VLSAT_PLANE_HD uint32_t plane_draw(unsigned long long seed, unsigned long long k, uint32_t n) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (k + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(((z >> 32) * (unsigned long long)n) >> 32);
}

// ---- fp64 and fp32, one rounding per operation ----------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
VLSAT_PLANE_HD double plane_add(double a, double b) { return __dadd_rn(a, b); }
VLSAT_PLANE_HD double plane_sub(double a, double b) { return __dsub_rn(a, b); }
VLSAT_PLANE_HD double plane_mul(double a, double b) { return __dmul_rn(a, b); }
VLSAT_PLANE_HD double plane_div(double a, double b) { return __ddiv_rn(a, b); }
VLSAT_PLANE_HD double plane_sqrt(double a) { return __dsqrt_rn(a); }
VLSAT_PLANE_HD float plane_fadd(float a, float b) { return __fadd_rn(a, b); }
VLSAT_PLANE_HD float plane_fmul(float a, float b) { return __fmul_rn(a, b); }
#else
VLSAT_PLANE_HD double plane_add(double a, double b) { volatile double r = a + b; return r; }
VLSAT_PLANE_HD double plane_sub(double a, double b) { volatile double r = a - b; return r; }
VLSAT_PLANE_HD double plane_mul(double a, double b) { volatile double r = a * b; return r; }
VLSAT_PLANE_HD double plane_div(double a, double b) { volatile double r = a / b; return r; }
VLSAT_PLANE_HD double plane_sqrt(double a) { volatile double r = sqrt(a); return r; }
VLSAT_PLANE_HD float plane_fadd(float a, float b) { volatile float r = a + b; return r; }
VLSAT_PLANE_HD float plane_fmul(float a, float b) { volatile float r = a * b; return r; }
#endif

VLSAT_PLANE_HD bool plane_point_valid(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;       // (a NaN fails the comparison)
}

// ---- the plane through a, b, c (rule 3) -----------------------------------------------------------------------------------------
// m = (b - a) x (c - a) in fp64, l2 = fl(fl(mx mx + my my) + mz mz); void unless l2 > 0 and finite; n = m / sqrt(l2); the component of
// largest magnitude made positive (ties to the lower axis); d = -fl(fl(nx ax + ny ay) + nz az); all four rounded to fp32.
struct Plane {
    float nx, ny, nz, d;
};
VLSAT_PLANE_HD bool plane_from_points(const float* a, const float* b, const float* c, Plane& out) {
    const double ax = (double)a[0], ay = (double)a[1], az = (double)a[2];
    const double ux = plane_sub((double)b[0], ax), uy = plane_sub((double)b[1], ay), uz = plane_sub((double)b[2], az);
    const double vx = plane_sub((double)c[0], ax), vy = plane_sub((double)c[1], ay), vz = plane_sub((double)c[2], az);
    const double mx = plane_sub(plane_mul(uy, vz), plane_mul(uz, vy));
    const double my = plane_sub(plane_mul(uz, vx), plane_mul(ux, vz));
    const double mz = plane_sub(plane_mul(ux, vy), plane_mul(uy, vx));
    const double l2 = plane_add(plane_add(plane_mul(mx, mx), plane_mul(my, my)), plane_mul(mz, mz));
    out.nx = out.ny = out.nz = out.d = 0.0f;
    if (!(l2 > 0.0 && l2 < (double)INFINITY)) return false;
    const double l = plane_sqrt(l2);
    double nx = plane_div(mx, l), ny = plane_div(my, l), nz = plane_div(mz, l);
    double big = nx;
    if (fabs(ny) > fabs(big)) big = ny;
    if (fabs(nz) > fabs(big)) big = nz;
    if (big < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double d = -plane_add(plane_add(plane_mul(nx, ax), plane_mul(ny, ay)), plane_mul(nz, az));
    out.nx = (float)nx;
    out.ny = (float)ny;
    out.nz = (float)nz;
    out.d = (float)d;
    return true;
}

// ---- the score of a point (rule 4) ----------------------------------------------------------------------------------------------
// s = fl(fl(fl(fl(nx x) + fl(ny y)) + fl(nz z)) + d) in fp32
VLSAT_PLANE_HD float plane_score(float nx, float ny, float nz, float d, float x, float y, float z) {
    return plane_fadd(plane_fadd(plane_fadd(plane_fmul(nx, x), plane_fmul(ny, y)), plane_fmul(nz, z)), d);
}
VLSAT_PLANE_HD bool plane_inlier(float s, float dist) { return fabsf(s) <= dist; }       // a NaN is neither: it counts as below
VLSAT_PLANE_HD bool plane_above(float s, float dist) { return s > dist; }

// ---- eligibility and the key (rules 5 and 6) ------------------------------------------------------------------------------------
VLSAT_PLANE_HD int32_t plane_outside_limit(int32_t n, int32_t outside_ppm) { return (int32_t)(((int64_t)n * outside_ppm) / 1000000); }
VLSAT_PLANE_HD bool plane_eligible(int32_t inliers, int32_t above, int32_t n, int32_t min_inliers, int32_t outside_ppm) {
    const int32_t below = n - inliers - above;
    return inliers >= min_inliers && (above < below ? above : below) <= plane_outside_limit(n, outside_ppm);
}
// most inliers win, ties go to the lower h; never 0 for an eligible hypothesis (inliers >= 3)
VLSAT_PLANE_HD unsigned long long plane_key(int32_t inliers, int32_t h) {
    return ((unsigned long long)(uint32_t)inliers << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)h);
}
VLSAT_PLANE_HD int32_t plane_key_hypothesis(unsigned long long key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xffffffffull)); }

// ---- limits ---------------------------------------------------------------------------------------------------------------------
inline bool plane_sizes_ok(int64_t n_points, int32_t n_hyp, int32_t max_planes) {
    return n_points >= 3 && n_points <= PLANE_MAX_POINTS && n_hyp >= 1 && n_hyp <= PLANE_MAX_HYP && max_planes >= 1 && max_planes <= PLANE_MAX_PLANES;
}
inline bool cluster_sizes_ok(int64_t n_points, int32_t k) { return n_points >= 1 && n_points <= PLANE_MAX_POINTS && k >= 1 && k <= CLUSTER_MAX_K; }

// ---- the scratch blocks: byte offsets, every part 256-byte aligned ---------------------------------------------------------------
constexpr int PLANE_THREADS = 256;
inline size_t plane_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t plane_blocks(int64_t n_points) { return ((size_t)n_points + PLANE_THREADS - 1) / PLANE_THREADS; }

struct PlaneLayout {
    size_t state;        // i32 [8]: done, n, winner, the winner's plane as four fp32 bit patterns
    size_t best;         // u64 [1]
    size_t hyp;          // f32 [H,4]
    size_t hyp_ok;       // i32 [H]
    size_t counts;       // i32 [H,2]: inliers, above
    size_t alive;        // i32 [V]
    size_t alive_list;   // i32 [V]
    size_t block_alive;  // i32 [blocks + 1]: alive points per block of PLANE_THREADS points, then their exclusive scan
    size_t bytes;
};
inline PlaneLayout plane_layout(int64_t n_points, int32_t n_hyp) {
    const size_t v = (size_t)n_points, h = (size_t)n_hyp;
    PlaneLayout l;
    l.state = 0;
    l.best = plane_align(l.state + 4 * 8);
    l.hyp = plane_align(l.best + 8);
    l.hyp_ok = plane_align(l.hyp + 16 * h);
    l.counts = plane_align(l.hyp_ok + 4 * h);
    l.alive = plane_align(l.counts + 8 * h);
    l.alive_list = plane_align(l.alive + 4 * v);
    l.block_alive = plane_align(l.alive_list + 4 * v);
    l.bytes = plane_align(l.block_alive + 4 * (plane_blocks(n_points) + 1));
    return l;
}

struct ClusterLayout {
    size_t parent;       // i32 [V]
    size_t root;         // i32 [V]
    size_t size;         // i32 [V]
    size_t num;          // i32 [V]
    size_t block_kept;   // i32 [blocks + 1]
    size_t bytes;
};
inline ClusterLayout cluster_layout(int64_t n_points) {
    const size_t v = (size_t)n_points;
    ClusterLayout l;
    l.parent = 0;
    l.root = plane_align(l.parent + 4 * v);
    l.size = plane_align(l.root + 4 * v);
    l.num = plane_align(l.size + 4 * v);
    l.block_kept = plane_align(l.num + 4 * v);
    l.bytes = plane_align(l.block_kept + 4 * (plane_blocks(n_points) + 1));
    return l;
}

}  // namespace vlsat
