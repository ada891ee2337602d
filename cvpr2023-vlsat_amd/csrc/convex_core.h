// The arithmetic of the convexity clusters (include/vlsat_convex.h), for the kernels of convex.hip and for the host
// (tests/convex_core_check.cpp): which points are eligible and oriented, the convexity value c of a table entry, the test that makes
// it concave, the limits and the scratch layout, each stated once so that both sides cannot drift apart.  The rounded operations are
// plane_core.h's (device: __fmul_rn, __fadd_rn, __fsub_rn; host: -ffp-contract=off and volatile temporaries).
#pragma once
#include "plane_core.h"

namespace vlsat {

constexpr int CONVEX_MAX_ROUNDS = 64;
// state of a point (rule 7)
enum { CONVEX_OUT = 0, CONVEX_CORE = 1, CONVEX_BOUNDARY = 2, CONVEX_NO_NORMAL = 3, CONVEX_DISSOLVED = 4 };

#if defined(__HIP_DEVICE_COMPILE__)
VLSAT_PLANE_HD float convex_fsub(float a, float b) { return __fsub_rn(a, b); }
#else
VLSAT_PLANE_HD float convex_fsub(float a, float b) { volatile float r = a - b; return r; }
#endif

// rule 1: the normal of an eligible point is usable when it is finite and not (0, 0, 0); -0 is 0
VLSAT_PLANE_HD bool convex_normal_usable(float nx, float ny, float nz) {
    return plane_point_valid(nx, ny, nz) && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
}

// fl(fl(fl(nx dx) + fl(ny dy)) + fl(nz dz))
VLSAT_PLANE_HD float convex_dot(const float* n, float dx, float dy, float dz) {
    return plane_fadd(plane_fadd(plane_fmul(n[0], dx), plane_fmul(n[1], dy)), plane_fmul(n[2], dz));
}

// rule 2: c = fl(n_i . d - n_j . d) for d = x_j - x_i.  Seen from j every difference, product and sum changes its sign and nothing
// else (rounding to nearest is symmetric), a and b change places, and fl(-b - -a) = fl(a - b): the same bit pattern from either end.
// The one exception changes nothing: a sum of opposite terms is +0 from both ends, so a c that is zero may be +0 here and -0 there.
VLSAT_PLANE_HD float convex_c(const float* xi, const float* ni, const float* xj, const float* nj) {
    const float dx = convex_fsub(xj[0], xi[0]), dy = convex_fsub(xj[1], xi[1]), dz = convex_fsub(xj[2], xi[2]);
    return convex_fsub(convex_dot(ni, dx, dy, dz), convex_dot(nj, dx, dy, dz));
}

// whether the distance of an entry lets it count as evidence: finite and >= 0
VLSAT_PLANE_HD bool convex_sqdist_ok(float q) { return q >= 0.0f && q < INFINITY; }

// concave: c > 0 and fl(c c) > fl(fl(tau tau) q); a NaN fails a comparison and is not concave
VLSAT_PLANE_HD bool convex_concave(float c, float tau, float q) { return c > 0.0f && plane_fmul(c, c) > plane_fmul(plane_fmul(tau, tau), q); }

inline bool convex_sizes_ok(int64_t n_points, int32_t k) { return cluster_sizes_ok(n_points, k); }

// ---- the scratch block: byte offsets, every part 256-byte aligned -----------------------------------------------------------------
struct ConvexLayout {
    size_t parent;       // i32 [V]
    size_t root;         // i32 [V]: the root of a core point, -1 for everybody else
    size_t size;         // i32 [V]: core points per root
    size_t boundary;     // i32 [V]
    size_t label_a;      // i32 [V]: the label (a root, or -1) after the odd absorption rounds
    size_t label_b;      // i32 [V]: after the even ones
    size_t num;          // i32 [V]
    size_t block_kept;   // i32 [blocks + 1]
    size_t bytes;
};
inline ConvexLayout convex_layout(int64_t n_points) {
    const size_t v = (size_t)n_points;
    ConvexLayout l;
    l.parent = 0;
    l.root = plane_align(l.parent + 4 * v);
    l.size = plane_align(l.root + 4 * v);
    l.boundary = plane_align(l.size + 4 * v);
    l.label_a = plane_align(l.boundary + 4 * v);
    l.label_b = plane_align(l.label_a + 4 * v);
    l.num = plane_align(l.label_b + 4 * v);
    l.block_kept = plane_align(l.num + 4 * v);
    l.bytes = plane_align(l.block_kept + 4 * (plane_blocks(n_points) + 1));
    return l;
}

}  // namespace vlsat
