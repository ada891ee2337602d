// The arithmetic of the point-cloud front end (include/vlsat_cloud.h), for the kernels of cloud.hip and mesh_segment.hip and for the
// host (tests/cloud_core_check.cpp): the squared distance and its key, the covariance fold, the Jacobi step, the choice of the normal
// and of its sign, the whole rule for one point and the unsigned edge weight, each stated once so that both sides cannot drift apart.
// (The neighbour search needs no scratch of its own: its block is the grid's, nn_grid_scratch_bytes in label_transfer.hip.)  The device
// side spells every rounded operation out (__dadd_rn, __dmul_rn, __ddiv_rn, __dsqrt_rn: IEEE, round to nearest even); the host side
// relies on -ffp-contract=off and on volatile temporaries, and a host compiler must not contract.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VLSAT_CLOUD_HD __host__ __device__ __forceinline__
#else
#define VLSAT_CLOUD_HD inline
#endif

namespace vlsat {

constexpr int64_t CLOUD_MAX_POINTS = (int64_t)1 << 24;
constexpr int CLOUD_MAX_K = 32;
constexpr int CLOUD_MIN_POINTS = 3;                       // the least number of members a normal is estimated from
constexpr int CLOUD_SWEEPS = 6;                           // cyclic Jacobi sweeps (include/vlsat_cloud.h says why six)
constexpr unsigned long long CLOUD_NO_KEY = ~0ull;        // never a key: a finite d2 has bits below those of +inf

VLSAT_CLOUD_HD uint32_t cloud_f32_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
#endif
}
VLSAT_CLOUD_HD float cloud_bits_f32(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    memcpy(&x, &u, 4);
    return x;
#endif
}

// ---- fp64, one rounding per operation -------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
VLSAT_CLOUD_HD double cloud_add(double a, double b) { return __dadd_rn(a, b); }
VLSAT_CLOUD_HD double cloud_sub(double a, double b) { return __dsub_rn(a, b); }
VLSAT_CLOUD_HD double cloud_mul(double a, double b) { return __dmul_rn(a, b); }
VLSAT_CLOUD_HD double cloud_div(double a, double b) { return __ddiv_rn(a, b); }
VLSAT_CLOUD_HD double cloud_sqrt(double a) { return __dsqrt_rn(a); }
#else
VLSAT_CLOUD_HD double cloud_add(double a, double b) { volatile double r = a + b; return r; }
VLSAT_CLOUD_HD double cloud_sub(double a, double b) { volatile double r = a - b; return r; }
VLSAT_CLOUD_HD double cloud_mul(double a, double b) { volatile double r = a * b; return r; }
VLSAT_CLOUD_HD double cloud_div(double a, double b) { volatile double r = a / b; return r; }
VLSAT_CLOUD_HD double cloud_sqrt(double a) { volatile double r = sqrt(a); return r; }
#endif

// ---- neighbours -----------------------------------------------------------------------------------------------------------------
// d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) in fp32, the d2 of nearest_points.
VLSAT_CLOUD_HD float cloud_d2(float ax, float ay, float az, float bx, float by, float bz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
#else
    volatile float dx = ax - bx, dy = ay - by, dz = az - bz;
    volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    volatile float s = xx + yy;
    return s + zz;
#endif
}
// (d2, index) as one unsigned number: d2 >= 0 (never -0: a sum of squares), so the order of its bits is the order of its values.
VLSAT_CLOUD_HD unsigned long long cloud_key(float d2, int32_t j) {
    return ((unsigned long long)cloud_f32_bits(d2) << 32) | (unsigned long long)(uint32_t)j;
}
VLSAT_CLOUD_HD int32_t cloud_key_index(unsigned long long key) { return (int32_t)(uint32_t)(key & 0xffffffffull); }
VLSAT_CLOUD_HD float cloud_key_d2(unsigned long long key) { return cloud_bits_f32((uint32_t)(key >> 32)); }

// One step of the sorted insertion the kNN kernel unrolls: after it lo <= hi.
VLSAT_CLOUD_HD void cloud_order(unsigned long long& lo, unsigned long long& hi) {
    const unsigned long long a = lo, b = hi;
    lo = a < b ? a : b;
    hi = a < b ? b : a;
}
// key into the ascending list best[0 .. CAP): the guard keeps the chain off the common path.  Compile-time indices only.
template <int CAP>
VLSAT_CLOUD_HD void cloud_insert(unsigned long long (&best)[CAP], unsigned long long key) {
    if (!(key < best[CAP - 1])) return;
    best[CAP - 1] = key;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = CAP - 1; k > 0; --k) cloud_order(best[k - 1], best[k]);
}

// ---- normal and flatness ---------------------------------------------------------------------------------------------------------
// The symmetric matrix a and the accumulated rotations v (columns = eigenvectors), named entries so that no index is ever a variable.
struct CloudEig {
    double a00, a11, a22, a01, a02, a12;
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
};

// one member's contribution: the differences to the centroid, their six products added to the running sums
VLSAT_CLOUD_HD void cloud_cov_add(CloudEig& e, double px, double py, double pz, double cx, double cy, double cz) {
    const double dx = cloud_sub(px, cx), dy = cloud_sub(py, cy), dz = cloud_sub(pz, cz);
    e.a00 = cloud_add(e.a00, cloud_mul(dx, dx));
    e.a01 = cloud_add(e.a01, cloud_mul(dx, dy));
    e.a02 = cloud_add(e.a02, cloud_mul(dx, dz));
    e.a11 = cloud_add(e.a11, cloud_mul(dy, dy));
    e.a12 = cloud_add(e.a12, cloud_mul(dy, dz));
    e.a22 = cloud_add(e.a22, cloud_mul(dz, dz));
}
VLSAT_CLOUD_HD double cloud_trace(const CloudEig& e) { return cloud_add(cloud_add(e.a00, e.a11), e.a22); }

// The rotation in the plane (p, q), r the third index.  An off-diagonal entry of exactly 0 is skipped.  theta = (aqq - app) / (2 apq),
// t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with sgn(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c; then
//   app -= t apq, aqq += t apq, apq = 0, (arp, arq) = (c arp - s arq, s arp + c arq), and for every row k of v
//   (vkp, vkq) = (c vkp - s vkq, s vkp + c vkq).   A theta^2 that overflows gives t = 0: the identity, and apq = 0.
VLSAT_CLOUD_HD void cloud_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                                 double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = cloud_div(cloud_sub(aqq, app), cloud_mul(2.0, apq));
    const double den = cloud_add(fabs(theta), cloud_sqrt(cloud_add(cloud_mul(theta, theta), 1.0)));
    const double t = cloud_div(theta < 0.0 ? -1.0 : 1.0, den);        // (-0 counts as 0: +1)
    const double c = cloud_div(1.0, cloud_sqrt(cloud_add(cloud_mul(t, t), 1.0)));
    const double s = cloud_mul(t, c);
    const double tap = cloud_mul(t, apq);
    app = cloud_sub(app, tap);
    aqq = cloud_add(aqq, tap);
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = cloud_sub(cloud_mul(c, rp), cloud_mul(s, rq));
    arq = cloud_add(cloud_mul(s, rp), cloud_mul(c, rq));
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = cloud_sub(cloud_mul(c, a0), cloud_mul(s, b0));
    v0q = cloud_add(cloud_mul(s, a0), cloud_mul(c, b0));
    v1p = cloud_sub(cloud_mul(c, a1), cloud_mul(s, b1));
    v1q = cloud_add(cloud_mul(s, a1), cloud_mul(c, b1));
    v2p = cloud_sub(cloud_mul(c, a2), cloud_mul(s, b2));
    v2q = cloud_add(cloud_mul(s, a2), cloud_mul(c, b2));
}
// one cyclic sweep: (0,1), (0,2), (1,2)
VLSAT_CLOUD_HD void cloud_sweep(CloudEig& e) {
    cloud_rotate(e.a00, e.a11, e.a01, e.a02, e.a12, e.v00, e.v01, e.v10, e.v11, e.v20, e.v21);
    cloud_rotate(e.a00, e.a22, e.a02, e.a01, e.a12, e.v00, e.v02, e.v10, e.v12, e.v20, e.v22);
    cloud_rotate(e.a11, e.a22, e.a12, e.a01, e.a02, e.v01, e.v02, e.v11, e.v12, e.v21, e.v22);
}
VLSAT_CLOUD_HD void cloud_eig_start(CloudEig& e) {
    e.a00 = e.a11 = e.a22 = e.a01 = e.a02 = e.a12 = 0.0;
    e.v00 = e.v11 = e.v22 = 1.0;
    e.v01 = e.v02 = e.v10 = e.v12 = e.v20 = e.v21 = 0.0;
}

struct CloudNormal { double x, y, z, curvature; };

// The column of the smallest diagonal entry (ties to the lower index) and curvature = max(lambda_min, 0) / ((l0 + l1) + l2).
VLSAT_CLOUD_HD CloudNormal cloud_select(const CloudEig& e) {
    CloudNormal n;
    double lmin = e.a00;
    n.x = e.v00; n.y = e.v10; n.z = e.v20;
    if (e.a11 < lmin) { lmin = e.a11; n.x = e.v01; n.y = e.v11; n.z = e.v21; }
    if (e.a22 < lmin) { lmin = e.a22; n.x = e.v02; n.y = e.v12; n.z = e.v22; }
    n.curvature = cloud_div(lmin > 0.0 ? lmin : 0.0, cloud_trace(e));
    return n;
}

// The sign.  With a viewpoint: d = ((nx tx + ny ty) + nz tz), t = viewpoint - point; d < 0 flips, d > 0 keeps.  Without one, or when d
// is neither (0 or NaN): the component of largest magnitude is made positive, ties to the lower axis.  A flip negates all three.
VLSAT_CLOUD_HD void cloud_orient(CloudNormal& n, bool use_viewpoint, double tx, double ty, double tz) {
    bool flip;
    double d = 0.0;
    if (use_viewpoint) d = cloud_add(cloud_add(cloud_mul(n.x, tx), cloud_mul(n.y, ty)), cloud_mul(n.z, tz));
    if (d < 0.0) flip = true;
    else if (d > 0.0) flip = false;
    else {
        double big = n.x;
        if (fabs(n.y) > fabs(big)) big = n.y;
        if (fabs(n.z) > fabs(big)) big = n.z;
        flip = big < 0.0;
    }
    if (flip) { n.x = -n.x; n.y = -n.y; n.z = -n.z; }
}

// The whole rule for one point.  `members(k, x, y, z)` gives neighbour k < listed of the point (false: the entry names no point and
// is no member); the point itself, (px, py, pz), is the first member.  No estimate: normal (0, 0, 0), curvature 1.
template <class Members>
VLSAT_CLOUD_HD CloudNormal cloud_point_normal(const Members& members, int listed, double px, double py, double pz, int min_points,
                                              bool use_viewpoint, double vx, double vy, double vz) {
    CloudNormal none;
    none.x = none.y = none.z = 0.0;
    none.curvature = 1.0;
    double sx = px, sy = py, sz = pz, x, y, z;
    int n = 1;
    for (int k = 0; k < listed; ++k) {
        if (!members(k, x, y, z)) continue;
        sx = cloud_add(sx, x);
        sy = cloud_add(sy, y);
        sz = cloud_add(sz, z);
        ++n;
    }
    if (n < min_points) return none;
    const double cx = cloud_div(sx, (double)n), cy = cloud_div(sy, (double)n), cz = cloud_div(sz, (double)n);
    CloudEig e;
    cloud_eig_start(e);
    cloud_cov_add(e, px, py, pz, cx, cy, cz);
    for (int k = 0; k < listed; ++k)
        if (members(k, x, y, z)) cloud_cov_add(e, x, y, z, cx, cy, cz);
    if (!(cloud_trace(e) > 0.0)) return none;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < CLOUD_SWEEPS; ++sweep) cloud_sweep(e);
    CloudNormal r = cloud_select(e);
    cloud_orient(r, use_viewpoint, cloud_sub(vx, px), cloud_sub(vy, py), cloud_sub(vz, pz));
    return r;
}

// ---- segments of a cloud ---------------------------------------------------------------------------------------------------------
// w = fl(1 - |d|) clamped to [0, 2], d as in seg_weight; a NaN d gives 2.  Symmetric, never -0.
VLSAT_CLOUD_HD float cloud_unsigned_weight(float ax, float ay, float az, float bx, float by, float bz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
    const float w = __fsub_rn(1.0f, fabsf(d));
#else
    volatile float xx = ax * bx, yy = ay * by, zz = az * bz;
    volatile float s = xx + yy;
    const float d = s + zz;
    const float w = 1.0f - fabsf(d);
#endif
    if (d != d) return 2.0f;
    return w < 0.0f ? 0.0f : (w > 2.0f ? 2.0f : w);
}

VLSAT_CLOUD_HD bool cloud_sizes_ok(int64_t n_points, int64_t k) {
    return n_points >= 1 && n_points <= CLOUD_MAX_POINTS && k >= 1 && k <= CLOUD_MAX_K;
}
// the register capacity the kNN kernel is instantiated with: the least of 8, 16, 32 that holds K
VLSAT_CLOUD_HD int cloud_knn_capacity(int64_t k) { return k <= 8 ? 8 : (k <= 16 ? 16 : 32); }

}  // namespace vlsat
