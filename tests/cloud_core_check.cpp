// Host-only check of csrc/cloud_core.h (the arithmetic of the point-cloud front end): prints what the header computes, for
// tests/test_cloud_cpu.py to compare bit for bit with the numpy restatements, and checks in place what needs no second opinion.
//   d ax ay az bx by bz j -> d2 key        the squared distance of two points (fp32 bit patterns) and the key with index j
//   u ax ay az bx by bz -> w               the unsigned weight of two normals
//   n vp vx vy vz min n m.. -> x y z c     one neighbourhood through cloud_point_normal: use_viewpoint, the viewpoint (fp64 bits),
//                                          min_points, the members (the point first; fp32 bits, three each) -> the normal and the
//                                          curvature as fp64 bits, before the rounding to fp32
// The neighbourhoods: planar (axis-aligned, tilted, a regular grid whose eigenvalues tie), collinear, isotropic (octahedron, cube),
// coincident points, fewer than min_points, the same shapes at 1e-6 and 1e+6 scale, pseudo-random ones; each without a viewpoint and
// with one on either side and one inside the surface (the dot product is 0: the axis rule decides).
// In place: d2 is symmetric and the key order equals (d2, j) order; cloud_insert keeps the CAP smallest keys ascending for CAP = 8, 16,
// 32 against std::sort; the unsigned weight is symmetric, in [0, 2], never -0, and equal for a normal and its negative; a normal has
// length 1 to 1e-12 and a curvature in [0, 1/3 + 1e-12] or is the "no estimate" pair.  tests/cloud_core_host.py builds it with g++
// -ffp-contract=off, optionally with -fsanitize=address,undefined, and runs it as a child process; a non-zero exit status is a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cloud_core.h"

using namespace vlsat;

static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
static unsigned long long f64_bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Members {
    const std::vector<float>* m;                                      // the point first, then its neighbours
    bool operator()(int k, double& x, double& y, double& z) const {
        x = (*m)[(size_t)(k + 1) * 3];
        y = (*m)[(size_t)(k + 1) * 3 + 1];
        z = (*m)[(size_t)(k + 1) * 3 + 2];
        return true;
    }
};

static uint32_t lcg_state = 2463534242u;
static float lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(int32_t)lcg_state / 2147483648.0f; }

static int emit(const std::vector<float>& m, int min_points, bool use_vp, double vx, double vy, double vz) {
    const int count = (int)(m.size() / 3);
    const Members mem{&m};
    const CloudNormal n = cloud_point_normal(mem, count - 1, (double)m[0], (double)m[1], (double)m[2], min_points, use_vp, vx, vy, vz);
    const bool none = n.x == 0.0 && n.y == 0.0 && n.z == 0.0 && n.curvature == 1.0;
    if (!none) {
        const double len = std::sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
        REQUIRE(std::fabs(len - 1.0) < 1e-12 && n.curvature >= 0.0 && n.curvature <= 1.0 / 3.0 + 1e-12);
    }
    std::printf("n %d %016llx %016llx %016llx %d %d", (int)use_vp, f64_bits(vx), f64_bits(vy), f64_bits(vz), min_points, count);
    for (float x : m) std::printf(" %08x", cloud_f32_bits(x));
    std::printf(" -> %016llx %016llx %016llx %016llx\n", f64_bits(n.x), f64_bits(n.y), f64_bits(n.z), f64_bits(n.curvature));
    return 0;
}

template <int CAP>
static int check_insert(const std::vector<unsigned long long>& keys) {
    unsigned long long best[CAP];
    for (int k = 0; k < CAP; ++k) best[k] = CLOUD_NO_KEY;
    for (unsigned long long key : keys) cloud_insert<CAP>(best, key);
    std::vector<unsigned long long> want = keys;
    std::sort(want.begin(), want.end());
    for (int k = 0; k < CAP; ++k) REQUIRE(best[k] == ((size_t)k < want.size() ? want[k] : CLOUD_NO_KEY));
    return 0;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const float tiny = from_bits(1), big = 3.0e38f;
    // ---- d2 and keys
    std::vector<float> v = {0.f, -0.f, 1.f, -1.f, 0.1f, 0.2f, 0.3f, 0.05f, 1e-20f, 1e-30f, tiny, 1e19f, big, -big, 1e6f, 1e6f + 0.0625f, 1e-6f};
    for (int k = 0; k < 48; ++k) v.push_back(lcg());
    const size_t nv = v.size();
    int32_t j = 0;
    for (size_t a = 0; a < nv; ++a)
        for (size_t b = 0; b < nv; ++b) {
            const float p[3] = {v[a], v[(a * 7 + 3) % nv], v[(a * 13 + 5) % nv]}, q[3] = {v[b], v[(b * 5 + 1) % nv], v[(b * 11 + 7) % nv]};
            const float d2 = cloud_d2(p[0], p[1], p[2], q[0], q[1], q[2]);
            REQUIRE(cloud_f32_bits(d2) == cloud_f32_bits(cloud_d2(q[0], q[1], q[2], p[0], p[1], p[2])) && !(d2 < 0.f) && !std::signbit(d2));
            j = (int32_t)((a * nv + b) * 2654435761u % (1u << 24));
            const unsigned long long key = cloud_key(d2, j);
            REQUIRE(cloud_key_index(key) == j && cloud_f32_bits(cloud_key_d2(key)) == cloud_f32_bits(d2) && (key != CLOUD_NO_KEY));
            if ((a * nv + b) % 3 == 0)
                std::printf("d %08x %08x %08x %08x %08x %08x %d -> %08x %016llx\n", cloud_f32_bits(p[0]), cloud_f32_bits(p[1]), cloud_f32_bits(p[2]),
                            cloud_f32_bits(q[0]), cloud_f32_bits(q[1]), cloud_f32_bits(q[2]), j, cloud_f32_bits(d2), key);
        }
    const float ds[] = {0.f, tiny, from_bits(0x007fffffu), from_bits(0x00800000u), 1e-7f, 0.0225f, from_bits(0x3cb851ecu), 1.f, big, inf};
    const int32_t js[] = {0, 1, 65535, 65536, (1 << 24) - 1};
    for (float da : ds)
        for (int32_t ja : js)
            for (float db : ds)
                for (int32_t jb : js) {
                    const unsigned long long ka = cloud_key(da, ja), kb = cloud_key(db, jb);
                    REQUIRE((ka < kb) == (da < db || (da == db && ja < jb)) && (ka == kb) == (da == db && ja == jb));
                }
    // ---- the insertion chain
    for (int n : {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 1000}) {
        std::vector<unsigned long long> keys;
        for (int k = 0; k < n; ++k) keys.push_back(cloud_key(std::fabs(lcg()) * (k % 3 ? 1.f : 0.f), (int32_t)(std::fabs(lcg()) * 1000.f) * 1000 + k));
        if (check_insert<8>(keys) || check_insert<16>(keys) || check_insert<32>(keys)) return 1;
        std::sort(keys.begin(), keys.end());
        if (check_insert<8>(keys)) return 1;
        std::reverse(keys.begin(), keys.end());
        if (check_insert<16>(keys) || check_insert<32>(keys)) return 1;
    }
    REQUIRE(cloud_knn_capacity(1) == 8 && cloud_knn_capacity(8) == 8 && cloud_knn_capacity(9) == 16 && cloud_knn_capacity(16) == 16 &&
            cloud_knn_capacity(17) == 32 && cloud_knn_capacity(32) == 32);
    REQUIRE(cloud_sizes_ok(1, 1) && cloud_sizes_ok(CLOUD_MAX_POINTS, 32) && !cloud_sizes_ok(0, 1) && !cloud_sizes_ok(CLOUD_MAX_POINTS + 1, 1) &&
            !cloud_sizes_ok(1, 0) && !cloud_sizes_ok(1, 33));

    // ---- the unsigned weight
    const float r2 = 0.70710678f, nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> w = {0.f, -0.f, 1.f, -1.f, 0.5f, 0.6f, 0.8f, r2, -r2, 0.57735027f, 2.f, -2.f, 1e-20f, tiny, big, -big, inf, -inf, nan};
    for (int k = 0; k < 32; ++k) w.push_back(lcg());
    const size_t nw = w.size();
    for (size_t a = 0; a < nw; ++a)
        for (size_t b = 0; b < nw; ++b) {
            const float p[3] = {w[a], w[(a * 7 + 3) % nw], w[(a * 13 + 5) % nw]}, q[3] = {w[b], w[(b * 5 + 1) % nw], w[(b * 11 + 7) % nw]};
            const float u = cloud_unsigned_weight(p[0], p[1], p[2], q[0], q[1], q[2]);
            REQUIRE(u >= 0.f && u <= 2.f && !std::signbit(u));
            REQUIRE(cloud_f32_bits(u) == cloud_f32_bits(cloud_unsigned_weight(q[0], q[1], q[2], p[0], p[1], p[2])));
            REQUIRE(cloud_f32_bits(u) == cloud_f32_bits(cloud_unsigned_weight(-p[0], -p[1], -p[2], q[0], q[1], q[2])));
            std::printf("u %08x %08x %08x %08x %08x %08x -> %08x\n", cloud_f32_bits(p[0]), cloud_f32_bits(p[1]), cloud_f32_bits(p[2]),
                        cloud_f32_bits(q[0]), cloud_f32_bits(q[1]), cloud_f32_bits(q[2]), cloud_f32_bits(u));
        }
    REQUIRE(cloud_unsigned_weight(0, 0, 1, 0, 0, 1) == 0.f && cloud_unsigned_weight(0, 0, 1, 0, 0, -1) == 0.f &&
            cloud_unsigned_weight(0, 0, 1, 0, 1, 0) == 1.f && cloud_unsigned_weight(0, 0, 0, 0, 0, 1) == 1.f &&
            cloud_unsigned_weight(nan, 0, 0, 1, 0, 0) == 2.f && cloud_unsigned_weight(0, 0, 2, 0, 0, -2) == 0.f);

    // ---- neighbourhoods
    std::vector<std::vector<float>> shapes;
    {   // a 3 x 3 grid in z = 0 around its centre: two eigenvalues tie exactly
        std::vector<float> m = {0.f, 0.f, 0.f};
        for (int a = -1; a <= 1; ++a) for (int b = -1; b <= 1; ++b) if (a || b) { m.push_back(a * 0.1f); m.push_back(b * 0.1f); m.push_back(0.f); }
        shapes.push_back(m);
    }
    {   // the same in x = 0.25 and y = -3, seen from a corner point
        std::vector<float> mx, my;
        for (int a = 0; a <= 2; ++a) for (int b = 0; b <= 2; ++b) {
            mx.push_back(0.25f); mx.push_back(a * 0.1f); mx.push_back(b * 0.1f);
            my.push_back(a * 0.1f); my.push_back(-3.f); my.push_back(b * 0.1f);
        }
        shapes.push_back(mx);
        shapes.push_back(my);
    }
    {   // a tilted plane x + 2 y - z = 1 with and without noise
        std::vector<float> m, noisy;
        for (int k = 0; k < 14; ++k) {
            const float x = lcg(), y = lcg(), z = x + 2.f * y - 1.f;
            m.push_back(x); m.push_back(y); m.push_back(z);
            noisy.push_back(x + 0.003f * lcg()); noisy.push_back(y + 0.003f * lcg()); noisy.push_back(z + 0.003f * lcg());
        }
        shapes.push_back(m);
        shapes.push_back(noisy);
    }
    {   // collinear: along an axis and along a diagonal
        std::vector<float> ax, dg;
        for (int k = 0; k < 7; ++k) { ax.push_back(k * 0.25f); ax.push_back(1.f); ax.push_back(-2.f); dg.push_back(k * 0.1f); dg.push_back(k * 0.2f); dg.push_back(k * -0.3f); }
        shapes.push_back(ax);
        shapes.push_back(dg);
    }
    {   // isotropic: the centre of an octahedron and of a cube
        std::vector<float> oc = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, -1.f};
        std::vector<float> cu = {0.5f, 0.5f, 0.5f};
        for (int k = 0; k < 8; ++k) { cu.push_back((float)(k & 1)); cu.push_back((float)((k >> 1) & 1)); cu.push_back((float)((k >> 2) & 1)); }
        shapes.push_back(oc);
        shapes.push_back(cu);
    }
    {   // coincident points, and two clusters of coincident points
        std::vector<float> same, two;
        for (int k = 0; k < 6; ++k) { same.push_back(0.3f); same.push_back(-0.7f); same.push_back(1.1f); two.push_back(k < 3 ? 0.f : 0.1f); two.push_back(2.f); two.push_back(2.f); }
        shapes.push_back(same);
        shapes.push_back(two);
    }
    for (int s = 0; s < 24; ++s) {  // pseudo-random, 3 .. 33 members, flat to round
        std::vector<float> m;
        const int count = 3 + (s * 7) % 31;
        const float flat = s % 4 == 0 ? 0.f : (s % 4 == 1 ? 0.01f : (s % 4 == 2 ? 0.2f : 1.f));
        for (int k = 0; k < count; ++k) { m.push_back(lcg()); m.push_back(lcg()); m.push_back(flat * lcg()); }
        shapes.push_back(m);
    }
    const size_t base = shapes.size();
    for (size_t s = 0; s < base; ++s)
        for (float scale : {1e-6f, 1e6f}) {
            std::vector<float> m = shapes[s];
            for (float& x : m) x *= scale;
            shapes.push_back(m);
        }
    for (const std::vector<float>& m : shapes) {
        const double px = m[0], py = m[1], pz = m[2];
        if (emit(m, 3, false, 0, 0, 0) || emit(m, 5, false, 0, 0, 0) || emit(m, 3, true, px + 1.0, py + 2.0, pz + 3.0) ||
            emit(m, 3, true, px - 1.0, py - 2.0, pz - 3.0) || emit(m, 3, true, px, py, pz) || emit(m, 3, true, px + 0.5, py, pz) ||
            emit(m, 3, true, px, py - 0.5, pz) || emit(m, 3, true, px, py, pz + 1e6) || emit(m, 33, false, 0, 0, 0))
            return 1;
    }
    return 0;
}
