// Host-only check of csrc/convex_core.h (the arithmetic of the convexity clusters): prints what the header computes, for
// tests/test_convex_cpu.py to compare bit for bit with the numpy restatement, and checks in place what needs no second opinion.
//   t xi[3] ni[3] xj[3] nj[3] tau q -> c c' usable_i usable_j q_ok concave      fp32 bit patterns; c' is c seen from j
// In place: c on a convex and on a concave crease derived by hand, c from both ends (equal bits, but for the sign of a zero), d = 0,
// the test at equality and one float beyond, tau = 0 and 1, NaN, the usable normals, the distances that count, the limits and the scratch layout.  tests/convex_core_host.py
// builds it with g++ -ffp-contract=off, optionally with -fsanitize=address,undefined, and runs it as a child process; a non-zero exit
// status is a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "convex_core.h"

using namespace vlsat;

static uint32_t f32_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float bits_f32(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static uint32_t lcg_state = 2463534242u;
static uint32_t lcg_u32() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float lcg() { return (float)(int32_t)lcg_u32() / 2147483648.0f; }

static int emit(const float* xi, const float* ni, const float* xj, const float* nj, float tau, float q) {
    const float c = convex_c(xi, ni, xj, nj), back = convex_c(xj, nj, xi, ni);
    // the same bit pattern from either end; only a zero may change its sign (x + -x is +0 from both ends) and a NaN its payload
    REQUIRE((c != c) == (back != back) && (c == 0.0f) == (back == 0.0f));
    if (c == c && c != 0.0f) REQUIRE(f32_bits(c) == f32_bits(back));
    const float* all[4] = {xi, ni, xj, nj};
    std::printf("t");
    for (int a = 0; a < 4; ++a)
        for (int d = 0; d < 3; ++d) std::printf(" %08x", f32_bits(all[a][d]));
    std::printf(" %08x %08x -> %08x %08x %d %d %d %d\n", f32_bits(tau), f32_bits(q), f32_bits(c), f32_bits(back),
                (int)convex_normal_usable(ni[0], ni[1], ni[2]), (int)convex_normal_usable(nj[0], nj[1], nj[2]), (int)convex_sqdist_ok(q),
                (int)convex_concave(c, tau, q));
    return 0;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float up[3] = {0, 0, 1}, right[3] = {1, 0, 0}, left[3] = {-1, 0, 0}, zero[3] = {0, 0, 0};
    // a floor point and a point on a wall that rises from it at x = 0 (the wall's normal looks along +x): a CONCAVE junction.
    // d = (-1, 0, 1): a = n_i . d = 1, b = n_j . d = -1, c = 2
    const float floor_pt[3] = {1, 0, 0}, wall_pt[3] = {0, 0, 1};
    REQUIRE(convex_c(floor_pt, up, wall_pt, right) == 2.0f && convex_c(wall_pt, right, floor_pt, up) == 2.0f);
    // a table top and its side that falls from the edge x = 0 (the side's normal looks along -x, the point lies below): CONVEX, c = -2
    const float top_pt[3] = {1, 0, 0}, side_pt[3] = {0, 0, -1};
    REQUIRE(convex_c(top_pt, up, side_pt, left) == -2.0f && convex_c(side_pt, left, top_pt, up) == -2.0f);
    // one plane, equal normals: c = 0 whatever d is; coincident points: d = 0 and c = 0
    const float far_pt[3] = {5, -3, 0};
    REQUIRE(convex_c(floor_pt, up, far_pt, up) == 0.0f && convex_c(floor_pt, up, floor_pt, right) == 0.0f);
    // the test: c > 0 and fl(c c) > fl(fl(tau tau) q).  c = 0.5, tau = 0.5, q = 1: 0.25 > 0.25 is false, one float above is true
    REQUIRE(!convex_concave(0.5f, 0.5f, 1.0f) && convex_concave(bits_f32(f32_bits(0.5f) + 1), 0.5f, 1.0f));
    REQUIRE(!convex_concave(0.5f, 0.5f, bits_f32(f32_bits(1.0f) + 1)) && convex_concave(0.5f, 0.5f, bits_f32(f32_bits(1.0f) - 1)));
    REQUIRE(!convex_concave(-2.0f, 0.0f, 1.0f) && !convex_concave(0.0f, 0.0f, 1.0f) && !convex_concave(-0.0f, 0.0f, 0.0f));
    REQUIRE(convex_concave(1e-30f, 0.0f, 1.0f) == false);                              // fl(c c) underflows to 0: 0 > 0 is false
    REQUIRE(convex_concave(1e-10f, 0.0f, 1.0f) && convex_concave(2.0f, 1.0f, 3.9f) && !convex_concave(2.0f, 1.0f, 4.0f));
    REQUIRE(!convex_concave(nan, 0.0f, 1.0f) && !convex_concave(1.0f, 0.0f, nan) && !convex_concave(1.0f, nan, 1.0f));
    REQUIRE(convex_concave(3e38f, 1.0f, 3e38f) && !convex_concave(inf, 1.0f, inf));    // inf > 3e38; inf > inf is false
    // usable normals and distances that count
    REQUIRE(convex_normal_usable(0, 0, 1) && convex_normal_usable(1e-45f, 0, 0) && convex_normal_usable(3e38f, -3e38f, 3e38f));
    REQUIRE(!convex_normal_usable(0, 0, 0) && !convex_normal_usable(-0.0f, 0, -0.0f) && !convex_normal_usable(nan, 0, 1));
    REQUIRE(!convex_normal_usable(0, inf, 1) && !convex_normal_usable(0, 1, -inf));
    REQUIRE(convex_sqdist_ok(0.0f) && convex_sqdist_ok(-0.0f) && convex_sqdist_ok(3.4e38f) && !convex_sqdist_ok(inf) && !convex_sqdist_ok(nan) &&
            !convex_sqdist_ok(-1e-45f));
    // the limits and the layout: 28 bytes per point in seven aligned parts, then the block counts
    REQUIRE(convex_sizes_ok(1, 1) && convex_sizes_ok((int64_t)1 << 24, 32) && !convex_sizes_ok(0, 1) && !convex_sizes_ok(((int64_t)1 << 24) + 1, 1));
    REQUIRE(!convex_sizes_ok(5, 0) && !convex_sizes_ok(5, 33) && CONVEX_MAX_ROUNDS == 64);
    for (int64_t v : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)257, (int64_t)100000, (int64_t)1 << 24}) {
        const ConvexLayout l = convex_layout(v);
        const size_t parts[9] = {l.parent, l.root, l.size, l.boundary, l.label_a, l.label_b, l.num, l.block_kept, l.bytes};
        REQUIRE(parts[0] == 0);
        for (int a = 0; a < 8; ++a) REQUIRE(parts[a] % 256 == 0 && parts[a + 1] >= parts[a] + (a < 7 ? 4 * (size_t)v : 4 * (plane_blocks(v) + 1)));
        REQUIRE(l.bytes % 256 == 0 && l.bytes <= 28 * (size_t)v + 4 * plane_blocks(v) + 9 * 256);
    }
    // rows for the restatement: random triples, then the special values in every place
    for (int t = 0; t < 3000; ++t) {
        float x[4][3];
        for (int a = 0; a < 4; ++a)
            for (int d = 0; d < 3; ++d) x[a][d] = lcg();
        const float scale = (t % 5 == 4) ? 0.01f : 1.0f;                               // every fifth pair lies close, as table entries do
        for (int d = 0; d < 3; ++d) x[2][d] = x[0][d] + scale * x[2][d];
        const float tau = t % 7 == 0 ? 0.0f : t % 7 == 1 ? 1.0f : 0.5f * (lcg() + 1.0f), q = fabsf(lcg()) * scale * scale * 3.0f;
        if (emit(x[0], x[1], x[2], x[3], tau, q)) return 1;
    }
    const float special[10] = {0.0f, -0.0f, nan, inf, -inf, 3e38f, -3e38f, 1e-38f, 1e-45f, 1.0f};
    for (int t = 0; t < 600; ++t) {
        float x[4][3];
        for (int a = 0; a < 4; ++a)
            for (int d = 0; d < 3; ++d) x[a][d] = lcg();
        x[t % 4][(t / 4) % 3] = special[(t / 12) % 10];
        if (t % 3 == 0) x[(t + 1) % 4][t % 3] = special[(t / 7) % 10];
        if (t % 50 == 0) memcpy(x[2], x[0], sizeof x[0]);                              // d = 0
        if (t % 50 == 1) memcpy(x[1], zero, sizeof zero);                              // a zero normal
        const float tau = t % 2 ? 1.0f : 0.0f, q = special[(t / 3) % 10];
        if (emit(x[0], x[1], x[2], x[3], tau, q)) return 1;
    }
    for (int t = 0; t < 200; ++t) {                                                    // values near the largest float: products overflow
        float x[4][3];
        for (int a = 0; a < 4; ++a)
            for (int d = 0; d < 3; ++d) x[a][d] = lcg() * (a % 2 ? 1.0f : 3e38f);
        if (t % 2) for (int d = 0; d < 3; ++d) x[3][d] *= 3e38f;
        if (emit(x[0], x[1], x[2], x[3], 0.17f, fabsf(lcg()) * 3e38f)) return 1;
    }
    return 0;
}
