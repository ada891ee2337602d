// Host-only check of csrc/plane_core.h (the arithmetic of the structural-plane search): prints what the header computes, for
// tests/test_objects_cpu.py to compare bit for bit with the numpy restatement, and checks in place what needs no second opinion.
//   d seed k n -> rank                      one draw (decimals)
//   p ax ay az bx by bz cx cy cz -> ok nx ny nz d     the plane through three points (fp32 bit patterns; ok is 0 or 1)
//   s nx ny nz d x y z dist -> score class  the score of a point (fp32 bit patterns) and its class: 0 inlier, 1 above, 2 below
//   e inliers above n min_inliers ppm -> eligible
//   k inliers h -> key                      (decimals in, the 64-bit key in hex out)
// In place: the axis-aligned planes and their sign, ties of the largest component, void triples (repeated and collinear points), points
// at exactly +-dist and one float beyond, NaN scores, the eligibility bound with its integer division, the order of the keys, the limits and both scratch layouts.  tests/plane_core_host.py builds it with g++ -ffp-contract=off,
// optionally with -fsanitize=address,undefined, and runs it as a child process; a non-zero exit status is a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "plane_core.h"

using namespace vlsat;

static uint32_t f32_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static uint32_t lcg_state = 2463534242u;
static uint32_t lcg_u32() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float lcg() { return (float)(int32_t)lcg_u32() / 2147483648.0f; }

static bool plane3(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, Plane& pl) {
    const float a[3] = {ax, ay, az}, b[3] = {bx, by, bz}, c[3] = {cx, cy, cz};
    return plane_from_points(a, b, c, pl);
}

static void emit_plane(const float* a, const float* b, const float* c) {
    Plane pl;
    const bool ok = plane_from_points(a, b, c, pl);
    std::printf("p %08x %08x %08x %08x %08x %08x %08x %08x %08x -> %d %08x %08x %08x %08x\n", f32_bits(a[0]), f32_bits(a[1]), f32_bits(a[2]),
                f32_bits(b[0]), f32_bits(b[1]), f32_bits(b[2]), f32_bits(c[0]), f32_bits(c[1]), f32_bits(c[2]), (int)ok, f32_bits(pl.nx),
                f32_bits(pl.ny), f32_bits(pl.nz), f32_bits(pl.d));
}

static int klass(float s, float dist) { return plane_inlier(s, dist) ? 0 : (plane_above(s, dist) ? 1 : 2); }

static void emit_score(const Plane& pl, float x, float y, float z, float dist) {
    const float s = plane_score(pl.nx, pl.ny, pl.nz, pl.d, x, y, z);
    std::printf("s %08x %08x %08x %08x %08x %08x %08x %08x -> %08x %d\n", f32_bits(pl.nx), f32_bits(pl.ny), f32_bits(pl.nz), f32_bits(pl.d),
                f32_bits(x), f32_bits(y), f32_bits(z), f32_bits(dist), f32_bits(s), klass(s, dist));
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    Plane pl;
    // the three axis-aligned planes, the normal's largest component positive whatever the winding
    REQUIRE(plane3(0, 0, 0, 1, 0, 0, 0, 1, 0, pl) && pl.nx == 0.0f && pl.ny == 0.0f && pl.nz == 1.0f && pl.d == 0.0f);
    REQUIRE(plane3(0, 0, 0, 0, 1, 0, 1, 0, 0, pl) && pl.nz == 1.0f && pl.d == 0.0f);
    REQUIRE(plane3(0, 0, 2, 4, 0, 2, 0, 0.5f, 2, pl) && pl.nz == 1.0f && pl.d == -2.0f);
    REQUIRE(plane3(3, 0, 0, 3, 1, 0, 3, 0, 1, pl) && pl.nx == 1.0f && pl.ny == 0.0f && pl.nz == 0.0f && pl.d == -3.0f);
    REQUIRE(plane3(0, -1, 0, 0, -1, 1, 1, -1, 0, pl) && pl.ny == 1.0f && pl.d == 1.0f);
    // ties of the largest component go to the lower axis: m = (-1, -1, 0) is flipped, (1, 1, 0) and (1, -1, 0) are kept, and (-1, 1, 0)
    // is flipped to (1, -1, 0)
    REQUIRE(plane3(0, 0, 0, 1, -1, 0, 0, 0, 1, pl) && pl.nx > 0.0f && pl.nx == pl.ny && pl.nz == 0.0f);
    REQUIRE(plane3(0, 0, 0, 0, 0, 1, 1, -1, 0, pl) && pl.nx > 0.0f && pl.nx == pl.ny);
    REQUIRE(plane3(0, 0, 0, 1, 1, 0, 0, 0, 1, pl) && pl.nx > 0.0f && pl.ny == -pl.nx);
    REQUIRE(plane3(0, 0, 0, 0, 0, 1, 1, 1, 0, pl) && pl.nx > 0.0f && pl.ny == -pl.nx);
    // void: a repeated point and three collinear points; the largest fp32 coordinates still give a finite l2
    REQUIRE(!plane3(1, 2, 3, 1, 2, 3, 4, 5, 6, pl) && pl.nx == 0.0f && pl.ny == 0.0f && pl.nz == 0.0f && pl.d == 0.0f);
    REQUIRE(!plane3(1, 2, 3, 4, 5, 6, 1, 2, 3, pl) && !plane3(0, 0, 0, 1, 1, 1, 3, 3, 3, pl) && !plane3(5, 5, 5, 5, 5, 5, 5, 5, 5, pl));
    REQUIRE(plane3(-3e38f, -3e38f, 0, 3e38f, -3e38f, 0, -3e38f, 3e38f, 0, pl) && pl.nz == 1.0f && pl.d == 0.0f);   // l2 ~ 2e155: finite
    // the score and its classes: exactly +-dist is an inlier, one float beyond is not, a NaN is below
    const Plane flat = {0.0f, 0.0f, 1.0f, 0.0f};
    const float dist = 0.125f, up = std::nextafterf(dist, inf);
    REQUIRE(klass(plane_score(0, 0, 1, 0, 7, -3, dist), dist) == 0 && klass(plane_score(0, 0, 1, 0, 7, -3, -dist), dist) == 0);
    REQUIRE(klass(plane_score(0, 0, 1, 0, 7, -3, up), dist) == 1 && klass(plane_score(0, 0, 1, 0, 7, -3, -up), dist) == 2);
    REQUIRE(klass(nan, dist) == 2 && klass(inf, dist) == 1 && klass(-inf, dist) == 2 && klass(0.0f, dist) == 0 && klass(-0.0f, dist) == 0);
    REQUIRE(klass(plane_score(0, 0, 1, inf, 1, 1, -inf), dist) == 2);                          // inf - inf
    REQUIRE(plane_score(0.5f, 0.25f, 2.0f, -1.0f, 2.0f, 4.0f, 8.0f) == 17.0f);
    REQUIRE(plane_point_valid(0, -0.0f, 3e38f) && !plane_point_valid(nan, 0, 0) && !plane_point_valid(0, inf, 0) && !plane_point_valid(0, 0, -inf));
    // eligibility: the bound is (n ppm) / 10^6 in integers, and min(above, below) must not exceed it
    REQUIRE(plane_outside_limit(530, 10000) == 5 && plane_outside_limit(99, 10000) == 0 && plane_outside_limit(1 << 24, 500000) == 1 << 23);
    REQUIRE(plane_outside_limit(1 << 24, 499999) == 8388591);                                  // the product needs 64 bits
    REQUIRE(plane_eligible(400, 130, 530, 50, 10000) && !plane_eligible(100, 30, 530, 50, 10000) && plane_eligible(100, 30, 130, 50, 500000));
    REQUIRE(!plane_eligible(49, 0, 530, 50, 10000) && plane_eligible(50, 5, 530, 50, 10000) && !plane_eligible(50, 6, 62, 50, 10000));
    REQUIRE(plane_eligible(50, 475, 530, 50, 10000) && !plane_eligible(50, 474, 530, 50, 10000));   // below = 5 and 6
    // the key: more inliers win; equal inliers: the lower h wins; never 0 for three inliers or more
    REQUIRE(plane_key(10, 5) > plane_key(9, 0) && plane_key(10, 4) > plane_key(10, 5) && plane_key(3, 4095) != 0ull);
    REQUIRE(plane_key(1 << 24, 0) == (((unsigned long long)1 << 56) | 0xFFFFFFFFull) && plane_key_hypothesis(plane_key(77, 4095)) == 4095);
    REQUIRE(plane_key_hypothesis(plane_key(3, 0)) == 0);
    // the draw: below n, and the whole range is reached
    {
        std::vector<int> seen(7, 0);
        for (unsigned long long k = 0; k < 2000; ++k) {
            const uint32_t r = plane_draw(12345ull, k, 7u);
            REQUIRE(r < 7u);
            seen[r] = 1;
        }
        for (int v : seen) REQUIRE(v == 1);
        REQUIRE(plane_draw(0ull, 0ull, 1u) == 0u && plane_draw(~0ull, ~0ull, 1u << 24) < (1u << 24));
    }
    // the limits and the scratch blocks
    REQUIRE(plane_sizes_ok(3, 1, 1) && plane_sizes_ok(PLANE_MAX_POINTS, PLANE_MAX_HYP, PLANE_MAX_PLANES) && !plane_sizes_ok(2, 1, 1));
    REQUIRE(!plane_sizes_ok(PLANE_MAX_POINTS + 1, 1, 1) && !plane_sizes_ok(3, 0, 1) && !plane_sizes_ok(3, 4097, 1) && !plane_sizes_ok(3, 1, 0) && !plane_sizes_ok(3, 1, 33));
    REQUIRE(cluster_sizes_ok(1, 1) && cluster_sizes_ok(PLANE_MAX_POINTS, 32) && !cluster_sizes_ok(0, 1) && !cluster_sizes_ok(1, 0) && !cluster_sizes_ok(1, 33));
    for (int64_t v : {(int64_t)3, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)100000, PLANE_MAX_POINTS})
        for (int32_t h : {1, 65, 256, 300, 4096}) {
            const PlaneLayout l = plane_layout(v, h);
            const size_t blocks = plane_blocks(v);
            REQUIRE(blocks * PLANE_THREADS >= (size_t)v && (blocks - 1) * PLANE_THREADS < (size_t)v);
            REQUIRE(l.state == 0 && l.best >= 32 && l.hyp >= l.best + 8 && l.hyp_ok >= l.hyp + 16 * (size_t)h && l.counts >= l.hyp_ok + 4 * (size_t)h);
            REQUIRE(l.alive >= l.counts + 8 * (size_t)h && l.alive_list >= l.alive + 4 * (size_t)v && l.block_alive >= l.alive_list + 4 * (size_t)v);
            REQUIRE(l.bytes >= l.block_alive + 4 * (blocks + 1));
            for (size_t off : {l.best, l.hyp, l.hyp_ok, l.counts, l.alive, l.alive_list, l.block_alive, l.bytes}) REQUIRE(off % 256 == 0);
            const ClusterLayout c = cluster_layout(v);
            REQUIRE(c.parent == 0 && c.root >= 4 * (size_t)v && c.size >= c.root + 4 * (size_t)v && c.num >= c.size + 4 * (size_t)v);
            REQUIRE(c.block_kept >= c.num + 4 * (size_t)v && c.bytes >= c.block_kept + 4 * (blocks + 1));
            for (size_t off : {c.root, c.size, c.num, c.block_kept, c.bytes}) REQUIRE(off % 256 == 0);
        }

    // ---- rows for the restatement ----
    const unsigned long long seeds[] = {0ull, 1ull, 0x9E3779B97F4A7C15ull, ~0ull, 123456789012345ull};
    for (unsigned long long seed : seeds)
        for (int i = 0; i < 40; ++i) {
            const unsigned long long k = i < 20 ? (unsigned long long)i : ((unsigned long long)lcg_u32() << 20) | lcg_u32();
            const uint32_t n = i % 4 == 0 ? 3u : 1u + lcg_u32() % (1u << 24);
            std::printf("d %llu %llu %u -> %u\n", seed, k, n, plane_draw(seed, k, n));
        }
    std::vector<Plane> planes;
    for (int i = 0; i < 400; ++i) {
        const float scale = i % 4 == 0 ? 1.0f : (i % 4 == 1 ? 10.0f : (i % 4 == 2 ? 1e-3f : 3e4f));
        float a[3], b[3], c[3];
        for (int j = 0; j < 3; ++j) { a[j] = lcg() * scale; b[j] = lcg() * scale; c[j] = lcg() * scale; }
        if (i % 7 == 0) b[2] = c[2] = a[2];                                                  // a horizontal plane
        if (i % 11 == 0) { c[0] = b[0]; c[1] = b[1]; c[2] = b[2]; }                          // a repeated point
        if (i % 13 == 0) for (int j = 0; j < 3; ++j) c[j] = a[j] + 2.0f * (b[j] - a[j]);     // (nearly) collinear
        emit_plane(a, b, c);
        if (plane_from_points(a, b, c, pl)) planes.push_back(pl);
    }
    planes.push_back(flat);
    for (size_t i = 0; i < planes.size(); ++i)
        for (int j = 0; j < 6; ++j) {
            const float scale = j % 3 == 0 ? 1.0f : (j % 3 == 1 ? 10.0f : 1e-2f);
            emit_score(planes[i], lcg() * scale, lcg() * scale, lcg() * scale, j % 2 ? 0.02f : 0.125f);
        }
    emit_score(flat, 1.0f, 2.0f, dist, dist);
    emit_score(flat, 1.0f, 2.0f, up, dist);
    emit_score(flat, 1.0f, 2.0f, -dist, dist);
    emit_score(flat, 1.0f, 2.0f, -up, dist);
    emit_score(flat, nan, 2.0f, 0.0f, dist);
    emit_score(flat, 1.0f, inf, 0.0f, dist);
    for (int i = 0; i < 300; ++i) {
        const int32_t n = 3 + (int32_t)(lcg_u32() % (i < 150 ? 1000u : (1u << 24) - 3u));
        const int32_t inliers = (int32_t)(lcg_u32() % (uint32_t)(n + 1)), above = (int32_t)(lcg_u32() % (uint32_t)(n - inliers + 1));
        const int32_t min_inliers = 3 + (int32_t)(lcg_u32() % (uint32_t)n), ppm = (int32_t)(lcg_u32() % 500001u);
        std::printf("e %d %d %d %d %d -> %d\n", inliers, above, n, min_inliers, ppm, (int)plane_eligible(inliers, above, n, min_inliers, ppm));
        const int32_t h = (int32_t)(lcg_u32() % 4096u);
        std::printf("k %d %d -> %016llx\n", inliers, h, plane_key(inliers, h));
    }
    return 0;
}
