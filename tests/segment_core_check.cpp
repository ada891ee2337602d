// Host-only check of csrc/segment_core.h (the arithmetic of the mesh segmenter): prints what the header computes, for
// tests/test_mesh_segment_cpu.py to compare with the numpy restatement and the library, and checks in place what needs no second opinion.
//   w ax ay az bx by bz -> bits     the weight of a pair of normals (all seven as fp32 bit patterns): axes, creases, NaN, infinities,
//                                   overflow, denormals, lengths above 1 (clamping at both ends) and pseudo-random values
//   k wbits root -> key             the packed key
//   r min_verts -> rounds           the round count
//   s n_verts -> bytes              the scratch size
// In place: w is symmetric, never negative, never -0, never above 2; key order equals (weight, root) order for every pair of a set that
// holds 0, denormals, 2.0 and the extreme roots; no key equals SEG_NO_KEY; 2^rounds >= min_verts > 2^(rounds - 1); the scratch parts
// are 16-byte aligned, in order and disjoint; edges and sizes out of range are refused.  tests/test_mesh_segment_cpu.py builds it with
// g++ -fsanitize=address,undefined and runs it as a child process; a non-zero exit status is a failure.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "segment_core.h"

using namespace vlsat;

static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float tiny = from_bits(1), big = 3.0e38f, r2 = 0.70710678f;
    std::vector<float> v = {0.f, -0.f, 1.f, -1.f, 0.5f, 0.6f, 0.8f, r2, -r2, 0.57735027f, 2.f, -2.f, 1e-20f, tiny, big, -big, inf, -inf, nan};
    uint32_t state = 12345u;
    for (int k = 0; k < 64; ++k) { state = state * 1664525u + 1013904223u; v.push_back((float)(int32_t)state / 2147483648.0f); }
    // normals from triples of the list: every special value meets every other
    std::vector<float> tri;
    const size_t n = v.size();
    for (size_t i = 0; i < n; ++i) { tri.push_back(v[i]); tri.push_back(v[(i * 7 + 3) % n]); tri.push_back(v[(i * 13 + 5) % n]); }
    for (size_t i = 0; i < n; ++i) { tri.push_back(v[i]); tri.push_back(0.f); tri.push_back(0.f); }
    const size_t m = tri.size() / 3;
    for (size_t i = 0; i < m; ++i)
        for (size_t j = 0; j < m; ++j) {
            const float* a = &tri[i * 3];
            const float* b = &tri[j * 3];
            const float w = seg_weight(a[0], a[1], a[2], b[0], b[1], b[2]);
            REQUIRE(w >= 0.f && w <= 2.f && !std::signbit(w));
            REQUIRE(seg_f32_bits(w) == seg_f32_bits(seg_weight(b[0], b[1], b[2], a[0], a[1], a[2])));
            if ((i * m + j) % 5 == 0)
                std::printf("w %08x %08x %08x %08x %08x %08x -> %08x\n", seg_f32_bits(a[0]), seg_f32_bits(a[1]), seg_f32_bits(a[2]),
                            seg_f32_bits(b[0]), seg_f32_bits(b[1]), seg_f32_bits(b[2]), seg_f32_bits(w));
        }
    REQUIRE(seg_weight(0, 0, 1, 0, 0, 1) == 0.f && seg_weight(0, 0, 1, 0, 1, 0) == 1.f && seg_weight(0, 0, 1, 0, 0, -1) == 2.f);
    REQUIRE(seg_weight(0, 0, 2, 0, 0, 2) == 0.f && seg_weight(0, 0, 2, 0, 0, -2) == 2.f && seg_weight(nan, 0, 0, 1, 0, 0) == 2.f);
    REQUIRE(seg_weight(inf, 0, 0, 1, 0, 0) == 0.f && seg_weight(inf, 0, 0, -1, 0, 0) == 2.f && seg_weight(inf, 1, 0, 1, -inf, 0) == 2.f);

    const float ws[] = {0.f, tiny, from_bits(0x007fffffu), from_bits(0x00800000u), 1e-7f, 0.25f, 0.5f, from_bits(0x3f000001u), 1.f, 1.9999999f, 2.f};
    const int32_t roots[] = {0, 1, 2, 65535, 65536, (1 << 24) - 2, (1 << 24) - 1};
    for (float wa : ws)
        for (int32_t ra : roots) {
            const unsigned long long ka = seg_key(wa, ra);
            REQUIRE(ka != SEG_NO_KEY && seg_key_root(ka) == ra);
            std::printf("k %08x %d -> %016llx\n", seg_f32_bits(wa), ra, ka);
            for (float wb : ws)
                for (int32_t rb : roots) {
                    const unsigned long long kb = seg_key(wb, rb);
                    const bool less = wa < wb || (wa == wb && ra < rb);
                    REQUIRE((ka < kb) == less && (ka == kb) == (wa == wb && ra == rb));
                }
        }

    const int64_t mins[] = {-5, 0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 19, 20, 31, 32, 33, 63, 64, 65, 1000, 1024, 1025, (int64_t)1 << 24,
                            ((int64_t)1 << 24) + 1, 0x7fffffff};
    for (int64_t mv : mins) {
        const int r = seg_rounds(mv);
        REQUIRE(r >= 0 && r <= 31 && ((int64_t)1 << r) >= mv && (r == 0 || ((int64_t)1 << (r - 1)) < mv));
        std::printf("r %lld -> %d\n", (long long)mv, r);
    }
    REQUIRE(seg_rounds(20) == 5 && seg_rounds(1) == 0 && seg_rounds(2) == 1);

    const int64_t sizes[] = {1, 2, 3, 4, 5, 1023, 1024, 1025, 2048, 2049, 54321, 1000000, SEG_MAX_VERTS - 1, SEG_MAX_VERTS};
    for (int64_t V : sizes) {
        const SegScratch s = seg_scratch_layout(V);
        const size_t at[] = {s.key, s.parent, s.root, s.size, s.num, s.block_count, s.block_first, s.bytes};
        const size_t need[] = {(size_t)V * 8, (size_t)V * 4, (size_t)V * 4, (size_t)V * 4, (size_t)V * 4, (size_t)s.tiles * 4, (size_t)(s.tiles + 1) * 4};
        REQUIRE(s.key == 0 && s.tiles * SEG_NUMBER_TILE >= V && (s.tiles - 1) * SEG_NUMBER_TILE < V);
        for (int k = 0; k < 7; ++k) REQUIRE(at[k] % 16 == 0 && at[k] + need[k] <= at[k + 1] && at[k + 1] - at[k] < need[k] + 16);
        std::printf("s %lld -> %zu\n", (long long)V, s.bytes);
    }
    REQUIRE(seg_sizes_ok(1, 0) && seg_sizes_ok(SEG_MAX_VERTS, SEG_MAX_EDGES));
    REQUIRE(!seg_sizes_ok(0, 0) && !seg_sizes_ok(SEG_MAX_VERTS + 1, 0) && !seg_sizes_ok(1, -1) && !seg_sizes_ok(1, SEG_MAX_EDGES + 1));
    REQUIRE(seg_edge_ok(0, 1, 2) && !seg_edge_ok(1, 1, 2) && !seg_edge_ok(-1, 1, 2) && !seg_edge_ok(0, 2, 2) && !seg_edge_ok(2, 0, 2));
    return 0;
}
