// Host-only check of csrc/voxel_core.h (the arithmetic of the voxel-grid filter): prints what the header computes, for
// tests/test_voxel_cpu.py to compare bit for bit with the numpy restatement, and checks in place what needs no second opinion.
//   k x y z ox oy oz voxel -> key          the key of a point (fp32 bit patterns in, the 64-bit key out; all ones = out of range)
//   q x -> qp qn                           one value quantised as a position (2^24) and as a normal component (2^20), as signed decimals
//   m sum count -> mean                    the mean of a position sum (decimal in, fp32 bits out)
//   n sx sy sz -> nx ny nz                 the normal of three sums (decimals in, fp32 bits out)
//   c sum count -> value                   the rounded colour mean
// In place: cell coordinates at exact multiples of 0.125 and just below them, negative coordinates, the 2^20 and 32768 limits from both
// sides, non-finite coordinates, quantisation ties (half to even), colour rounding at .5, the key packing and its fields, the refused
// cell edges, the table size and the scratch layout.  tests/voxel_core_host.py builds it with g++ -ffp-contract=off, optionally with
// -fsanitize=address,undefined, and runs it as a child process; a non-zero exit status is a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "voxel_core.h"

using namespace vlsat;

static uint32_t f32_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static uint32_t lcg_state = 2463534242u;
static uint32_t lcg_u32() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float lcg() { return (float)(int32_t)lcg_u32() / 2147483648.0f; }

static void emit_key(float x, float y, float z, float ox, float oy, float oz, float voxel) {
    float inv = 0.0f;
    if (!voxel_inverse(voxel, inv)) return;
    std::printf("k %08x %08x %08x %08x %08x %08x %08x -> %016llx\n", f32_bits(x), f32_bits(y), f32_bits(z), f32_bits(ox), f32_bits(oy),
                f32_bits(oz), f32_bits(voxel), voxel_key(x, y, z, ox, oy, oz, inv));
}

static int cell(float x, float o, float voxel, int32_t& t) {
    float inv = 0.0f;
    if (!voxel_inverse(voxel, inv)) return -1;
    return voxel_axis(x, o, inv, t) ? 1 : 0;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    int32_t t = 0;
    // the refused cell edges: <= 0, NaN, +inf (inv = 0), and so small that 1 / voxel overflows
    float inv = 0.0f;
    REQUIRE(!voxel_inverse(0.0f, inv) && !voxel_inverse(-1.0f, inv) && !voxel_inverse(nan, inv) && !voxel_inverse(inf, inv));
    REQUIRE(!voxel_inverse(1e-39f, inv) && !voxel_inverse(std::numeric_limits<float>::denorm_min(), inv));
    REQUIRE(voxel_inverse(0.125f, inv) && inv == 8.0f && voxel_inverse(3e38f, inv) && inv > 0.0f);
    // exact multiples of 0.125 open a cell; the value just below belongs to the cell before; negative coordinates round down
    for (int k = -64; k <= 64; ++k) {
        const float x = (float)k * 0.125f;
        REQUIRE(cell(x, 0.0f, 0.125f, t) == 1 && t == k);
        REQUIRE(cell(std::nextafterf(x, -inf), 0.0f, 0.125f, t) == 1 && t == k - 1);
        REQUIRE(cell(x, 0.25f, 0.125f, t) == 1 && t == k - 2);
    }
    REQUIRE(cell(-0.0f, 0.0f, 0.125f, t) == 1 && t == 0);
    REQUIRE(cell(-1e-30f, 0.0f, 0.125f, t) == 1 && t == -1);
    // |x| < 32768 from both sides, and the non-finite values
    REQUIRE(cell(std::nextafterf(32768.0f, 0.0f), 0.0f, 1.0f, t) == 1 && t == 32767);
    REQUIRE(cell(32768.0f, 0.0f, 1.0f, t) == 0 && cell(-32768.0f, 0.0f, 1.0f, t) == 0);
    REQUIRE(cell(std::nextafterf(-32768.0f, 0.0f), 0.0f, 1.0f, t) == 1 && t == -32768);
    REQUIRE(cell(nan, 0.0f, 1.0f, t) == 0 && cell(inf, 0.0f, 1.0f, t) == 0 && cell(-inf, 0.0f, 1.0f, t) == 0);
    // |t| < 2^20 from both sides: cell edge 2^-10, so t = 2^20 at x = 1024
    const float edge = 0.0009765625f;
    REQUIRE(cell(std::nextafterf(1024.0f, 0.0f), 0.0f, edge, t) == 1 && t == 1048575);
    REQUIRE(cell(1024.0f, 0.0f, edge, t) == 0);
    REQUIRE(cell(-1023.9990234375f, 0.0f, edge, t) == 1 && t == -1048575);                   // the limit is on |t|, symmetric:
    REQUIRE(cell(std::nextafterf(-1024.0f, 0.0f), 0.0f, edge, t) == 0 && cell(-1024.0f, 0.0f, edge, t) == 0);   // floor(-1048575.9) = -2^20
    REQUIRE(cell(1.0f, 0.0f, 1e-38f, t) == 0 && cell(3e38f, -3e38f, 1e-38f, t) == 0);        // a huge or an overflowing product: out of range
    // the key: three 21-bit fields, biased by 2^20; never the empty value
    REQUIRE(voxel_pack(0, 0, 0) == ((1ull << 62) | (1ull << 41) | (1ull << 20)));
    REQUIRE(voxel_pack(-1048575, -1048575, -1048575) == ((1ull << 42) | (1ull << 21) | 1ull));
    REQUIRE(voxel_pack(1048575, 1048575, 1048575) == 0x7fffffffffffffffull && voxel_pack(1048575, 1048575, 1048575) != VOXEL_EMPTY);
    REQUIRE(voxel_pack(3, -2, 5) == (((1ull << 20) + 5) << 42 | ((1ull << 20) - 2) << 21 | ((1ull << 20) + 3)));
    REQUIRE(voxel_key(nan, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f) == VOXEL_EMPTY && voxel_key(0.0f, 0.0f, 40000.0f, 0.0f, 0.0f, 0.0f, 1.0f) == VOXEL_EMPTY);
    REQUIRE(voxel_key(0.3f, -0.3f, 2.5f, 0.0f, 0.0f, 0.0f, 1.0f) == voxel_pack(0, -1, 2));
    // quantisation: exact for everything with 24 fractional bits; ties go to even
    REQUIRE(voxel_quantise(1.0f, VOXEL_POINT_SCALE) == 16777216ll && voxel_quantise(-0.5f, VOXEL_POINT_SCALE) == -8388608ll);
    const float ulp = 5.9604644775390625e-08f;                                             // 2^-24
    REQUIRE(voxel_quantise(0.5f * ulp, VOXEL_POINT_SCALE) == 0 && voxel_quantise(1.5f * ulp, VOXEL_POINT_SCALE) == 2);
    REQUIRE(voxel_quantise(2.5f * ulp, VOXEL_POINT_SCALE) == 2 && voxel_quantise(-0.5f * ulp, VOXEL_POINT_SCALE) == 0);
    REQUIRE(voxel_quantise(-1.5f * ulp, VOXEL_POINT_SCALE) == -2 && voxel_quantise(0.75f * ulp, VOXEL_POINT_SCALE) == 1);
    REQUIRE(voxel_quantise(std::nextafterf(32768.0f, 0.0f), VOXEL_POINT_SCALE) == (1ll << 39) - (1ll << 15));
    REQUIRE(voxel_quantise_normal(nan) == 0 && voxel_quantise_normal(inf) == 0 && voxel_quantise_normal(-inf) == 0);
    REQUIRE(voxel_quantise_normal(32768.0f) == 0 && voxel_quantise_normal(1.0f) == 1048576ll && voxel_quantise_normal(-0.25f) == -262144ll);
    // the mean: one point gives its own coordinate back when it has at most 24 fractional bits
    REQUIRE(voxel_mean(voxel_quantise(0.3f, VOXEL_POINT_SCALE), 1) == 0.3f && voxel_mean(3ll << 24, 2) == 1.5f && voxel_mean(-(1ll << 24), 3) == -1.0f / 3.0f);
    // colours: (2 S + n) / (2 n): halves go up, and 255 stays 255
    REQUIRE(voxel_color(1, 2) == 1 && voxel_color(3, 2) == 2 && voxel_color(0, 5) == 0 && voxel_color(255u * 7u, 7) == 255);
    REQUIRE(voxel_color(4, 3) == 1 && voxel_color(5, 3) == 2 && voxel_color(255u << 24, 1 << 24) == 255 && voxel_color(509, 2) == 255);
    // normals: cancelling sums give zeros, a single axis gives a unit vector
    float nx, ny, nz;
    voxel_normal(0, 0, 0, nx, ny, nz);
    REQUIRE(nx == 0.0f && ny == 0.0f && nz == 0.0f && !std::signbit(nx));
    voxel_normal(0, -5, 0, nx, ny, nz);
    REQUIRE(nx == 0.0f && ny == -1.0f && nz == 0.0f);
    voxel_normal(3ll << 40, 0, 4ll << 40, nx, ny, nz);
    REQUIRE(nx == 0.6f && ny == 0.0f && nz == 0.8f);
    // the table and the scratch block
    REQUIRE(voxel_log2_slots(1) == 1 && voxel_log2_slots(2) == 2 && voxel_log2_slots(3) == 3 && voxel_log2_slots(4) == 3 && voxel_log2_slots(5) == 4);
    REQUIRE(voxel_log2_slots(VOXEL_MAX_POINTS) == 25 && !voxel_sizes_ok(0) && !voxel_sizes_ok(VOXEL_MAX_POINTS + 1) && voxel_sizes_ok(VOXEL_MAX_POINTS));
    for (int64_t v : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)100000, VOXEL_MAX_POINTS}) {
        const VoxelLayout l = voxel_layout(v);
        const size_t blocks = ((size_t)v + VOXEL_THREADS - 1) / VOXEL_THREADS;
        REQUIRE(((int64_t)1 << voxel_log2_slots(v)) >= 2 * v && ((int64_t)1 << voxel_log2_slots(v)) < 4 * v + 2);
        REQUIRE(l.table == 0 && l.slot_of_point >= ((size_t)16 << voxel_log2_slots(v)) && l.head_number >= l.slot_of_point + 4 * (size_t)v);
        REQUIRE(l.block_heads >= l.head_number + 4 * (size_t)v && l.point_sum >= l.block_heads + 4 * (blocks + 1));
        REQUIRE(l.normal_sum >= l.point_sum + 24 * (size_t)v && l.color_sum >= l.normal_sum + 24 * (size_t)v && l.bytes >= l.color_sum + 12 * (size_t)v);
        for (size_t off : {l.slot_of_point, l.head_number, l.block_heads, l.point_sum, l.normal_sum, l.color_sum, l.bytes}) REQUIRE(off % 256 == 0);
        for (int k = 0; k < 1000; ++k) REQUIRE(voxel_hash(((unsigned long long)lcg_u32() << 32) | lcg_u32(), voxel_log2_slots(v)) < (1u << voxel_log2_slots(v)));
    }

    // ---- rows for the restatement ----
    const float edges[] = {0.125f, 0.05f, 1.0f, 0.003f, 7.5f};
    const float origins[][3] = {{0.0f, 0.0f, 0.0f}, {0.0625f, -0.25f, 1.0f}, {-3.7f, 12.1f, 0.01f}};
    for (float e : edges)
        for (const auto& o : origins) {
            for (int k = 0; k < 60; ++k) emit_key(lcg() * 4.0f, lcg() * 4.0f, lcg() * 4.0f, o[0], o[1], o[2], e);
            for (int k = -8; k <= 8; ++k) emit_key((float)k * e, (float)k * 0.125f, (float)-k * e, o[0], o[1], o[2], e);
            emit_key(nan, 0.0f, 0.0f, o[0], o[1], o[2], e);
            emit_key(0.0f, inf, 0.0f, o[0], o[1], o[2], e);
            emit_key(0.0f, 0.0f, 32768.0f, o[0], o[1], o[2], e);
            emit_key(lcg() * 40000.0f, lcg() * 40000.0f, lcg() * 40000.0f, o[0], o[1], o[2], e);
            emit_key(lcg() * 30000.0f, lcg() * 3000.0f, lcg() * 300.0f, o[0], o[1], o[2], e);
        }
    std::vector<float> values = {0.0f, -0.0f, 1.0f, 0.3f, -0.3f, 0.5f * ulp, 1.5f * ulp, 2.5f * ulp, -2.5f * ulp, 32767.998f, -32767.998f};
    for (int k = 0; k < 300; ++k) values.push_back(lcg() * (k % 3 == 0 ? 1.0f : (k % 3 == 1 ? 1e-6f : 30000.0f)));
    for (float x : values) std::printf("q %08x -> %lld %lld\n", f32_bits(x), voxel_quantise(x, VOXEL_POINT_SCALE), voxel_quantise_normal(x));
    for (int k = 0; k < 300; ++k) {
        const int32_t count = 1 + (int32_t)(lcg_u32() % (k < 150 ? 40u : 16000000u));
        long long sum = 0;
        const float centre = lcg() * 100.0f;
        for (int j = 0; j < 8; ++j) sum += voxel_quantise(centre + lcg(), VOXEL_POINT_SCALE);
        sum = sum / 8 * count + (long long)(lcg_u32() % 1000u);
        std::printf("m %lld %d -> %08x\n", sum, count, f32_bits(voxel_mean(sum, count)));
        const long long sx = (long long)(int32_t)lcg_u32() * (k % 5), sy = (long long)(int32_t)lcg_u32() * 1000, sz = (long long)(int32_t)lcg_u32();
        voxel_normal(sx, sy, sz, nx, ny, nz);
        std::printf("n %lld %lld %lld -> %08x %08x %08x\n", sx, sy, sz, f32_bits(nx), f32_bits(ny), f32_bits(nz));
        const uint32_t csum = (uint32_t)(lcg_u32() % (255u * (uint32_t)count + 1u));
        std::printf("c %u %d -> %u\n", csum, count, (unsigned)voxel_color(csum, count));
    }
    return 0;
}
