// Host-only check of the split-fp16 GEMM's plane arithmetic (csrc/gemm_f16s_planes.h) and of the sibling list and pick function of
// csrc/gemm_plan.h.  g++ only (optionally ASan + UBSan): no HIP header, no library, no device.  One line per check: "<name> -> ok ...".
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gemm_f16s_planes.h"
#include "gemm_plan.h"

using namespace vlsat;

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }
static float uniform() { return (float)((rng() >> 8) * (1.0 / 16777216.0)) * 2.f - 1.f; }

// an independent fp16 -> double: the definition, not the header's code
static double half_value(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    const double v = e == 31 ? (m ? NAN : INFINITY) : e ? std::ldexp(1.0 + m / 1024.0, e - 15) : std::ldexp((double)m, -24);
    return (h & 0x8000) ? -v : v;
}

static int fails = 0;
static void line(const char* name, bool ok, const char* fmt, long a = 0, long b = 0) {
    char buf[128];
    std::snprintf(buf, sizeof buf, fmt, a, b);
    std::printf("%s -> %s %s\n", name, ok ? "ok" : "FAILED", buf);
    if (!ok) ++fails;
}

// k, planes and their properties for one tensor; returns the number of violations
static long check_tensor(const std::vector<float>& w, int* k_out = nullptr) {
    uint32_t mx = 0;
    for (float x : w) { const uint32_t a = f16s_bits(x) & 0x7fffffffu; mx = a > mx ? a : mx; }
    const int k = f16s_exponent(mx);
    if (k_out) *k_out = k;
    long bad = 0;
    const double top = std::ldexp((double)f16s_float(mx), k);
    if (mx && k > -F16S_K_MAX && k < F16S_K_MAX && !(top > 4096.0 && top <= 8192.0)) ++bad;      // max |W 2^k| in (2^12, 2^13]
    if (!mx && k != 0) ++bad;
    if (f16s_pow2(k) != std::ldexp(1.f, k)) ++bad;
    for (float x : w) {
        uint16_t hi, lo;
        f16s_split(x, k, hi, lo);
        const double s = std::ldexp((double)x, k), h = half_value(hi), l = half_value(lo);
        if (!std::isfinite(h) || !std::isfinite(l)) { ++bad; continue; }
        if (std::fabs(s) <= 65504.0 && std::fabs(h + l - s) > std::ldexp(std::fabs(s), -22) + std::ldexp(1.0, -25)) ++bad;      // hi + lo within 2^-22 (lo below fp16's normal range: + half a subnormal ulp)
        if ((double)f16s_from_half(hi) != h || (double)f16s_from_half(lo) != l) ++bad;                                       // the header's own fp16 -> fp32
        // Wh 2^-11 is exact in fp16 whenever |Wh| >= 2^-3 (or zero): the product must be a normal fp16 number or zero
        const double third = h / 2048.0;
        if ((h == 0.0 || std::fabs(h) >= 0.125) && half_value(f16s_to_half((float)third)) != third) ++bad;
        if (std::signbit(x) != ((hi & 0x8000) != 0) && (hi & 0x7fff)) ++bad;
    }
    return bad;
}

int main() {
    // fp32 -> fp16 of the header against the definition: every fp16 value, the midpoints between neighbours (ties to even), random bits
    {
        long bad = 0, n = 0;
        for (uint32_t h = 0; h < 0x7c00; ++h) {
            const double v = half_value((uint16_t)h), v1 = h + 1 < 0x7c00 ? half_value((uint16_t)(h + 1)) : 65536.0;
            const float exact = (float)v, mid = (float)(0.5 * (v + v1)), below = std::nextafterf(mid, 0.f), above = std::nextafterf(mid, 1e30f);
            const uint16_t up = h + 1 < 0x7c00 ? (uint16_t)(h + 1) : (uint16_t)0x7c00, even = (h & 1) ? up : (uint16_t)h;
            bad += f16s_to_half(exact) != h;
            bad += f16s_to_half(-exact) != (h | 0x8000u);
            bad += f16s_to_half(mid) != even;
            bad += f16s_to_half(below) != h;
            bad += f16s_to_half(above) != up;
            n += 5;
        }
        for (int i = 0; i < 200000; ++i) {
            const float x = f16s_float(rng());
            if (!std::isfinite(x)) continue;
            const uint16_t got = f16s_to_half(x);
            const double v = half_value(got), ax = std::fabs((double)x);
            // nearest: no fp16 neighbour is closer
            const uint16_t mag = got & 0x7fff;
            const double dn = mag ? half_value((uint16_t)(mag - 1)) : 0.0, upv = mag < 0x7bff ? half_value((uint16_t)(mag + 1)) : 65536.0;
            if (mag == 0x7c00) bad += ax < 65520.0;
            else bad += std::fabs(std::fabs(v) - ax) > std::fabs(dn - ax) || std::fabs(std::fabs(v) - ax) > std::fabs(upv - ax);
            ++n;
        }
        line("to_half", bad == 0, "%ld conversions, %ld wrong", n, bad);
    }
    // the planes: random Xavier-like tensors, tiny, huge, zero and negative-zero weights
    {
        long bad = 0, tensors = 0;
        for (int t = 0; t < 40; ++t) {
            const float scale = std::ldexp(1.f, -30 + 2 * t) * (0.6f + 0.4f * std::fabs(uniform()));      // 2^-30 .. 2^48
            std::vector<float> w(1500);
            for (float& x : w) x = uniform() * scale;
            w[3] = 0.f; w[4] = -0.f; w[5] = scale; w[6] = -scale; w[7] = scale * 1e-7f; w[8] = f16s_float(1u);      // (a denormal element)
            bad += check_tensor(w);
            ++tensors;
        }
        int k = 99;
        bad += check_tensor(std::vector<float>(64, 0.f), &k); bad += k != 0; ++tensors;
        bad += check_tensor(std::vector<float>(64, -0.f), &k); bad += k != 0; ++tensors;
        bad += check_tensor({1.f}, &k); bad += k != 13; ++tensors;                    // a power of two: ceil(log2) = log2
        bad += check_tensor({-1.0000001f, 0.5f}, &k); bad += k != 12; ++tensors;
        bad += check_tensor({0.05f, -0.049f}, &k); bad += k != 17; ++tensors;         // Xavier scale: 0.05 2^17 = 6553.6
        bad += check_tensor({3.0e38f, 1.f}, &k); bad += k != -F16S_K_MAX; ++tensors;  // 13 - 128 cut off at -100: saturated, finite planes
        bad += check_tensor({f16s_float(1u), f16s_float(3u)}, &k); bad += k != F16S_K_MAX; ++tensors;      // denormals only: cut off at +100
        line("planes", bad == 0, "%ld tensors, %ld violations", tensors, bad);
    }
    // the sibling list: every (ADD, RELU) the fp32 forward can ask of the 8-phase kernel has a sibling, nothing else has
    {
        long with = 0, without = 0, bad = 0;
        GemmArgs a;
        for (int v = -1; v <= kGemmP8Count; ++v) {
            for (int f16s = 0; f16s < 2; ++f16s) {
                a.f16s = f16s;
                const int s = gemm_p8s_pick(a, v);
                const bool row = v >= 0 && v < kGemmP8Count;
                const bool want = f16s && row && kGemmP8Variants[v].mode == 1 && kGemmP8Variants[v].abl == 0;
                if (want) {
                    ++with;
                    bad += s < 0 || s >= kGemmP8sCount || kGemmP8sVariants[s].add != kGemmP8Variants[v].add || kGemmP8sVariants[s].relu != kGemmP8Variants[v].relu;
                } else {
                    ++without;
                    bad += s != -1;
                }
            }
        }
        bool seen[kGemmP8sCount] = {};
        for (int v = 0; v < kGemmP8Count; ++v) { a.f16s = 1; const int s = gemm_p8s_pick(a, v); if (s >= 0) { bad += seen[s]; seen[s] = true; } }
        for (bool s : seen) bad += !s;                                              // no sibling without a MODE 1 row
        int mode1 = 0;
        for (int v = 0; v < kGemmP8Count; ++v) mode1 += kGemmP8Variants[v].mode == 1 && kGemmP8Variants[v].abl == 0;
        bad += mode1 != kGemmP8sCount || kGemmP8sCount != 5;
        line("siblings", bad == 0 && with == 5, "%ld rows with a sibling, %ld picks without", with, without);
    }
    // the planner answers the same with and without f16s, and refuses f16s next to another precision or without planes
    {
        long bad = 0, n = 0;
        alignas(16) static float dummy[4];
        alignas(16) static uint16_t planes[16];
        for (int M : {300, 801, 16384, 16929, 70000})
            for (int N : {256, 512, 1024})
                for (int K : {128, 512, 1024})
                    for (int part : {0, 1}) {
                        GemmArgs a;
                        a.A = dummy; a.W = dummy; a.C = dummy; a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N; a.p8_part_min = part;
                        GemmArgs b = a;
                        b.f16s = 1; b.Wh16 = planes; b.Wl16 = planes; b.w_exp = 17;
                        const GemmPlan p = plan_gemm(a, 512), q = plan_gemm(b, 512);
                        bad += gemm_invalid(b) != nullptr || !same_plan(p, q) || p.variant != q.variant;
                        ++n;
                    }
        GemmArgs a;
        a.A = dummy; a.W = dummy; a.C = dummy; a.M = 801; a.N = 256; a.K = 128; a.lda = 128; a.ldw = 128; a.ldc = 256; a.f16s = 1;
        bad += gemm_invalid(a) == nullptr;                     // no planes
        a.Wh16 = planes; a.Wl16 = planes;
        bad += gemm_invalid(a) != nullptr;
        a.w_exp = 101; bad += gemm_invalid(a) == nullptr; a.w_exp = 0;
        a.prec = 3; a.Whi = planes; a.Wlo = planes; bad += gemm_invalid(a) == nullptr;
        line("planner", bad == 0, "%ld plans compared, %ld wrong", n, bad);
    }
    return fails ? 1 : 0;
}
