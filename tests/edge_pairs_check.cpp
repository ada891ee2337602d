// Host-only check of the fp32 mode's GEMM pair words (csrc/gemm_f16s_planes.h f16s_pair_pack) and of the function that decides which
// edge tensors of a forward carry them (csrc/edge_pairs.h edge_pairs_plan).  g++ only (optionally ASan + UBSan): no HIP header, no
// library, no device.
//   edge_pairs_check                 one line per plan: "<case> -> Hbig3 .. | Hbig2 .. | R1_3 .. | R1_2 .. | E3 .. | Oe .. | KV ..", each tensor
//                                    "pairs" or "fp32 (<reason>)", then "format -> ok ..." and "forms -> ok ..."
//   edge_pairs_check pack <hex>...   the GEMM pair word of each fp32 bit pattern, the word after a pending ReLU and the attention pair words
//                                    of a K and of a V element: "<hex> -> <word> <relu word> <K word> <V word>"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "edge_pairs.h"
#include "gemm_f16s_planes.h"

using namespace vlsat;

// an independent fp16 value -> double and double -> nearest-even fp16 (the definition, not the header's code)
static double half_value(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    const double v = e == 31 ? (m ? NAN : INFINITY) : e ? std::ldexp(1.0 + m / 1024.0, e - 15) : std::ldexp((double)m, -24);
    return (h & 0x8000) ? -v : v;
}
static uint16_t nearest_half(double x) {
    const uint16_t sign = std::signbit(x) ? 0x8000 : 0;
    const double a = std::fabs(x);
    if (a == 0.0) return sign;
    int e;
    std::frexp(a, &e);                                   // a = f 2^e, f in [0.5, 1)
    const int q = (e - 1 < -14 ? -14 : e - 1) - 10;      // exponent of the last kept bit
    const double n = std::nearbyint(std::ldexp(a, -q)); // ties to even (default rounding mode)
    const double v = std::ldexp(n, q);
    if (v >= 65536.0) return sign | 0x7c00;
    if (v < std::ldexp(1.0, -14)) return (uint16_t)(sign | (uint16_t)std::ldexp(v, 24));        // subnormal: v = m 2^-24
    int ev;
    const double f = std::frexp(v, &ev);                 // v = f 2^ev, f in [0.5, 1): 1.m = 2 f, exponent ev - 1
    return (uint16_t)(sign | (uint16_t)(((ev - 1 + 15) << 10) + (int)std::ldexp(2.0 * f - 1.0, 10)));
}

static std::string tensor(const char* name, bool on, const char* why) {
    return std::string(name) + (on ? " pairs" : std::string(" fp32 (") + (why ? why : "?") + ")");
}
static void plan_line(const char* name, const EdgePairsIn& in) {
    const EdgePairs r = edge_pairs_plan(in);
    std::printf("%s -> %s | %s | %s | %s | %s | %s | %s\n", name, tensor("Hbig3", r.hbig[0], r.why_hbig[0]).c_str(),
                tensor("Hbig2", r.hbig[1], r.why_hbig[1]).c_str(), tensor("R1_3", r.r1[0], r.why_r1[0]).c_str(),
                tensor("R1_2", r.r1[1], r.why_r1[1]).c_str(), tensor("E3", r.e3, r.why_e3).c_str(), tensor("Oe", r.oe, r.why_oe).c_str(),
                tensor("KV", r.kv, r.why_kv).c_str());
}

int main(int argc, char** argv) {
    if (argc > 2 && !std::strcmp(argv[1], "pack")) {
        for (int i = 2; i < argc; ++i) {
            const uint32_t bits = (uint32_t)std::strtoul(argv[i], nullptr, 16);
            const uint32_t w = f16s_pair_pack(f16s_float(bits));
            std::printf("%08x -> %08x %08x %08x %08x\n", bits, w, f16s_pair_relu(w), f16s_attn_pack(f16s_float(bits), 0),
                        f16s_attn_pack(f16s_float(bits), F16S_V_SHIFT));
        }
        return 0;
    }
    // ---- which tensors pair, per plan ----
    EdgePairsIn bench;                                   // the bench batch: 64 scenes x 40 objects, 256 CUs
    bench.E = 64 * 40 * 39; bench.G = 512;
    plan_line("bench batch, 256 CUs", bench);
    { EdgePairsIn in = bench; in.option = 0; plan_line("bench batch, edge_pairs 0", in); }
    { EdgePairsIn in = bench; in.gemm_exact = true; plan_line("bench batch, gemm_exact 1", in); }
    { EdgePairsIn in = bench; in.gemm_small_exact = true; plan_line("bench batch, gemm_small_exact 1", in); }
    { EdgePairsIn in = bench; in.fp32_mode = false; plan_line("bench batch, a bf16 mode", in); }
    { EdgePairsIn in = bench; in.feature_transform = true; plan_line("bench batch, feature_transform", in); }
    { EdgePairsIn in = bench; in.train = true; plan_line("bench batch, training outputs", in); }
    { EdgePairsIn in = bench; in.debug_stop = 12; plan_line("bench batch, debug stop", in); }
    { EdgePairsIn in = bench; in.prob_tap = true; plan_line("bench batch, probability tap", in); }
    { EdgePairsIn in = bench; in.do2d = false; plan_line("bench batch, 3D only", in); }
    { EdgePairsIn in = bench; in.no_dma = true; plan_line("bench batch, gemm_dma 0", in); }
    { EdgePairsIn in = bench; in.no_p8 = true; plan_line("bench batch, gemm_p8 0", in); }
    { EdgePairsIn in = bench; in.flash_x3 = false; plan_line("bench batch, flash_exact 1", in); }
    { EdgePairsIn in = bench; in.flash_x3 = false; in.head_dim = 32; plan_line("bench batch, head dim 32", in); }
    { EdgePairsIn in = bench; in.flash_x3 = false; in.head_dim = 128; plan_line("bench batch, head dim 128", in); }
    { EdgePairsIn in = bench; in.head_dim = 128; plan_line("bench batch, head dim 128 asked of the split-fp16 kernel", in); }
    { EdgePairsIn in = bench; in.flash_tr = 0; plan_line("bench batch, flash_tr 0", in); }
    { EdgePairsIn in = bench; in.fa_parts = 4; plan_line("bench batch, four key parts", in); }
    EdgePairsIn small;                                   // 3 scenes x 16 objects
    small.E = 720; small.G = 512;
    plan_line("E = 720", small);
    { EdgePairsIn in = small; in.p8_part_min = 1; plan_line("E = 720, gemm_p8_part_min 1", in); }
    { EdgePairsIn in = small; in.fa_parts = 3; plan_line("E = 720, three key parts", in); }
    { EdgePairsIn in = small; in.splitk = false; plan_line("E = 720, gemm_splitk 0", in); }
    { EdgePairsIn in = small; in.splitk = false; in.p8_part_min = 1; plan_line("E = 720, gemm_p8_part_min 1, gemm_splitk 0", in); }
    { EdgePairsIn in = small; in.E = 5 * 4 + 0 + 7 * 6; plan_line("scenes of 5, 1 and 7 objects (E = 62)", in); }
    { EdgePairsIn in = small; in.E = 0; plan_line("E = 0", in); }
    { EdgePairsIn in = small; in.E = 72; in.paired = true; plan_line("one scene of 9 objects, paired schedule", in); }
    { EdgePairsIn in = small; in.E = 72; plan_line("one scene of 9 objects, pair_twins 0", in); }
    { EdgePairsIn in; in.E = 200 * 199; in.G = 512; plan_line("one scene of 200 objects", in); }

    // ---- the format: the header's integer code against the definition ----
    {
        long n = 0, bad = 0;
        uint32_t state = 777u;
        auto check = [&](float x) {
            if (std::isnan(x)) return;
            const uint32_t w = f16s_pair_pack(x);
            const double xc = x > 65504.f ? 65504.0 : x < -65504.f ? -65504.0 : (double)x;
            const uint16_t hi = nearest_half(xc);
            const uint16_t lo = nearest_half((xc - half_value(hi)) * 2048.0);
            bad += f16s_pair_hi(w) != hi || f16s_pair_lo(w) != lo;
            bad += (hi & 0x7c00) == 0x7c00 || (lo & 0x7c00) == 0x7c00;                           // nothing infinite
            bad += ((w >> 31) != 0) != std::signbit(x);                                          // the word's sign bit is the sign of x
            // a pending ReLU on the word: the word of max(x, 0) (the halves of zero are both +0)
            bad += f16s_pair_relu(w) != (x > 0.f ? w : 0u);
            bad += x > 0.f && f16s_pair_pack(x < 0.f ? 0.f : x) != f16s_pair_relu(w);
            // hi + lo 2^-11 within 2^-22 of x (lo parts below fp16's normal range: half a subnormal ulp of the scaled lo)
            const double back = half_value(hi) + half_value(lo) / 2048.0;
            bad += std::fabs(back - xc) > std::ldexp(std::fabs(xc), -22) + std::ldexp(1.0, -25 - 11);
            ++n;
        };
        for (float x : {0.f, -0.f, 1.f, -1.f, 65504.f, -65504.f, 65519.9f, 65520.f, 1e9f, -1e9f, INFINITY, -INFINITY, 6.1e-5f, -6.1e-5f,
                        1.2207031e-4f, 1.2e-4f, 5.96e-8f, 2.9e-8f, 3.0e-8f, 1e-12f, -1e-12f, 1e-40f, 1234.5678f, -4097.3f, 0.33333334f})
            check(x);
        for (int i = 0; i < 300000; ++i) {
            state = state * 1664525u + 1013904223u;
            check(f16s_float(state));
        }
        for (int i = 0; i < 100000; ++i) {                // the values the forward has: |x| up to a few thousand, and around 2^-13
            state = state * 1664525u + 1013904223u;
            const float u = (float)((state >> 8) * (1.0 / 16777216.0)) * 2.f - 1.f;
            check(u * 4000.f);
            check(u * 2.5e-4f);
        }
        // the attention pair word: hi = f16(xc), lo = f16(xc - hi), xc = x 2^s clamped
        auto check_attn = [&](float x, int shift) {
            if (std::isnan(x)) return;
            const uint32_t w = f16s_attn_pack(x, shift);
            const double xs = std::ldexp((double)x, shift), xc = xs > 65504.0 ? 65504.0 : xs < -65504.0 ? -65504.0 : xs;
            if (std::fabs(xs) > 3e38) return;                                    // (x 2^s overflows fp32: outside the kernel's domain as well)
            const uint16_t hi = nearest_half(xc), lo = nearest_half(xc - half_value(hi));
            bad += (uint16_t)(w >> 16) != hi || (uint16_t)(w & 0xffff) != lo || (hi & 0x7c00) == 0x7c00 || (lo & 0x7c00) == 0x7c00;
            ++n;
        };
        for (int i = 0; i < 100000; ++i) {
            state = state * 1664525u + 1013904223u;
            const float u = (float)((state >> 8) * (1.0 / 16777216.0)) * 2.f - 1.f;
            for (int shift : {0, F16S_V_SHIFT}) { check_attn(f16s_float(state), shift); check_attn(u * 3000.f, shift); check_attn(u * 0.02f, shift); }
        }
        for (float x : {0.f, -0.f, 8188.f, 8189.f, -8190.f, 65504.f, 7e4f, -7e4f, 0.015625f, 0.0156f, 1e-6f, -1e-9f})
            for (int shift : {0, F16S_V_SHIFT}) check_attn(x, shift);
        bad += f16s_pair_pack(-0.f) != 0x80000000u || f16s_pair_relu(f16s_pair_pack(-0.f)) != 0u || f16s_pair_pack(0.f) != 0u;
        std::printf("format -> %s %ld values, %ld wrong\n", bad ? "FAILED" : "ok", n, bad);
        if (bad) return 1;
    }
    // ---- every pair form a forward can ask of the 8-phase sibling is in its list, and nothing is there twice ----
    {
        long bad = 0;
        for (int i = 0; i < kGemmP8sPairCount; ++i) {
            const GemmP8sPairVariant& v = kGemmP8sPairVariants[i];
            bad += gemm_p8s_pair_find(v.add, v.relu, v.pf) != i || gemm_p8s_find(v.add, v.relu) < 0 || !(v.pf == 1 || v.pf == 2 || v.pf == 4 || v.pf == 5 || v.pf == 6);
        }
        for (int relu = 0; relu < 2; ++relu) {
            for (int pf : {1, 4, 5}) bad += gemm_p8s_pair_find(0, relu != 0, pf) < 0;
            for (int pf : {1, 5}) bad += gemm_p8s_pair_find(6, relu != 0, pf) < 0;
        }
        bad += gemm_p8s_pair_find(0, false, 2) < 0 || gemm_p8s_pair_find(0, false, 6) < 0 || gemm_p8s_pair_find(1, false, 4) < 0;
        bad += gemm_pair_form(0, 2) != 2 || gemm_pair_form(1, 2) != 6 || gemm_f16s_pair_prec(0, 2) != 21 || gemm_f16s_pair_prec(1, 2) != 22;
        bad += !gemm_f16s_pair_built(0, 21) || !gemm_f16s_pair_built(0, 22) || gemm_f16s_pair_built(1, 21) || gemm_f16s_pair_built(6, 22) || !gemm_f16s_pair_built(6, 20);
        bad += flash_f16x3_pair_pick(64, 1, 4).index < 0 || flash_f16x3_pair_pick(64, 0, 5).index < 0 || flash_f16x3_pair_pick(64, 1, 5, 2).index >= 0 ||
               flash_f16x3_pair_pick(32, 1, 4).index >= 0 || flash_f16x3_pair_pick(64, 1, 3).index >= 0 || flash_f16x3_pair_pick(64, 1, 4, 2).index < 0;
        bad += gemm_pair_form(0, 0) != 0 || gemm_pair_form(1, 0) != 4 || gemm_pair_form(0, 1) != 1 || gemm_pair_form(1, 1) != 5;
        bad += gemm_f16s_pair_prec(0, 1) != 18 || gemm_f16s_pair_prec(1, 0) != 19 || gemm_f16s_pair_prec(1, 1) != 20;
        std::printf("forms -> %s %d rows, %ld wrong\n", bad ? "FAILED" : "ok", kGemmP8sPairCount, bad);
        if (bad) return 1;
    }
    return 0;
}
