// The arithmetic of the split-fp16 weight planes of the 8-phase GEMM's fp32-mode sibling (gemm_bf16_p8.hip, gemm_p8s_kernel), stated
// once: the exponent k of a weight tensor and the two fp16 planes  Wh = f16(W 2^k),  Wl = f16(W 2^k - Wh)  of its elements.  No HIP
// header and no _Float16: the device kernel that makes the planes (small_ops.hip) and tests/gemm_f16s_planes_check.cpp (g++) compile the
// same integer code, so both give the same bits.  At the end: the two PAIR-WORD formats in which the fp32 mode's edge activations travel
// between its split-fp16 kernels ("edge_pairs"), stated once for the kernels (gemm_core.h, with the hardware's conversions) and for
// tests/edge_pairs_check.cpp (this integer code).
//
// Why the scale: Wl is a subnormal fp16 (fewer than 11 bits) once |Wh| < 2^-3, and Xavier weights are about 0.05 -- every lo part
// would be one.  With max |W 2^k| in (2^12, 2^13] the lo part of an element keeps its bits down to 2^-16 of the tensor's maximum, and
// Wh 2^-11 (the third operand the kernel makes in registers) is exact for every |Wh| >= 2^-3.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VLSAT_F16S_HD __host__ __device__
#else
#define VLSAT_F16S_HD
#endif

namespace vlsat {

constexpr int F16S_TOP = 13;         // max |W 2^k| <= 2^13
constexpr int F16S_A_SHIFT = 11;     // the lo part of an activation is stored times 2^11 (and meets Wh 2^-11)
constexpr int F16S_K_MAX = 100;      // |k| bound: 2^k and 2^-k stay normal fp32 numbers

VLSAT_F16S_HD inline uint32_t f16s_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
VLSAT_F16S_HD inline float f16s_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// fp32 -> fp16 bits, round to nearest even, subnormals kept, overflow to infinity (IEEE; what v_cvt_f16_f32 gives)
VLSAT_F16S_HD inline uint16_t f16s_to_half(float x) {
    const uint32_t u = f16s_bits(x), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u));
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                       // >= 65520 rounds to infinity
    if (a < 0x33000001u) return (uint16_t)sign;                                    // <= 2^-25 rounds to zero
    const int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;                                      // 24-bit significand
    const int shift = e >= -14 ? 13 : 13 + (-14 - e);                              // bits dropped (subnormal: more)
    const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1);
    m >>= shift;
    if (rest > half || (rest == half && (m & 1))) ++m;
    // normal: m has the hidden bit at 0x400, adding (e + 14) << 10 lets a carry run into the exponent; subnormal: exponent field 0
    return (uint16_t)(sign | (e >= -14 ? (uint32_t)((e + 14) << 10) + m : m));
}
// fp16 bits -> fp32 (exact)
VLSAT_F16S_HD inline float f16s_from_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31) return f16s_float(sign | 0x7f800000u | (m << 13));
    if (e) return f16s_float(sign | ((e + 112) << 23) | (m << 13));
    const float v = (float)m * 5.9604644775390625e-08f;                            // m 2^-24
    return sign ? -v : v;
}

// k = 13 - ceil(log2(max |W|)) from the bits of max |W| (a finite fp32 number >= 0); 0 for an all-zero tensor
VLSAT_F16S_HD inline int f16s_exponent(uint32_t max_abs_bits) {
    const uint32_t a = max_abs_bits & 0x7fffffffu;
    if (a == 0 || a >= 0x7f800000u) return 0;
    int e;                       // a = m 2^e, m in [1, 2)
    uint32_t frac;
    if (a >> 23) { e = (int)(a >> 23) - 127; frac = a & 0x7fffffu; }
    else { int top = 22; while (!((a >> top) & 1)) --top; e = top - 149; frac = a & ((1u << top) - 1); }
    const int k = F16S_TOP - (frac ? e + 1 : e);
    return k > F16S_K_MAX ? F16S_K_MAX : k < -F16S_K_MAX ? -F16S_K_MAX : k;
}
// 2^k, |k| <= F16S_K_MAX
VLSAT_F16S_HD inline float f16s_pow2(int k) { return f16s_float((uint32_t)(k + 127) << 23); }

// the two plane elements of a weight: hi = f16(w 2^k), lo = f16(w 2^k - hi); the product with 2^k and the difference are exact
VLSAT_F16S_HD inline void f16s_split(float w, int k, uint16_t& hi, uint16_t& lo) {
    float x = w * f16s_pow2(k);
    x = x > 65504.f ? 65504.f : x < -65504.f ? -65504.f : x;      // (a k cut off at F16S_K_MAX, or a NaN-free tensor with an infinity: stay finite)
    hi = f16s_to_half(x);
    lo = f16s_to_half(x - f16s_from_half(hi));
}

// ---- activations: the GEMM pair word (fp32 mode, "edge_pairs") ----
// A kernel that reads an fp32 activation x as an A operand splits it into  Ah = f16(xc)  and  Al = f16((xc - Ah) 2^11),  xc = x clamped to
// +-65504 (gemm_p8_kernel.h FS, gemm_core.h f16s_split8).  The split depends on the word alone, so the kernel that WRITES an edge tensor
// whose only readers are such A operands stores the two halves instead of x, one 32-bit word per element:
//     word = Ah << 16 | Al          (Ah: bits 31..16, so the word's sign bit is the sign of x; Al 2^11 as it is used: bits 15..0)
// Same shape, pitch and buffer as the fp32 tensor.  The reader separates the halves of two neighbouring words with two byte permutes
// and applies a pending ReLU as max((int)word, 0): x < 0 <=> Ah < 0 (rounding keeps the sign), and the halves of a clamped-to-zero x are
// both +0.  The difference xc - Ah and its product with 2^11 are exact in fp32; the only roundings are the two conversions to fp16, and
// they are the ones the reader would have made: every MFMA operand is bit for bit what the on-the-fly split gives.
VLSAT_F16S_HD inline float f16s_pair_clamp(float x) { return x > 65504.f ? 65504.f : x < -65504.f ? -65504.f : x; }
VLSAT_F16S_HD inline uint32_t f16s_pair_pack(float x) {
    const float xc = f16s_pair_clamp(x);
    const uint16_t hi = f16s_to_half(xc);
    const uint16_t lo = f16s_to_half((xc - f16s_from_half(hi)) * f16s_pow2(F16S_A_SHIFT));
    return (uint32_t)hi << 16 | lo;
}
VLSAT_F16S_HD inline uint16_t f16s_pair_hi(uint32_t word) { return (uint16_t)(word >> 16); }
VLSAT_F16S_HD inline uint16_t f16s_pair_lo(uint32_t word) { return (uint16_t)(word & 0xffffu); }
// a pending ReLU on a pair word
VLSAT_F16S_HD inline uint32_t f16s_pair_relu(uint32_t word) { return (int32_t)word < 0 ? 0u : word; }
// ---- the ATTENTION pair word: what the split-fp16 edge attention (flash_attn_f16x3_kernel) makes of a K or V element while staging ----
//     word = hi << 16 | lo,   hi = f16(xc),  lo = f16(xc - hi),  xc = x 2^s clamped to +-65504;   s = 0 for K, F16S_V_SHIFT for V
// (split4h<true>; V times 2^3 so that its lo parts are normal fp16 numbers down to |v| = 2^-6 -- the factor leaves with the final 1 / l).
// The key | value projection writes its K columns and its V columns in this format; the attention kernel then separates the halves
// with byte permutes instead of clamping, converting and subtracting every word once per block of 128 queries.
constexpr int F16S_V_SHIFT = 3;
VLSAT_F16S_HD inline uint32_t f16s_attn_pack(float x, int shift) {
    const float xc = f16s_pair_clamp(x * f16s_pow2(shift));
    const uint16_t hi = f16s_to_half(xc);
    const uint16_t lo = f16s_to_half(xc - f16s_from_half(hi));
    return (uint32_t)hi << 16 | lo;
}

}  // namespace vlsat
