/*
 * vlsat_gemm.h -- the part of libvlsat_hip.so's C ABI that runs the split-fp16 8-phase GEMM on its own (csrc/gemm_bf16_p8.hip,
 * gemm_p8s_kernel): the kernel the fp32 precision mode uses for the full rounds of its large edge-row launches, next to vlsat_k_gemm
 * (always the exact fp32-MFMA kernels) of vlsat.h.  Conventions, error codes and vlsat_last_error() are those of vlsat.h; the symbols
 * are exported from the same library and bound by lib.py from its registry row HEADERS["gemm"].
 */
#ifndef VLSAT_GEMM_H
#define VLSAT_GEMM_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weight planes of that kernel (device pointers, n elements each; csrc/gemm_f16s_planes.h states the arithmetic once):
 *   k = 13 - ceil(log2(max |w|)) (0 for an all-zero tensor, |k| <= 100),  hi[i] = f16(w[i] 2^k),  lo[i] = f16(w[i] 2^k - hi[i]),
 * fp16 bit patterns, round to nearest even.  *k (host) receives the exponent; synchronises `stream`. */
int vlsat_k_split_f16s(const float* w, size_t n, uint16_t* hi, uint16_t* lo, int32_t* k, void* stream);

/* vlsat_k_gemm (same arguments, same contract; relu_a: bit 0 only) as the fp32 precision mode runs an edge-row launch: where the
 * planner sends the launch's full rounds to the 256 x 256 8-phase kernel (N % 256 == 0, K % 128 == 0, K >= 256, no row scale, no sigmoid,
 * additive operands none | residual | both gathered rows, enough tiles: p8_part_min > 0 lowers that bound to so many tiles, 0 keeps the
 * built-in one), those rows run on its split-fp16 sibling: fp32 tensors in and out, every product as three v_mfma_f32_32x32x16_f16 into an
 * fp32 accumulator -- A as fp16 hi + (lo 2^11), the weights as the planes above -- 0.5 to 1 times the exact kernel's error against fp64.
 * Every other row (tail launches, small launches) is the exact kernel's, bit for bit.  W must be dense [N,K] (ldw == K): its planes
 * are made on the spot (allocates, synchronises).
 * p8_part_min = v < 0: the bound is -1 - v (so -1 keeps the built-in one), and the launches of the persistent kernel -- tails, small launches,
 * node rows -- run on ITS split-fp16 siblings as well (gemm_f16s_kernel: same tiles and grids, same arithmetic), as the fp32 mode's forward
 * runs them: N >= 64, additive operands none | residual | both gathered rows, operands within 32-bit byte offsets; anything else, and every
 * split-K launch, stays the exact kernel's, bit for bit.
 * Domain: |A| <= 65504 -- beyond, the operand saturates at +-65504 and results stay finite (no Inf or NaN from finite input);
 * weights below 2^-16 of their tensor's largest lose low bits. */
int vlsat_k_gemm_f16s(const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc, int32_t M, int32_t N,
                      int32_t K, const float* bias, const float* rowscale, const float* resid, int32_t ldr, float resid_scale,
                      const float* g0, const int32_t* gi0, int32_t ldg0, const float* g1, const int32_t* gi1, int32_t ldg1,
                      int32_t relu_a, int32_t act, int32_t p8_part_min, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_GEMM_H */
