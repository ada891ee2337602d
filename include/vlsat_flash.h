/*
 * vlsat_flash.h -- the part of libvlsat_hip.so's C ABI that runs the split-fp16 edge attention on its own (csrc/flash_attn_bf16.hip,
 * flash_attn_f16x3_kernel): the kernel the fp32 precision mode uses for the edge cross-attention at head dim 64, next to
 * vlsat_k_flash_attn (the exact fp32-MFMA kernel) and vlsat_k_flash_attn_bf16 of vlsat.h.  Conventions, error codes and
 * vlsat_last_error() are those of vlsat.h; the symbol is exported from the same library and bound by lib.py from its registry row HEADERS["flash"].
 */
#ifndef VLSAT_FLASH_H
#define VLSAT_FLASH_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The attention of vlsat_k_flash_attn as the fp32 precision mode runs it at head dim 64 (n_heads * 64 <= ld): plain fp32 Q, K, V, O, every operand
 * split into fp16 hi + fp16 lo (2^-22 per operand) and every product issued as three f16 MFMAs with fp32 accumulation and an fp32
 * softmax -- the error of the exact kernel times 0.7 to 2.  Domain: |Q * scale * log2 e|, |K| < 65504, |V| < 8188 (V is
 * multiplied by 2^3 before the split so that its lo parts are normal fp16 numbers down to 2^-6; values beyond are clamped).  use_tr = 1 reads the V operand with the LDS transpose read, 0 gathers it (same bits).  key_parts > 1 runs the
 * split-key path: every scene's keys in key_parts parts (of 32-key tiles, empty parts included) and the merge kernel. */
int vlsat_k_flash_attn_f16x3(const float* Q, const float* K, const float* V, float* O,
                             int32_t ld, const int64_t* tok_ptr_host, int32_t n_scenes, int32_t n_heads,
                             float scale, int32_t key_parts, int32_t use_tr, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_FLASH_H */
