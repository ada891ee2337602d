// Edge cross-attention core on the bf16 matrix cores (BASELINE configs[2]): the same flash-style kernel as
// flash_attn_f32.hip -- reference transformer/attention.py:60-76 as called from network_MMG.py:231, scores never
// leave registers -- with QK^T and PV on v_mfma_f32_32x32x16_bf16 (16x the fp32-MFMA rate) and fp32 softmax.
//
// TERMS = 3 (split-bf16, ~1e-5): every operand x is carried as bf16 hi + bf16 lo (x ~= hi + lo to 2^-17) and each
// product is three MFMAs  a_lo.b_hi + a_hi.b_lo + a_hi.b_hi  (small terms first), fp32 accumulate.
// TERMS = 1 (single rounding): hi parts only.
//
// Q, K, V arrive as fp32 (the projection GEMMs' outputs) and are split while staging: Q once per block into registers
// (pre-multiplied by scale*log2 e), K/V per key tile into LDS planes.
//   block   = 128 queries (4 waves x 32), key tiles of 64, double-buffered LDS, one barrier per tile;
//   S^T     = K_tile . Q^T  : A = K rows from LDS (ds_read_b128: 8 consecutive d, row pitch 144 B = conflict-free),
//             B = Q from registers; "swapped" product so a lane owns ONE query column: the softmax row reductions
//             are in-lane plus one lane^32 shuffle;
//   O^T    += V^T . P^T     : B = P straight from the S registers -- the k-slot (half hi, element e) of step j is key
//             32(j>>1) + 16(j&1) + 8(e>>2) + 4 hi + (e&3), i.e. exactly the keys registers 8(j&1)+e already hold, so P
//             needs no cross-lane movement; A = V^T[d][those keys] read from the ROW-major V tile with the gfx950
//             LDS transpose read ds_read_b64_tr_b16 (two reads of 4 keys x 16 d per operand).  The V image is
//             4 sub-tiles [64 keys][16 d] (32-byte rows) 2176 B apart, so the two 16-lane groups of a half-wave land
//             on disjoint bank halves (semantics and bank behaviour: tools/tr_read_probe.hip).
//   TR = false keeps a gather fallback for the V operand (eight ds_read_u16 per operand) -- the reference
//   implementation the transpose-read path is tested against.
// Split keys (plans that cannot fill the chip) and the output transpose through LDS are as in flash_attn_f32.hip.
// The kernel's text is flash_attn_16bit_kernel.h, compiled under two names: flash_attn_bf16_kernel (everything above) and
// flash_attn_f16x3_kernel, the TERMS = 3 form on fp16 hi / lo planes and v_mfma_f32_32x32x16_f16 (x ~= hi + lo to 2^-22: the edge
// attention of the fp32 precision mode, fp32 tensors in and out).
// Which instantiations exist and which one a launch gets: flash_pick.h; what each template argument does: the comment above the kernel.
// Roofline: bf16 MFMA, 2.5 PF / TERMS; algorithmic work 4*T^2*64 flop per (scene, head).
#include <type_traits>

#include "gemm_core.h"
#include "kernels.h"

namespace vlsat {

namespace {

constexpr int FB_KV = 64;              // keys per tile
constexpr int FB_VSUB = FB_KV * 32 + 128;                     // 2176: one [64 keys][16 d] sub-tile + half a bank row
// FB_D (template): head dim = 512 / MODEL.NUM_HEADS: 64 as shipped, 32 or 128 for 16 / 4 heads (round 3).  It sets the number
// of 16-wide k-steps of QK^T (FB_D / 16), of 32-wide output blocks (FB_D / 32) and of V sub-tiles (FB_D / 16); K rows are
// 2 FB_D + 16 bytes apart (80 / 144 / 272: every 16-lane group of a ds_read_b128 lands on 16 different 4-bank groups).

typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int N> __device__ __forceinline__ void fb_wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
// max of three without the canonicalising v_max hipcc puts in front of an fmaxf on MFMA results
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// packed fp32 pairs: one full-rate VALU instruction for two values.  Inline asm is invisible to hipcc's hazard recogniser: on
// gfx950 a VALU instruction that reads the result of a transcendental one (v_exp_f32) needs a wait state in between, which the
// compiler inserts only before instructions it knows to be VALU -- hence the s_nop in front of the add that takes the exponentials
// (found by the kernel tests: without it the row sums used stale registers).
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
    f32x2 d;
    asm("s_nop 0\n\tv_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, float m) {      // {a.x - m, a.y - m}
    f32x2 d;
    const f32x2 mm = {m, m};
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(mm));
    return d;
}

__device__ __forceinline__ void split4(const f32x4& x, bf16x4& hi, bf16x4& lo) {
    hi = __builtin_convertvector(x, bf16x4);
    lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x4), bf16x4);
}
// split-fp16 (X3): hi = fp16(x) round-to-nearest, lo = fp16(x - hi), in registers declared bf16x4 (mfma_h reinterprets the bits).
// x ~= hi + lo to 2^-22 while lo is a normal fp16 (|x| >= 2^-3; the kernel pre-scales V and P for that: VS, PBIAS).  CLAMP: the
// tensor operands are clamped to the fp16 range first, like the other fp16 paths (probabilities lie in [0, 1] and need none).
template <bool CLAMP>
__device__ __forceinline__ void split4h(f32x4 x, bf16x4& hi, bf16x4& lo) {
    typedef _Float16 f16x4_s __attribute__((ext_vector_type(4)));
    if (CLAMP) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = __builtin_amdgcn_fmed3f(x[c], -65504.f, 65504.f);
    }
    const f16x4_s h = __builtin_convertvector(x, f16x4_s);
    hi = __builtin_bit_cast(bf16x4, h);
    lo = __builtin_bit_cast(bf16x4, __builtin_convertvector(x - __builtin_convertvector(h, f32x4), f16x4_s));
}
// four elements of an operand tensor -> bf16 hi / lo.  IO_S: the tensor is in the split-pair format (common.h
// pack_split; written by the projection GEMMs' epilogues in the bf16 modes), so this is two v_perm_b32 per plane
template <int IO>
__device__ __forceinline__ void planes4(const f32x4& x, bf16x4& hi, bf16x4& lo) {
    if (IO == 1) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x4 w = __builtin_bit_cast(u32x4, x);
        u32x2 h, l;
        h[0] = __builtin_amdgcn_perm(w[1], w[0], 0x07060302u); h[1] = __builtin_amdgcn_perm(w[3], w[2], 0x07060302u);
        l[0] = __builtin_amdgcn_perm(w[1], w[0], 0x05040100u); l[1] = __builtin_amdgcn_perm(w[3], w[2], 0x05040100u);
        hi = __builtin_bit_cast(bf16x4, h);
        lo = __builtin_bit_cast(bf16x4, l);
    } else {
        split4(x, hi, lo);
    }
}

// four consecutive elements of a row, whatever the tensor format: IO = 0 fp32, 1 split-pair words (16 bytes each way),
// 2 half rows (8 bytes: four bf16, returned in the low half of the f32x4)
template <int IO>
__device__ __forceinline__ f32x4 load4(const float* row, size_t col) {
    if (IO >= 2) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 v = *reinterpret_cast<const f32x2*>(reinterpret_cast<const char*>(row) + col * 2);
        return f32x4{v[0], v[1], 0.f, 0.f};
    }
    return *reinterpret_cast<const f32x4*>(row + col);
}
template <int IO, bool X3 = false>
__device__ __forceinline__ void planes_of(const f32x4& x, bf16x4& hi, bf16x4& lo) {
    if (X3) {
        split4h<true>(x, hi, lo);
    } else if (IO >= 2) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        hi = __builtin_bit_cast(bf16x4, f32x2{x[0], x[1]});
        lo = hi;                                   // (never read: TERMS = 1)
    } else {
        planes4<IO>(x, hi, lo);
    }
}

// IO = 1 / 2: Q, K, V arrive and O leaves in the split-pair / half-row format; Q is then already multiplied by
// scale * log2 e (the projection GEMM's epilogue did it)
// PVT (split-bf16 mode only): MFMAs per P.V product.  3 = V_hi.P_hi + V_lo.P_hi + V_hi.P_lo; 2 drops the last term, i.e. the
// probabilities enter the second product single-rounded (V stays exact) -- an experiment switch (flash_pv_terms).
// DMA (round 4; half rows, single rounding, head dim 64): K / V tiles arrive by LDS-direct loads (buffer_load ... lds, no VGPR
// round trip, no ds_write) into a ring of RING tile buffers (2 as shipped: one tile ahead, four blocks per CU), RING - 1 tiles
// ahead of the one being computed, with counted s_waitcnt vmcnt and a raw s_barrier per tile.  Measured before: with the staging loads switched off the kernel ran 28 %
// faster, with the LDS stores off as well 43 % (profiles/r04_probes/flash_bf16_staging_ablation.txt) -- one tile of look-ahead
// through registers does not cover an L2 / HBM round trip inside a 0.45 us iteration.  The K image is then 64 rows x 128 B with
// the 16-byte chunks XOR-swizzled by (row >> 1) & 7 on the global side and on the fragment reads (an LDS-direct load writes
// lane-linear, so the 144-byte row pitch of the register-staged image cannot be produced); the V image is unchanged (four
// [64 keys][16 d] sub-tiles: a wave instruction fills 32 keys x 32 B of one of them).
// BQW: waves = 32-query groups per block: 4 (128 queries, the default) or -- LDS-direct staging only -- 8 (256 queries sharing every
// K / V tile: half the L2 -> LDS bytes per query; for scenes of thousands of tokens, whose K / V no longer sit in one XCD's L2 and
// whose last, partly filled query tile is a negligible share: round 5, +4 % at cfg 5)
// ABL (experiments build only, compile-time so that the shipped code generation is what gets timed; results are GARBAGE): 4 no exponentials,
// 8 no maximum, 16 no cross-half exchanges, 32 no P.V MFMAs, 64 no Q.K MFMAs, 256 no barrier per tile
// (round 6, measured and dropped: the V fragments by inline-asm ds_read_b64_tr_b16 with hand-counted lgkmcnt waits, two register sets a
//  16-key chunk apart -- through the builtin, which carries no alias information, hipcc drains vmcnt in front of the first transpose read
//  of an iteration, i.e. a wave waits for the NEXT tile's LDS-direct loads where its P.V product starts.  Bit-identical, 120 VGPRs, still
//  four blocks per CU, no vmcnt wait left inside the iteration: 9844-9894 vs 9822-9870 scenes/s in the cfg 3 step (+0.2 %), 80.4-81.0 vs
//  80.7-81.7 at cfg 5 (-0.7...-1.2 %): with K / V resident in L2 the loads have landed by then, and the fixed read order costs more than
//  the compiler's.  profiles/r06_probes/krot_asmv_step_ab.txt)
// QG (round 6): 32-query groups per WAVE.  2 = a wave owns 64 queries: every K and V fragment it reads from LDS feeds
// two MFMAs (half the fragment reads, address arithmetic, waits and loop control per product), Q and O of both groups stay in
// registers (~200 VGPRs: two waves per SIMD where QG = 1 has four of 120).  A query's arithmetic is the same instruction sequence on
// the same keys in the same order, so the outputs equal QG = 1 BIT FOR BIT (tests/test_hip_round6.py).  Block = BQW waves x 32 QG
// queries: (BQW 2, QG 2) serves the 128-query tile table, (4, 2) the 256-query one.  ORD 1: the P.V product of group 0 is issued
// in front of group 1's softmax (its V fragments are then read twice).
// the kernel text, once per name (flash_attn_16bit_kernel.h): the bf16 list's kernels, and the split-fp16 form of the three-term one
#define VLSAT_FLASH_KERNEL_NAME flash_attn_bf16_kernel
#define VLSAT_FLASH_KERNEL_X3 false
#include "flash_attn_16bit_kernel.h"
#undef VLSAT_FLASH_KERNEL_NAME
#undef VLSAT_FLASH_KERNEL_X3
#define VLSAT_FLASH_KERNEL_NAME flash_attn_f16x3_kernel
#define VLSAT_FLASH_KERNEL_X3 true
#include "flash_attn_16bit_kernel.h"
#undef VLSAT_FLASH_KERNEL_NAME
#undef VLSAT_FLASH_KERNEL_X3

// one kernel pointer per row of the variant list (flash_pick.h), in its order: taking the address is what instantiates a row
typedef void (*FlashKernel)(const float*, const float*, const float*, float*, int, int, int, const int4*, int, float, FlashSplit);
#define VLSAT_FLASH_KERNEL(T, R, S, P, D, G, W, A, Q, O) flash_attn_bf16_kernel<T, R, S, P, D, G, W, A, Q, O>,
constexpr FlashKernel kFlashKernels[] = {VLSAT_FLASH_BF16_VARIANTS(VLSAT_FLASH_KERNEL)};
#undef VLSAT_FLASH_KERNEL
static_assert(sizeof kFlashKernels / sizeof kFlashKernels[0] == kFlashVariantCount, "one kernel per row of the variant list");
#define VLSAT_FLASH_F16X3_KERNEL(R, D) flash_attn_f16x3_kernel<3, R, 0, 3, D>,
constexpr FlashKernel kFlashF16x3Kernels[] = {VLSAT_FLASH_F16X3_VARIANTS(VLSAT_FLASH_F16X3_KERNEL)};
#undef VLSAT_FLASH_F16X3_KERNEL
static_assert(sizeof kFlashF16x3Kernels / sizeof kFlashF16x3Kernels[0] == kFlashF16x3VariantCount, "one kernel per row of the split-fp16 list");
#define VLSAT_FLASH_F16X3_PAIR_KERNEL(R, D, I) flash_attn_f16x3_kernel<3, R, I, 3, D>,
constexpr FlashKernel kFlashF16x3PairKernels[] = {VLSAT_FLASH_F16X3_PAIR_VARIANTS(VLSAT_FLASH_F16X3_PAIR_KERNEL)};
#undef VLSAT_FLASH_F16X3_PAIR_KERNEL
static_assert(sizeof kFlashF16x3PairKernels / sizeof kFlashF16x3PairKernels[0] == kFlashF16x3PairVariantCount, "one kernel per row of the pair-word list");

}  // namespace

int launch_flash_attn_bf16(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo,
                           const int4* tiles, int n_tiles, float scale_log2e, int terms, int use_tr, int io_split,
                           hipStream_t s, const FlashSplit* split, int pv_terms, int head_dim) {
    if (n_tiles <= 0) return 0;
    if ((ldq | ldkv | ldo) & 3) return fail(-1, "flash_attn: leading dims must be multiples of 4");
    FlashSplit sp{};
    if (split && split->parts > 1) {
        sp = *split;
        if (!sp.krange || !sp.o_part || !sp.m_part || !sp.l_part || sp.heads * head_dim > ldo)
            return fail(-1, "flash_attn: incomplete split-key workspace");
    }
    if (split) { sp.ablate = split->ablate; sp.bq = split->bq; sp.rows = split->rows; sp.qg = split->qg; }
    // (FlashSplit::rows: the rows of the whole tensor, an upper bound of any scene and of the batch-wide attention of batch_mode 'reference')
    const bool rows_fit_32bit = split && split->rows > 0 && (size_t)split->rows * (size_t)ldkv * 4 < (1ull << 32);
    const FlashPick pick = flash_bf16_pick(head_dim, terms, use_tr, io_split, pv_terms, sp.bq, sp.qg, sp.parts, rows_fit_32bit, sp.ablate);
    if (pick.index < 0) return fail(-1, pick.error);
    hipLaunchKernelGGL(kFlashKernels[pick.index], dim3(n_tiles), dim3(64 * kFlashVariants[pick.index].bqw), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
    VLSAT_LAUNCH_CHECK("flash_attn_bf16");
    if (sp.parts > 1) return launch_flash_merge(O, ldo, sp, s, io_split, head_dim);
    return 0;
}

int launch_flash_attn_f16x3(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo,
                            const int4* tiles, int n_tiles, float scale_log2e, int use_tr, hipStream_t s, const FlashSplit* split, int head_dim, int io) {
    if (n_tiles <= 0) return 0;
    if ((ldq | ldkv | ldo) & 3) return fail(-1, "flash_attn: leading dims must be multiples of 4");
    FlashSplit sp{};
    if (split && split->parts > 1) {
        sp = *split;
        if (!sp.krange || !sp.o_part || !sp.m_part || !sp.l_part || sp.heads * head_dim > ldo)
            return fail(-1, "flash_attn: incomplete split-key workspace");
    }
    if (split) { sp.ablate = split->ablate; sp.bq = split->bq; sp.rows = split->rows; sp.qg = split->qg; }
    // io 0: fp32 tensors; 4 | 5: K and V as attention pair words (5: O as GEMM pair words) -- what is not in the lists is an error
    const FlashPick pick = io ? flash_f16x3_pair_pick(head_dim, use_tr, io, sp.parts > 1 ? sp.parts : 1, sp.bq, sp.qg, sp.ablate)
                              : flash_f16x3_pick(head_dim, use_tr, 0, sp.bq, sp.qg, sp.ablate);
    if (pick.index < 0) return fail(-1, pick.error);
    hipLaunchKernelGGL(io ? kFlashF16x3PairKernels[pick.index] : kFlashF16x3Kernels[pick.index], dim3(n_tiles), dim3(256), 0, s, Q, K, V, O, ldq, ldkv, ldo, tiles, n_tiles, scale_log2e, sp);
    VLSAT_LAUNCH_CHECK("flash_attn_f16x3");
    if (sp.parts > 1) return launch_flash_merge(O, ldo, sp, s, 0, head_dim);
    return 0;
}

}  // namespace vlsat
