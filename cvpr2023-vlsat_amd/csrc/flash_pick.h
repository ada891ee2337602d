// Which instantiation of flash_attn_bf16_kernel (flash_attn_bf16.hip) a launch gets: the list of the instantiations that are built and
// the one function that picks among them.  No HIP header: tests/flash_pick_check.cpp compiles this with g++.  flash_bf16_pick works out
// the ten template arguments a call asks for and looks them up, so what is not in the list is an error, never another kernel; the
// kernel's static_asserts state the same rules on the device side, and a row that breaks them does not compile.
// The split-fp16 form of the three-term kernel (flash_attn_f16x3_kernel) has a list and a pick function of its own at the end.
#pragma once

namespace vlsat {

constexpr int FLASH_BQ = 128;       // queries per block
constexpr int FLASH_BQ_BIG = 256;   // ... of the tile table for scenes of thousands of tokens (FlashSplit::bq)

struct FlashVariant {               // the kernel's template arguments, in its order (what each one does: the comment above the kernel)
    int terms; bool tr; int io, pvt, d, ring, bqw, abl, qg, ord;
    constexpr bool operator==(const FlashVariant& o) const {
        return terms == o.terms && tr == o.tr && io == o.io && pvt == o.pvt && d == o.d && ring == o.ring && bqw == o.bqw && abl == o.abl && qg == o.qg && ord == o.ord;
    }
};

// X(TERMS, TR, IO, PVT, FB_D, RING, BQW, ABL, QG, ORD), one row per instantiation: flash_attn_bf16.hip makes its table of kernel pointers
// from this list (which is what instantiates them), kFlashVariants below has the same rows at the same indices.
// By line: fp32 tensors | split pairs at head dim 64, 32, 128 | bf16 half rows, register-staged and LDS-direct | the same with eight
// waves (256-query tiles) and with 64 queries per wave (BQW 2 | 4 on 128- | 256-query tiles, ORD = flash_qg - 1) | fp16 half rows.
#define VLSAT_FLASH_BF16_RELEASE(X)                                                                                                              \
    X(3, true, 0, 3, 64, 0, 4, 0, 1, 0) X(3, false, 0, 3, 64, 0, 4, 0, 1, 0) X(1, true, 0, 3, 64, 0, 4, 0, 1, 0) X(1, false, 0, 3, 64, 0, 4, 0, 1, 0) \
    X(3, true, 1, 3, 64, 0, 4, 0, 1, 0) X(3, true, 1, 2, 64, 0, 4, 0, 1, 0)  X(1, true, 1, 3, 64, 0, 4, 0, 1, 0)                                 \
    X(3, true, 1, 3, 32, 0, 4, 0, 1, 0) X(3, true, 1, 2, 32, 0, 4, 0, 1, 0)  X(1, true, 1, 3, 32, 0, 4, 0, 1, 0) X(1, true, 1, 3, 128, 0, 4, 0, 1, 0) \
    X(1, true, 2, 3, 64, 0, 4, 0, 1, 0) X(1, true, 2, 3, 32, 0, 4, 0, 1, 0)  X(1, true, 2, 3, 128, 0, 4, 0, 1, 0)                                \
    X(1, true, 2, 3, 64, 2, 4, 0, 1, 0) X(1, true, 2, 3, 32, 2, 4, 0, 1, 0)  X(1, true, 2, 3, 128, 2, 4, 0, 1, 0)                                \
    X(1, true, 2, 3, 64, 2, 8, 0, 1, 0) X(1, true, 2, 3, 64, 2, 2, 0, 2, 0)  X(1, true, 2, 3, 64, 2, 2, 0, 2, 1) X(1, true, 2, 3, 64, 2, 4, 0, 2, 0) X(1, true, 2, 3, 64, 2, 4, 0, 2, 1) \
    X(1, true, 3, 3, 64, 2, 4, 0, 1, 0) X(1, true, 3, 3, 32, 2, 4, 0, 1, 0)  X(1, true, 3, 3, 128, 2, 4, 0, 1, 0) X(1, true, 3, 3, 64, 2, 8, 0, 1, 0)
// Experiments build only (common.h), bf16 half rows at head dim 64: rings of 3 and 4 tile buffers ("flash_dma" 3 | 4), and the timing
// ablations of the eight-wave kernel (ABL = FlashSplit::ablate without its bits 0, 1; results are GARBAGE).  The rings, measured on one
// box, interleaved (profiles/r04_probes/flash_bf16_dma_ab.txt): register-staged 596 TFLOP/s; ring of 3 (3 blocks per CU) 745-773; ring of 4
// (2 blocks per CU) 650-659; ring of 2 with FOUR blocks per CU (34 KB of LDS, 120 VGPRs) 813-817: occupancy beats look-ahead depth.
#ifdef VLSAT_EXPERIMENTS
#define VLSAT_FLASH_BF16_LAB(X)                                                                                                                  \
    X(1, true, 2, 3, 64, 3, 4, 0, 1, 0)  X(1, true, 2, 3, 64, 4, 4, 0, 1, 0)  X(1, true, 2, 3, 64, 2, 8, 4, 1, 0)   X(1, true, 2, 3, 64, 2, 8, 8, 1, 0)   \
    X(1, true, 2, 3, 64, 2, 8, 16, 1, 0) X(1, true, 2, 3, 64, 2, 8, 28, 1, 0) X(1, true, 2, 3, 64, 2, 8, 32, 1, 0)  X(1, true, 2, 3, 64, 2, 8, 64, 1, 0)  \
    X(1, true, 2, 3, 64, 2, 8, 96, 1, 0) X(1, true, 2, 3, 64, 2, 8, 256, 1, 0) X(1, true, 2, 3, 64, 2, 8, 124, 1, 0) X(1, true, 2, 3, 64, 2, 8, 380, 1, 0)
constexpr bool kFlashLab = true;
#else
#define VLSAT_FLASH_BF16_LAB(X)
constexpr bool kFlashLab = false;
#endif
#define VLSAT_FLASH_BF16_VARIANTS(X) VLSAT_FLASH_BF16_RELEASE(X) VLSAT_FLASH_BF16_LAB(X)

#define VLSAT_FLASH_ROW(T, R, S, P, D, G, W, A, Q, O) {T, R, S, P, D, G, W, A, Q, O},
constexpr FlashVariant kFlashVariants[] = {VLSAT_FLASH_BF16_VARIANTS(VLSAT_FLASH_ROW)};
#undef VLSAT_FLASH_ROW
constexpr int kFlashVariantCount = (int)(sizeof kFlashVariants / sizeof kFlashVariants[0]);

constexpr int flash_bf16_find(const FlashVariant& v) {
    for (int i = 0; i < kFlashVariantCount; ++i)
        if (kFlashVariants[i] == v) return i;
    return -1;
}

struct FlashPick { int index; const char* error; };      // a row of kFlashVariants, or -1 and why

// The kernel for head dim d; terms 1 | 3 (single rounding | split-bf16); use_tr 0 gather fallback | 1 transpose read, and LDS-direct K / V
// staging where the format has it | 2 transpose read, register-staged | 3, 4 (experiments build) rings of 3 / 4; io 0 fp32 | 1 split pairs |
// 2 bf16 half rows | 3 fp16 half rows; pv_terms (split-bf16 on split pairs) 3 | 2; bq, qg, ablate as in FlashSplit; parts > 1: split keys.
// rows_fit_32bit: the caller has stated the rows of the tensors (FlashSplit::rows) and they span less than 4 GiB -- the LDS-direct staging
// addresses a scene with 32-bit byte offsets (buffer descriptor of n_tok * ldkv * 4 bytes, row * ld4 VGPR offsets).
inline FlashPick flash_bf16_pick(int d, int terms, int use_tr, int io, int pv_terms = 3, int bq = FLASH_BQ, int qg = 0, int parts = 1,
                                 bool rows_fit_32bit = true, int ablate = 0) {
    const bool big = bq == FLASH_BQ_BIG;
    // head dims other than 64 exist for the tensor formats of the bf16 modes only (transpose read), and split-bf16 not at 128
    if (d != 64 && !((d == 32 || d == 128) && use_tr && io && (io < 2 || terms == 1) && (d == 32 || terms == 1)))
        return {-1, "flash_attn_bf16: head dim / format combination not built"};
    if (terms != 1 && terms != 3) return {-1, "flash_attn_bf16: terms must be 1 or 3"};
    if (io == 3 && !rows_fit_32bit)
        return {-1, "flash_attn_bf16: fp16 half rows are built for scenes addressable with 32-bit offsets (the LDS-direct kernel)"};
    if (bq != FLASH_BQ && !(big && d == 64 && io >= 2 && use_tr == 1 && parts <= 1 && rows_fit_32bit))
        return {-1, "flash_attn_bf16: 256-query tiles are built for half rows, head dim 64, the LDS-direct kernel, no key split"};
    if (io == 2 && use_tr && !rows_fit_32bit) use_tr = 2;      // unknown or larger: the register-staged kernel, which addresses rows with size_t
    FlashVariant v{terms, use_tr != 0, io, 3, d, 0, big ? 8 : 4, 0, 1, 0};
    if (io == 3) {
        if (!use_tr || terms != 1 || use_tr == 2 || (d == 64 && use_tr >= 3))
            return {-1, "flash_attn_bf16: fp16 half rows are built for the LDS-direct single-rounding kernel only"};
        v.ring = 2;
    } else if (io == 2) {
        if (!use_tr || terms != 1) return {-1, "flash_attn_bf16: half-row tensors need terms = 1 and the transpose-read path"};
        const int abl = ablate & ~3;
        v.ring = use_tr == 2 ? 0 : (kFlashLab && d == 64 && (use_tr == 3 || use_tr == 4)) ? use_tr : 2;
        if (v.ring == 2 && d == 64) {          // the forms of the shipped kernel
            if (kFlashLab && big && abl && flash_bf16_find({1, true, 2, 3, 64, 2, 8, abl, 1, 0}) >= 0) {
                v.abl = abl;
            } else if ((qg == 1 || qg == 2) && (big || parts <= 1)) {      // 64 queries per wave
                v.bqw = big ? 4 : 2; v.qg = 2; v.ord = qg - 1;
            }
        }
    } else if (io) {
        if (!use_tr) return {-1, "flash_attn_bf16: the split-pair format is built for the transpose-read path only"};
        v.io = 1;
        v.pvt = terms == 3 && pv_terms == 2 ? 2 : 3;
    }
    const int i = flash_bf16_find(v);
    return i < 0 ? FlashPick{-1, "flash_attn_bf16: head dim / format combination not built"} : FlashPick{i, nullptr};
}

// which (head dim, format) combinations are built: the pick with 128-query tiles, 32 queries per wave, no key split, rows that fit
inline bool flash_attn_bf16_supports(int head_dim, int terms, int use_tr, int io_split) {
    return flash_bf16_pick(head_dim, terms, use_tr, io_split).index >= 0;
}

// ---- the split-fp16 form of the three-term kernel (flash_attn_f16x3_kernel, flash_attn_bf16.hip): the edge attention of the fp32
// precision mode.  fp32 tensors in and out, every operand carried as fp16 hi + fp16 lo (2^-22), three f16 MFMAs per product,
// register-staged K / V, split keys supported.  A list and a pick function of its own: the bf16 list above and flash_bf16_pick stay
// what tests/flash_pick_check.cpp pins them to.  Y(TR, FB_D), one row per instantiation: the transpose read, and the gather form
// the tests hold it against.
#define VLSAT_FLASH_F16X3_VARIANTS(Y) Y(true, 64) Y(false, 64)

struct FlashF16x3Variant {
    bool tr; int d;
    constexpr bool operator==(const FlashF16x3Variant& o) const { return tr == o.tr && d == o.d; }
};
#define VLSAT_FLASH_F16X3_ROW(R, D) {R, D},
constexpr FlashF16x3Variant kFlashF16x3Variants[] = {VLSAT_FLASH_F16X3_VARIANTS(VLSAT_FLASH_F16X3_ROW)};
#undef VLSAT_FLASH_F16X3_ROW
constexpr int kFlashF16x3VariantCount = (int)(sizeof kFlashF16x3Variants / sizeof kFlashF16x3Variants[0]);

// The split-fp16 kernel for head dim d; use_tr 0 gather | 1 transpose read; io 0 (fp32 tensors: the only format); bq, qg, ablate as in
// FlashSplit (128-query tiles, 32 queries per wave, no timing ablation: the only forms).  Split keys need no row of their own.  What
// is not in the list is an error, never another kernel.
inline FlashPick flash_f16x3_pick(int d, int use_tr, int io = 0, int bq = FLASH_BQ, int qg = 0, int ablate = 0) {
    if (io != 0) return {-1, "flash_attn_f16x3: built for fp32 tensors only"};
    if (use_tr != 0 && use_tr != 1) return {-1, "flash_attn_f16x3: use_tr must be 0 (gather) or 1 (transpose read)"};
    if (bq != FLASH_BQ || qg != 0) return {-1, "flash_attn_f16x3: built for 128-query tiles with 32 queries per wave only"};
    if (ablate != 0) return {-1, "flash_attn_f16x3: no timing ablations are built"};
    for (int i = 0; i < kFlashF16x3VariantCount; ++i)
        if (kFlashF16x3Variants[i] == FlashF16x3Variant{use_tr == 1, d}) return {i, nullptr};
    return {-1, "flash_attn_f16x3: head dim not built"};
}
inline bool flash_f16x3_supports(int head_dim, int use_tr) { return flash_f16x3_pick(head_dim, use_tr).index >= 0; }
// ... on pair words (fp32 mode, "edge_pairs"): Z(TR, FB_D, IO) = flash_attn_f16x3_kernel<3, TR, IO, 3, FB_D>, IO 4: K and V arrive as attention
// pair words (gemm_f16s_planes.h), 5: and O leaves as GEMM pair words.  A list and a pick of their own: flash_f16x3_pick stays what
// tests/flash_f16x3_pick_check.cpp pins it to.
#define VLSAT_FLASH_F16X3_PAIR_VARIANTS(Z) Z(true, 64, 4) Z(true, 64, 5) Z(false, 64, 4) Z(false, 64, 5)
struct FlashF16x3PairVariant { bool tr; int d, io; };
#define VLSAT_FLASH_F16X3_ROW(R, D, I) {R, D, I},
constexpr FlashF16x3PairVariant kFlashF16x3PairVariants[] = {VLSAT_FLASH_F16X3_PAIR_VARIANTS(VLSAT_FLASH_F16X3_ROW)};
#undef VLSAT_FLASH_F16X3_ROW
constexpr int kFlashF16x3PairVariantCount = (int)(sizeof kFlashF16x3PairVariants / sizeof kFlashF16x3PairVariants[0]);
// io 4 | 5; parts: key parts of the launch (O as pair words needs one: the merge kernel writes fp32)
inline FlashPick flash_f16x3_pair_pick(int d, int use_tr, int io, int parts = 1, int bq = FLASH_BQ, int qg = 0, int ablate = 0) {
    if (flash_f16x3_pick(d, use_tr, 0, bq, qg, ablate).index < 0) return flash_f16x3_pick(d, use_tr, 0, bq, qg, ablate);
    if (io == 5 && parts > 1) return {-1, "flash_attn_f16x3: O as pair words needs one key part"};
    for (int i = 0; i < kFlashF16x3PairVariantCount; ++i)
        if (const FlashF16x3PairVariant& v = kFlashF16x3PairVariants[i]; v.tr == (use_tr == 1) && v.d == d && v.io == io) return {i, nullptr};
    return {-1, "flash_attn_f16x3: pair-word form not built"};
}

}  // namespace vlsat
