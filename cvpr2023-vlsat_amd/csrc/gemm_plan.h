// Which GEMM kernels a launch gets: the lists of the instantiations that are built -- one per family: 8-phase (gemm_bf16_p8.hip), ring
// (gemm_bf16_ring.hip), persistent (gemm_f32.hip), split-K (gemm_splitk.hip) -- one predicate per family from a launch's operands to a row
// of its list, and the planner that uses them (plan_gemm, gemm_pair_plan).  No HIP header: tests/gemm_plan_check.cpp compiles this with
// g++ and pins every decision.  The .hip files make their tables of kernel pointers from the lists (which is what instantiates the
// kernels) and launch table[plan.variant]; what is not in a list is never launched.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace vlsat {

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2 };
// C[M,N] = act(rowscale[m]*(reluA?(A) . W^T) + bias[n] + resid_scale*resid[m,n] + g0[gi0[m],n] + g1[gi1[m],n])
struct GemmArgs {
    const float* A = nullptr; int lda = 0;      // [M,K]
    const float* W = nullptr; int ldw = 0;      // [N,K]  (nn.Linear layout)
    float* C = nullptr;       int ldc = 0;      // [M,N]
    int M = 0, N = 0, K = 0;
    const float* bias = nullptr;                // [N]
    const float* rowscale = nullptr;            // [M]
    const float* resid = nullptr; int ldr = 0; float resid_scale = 1.f;
    const float* g0 = nullptr; const int32_t* gi0 = nullptr; int ldg0 = 0;   // gathered row add
    const float* g1 = nullptr; const int32_t* gi1 = nullptr; int ldg1 = 0;
    int relu_a = 0;                             // apply ReLU to A while staging
    int act = ACT_NONE;
    // split-bf16 path: prec 0 = exact fp32 MFMA, 1 = bf16, 3 = bf16x3; weights pre-split [N,K] bf16 (ldw shared)
    int prec = 0;
    const uint16_t* Whi = nullptr;
    const uint16_t* Wlo = nullptr;
    long long* clock_probe = nullptr;           // optional [grid][4] DVFS probe buffer (vlsat_debug_gemm_clock_probe)
    // storage format of A / the residual / C: 0 fp32, 1 split-pair words (common.h pack_split; split-bf16 mode),
    // 2 half rows (bf16 values at byte 2 * column of an fp32-pitched row; single-rounding modes)
    int a_split = 0, r_split = 0, c_split = 0;
    float c_scale = 1.f;                        // final multiplier of C (after bias / activation)
    int ablate = 0;                             // timing experiments on the ring kernel: bit 0 no operand loads after the first slices, bit 1 no MFMAs, bit 2 (8-phase kernel) no fragment reads (results are garbage)
    int ring_nodb = 0;                          // experiment: half-row ring kernel without the double-buffered fragment sets
    int ring_bk32 = 0;                          // experiment: half-row ring kernel with 32-wide k slices (default 64 where K allows)
    int ring_wide = 0;                          // experiment (experiments build): bf16 ring kernel with 128 x 256 tiles where N allows (measured equal)
    int no_ring = 0;                            // debug: keep large bf16 launches on the two-stage 128 x 128 kernel
    int no_p8 = 0;                              // debug: large launches skip the 256 x 256 8-phase kernel (gemm_bf16_p8.hip)
    int p8_part_min = 0;                        // 8-phase kernel: tiles from which a remainder rides along as balanced rounds / a partial round (0: the built-in bound, 32 in bf16, 5/8 of a round otherwise)
    int sk_max_tiles = 0;                       // split-K kernel only for launches of at most this many 64 x 64 tiles (0: half the resident slots, the rule of rounds 2-5)
    int k_rot = 0;                              // A-B: the column tiles of a row panel walk their K-tiles rotated by tn * k_rot (8-phase kernel: siblings re-read the A panel out of step)
    // fp16 additive tables (round 6; the single-rounding modes): the first c_f16_cols columns of C (a multiple of the block tile's width) are
    // stored as fp16 HALF ROWS (element n at byte 2 n of the fp32-pitched row, values clamped to +-65504) -- what the node-side projection
    // writes for [P_i | P_j]; g_f16: g0 / g1 are such half rows (launches without a residual).  Halves the bytes nn_edge.0 gathers per edge.
    int c_f16_cols = 0, g_f16 = 0;
    // fp16 half-row OPERANDS (precision mode "fp16_mixed"): A (a_split == 2) holds fp16 instead of bf16, Whi is an fp16 plane, the products run on
    // v_mfma_f32_32x32x16_f16 (same rate as bf16 on CDNA4, 2^-12 instead of 2^-9 per operand); half-row outputs then go through c_f16_cols == N
    int half_f16 = 0;
    int force_tile = 0;                         // experiment (tools/gemm_tile_sweep.py): 1 = 128x128, 2 = 128x64, 3 = 64x128, 4 = 64x64 tiles of gemm_f32_kernel, whatever the heuristic says
    int prefetch = -1;                          // bf16 LDS-direct pipe: slices of look-ahead of the A-panel prefetch (0 off, -1 default)
    int no_dma = 0;                             // debug: VGPR-staged fp32 operands instead of LDS-direct (vlsat_debug_option "gemm_dma")
    long* launches = nullptr;                   // optional host counter, +1 per kernel launched (profiling)
    // split-K path of small launches (gemm_splitk.hip): partial-sum workspace + per-tile arrival counters (zero between
    // launches), owned by the caller and private to the stream the launch goes to; null = never split
    float* sk_ws = nullptr; size_t sk_ws_floats = 0;
    unsigned* sk_counters = nullptr; size_t sk_n_counters = 0;
    // split-fp16 form of the exact-fp32 8-phase launch (prec 0 only; gemm_p8s_pick): fp16 planes Wh16 = f16(W 2^w_exp), Wl16 = f16(W 2^w_exp - Wh16)
    // of the weight tensor ([N,K], pitch ldw; gemm_f16s_planes.h), fp32 tensors in and out, three f16 MFMAs per product.  f16s = 1: the 8-phase
    // launches only, every other kernel a launch may get (tails, small launches) stays exact; 2: the persistent kernel's launches too, on
    // gemm_f16s_kernel (gemm_f16s_tiled_pick); 3: those only.  Split-K launches always stay exact.
    int f16s = 0;
    const uint16_t* Wh16 = nullptr;
    const uint16_t* Wl16 = nullptr;
    int w_exp = 0;
    // fp32 mode, "edge_pairs": A is read / C is written as GEMM PAIR WORDS (gemm_f16s_planes.h: Ah << 16 | Al of the split-fp16 operand, one
    // word per element, same pitch).  Only on the split-fp16 siblings (f16s == 2: every part of the launch on one; gemm_pairs_pick says
    // whether a plan's part has the form) -- which launches get them is decided once per forward (edge_pairs.h).
    // c_pair 2: C as ATTENTION pair words -- columns [0, N / 2) in the K format, [N / 2, N) in the V format (times 2^3) of the split-fp16 edge
    // attention (the key | value projection; N % 512 == 0, no additive operands)
    // (two 16-bit fields in what was the struct's tail padding: the kernel-argument layout, and with it the code of every kernel that existed
    //  before them, is unchanged)
    int16_t a_pair = 0, c_pair = 0;
};
static_assert(sizeof(GemmArgs) % 8 == 0 && offsetof(GemmArgs, c_pair) + 2 == sizeof(GemmArgs), "a_pair / c_pair fill the tail padding behind w_exp");
// The first launch of a GEMM as plan_gemm chooses it: kernel family, the row of the family's list, geometry, and the rows [0, rows) it
// covers -- the rows after them are planned again as a problem of their own (the tail).
struct GemmPlan {
    enum Family { SPLITK, P8, RING, TILED };
    int family = TILED;
    int rows = 0;
    int bm = 64, bn = 64;           // output tile (8-phase: 256 x 256; ring: 32768 / bn x bn)
    int ksl = 1, slot_mult = 2;     // persistent kernel: k-slices per pipeline step, resident blocks per CU its grid is sized for
    int ks = 0, slices = 0;         // split-K: parts of the k range, k-slices per part
    int n_tiles = 0, grid = 0;
    int variant = -1;               // row of the family's list; -1 (persistent kernel only): no kernel takes these operands (gemm_tiled_pick says why)
};
struct GemmPick { int index; const char* why; };      // a row of a family's list, or -1 and the reason

constexpr int BK = 32;    // k-slice held in LDS per pipeline stage
constexpr size_t SPLITK_WS_FLOATS = (size_t)768 * 4096;    // room for 768 partial 64 x 64 tiles (12 MB)
constexpr size_t SPLITK_COUNTERS = 512;

// the byte offsets of rows [0, rows + 256) of an operand with a pitch of ld floats fit in 32 bits (LDS-direct loads, buffer descriptors)
inline bool offsets32(size_t rows, size_t ld) { return (rows + 256) * ld * 4 < (1ull << 32); }
// additive operands of a launch: bit 0 = residual, bit 1 = gathered rows g0, bit 2 = gathered rows g1
inline int gemm_add_mode(const GemmArgs& a) { return (a.resid ? 1 : 0) | (a.g0 ? 2 : 0) | (a.g1 ? 4 : 0); }
// ... of which the 8-phase and ring kernels and the LDS-direct pipes of the persistent kernel are built for: none, residual, both gathered rows
inline bool gemm_add_built(int add) { return add == 0 || add == 1 || add == 6; }
// PipeSel code (gemm_core.h) of the persistent and split-K kernels for a launch's operands: exact fp32 without ReLU-on-A and the bf16
// modes take the LDS-direct pipes (codes 4..15) where the operands allow it; -1 = no pipe, and why.
// relu_a: ReLU-on-A of the launch -- of either problem of a pair, which then both take the staging pipe (same products).
// add_modes: the LDS-direct pipes only for the additive modes the persistent kernel instantiates them for; the split-K kernel has
// every mode on every pipe.
inline GemmPick gemm_pipe_prec(const GemmArgs& a, bool relu_a, bool add_modes) {
    const bool dma_ok = !a.no_dma && (!add_modes || gemm_add_built(gemm_add_mode(a))) && offsets32(a.M, a.lda) && offsets32(a.N, a.ldw);
    const int prec = (a.prec == 0 && dma_ok && !relu_a) ? 4 : a.prec;
    if (a.a_split == 2 && !(prec == 1 && dma_ok)) return {-1, "gemm: half-row A needs the single-rounding bf16 precision and the LDS-direct pipe"};
    if ((prec == 1 || prec == 3) && dma_ok) return {prec + (a.a_split == 2 ? (a.half_f16 ? 14 : 12) : a.a_split ? 8 : 4), nullptr};   // bf16 modes: A split on the fragment-read side, so ReLU-on-A is fine
    if (a.a_split) return {-1, "gemm: split-pair A needs a bf16 precision and the LDS-direct pipe"};
    return {prec, nullptr};
}

// ---- the lists of the 8-phase and ring kernels ----
// 8-phase: X(MODE, ADD, RELU, CF), the template arguments of gemm_p8_kernel in its order (ABL = 0).
// MODE 0 bf16 half rows | 1 exact fp32 | 2 split-bf16 on split pairs | 3 fp16 half rows; CF: format of C, 0 fp32 | 1 split pairs |
// 2 bf16 half rows | 3 fp16 half rows (GemmArgs::c_f16_cols == N).  By line: the four modes.
#define VLSAT_GEMM_P8_RELEASE(X)                                                                                                     \
    X(0, 0, false, 0) X(0, 0, false, 2) X(0, 0, true, 0) X(0, 0, true, 2) X(0, 1, false, 0) X(0, 1, false, 2) X(0, 6, false, 2) X(0, 6, true, 2) X(0, 0, false, 3) \
    X(1, 0, false, 0) X(1, 0, true, 0) X(1, 1, false, 0) X(1, 6, false, 0) X(1, 6, true, 0)                                           \
    X(2, 0, false, 0) X(2, 0, false, 1) X(2, 0, true, 0) X(2, 0, true, 1) X(2, 1, false, 0) X(2, 6, false, 1) X(2, 6, true, 1)         \
    X(3, 0, false, 0) X(3, 0, false, 3) X(3, 0, true, 0) X(3, 0, true, 3) X(3, 6, false, 3) X(3, 6, true, 3)
// Ring: X(TERMS, AFMT, ADD, RBN, RBK, DB), the template arguments of gemm_ring_kernel in its order.
// TERMS 1 | 3; AFMT: A as 0 fp32 | 1 split pairs | 2 bf16 half rows | 3 fp16 half rows; tile 32768 / RBN x RBN; RBK: k per slice, 64 for
// half-row A only, there with and without the double-buffered fragment sets (DB).
// By line: split-bf16 | single rounding on fp32 / split-pair A | bf16 half rows | fp16 half rows.
#define VLSAT_GEMM_RING_RELEASE(X)                                                                                                           \
    X(3, 0, 0, 128, 32, false) X(3, 0, 1, 128, 32, false) X(3, 0, 6, 128, 32, false) X(3, 1, 0, 128, 32, false) X(3, 1, 1, 128, 32, false) X(3, 1, 6, 128, 32, false) \
    X(1, 0, 0, 128, 32, false) X(1, 0, 1, 128, 32, false) X(1, 0, 6, 128, 32, false) X(1, 1, 0, 128, 32, false) X(1, 1, 1, 128, 32, false) X(1, 1, 6, 128, 32, false) \
    X(1, 2, 0, 128, 32, false) X(1, 2, 1, 128, 32, false) X(1, 2, 6, 128, 32, false) X(1, 2, 0, 128, 64, false) X(1, 2, 1, 128, 64, false) X(1, 2, 6, 128, 64, false) \
    X(1, 2, 0, 128, 64, true) X(1, 2, 1, 128, 64, true) X(1, 2, 6, 128, 64, true)                                                                \
    X(1, 3, 0, 128, 32, false) X(1, 3, 1, 128, 32, false) X(1, 3, 6, 128, 32, false) X(1, 3, 0, 128, 64, false) X(1, 3, 1, 128, 64, false) X(1, 3, 6, 128, 64, false) \
    X(1, 3, 0, 128, 64, true) X(1, 3, 1, 128, 64, true) X(1, 3, 6, 128, 64, true)
// Experiments build only.  8-phase: X(MODE, ADD, RELU, CF, ABL), the timing ablations (GemmArgs::ablate; results are GARBAGE) of the gathered-row
// launch (ABL 256, 512) and of the plain half-row launch (tools/p8_check.py --ablate).  Ring: 128 x 256 tiles (GemmArgs::ring_wide) -- half the
// bytes of A per flop, twice those of the weights; measured equal
#ifdef VLSAT_EXPERIMENTS
#define VLSAT_GEMM_P8_LAB(X)                                                                                                         \
    X(0, 6, true, 2, 256) X(0, 6, true, 2, 512) X(0, 0, false, 2, 1) X(0, 0, false, 2, 2) X(0, 0, false, 2, 3) X(0, 0, false, 2, 4) X(0, 0, false, 2, 5) \
    X(0, 0, false, 2, 6) X(0, 0, false, 2, 7) X(0, 0, false, 2, 8) X(0, 0, false, 2, 15) X(0, 0, false, 2, 37) X(0, 0, false, 2, 65)
#define VLSAT_GEMM_RING_LAB(X)                                                                                                               \
    X(3, 0, 0, 256, 32, false) X(3, 0, 1, 256, 32, false) X(3, 0, 6, 256, 32, false) X(3, 1, 0, 256, 32, false) X(3, 1, 1, 256, 32, false) X(3, 1, 6, 256, 32, false) \
    X(1, 0, 0, 256, 32, false) X(1, 0, 1, 256, 32, false) X(1, 0, 6, 256, 32, false) X(1, 1, 0, 256, 32, false) X(1, 1, 1, 256, 32, false) X(1, 1, 6, 256, 32, false) \
    X(1, 2, 0, 256, 32, false) X(1, 2, 1, 256, 32, false) X(1, 2, 6, 256, 32, false) X(1, 3, 0, 256, 32, false) X(1, 3, 1, 256, 32, false) X(1, 3, 6, 256, 32, false)
constexpr bool kGemmLab = true;
#else
#define VLSAT_GEMM_P8_LAB(X)
#define VLSAT_GEMM_RING_LAB(X)
constexpr bool kGemmLab = false;
#endif

// ---- 8-phase kernel (its list: above) ----
#define VLSAT_GEMM_P8_VARIANTS(X) VLSAT_GEMM_P8_RELEASE(X) VLSAT_GEMM_P8_LAB(X)
struct GemmP8Variant { int mode, add; bool relu; int cf, abl; };
#define VLSAT_ROW(M, A, R, C, ...) {M, A, R, C, __VA_ARGS__},      // (a release row has no ABL: 0)
constexpr GemmP8Variant kGemmP8Variants[] = {VLSAT_GEMM_P8_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmP8Count = (int)(sizeof kGemmP8Variants / sizeof kGemmP8Variants[0]);
constexpr int gemm_p8_find(int mode, int add, bool relu, int cf, int abl = 0) {
    for (int i = 0; i < kGemmP8Count; ++i)
        if (const GemmP8Variant& v = kGemmP8Variants[i]; v.mode == mode && v.add == add && v.relu == relu && v.cf == cf && v.abl == abl) return i;
    return -1;
}
// The row for a launch's operands.  Shapes: 256 x 256 tiles, K-tiles of 32 (4-byte A elements) or 64; M need not be a multiple of the
// tile (the last panel's rows past M are outside every buffer descriptor -- loads return zeros, stores are dropped -- and tile_init
// clamps the row of an additive operand).
inline GemmPick gemm_p8_pick(const GemmArgs& a) {
    const int add = gemm_add_mode(a);
    const bool f32 = a.prec == 0, x3 = a.prec == 3, c16 = a.c_f16_cols > 0;
    if (a.rowscale || a.act == ACT_SIGMOID || !gemm_add_built(add)) return {-1, "gemm_p8: no row scale, no sigmoid, additive operands none | residual | both gathered rows"};
    // the fp32 / split-bf16 epilogues read the bias as float4 (the half-row one as scalars): an unaligned bias pointer of a
    // caller of vlsat_k_gemm goes to the older kernels, which have the scalar fallback
    if ((f32 || x3) && a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 15)) return {-1, "gemm_p8: bias must be 16-byte aligned"};
    if (f32 ? (a.a_split || a.c_split || a.r_split || a.c_scale != 1.f)
            : x3 ? (a.a_split != 1 || a.c_split == 2 || !a.Wlo) : (a.prec != 1 || a.a_split != 2 || a.c_split == 1))
        return {-1, "gemm_p8: fp32 on fp32 tensors, split-bf16 on split-pair A, single-rounding bf16 on half-row A"};
    const int kt = (f32 || x3) ? 32 : 64;          // an output tile is an even number (>= 4) of K-tiles
    if (a.N % 256 || a.K % (2 * kt) || a.K < 4 * kt) return {-1, "gemm_p8: N % 256 == 0, K an even number (>= 4) of K-tiles"};
    // the whole output as fp16 half rows, and fp16 operands (whose half-row outputs come as c_f16_cols == N): half-row launches only
    if ((c16 && a.c_f16_cols != a.N) || ((c16 || a.half_f16) && (f32 || x3 || a.c_split))) return {-1, "gemm_p8: fp16 columns / operands belong to half-row launches, c_f16_cols == N"};
    const int mode = f32 ? 1 : x3 ? 2 : a.half_f16 ? 3 : 0, cf = c16 ? 3 : a.c_split;
    int abl = 0;
    if (kGemmLab && a.ablate && mode == 0 && cf == 2 && add == 6 && a.relu_a) abl = a.ablate == 1 ? 256 : 512;       // timing experiments on the gathered-row launch
    if (kGemmLab && a.ablate && mode == 0 && cf == 2 && add == 0 && !a.relu_a) abl = gemm_p8_find(0, 0, false, 2, a.ablate) >= 0 ? a.ablate : 15;
    const int i = gemm_p8_find(mode, add, a.relu_a != 0, cf, abl);
    return i < 0 ? GemmPick{-1, "gemm_p8: operand combination not built"} : GemmPick{i, nullptr};
}
// Split-fp16 siblings of the exact-fp32 rows (MODE 1): X(ADD, RELU) = gemm_p8s_kernel<2, ADD, RELU, 0> -- the (additive operands,
// ReLU-on-A) combinations the fp32 forward launches.  A sibling takes the launch of its MODE 1 row as planned: same tiles, grid and rows.
#define VLSAT_GEMM_P8S_VARIANTS(X) X(0, false) X(0, true) X(1, false) X(6, false) X(6, true)
// ... and their forms on GEMM pair words (GemmArgs::a_pair / c_pair): X(ADD, RELU, PF) = gemm_p8s_kernel<2, ADD, RELU, PF>, PF bit 0: C is
// written as pair words, bit 1: C is written as ATTENTION pair words (c_pair 2), bit 2: A is read as pair words (PF 0 is the sibling
// itself).  By line: nn_edge.0 (gathered rows; C = Hbig), the launches without additive operands (nn_edge.2, proj_edge, relation
// encoder conv3, relation head), the key | value projection of the edge attention and its out-projection (A = Oe, + residual)
#define VLSAT_GEMM_P8S_PAIR_VARIANTS(X)                                  \
    X(6, false, 1) X(6, false, 5) X(6, true, 1) X(6, true, 5)            \
    X(0, false, 1) X(0, false, 4) X(0, false, 5) X(0, true, 1) X(0, true, 4) X(0, true, 5)            \
    X(0, false, 2) X(0, false, 6) X(1, false, 4)
struct GemmP8sVariant { int add; bool relu; };
#define VLSAT_ROW(A, R) {A, R},
constexpr GemmP8sVariant kGemmP8sVariants[] = {VLSAT_GEMM_P8S_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmP8sCount = (int)(sizeof kGemmP8sVariants / sizeof kGemmP8sVariants[0]);
struct GemmP8sPairVariant { int add; bool relu; int pf; };
#define VLSAT_ROW(A, R, P) {A, R, P},
constexpr GemmP8sPairVariant kGemmP8sPairVariants[] = {VLSAT_GEMM_P8S_PAIR_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmP8sPairCount = (int)(sizeof kGemmP8sPairVariants / sizeof kGemmP8sPairVariants[0]);
constexpr int gemm_pair_form(int a_pair, int c_pair) { return (a_pair ? 4 : 0) | (c_pair == 2 ? 2 : c_pair ? 1 : 0); }
constexpr int gemm_p8s_pair_find(int add, bool relu, int pf) {
    for (int i = 0; i < kGemmP8sPairCount; ++i)
        if (kGemmP8sPairVariants[i].add == add && kGemmP8sPairVariants[i].relu == relu && kGemmP8sPairVariants[i].pf == pf) return i;
    return -1;
}
constexpr int gemm_p8s_find(int add, bool relu) {
    for (int i = 0; i < kGemmP8sCount; ++i)
        if (kGemmP8sVariants[i].add == add && kGemmP8sVariants[i].relu == relu) return i;
    return -1;
}
// GemmArgs::f16s: which exact-fp32 launches of a problem run on their split-fp16 sibling -- 1 the 8-phase launches, 2 those and the
// persistent kernel's, 3 the persistent kernel's only (the split-K launches always stay exact)
// The code of a launch of the fp32 mode, the one place that states it (gemm_resolve of engine_forward.hip and edge_pairs_plan ask): the
// full rounds of an 8-phase launch run on the sibling unless "gemm_exact" asks for the exact kernel, the persistent kernel's launches
// (tails, small launches, node rows) unless "gemm_small_exact" does -- and with "gemm_small_exact" node-row launches are exact whatever
// they run on (the releases before the persistent kernel's siblings)
inline int gemm_f16s_code(bool gemm_exact, bool gemm_small_exact, bool node_rows) {
    const bool small = !gemm_small_exact, big = !gemm_exact && !(node_rows && !small);
    return small ? (big ? 2 : 3) : (big ? 1 : 0);
}
inline bool gemm_f16s_p8(const GemmArgs& a) { return a.f16s == 1 || a.f16s == 2; }
inline bool gemm_f16s_tiled(const GemmArgs& a) { return a.f16s == 2 || a.f16s == 3; }
// The sibling that runs row `variant` of the 8-phase list for a launch with GemmArgs::f16s 1 or 2, or -1: the row itself runs.  The one
// place that decides it (launch_gemm_p8 asks; a pair of problems never is an 8-phase launch, gemm_pair_plan).
inline int gemm_p8s_pick(const GemmArgs& a, int variant) {
    if (!gemm_f16s_p8(a) || variant < 0 || variant >= kGemmP8Count) return -1;
    const GemmP8Variant& v = kGemmP8Variants[variant];
    return v.mode == 1 && v.abl == 0 ? gemm_p8s_find(v.add, v.relu) : -1;
}
// ... and for a launch on pair words (a_pair | c_pair): the row of the pair list that runs it, or -1 -- then NOTHING runs it (an error)
inline int gemm_p8s_pair_pick(const GemmArgs& a, int variant) {
    if (gemm_p8s_pick(a, variant) < 0) return -1;
    const GemmP8Variant& v = kGemmP8Variants[variant];
    return gemm_p8s_pair_find(v.add, v.relu, gemm_pair_form(a.a_pair, a.c_pair));
}
// n_tiles tiles of the problem on a grid of `grid` blocks: the kernel keeps one column tile per block (bias registers)
inline bool gemm_p8_geometry_ok(int M, int N, long n_tiles, long grid) {
    return n_tiles <= (long)((M + 255) / 256) * (N / 256) && grid % 8 == 0 && (grid / 8) % (N / 256) == 0;
}

// ---- ring kernel (its list: above) ----
#define VLSAT_GEMM_RING_VARIANTS(X) VLSAT_GEMM_RING_RELEASE(X) VLSAT_GEMM_RING_LAB(X)
struct GemmRingVariant { int terms, afmt, add, rbn, rbk; bool db; };
#define VLSAT_ROW(T, S, A, N, K, D) {T, S, A, N, K, D},
constexpr GemmRingVariant kGemmRingVariants[] = {VLSAT_GEMM_RING_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmRingCount = (int)(sizeof kGemmRingVariants / sizeof kGemmRingVariants[0]);
constexpr int gemm_ring_find(int terms, int afmt, int add, int rbn, int rbk, bool db) {
    for (int i = 0; i < kGemmRingCount; ++i)
        if (const GemmRingVariant& v = kGemmRingVariants[i]; v.terms == terms && v.afmt == afmt && v.add == add && v.rbn == rbn && v.rbk == rbk && v.db == db) return i;
    return -1;
}
// The row for a launch's operands (prec 1 | 3) on tiles rbn wide.  Half-row A, one plane: 64-wide slices whenever K allows.
inline GemmPick gemm_ring_pick(const GemmArgs& a, int rbn) {
    const int add = gemm_add_mode(a);
    if (a.rowscale || !gemm_add_built(add)) return {-1, "gemm_ring: no row scale, additive operands none | residual | both gathered rows"};
    if (a.prec == 3 && a.a_split == 2) return {-1, "gemm_ring: half-row A belongs to the single-rounding precision"};
    const int terms = a.prec == 3 ? 3 : 1, afmt = a.a_split == 2 ? (a.half_f16 ? 3 : 2) : a.a_split ? 1 : 0;
    const bool k64 = afmt >= 2 && rbn == 128 && !a.ring_bk32 && a.K % 64 == 0, db = k64 && !a.ring_nodb && a.K % 128 == 0;
    const int i = gemm_ring_find(terms, afmt, add, rbn, k64 ? 64 : 32, db);
    return i < 0 ? GemmPick{-1, "gemm_ring: operand combination not built"} : GemmPick{i, nullptr};
}

// ---- persistent kernel: X(ADD, PREC, TWIN), ADD and PREC (the PipeSel code) of gemm_f32_kernel; TWIN: has the form for two problems ----
// Every row is instantiated for the tiles of kGemmTiles, and with TWIN for a pair on 64 x 64 tiles at two k-slices per step as well.
#define VLSAT_GEMM_TILED_VARIANTS(X)                                                                                   \
    X(0, 13, true) X(1, 13, true) X(6, 13, true) X(0, 15, true) X(6, 15, true)                                         \
    X(0, 9, true) X(1, 9, true) X(6, 9, true) X(0, 11, true) X(1, 11, true) X(6, 11, true)                             \
    X(0, 4, true) X(1, 4, true) X(6, 4, true) X(0, 5, true) X(1, 5, true) X(6, 5, true) X(0, 7, true) X(1, 7, true) X(6, 7, true) \
    X(0, 0, true) X(1, 0, true) X(2, 0, false) X(3, 0, false) X(4, 0, false) X(5, 0, false) X(6, 0, true) X(7, 0, false) \
    X(0, 1, false) X(1, 1, false) X(6, 1, false) X(0, 3, false) X(1, 3, false) X(6, 3, false)
struct GemmTiledVariant { int add, prec; bool twin; };
struct GemmTile { int bm, bn, ksl; };
constexpr GemmTile kGemmTiles[] = {{128, 128, 1}, {128, 64, 1}, {64, 128, 1}, {64, 64, 1}, {64, 64, 2}};
constexpr int kGemmTileCount = 5;                         // (the twin form: the last tile)
constexpr int gemm_tile_index(int bm, int bn, int ksl) { return bm == 128 ? (bn == 128 ? 0 : 1) : bn == 128 ? 2 : ksl == 2 ? 4 : 3; }
#define VLSAT_ROW(A, P, T) {A, P, T},
constexpr GemmTiledVariant kGemmTiledVariants[] = {VLSAT_GEMM_TILED_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmTiledCount = (int)(sizeof kGemmTiledVariants / sizeof kGemmTiledVariants[0]);
constexpr int gemm_tiled_find(int add, int prec) {
    for (int i = 0; i < kGemmTiledCount; ++i)
        if (kGemmTiledVariants[i].add == add && kGemmTiledVariants[i].prec == prec) return i;
    return -1;
}
// relu_a: of either problem of a pair; twin: the row must have the twin form
inline GemmPick gemm_tiled_pick(const GemmArgs& a, bool relu_a, bool twin = false) {
    if (a.prec == 0 && (a.a_split || a.r_split || a.c_split || a.c_scale != 1.f))
        return {-1, "gemm: operand formats and c_scale exist in the bf16 modes only"};      // (the fp32 kernels fold them away)
    const GemmPick pipe = gemm_pipe_prec(a, relu_a, true);
    if (pipe.index < 0) return pipe;
    const int i = gemm_tiled_find(gemm_add_mode(a), pipe.index);
    if (i < 0) return {-1, "gemm: this precision / additive-operand combination is not built"};
    return twin && !kGemmTiledVariants[i].twin ? GemmPick{-1, "gemm: no twin form"} : GemmPick{i, nullptr};
}
// Split-fp16 siblings of the persistent kernel's exact-fp32 rows (PREC 0 / 4): X(ADD) = gemm_f16s_kernel<.., ADD, 17, ..> on every tile of
// kGemmTiles and as a twin.  One pipe for both ReLU-on-A settings (its clamp does the ReLU).  A sibling takes the launch as planned: same
// tile, grid and rows.
#define VLSAT_GEMM_F16S_TILED_VARIANTS(X) X(0) X(1) X(6)
// ... on GEMM pair words (GemmArgs::a_pair / c_pair): PREC 18 (C written as pairs), 19 (A read as pairs), 20 (both) of the same rows, on every
// tile (no twin form: a pair of problems never carries pair words); PREC 21 / 22 (C as ATTENTION pair words, c_pair 2; 22: A read as
// pairs) of the row without additive operands only (the key | value projection)
constexpr int gemm_f16s_pair_prec(int a_pair, int c_pair) { return c_pair == 2 ? 21 + (a_pair ? 1 : 0) : 17 + (c_pair ? 1 : 0) + (a_pair ? 2 : 0); }
constexpr bool gemm_f16s_pair_built(int add, int prec) { return prec >= 18 && prec <= 22 && (prec <= 20 || add == 0); }
#define VLSAT_ROW(A) A,
constexpr int kGemmF16sTiledAdds[] = {VLSAT_GEMM_F16S_TILED_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmF16sTiledCount = (int)(sizeof kGemmF16sTiledAdds / sizeof kGemmF16sTiledAdds[0]);
// The sibling that runs row `variant` of the persistent kernel's list for a launch, or -1 and the reason: the row itself (the exact
// kernel) runs.  ReLU-on-A does not enter: one sibling serves both settings, of one problem or of a pair.  Not built for: the VGPR-staged pipe where it was picked for anything but ReLU-on-A (operands
// beyond 32-bit offsets, additive modes 2-5 and 7, GemmArgs::no_dma), operand formats, fewer than 64 output columns (less than one column
// tile: such a launch is bound by its latency, not by the matrix pipe).  K: a multiple of 32 like every launch; the planes need ldw % 8 == 0
// (gemm_invalid).  The one place that decides it (launch_tiled asks, for single and paired launches).
inline GemmPick gemm_f16s_tiled_pick(const GemmArgs& a, int variant) {
    if (!gemm_f16s_tiled(a)) return {-1, "gemm_f16s: not asked for"};
    if (variant < 0 || variant >= kGemmTiledCount) return {-1, "gemm_f16s: no planned row"};
    const GemmTiledVariant& v = kGemmTiledVariants[variant];
    if (v.prec != 0 && v.prec != 4) return {-1, "gemm_f16s: the siblings are those of the exact-fp32 rows"};
    if (a.prec != 0 || a.a_split || a.r_split || a.c_split || a.c_scale != 1.f || a.c_f16_cols || a.g_f16) return {-1, "gemm_f16s: fp32 tensors in and out"};
    if (gemm_pipe_prec(a, false, true).index != 4) return {-1, "gemm_f16s: needs the LDS-direct pipe (32-bit offsets, additive operands none | residual | both gathered rows)"};
    if (a.N < 64) return {-1, "gemm_f16s: fewer than 64 output columns"};
    for (int i = 0; i < kGemmF16sTiledCount; ++i)
        if (kGemmF16sTiledAdds[i] == v.add) return {i, nullptr};
    return {-1, "gemm_f16s: additive-operand combination not built"};
}

// ---- split-K kernel: X(PREC), the PipeSel code; every row single and as a twin, every additive mode ----
#define VLSAT_GEMM_SPLITK_VARIANTS(X) X(0) X(1) X(3) X(4) X(5) X(7) X(9) X(11) X(13) X(15)
#define VLSAT_ROW(P) P,
constexpr int kGemmSplitkVariants[] = {VLSAT_GEMM_SPLITK_VARIANTS(VLSAT_ROW)};
#undef VLSAT_ROW
constexpr int kGemmSplitkCount = (int)(sizeof kGemmSplitkVariants / sizeof kGemmSplitkVariants[0]);
// (a pair takes the staging pipe that can apply ReLU to A if either needs it: same products)
inline GemmPick gemm_splitk_pick(const GemmArgs& a, bool relu_a) {
    const GemmPick pipe = gemm_pipe_prec(a, relu_a, false);
    for (int i = 0; pipe.index >= 0 && i < kGemmSplitkCount; ++i)
        if (kGemmSplitkVariants[i] == pipe.index) return {i, nullptr};
    return {-1, pipe.why ? pipe.why : "gemm_splitk: pipe not built"};
}

// ---- the planner ----
// nullptr when launch_gemm takes the problem (an empty one included), else what it reports
inline const char* gemm_invalid(const GemmArgs& a) {
    if (!a.A || !a.W || !a.C) return "gemm: null A/W/C";
    if (a.M <= 0 || a.N <= 0) return nullptr;
    if (a.K <= 0 || a.K % BK) return "gemm: K must be a positive multiple of 32";
    if ((a.lda & 3) || (a.ldw & 3)) return "gemm: lda/ldw must be multiples of 4 floats";
    if (a.prec != 0 && a.prec != 1 && a.prec != 3) return "gemm: prec must be 0 (fp32), 1 (bf16) or 3 (bf16x3)";
    if (a.prec && (!a.Whi || (a.prec == 3 && !a.Wlo) || (a.ldw & 7))) return "gemm: bf16 path needs pre-split weights and ldw % 8 == 0";
    if (a.rowscale && (a.resid || a.g0 || a.g1)) return "gemm: rowscale cannot be combined with resid/g0/g1 (additive operands are accumulator inits)";
    if ((reinterpret_cast<uintptr_t>(a.A) & 15) || (reinterpret_cast<uintptr_t>(a.W) & 15)) return "gemm: A/W must be 16-byte aligned";
    if (a.half_f16 && (a.prec != 1 || a.a_split != 2 || a.c_split || a.r_split)) return "gemm: fp16 operands are half-row A launches of the single-rounding precision; their half-row output is c_f16_cols == N";
    if ((a.c_f16_cols || a.g_f16) && a.prec == 0) return "gemm: fp16 half-row columns / tables belong to the bf16 modes (the exact-fp32 kernels read and write fp32)";
    if (a.c_f16_cols && ((a.c_f16_cols != a.N && a.c_f16_cols % 256) || a.c_f16_cols > a.N || a.c_split)) return "gemm: c_f16_cols must be N or a multiple of 256 within N, of an fp32 output";
    if (a.f16s && (a.prec != 0 || !a.Wh16 || !a.Wl16 || (a.ldw & 7) || ((reinterpret_cast<uintptr_t>(a.Wh16) | reinterpret_cast<uintptr_t>(a.Wl16)) & 15) ||
                   a.w_exp < -100 || a.w_exp > 100))
        return "gemm: f16s is the exact-fp32 precision with two 16-byte aligned fp16 weight planes, ldw % 8 == 0 and |w_exp| <= 100";
    if ((a.a_pair || a.c_pair) && (a.f16s != 2 || a.rowscale || a.act == ACT_SIGMOID || a.N % 64))
        return "gemm: pair words are read and written by the split-fp16 siblings only (f16s 2), no row scale, no sigmoid, N % 64 == 0";
    if (a.c_pair == 2 && (a.N % 512 || a.resid || a.g0 || a.g1 || a.act != ACT_NONE)) return "gemm: attention pair words are the output of a plain Linear with N % 512 == 0";
    if (a.g_f16 && (a.resid || !(a.g0 || a.g1) || a.N % 256 || ((a.ldg0 | a.ldg1) & 1) || ((reinterpret_cast<uintptr_t>(a.g0) | reinterpret_cast<uintptr_t>(a.g1)) & 7)))
        return "gemm: g_f16 needs gathered rows, no residual, N % 256 == 0 and 8-byte aligned tables";
    return nullptr;
}

// rows [row0, M) of the problem as a sub-problem
inline GemmArgs tail_of(const GemmArgs& a, int row0) {
    GemmArgs t = a;
    t.A += (size_t)row0 * a.lda; t.C += (size_t)row0 * a.ldc; t.M = a.M - row0;
    if (a.rowscale) t.rowscale += row0;
    if (a.resid) t.resid += (size_t)row0 * a.ldr;
    if (a.gi0) t.gi0 += row0;
    if (a.gi1) t.gi1 += row0;
    return t;
}

// the persistent kernel on BM x BN tiles, a grid of slot_mult blocks per CU (G: resident slots at two per CU)
inline GemmPlan plan_tiled(const GemmArgs& a, int G, int bm, int bn, int slot_mult = 2) {
    GemmPlan p;
    p.bm = bm; p.bn = bn; p.slot_mult = slot_mult; p.rows = a.M;
    const int Gs = G / 2 * slot_mult;
    const int nbm = (a.M + bm - 1) / bm, nbn = (a.N + bn - 1) / bn;
    const long T = (long)nbm * nbn, main_panels = (T / Gs * Gs) / nbn;
    p.n_tiles = (int)T;
    if (T <= Gs) {                                  // one round: grid = tiles (rounded up to 8)
        p.grid = (int)((T + 7) / 8) * 8;
        // latency-bound: two k-slices per pipeline step (four per step measured no faster: tools/latency_probe.py, round 2)
        if (bm == 64 && bn == 64 && a.K % (2 * BK) == 0) p.ksl = 2;
    } else {
        // full rounds with this tile; the remaining M-panels go to a smaller tile (see the header of gemm_f32.hip)
        p.grid = Gs;
        if (main_panels > 0 && main_panels < nbm && !(bm == 64 && bn == 64)) {
            p.rows = (int)(main_panels * bm);
            p.n_tiles = (int)(main_panels * nbn);
        }
    }
    GemmArgs m = a;
    m.M = p.rows;                                   // (the pipe goes by the rows of this launch: 32-bit offsets)
    p.variant = gemm_tiled_pick(m, a.relu_a).index;
    return p;
}

// the 8-phase / ring kernel on rows [0, rows)
inline GemmPlan big_plan(int family, int variant, int rows, int bm, int bn, long n_tiles, long grid) {
    GemmPlan p;
    p.family = family; p.variant = variant; p.rows = rows; p.bm = bm; p.bn = bn; p.n_tiles = (int)n_tiles; p.grid = (int)grid;
    return p;
}

// Small launches: the k range cut over several CUs, deterministic in-kernel reduction (gemm_splitk.hip).  0 = that kernel takes the
// launch (p: its geometry), 1 = not applicable (the caller falls through to the persistent kernel).
inline int plan_gemm_splitk(const GemmArgs& a, int slots, GemmPlan& p) {
    if (!a.sk_ws || !a.sk_counters) return 1;
    const long nbm = (a.M + 63) / 64, nbn = (a.N + 63) / 64, T = nbm * nbn;
    const int total = a.K / BK;                                      // k-slices
    if (total < 4 || T > slots / 2 || (a.sk_max_tiles > 0 && T > a.sk_max_tiles)) return 1;      // at least two parts of >= 2 slices, and room for them
    // as many parts as fill the resident slots once, each at least two slices (64 of K) long
    int ks = (int)std::min<long>(total / 2, std::max<long>(1, slots / T));
    ks = std::min(ks, 16);
    if (ks < 2) return 1;
    const int slices = (total + ks - 1) / ks;
    ks = (total + slices - 1) / slices;                              // no empty parts
    if ((size_t)T * ks * 4096 > a.sk_ws_floats || (size_t)T > a.sk_n_counters) return 1;
    const GemmPick pick = gemm_splitk_pick(a, a.relu_a);
    if (pick.index < 0) return 1;
    p.family = GemmPlan::SPLITK; p.variant = pick.index; p.rows = a.M; p.bm = p.bn = 64; p.ks = ks; p.slices = slices;
    p.n_tiles = (int)T; p.grid = (int)((T + 7) / 8) * 8 * ks;
    return 0;
}

// The first launch of a GEMM (launch_gemm plans the rows it leaves as a problem of their own).  Pure: no HIP call, no state; which
// operand combinations a kernel takes is the pick of its list above.  G: resident 256-thread blocks at two per CU.
inline GemmPlan plan_gemm(const GemmArgs& a, int G) {
    GemmPlan p;
    if (a.sk_ws && !a.clock_probe && plan_gemm_splitk(a, G, p) == 0) return p;     // small launch: k range spread over otherwise idle CUs
    const int G1 = G / 2;
    // Large M; exact fp32, single-rounding bf16 with half-row operands or split-bf16 with split-pair operands (gemm_p8_pick): the full rounds of 256 x 256 tiles go to
    // the 8-phase kernel (gemm_bf16_p8.hip: one 8-wave block per CU), the remaining row panels to the kernels below
    const GemmPick p8 = gemm_p8_pick(a);
    if (p8.index >= 0 && !a.no_dma && !a.no_ring && !a.no_p8 && !a.clock_probe && a.K % 128 == 0 &&
        offsets32(a.M, a.lda) && offsets32(a.M, a.ldc) && offsets32(a.N, a.ldw)) {
        // (a last, partly filled panel rides along with a partial round: rows past M read as zeros through the buffer descriptors,
        //  their stores are dropped by them, additive operands clamp the row -- round 5: the 120-row remainder of the cfg 5 scene
        //  no longer is a launch of its own)
        const long nbn = a.N / 256, full = a.M / 256, panels = full + (a.M % 256 ? 1 : 0), rounds = full * nbn / G1;
        long main_panels = rounds * G1 / nbn;
        // less than one round left (the tail of a big launch, or a medium-sized one): a partial round costs a whole tile time
        // (one tile per CU), the 128 x 128 kernels ~0.7 (fp32) / ~0.5 (bf16) of it per full round of tiles -- from 5/8 of a
        // round on this kernel is the faster one
        // (single-rounding bf16: a tile is 17-30 us against 8 + 0.4-0.7 us per tile-equivalent on the small kernels -- from 32 tiles on
        //  the partial round wins; the cfg 5 scene's 7 032 remainder rows = 54 tiles took 27.7 us per launch on 64 x 64 tiles, as long
        //  as the full round in front of them: profiles/r05_cfg5_bf16_mixed_kernel_stats_serial.md)
        const long part_min = a.p8_part_min > 0 ? a.p8_part_min : a.prec == 1 ? 32 : (G1 * 5) / 8;          // tiles from which a partial round beats the small kernels
        // ... and from which the REMAINDER behind full rounds rides along as one more (balanced) round instead of a tail launch.  Round 6,
        // interleaved A/B at the bench batch (profiles/r06_probes/ab_p8_part_min_*.txt): single-rounding bf16 from 12 tiles on (the
        // 12 / 24 remainder tiles of every N = 512 / 1024 launch: bf16_mixed 10127-10139 -> 10518-10565 scenes/s, +4 % -- a fourth
        // round on 208 of the 256 CUs costs what the tail launch cost, but it is one dependent launch less per GEMM and leaves 48 CUs
        // to the other lanes); split-bf16 from 24 on (+1.2 %; with 12 only +0.5 %: its tiles are three times as long); exact fp32
        // keeps 5/8 of a round (24: -1.7 %, 12: -10 %: a tile is 131 us there)
        const long rem_min = a.p8_part_min > 0 ? a.p8_part_min : a.prec == 1 ? 12 : a.prec == 3 ? 24 : (G1 * 5) / 8;
        if (main_panels == 0 && panels * nbn >= part_min) main_panels = panels;
        // Full rounds followed by a remainder that would be a partial round of its own (the cfg 5 scene: 312 tiles = 1.2 rounds at
        // N = 512, 624 = 2.4 at N = 1024): ONE launch of rounds + 1 BALANCED rounds on T / (rounds + 1) blocks instead of a full and a
        // partial launch -- the same number of tile times, one launch skeleton less, and the CUs it leaves out are free for the other
        // lanes' kernels (round 5: kproj 41.7 -> 30.1 us, nn_edge.2 64.7 -> 48.6 at E = 39 800; cfg 5 step +3 %)
        if (rounds >= 1 && main_panels > 0 && main_panels < panels && (panels - main_panels) * nbn >= rem_min) {
            const long step = 8 * nbn, g2 = ((panels * nbn + rounds) / (rounds + 1) + step - 1) / step * step;
            if (g2 <= G1 && gemm_p8_geometry_ok(a.M, a.N, panels * nbn, g2)) return big_plan(GemmPlan::P8, p8.index, a.M, 256, 256, panels * nbn, g2);
        }
        if (main_panels > 0) {
            const int rows = (int)std::min<long>(main_panels * 256, a.M);
            if (gemm_p8_geometry_ok(rows, a.N, main_panels * nbn, G1)) return big_plan(GemmPlan::P8, p8.index, rows, 256, 256, main_panels * nbn, G1);
        }
    }
    // bf16 modes, large M: the full rounds go to the 3-stage ring kernel (gemm_bf16_ring.hip: one 8-wave block per CU,
    // 256 x 128 tiles, two slices in flight), the remaining row panels to the kernels below
    if ((a.prec == 1 || a.prec == 3) && !a.no_dma && !a.no_ring && a.N > 64 && offsets32(a.M, a.lda) && offsets32(a.N, a.ldw)) {
        // (experiments build: 128 x 256 tiles when N is a multiple of 256 and they still make full rounds -- half the A bytes per flop)
        for (int rbn = (kGemmLab && a.ring_wide && a.N % 256 == 0) ? 256 : 128; rbn >= 128; rbn -= 128) {
            const int rbm = 32768 / rbn;
            const long nbm = (a.M + rbm - 1) / rbm, nbn = (a.N + rbn - 1) / rbn;
            const long main_panels = nbm * nbn / G1 * G1 / nbn;
            if (main_panels <= 0) continue;
            const GemmPick ring = gemm_ring_pick(a, rbn);
            if (ring.index >= 0) return big_plan(GemmPlan::RING, ring.index, (int)std::min<long>(main_panels * rbm, a.M), rbm, rbn, main_panels * nbn, G1);
            break;
        }
    }
    // (experiment switch: the tile the sweep asks for, 1..7 -- 5, 6, 7: four 64 x 64, three 64 x 128, three 64 x 64 blocks per CU)
    constexpr int forced[7][3] = {{128, 128, 2}, {128, 64, 2}, {64, 128, 2}, {64, 64, 2}, {64, 64, 4}, {64, 128, 3}, {64, 64, 3}};
    if (a.force_tile >= 1 && a.force_tile <= 7) return plan_tiled(a, G, forced[a.force_tile - 1][0], forced[a.force_tile - 1][1], forced[a.force_tile - 1][2]);
    auto blocks = [&](int bm, int bn) { return (long)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn); };
    // split-bf16 node-row launches with 1024..2048 output columns (self-attention QKV, cross-attention KV at the bench batch):
    // one round of 64 x 128 tiles beats two rounds of 64 x 64 by 6-8 us per launch (tools/gemm_tile_sweep.py, round 4:
    // 30.1 -> 24.2 us and 29.4 -> 22.0 us; every other node-row shape is best on what the rule below picks, fp32 within 2-4 us)
    if (a.prec == 3 && !a.a_split && a.N >= 1024 && a.N <= 2048 && blocks(64, 128) <= G && blocks(64, 128) >= G / 2)
        return plan_tiled(a, G, 64, 128);
    // Largest tile that still gives every resident slot a tile; small problems (and the tails
    // of big ones) take smaller tiles so the launch covers as many CUs as the problem allows.
    if (a.N > 64 && blocks(128, 128) >= G) return plan_tiled(a, G, 128, 128);
    if (a.N <= 64 && blocks(128, 64) >= G) return plan_tiled(a, G, 128, 64);
    if (a.N > 64 && blocks(64, 128) >= G) return plan_tiled(a, G, 64, 128);
    // exact fp32 on 64 x 64 tiles over more than one round of two blocks per CU (node rows of a batch: QKV 960 tiles, KV 640,
    // the node-side projection 2080): the kernel holds 80 VGPRs and 32 KB of LDS, so four blocks fit a CU and these latency-bound
    // launches take the wider grid -- KV 42.6 -> 31.0 us, QKV 46.5 -> 39.9, wnode 90.3 -> 78.9 (tools/gemm_tile_sweep.py, round 4)
    if (a.prec == 0 && blocks(64, 64) > G) return plan_tiled(a, G, 64, 64, 4);
    return plan_tiled(a, G, 64, 64);
}

// ---- two problems, one launch (one-scene plans, round 6) ----
inline bool twin_shapes(const GemmArgs& a, const GemmArgs& b) {
    return a.M == b.M && a.N == b.N && a.K == b.K && a.lda == b.lda && a.ldw == b.ldw && a.ldc == b.ldc && a.ldr == b.ldr &&
           a.ldg0 == b.ldg0 && a.ldg1 == b.ldg1 && a.act == b.act && a.prec == b.prec && a.a_split == b.a_split && a.r_split == b.r_split &&
           a.c_split == b.c_split && a.c_scale == b.c_scale && a.resid_scale == b.resid_scale && !a.bias == !b.bias && !a.resid == !b.resid &&
           !a.g0 == !b.g0 && !a.g1 == !b.g1 && !a.rowscale == !b.rowscale && a.no_dma == b.no_dma && a.no_ring == b.no_ring &&
           a.no_p8 == b.no_p8 && !a.a_pair && !a.c_pair && !b.a_pair && !b.c_pair && a.k_rot == b.k_rot && a.c_f16_cols == b.c_f16_cols && a.g_f16 == b.g_f16 && a.half_f16 == b.half_f16 && !a.force_tile && !b.force_tile && !a.ablate && !b.ablate && a.prefetch == b.prefetch;
}
inline bool same_plan(const GemmPlan& p, const GemmPlan& q) {
    return p.family == q.family && p.rows == q.rows && p.bm == q.bm && p.bn == q.bn && p.ksl == q.ksl && p.slot_mult == q.slot_mult &&
           p.ks == q.ks && p.slices == q.slices && p.n_tiles == q.n_tiles && p.grid == q.grid;
}
// The one launch that runs problems a and b together (variant: the row of the pair, which takes the staging pipe that can apply ReLU
// to A if either problem needs it), or a plan with variant = -1 for "not pairable": invalid or different problems, plans of launch_gemm
// that are not the same single launch of a kernel with a twin form (split-K; one round of 64 x 64 tiles at two blocks per CU with two
// k-slices per step), twins that share a split-K workspace, or the clock probe (both problems' blocks would write the same probe rows).
inline GemmPlan gemm_pair_plan(const GemmArgs& a, const GemmArgs& b, int G, bool clock_probe_set) {
    GemmPlan p;
    if (gemm_invalid(a) || gemm_invalid(b) || a.M <= 0 || a.N <= 0 || !twin_shapes(a, b) || clock_probe_set) return p;
    p = plan_gemm(a, G);
    const bool splitk = p.family == GemmPlan::SPLITK;
    const bool twin_form = p.rows == a.M && (splitk || (p.family == GemmPlan::TILED && p.bm == 64 && p.bn == 64 && p.ksl == 2 && p.slot_mult == 2));
    // b's own plan too: twin_shapes leaves out what may differ between the twins (ReLU-on-A), and each problem must run what it would alone
    const bool pairable = twin_form && same_plan(p, plan_gemm(b, G)) && !(splitk && (b.sk_ws == a.sk_ws || b.sk_counters == a.sk_counters));
    p.variant = !pairable ? -1 : (splitk ? gemm_splitk_pick(a, a.relu_a || b.relu_a) : gemm_tiled_pick(a, a.relu_a || b.relu_a, true)).index;
    return p;
}

}  // namespace vlsat
