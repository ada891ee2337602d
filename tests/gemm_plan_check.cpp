// Host-only check of csrc/gemm_plan.h (built with g++ by tests/host_check.py; opens no device): the planner and the four variant
// lists against the planner and the four launcher dispatches the library had before the lists existed, over whole launch sequences.
// Prints one "name -> ok ..." line per check and exits 1 at the first failure; "bench" prints the launch sequences of the bench
// batch's shapes as "table | ..." lines.  With -DVLSAT_EXPERIMENTS the lists have the lab rows and the lab switches are enumerated too.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "gemm_plan.h"

namespace {

// what one launch is: the plan that led to it, the kernel (family letter and template arguments) and the launch geometry
struct Rec {
    int family = -1, rows = 0, bm = 0, bn = 0, ksl = 0, slot_mult = 0, ks = 0, slices = 0, n_tiles = 0, grid = 0;      // the plan
    char kernel = '?';                                      // 'T' gemm_f32_kernel, 'P' gemm_p8_kernel, 'R' gemm_ring_kernel, 'S' gemm_splitk_kernel
    int targ[6] = {0, 0, 0, 0, 0, 0};                       // its template arguments in order
    int gx = 0, gy = 0, block = 0, k_tiles = 0, k_nbn = 0, k_ks = 0, k_slices = 0, M = 0;      // grid, block, kernel arguments, rows of the problem handed in
    bool operator==(const Rec& o) const {
        return family == o.family && rows == o.rows && bm == o.bm && bn == o.bn && ksl == o.ksl && slot_mult == o.slot_mult && ks == o.ks &&
               slices == o.slices && n_tiles == o.n_tiles && grid == o.grid && kernel == o.kernel && !memcmp(targ, o.targ, sizeof targ) &&
               gx == o.gx && gy == o.gy && block == o.block && k_tiles == o.k_tiles && k_nbn == o.k_nbn && k_ks == o.k_ks &&
               k_slices == o.k_slices && M == o.M;
    }
};
struct Run {                        // a whole launch_gemm / launch_gemm_pair call: return code, error text, launches in order
    int rc = 0;
    const char* error = nullptr;
    std::vector<Rec> launches;
};
Run g_run;
Rec g_plan;                         // the plan noted before the launch it leads to
int g_G = 512;                      // resident slots of the "device"

}  // namespace

// ---- the frozen oracle: host code of commit 0cd5cf4, word for word -- kernels.h (Act .. launch_gemm_p8), gemm_core.h (offsets32,
//      gemm_pipe_prec), gemm_splitk.hip, gemm_bf16_ring.hip and gemm_bf16_p8.hip (from the end of the kernel), gemm_f32.hip (from
//      launch_t; slots() answers g_G).  A "kernel" here returns its own template arguments, a "launch" records them with grid, block
//      and kernel arguments, fail() records the text; launch_plan also notes the plan it was handed. ----
namespace legacy {

typedef void* hipStream_t;
struct dim3 { int x, y; dim3(int x_, int y_ = 1) : x(x_), y(y_) {} };
struct Kern { char kernel; int targ[6]; };
template <int BM, int BN, int ADD, int PREC, int KSL, bool TWIN = false> Kern gemm_f32_kernel() { return {'T', {BM, BN, ADD, PREC, KSL, TWIN}}; }
template <int MODE, int ADD, bool RELU, int CF, int ABL = 0> Kern gemm_p8_kernel() { return {'P', {MODE, ADD, RELU, CF, ABL, 0}}; }
template <int TERMS, int AFMT, int ADD, int RBN, int RBK = 32, bool DB = false> Kern gemm_ring_kernel() { return {'R', {TERMS, AFMT, ADD, RBN, RBK, DB}}; }
template <int PREC, bool TWIN = false> Kern gemm_splitk_kernel() { return {'S', {PREC, TWIN, 0, 0, 0, 0}}; }
struct GemmArgs;
void record(const Kern& k, dim3 grid, dim3 block, int M, int n_tiles, int nbn, int ks = 0, int slices = 0) {
    Rec r = g_plan;
    r.kernel = k.kernel;
    memcpy(r.targ, k.targ, sizeof r.targ);
    r.gx = grid.x; r.gy = grid.y; r.block = block.x; r.k_tiles = n_tiles; r.k_nbn = nbn; r.k_ks = ks; r.k_slices = slices; r.M = M;
    g_run.launches.push_back(r);
}
template <class A> void record(const Kern& k, dim3 grid, dim3 block, const A& a, int n_tiles, int nbn) { record(k, grid, block, a.M, n_tiles, nbn); }
template <class A> void record(const Kern& k, dim3 grid, dim3 block, const A& a, const A&, int n_tiles, int nbn) { record(k, grid, block, a.M, n_tiles, nbn); }
template <class A> void record(const Kern& k, dim3 grid, dim3 block, const A& a, const A&, int n_tiles, int nbn, int ks, int slices, float*, unsigned*, float*, unsigned*) {
    record(k, grid, block, a.M, n_tiles, nbn, ks, slices);
}
#define hipLaunchKernelGGL(kernel, grid, blk, shmem, stream, ...) record((kernel)(), grid, blk, __VA_ARGS__)
#define fail(code, text) (g_run.error = text, code)
#define VLSAT_LAUNCH_CHECK(what) (void)0
static int slots() { return g_G; }
static long long* g_clock_probe = nullptr;

// ---- kernels.h ----
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
    int ring_wide = 0;                          // experiment: bf16 ring kernel with 128 x 256 tiles where N allows (measured equal)
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
};
int launch_gemm(const GemmArgs& a, hipStream_t s);
// The first launch of a GEMM as the planner of launch_gemm (gemm_f32.hip plan_gemm) chooses it: kernel family, geometry, and the
// rows [0, rows) it covers -- the rows after them are planned again as a problem of their own (the tail).
struct GemmPlan {
    enum Family { SPLITK, P8, RING, TILED };
    int family = TILED;
    int rows = 0;
    int bm = 64, bn = 64;           // output tile (8-phase: 256 x 256; ring: 32768 / bn x bn)
    int ksl = 1, slot_mult = 2;     // persistent kernel: k-slices per pipeline step, resident blocks per CU its grid is sized for
    int ks = 0, slices = 0;         // split-K: parts of the k range, k-slices per part
    int n_tiles = 0, grid = 0;
};
// small launches: k range cut over several CUs, deterministic in-kernel reduction.  plan: 0 = this kernel takes the launch (p),
// 1 = not applicable; launch: runs the plan, twin = a second problem whose own plan is p in the same launch (1 = not pairable)
int plan_gemm_splitk(const GemmArgs& a, int slots, GemmPlan& p);
int launch_gemm_splitk(const GemmArgs& a, const GemmPlan& p, hipStream_t s, const GemmArgs* twin = nullptr);
// two problems of the same shape and flags in ONE launch (round 6: the 3D / 2D twins of a one-scene forward): 0 = launched,
// 1 = not pairable: invalid or different problems, or plans of launch_gemm that are not the same single launch of a kernel with a
// twin form (split-K, one round of 64 x 64 tiles at two k-slices per step).  The caller then launches them one after the other;
// results are bit-identical either way
int launch_gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t s);
constexpr size_t SPLITK_WS_FLOATS = (size_t)768 * 4096;    // room for 768 partial 64 x 64 tiles (12 MB)
constexpr size_t SPLITK_COUNTERS = 512;
// bf16 modes, full rounds of large-M launches: 3-stage LDS ring, 256 x 128 tiles, one 8-wave block per CU
// (gemm_bf16_ring.hip); returns 1 if the operand combination is not built.  dry: decide only (the planner), launch nothing
int launch_gemm_ring(const GemmArgs& a, int rbn, int n_tiles, int grid, hipStream_t s, bool dry = false);   // rbn: tile width 128 | 256
// full rounds of large-M launches, exact fp32 or single-rounding bf16 with half-row A: 256 x 256 tiles, 8-phase pipeline,
// one 8-wave block per CU (gemm_bf16_p8.hip); needs N % 256 == 0, K % 128 == 0; returns 1 if the combination is not built.
// dry: decide only (the planner), launch nothing
int launch_gemm_p8(const GemmArgs& a, int n_tiles, int grid, hipStream_t s, bool dry = false);

// ---- gemm_core.h ----
constexpr int BK = 32;    // k-slice held in LDS per pipeline stage
// the byte offsets of rows [0, rows + 256) of an operand with a pitch of ld floats fit in 32 bits (LDS-direct loads, buffer descriptors)
inline bool offsets32(size_t rows, size_t ld) { return (rows + 256) * ld * 4 < (1ull << 32); }

// PipeSel code of the persistent (gemm_f32.hip) and split-K (gemm_splitk.hip) kernels for a launch's operands: exact fp32 without
// ReLU-on-A and the bf16 modes take the LDS-direct pipes (codes 4..15) where the operands allow it; -1 = no pipe (*why: the reason).
// relu_a: ReLU-on-A of the launch -- of either problem of a pair, which then both take the staging pipe (same products).
// add_modes: the LDS-direct pipes only for the additive modes the persistent kernel instantiates them for (none, residual, both
// gathered rows); the split-K kernel has every mode on every pipe.
inline int gemm_pipe_prec(const GemmArgs& a, bool relu_a, bool add_modes, const char** why = nullptr) {
    const int add = (a.resid ? 1 : 0) | (a.g0 ? 2 : 0) | (a.g1 ? 4 : 0);
    const bool dma_ok = !a.no_dma && (!add_modes || add == 0 || add == 1 || add == 6) && offsets32(a.M, a.lda) && offsets32(a.N, a.ldw);
    int prec = a.prec;
    if (prec == 0 && dma_ok && !relu_a) prec = 4;
    if (a.a_split == 2 && !(prec == 1 && dma_ok)) {
        if (why) *why = "gemm: half-row A needs the single-rounding bf16 precision and the LDS-direct pipe";
        return -1;
    }
    if ((prec == 1 || prec == 3) && dma_ok) return prec + (a.a_split == 2 ? (a.half_f16 ? 14 : 12) : a.a_split ? 8 : 4);   // bf16 modes: A split on the fragment-read side, so ReLU-on-A is fine
    if (a.a_split) {
        if (why) *why = "gemm: split-pair A needs a bf16 precision and the LDS-direct pipe";
        return -1;
    }
    return prec;
}


// ---- gemm_splitk.hip ----
// Decides whether the launch is one of the small ones this kernel is for: 0 = yes (p: its geometry), 1 = not applicable (the caller
// falls through to the persistent kernel).
int plan_gemm_splitk(const GemmArgs& a, int slots, GemmPlan& p) {
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
    if (gemm_pipe_prec(a, a.relu_a, false) < 0) return 1;
    p.family = GemmPlan::SPLITK;
    p.rows = a.M;
    p.bm = p.bn = 64;
    p.ks = ks;
    p.slices = slices;
    p.n_tiles = (int)T;
    p.grid = (int)((T + 7) / 8) * 8 * ks;
    return 0;
}

// twin: a second problem of the same shape and flags whose own plan is p (launch_gemm_pair has checked both), in the same launch:
// each problem is computed as it would be alone.
int launch_gemm_splitk(const GemmArgs& a, const GemmPlan& p, hipStream_t s, const GemmArgs* twin) {
    if (twin && (twin->sk_ws == a.sk_ws || twin->sk_counters == a.sk_counters)) return 1;
    const GemmArgs& b = twin ? *twin : a;
    const int nbn = (a.N + 63) / 64;
    // (a pair takes the staging pipe that can apply ReLU to A if either needs it: same products)
#define VLSAT_SK_CASE(PREC) \
    case PREC: \
        if (twin) hipLaunchKernelGGL((gemm_splitk_kernel<PREC, true>), dim3(p.grid, 2), dim3(256), 0, s, a, b, p.n_tiles, nbn, p.ks, p.slices, a.sk_ws, a.sk_counters, b.sk_ws, b.sk_counters); \
        else hipLaunchKernelGGL((gemm_splitk_kernel<PREC, false>), dim3(p.grid), dim3(256), 0, s, a, a, p.n_tiles, nbn, p.ks, p.slices, a.sk_ws, a.sk_counters, a.sk_ws, a.sk_counters); \
        break;
    switch (gemm_pipe_prec(a, a.relu_a || b.relu_a, false)) {
        VLSAT_SK_CASE(0) VLSAT_SK_CASE(1) VLSAT_SK_CASE(3) VLSAT_SK_CASE(4) VLSAT_SK_CASE(5) VLSAT_SK_CASE(7)
        VLSAT_SK_CASE(9) VLSAT_SK_CASE(11) VLSAT_SK_CASE(13) VLSAT_SK_CASE(15)
        default: return 1;
    }
#undef VLSAT_SK_CASE
    if (a.launches) ++*a.launches;
    VLSAT_LAUNCH_CHECK("gemm_splitk");
    return 0;
}


// ---- gemm_bf16_ring.hip ----
template <int T, int S, int ADD>
static void ring_launch(bool wide, const GemmArgs& a, int n_tiles, int nbn, int grid, hipStream_t s) {
    if constexpr (T == 1 && S >= 2) {          // half-row A, one plane: 64-wide slices whenever K allows
        if (!wide && a.K % 128 == 0 && !a.ring_bk32 && !a.ring_nodb) {
            hipLaunchKernelGGL((gemm_ring_kernel<T, S, ADD, 128, 64, true>), dim3(grid), dim3(512), 0, s, a, n_tiles, nbn);
            return;
        }
        if (!wide && a.K % 64 == 0 && !a.ring_bk32) {
            hipLaunchKernelGGL((gemm_ring_kernel<T, S, ADD, 128, 64>), dim3(grid), dim3(512), 0, s, a, n_tiles, nbn);
            return;
        }
    }
    if (!wide) hipLaunchKernelGGL((gemm_ring_kernel<T, S, ADD, 128>), dim3(grid), dim3(512), 0, s, a, n_tiles, nbn);
    else hipLaunchKernelGGL((gemm_ring_kernel<T, S, ADD, 256>), dim3(grid), dim3(512), 0, s, a, n_tiles, nbn);
}

// full rounds of a large-M bf16 launch; returns 1 if this operand combination is not built (the caller then uses the
// 128 x 128 kernel for everything); dry: decide only
int launch_gemm_ring(const GemmArgs& a, int rbn, int n_tiles, int grid, hipStream_t s, bool dry) {
    const int add = (a.resid ? 1 : 0) | (a.g0 ? 2 : 0) | (a.g1 ? 4 : 0);
    if (a.rowscale || (add != 0 && add != 1 && add != 6)) return 1;
    const bool wide = rbn == 256;
    const int nbn = (a.N + rbn - 1) / rbn;
#define VLSAT_RING(T, S, ADD) do { if (!dry) ring_launch<T, S, ADD>(wide, a, n_tiles, nbn, grid, s); } while (0)
#define VLSAT_RING_ADD(T, S)                      \
    switch (add) {                                \
        case 0: VLSAT_RING(T, S, 0); break;       \
        case 1: VLSAT_RING(T, S, 1); break;       \
        default: VLSAT_RING(T, S, 6); break;      \
    }
    if (a.prec == 3) {
        if (a.a_split == 2) return 1;
        if (a.a_split) { VLSAT_RING_ADD(3, 1) } else { VLSAT_RING_ADD(3, 0) }
    } else {
        if (a.a_split == 2 && a.half_f16) { VLSAT_RING_ADD(1, 3) } else if (a.a_split == 2) { VLSAT_RING_ADD(1, 2) } else if (a.a_split) { VLSAT_RING_ADD(1, 1) } else { VLSAT_RING_ADD(1, 0) }
    }
#undef VLSAT_RING_ADD
#undef VLSAT_RING
    if (dry) return 0;
    if (a.launches) ++*a.launches;
    VLSAT_LAUNCH_CHECK("gemm_bf16_ring");
    return 0;
}


// ---- gemm_bf16_p8.hip ----
constexpr int P8_BM = 256, P8_BN = 256, P8_BK = 64;
// full rounds of a large-M launch on 256 x 256 tiles: half-row bf16 operands (prec 1), exact fp32 (prec 0) or split-bf16
// on split-pair operands (prec 3); 1 = operand combination not built (the caller falls back to the older kernels); dry: decide only
int launch_gemm_p8(const GemmArgs& a, int n_tiles, int grid, hipStream_t s, bool dry) {
    const int add = (a.resid ? 1 : 0) | (a.g0 ? 2 : 0) | (a.g1 ? 4 : 0);
    const bool f32 = a.prec == 0, x3 = a.prec == 3;
    if (a.rowscale || a.act == ACT_SIGMOID || (add != 0 && add != 1 && add != 6)) return 1;
    // the fp32 / split-bf16 epilogues read the bias as float4 (the half-row one as scalars): an unaligned bias pointer of a
    // caller of vlsat_k_gemm goes to the older kernels, which have the scalar fallback
    if ((f32 || x3) && a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 15)) return 1;
    // (round 4, measured and dropped: loading the accumulator inits of the wave tile's second row half one phase later, under
    //  the MFMAs of phases 1 / 2 -- fp32 nn_edge.0 + gathered rows 923 vs 917 us, out-projection + residual 480 vs 483: the
    //  cost of additive operands is not latency at the start of a tile; it is consistent with every CU pulling its 256-512 KB at the same
    //  moment: 64-128 MB per round of tiles at what the memory system delivers)
    if (f32 ? (a.a_split || a.c_split || a.r_split || a.c_scale != 1.f)
            : x3 ? (a.a_split != 1 || a.c_split == 2 || !a.Wlo) : (a.prec != 1 || a.a_split != 2 || a.c_split == 1)) return 1;
    const int kt = (f32 || x3) ? 32 : P8_BK;          // an output tile is an even number (>= 4) of K-tiles
    // (M need not be a multiple of the tile: the last panel's rows past M are outside every buffer descriptor -- loads return zeros,
    //  stores are dropped -- and tile_init clamps the row of an additive operand)
    if (a.N % P8_BN || a.K % (2 * kt) || a.K < 4 * kt || n_tiles > (long)((a.M + P8_BM - 1) / P8_BM) * (a.N / P8_BN)) return 1;
    const int nbn = a.N / P8_BN;
    if (grid % 8 || (grid / 8) % nbn) return 1;      // the kernel keeps one column tile per block (bias registers)
#define VLSAT_P8_K(...) do { if (!dry) hipLaunchKernelGGL((gemm_p8_kernel<__VA_ARGS__>), dim3(grid), dim3(512), 0, s, a, n_tiles, nbn); } while (0)
#define VLSAT_P8(MODE, ADD, RELU, CF) VLSAT_P8_K(MODE, ADD, RELU, CF)
#define VLSAT_P8_ABL(X) VLSAT_P8_K(0, 0, false, 2, X)
    const bool c16 = a.c_f16_cols > 0;            // (the whole output as fp16 half rows: half-row launches only)
    if (c16 && (a.c_f16_cols != a.N || f32 || x3 || a.c_split)) return 1;
    if (a.half_f16 && (f32 || x3 || a.c_split)) return 1;         // (fp16 operands: half-row launches; their half-row outputs come as c_f16_cols == N)
    const int key = add * 4 + (a.relu_a ? 2 : 0) + (a.c_split ? 1 : 0);
    if (f32) {
        switch (key) {
            case 0: VLSAT_P8(1, 0, false, 0); break;
            case 2: VLSAT_P8(1, 0, true, 0); break;
            case 4: VLSAT_P8(1, 1, false, 0); break;
            case 24: VLSAT_P8(1, 6, false, 0); break;
            case 26: VLSAT_P8(1, 6, true, 0); break;
            default: return 1;
        }
    } else if (x3) {
        switch (key) {
            case 0: VLSAT_P8(2, 0, false, 0); break;
            case 1: VLSAT_P8(2, 0, false, 1); break;
            case 2: VLSAT_P8(2, 0, true, 0); break;
            case 3: VLSAT_P8(2, 0, true, 1); break;
            case 4: VLSAT_P8(2, 1, false, 0); break;
            case 25: VLSAT_P8(2, 6, false, 1); break;
            case 27: VLSAT_P8(2, 6, true, 1); break;
            default: return 1;
        }
#ifdef VLSAT_EXPERIMENTS
    } else if (a.ablate && key == 27) {               // timing experiments on the gathered-row launch
        switch (a.ablate) {
            case 1: VLSAT_P8_K(0, 6, true, 2, 256); break;
            default: VLSAT_P8_K(0, 6, true, 2, 512); break;
        }
    } else if (a.ablate && key == 1) {                // timing experiments (tools/p8_check.py --ablate)
        switch (a.ablate) {
            case 1: VLSAT_P8_ABL(1); break;
            case 2: VLSAT_P8_ABL(2); break;
            case 3: VLSAT_P8_ABL(3); break;
            case 4: VLSAT_P8_ABL(4); break;
            case 6: VLSAT_P8_ABL(6); break;
            case 7: VLSAT_P8_ABL(7); break;
            case 8: VLSAT_P8_ABL(8); break;
            case 5: VLSAT_P8_ABL(5); break;
            case 37: VLSAT_P8_ABL(37); break;
            case 65: VLSAT_P8_ABL(65); break;
            default: VLSAT_P8_ABL(15); break;
        }
#endif
    } else {
        if (a.half_f16) {                     // MODE 3: fp16 operands; output fp32 (CF 0) or fp16 half rows (CF 3)
            switch (add * 4 + (a.relu_a ? 2 : 0) + (c16 ? 1 : 0)) {
                case 0: VLSAT_P8(3, 0, false, 0); break;
                case 1: VLSAT_P8(3, 0, false, 3); break;
                case 2: VLSAT_P8(3, 0, true, 0); break;
                case 3: VLSAT_P8(3, 0, true, 3); break;
                case 25: VLSAT_P8(3, 6, false, 3); break;
                case 27: VLSAT_P8(3, 6, true, 3); break;
                default: return 1;
            }
        } else
        switch (key) {
            case 0: if (c16) VLSAT_P8(0, 0, false, 3); else VLSAT_P8(0, 0, false, 0); break;
            case 1: VLSAT_P8(0, 0, false, 2); break;
            case 2: VLSAT_P8(0, 0, true, 0); break;
            case 3: VLSAT_P8(0, 0, true, 2); break;
            case 4: VLSAT_P8(0, 1, false, 0); break;
            case 5: VLSAT_P8(0, 1, false, 2); break;
            case 25: VLSAT_P8(0, 6, false, 2); break;
            case 27: VLSAT_P8(0, 6, true, 2); break;
            default: return 1;
        }
    }
#undef VLSAT_P8_ABL
#undef VLSAT_P8
#undef VLSAT_P8_K
    if (dry) return 0;
    if (a.launches) ++*a.launches;
    VLSAT_LAUNCH_CHECK("gemm_p8");
    return 0;
}


// ---- gemm_f32.hip ----
// persistent kernel on BM x BN tiles; TWIN: problems a and b in one launch (grid.y = 2; launch_gemm_pair) -- 1 = not pairable,
// for everything a single launch would refuse and for the combinations that have no TWIN variant
template <int BM, int BN, int KSL = 1, bool TWIN = false>
static int launch_t(const GemmArgs& a, const GemmArgs& b, int n_tiles, int grid, hipStream_t s) {
    const int nbn = (a.N + BN - 1) / BN;
    const int add = (a.resid ? 1 : 0) | (a.g0 ? 2 : 0) | (a.g1 ? 4 : 0);
    auto refuse = [](const char* why) { return TWIN ? 1 : fail(-1, why); };
    if (a.prec == 0 && (a.a_split || a.r_split || a.c_split || a.c_scale != 1.f))
        return refuse("gemm: operand formats and c_scale exist in the bf16 modes only");      // (the fp32 kernels fold them away)
    const char* why = nullptr;
    const int prec = gemm_pipe_prec(a, a.relu_a || b.relu_a, true, &why);
    if (prec < 0) return refuse(why);
#define VLSAT_GEMM_CASE(ADD, PREC) \
    case (PREC) * 8 + (ADD): hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, ADD, PREC, KSL, TWIN>), dim3(grid, TWIN ? 2 : 1), dim3(256), 0, s, a, b, n_tiles, nbn); break;
#define VLSAT_GEMM_SINGLE(ADD, PREC) \
    case (PREC) * 8 + (ADD): if constexpr (TWIN) return 1; else hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, ADD, PREC, KSL>), dim3(grid), dim3(256), 0, s, a, b, n_tiles, nbn); break;
    switch (prec * 8 + add) {
        VLSAT_GEMM_CASE(0, 13) VLSAT_GEMM_CASE(1, 13) VLSAT_GEMM_CASE(6, 13)
        VLSAT_GEMM_CASE(0, 15) VLSAT_GEMM_CASE(6, 15)
        VLSAT_GEMM_CASE(0, 9) VLSAT_GEMM_CASE(1, 9) VLSAT_GEMM_CASE(6, 9)
        VLSAT_GEMM_CASE(0, 11) VLSAT_GEMM_CASE(1, 11) VLSAT_GEMM_CASE(6, 11)
        VLSAT_GEMM_CASE(0, 4) VLSAT_GEMM_CASE(1, 4) VLSAT_GEMM_CASE(6, 4)
        VLSAT_GEMM_CASE(0, 5) VLSAT_GEMM_CASE(1, 5) VLSAT_GEMM_CASE(6, 5)
        VLSAT_GEMM_CASE(0, 7) VLSAT_GEMM_CASE(1, 7) VLSAT_GEMM_CASE(6, 7)
        VLSAT_GEMM_CASE(0, 0) VLSAT_GEMM_CASE(1, 0) VLSAT_GEMM_SINGLE(2, 0) VLSAT_GEMM_SINGLE(3, 0)
        VLSAT_GEMM_SINGLE(4, 0) VLSAT_GEMM_SINGLE(5, 0) VLSAT_GEMM_CASE(6, 0) VLSAT_GEMM_SINGLE(7, 0)
        VLSAT_GEMM_SINGLE(0, 1) VLSAT_GEMM_SINGLE(1, 1) VLSAT_GEMM_SINGLE(6, 1)
        VLSAT_GEMM_SINGLE(0, 3) VLSAT_GEMM_SINGLE(1, 3) VLSAT_GEMM_SINGLE(6, 3)
        default: return refuse("gemm: this precision / additive-operand combination is not built");
    }
#undef VLSAT_GEMM_SINGLE
#undef VLSAT_GEMM_CASE
    if (a.launches) ++*a.launches;         // a logical GEMM is a main launch plus (usually) a small-tile tail launch
    VLSAT_LAUNCH_CHECK((TWIN ? "gemm_f32 (pair)" : "gemm_f32"));
    return 0;
}

// rows [row0, M) of the problem as a sub-problem
static GemmArgs tail_of(const GemmArgs& a, int row0) {
    GemmArgs t = a;
    t.A += (size_t)row0 * a.lda;
    t.C += (size_t)row0 * a.ldc;
    t.M = a.M - row0;
    if (a.rowscale) t.rowscale += row0;
    if (a.resid) t.resid += (size_t)row0 * a.ldr;
    if (a.gi0) t.gi0 += row0;
    if (a.gi1) t.gi1 += row0;
    return t;
}

// the persistent kernel on BM x BN tiles, a grid of slot_mult blocks per CU (G: resident slots at two per CU)
static GemmPlan plan_tiled(const GemmArgs& a, int G, int bm, int bn, int slot_mult = 2) {
    GemmPlan p;
    p.bm = bm;
    p.bn = bn;
    p.slot_mult = slot_mult;
    p.rows = a.M;
    const int Gs = G / 2 * slot_mult;
    const int nbm = (a.M + bm - 1) / bm, nbn = (a.N + bn - 1) / bn;
    const long T = (long)nbm * nbn;
    p.n_tiles = (int)T;
    if (T <= Gs) {                                  // one round: grid = tiles (rounded up to 8)
        p.grid = (int)((T + 7) / 8) * 8;
        // latency-bound: two k-slices per pipeline step (four per step measured no faster: tools/latency_probe.py, round 2)
        if (bm == 64 && bn == 64 && a.K % (2 * BK) == 0) p.ksl = 2;
        return p;
    }
    // full rounds with this tile; the remaining M-panels go to a smaller tile (see header)
    p.grid = Gs;
    const long main_panels = (T / Gs * Gs) / nbn;
    if (main_panels > 0 && main_panels < nbm && !(bm == 64 && bn == 64)) {
        p.rows = (int)(main_panels * bm);
        p.n_tiles = (int)(main_panels * nbn);
    }
    return p;
}

// the 8-phase / ring kernel on rows [0, rows)
static GemmPlan big_plan(int family, int rows, int bm, int bn, long n_tiles, long grid) {
    GemmPlan p;
    p.family = family;
    p.rows = rows;
    p.bm = bm;
    p.bn = bn;
    p.n_tiles = (int)n_tiles;
    p.grid = (int)grid;
    return p;
}

// The first launch of a GEMM (launch_gemm plans the rows it leaves as a problem of their own).  Pure: no HIP call, no state; the
// kernels with operand combinations they do not build (split-K, 8-phase, ring) decide for themselves whether they take a launch.
// G: resident 256-thread blocks at two per CU (slots()).
static GemmPlan plan_gemm(const GemmArgs& a, int G) {
    GemmPlan p;
    if (a.sk_ws && !a.clock_probe && plan_gemm_splitk(a, G, p) == 0) return p;     // small launch: k range spread over otherwise idle CUs
    const int G1 = G / 2;
    // Large M; exact fp32, single-rounding bf16 with half-row operands or split-bf16 with split-pair operands: the full rounds of 256 x 256 tiles go to the 8-phase
    // kernel (gemm_bf16_p8.hip: one 8-wave block per CU), the remaining row panels to the kernels below
    if (((a.prec == 1 && a.a_split == 2) || (a.prec == 3 && a.a_split == 1) || (a.prec == 0 && !a.a_split && !a.c_split && !a.r_split)) && !a.no_dma && !a.no_ring &&
        !a.no_p8 && !a.rowscale && !a.clock_probe && (!a.c_f16_cols || (a.c_f16_cols == a.N && a.prec == 1 && !a.resid && (a.half_f16 || (!a.g0 && !a.g1 && !a.relu_a)))) && a.N % 256 == 0 && a.K % 128 == 0 &&
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
            if (g2 <= G1 && launch_gemm_p8(a, (int)(panels * nbn), (int)g2, nullptr, true) == 0) return big_plan(GemmPlan::P8, a.M, 256, 256, panels * nbn, g2);
        }
        if (main_panels > 0) {
            GemmArgs m = a;
            m.M = (int)std::min<long>(main_panels * 256, a.M);
            if (launch_gemm_p8(m, (int)(main_panels * nbn), G1, nullptr, true) == 0) return big_plan(GemmPlan::P8, m.M, 256, 256, main_panels * nbn, G1);
        }
    }
    // bf16 modes, large M: the full rounds go to the 3-stage ring kernel (gemm_bf16_ring.hip: one 8-wave block per CU,
    // 256 x 128 tiles, two slices in flight), the remaining row panels to the kernels below
    if ((a.prec == 1 || a.prec == 3) && !a.no_dma && !a.no_ring && a.N > 64 && !a.rowscale && offsets32(a.M, a.lda) && offsets32(a.N, a.ldw)) {
        // 128 x 256 tiles when N is a multiple of 256 and they still make full rounds (half the A bytes per flop), else 256 x 128
        for (int rbn = (a.ring_wide && a.N % 256 == 0) ? 256 : 128; rbn >= 128; rbn -= 128) {
            const int rbm = 32768 / rbn;
            const long nbm = (a.M + rbm - 1) / rbm, nbn = (a.N + rbn - 1) / rbn;
            const long main_panels = nbm * nbn / G1 * G1 / nbn;
            if (main_panels <= 0) continue;
            GemmArgs m = a;
            m.M = (int)std::min<long>(main_panels * rbm, a.M);
            if (launch_gemm_ring(m, rbn, (int)(main_panels * nbn), G1, nullptr, true) == 0) return big_plan(GemmPlan::RING, m.M, rbm, rbn, main_panels * nbn, G1);
            break;
        }
    }
    switch (a.force_tile) {                       // (experiment switch: the tile the sweep asks for)
        case 1: return plan_tiled(a, G, 128, 128);
        case 2: return plan_tiled(a, G, 128, 64);
        case 3: return plan_tiled(a, G, 64, 128);
        case 4: return plan_tiled(a, G, 64, 64);
        case 5: return plan_tiled(a, G, 64, 64, 4);        // (experiment: four 64 x 64 blocks per CU)
        case 6: return plan_tiled(a, G, 64, 128, 3);       // (experiment: three 64 x 128 blocks per CU)
        case 7: return plan_tiled(a, G, 64, 64, 3);
        default: break;
    }
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

// the launch of a plan on rows [0, m.M) (m.M == p.rows)
static int launch_plan(const GemmArgs& m, const GemmPlan& p, hipStream_t s) {
    switch (p.family) {
        case GemmPlan::SPLITK: return launch_gemm_splitk(m, p, s);
        case GemmPlan::P8: return launch_gemm_p8(m, p.n_tiles, p.grid, s);
        case GemmPlan::RING: return launch_gemm_ring(m, p.bn, p.n_tiles, p.grid, s);
    }
    if (p.bm == 128) return p.bn == 128 ? launch_t<128, 128>(m, m, p.n_tiles, p.grid, s) : launch_t<128, 64>(m, m, p.n_tiles, p.grid, s);
    if (p.bn == 128) return launch_t<64, 128>(m, m, p.n_tiles, p.grid, s);
    return p.ksl == 2 ? launch_t<64, 64, 2>(m, m, p.n_tiles, p.grid, s) : launch_t<64, 64>(m, m, p.n_tiles, p.grid, s);
}


template <class P> void note_plan(const P& p) {
    g_plan = Rec{};
    g_plan.family = p.family; g_plan.rows = p.rows; g_plan.bm = p.bm; g_plan.bn = p.bn; g_plan.ksl = p.ksl; g_plan.slot_mult = p.slot_mult;
    g_plan.ks = p.ks; g_plan.slices = p.slices; g_plan.n_tiles = p.n_tiles; g_plan.grid = p.grid;
}
#define launch_plan(m, p, s) (note_plan(p), launch_plan(m, p, s))

// nullptr when launch_gemm takes the problem (an empty one included), else what it reports
static const char* gemm_invalid(const GemmArgs& a) {
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
    if (a.g_f16 && (a.resid || !(a.g0 || a.g1) || a.N % 256 || ((a.ldg0 | a.ldg1) & 1) || ((reinterpret_cast<uintptr_t>(a.g0) | reinterpret_cast<uintptr_t>(a.g1)) & 7)))
        return "gemm: g_f16 needs gathered rows, no residual, N % 256 == 0 and 8-byte aligned tables";
    return nullptr;
}

int launch_gemm(const GemmArgs& a_in, hipStream_t s) {
    GemmArgs a = a_in;
    a.clock_probe = g_clock_probe;
    if (const char* why = gemm_invalid(a)) return fail(-1, why);
    if (a.M <= 0 || a.N <= 0) return 0;
    const int G = slots();
    while (true) {
        const GemmPlan p = plan_gemm(a, G);
        if (p.rows == a.M) return launch_plan(a, p, s);
        GemmArgs m = a;
        m.M = p.rows;
        if (const int r = launch_plan(m, p, s)) return r;
        a = tail_of(a, p.rows);                 // strictly fewer rows: terminates
    }
}

// ---- two problems, one launch (one-scene plans, round 6) ----
static bool twin_shapes(const GemmArgs& a, const GemmArgs& b) {
    return a.M == b.M && a.N == b.N && a.K == b.K && a.lda == b.lda && a.ldw == b.ldw && a.ldc == b.ldc && a.ldr == b.ldr &&
           a.ldg0 == b.ldg0 && a.ldg1 == b.ldg1 && a.act == b.act && a.prec == b.prec && a.a_split == b.a_split && a.r_split == b.r_split &&
           a.c_split == b.c_split && a.c_scale == b.c_scale && a.resid_scale == b.resid_scale && !a.bias == !b.bias && !a.resid == !b.resid &&
           !a.g0 == !b.g0 && !a.g1 == !b.g1 && !a.rowscale == !b.rowscale && a.no_dma == b.no_dma && a.no_ring == b.no_ring &&
           a.no_p8 == b.no_p8 && a.k_rot == b.k_rot && a.c_f16_cols == b.c_f16_cols && a.g_f16 == b.g_f16 && a.half_f16 == b.half_f16 && !a.force_tile && !b.force_tile && !a.ablate && !b.ablate && a.prefetch == b.prefetch;
}
static bool same_plan(const GemmPlan& p, const GemmPlan& q) {
    return p.family == q.family && p.rows == q.rows && p.bm == q.bm && p.bn == q.bn && p.ksl == q.ksl && p.slot_mult == q.slot_mult &&
           p.ks == q.ks && p.slices == q.slices && p.n_tiles == q.n_tiles && p.grid == q.grid;
}

int launch_gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t s) {
    // (no pair under the clock probe: the blocks of both problems would write the same probe rows)
    if (gemm_invalid(a) || gemm_invalid(b) || a.M <= 0 || a.N <= 0 || !twin_shapes(a, b) || g_clock_probe) return 1;
    // the launches with a twin form: split-K, and one round of 64 x 64 tiles at two blocks per CU with two k-slices per step
    const int G = slots();
    const GemmPlan p = plan_gemm(a, G);
    const bool splitk = p.family == GemmPlan::SPLITK;
    if (p.rows != a.M || !(splitk || (p.family == GemmPlan::TILED && p.bm == 64 && p.bn == 64 && p.ksl == 2 && p.slot_mult == 2))) return 1;
    // b's own plan too: twin_shapes leaves out what may differ between the twins (ReLU-on-A), and each problem must run what it would alone
    if (!same_plan(p, plan_gemm(b, G))) return 1;
    return splitk ? launch_gemm_splitk(a, p, s, &b) : launch_t<64, 64, 2, true>(a, b, p.n_tiles, p.grid, s);
}

#undef launch_plan
#undef VLSAT_LAUNCH_CHECK
#undef fail
#undef hipLaunchKernelGGL

}  // namespace legacy
// ---- end of the oracle ----

namespace {

using vlsat::GemmPlan;

// ---- a case: the fields of GemmArgs the enumeration sets, filled into the old and the new struct alike ----
struct Case {
    int G = 512, M = 0, N = 0, K = 0, lda_pad = 0, prec = 0, a_split = 0, half_f16 = 0;
    int add = 0, relu_a = 0, rowscale = 0, c_split = 0, c_f16 = 0 /* 0 | 1 = N | 2 = 256 */, g_f16 = 0, no_ws = 0, sk_max_tiles = 0;
    int no_dma = 0, no_ring = 0, no_p8 = 0, p8_part_min = 0, bias_off = 0;
    int lda_big = 0;                                        // a pitch of A of 16 384 floats more
    int ring_wide = 0, ring_bk32 = 0, ring_nodb = 0, force_tile = 0, ablate = 0;        // (experiments build)
};
alignas(16) char g_mem[1 << 12];    // operand "buffers": the planner reads the pointers' values only (null, alignment)
template <class A> void fill(A& a, const Case& c, int twin = 0) {
    float* base = reinterpret_cast<float*>(g_mem) + 256 * twin;
    a.A = base; a.W = base + 16; a.C = base + 32;
    a.M = c.M; a.N = c.N; a.K = c.K;
    a.lda = c.K + c.lda_pad + 16384 * c.lda_big; a.ldw = c.K; a.ldc = c.N; a.ldr = c.N; a.ldg0 = a.ldg1 = c.N;
    a.bias = base + 48 + c.bias_off;
    if (c.rowscale) a.rowscale = base + 64;
    if (c.add & 1) a.resid = base + 80;
    if (c.add & 2) { a.g0 = base + 96; a.gi0 = reinterpret_cast<const int32_t*>(base + 112); }
    if (c.add & 4) { a.g1 = base + 128; a.gi1 = reinterpret_cast<const int32_t*>(base + 144); }
    a.relu_a = c.relu_a;
    a.prec = c.prec; a.a_split = c.a_split; a.half_f16 = c.half_f16; a.c_split = c.c_split;
    if (c.prec) { a.Whi = reinterpret_cast<const uint16_t*>(base + 160); a.Wlo = reinterpret_cast<const uint16_t*>(base + 176); }
    a.c_f16_cols = c.c_f16 == 1 ? c.N : c.c_f16 == 2 ? 256 : 0;
    a.g_f16 = c.g_f16;
    if (!c.no_ws) {
        a.sk_ws = base + 192; a.sk_ws_floats = vlsat::SPLITK_WS_FLOATS;
        a.sk_counters = reinterpret_cast<unsigned*>(base + 208); a.sk_n_counters = vlsat::SPLITK_COUNTERS;
    }
    a.sk_max_tiles = c.sk_max_tiles;
    a.no_dma = c.no_dma; a.no_ring = c.no_ring; a.no_p8 = c.no_p8; a.p8_part_min = c.p8_part_min;
    a.ring_wide = c.ring_wide; a.ring_bk32 = c.ring_bk32; a.ring_nodb = c.ring_nodb; a.force_tile = c.force_tile; a.ablate = c.ablate;
}
std::string show(const Case& c) {
    char b[512];
    snprintf(b, sizeof b, "G %d M %d N %d K %d lda+%d prec %d a_split %d half_f16 %d add %d relu %d rowscale %d c_split %d c_f16 %d g_f16 %d no_ws %d sk_max %d "
             "no_dma %d no_ring %d no_p8 %d part_min %d bias+%d wide %d bk32 %d nodb %d force_tile %d ablate %d", c.G, c.M, c.N, c.K, c.lda_pad + 16384 * c.lda_big, c.prec, c.a_split, c.half_f16,
             c.add, c.relu_a, c.rowscale, c.c_split, c.c_f16, c.g_f16, c.no_ws, c.sk_max_tiles, c.no_dma, c.no_ring, c.no_p8, c.p8_part_min, c.bias_off,
             c.ring_wide, c.ring_bk32, c.ring_nodb, c.force_tile, c.ablate);
    return b;
}
std::string show(const Rec& r) {
    char b[256];
    snprintf(b, sizeof b, "%c<%d,%d,%d,%d,%d,%d> family %d rows %d tile %dx%d ksl %d slot_mult %d ks %d slices %d n_tiles %d grid %d | <<<(%d,%d),%d>>>(M %d, %d, %d, %d, %d)",
             r.kernel, r.targ[0], r.targ[1], r.targ[2], r.targ[3], r.targ[4], r.targ[5], r.family, r.rows, r.bm, r.bn, r.ksl, r.slot_mult, r.ks, r.slices,
             r.n_tiles, r.grid, r.gx, r.gy, r.block, r.M, r.k_tiles, r.k_nbn, r.k_ks, r.k_slices);
    return b;
}

// ---- the new code: the launch of a plan as the table launchers of the .hip files make it from the plan and the row of the list ----
std::set<int> g_reached[4];         // rows of each family's list that a launch used (index: GemmPlan::Family)
std::set<int> g_twin_reached;       // rows of the persistent kernel's list whose twin form a pair used
Rec launch_of(const vlsat::GemmArgs& m, const GemmPlan& p, bool twin) {
    Rec r;
    r.family = p.family; r.rows = p.rows; r.bm = p.bm; r.bn = p.bn; r.ksl = p.ksl; r.slot_mult = p.slot_mult; r.ks = p.ks; r.slices = p.slices;
    r.n_tiles = p.n_tiles; r.grid = p.grid;
    r.gx = p.grid; r.gy = 1; r.block = 512; r.k_tiles = p.n_tiles; r.M = m.M;
    g_reached[p.family].insert(p.variant);
    switch (p.family) {
        case GemmPlan::P8: {
            const vlsat::GemmP8Variant& v = vlsat::kGemmP8Variants[p.variant];
            r.kernel = 'P'; r.targ[0] = v.mode; r.targ[1] = v.add; r.targ[2] = v.relu; r.targ[3] = v.cf; r.targ[4] = v.abl;
            r.k_nbn = m.N / 256;
            break;
        }
        case GemmPlan::RING: {
            const vlsat::GemmRingVariant& v = vlsat::kGemmRingVariants[p.variant];
            r.kernel = 'R'; r.targ[0] = v.terms; r.targ[1] = v.afmt; r.targ[2] = v.add; r.targ[3] = v.rbn; r.targ[4] = v.rbk; r.targ[5] = v.db;
            r.k_nbn = (m.N + p.bn - 1) / p.bn;
            break;
        }
        case GemmPlan::SPLITK:
            r.kernel = 'S'; r.targ[0] = vlsat::kGemmSplitkVariants[p.variant]; r.targ[1] = twin;
            r.block = 256; r.gy = twin ? 2 : 1; r.k_nbn = (m.N + 63) / 64; r.k_ks = p.ks; r.k_slices = p.slices;
            break;
        default: {
            const vlsat::GemmTiledVariant& v = vlsat::kGemmTiledVariants[p.variant];
            const vlsat::GemmTile& t = vlsat::kGemmTiles[twin ? vlsat::kGemmTileCount - 1 : vlsat::gemm_tile_index(p.bm, p.bn, p.ksl)];
            r.kernel = 'T'; r.targ[0] = t.bm; r.targ[1] = t.bn; r.targ[2] = v.add; r.targ[3] = v.prec; r.targ[4] = t.ksl; r.targ[5] = twin;
            r.block = 256; r.gy = twin ? 2 : 1; r.k_nbn = (m.N + p.bn - 1) / p.bn;
            if (twin) g_twin_reached.insert(p.variant);
        }
    }
    return r;
}
bool variant_in_range(const GemmPlan& p) {
    const int n = p.family == GemmPlan::P8 ? vlsat::kGemmP8Count : p.family == GemmPlan::RING ? vlsat::kGemmRingCount
                : p.family == GemmPlan::SPLITK ? vlsat::kGemmSplitkCount : vlsat::kGemmTiledCount;
    return p.variant >= 0 && p.variant < n;
}
// launch_gemm of gemm_f32.hip: validate, plan, launch, plan the tail again
Run new_gemm(vlsat::GemmArgs a, int G) {
    Run run;
    if (const char* why = vlsat::gemm_invalid(a)) { run.rc = -1; run.error = why; return run; }
    if (a.M <= 0 || a.N <= 0) return run;
    while (true) {
        const GemmPlan p = vlsat::plan_gemm(a, G);
        vlsat::GemmArgs m = a;
        m.M = p.rows;
        if (p.family == GemmPlan::TILED && p.variant < 0) { run.rc = -1; run.error = vlsat::gemm_tiled_pick(m, m.relu_a).why; return run; }      // (launch_tiled of gemm_f32.hip)
        if (!variant_in_range(p) || p.rows <= 0 || p.rows > a.M) { run.rc = -99; run.error = "(plan without a row of its list, or without rows)"; return run; }
        run.launches.push_back(launch_of(m, p, false));
        if (p.rows == a.M) return run;
        a = vlsat::tail_of(a, p.rows);
    }
}
Run new_pair(const vlsat::GemmArgs& a, const vlsat::GemmArgs& b, int G) {
    Run run;
    const GemmPlan p = vlsat::gemm_pair_plan(a, b, G, false);
    if (p.variant < 0) { run.rc = 1; return run; }
    if (!variant_in_range(p)) { run.rc = -99; return run; }
    run.launches.push_back(launch_of(a, p, true));
    return run;
}

[[noreturn]] void die(const char* what, const Case& c, const Run& want, const Run& got) {
    printf("%s -> FAILED at %s\n  old: rc %d %s, %d launches\n  new: rc %d %s, %d launches\n", what, show(c).c_str(), want.rc, want.error ? want.error : "-",
           (int)want.launches.size(), got.rc, got.error ? got.error : "-", (int)got.launches.size());
    for (size_t i = 0; i < std::max(want.launches.size(), got.launches.size()); ++i)
        printf("  %d old %s\n    new %s\n", (int)i, i < want.launches.size() ? show(want.launches[i]).c_str() : "-", i < got.launches.size() ? show(got.launches[i]).c_str() : "-");
    exit(1);
}
void compare(const char* what, const Case& c, const Run& want, const Run& got) {
    // (an error after some launches: the old code had launched them too -- both sides keep them)
    const bool same_error = (!want.error && !got.error) || (want.error && got.error && !strcmp(want.error, got.error));
    if (want.rc != got.rc || !same_error || want.launches.size() != got.launches.size()) die(what, c, want, got);
    for (size_t i = 0; i < want.launches.size(); ++i)
        if (!(want.launches[i] == got.launches[i])) die(what, c, want, got);
}

long g_cases = 0, g_launches = 0, g_errors = 0;
void check_single(const Case& c) {
    legacy::GemmArgs o;
    vlsat::GemmArgs n;
    fill(o, c);
    fill(n, c);
    g_run = Run{};
    g_plan = Rec{};
    g_G = c.G;
    g_run.rc = legacy::launch_gemm(o, nullptr);
    const Run got = new_gemm(n, c.G);
    compare("legacy", c, g_run, got);
    ++g_cases;
    g_launches += (long)got.launches.size();
    g_errors += got.rc != 0;
}

long g_pairs = 0, g_paired = 0;
// twins: b is a's case with `diff` applied: 0 nothing, 1 ReLU-on-A of b only, 2 of a only, 3 M, 4 N, 5 K, 6 lda, 7 the same split-K workspace
void check_pair(const Case& ca, int diff) {
    Case cb = ca, c = ca;
    if (diff == 1) cb.relu_a = 1;
    if (diff == 2) c.relu_a = 1;
    if (diff == 3) cb.M += 1;
    if (diff == 4) cb.N += 64;
    if (diff == 5) cb.K += 32;
    if (diff == 6) cb.lda_pad += 8;
    legacy::GemmArgs oa, ob;
    vlsat::GemmArgs na, nb;
    fill(oa, c); fill(ob, cb, 1);
    fill(na, c); fill(nb, cb, 1);
    if (diff == 7) { ob.sk_ws = oa.sk_ws; nb.sk_ws = na.sk_ws; }
    g_run = Run{};
    g_plan = Rec{};
    g_G = c.G;
    g_run.rc = legacy::launch_gemm_pair(oa, ob, nullptr);
    Run got = new_pair(na, nb, c.G);
    // (the pair launch of the old code went past launch_plan: the plan fields of its record are those of the new plan when the
    //  launch itself -- kernel, template arguments, grid, block, kernel arguments -- is the same; error texts of refusals never left it)
    Run want = g_run;
    want.error = nullptr;
    if (want.launches.size() == 1 && got.launches.size() == 1) {
        Rec& w = want.launches[0];
        const Rec& g = got.launches[0];
        w.family = g.family; w.rows = g.rows; w.bm = g.bm; w.bn = g.bn; w.ksl = g.ksl; w.slot_mult = g.slot_mult; w.ks = g.ks; w.slices = g.slices;
        w.n_tiles = g.n_tiles; w.grid = g.grid;
        if (g.rows != c.M || g.n_tiles != w.k_tiles || g.grid != w.gx || g.ks != w.k_ks || g.slices != w.k_slices || (g.family == GemmPlan::TILED && (g.bm != w.targ[0] || g.bn != w.targ[1] || g.ksl != w.targ[4] || g.slot_mult != 2)))
            die("pairs", c, want, got);
    }
    compare("pairs", c, want, got);
    ++g_pairs;
    g_paired += got.rc == 0;
}

const int kG[] = {512, 608, 8};
const int kM[] = {1, 9, 80, 300, 1560, 2560, 7032, 35143, 39800, 70000, 70001, 99840};
const int kN[] = {26, 64, 160, 200, 256, 512, 1024, 3328};
const int kK[] = {32, 64, 96, 128, 256, 512, 768, 1024};
const int kFmt[][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 2, 0}, {1, 2, 1}, {3, 0, 0}, {3, 1, 0}, {3, 2, 0}};      // prec, a_split, half_f16
const int kAdd[] = {0, 1, 2, 6, 7};

const char* family_name(int f) { return f == GemmPlan::SPLITK ? "split-K" : f == GemmPlan::P8 ? "8-phase" : f == GemmPlan::RING ? "ring" : "persistent"; }

// the launch sequence of a bench-batch shape, one table row
void bench_row(const char* mode, const char* what, int M, int N, int K, int prec, int a_split) {
    Case c;
    c.M = M; c.N = N; c.K = K; c.prec = prec; c.a_split = a_split;
    vlsat::GemmArgs a;
    fill(a, c);
    const Run run = new_gemm(a, 512);
    std::string s;
    for (const Rec& r : run.launches) {
        char b[160];
        if (r.family == GemmPlan::P8 || r.family == GemmPlan::RING)
            snprintf(b, sizeof b, "%s%s %d x %d: %d rows, %d tiles on %d blocks (%.2f rounds)", s.empty() ? "" : "; ", family_name(r.family), r.bm, r.bn, r.rows, r.n_tiles, r.grid, (double)r.n_tiles / r.grid);
        else if (r.family == GemmPlan::SPLITK)
            snprintf(b, sizeof b, "%s%s: %d rows, %d tiles x %d parts", s.empty() ? "" : "; ", family_name(r.family), r.rows, r.n_tiles, r.ks);
        else
            snprintf(b, sizeof b, "%s%s %d x %d, %d slice%s per step, %d blocks per CU: %d rows, %d tiles on %d blocks", s.empty() ? "" : "; ", family_name(r.family), r.bm, r.bn, r.ksl, r.ksl > 1 ? "s" : "", r.slot_mult, r.rows, r.n_tiles, r.grid);
        s += b;
    }
    printf("table | %s | %s | %d | %d | %d | %s |\n", mode, what, M, N, K, run.rc ? run.error : s.c_str());
}

}  // namespace

int main() {
    // ---- 1. shapes x formats (36 864), every other switch varied one at a time from the baseline (no additive operand, no ReLU, no row
    //         scale, fp32 C, split-K workspace present, aligned bias) ----
    std::vector<Case> variations;
    variations.push_back(Case{});
    auto vary = [&](auto set) { Case v; set(v); variations.push_back(v); };
    for (int add : kAdd) if (add) vary([&](Case& v) { v.add = add; });
    vary([](Case& v) { v.relu_a = 1; });
    vary([](Case& v) { v.rowscale = 1; });
    vary([](Case& v) { v.c_split = 1; });
    vary([](Case& v) { v.c_split = 2; });
    vary([](Case& v) { v.c_f16 = 1; });
    vary([](Case& v) { v.c_f16 = 2; });
    vary([](Case& v) { v.g_f16 = 1; });
    vary([](Case& v) { v.g_f16 = 1; v.add = 6; });          // (fp16 tables are refused without gathered rows: with them too)
    vary([](Case& v) { v.no_ws = 1; });
    vary([](Case& v) { v.sk_max_tiles = 16; });
    vary([](Case& v) { v.no_dma = 1; });
    vary([](Case& v) { v.no_ring = 1; });
    vary([](Case& v) { v.no_p8 = 1; });
    vary([](Case& v) { v.p8_part_min = 12; });
    vary([](Case& v) { v.bias_off = 1; });
    vary([](Case& v) { v.lda_big = 1; });                   // (rows of A beyond 32-bit byte offsets at the large M)
#ifdef VLSAT_EXPERIMENTS
    vary([](Case& v) { v.ring_wide = 1; });
    vary([](Case& v) { v.ring_bk32 = 1; });
    vary([](Case& v) { v.ring_nodb = 1; });
    vary([](Case& v) { v.ring_wide = 1; v.no_p8 = 1; });    // (the wide ring tiles need N % 256 == 0, where the 8-phase kernel comes first)
    vary([](Case& v) { v.ring_bk32 = 1; v.no_p8 = 1; });
    vary([](Case& v) { v.ring_nodb = 1; v.no_p8 = 1; });
    for (int t = 1; t <= 7; ++t) vary([&](Case& v) { v.force_tile = t; });
#endif
    for (int G : kG) for (int M : kM) for (int N : kN) for (int K : kK) for (int pad : {0, 256}) for (const auto& f : kFmt)
        for (Case c : variations) {
            c.G = G; c.M = M; c.N = N; c.K = K; c.lda_pad = pad; c.prec = f[0]; c.a_split = f[1]; c.half_f16 = f[2];
            check_single(c);
        }
    const long one_at_a_time = g_cases;
    // ---- 2. the operand switches that name a row TOGETHER (additive mode 0..7 x ReLU x format of C x fp16 columns x no_dma x no_p8 = 576)
    //         over 60 shapes x formats at G = 512: the rows of the lists are combinations of them ----
    for (int M : {9, 300, 2560, 35143, 99840}) for (int N : {64, 160, 512, 3328}) for (int K : {64, 96, 512}) for (const auto& f : kFmt)
        for (int add = 0; add < 8; ++add) for (int relu : {0, 1}) for (int cs : {0, 1, 2}) for (int c16 : {0, 1, 2}) for (int nd : {0, 1}) for (int np : {0, 1}) {
            Case c;
            c.M = M; c.N = N; c.K = K; c.prec = f[0]; c.a_split = f[1]; c.half_f16 = f[2];
            c.add = add; c.relu_a = relu; c.c_split = cs; c.c_f16 = c16; c.no_dma = nd; c.no_p8 = np;
            check_single(c);
        }
    const long products = g_cases - one_at_a_time;
    // ---- 2b. the thresholds of the planner, each from both sides: M at every multiple of 64 up to 10 240 and one past it (tiles per
    //          round of every tile size at G = 512 | 608, the split-K bounds, the 64 x 128 rule, part_min = 32 tiles at N = 256), and around
    //          part_min / rem_min of the other precisions: 5/8 of a round = 160 | 190 panels at N = 256, 256 | 304 panels + 12 | 24;
    //          N around the 1024..2048 window; K = 192 (a multiple of 64, not of 128) ----
    std::vector<int> edge_m;
    for (int k = 0; k <= 160; ++k) { edge_m.push_back(64 * k); edge_m.push_back(64 * k + 1); }
    for (int panels : {159, 160, 189, 190, 256 + 11, 256 + 12, 256 + 23, 256 + 24, 304 + 11, 304 + 12, 304 + 23, 304 + 24, 256 + 159, 256 + 160, 304 + 189, 304 + 190})
        for (int d : {0, 1}) edge_m.push_back(256 * panels + d);
    for (int G : {512, 608}) for (int M : edge_m) for (int N : {64, 128, 256, 512, 960, 1024, 2048, 2176}) for (int K : {64, 128, 192, 512}) for (const auto& f : kFmt)
        for (int no_ws : {0, 1}) {
            Case c;
            c.G = G; c.M = M; c.N = N; c.K = K; c.prec = f[0]; c.a_split = f[1]; c.half_f16 = f[2]; c.no_ws = no_ws;
            check_single(c);
        }
    const long thresholds = g_cases - one_at_a_time - products;
#ifdef VLSAT_EXPERIMENTS
    // ---- 2c. the timing ablations of the 8-phase kernel: half rows in and out, plain or gathered rows with ReLU ----
    for (int M : {35143, 99840}) for (int N : {512, 3328}) for (int K : {512}) for (int half : {0, 1}) for (int gathered : {0, 1})
        for (int ablate : {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 37, 65}) {
            Case c;
            c.M = M; c.N = N; c.K = K; c.prec = 1; c.a_split = 2; c.half_f16 = half; c.c_split = 2; c.add = gathered ? 6 : 0; c.relu_a = gathered; c.ablate = ablate;
            check_single(c);
        }
    // ---- 2d. the ring kernel's lab switches together with the additive modes that name its rows ----
    for (int M : {35143, 99840}) for (int N : {512, 3328}) for (int K : {64, 96, 512}) for (const auto& f : kFmt) for (int add : {0, 1, 6}) for (int np : {0, 1})
        for (int sw = 0; sw < 8; ++sw) {
            Case c;
            c.M = M; c.N = N; c.K = K; c.prec = f[0]; c.a_split = f[1]; c.half_f16 = f[2]; c.add = add; c.no_p8 = np;
            c.ring_wide = sw & 1; c.ring_bk32 = (sw >> 1) & 1; c.ring_nodb = sw >> 2;
            check_single(c);
        }
#endif
    printf("legacy -> ok %ld cases (%ld one switch at a time, %ld operand products, %ld thresholds), %ld launches, %ld refused\n", g_cases, one_at_a_time, products,
           thresholds, g_launches, g_errors);

    // ---- 3. pairs: twins that differ in nothing, in ReLU-on-A only, in one shape field, and twins that share a workspace ----
    for (int G : kG) for (int M : kM) for (int N : kN) for (int K : kK) for (const auto& f : kFmt) for (int add : kAdd) for (int nd : {0, 1})
        for (int diff = 0; diff <= 7; ++diff) {
            Case c;
            c.G = G; c.M = M; c.N = N; c.K = K; c.prec = f[0]; c.a_split = f[1]; c.half_f16 = f[2]; c.add = add; c.no_dma = nd;
            check_pair(c, diff);
            if (diff <= 2) { c.no_ws = 1; check_pair(c, diff); }      // (without split-K: the persistent kernel's twin form)
        }
    printf("pairs -> ok %ld pairs, %ld in one launch\n", g_pairs, g_paired);

    // ---- 4. every row of every list is reached by a case above (a row nothing reaches is dead, or the enumeration too thin) ----
    const int counts[4] = {vlsat::kGemmSplitkCount, vlsat::kGemmP8Count, vlsat::kGemmRingCount, vlsat::kGemmTiledCount};
    int twin_rows = 0;
    for (const vlsat::GemmTiledVariant& v : vlsat::kGemmTiledVariants) twin_rows += v.twin;
    for (int f = 0; f < 4; ++f)
        for (int i = 0; i < counts[f]; ++i)
            if (!g_reached[f].count(i)) { printf("reachable -> FAILED (%s row %d)\n", family_name(f), i); return 1; }
    for (int i = 0; i < vlsat::kGemmTiledCount; ++i)
        if (vlsat::kGemmTiledVariants[i].twin && !g_twin_reached.count(i)) { printf("reachable -> FAILED (twin form of persistent row %d)\n", i); return 1; }
    printf("reachable -> ok 8-phase %d, ring %d, persistent %d (%d with a twin form), split-K %d\n", counts[1], counts[2], counts[3], twin_rows, counts[0]);

    // ---- 5. the lists themselves: no row twice, no 128 x 256 ring tile and no ablation outside the experiments build ----
    int ring256 = 0, abl = 0;
    for (int i = 0; i < vlsat::kGemmP8Count; ++i) {
        const vlsat::GemmP8Variant& v = vlsat::kGemmP8Variants[i];
        if (vlsat::gemm_p8_find(v.mode, v.add, v.relu, v.cf, v.abl) != i) { printf("lists -> FAILED (8-phase row %d is listed twice)\n", i); return 1; }
        abl += v.abl != 0;
    }
    for (int i = 0; i < vlsat::kGemmRingCount; ++i) {
        const vlsat::GemmRingVariant& v = vlsat::kGemmRingVariants[i];
        if (vlsat::gemm_ring_find(v.terms, v.afmt, v.add, v.rbn, v.rbk, v.db) != i) { printf("lists -> FAILED (ring row %d is listed twice)\n", i); return 1; }
        ring256 += v.rbn == 256;
    }
    for (int i = 0; i < vlsat::kGemmTiledCount; ++i)
        if (vlsat::gemm_tiled_find(vlsat::kGemmTiledVariants[i].add, vlsat::kGemmTiledVariants[i].prec) != i) { printf("lists -> FAILED (persistent row %d is listed twice)\n", i); return 1; }
    for (int i = 0; i < vlsat::kGemmTileCount; ++i)
        if (vlsat::gemm_tile_index(vlsat::kGemmTiles[i].bm, vlsat::kGemmTiles[i].bn, vlsat::kGemmTiles[i].ksl) != i) { printf("lists -> FAILED (tile %d)\n", i); return 1; }
    if (!vlsat::kGemmLab && (ring256 || abl)) { printf("lists -> FAILED (lab rows in the release lists)\n"); return 1; }
    printf("lists -> ok %d ring rows with 128 x 256 tiles, %d ablations\n", ring256, abl);

    // ---- 6. the bench batch (512 scenes: 2 560 node rows, 99 840 edge rows) at G = 512 ----
    const struct { const char* mode; int prec, edge_split; } modes[] = {{"fp32", 0, 0}, {"bf16x3", 3, 1}, {"bf16_mixed", 1, 2}};
    for (const auto& m : modes) {
        for (int N : {512, 1024}) for (int K : {512, 1024}) bench_row(m.mode, "edge rows", 99840, N, K, m.prec, m.edge_split);
        for (int N : {512, 1024}) for (int K : {512, 1024}) bench_row(m.mode, "node rows", 2560, N, K, m.prec, 0);
        bench_row(m.mode, "node projection", 2560, 3328, 512, m.prec, 0);
    }
    printf("bench -> ok\n");
    return 0;
}
