// Kernel-level C entry points (unit tests and tools drive single kernels through these) and debug hooks.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

#include "engine.h"

using namespace vlsat;

extern "C" {

const char* vlsat_last_error(void) { return last_error_cstr(); }

// debug: stop the forward after stage `stage` (see DESIGN.md "debug stages"); -1 = run all
int vlsat_debug_stop_after(vlsat_handle h, int32_t stage) {
    if (!h) return fail(VLSAT_EINVAL, "null handle");
    h->debug_stop = stage;
    return 0;
}

// debug: while `buf` (device, >= 4 * 512 int64) is set, every persistent GEMM block writes
// {shader cycles, 100 MHz wall ticks, tiles done, 1} at exit: effective clock = cycles / (ticks / 1e8)
int vlsat_debug_gemm_clock_probe(int64_t* buf) {
    gemm_set_clock_probe(reinterpret_cast<long long*>(buf));
    return 0;
}

// Keys of the edge cross-attention for plans created from now on (see vlsat.h)
int vlsat_set_edge_attention_scope(vlsat_handle h, int32_t scope) {
    if (!h) return fail(VLSAT_EINVAL, "null handle");
    if (scope != 0 && scope != 1) return fail(VLSAT_EINVAL, "edge attention scope: 0 (per scene) or 1 (whole batch)");
    h->edge_scope = scope;
    ++h->config_epoch;
    return 0;
}

// Switches of one handle (none changes results beyond fp32 summation order / the mode's rounding; defaults are the measured-best
// settings).  The RELEASE library knows the ones a deployment or a test has a use for:
//   "dual_stream" 0|1|2 a second (and third) stream for the 2D chains: 1 small plans only, 2 every plan (plans created afterwards)
//   "sched"       -1|0|1  two-stream plans: dependency-exact three-lane schedule (1), the fork / join schedule of round 4 (0), or by
//                       plan size (-1, default: exact on plans of more than 16384 edges in every precision mode, fork / join below)
//   "flash_split" 0|1   split-key edge attention for plans that cannot fill the chip (plans created afterwards)
//   "prof_dual"   0|1   per-class profiling keeps the multi-stream execution (1, default) or serialises on the launch stream
//   "pair_twins" 0|1 / "pair_max_edges" n   paired schedule of one-scene plans (engine_forward.hip): twin stages as launches of two problems
//   "gather_f16" -1|0|1    [P_i | P_j] of the node-side projection as fp16 half rows (-1: on in the single-rounding modes)
//   "outproj_f16" -1|0|1   out-projection of the single-rounded edge attention -> LayerNorm as fp16 half rows instead of fp32 (-1: on)
//   "gemm_k_rot" -1|0..7   K-tile rotation per column tile of the 8-phase GEMM (-1: 1 for half-row bf16 launches, else 0)
//   "gemm_p8" / "gemm_dma" / "gemm_splitk" 0|1   GEMM kernel selection: 256 x 256 8-phase kernel for large launches, LDS-direct staging of
//                       fp32 operands, split-K kernel for small launches (0: the older kernels; parity-tested both ways)
//   "split_fmt" / "flash_bf16" / "flash_tr" / "pointnet_bf16" / "gate_bf16" / "ln_resid" 0|1   bf16 modes: edge tensors between matrix
//                       kernels as bf16 hi/lo pairs or half rows, attention / object encoder / gate on the bf16 matrix cores, V operand by
//                       LDS transpose read, attention residual added by the LayerNorm kernel (0: the fp32 forms; parity-tested both ways)
//   "flash_pv_terms" 3|2   split-bf16 edge attention: MFMAs per P.V product
//   "flash_exact" -1|0|1   fp32 mode, head dim 64: the edge attention's products as three fp16 MFMAs each (-1 default, 0) or the exact
//                       fp32-MFMA kernel (1: the forward of the releases before the split-fp16 kernel, bit for bit)
//   "gemm_exact" -1|0|1    fp32 mode: the full rounds of the large edge-row GEMM launches as three fp16 MFMAs per product (-1 default, 0;
//                       gemm_p8s_kernel) or on the exact fp32-MFMA kernel (1); governs the 8-phase launches only
//   "gemm_small_exact" -1|0|1  fp32 mode: the launches of the persistent GEMM kernel (tails, small launches, node rows) as three fp16 MFMAs
//                       per product (-1 default, 0; gemm_f16s_kernel) or exact, and node rows exact on every kernel (1); independent of "gemm_exact"
//   "pointnet_exact" -1|0|1  fp32 mode: conv2 / conv3 of the object encoder as three fp16 MFMAs per product (-1 default, 0;
//                       pointnet_bf16_kernel<CIN, 5>) or the exact fp32-MFMA kernel (1)
//   "gate_exact" -1|0|1    fp32 mode, shipped head geometry: the edge gate's products as three fp16 MFMAs each (-1 default, 0;
//                       edge_gate_f16s_kernel) or the exact fp32-MFMA kernel (1: the forward of the release before, bit for bit)
//                       ("flash_exact", "gemm_exact", "gemm_small_exact", "pointnet_exact" and "gate_exact" all 1: the forward of the
//                       releases before the split-fp16 kernels, bit for bit)
//   "edge_pairs" 0|1     fp32 mode: Hbig, R1 and the 3D chain tensor E3 travel between the split-fp16 GEMMs as pair words (the halves of the
//                       split operand, made once by the writer) wherever every launch that touches them has the form (1, default;
//                       edge_pairs.h), or stay fp32 (0: the forward of the releases before the pair words); same outputs bit for bit
//   "edge_pairs_e2" 0|1  fp32 mode, with "edge_pairs" 1: the 2D chain tensor E2 as the LayerNorm of the edge attention and conv3 of
//                       rel_encoder_2d write it (read only by nn_edge.0 / proj_edge of gcn_2ds and the 2D relation head) as pair words too
//                       (1, default), or fp32 (0: the forward of the release before); what nn_edge.2 writes into E2 is fp32 either way
//   "flash_bq_big" 0|1   half-row edge attention on plans whose scenes all have >= 4096 edges: 256 queries per block (1, default) or 128
//   "gate_fuse_agg" 0|1|2  max aggregation inside the gate kernel: never / bf16 modes, and fp32 on plans of more than 16384 edges (default) /
//                       fp32 on every plan
//   "gate_row_map" 0|1, "gate_heads_mfma" 0|1|2   gate kernel variants the tests compare bit for bit
// An EXPERIMENTS build (build.py --experiments, -DVLSAT_EXPERIMENTS) also accepts the lab switches -- "gate_grid" n, "gate_heads_bf16",
// "flash_heads_bf16", "node_attn_split" n, "half_fmt", "flash_dma" 0|1|3|4, "flash_ablate" bits (GARBAGE results: timing only) -- and
// honours the ablation bits of GemmArgs / FlashSplit; the release library answers them with an error.
int vlsat_debug_option(vlsat_handle h, const char* name, int32_t value) {
    if (!h || !name) return fail(VLSAT_EINVAL, "vlsat_debug_option: null argument");
    const std::string k(name);
    ++h->config_epoch;
    if (k == "dual_stream") h->dual_stream = value < 0 ? 0 : value;
    else if (k == "sched") h->sched = value < 0 ? -1 : value != 0;
    else if (k == "flash_split") h->fa_split = value != 0;
    else if (k == "gemm_dma") h->gemm_no_dma = value == 0;
    else if (k == "gemm_p8") h->gemm_no_p8 = value == 0;
    else if (k == "pair_twins") h->pair_twins = value != 0;
    else if (k == "pair_max_edges") h->pair_max_edges = value < 0 ? 0 : value;
    else if (k == "gather_f16") h->gather_f16 = value < 0 ? -1 : value != 0;
    else if (k == "outproj_f16") h->outproj_f16 = value < 0 ? -1 : value != 0;
    else if (k == "gemm_k_rot") h->gemm_k_rot = value < 0 ? -1 : value > 7 ? 7 : value;
    else if (k == "gate_row_map") h->gate_row_map = value != 0;
    else if (k == "prof_dual") h->prof_dual = value != 0;
    else if (k == "gate_heads_mfma") h->gate_heads_mfma = value < 0 ? 0 : value > 2 ? 2 : value;
    else if (k == "gemm_splitk") h->gemm_splitk = value != 0;
    else if (k == "gemm_p8_part_min") h->gemm_p8_part_min = value < 0 ? 0 : value;
    else if (k == "gemm_splitk_max_tiles") h->gemm_splitk_max_tiles = value < 0 ? 0 : value;
    else if (k == "split_fmt") h->split_fmt = value != 0;
    else if (k == "ln_resid") h->ln_resid = value != 0;
    else if (k == "gate_fuse_agg") h->gate_fuse_agg = value < 0 ? 0 : value > 2 ? 2 : value;
    else if (k == "flash_pv_terms") h->flash_pv_terms = value == 2 ? 2 : 3;
    else if (k == "flash_exact") h->flash_exact = value < 0 ? -1 : value != 0;
    else if (k == "edge_pairs") h->edge_pairs = value != 0;
    else if (k == "edge_pairs_e2") h->edge_pairs_e2 = value != 0;
    else if (k == "gemm_exact") h->gemm_exact = value < 0 ? -1 : value != 0;
    else if (k == "pointnet_exact") h->pointnet_exact = value < 0 ? -1 : value != 0;
    else if (k == "gemm_small_exact") h->gemm_small_exact = value < 0 ? -1 : value != 0;
    else if (k == "gate_exact") h->gate_exact = value < 0 ? -1 : value != 0;
    else if (k == "flash_bf16") h->flash_bf16 = value != 0;
    else if (k == "pointnet_bf16") h->pointnet_bf16 = value != 0;
    else if (k == "gate_bf16") h->gate_bf16 = value != 0;
    else if (k == "flash_tr") h->flash_tr = value != 0;
    else if (k == "flash_bq_big") h->flash_bq_big = value != 0;
    else if (k == "flash_qg") h->flash_qg = value < 0 || value > 2 ? 0 : value;
    else if (k == "flash_bq_big_min") h->flash_bq_big_min = value < 256 ? 256 : value;
#ifdef VLSAT_EXPERIMENTS
    else if (k == "gate_grid") h->gate_grid = value > 0 ? value : 0;
    else if (k == "gate_heads_bf16") h->gate_heads_bf16 = value != 0;
    else if (k == "flash_heads_bf16") h->flash_heads_bf16 = value != 0;
    else if (k == "node_attn_split") h->node_attn_split = value;
    else if (k == "half_fmt") h->half_fmt = value != 0;
    else if (k == "flash_dma") h->flash_dma = (value == 3 || value == 4) ? value : value != 0;
    else if (k == "flash_ablate") h->flash_ablate = value;
#else
    else if (k == "gate_grid" || k == "gate_heads_bf16" || k == "flash_heads_bf16" || k == "node_attn_split" || k == "half_fmt" ||
             k == "flash_dma" || k == "flash_ablate")
        return fail(VLSAT_EINVAL, "vlsat_debug_option: " + k + " is a lab switch of the experiments build (build.py --experiments)");
#endif
    else return fail(VLSAT_EINVAL, "vlsat_debug_option: unknown option " + k);
    return 0;
}

// -------------------------------------------------------------------------------------------
// workspace of the split-K kernel for the handle-free test entry points (allocated on first use, never freed)
static int test_splitk_ws(GemmArgs& a) {
    static float* ws = nullptr;
    static unsigned* cnt = nullptr;
    if (!ws) {
        VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ws), SPLITK_WS_FLOATS * sizeof(float)));
        VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&cnt), SPLITK_COUNTERS * sizeof(unsigned)));
        VLSAT_HIP_CHECK(hipMemset(cnt, 0, SPLITK_COUNTERS * sizeof(unsigned)));
    }
    a.sk_ws = ws; a.sk_ws_floats = SPLITK_WS_FLOATS; a.sk_counters = cnt; a.sk_n_counters = SPLITK_COUNTERS;
    return 0;
}

int vlsat_k_gemm(const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc, int32_t M, int32_t N,
                 int32_t K, const float* bias, const float* rowscale, const float* resid, int32_t ldr, float resid_scale,
                 const float* g0, const int32_t* gi0, int32_t ldg0, const float* g1, const int32_t* gi1, int32_t ldg1,
                 int32_t relu_a, int32_t act, void* stream) {
    GemmArgs a;
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.rowscale = rowscale; a.resid = resid; a.ldr = ldr; a.resid_scale = resid_scale;
    a.g0 = g0; a.gi0 = gi0; a.ldg0 = ldg0; a.g1 = g1; a.gi1 = gi1; a.ldg1 = ldg1; a.relu_a = relu_a & 1; a.act = act;
    if (relu_a & 2) a.prefetch = 0;             // (bit 1 of relu_a: no A-panel prefetch -- benchmarking)
    if (relu_a & 4) RUN(test_splitk_ws(a));     // (bit 2: small launches may take the split-K kernel)
    if (relu_a & 8) a.no_p8 = 1;                // (bit 3: large launches stay off the 256 x 256 8-phase kernel)
    if (kExperiments) {
        a.force_tile = (relu_a >> 4) & 7;       // (bits 4..6: tile of gemm_f32_kernel, GemmArgs::force_tile -- benchmarking; experiments build)
        if (a.force_tile) { a.no_p8 = 1; a.no_ring = 1; }
    }
    return launch_gemm(a, static_cast<hipStream_t>(stream));
}

// w[i] -> bf16 hi[i] + bf16 lo[i]: the planes the bf16 GEMM modes read (asynchronous on `stream`)
int vlsat_k_split_bf16(const float* w, size_t n, uint16_t* hi, uint16_t* lo, void* stream) {
    if (!w || !hi || !lo) return fail(VLSAT_EINVAL, "split_bf16: null argument");
    return launch_split_bf16(w, n, hi, lo, static_cast<hipStream_t>(stream));
}

// vlsat_k_gemm on the bf16 matrix cores with caller-provided weight planes (asynchronous): prec 1 = bf16, 3 = split-bf16;
// no_dma = 1 selects the VGPR-staged operand pipe of round 1, prefetch = slices of look-ahead of the A prefetch (0 = off)
int vlsat_k_gemm_planes(const float* A, int32_t lda, const float* W, const uint16_t* Whi, const uint16_t* Wlo, int32_t ldw,
                        float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias,
                        const float* resid, int32_t ldr, float resid_scale,
                        const float* g0, const int32_t* gi0, int32_t ldg0, const float* g1, const int32_t* gi1, int32_t ldg1,
                        int32_t relu_a, int32_t act, int32_t prec, int32_t no_dma, int32_t prefetch, int32_t fmt, float c_scale,
                        void* stream) {
    if (prec != 1 && prec != 3) return fail(VLSAT_EINVAL, "gemm_planes: prec must be 1 or 3");
    GemmArgs a;
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.resid = resid; a.ldr = ldr; a.resid_scale = resid_scale;
    a.g0 = g0; a.gi0 = gi0; a.ldg0 = ldg0; a.g1 = g1; a.gi1 = gi1; a.ldg1 = ldg1; a.relu_a = relu_a; a.act = act;
    a.prec = prec; a.Whi = Whi; a.Wlo = Wlo; a.no_dma = no_dma; a.prefetch = prefetch;
    const int code = (fmt >> 5) & 1 ? 2 : 1;   // (bit 5: the flagged operands are half rows instead of split pairs)
    a.a_split = (fmt & 1) * code; a.r_split = ((fmt >> 1) & 1) * code; a.c_split = ((fmt >> 2) & 1) * code; a.c_scale = c_scale;
    // (bit 3: g0 / g1 are fp16 half rows; bits 25..28: that many times 256 leading columns of C are written as fp16 half rows -- GemmArgs::g_f16,
    //  c_f16_cols; bit 4: no ring kernel -- benchmarking)
    a.g_f16 = (fmt >> 3) & 1;
    a.c_f16_cols = ((fmt >> 25) & 15) * 256;
    a.no_ring = (fmt >> 4) & 1;
    a.no_p8 = (fmt >> 12) & 1;                 // (bit 12: half-row launches skip the 256 x 256 8-phase kernel)
    a.k_rot = (fmt >> 22) & 7;                 // (bits 22..24: K-tile rotation per column tile of the 8-phase kernel -- A/B)
    if (kExperiments) {                        // lab bits (tools/gemm_bench.py, p8_check.py, gemm_tile_sweep.py): the experiments build only
        a.ring_wide = (fmt >> 7) & 1;              // (bit 7: ring kernel with 128 x 256 tiles where N allows)
        a.ablate = ((fmt >> 8) & 3) | (((fmt >> 13) & 63) << 2);   // (bits 8, 9, 13..18: timing experiments, see GemmArgs::ablate)
        a.ring_bk32 = (fmt >> 10) & 1;             // (bit 10: half-row ring kernel with 32-wide k slices)
        a.ring_nodb = (fmt >> 11) & 1;             // (bit 11: ... without the double-buffered fragment sets)
        a.force_tile = (fmt >> 19) & 7;            // (bits 19..21: tile of gemm_f32_kernel, GemmArgs::force_tile -- benchmarking)
        if (a.force_tile) { a.no_p8 = 1; a.no_ring = 1; }
    } else if (fmt & ((1 << 7) | (3 << 8) | (3 << 10) | (0x1ff << 13))) {
        return fail(VLSAT_EINVAL, "gemm_planes: timing / tile experiment bits need the experiments build (build.py --experiments)");
    }
    if ((fmt >> 6) & 1) RUN(test_splitk_ws(a));    // (bit 6: small launches may take the split-K kernel)
    return launch_gemm(a, static_cast<hipStream_t>(stream));
}

// test entry point: splits a dense W [N,K] on the spot (allocates, synchronises) and runs vlsat_k_gemm_planes
int vlsat_k_gemm_bf16(const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc, int32_t M, int32_t N,
                      int32_t K, const float* bias, const float* resid, int32_t ldr, float resid_scale,
                      const float* g0, const int32_t* gi0, int32_t ldg0, const float* g1, const int32_t* gi1, int32_t ldg1,
                      int32_t relu_a, int32_t act, int32_t prec, int32_t no_dma, void* stream) {
    if (ldw != K) return fail(VLSAT_EINVAL, "gemm_bf16: W must be dense [N,K] (the planes are made from it)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)N * K;
    uint16_t *hi = nullptr, *lo = nullptr;
    VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&hi), n * 2 + 256));
    VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&lo), n * 2 + 256));
    int r = launch_split_bf16(W, n, hi, lo, st);
    if (!r) r = vlsat_k_gemm_planes(A, lda, W, hi, lo, ldw, C, ldc, M, N, K, bias, resid, ldr, resid_scale, g0, gi0, ldg0, g1, gi1,
                                    ldg1, relu_a, act, prec, no_dma, -1, 0, 1.f, stream);
    hipStreamSynchronize(st);
    hipFree(hi);
    hipFree(lo);
    return r;
}

// include/vlsat_gemm.h -- w[i] 2^k -> fp16 hi[i] + fp16 lo[i] with the tensor's exponent k (gemm_f16s_planes.h): the planes the split-fp16
// 8-phase GEMM reads.  Allocates two words of scratch and synchronises the stream (k comes back to the host): a test entry point.
int vlsat_k_split_f16s(const float* w, size_t n, uint16_t* hi, uint16_t* lo, int32_t* k, void* stream) {
    if (!w || !hi || !lo || !k) return fail(VLSAT_EINVAL, "split_f16s: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned* scratch = nullptr;
    *k = 0;
    if (!n) return 0;
    VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&scratch), 256));
    int r = launch_split_f16s(w, n, hi, lo, scratch, st);
    if (!r && hipMemcpyAsync(k, scratch + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess) r = fail(VLSAT_EHIP, "split_f16s: copy failed");
    hipStreamSynchronize(st);
    hipFree(scratch);
    return r;
}

// vlsat_k_gemm as the fp32 precision mode runs an edge-row launch: the planes of a dense W [N,K] are made on the spot (allocates,
// synchronises), the full rounds of a launch the planner sends to the 8-phase kernel run on its split-fp16 sibling, everything else on the
// exact kernels.  p8_part_min >= 0: GemmArgs::p8_part_min (tests reach the 8-phase kernel with a few tiles); v < 0: GemmArgs::f16s = 2 -- the
// launches of the persistent kernel run on their split-fp16 siblings as well -- with p8_part_min = -1 - v.  relu_a: bit 0 only.
int vlsat_k_gemm_f16s(const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc, int32_t M, int32_t N,
                      int32_t K, const float* bias, const float* rowscale, const float* resid, int32_t ldr, float resid_scale,
                      const float* g0, const int32_t* gi0, int32_t ldg0, const float* g1, const int32_t* gi1, int32_t ldg1,
                      int32_t relu_a, int32_t act, int32_t p8_part_min, void* stream) {
    if (!W || ldw != K || N <= 0 || K <= 0) return fail(VLSAT_EINVAL, "gemm_f16s: W must be dense [N,K] (the planes are made from it)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)N * K;
    GemmArgs a;
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.rowscale = rowscale; a.resid = resid; a.ldr = ldr; a.resid_scale = resid_scale;
    a.g0 = g0; a.gi0 = gi0; a.ldg0 = ldg0; a.g1 = g1; a.gi1 = gi1; a.ldg1 = ldg1; a.relu_a = relu_a & 1; a.act = act;
    const int f16s = p8_part_min < 0 ? 2 : 1;        // v < 0: the persistent kernel's launches on their siblings too, p8_part_min = -1 - v
    a.p8_part_min = p8_part_min < 0 ? -1 - p8_part_min : p8_part_min;
    uint16_t *hi = nullptr, *lo = nullptr;
    VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&hi), n * 2 + 256));
    VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&lo), n * 2 + 256));
    int32_t k = 0;
    int r = vlsat_k_split_f16s(W, n, hi, lo, &k, stream);
    if (!r) {
        a.f16s = f16s; a.Wh16 = hi; a.Wl16 = lo; a.w_exp = k;
        r = launch_gemm(a, st);
    }
    hipStreamSynchronize(st);
    hipFree(hi);
    hipFree(lo);
    return r;
}

int vlsat_k_pointnet(const float* pts, int32_t n_obj, int32_t n_points, const float* w1, const float* b1,
                     const float* w2, const float* b2, const float* w3, const float* b3, int32_t n_out, float* out,
                     void* stream) {
    return launch_pointnet(pts, n_obj, n_points, 3, w1, b1, w2, b2, w3, b3, n_out, out, static_cast<hipStream_t>(stream));
}

namespace {
struct DevTable {                       // a host table copied to the device for the duration of one call
    void* d = nullptr;
    ~DevTable() { if (d) hipFree(d); }
    int alloc(size_t bytes) {           // (or scratch of one call, uninitialised)
        VLSAT_HIP_CHECK(hipMalloc(&d, bytes));
        return 0;
    }
    int put(const void* host, size_t bytes) {
        if (!bytes) return 0;
        VLSAT_HIP_CHECK(hipMalloc(&d, bytes));
        VLSAT_HIP_CHECK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        return 0;
    }
};
// the FLASH_BQ-query tiles (scene start, scene tokens, first query, head) of a test call's attention, uploaded; *n = their count
static int flash_tiles(const int64_t* tok_ptr, int n_scenes, int n_heads, DevTable& d, int* n) {
    if (!tok_ptr || n_scenes <= 0) return fail(VLSAT_EINVAL, "flash_attn: bad scene table");
    std::vector<PlanTile> tiles;                 // (int4's size and alignment: engine_plan.hip)
    for (int s = 0; s < n_scenes; ++s) append_tile_rows(tiles, tok_ptr[s], tok_ptr[s + 1] - tok_ptr[s], n_heads, FLASH_BQ);
    *n = (int)tiles.size();
    return d.put(tiles.data(), tiles.size() * sizeof(PlanTile));
}
}  // namespace

int vlsat_k_flash_attn(const float* Q, const float* K, const float* V, float* O, int32_t ld, const int64_t* tok_ptr,
                       int32_t n_scenes, int32_t n_heads, float scale, void* stream) {
    DevTable d;
    int n = 0;
    RUN(flash_tiles(tok_ptr, n_scenes, n_heads, d, &n));
    if (!n) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int r = launch_flash_attn(Q, ld, K, V, ld, O, ld, static_cast<const int4*>(d.d), n, scale * 1.4426950408889634f, st);
    hipStreamSynchronize(st);     // test entry point only: the tile table is freed right away
    return r;
}

int vlsat_k_flash_attn_bf16(const float* Q, const float* K, const float* V, float* O, int32_t ld, const int64_t* tok_ptr,
                            int32_t n_scenes, int32_t n_heads, float scale, int32_t terms, int32_t use_tr, void* stream) {
    DevTable d;
    int n = 0;
    RUN(flash_tiles(tok_ptr, n_scenes, n_heads, d, &n));
    if (!n) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    FlashSplit sp;                              // (no split keys; rows = the tensors' rows: lets the half-row variant take its LDS-direct staging)
    sp.rows = (int)tok_ptr[n_scenes];
    int r = launch_flash_attn_bf16(Q, ld, K, V, ld, O, ld, static_cast<const int4*>(d.d), n, scale * 1.4426950408889634f, terms, use_tr != 0,
                                   use_tr == 2 ? 1 : use_tr == 3 ? 2 : 0, st, &sp);
    hipStreamSynchronize(st);     // test entry point only: the tile table is freed right away
    return r;
}

// key_parts > 1: the split-key path on a table made here -- every tile key_parts times, part p of a scene of kt 32-key tiles covers
// tiles [kt p / key_parts, kt (p + 1) / key_parts), empty parts included (more parts than tiles: a part without keys, and, where it
// starts at an odd tile, one whose only 64-key tile is masked throughout)
int vlsat_k_flash_attn_f16x3(const float* Q, const float* K, const float* V, float* O, int32_t ld, const int64_t* tok_ptr,
                             int32_t n_scenes, int32_t n_heads, float scale, int32_t key_parts, int32_t use_tr, void* stream) {
    if (key_parts < 1 || key_parts > 64) return fail(VLSAT_EINVAL, "flash_attn_f16x3: key_parts must be 1..64");
    if (!tok_ptr || n_scenes <= 0) return fail(VLSAT_EINVAL, "flash_attn: bad scene table");
    std::vector<PlanTile> tiles, split, krange;
    for (int s = 0; s < n_scenes; ++s) append_tile_rows(tiles, tok_ptr[s], tok_ptr[s + 1] - tok_ptr[s], n_heads, FLASH_BQ);
    if (tiles.empty()) return 0;
    const int rows = (int)tok_ptr[n_scenes];
    FlashSplit sp;
    sp.rows = rows;
    DevTable d, dk, dw;
    if (key_parts > 1) {
        for (const PlanTile& t : tiles) {
            const int kt = (t.y + 31) / 32;
            for (int p = 0; p < key_parts; ++p) {
                split.push_back(t);
                krange.push_back({(int)((int64_t)kt * p / key_parts), (int)((int64_t)kt * (p + 1) / key_parts), p, 0});
            }
        }
        tiles.swap(split);
        RUN(dk.put(krange.data(), krange.size() * sizeof(PlanTile)));
        const size_t o_floats = (size_t)key_parts * rows * ld, ml_floats = (size_t)key_parts * rows * n_heads;
        std::vector<float> zeros(o_floats + 2 * ml_floats, 0.f);
        RUN(dw.put(zeros.data(), zeros.size() * sizeof(float)));
        sp.parts = key_parts; sp.krange = static_cast<const int4*>(dk.d); sp.heads = n_heads; sp.part_stride = (size_t)rows * ld;
        sp.o_part = static_cast<float*>(dw.d); sp.m_part = sp.o_part + o_floats; sp.l_part = sp.m_part + ml_floats;
    }
    RUN(d.put(tiles.data(), tiles.size() * sizeof(PlanTile)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int r = launch_flash_attn_f16x3(Q, ld, K, V, ld, O, ld, static_cast<const int4*>(d.d), (int)tiles.size(), scale * 1.4426950408889634f, use_tr, st, &sp);
    hipStreamSynchronize(st);     // test entry point only: the tables are freed right away
    return r;
}

int vlsat_prepare_objects(const float* scene_points, const int32_t* choice, int32_t n_obj, int32_t n_points,
                          float* obj_points, float* descriptor, void* stream) {
    if (!scene_points || !choice || !obj_points || !descriptor) return fail(VLSAT_EINVAL, "prepare_objects: null argument");
    return launch_prepare_objects(scene_points, choice, n_obj, n_points, obj_points, descriptor, static_cast<hipStream_t>(stream));
}

// Per-object point selection on the device (the step in front of vlsat_prepare_objects; reference dataset_3dssg.py:279-289): see
// include/vlsat.h.  vlsat_sample_objects_scratch gives the int32 count of `scratch`.
size_t vlsat_sample_objects_scratch(int64_t n_points, int32_t n_obj) { return sample_objects_scratch_ints(n_points, n_obj); }
int vlsat_sample_objects(const int32_t* instances, int64_t n_points, const int32_t* instance_ids, int32_t n_obj, int32_t n_sample,
                         uint64_t seed, int32_t* id_map, int32_t map_size, int32_t* scratch, int32_t* choice, int32_t* counts, void* stream) {
    if (!instances || !instance_ids || !id_map || !scratch || !choice || !counts) return fail(VLSAT_EINVAL, "sample_objects: null argument");
    return launch_sample_objects(instances, n_points, instance_ids, n_obj, n_sample, seed, id_map, map_size, scratch, choice, counts,
                                 static_cast<hipStream_t>(stream));
}

int vlsat_fc_edges(const int32_t* node_ptr, const int64_t* edge_ptr, int32_t n_scenes, int64_t n_nodes, int64_t n_edges,
                   int64_t* edges, int64_t* batch_ids, void* stream) {
    if (!node_ptr || !edge_ptr || !batch_ids || (n_edges > 0 && !edges) || n_scenes <= 0)
        return fail(VLSAT_EINVAL, "fc_edges: bad argument");
    return launch_fc_edges(node_ptr, edge_ptr, n_scenes, n_nodes, n_edges, edges, batch_ids, static_cast<hipStream_t>(stream));
}

// Proximity-pruned edge lists (csrc/proximity.hip; the rule is stated in include/vlsat.h)
int vlsat_instance_boxes(const int32_t* instances, const float* scene_points, int64_t n_points, const int32_t* instance_ids, int32_t n_obj,
                         int32_t* id_map, int32_t map_size, float* boxes, void* stream) {
    if (!instance_ids || !id_map || !boxes || (n_points > 0 && (!instances || !scene_points)))
        return fail(VLSAT_EINVAL, "instance_boxes: null argument");
    return launch_instance_boxes(instances, scene_points, n_points, instance_ids, n_obj, id_map, map_size, boxes, static_cast<hipStream_t>(stream));
}
int32_t vlsat_proximity_lds_boxes(void) { return proximity_lds_boxes(); }
size_t vlsat_proximity_scratch_bytes(int64_t n_nodes) { return proximity_scratch_bytes(n_nodes); }
int vlsat_proximity_count(const float* boxes, const int32_t* node_ptr, int32_t n_scenes, int64_t n_nodes, float padding, int32_t max_neighbors,
                          void* scratch, int64_t* edge_ptr, int64_t* batch_ids, void* stream) {
    if (!node_ptr || !edge_ptr || (n_nodes > 0 && (!boxes || !scratch || !batch_ids))) return fail(VLSAT_EINVAL, "proximity_count: null argument");
    return launch_proximity_count(boxes, node_ptr, n_scenes, n_nodes, padding, max_neighbors, scratch, edge_ptr, batch_ids,
                                  static_cast<hipStream_t>(stream));
}
int vlsat_proximity_fill(const float* boxes, const int32_t* node_ptr, int32_t n_scenes, int64_t n_nodes, float padding, int32_t max_neighbors,
                         const void* scratch, int64_t n_edges, int64_t capacity, int64_t* edges, void* stream) {
    if (!node_ptr || (n_nodes > 0 && (!boxes || !scratch)) || (n_edges > 0 && !edges)) return fail(VLSAT_EINVAL, "proximity_fill: null argument");
    return launch_proximity_fill(boxes, node_ptr, n_scenes, n_nodes, padding, max_neighbors, scratch, n_edges, capacity, edges,
                                 static_cast<hipStream_t>(stream));
}

// Annotation transfer onto a predicted segmentation (csrc/label_transfer.hip; the rule is stated in include/vlsat.h)
size_t vlsat_nearest_points_scratch_bytes(int64_t n_query, int64_t n_ref) { return nearest_points_scratch_bytes(n_query, n_ref); }
int vlsat_nearest_points(const float* query, int64_t n_query, const float* ref, int64_t n_ref, float max_sq_dist, void* scratch,
                         int32_t* nn_index, float* nn_sqdist, void* stream) {
    if (n_query > 0 && (!query || !nn_index || !nn_sqdist || (n_ref > 0 && (!ref || !scratch))))
        return fail(VLSAT_EINVAL, "nearest_points: null argument");
    return launch_nearest_points(query, n_query, ref, n_ref, max_sq_dist, scratch, nn_index, nn_sqdist, static_cast<hipStream_t>(stream));
}
size_t vlsat_segment_overlap_scratch_bytes(int32_t seg_map_size, int32_t gt_map_size) {
    return segment_overlap_scratch_bytes(seg_map_size, gt_map_size);
}
int vlsat_segment_overlap(const int32_t* pd_segments, const int32_t* nn_index, int64_t n_query, const int32_t* gt_instances, int64_t n_ref,
                          const int32_t* segment_ids, int32_t n_seg, const int32_t* gt_ids, int32_t n_gt, int32_t* id_maps,
                          int32_t seg_map_size, int32_t gt_map_size, int32_t min_seg_size, double corr_thres, double occ_thres,
                          int32_t occ_min_candidates, int32_t* size, int32_t* counts, int32_t* match, int32_t* best, int32_t* second,
                          int32_t* n_candidates, void* stream) {
    if (n_seg > 0 && (!segment_ids || !id_maps || !size || !match || !best || !second || !n_candidates || (n_gt > 0 && (!gt_ids || !counts)) ||
                      (n_query > 0 && (!pd_segments || !nn_index)) || (n_ref > 0 && !gt_instances)))
        return fail(VLSAT_EINVAL, "segment_overlap: null argument");
    return launch_segment_overlap(pd_segments, nn_index, n_query, gt_instances, n_ref, segment_ids, n_seg, gt_ids, n_gt, id_maps, seg_map_size,
                                  gt_map_size, min_seg_size, corr_thres, occ_thres, occ_min_candidates, size, counts, match, best, second,
                                  n_candidates, static_cast<hipStream_t>(stream));
}

// Segments merged into objects along "same part" edges (csrc/segment_merge.hip; the rule is stated in include/vlsat.h)
size_t vlsat_merge_segments_scratch_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes) {
    if (merge_segments_check_args(n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes)) return 0;
    return merge_segments_scratch_bytes(n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes);
}
int vlsat_merge_segments(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids, const float* weights,
                         int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes, int32_t same_part,
                         float threshold, int32_t mutual, void* scratch, int32_t* root, int32_t* object, int32_t* n_objects, int32_t* totals,
                         int32_t* member_ptr, int32_t* members, float* merged_probs, float* obj_weight, int64_t* obj_batch_ids,
                         int32_t* edge_to_pair, int64_t* pair_edges, int32_t* pair_count, float* pair_probs, void* stream) {
    RUN(merge_segments_check_args(n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes));
    if (same_part < 0 || same_part >= n_rel_class) return fail(VLSAT_EINVAL, "merge_segments: same_part is not a predicate class");
    if (threshold != threshold) return fail(VLSAT_EINVAL, "merge_segments: threshold is NaN");
    if (mutual != 0 && mutual != 1) return fail(VLSAT_EINVAL, "merge_segments: mutual must be 0 or 1");
    if (n_scenes > 1 && !batch_ids) return fail(VLSAT_EINVAL, "merge_segments: batch_ids is required for more than one scene");
    if (n_nodes > 0 && n_scenes < 1) return fail(VLSAT_EINVAL, "merge_segments: nodes without a scene");
    if (!scratch || !totals || !member_ptr || (n_scenes > 0 && !n_objects))
        return fail(VLSAT_EINVAL, "merge_segments: null output or scratch");
    if (n_nodes > 0 && (!obj_probs || !root || !object || !members || !merged_probs || !obj_weight || !obj_batch_ids))
        return fail(VLSAT_EINVAL, "merge_segments: null node argument");
    if (n_edges > 0 && (!rel_probs || !edges || !edge_to_pair || !pair_edges || !pair_count || !pair_probs))
        return fail(VLSAT_EINVAL, "merge_segments: null edge argument");
    return launch_merge_segments(obj_probs, rel_probs, edges, batch_ids, weights, n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes, same_part,
                                 threshold, mutual, scratch, root, object, n_objects, totals, member_ptr, members, merged_probs, obj_weight,
                                 obj_batch_ids, edge_to_pair, pair_edges, pair_count, pair_probs, static_cast<hipStream_t>(stream));
}

int vlsat_k_softmax_rows(const float* x, int32_t ld, int32_t rows, int32_t cols, float* out, void* stream) {
    if (!x || !out) return fail(VLSAT_EINVAL, "softmax_rows: null argument");
    return launch_softmax_rows(x, ld, rows, cols, out, 0, static_cast<hipStream_t>(stream));
}

int vlsat_eval_ranks(const float* obj_logits, const float* obj_probs, const float* rel_probs, const int64_t* gt_class,
                     const int64_t* gt_rel, const int64_t* edges, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class,
                     int32_t n_rel_class, int32_t topk_obj, int32_t topk_rel, int32_t topk_triplet, float threshold,
                     int32_t* obj_rank, int32_t* rel_rank, int32_t* tri_rank, int32_t* cnt, float* scratch, void* stream) {
    if (!obj_logits || !obj_probs || !gt_class || !obj_rank) return fail(VLSAT_EINVAL, "eval_ranks: null argument");
    if (n_edges > 0 && (!rel_probs || !gt_rel || !edges || !rel_rank || !tri_rank || !cnt || !scratch))
        return fail(VLSAT_EINVAL, "eval_ranks: null edge argument");
    return launch_eval_ranks(obj_logits, obj_probs, rel_probs, gt_class, gt_rel, edges, n_nodes, n_edges, n_obj_class,
                             n_rel_class, topk_obj, topk_rel, topk_triplet, threshold, obj_rank, rel_rank, tri_rank, cnt, scratch,
                             static_cast<hipStream_t>(stream), false);
}

int64_t vlsat_eval_ranks_scratch_floats(int32_t n_nodes, int32_t n_obj_class, int32_t topk_triplet) {
    if (n_nodes < 0 || n_obj_class < 0 || topk_triplet < 0) return 0;
    return (int64_t)n_nodes * eval_ranks_sorted_k(n_obj_class, topk_triplet);
}

int64_t vlsat_eval_recallk_scratch_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes) {
    if (n_nodes < 0 || n_edges < 0 || n_obj_class < 0 || n_rel_class < 0 || n_scenes < 0) return 0;
    return (int64_t)eval_recallk_scratch_bytes(n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes);
}

int vlsat_eval_recallk(const float* obj_probs, const float* rel_probs, const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges,
                       const int64_t* batch_ids, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                       int32_t n_scenes, int32_t variants_mask, void* scratch, int64_t* counts, void* stream) {
    if (n_scenes > 0 && (!counts || !scratch)) return fail(VLSAT_EINVAL, "eval_recallk: null counts or scratch");
    if (n_edges > 0 && (!rel_probs || !gt_rel || !edges || ((variants_mask & 12) && (!obj_probs || !gt_class))))
        return fail(VLSAT_EINVAL, "eval_recallk: null edge argument");
    if (n_scenes > 1 && !batch_ids) return fail(VLSAT_EINVAL, "eval_recallk: batch_ids is required for more than one scene");
    return launch_eval_recallk(obj_probs, rel_probs, gt_class, gt_rel, edges, batch_ids, n_nodes, n_edges, n_obj_class, n_rel_class,
                               n_scenes, variants_mask, scratch, reinterpret_cast<long long*>(counts), static_cast<hipStream_t>(stream));
}

int vlsat_eval_counts(const int32_t* obj_rank_3d, const int32_t* obj_rank_2d, const int32_t* rel_rank_3d, const int32_t* rel_rank_2d,
                      const int32_t* tri_rank_3d, const int32_t* tri_rank_2d, const int32_t* cnt, const int64_t* gt_class,
                      const int64_t* gt_rel, const int64_t* edges, int32_t n_nodes, int32_t n_edges, int32_t n_rel_class,
                      int32_t n_scenes, uint64_t* counts, void* stream) {
    if (!counts || n_nodes < 0 || n_edges < 0) return fail(VLSAT_EINVAL, "eval_counts: bad argument");
    // the three 2D tables go together: all NULL counts the 3D branch alone (a table without rows -- n_nodes / n_edges = 0 -- is not looked at)
    const bool two = obj_rank_2d || rel_rank_2d || tri_rank_2d;
    if (two && ((n_nodes > 0 && !obj_rank_2d) || (n_edges > 0 && (!rel_rank_2d || !tri_rank_2d))))
        return fail(VLSAT_EINVAL, "eval_counts: the 2D rank tables go together (obj, rel and tri: all, or none for the 3D branch alone)");
    if (n_nodes > 0 && (!obj_rank_3d || !gt_class)) return fail(VLSAT_EINVAL, "eval_counts: null node argument");
    if (n_edges > 0 && (!rel_rank_3d || !tri_rank_3d || !cnt || !gt_rel || !edges || !gt_class || !obj_rank_3d))
        return fail(VLSAT_EINVAL, "eval_counts: null edge argument");
    return launch_eval_counts(obj_rank_3d, obj_rank_2d, rel_rank_3d, rel_rank_2d, tri_rank_3d, tri_rank_2d, cnt, gt_class, gt_rel, edges,
                              n_nodes, n_edges, n_rel_class, n_scenes, reinterpret_cast<unsigned long long*>(counts),
                              static_cast<hipStream_t>(stream));
}

int vlsat_eval_triplet_split(const int32_t* tri_rank_3d, const int32_t* tri_rank_2d, const int32_t* cnt, const int64_t* gt_class,
                             const int64_t* gt_rel, const int64_t* edges, const uint8_t* table, int32_t n_edges, int32_t n_obj_class,
                             int32_t n_rel_class, uint64_t* counts, void* stream) {
    if (!counts || n_edges < 0) return fail(VLSAT_EINVAL, "eval_triplet_split: bad argument");
    // (tri_rank_2d NULL: the 3D half of counts alone)
    if (n_edges > 0 && (!tri_rank_3d || !cnt || !gt_class || !gt_rel || !edges || !table))
        return fail(VLSAT_EINVAL, "eval_triplet_split: null edge argument");
    return launch_eval_triplet_split(tri_rank_3d, tri_rank_2d, cnt, gt_class, gt_rel, edges, table, n_edges, n_obj_class, n_rel_class,
                                     reinterpret_cast<unsigned long long*>(counts), static_cast<hipStream_t>(stream));
}

// One scene (or batch) of an evaluation loop in ONE call: forward + softmax of the object logits + both ranking passes + the
// additive counts (vlsat_forward, vlsat_k_softmax_rows, vlsat_eval_ranks x 2, vlsat_eval_counts), all enqueued on `stream`,
// intermediates in the plan's own scratch -- what Mmgnet.process_val (reference SGFN_MMG/model.py:458-480) computes per scene,
// reduced to what MMGNet.validation keeps of it.  The host side of a one-scene-per-call loop is then one library call per scene
// instead of six plus a dozen tensor allocations.  gt_rel: the multi-hot [E, R] int64 target; edges_e2: [E, 2] int64 (from, to) as
// the loader yields it, in the plan's edge order; counts: device uint64 [1 + R + 2 (11 + 6 R)], zeroed once by the caller.
// Top-k bounds and threshold are process_val's constants (topk 11 / 6 / 101, 0.5: reference :463-472).
// Single-label handles (MODEL.multi_rel_outputs = false) take the same call: gt_rel is the one-hot row of the label with column 0
// ("none") cleared, the predicate ranks use the log-probabilities as they are and the triplet ranks their exp, taken inside the
// triplet kernel (launch_eval_ranks, rel_is_log) -- the counts of vlsat_eval_ranks on rel and on vlsat_k_exp(rel), in one pass.
// split_table / split_counts (vlsat_process_val_counts_split): the zero-shot split of the triplet ranks is counted as well.
// obj_2d_feats NULL: the 3D-only step -- vlsat_forward without its 2D outputs, one softmax, one ranking pass, the one-branch counts and
// split; the 2D blocks of counts / split_counts are not touched and the plan's scratch is the same (its 2D halves stay unused).
static int process_val_counts(vlsat_handle h, vlsat_plan p, const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                              const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges_e2, int32_t n_scenes,
                              uint64_t* counts, const uint8_t* split_table, uint64_t* split_counts, void* stream) {
    if (!h || !p || !gt_class || !counts) return fail(VLSAT_EINVAL, "vlsat_process_val_counts: null argument");
    if (p->h != h) return fail(VLSAT_EINVAL, "plan belongs to a different handle");
    const int N = (int)p->N, E = (int)p->E, C = h->d.n_obj_class, R = h->d.n_rel_class;
    if (E > 0 && (!gt_rel || !edges_e2)) return fail(VLSAT_EINVAL, "vlsat_process_val_counts: null edge argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EvalScratch v = eval_scratch_carve(p->ev_f, p->ev_i, N, E, C, R);        // (sorted: [N, min(C, 101)] of it)
    // obj_2d_feats NULL: the 3D-only step -- the 3D-only forward, one softmax, one ranking pass, the one-branch counts (and split); the 2D
    // halves of the scratch are not touched, the 2D blocks of counts / split_counts neither
    const bool do2d = obj_2d_feats != nullptr;
    // single-label model: the relation outputs are log-probabilities -- the predicate ranks take them as they are, the triplet kernel
    // exponentiates on load; still one ranking pass per branch, the same scratch, no [E, R] temporary
    const bool rel_is_log = !h->d.multi_rel_outputs;
    RUN(vlsat_forward(h, p, obj_points, obj_2d_feats, descriptor, v.obj3, do2d ? v.obj2 : nullptr, v.rel3, do2d ? v.rel2 : nullptr, stream));
    for (int br = 0; br < (do2d ? 2 : 1); ++br) {
        const float* lg = br ? v.obj2 : v.obj3;
        float* pr = br ? v.prob2 : v.prob3;
        RUN(launch_softmax_rows(lg, C, N, C, pr, 0, s));
        RUN(launch_eval_ranks(lg, pr, br ? v.rel2 : v.rel3, gt_class, gt_rel, edges_e2, N, E, C, R, 11, 6, 101, 0.5f, br ? v.or2 : v.or3,
                              br ? v.rr2 : v.rr3, br ? v.tr2 : v.tr3, br ? v.cn2 : v.cn3, v.sorted, s, rel_is_log));
    }
    RUN(launch_eval_counts(v.or3, do2d ? v.or2 : nullptr, v.rr3, do2d ? v.rr2 : nullptr, v.tr3, do2d ? v.tr2 : nullptr, v.cn3, gt_class, gt_rel,
                           edges_e2, N, E, R, n_scenes, reinterpret_cast<unsigned long long*>(counts), s));
    if (split_counts)
        RUN(launch_eval_triplet_split(v.tr3, do2d ? v.tr2 : nullptr, v.cn3, gt_class, gt_rel, edges_e2, split_table, E, C, R,
                                      reinterpret_cast<unsigned long long*>(split_counts), s));
    VLSAT_HIP_CHECK(hipEventRecord(p->last_use, s));       // (the scratch is the plan's: its next owner orders behind the counting)
    return 0;
}

int vlsat_process_val_counts(vlsat_handle h, vlsat_plan p, const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                             const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges_e2, int32_t n_scenes,
                             uint64_t* counts, void* stream) {
    return process_val_counts(h, p, obj_points, obj_2d_feats, descriptor, gt_class, gt_rel, edges_e2, n_scenes, counts, nullptr, nullptr,
                              stream);
}

// vlsat_process_val_counts + the zero-shot split of the triplet ranks (vlsat_eval_triplet_split) on the plan-scratch rank tables:
// a one-scene-per-call loop with the split on stays one library call per scene.  split_table: uint8 [C*C*R] of the model's classes.
int vlsat_process_val_counts_split(vlsat_handle h, vlsat_plan p, const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                                   const int64_t* gt_class, const int64_t* gt_rel, const int64_t* edges_e2, int32_t n_scenes,
                                   uint64_t* counts, const uint8_t* split_table, uint64_t* split_counts, void* stream) {
    if (!split_table || !split_counts) return fail(VLSAT_EINVAL, "vlsat_process_val_counts_split: null split table or counts");
    return process_val_counts(h, p, obj_points, obj_2d_feats, descriptor, gt_class, gt_rel, edges_e2, n_scenes, counts, split_table,
                              split_counts, stream);
}

// out = exp(x), n floats (out may be x): the predicate probabilities of a single-label model, by the kernel vlsat_forward_scene_graph uses
int vlsat_k_exp(const float* x, int64_t n, float* out, void* stream) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(VLSAT_EINVAL, "k_exp: bad argument");
    return launch_exp(x, out, (size_t)n, static_cast<hipStream_t>(stream));
}

// The predicted scene graph of every scene of a batch (scene_graph.hip; contract and tie rule: include/vlsat.h)
int64_t vlsat_scene_graph_scratch_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes,
                                        int32_t top_k, int32_t topk_each) {
    if (n_nodes < 0 || n_edges < 0 || n_scenes < 0 || scene_graph_check_args(n_obj_class, n_rel_class, 0, top_k, topk_each)) return 0;
    return (int64_t)scene_graph_scratch_bytes(n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes, topk_each);
}

int vlsat_scene_graph_topk(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids,
                           int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes, int32_t mode,
                           int32_t top_k, int32_t topk_each, void* scratch, int32_t* triplets, float* scores, int32_t* n_valid,
                           void* stream) {
    RUN(scene_graph_check_args(n_obj_class, n_rel_class, mode, top_k, topk_each));
    if (n_scenes > 0 && (!triplets || !scores || !n_valid || !scratch)) return fail(VLSAT_EINVAL, "scene_graph_topk: null output or scratch");
    if (n_edges > 0 && (!rel_probs || !edges || (mode == 0 && !obj_probs))) return fail(VLSAT_EINVAL, "scene_graph_topk: null edge argument");
    if (n_scenes > 1 && !batch_ids) return fail(VLSAT_EINVAL, "scene_graph_topk: batch_ids is required for more than one scene");
    if (n_scenes < 0 || n_nodes < 0 || n_edges < 0) return fail(VLSAT_EINVAL, "scene_graph_topk: bad sizes");
    const SceneGraphWs ws = scene_graph_carve(scratch, n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes, topk_each);
    return launch_scene_graph_topk(obj_probs, rel_probs, edges, batch_ids, nullptr, n_nodes, n_edges, n_obj_class, n_rel_class, n_scenes,
                                   mode, top_k, topk_each, ws, triplets, scores, n_valid, static_cast<hipStream_t>(stream));
}

// The label-free sibling of vlsat_process_val_counts: forward + softmax of both object heads + the selection for both branches,
// enqueued back to back on `stream`, one library call per scene.  Every intermediate lives in the plan's memory: logits,
// probabilities and predicate scores in the evaluation scratch (the class indices of the node argsort take the place of a branch's
// logits once its softmax has run, the sorted values the ranking's sorted-probability table), the scene offsets in the rank
// scratch, and the candidate slots (8 bytes x topk_each per edge) in Hbig, the 4 KB-per-edge hidden buffer that is dead once the
// forward has finished -- the arena does not grow.  With MODEL.multi_rel_outputs = false the log-probabilities are exponentiated
// in place first.
// obj_2d_feats and the three 2D outputs go together: all NULL runs the 3D-only forward and one selection; a mixture is refused.
int vlsat_forward_scene_graph(vlsat_handle h, vlsat_plan p, const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                              const int64_t* edges_e2, int32_t n_scenes, int32_t mode, int32_t top_k, int32_t topk_each,
                              int32_t* triplets_3d, float* scores_3d, int32_t* n_valid_3d, int32_t* triplets_2d, float* scores_2d,
                              int32_t* n_valid_2d, void* stream) {
    if (!h || !p) return fail(VLSAT_EINVAL, "vlsat_forward_scene_graph: null argument");
    if (p->h != h) return fail(VLSAT_EINVAL, "plan belongs to a different handle");
    const int N = (int)p->N, E = (int)p->E, C = h->d.n_obj_class, R = h->d.n_rel_class;
    RUN(scene_graph_check_args(C, R, mode, top_k, topk_each));
    if (n_scenes != p->S) return fail(VLSAT_EINVAL, "vlsat_forward_scene_graph: n_scenes is not the plan's scene count");
    if (!triplets_3d || !scores_3d || !n_valid_3d) return fail(VLSAT_EINVAL, "vlsat_forward_scene_graph: null 3D output");
    const bool any2 = triplets_2d || scores_2d || n_valid_2d;
    const bool all2 = triplets_2d && scores_2d && n_valid_2d;
    const bool do2d = obj_2d_feats != nullptr;
    if (do2d ? !all2 : any2)
        return fail(VLSAT_EINVAL, "vlsat_forward_scene_graph: obj_2d_feats and the three 2D outputs go together (all, or none for 3D-only)");
    if (E > 0 && !edges_e2) return fail(VLSAT_EINVAL, "vlsat_forward_scene_graph: null edge argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EvalScratch v = eval_scratch_carve(p->ev_f, p->ev_i, N, E, C, R);
    RUN(vlsat_forward(h, p, obj_points, obj_2d_feats, descriptor, v.obj3, do2d ? v.obj2 : nullptr, v.rel3, do2d ? v.rel2 : nullptr, stream));
    for (int br = 0; br < (do2d ? 2 : 1); ++br) {
        float* lg = br ? v.obj2 : v.obj3;
        float* pr = br ? v.prob2 : v.prob3;
        float* rl = br ? v.rel2 : v.rel3;
        RUN(launch_softmax_rows(lg, C, N, C, pr, 0, s));
        if (!h->d.multi_rel_outputs) RUN(launch_exp(rl, rl, (size_t)E * R, s));
        SceneGraphWs ws;
        ws.sv = v.sorted;                                       // ([N, min(C, 100)] of the [N, C] the plan holds)
        ws.si = reinterpret_cast<int32_t*>(lg);                 // (the logits are dead behind the softmax)
        ws.ptr = v.or3;                                         // (the rank scratch from its start: S + 1 <= 2 max(N, 1) entries)
        ws.keys = reinterpret_cast<uint32_t*>(p->Hbig);         // (2 x E x <= 100 of the E x 1024 words)
        ws.packs = ws.keys + (size_t)std::max(E, 1) * 100;
        RUN(launch_scene_graph_topk(pr, rl, edges_e2, nullptr, p->d_scene_ptr, N, E, C, R, n_scenes, mode, top_k, topk_each, ws,
                                    br ? triplets_2d : triplets_3d, br ? scores_2d : scores_3d, br ? n_valid_2d : n_valid_3d, s));
    }
    VLSAT_HIP_CHECK(hipEventRecord(p->last_use, s));       // (the scratch is the plan's: its next owner orders behind the selection)
    return 0;
}

int vlsat_scene_checksums(const float* obj3d, const float* obj2d, int64_t n_nodes, int32_t n_obj_class, const float* rel3d,
                          const float* rel2d, int64_t n_edges, int32_t n_rel_class, int32_t n_scenes, double* out9, double* scratch,
                          void* stream) {
    if (!obj3d || !obj2d || !out9 || !scratch || n_nodes < 0 || n_edges < 0) return fail(VLSAT_EINVAL, "scene_checksums: null argument");
    if (n_edges > 0 && (!rel3d || !rel2d)) return fail(VLSAT_EINVAL, "scene_checksums: null relation outputs");
    return launch_scene_checksums(obj3d, obj2d, (long)n_nodes, n_obj_class, rel3d, rel2d, (long)n_edges, n_rel_class, n_scenes, out9,
                                  scratch, static_cast<hipStream_t>(stream));
}

// The decoded scene graph of every scene of a batch (graph_decode.hip; contract: include/vlsat.h)
int64_t vlsat_graph_decode_scratch_bytes(int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t n_scenes, int32_t n_labels,
                                         int32_t max_rel) {
    if (n_edges < 0 || n_scenes < 0 || graph_decode_check_args(n_obj_class, n_rel_class, 1, 0, n_labels, max_rel)) return 0;
    return (int64_t)graph_decode_scratch_bytes(n_edges, n_rel_class, n_scenes);
}

int vlsat_graph_decode(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids,
                       const float* thresholds, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                       int32_t n_scenes, int32_t multi_label, int32_t score_mode, int32_t n_labels, int32_t max_rel, void* scratch,
                       int32_t* labels, float* label_probs, int32_t* rels, float* scores, int32_t* n_valid, int32_t* n_total,
                       void* stream) {
    RUN(graph_decode_check_args(n_obj_class, n_rel_class, multi_label, score_mode, n_labels, max_rel));
    if (n_scenes < 0 || n_nodes < 0 || n_edges < 0) return fail(VLSAT_EINVAL, "graph_decode: bad sizes");
    if (n_nodes > 0 && (!obj_probs || !labels || !label_probs)) return fail(VLSAT_EINVAL, "graph_decode: null node argument");
    if (n_scenes > 0 && (!rels || !scores || !n_valid || !n_total || !scratch)) return fail(VLSAT_EINVAL, "graph_decode: null output or scratch");
    if (n_edges > 0 && (!rel_probs || !edges || !thresholds)) return fail(VLSAT_EINVAL, "graph_decode: null edge argument");
    if (n_scenes > 1 && !batch_ids) return fail(VLSAT_EINVAL, "graph_decode: batch_ids is required for more than one scene");
    const GraphDecodeWs ws = graph_decode_carve(scratch, n_edges, n_rel_class, n_scenes);
    return launch_graph_decode(obj_probs, rel_probs, edges, batch_ids, nullptr, thresholds, n_nodes, n_edges, n_obj_class, n_rel_class,
                               n_scenes, multi_label, score_mode, n_labels, max_rel, ws, labels, label_probs, rels, scores, n_valid,
                               n_total, static_cast<hipStream_t>(stream));
}

int vlsat_graph_decode_counts(const float* obj_probs, const float* rel_probs, const int64_t* gt_class, const int64_t* gt_rel,
                              const float* thresholds, int32_t n_nodes, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class,
                              int32_t multi_label, uint64_t* counts, void* stream) {
    if (!counts || n_nodes < 0 || n_edges < 0) return fail(VLSAT_EINVAL, "graph_decode_counts: bad argument");
    if (n_nodes > 0 && (!obj_probs || !gt_class)) return fail(VLSAT_EINVAL, "graph_decode_counts: null node argument");
    if (n_edges > 0 && (!rel_probs || !gt_rel || !thresholds)) return fail(VLSAT_EINVAL, "graph_decode_counts: null edge argument");
    return launch_graph_decode_counts(obj_probs, rel_probs, gt_class, gt_rel, thresholds, n_nodes, n_edges, n_obj_class, n_rel_class,
                                      multi_label, reinterpret_cast<unsigned long long*>(counts), static_cast<hipStream_t>(stream));
}

// From points to the decoded graph in one call: forward (3D-only when obj_2d_feats is NULL) + softmax of the object heads + the
// decode per branch, enqueued back to back on `stream`.  Every intermediate lives in the plan's memory: logits, probabilities and
// predicate scores in the float half of the evaluation scratch, the decode's workspace -- scene offsets, per-edge counts, keys and
// predicates: 2 N + E (1 + R + R / 4) words -- in its integer half (2 N + E (4 R + 2) words): the arena does not grow.  With
// MODEL.multi_rel_outputs = false the log-probabilities are exponentiated in place first.
int vlsat_forward_graph(vlsat_handle h, vlsat_plan p, const float* obj_points, const float* obj_2d_feats, const float* descriptor,
                        const int64_t* edges_e2, int32_t n_scenes, int32_t multi_label, int32_t score_mode, int32_t n_labels,
                        int32_t max_rel, const float* thresholds, int32_t* labels_3d, float* label_probs_3d, int32_t* rels_3d,
                        float* scores_3d, int32_t* n_valid_3d, int32_t* n_total_3d, int32_t* labels_2d, float* label_probs_2d,
                        int32_t* rels_2d, float* scores_2d, int32_t* n_valid_2d, int32_t* n_total_2d, void* stream) {
    if (!h || !p) return fail(VLSAT_EINVAL, "vlsat_forward_graph: null argument");
    if (p->h != h) return fail(VLSAT_EINVAL, "plan belongs to a different handle");
    const int N = (int)p->N, E = (int)p->E, C = h->d.n_obj_class, R = h->d.n_rel_class;
    RUN(graph_decode_check_args(C, R, multi_label, score_mode, n_labels, max_rel));
    if (n_scenes != p->S) return fail(VLSAT_EINVAL, "vlsat_forward_graph: n_scenes is not the plan's scene count");
    if (!labels_3d || !label_probs_3d || !rels_3d || !scores_3d || !n_valid_3d || !n_total_3d)
        return fail(VLSAT_EINVAL, "vlsat_forward_graph: null 3D output");
    const bool any2 = labels_2d || label_probs_2d || rels_2d || scores_2d || n_valid_2d || n_total_2d;
    const bool all2 = labels_2d && label_probs_2d && rels_2d && scores_2d && n_valid_2d && n_total_2d;
    const bool do2d = obj_2d_feats != nullptr;
    if (do2d ? !all2 : any2)
        return fail(VLSAT_EINVAL, "vlsat_forward_graph: obj_2d_feats and the six 2D outputs go together (all, or none for 3D-only)");
    if (!thresholds || (E > 0 && !edges_e2)) return fail(VLSAT_EINVAL, "vlsat_forward_graph: null thresholds or edge argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t Es = eval_scratch_edge_rows(E);
    const EvalScratch v = eval_scratch_carve(p->ev_f, p->ev_i, N, E, C, R);
    RUN(vlsat_forward(h, p, obj_points, obj_2d_feats, descriptor, v.obj3, do2d ? v.obj2 : nullptr, v.rel3, do2d ? v.rel2 : nullptr, stream));
    GraphDecodeWs ws;                                           // in the rank scratch:
    ws.ptr = v.or3;                                             // its node part (S + 1 <= 2 max(N, 1) entries)
    ws.cnt = v.rr3;                                             // its edge part: E counts, E x R keys, E x R predicates
    ws.keys = reinterpret_cast<uint32_t*>(ws.cnt + Es);
    ws.preds = reinterpret_cast<uint8_t*>(ws.keys + Es * R);
    for (int br = 0; br < (do2d ? 2 : 1); ++br) {
        float* pr = br ? v.prob2 : v.prob3;
        float* rl = br ? v.rel2 : v.rel3;
        RUN(launch_softmax_rows(br ? v.obj2 : v.obj3, C, N, C, pr, 0, s));
        if (!h->d.multi_rel_outputs) RUN(launch_exp(rl, rl, (size_t)E * R, s));
        RUN(launch_graph_decode(pr, rl, edges_e2, nullptr, p->d_scene_ptr, thresholds, N, E, C, R, n_scenes, multi_label, score_mode,
                                n_labels, max_rel, ws, br ? labels_2d : labels_3d, br ? label_probs_2d : label_probs_3d,
                                br ? rels_2d : rels_3d, br ? scores_2d : scores_3d, br ? n_valid_2d : n_valid_3d,
                                br ? n_total_2d : n_total_3d, s));
    }
    VLSAT_HIP_CHECK(hipEventRecord(p->last_use, s));       // (the scratch is the plan's: its next owner orders behind the decode)
    return 0;
}

// -------------------------------------------------------------------------------------------
// Kernel-level entry points of the non-GEMM kernels of the GCN block and the node attention (SURVEY 8b's per-kernel list):
// test entry points like vlsat_k_flash_attn -- small index tables are built on the host, uploaded, and the call
// synchronises before it frees them.
namespace {
// node offsets of the scenes (int64 host, like batch_ids run lengths) -> int32 scene_ptr, int64 bias_ptr, largest scene
static int scene_tables(const int64_t* node_ptr, int n_scenes, int n_heads, std::vector<int32_t>& sp, std::vector<int64_t>& bp, int* max_n) {
    if (!node_ptr || n_scenes <= 0) return fail(VLSAT_EINVAL, "bad scene table");
    sp.resize(n_scenes + 1);
    bp.resize(n_scenes);
    int64_t off = 0;
    *max_n = 0;
    for (int s = 0; s <= n_scenes; ++s) {
        if (node_ptr[s] < 0 || node_ptr[s] > INT32_MAX || (s && node_ptr[s] < node_ptr[s - 1])) return fail(VLSAT_EINVAL, "scene table must be ascending int32 offsets");
        sp[s] = (int32_t)node_ptr[s];
        if (s < n_scenes) {
            const int64_t n = node_ptr[s + 1] - node_ptr[s];
            bp[s] = off;
            off += (int64_t)n_heads * n * n;
            if (n > *max_n) *max_n = (int)n;
        }
    }
    return 0;
}
}  // namespace

int vlsat_k_edge_gate(const float* kproj, const float* node, int32_t ld_node, int32_t gq_off, int32_t v_off, const int32_t* src,
                      const int32_t* dst, const float* w0k, const float* w3, const float* b3, float* gated, float* prob,
                      int32_t n_edges, int32_t n_heads, int32_t dk, int32_t dox, int32_t use_edge, int32_t variant, void* stream) {
    if (!node || !src || !dst || !w3 || !b3 || !gated || (use_edge && (!kproj || !w0k))) return fail(VLSAT_EINVAL, "edge_gate: null argument");
    if (n_edges < 0 || n_heads <= 0 || dk <= 0 || dox <= 0) return fail(VLSAT_EINVAL, "edge_gate: bad geometry");
    hipStream_t s = static_cast<hipStream_t>(stream);
    GateArgs g{};
    g.kproj = kproj; g.node = node; g.ld_node = ld_node; g.gq_off = gq_off; g.v_off = v_off; g.src = src; g.dst = dst;
    g.w0k = w0k; g.w3 = w3; g.b3 = b3; g.gated = gated; g.prob = prob; g.n_edges = n_edges; g.use_edge = use_edge != 0;
    if (variant < 0 || variant > 5) return fail(VLSAT_EINVAL, "edge_gate: variant 0..5");
    // 0: the exact fp32 kernel of this geometry; 1: the VALU kernel; 2: the fp32 template; 3 | 4: the split-bf16 | single-rounded
    // bf16 kernel of this geometry; 5: the split-fp16 kernel of the fp32 mode (shipped geometry only)
    if (variant == 5) {
        if (n_heads != 8 || dk != 64 || dox != 32) return fail(VLSAT_EINVAL, "edge_gate: the split-fp16 kernel is built for 8 heads x (64, 32) only");
        g.f16s = 1;
    }
    const int terms = variant == 3 ? 3 : variant == 4 ? 1 : 0;
    const GateChoice gc = variant == 1 ? gate_choice(GATE_VALU) : gate_select(n_heads, dk, dox, terms, true, variant == 2 ? 2 : 1, true);
    if (variant == 2 && gc.kernel != GATE_F32_HEADS) return fail(VLSAT_EINVAL, "edge_gate: head geometry not built on the MFMA template");
    if (terms && !gc.bits16()) return fail(VLSAT_EINVAL, "edge_gate: head geometry / terms not built on the bf16 template");
    return launch_gate(gc.kernel, g, n_heads, dk, dox, terms, 0, s);
}

int vlsat_k_aggregate(const float* gated, int32_t n_ch, const int64_t* index_host, int64_t n_edges, int32_t n_nodes, int32_t aggr,
                      float* out, int32_t ldo, int32_t col0, void* stream) {
    if (!out || n_nodes < 0 || n_edges < 0 || n_ch <= 0 || (n_edges > 0 && (!gated || !index_host))) return fail(VLSAT_EINVAL, "aggregate: bad argument");
    if (aggr < 0 || aggr > 2) return fail(VLSAT_EINVAL, "aggregate: aggr 0 max | 1 add | 2 mean");
    if (n_edges > INT32_MAX) return fail(VLSAT_EINVAL, "aggregate: too many rows");
    std::vector<int32_t> rowptr(n_nodes + 1, 0), order((size_t)n_edges);
    for (int64_t e = 0; e < n_edges; ++e) {
        if (index_host[e] < 0 || index_host[e] >= n_nodes) return fail(VLSAT_EINVAL, "aggregate: index out of range");
        ++rowptr[index_host[e] + 1];
    }
    for (int n = 0; n < n_nodes; ++n) rowptr[n + 1] += rowptr[n];
    std::vector<int32_t> fill(rowptr.begin(), rowptr.end() - 1);
    for (int64_t e = 0; e < n_edges; ++e) order[fill[index_host[e]]++] = (int32_t)e;      // stable: rows of a segment in input order
    DevTable dr, dord;
    RUN(dr.put(rowptr.data(), rowptr.size() * sizeof(int32_t)));
    RUN(dord.put(order.data(), order.size() * sizeof(int32_t)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int r = launch_aggregate(gated, n_ch, static_cast<const int32_t*>(dr.d), static_cast<const int32_t*>(dord.d), n_nodes, aggr, out, ldo, col0, s);
    hipStreamSynchronize(s);
    return r;
}

int vlsat_k_node_attn(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, float* O, int32_t ldo,
                      const float* bias, const int64_t* node_ptr_host, int32_t n_scenes, int32_t n_heads, float scale,
                      int32_t lanes_per_query, void* stream) {
    if (!Q || !K || !V || !O) return fail(VLSAT_EINVAL, "node_attn: null argument");
    if (n_heads <= 0 || 512 % n_heads) return fail(VLSAT_EINVAL, "node_attn: n_heads must divide 512");
    if (lanes_per_query != 0 && lanes_per_query != 1 && lanes_per_query != 16) return fail(VLSAT_EINVAL, "node_attn: lanes_per_query 0 (auto) | 1 | 16");
    std::vector<int32_t> sp;
    std::vector<int64_t> bp;
    int max_n = 0;
    RUN(scene_tables(node_ptr_host, n_scenes, n_heads, sp, bp, &max_n));
    DevTable dsp, dbp;
    RUN(dsp.put(sp.data(), sp.size() * sizeof(int32_t)));
    RUN(dbp.put(bp.data(), bp.size() * sizeof(int64_t)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int split_below = lanes_per_query == 16 ? INT32_MAX : lanes_per_query == 1 ? 0 : 1024;
    const int r = launch_node_attn(Q, ldq, K, ldk, V, ldv, O, ldo, bias, static_cast<const int32_t*>(dsp.d), static_cast<const int64_t*>(dbp.d),
                                   n_scenes, max_n, n_heads, 512 / n_heads, scale, s, split_below);
    hipStreamSynchronize(s);
    return r;
}

int vlsat_k_dist_bias(const float* desc, int32_t ld_desc, const int64_t* node_ptr_host, int32_t n_scenes, int32_t n_heads,
                      const float* w0, const float* b0, const float* ln2_w, const float* ln2_b, const float* w3, const float* b3,
                      const float* ln5_w, const float* ln5_b, const float* w6, const float* b6, float* bias, void* stream) {
    if (!desc || !w0 || !b0 || !ln2_w || !ln2_b || !w3 || !b3 || !ln5_w || !ln5_b || !w6 || !b6 || !bias) return fail(VLSAT_EINVAL, "dist_bias: null argument");
    if (n_heads <= 0 || ld_desc < 3) return fail(VLSAT_EINVAL, "dist_bias: bad geometry");
    std::vector<int32_t> sp;
    std::vector<int64_t> bp;
    int max_n = 0;
    RUN(scene_tables(node_ptr_host, n_scenes, n_heads, sp, bp, &max_n));
    DevTable dsp, dbp;
    RUN(dsp.put(sp.data(), sp.size() * sizeof(int32_t)));
    RUN(dbp.put(bp.data(), bp.size() * sizeof(int64_t)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DistBiasW w{w0, b0, ln2_w, ln2_b, w3, b3, ln5_w, ln5_b, w6, b6};
    const int r = launch_dist_bias(desc, ld_desc, static_cast<const int32_t*>(dsp.d), static_cast<const int64_t*>(dbp.d), n_scenes, max_n, n_heads, w, bias, s);
    hipStreamSynchronize(s);
    return r;
}

int vlsat_k_layernorm(float* x, int32_t ld, int32_t rows, int32_t dim, const float* gamma, const float* beta,
                      int32_t relu, void* stream) {
    return launch_layernorm(x, ld, rows, dim, gamma, beta, relu, static_cast<hipStream_t>(stream));
}

// -------------------------------------------------------------------------------------------
// Test entry points of the kernels that otherwise run only inside a forward: every PointNet kernel and operand form, every
// form of the LayerNorm kernel, and the glue kernels of small_ops.hip / stn.hip.  Each calls the launcher the forward calls.
int vlsat_k_pointnet_ex(const float* pts, int32_t n_obj, int32_t n_points, int32_t cin, const float* w1, const float* b1,
                        const float* w2, const float* b2, const float* w3, const float* b3, int32_t n_out, int32_t terms,
                        float* out, void* stream) {
    if (!pts || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out) return fail(VLSAT_EINVAL, "pointnet_ex: null argument");
    if ((terms < 0 || terms > 3) && terms != 5) return fail(VLSAT_EINVAL, "pointnet_ex: terms 0 (fp32) | 1 (bf16) | 2 (fp16) | 3 (split-bf16) | 5 (split-fp16)");
    if (n_out <= 0) return fail(VLSAT_EINVAL, "pointnet_ex: n_out must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (terms == 0) return launch_pointnet(pts, n_obj, n_points, cin, w1, b1, w2, b2, w3, b3, n_out, out, st);
    const size_t n2 = 128 * 64, n3 = (size_t)n_out * 128;
    DevTable planes;                            // [w2 hi | w2 lo | w3 hi | w3 lo], freed when the call returns
    RUN(planes.alloc(2 * (n2 + n3) * sizeof(uint16_t)));
    uint16_t* w2h = static_cast<uint16_t*>(planes.d);
    uint16_t *w2l = w2h + n2, *w3h = w2l + n2, *w3l = w3h + n3;
    int r;
    int32_t k2 = 0, k3 = 0;
    if (terms == 5) {                           // the fp32 mode's planes (gemm_f16s_planes.h) and their exponents
        r = vlsat_k_split_f16s(w2, n2, w2h, w2l, &k2, stream);
        if (!r) r = vlsat_k_split_f16s(w3, n3, w3h, w3l, &k3, stream);
    } else if (terms == 2) {
        r = launch_to_f16(w2, n2, w2h, st);
        if (!r) r = launch_to_f16(w3, n3, w3h, st);
    } else {
        r = launch_split_bf16(w2, n2, w2h, w2l, st);
        if (!r) r = launch_split_bf16(w3, n3, w3h, w3l, st);
    }
    if (!r) r = launch_pointnet_bf16(pts, n_obj, n_points, cin, w1, b1, w2h, w2l, b2, w3h, w3l, b3, n_out, terms, out, st, k2, k3);
    hipStreamSynchronize(st);     // test entry point only: the planes are freed right away
    return r;
}

int vlsat_k_layernorm_to(const float* x, int32_t ld, float* y, int32_t ldy, int32_t rows, int32_t dim, const float* gamma,
                         const float* beta, int32_t relu, int32_t out_fmt, const float* resid, int32_t ldr, int32_t resid_fmt,
                         int32_t x_f16, void* stream) {
    if (!x || !y || !gamma || !beta) return fail(VLSAT_EINVAL, "layernorm_to: null argument");
    return launch_layernorm_to(x, ld, y, ldy, rows, dim, gamma, beta, relu, out_fmt, static_cast<hipStream_t>(stream), resid, ldr, resid_fmt, x_f16);
}

int vlsat_k_edge_embed(const float* desc, const int32_t* src, const int32_t* dst, int32_t n_edges, const float* w1cat,
                       const float* b1cat, float* h1, void* stream) {
    return launch_edge_embed(desc, src, dst, n_edges, w1cat, b1cat, h1, static_cast<hipStream_t>(stream));
}

int vlsat_k_desc_tail(const float* desc, int32_t n_nodes, float* x, int32_t ldx, int32_t col0, void* stream) {
    return launch_desc_tail(desc, n_nodes, x, ldx, col0, static_cast<hipStream_t>(stream));
}

int vlsat_k_row_invnorm(const float* x, int32_t ld, int32_t rows, int32_t dim, float scale, float* out, const float* x2,
                        float* out2, void* stream) {
    return launch_row_invnorm(x, ld, rows, dim, scale, out, static_cast<hipStream_t>(stream), x2, out2);
}

int vlsat_k_copy_rows(float* dst, int64_t dst_ld, const float* src, int64_t src_ld, int32_t cols, int64_t rows, void* stream) {
    if (dst_ld < 0 || src_ld < 0 || rows < 0) return fail(VLSAT_EINVAL, "copy_rows: negative pitch or row count");
    return launch_copy_rows(dst, (size_t)dst_ld, src, (size_t)src_ld, cols, (size_t)rows, static_cast<hipStream_t>(stream));
}

int vlsat_k_pts_conv1_rows(const float* pts, int32_t n_obj, int32_t n_points, int32_t cin, const float* w1, const float* b1,
                           float* rows, void* stream) {
    return launch_pts_conv1_rows(pts, n_obj, n_points, cin, w1, b1, rows, static_cast<hipStream_t>(stream));
}

int vlsat_k_rowmax(const float* x, int32_t ld, int32_t n_obj, int32_t n_points, int32_t cols, float* out, int32_t ldo, void* stream) {
    return launch_rowmax(x, ld, n_obj, n_points, cols, out, ldo, static_cast<hipStream_t>(stream));
}

int vlsat_k_apply_stn(const float* h, int32_t ldh, const float* T, int64_t rows, int32_t n_points, float* out, int32_t ldo, void* stream) {
    if (rows < 0) return fail(VLSAT_EINVAL, "apply_stn: negative row count");
    return launch_apply_stn(h, ldh, T, (size_t)rows, n_points, out, ldo, static_cast<hipStream_t>(stream));
}

}  // extern "C"
