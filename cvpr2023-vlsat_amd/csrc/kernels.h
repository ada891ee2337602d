// Host-side launchers of the hand-written gfx950 kernels (internal C++ interface between the
// engine and the .hip files; the public surface is include/vlsat.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flash_pick.h"
#include "gemm_plan.h"

namespace vlsat {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }     // a: a power of two (scratch carving)

// ---- GEMM: GemmArgs, GemmPlan, the lists of the kernels that exist and the planner are gemm_plan.h (no HIP header) ----
int launch_gemm(const GemmArgs& a, hipStream_t s);
// two problems of the same shape and flags in ONE launch (round 6: the 3D / 2D twins of a one-scene forward): 0 = launched,
// 1 = not pairable (gemm_pair_plan).  The caller then launches them one after the other; results are bit-identical either way
int launch_gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t s);
// the launch of a plan of that family on rows [0, a.M): table[p.variant]; twin: a second problem whose own plan is p, in the same launch
int launch_gemm_splitk(const GemmArgs& a, const GemmPlan& p, hipStream_t s, const GemmArgs* twin = nullptr);
int launch_gemm_ring(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
int launch_gemm_p8(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
double gemm_flops(const GemmArgs& a);
void gemm_set_clock_probe(long long* buf);
int gemm_slots();                                // resident 256-thread blocks the persistent grid may use (2 per CU): what plan_gemm plans with

// ---- PointNet object encoder (fused conv1..conv3 + ReLU + max over points) ----
int launch_pointnet(const float* pts, int n_obj, int n_points, int cin, const float* w1, const float* b1,
                    const float* w2, const float* b2, const float* w3, const float* b3, int n_out,
                    float* out, hipStream_t s);

// the same on the bf16 matrix cores (pointnet_bf16.hip): conv2 / conv3 weights as bf16 hi / lo planes ([128,64], [n_out,128]);
// terms = 3 split-bf16 | 1 single-rounded (the lo planes are then not read) | 2 single-rounded fp16 | 5 split-fp16 (the fp32 mode: the
// planes are the fp16 ones of gemm_f16s_planes.h, k2 / k3 their tensors' exponents; fp32-grade results)
int launch_pointnet_bf16(const float* pts, int n_obj, int n_points, int cin, const float* w1, const float* b1,
                         const uint16_t* w2h, const uint16_t* w2l, const float* b2, const uint16_t* w3h, const uint16_t* w3l,
                         const float* b3, int n_out, int terms, float* out, hipStream_t s, int k2 = 0, int k3 = 0);

// ---- edge cross-attention (flash style, fp32 MFMA) ----
// tiles: device array of int4 {row_base, n_tokens, q0, head}; one block per entry.
// Split-key mode (plans with too few blocks to fill the chip): tile i covers key tiles [krange[i].x, krange[i].y)
// as part krange[i].z of `parts`; partial results go to o_part [parts][rows][ldo] (un-normalised), m_part / l_part
// [parts][rows][heads]; a merge kernel writes O.  A tile with an empty key range records m = -inf, l = 0.
struct FlashSplit {
    int parts = 1;
    const int4* krange = nullptr;
    float* o_part = nullptr; float* m_part = nullptr; float* l_part = nullptr;
    size_t part_stride = 0;      // floats between parts of o_part (= rows * ldo)
    int rows = 0, heads = 0;
    int ablate = 0;              // timing experiments (garbage results): bit 0 no K/V loads after the first tile, bit 1 no LDS stores of them either
    int qg = 0;                  // half rows, head dim 64, LDS-direct kernel, no key split: 1 | 2 = 64 queries per wave (flash_attn_bf16.hip QG = 2; 2 = ORD 1), 0 = 32
    int bq = 128;                // queries per block of the tile table handed in: FLASH_BQ, or FLASH_BQ_BIG (half rows, head dim 64, LDS-direct kernel only)
};
int launch_flash_attn(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo,
                      const int4* tiles, int n_tiles, float scale_log2e, hipStream_t s, const FlashSplit* split = nullptr,
                      int head_dim = 64);      // head_dim = 512 / NUM_HEADS: 32 | 64 | 128, one instantiation each
int launch_flash_merge(float* O, int ldo, const FlashSplit& sp, hipStream_t s, int out_split, int head_dim = 64);
// the same attention on the bf16 matrix cores (flash_attn_bf16.hip): terms = 3 split-bf16 (~1e-5) | 1 single-rounded;
// use_tr = 0 selects the gather fallback for the V operand instead of ds_read_b64_tr_b16 (tests); io_split = 1: Q (already
// scaled), K, V and O are in the split-pair format of the bf16 modes (common.h pack_split), 2 | 3: bf16 | fp16 half rows.
// Which kernel a call gets, which calls are an error and flash_attn_bf16_supports (the (head dim, format) combinations that
// are built) are all flash_bf16_pick of flash_pick.h, next to the list of the kernels that exist.
int launch_flash_attn_bf16(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo,
                           const int4* tiles, int n_tiles, float scale_log2e, int terms, int use_tr, int io_split,
                           hipStream_t s, const FlashSplit* split = nullptr, int pv_terms = 3, int head_dim = 64);
// the split-fp16 form of the three-term kernel (flash_attn_bf16.hip; the edge attention of the fp32 precision mode): plain fp32 Q, K,
// V, O, every operand as fp16 hi + fp16 lo (2^-22), three f16 MFMAs per product, fp32 accumulate and softmax.  Domain: |Q * scale_log2e|,
// |K| < 65504, |V| < 65504 / 2^3 (V is pre-scaled by 2^3; clamped there).  use_tr 0 | 1 as above; split keys as above.  Its kernels and
// what a call gets: flash_f16x3_pick of flash_pick.h; what is not in that list is an error.
int launch_flash_attn_f16x3(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo,
                            const int4* tiles, int n_tiles, float scale_log2e, int use_tr, hipStream_t s,
                            const FlashSplit* split = nullptr, int head_dim = 64, int io = 0);      // io 4 | 5: pair words (flash_f16x3_pair_pick)

// ---- node attention with distance bias (per scene, per head) ----
// scene_ptr: device [n_scenes+1] node offsets; bias_ptr: device [n_scenes] offsets into bias
// (layout per scene: [H][n][n], query-major).  grid covers max_n queries per scene.
// head dim dk = 512 / n_heads in {32, 64, 128}; bias may be NULL.  Also the generic (VALU) edge cross-attention for
// dk != 64 (scene_ptr = the scenes' edge ranges).
int launch_node_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                     float* O, int ldo, const float* bias, const int32_t* scene_ptr,
                     const int64_t* bias_ptr, int n_scenes, int max_n, int n_heads, int dk, float scale,
                     hipStream_t s, int split_below = 1024);
// distance-bias MLP (MMG.self_attn_fc): centres = desc[:,0:3] (ld = 11)
struct DistBiasW { const float *w0, *b0, *g2, *be2, *w3, *b3, *g5, *be5, *w6, *b6; };
int launch_dist_bias(const float* desc, int ld_desc, const int32_t* scene_ptr, const int64_t* bias_ptr,
                     int n_scenes, int max_n, int n_heads, DistBiasW w, float* bias, hipStream_t s);

// ---- small fused VALU kernels ----
// edge descriptor (Gen_edge_descriptor) + conv1 of both relation encoders:
// h1[e, 0:64] = relu(W1_3d ed + b), h1[e, 64:128] = relu(W1_2d ed + b)
int launch_edge_embed(const float* desc, const int32_t* src, const int32_t* dst, int n_edges,
                      const float* w1cat /*[128,11]*/, const float* b1cat /*[128]*/, float* h1, hipStream_t s);
// x3[n, 504:512] = [desc[3:9], log desc[9], log desc[10]]
int launch_desc_tail(const float* desc, int n_nodes, float* x, int ldx, int col0, hipStream_t s);
// in-place LayerNorm over rows of `dim` (dim == 512), optional ReLU
int launch_layernorm(float* x, int ld, int rows, int dim, const float* gamma, const float* beta, int relu,
                     hipStream_t s);
// out of place; out_split = 1 writes the split-pair format of the bf16 modes (common.h pack_split), 2 / 4 bf16 / fp16 half rows, 0 fp32,
// 6 the GEMM pair words of the fp32 mode (gemm_f16s_planes.h f16s_pair_pack, packed by f16s_pack2 like a GEMM epilogue); any other value is refused, as is an x_f16 outside {0, 1}
int launch_layernorm_to(const float* x, int ld, float* y, int ldy, int rows, int dim, const float* gamma, const float* beta,
                        int relu, int out_split, hipStream_t s, const float* resid = nullptr, int ldr = 0, int r_split = 0, int x_f16 = 0);
// (x_f16: the rows of x are fp16 half rows -- what the out-projection of the single-rounded edge attention writes, GemmArgs::c_f16_cols == N)
// rowscale[m] = scale / ||x[m,:]||_2  (dim == 512)
int launch_row_invnorm(const float* x, int ld, int rows, int dim, float scale, float* out, hipStream_t s, const float* x2 = nullptr, float* out2 = nullptr);

// ---- MODEL.feature_transform glue (stn.hip): conv1 as point rows, max over an object's rows, per-object 64x64 ----
int launch_pts_conv1_rows(const float* pts, int n_obj, int P, int cin, const float* w1, const float* b1, float* rows,
                          hipStream_t s);
int launch_rowmax(const float* x, int ld, int n_obj, int P, int cols, float* out, int ldo, hipStream_t s);
int launch_apply_stn(const float* h, int ldh, const float* T, size_t rows, int P, float* out, int ldo, hipStream_t s);

// ---- 'fat' edge gate: per (edge, head) MLP 2 d_k -> 2 d_k -> d_o, softmax over d_o, times value (gate_core.h) ----
// H heads, d_k = 512 / H query / edge channels and d_o = DIM_ATTEN / H output channels per head (shipped: 8 x (64, 32))
struct GateArgs {
    const float* kproj;      // [E, 512] head-major: kproj[e, h*d_k + c]; fp32, or the 16-bit kernels' `kproj_split` formats
    const float* node;       // node-side buffer, row pitch ld_node
    int ld_node;
    int gq_off;              // column offset of Gq[h*2 d_k + o] (layer-1 node part incl. bias)
    int v_off;               // column offset of value[h*d_o + m]  (head-major, see gate_core.h)
    const int32_t* src;      // [E]
    const int32_t* dst;      // [E]
    const float* w0k;        // [2 d_k, d_k]  layer-1 weights acting on the edge half
    const float* w3;         // [d_o, 2 d_k]
    const float* b3;         // [d_o]
    float* gated;            // [E, H d_o]  gated[e, h*d_o + m]
    float* prob;             // optional [E, d_o, H] tap (tests) or nullptr
    int n_edges;
    int use_edge = 1;        // MODEL.USE_GCN_EDGE: 0 -> the gate MLP sees the query alone (kproj / w0k unused)
    int grid_cap = 0;        // debug: persistent grid size (0 = the kernel's own; vlsat_debug_option "gate_grid")
    // Fused max aggregation (Aggre_Index with GCN_AGGR = max, reference network_util.py:64-73): when `agg` is set the gated rows
    // are not stored; every wave reduces its 32 rows by source node through LDS and folds the partial maxima into
    // agg[src, h*d_o + m] (row pitch ld_agg) with integer-ordered atomic max -- exact and order-independent.  `agg` must have been
    // initialised by launch_agg_init (-inf for nodes with out-edges, 0 for the others: torch_scatter's empty segment).
    float* agg = nullptr;
    int ld_agg = 0;
    int row_map = 1;         // rows of a wave: 1 = 32 edges of one head, 0 = 4 edges x 8 heads (vlsat_debug_option "gate_row_map")
    int f16s = 0;            // GATE_F32 only (fp32 mode): 1 = every product as three fp16 MFMAs, fp32 tensors in and out (edge_gate_f16s.hip; as GemmArgs::f16s)
};
// The five gate kernels, and the ONE place that says which of them runs and what it can do besides the plain gate.
enum GateKernel {
    GATE_VALU,          // any geometry, plain VALU (edge_gate.hip)
    GATE_F32,           // fp32 MFMA, the shipped 8 x (64, 32) (edge_gate.hip)
    GATE_F32_HEADS,     // fp32 MFMA, the template of the other head geometries (edge_gate_heads.hip)
    GATE_16,            // bf16 / fp16 MFMA, the shipped geometry (edge_gate_bf16.hip)
    GATE_16_HEADS       // bf16 / fp16 MFMA, the template (edge_gate_bf16_heads.hip)
};
struct GateChoice {
    GateKernel kernel;
    bool fuse_agg;      // implements GateArgs::agg
    bool twin;          // takes a second problem on the same edge list in the same launch (one-scene plans)
    bool row_map0;      // implements GateArgs::row_map = 0
    bool bits16() const { return kernel == GATE_16 || kernel == GATE_16_HEADS; }      // reads the 16-bit kproj formats
};
// only the two kernels of the shipped geometry implement the extras; launch_gate refuses them on the others
inline GateChoice gate_choice(GateKernel k) {
    const bool shipped = k == GATE_F32 || k == GATE_16;
    return {k, shipped, shipped, shipped};
}
// (d_k, d_o) the two head templates are instantiated for: MODEL.NUM_HEADS in {4, 8, 16} x DIM_ATTEN in {128, 256, 512}
#define VLSAT_GATE_HEAD_GEOMETRIES(X) X(32, 8) X(32, 16) X(32, 32) X(64, 16) X(64, 32) X(64, 64) X(128, 32) X(128, 64) X(128, 128)
inline bool gate_heads_built(int n_heads, int dk, int dox) {
#define VLSAT_GH(DK, DOX) || (dk == DK && dox == DOX)
    return n_heads * dk == 512 && (false VLSAT_GATE_HEAD_GEOMETRIES(VLSAT_GH));
#undef VLSAT_GH
}
// terms: 0 = fp32 operands, 3 = split-bf16, 1 = single-rounded bf16 / fp16 (precision of the edge rows); gate_bf16, heads_mfma,
// heads_bf16: the vlsat_debug_option switches "gate_bf16" (0: fp32 kernels in every mode), "gate_heads_mfma" (0: VALU kernel for the
// other head geometries, 2: the templates for the shipped geometry as well -- A/B) and "gate_heads_bf16" (0: fp32 template).
inline GateChoice gate_select(int n_heads, int dk, int dox, int terms, bool gate_bf16, int heads_mfma, bool heads_bf16) {
    const bool shipped = n_heads == 8 && dk == 64 && dox == 32 && heads_mfma != 2;
    const bool want16 = terms != 0 && gate_bf16;
    if (shipped) return gate_choice(want16 ? GATE_16 : GATE_F32);
    if (!heads_mfma || !gate_heads_built(n_heads, dk, dox)) return gate_choice(GATE_VALU);
    // (two plane sets of d_k = 128 do not fit the LDS: split-bf16 stays on the fp32 template there)
    if (want16 && heads_bf16 && !(terms == 3 && dk == 128)) return gate_choice(GATE_16_HEADS);
    if (want16 && n_heads == 8 && dk == 64 && dox == 32) return gate_choice(GATE_16);     // (2 with "gate_heads_bf16" off)
    return gate_choice(GATE_F32_HEADS);
}
// kernel: what gate_select (or a test that names a kernel) chose.  terms (1 | 3) and kproj_split (format of kproj: 0 fp32, 1 split-pair
// words of common.h pack_split, 2 bf16 half rows, 3 fp16 half rows -- 2 and 3 with terms = 1 only) are read by the 16-bit kernels.
// twin: a second gate on the same edge list with the same options in the same launch.  An `agg`, a twin or a row_map = 0 handed to a
// kernel that does not implement it is refused, as is a geometry the kernel is not built for.
int launch_gate(GateKernel kernel, const GateArgs& a, int n_heads, int dk, int dox, int terms, int kproj_split, hipStream_t s,
                const GateArgs* twin = nullptr);
// agg[n, 0:n_ch] = rowptr[n+1] > rowptr[n] ? -inf : 0   (start values of the fused max aggregation)
int launch_agg_init(const int32_t* rowptr, int n_nodes, int n_ch, float* agg, int ld_agg, hipStream_t s, float* agg2 = nullptr);
// p[0:n] = 0 with a kernel of the library (16-byte stores when n and p allow): the forward path does not use hipMemsetAsync
int launch_zero_f32(float* p, size_t n, hipStream_t s);
// dst[r, 0:cols] = src[r, 0:cols], r < rows (pitches in floats; 16-byte accesses when sizes and pointers allow)
int launch_copy_rows(float* dst, size_t dst_ld, const float* src, size_t src_ld, int cols, size_t rows, hipStream_t s);

// ---- scatter aggregation by source node over a CSR (rowptr[N+1], order[E]) ----
// out[n, col0 + c] = reduce_{k in rowptr[n]..rowptr[n+1]} gated[order[k], c]; empty -> 0
int launch_aggregate(const float* gated, int n_ch, const int32_t* rowptr, const int32_t* order,
                     int n_nodes, int aggr, float* out, int ldo, int col0, hipStream_t s, const float* gated2 = nullptr, float* out2 = nullptr);   // gated2 / out2: a twin problem on the same graph in the same launch

// w[i] -> bf16 hi[i] + bf16 lo[i] (split-bf16 GEMM weights, one-time)
int launch_split_bf16(const float* w, size_t n, uint16_t* hi, uint16_t* lo, hipStream_t s);
int launch_to_f16(const float* w, size_t n, uint16_t* out, hipStream_t s);        // fp16 plane (precision mode fp16_mixed)
// w[i] 2^k -> fp16 hi[i] + fp16 lo[i], k = 13 - ceil(log2(max |w|)) (gemm_f16s_planes.h; GemmArgs::f16s): scratch2[0] receives the bits of
// max |w|, scratch2[1] the integer k (device, two words, read back by the caller once the stream has run)
int launch_split_f16s(const float* w, size_t n, uint16_t* hi, uint16_t* lo, unsigned* scratch2, hipStream_t s);

// ---- eval ranking step: softmax + top-k ranks by counting ----
int launch_softmax_rows(const float* x, int ld, int rows, int cols, float* out, int log_out, hipStream_t s);
int launch_eval_ranks(const float* obj_logits, const float* obj_probs, const float* rel, const int64_t* gt_cls,
                      const int64_t* gt_rel, const int64_t* edges, int N, int E, int C, int R, int topk_obj,
                      int topk_rel, int topk_tri, float thr, int32_t* obj_rank, int32_t* rel_rank, int32_t* tri_rank,
                      int32_t* cnt, float* sorted_probs, hipStream_t s, bool rel_is_log);
// rel_is_log: `rel` holds log-probabilities (single-label model): rel_rank ranks them as they are, tri_rank ranks exp(rel), taken per
// lane on load -- the tables of two passes (rel, then exp(rel) by launch_exp) in one.  false: tri_rank needs rel >= 0 (the staircase).
// columns of the per-node sorted-probability scratch of launch_eval_ranks ([N, K] floats): only the topk largest matter
inline int eval_ranks_sorted_k(int C, int topk_tri) { return C < topk_tri ? C : topk_tri; }

// sorted[n, 0:K] = the K largest entries of probs[n, :] (C <= 1024), descending; si: optional [N, K] class indices of the entries
// (equal values in ascending class order)
int launch_sort_probs(const float* probs, int N, int C, int K, float* sorted, hipStream_t s, int32_t* si = nullptr);
// Recall@K / mR@K counts per scene (eval_recall.hip): counts [n_scenes][1 + R + 4 (3 + 3 R)] int64, every field written
size_t eval_recallk_scratch_bytes(int64_t N, int64_t E, int C, int R, int n_scenes);
int launch_eval_recallk(const float* obj_probs, const float* rel, const int64_t* gt_cls, const int64_t* gt_rel, const int64_t* edges,
                        const int64_t* batch_ids, int N, int E, int C, int R, int n_scenes, int vmask, void* scratch,
                        long long* counts, hipStream_t s);

// the predicted scene graph (scene_graph.hip): per scene the top_k candidates with their indices -- triplets [n_scenes][top_k][4]
// (edge, subject class, object class, predicate), scores [n_scenes][top_k], n_valid [n_scenes]; mode 0 triplet | 1 rels.
// The scene of an edge comes from batch_ids, else from node_ptr ([n_scenes + 1] node offsets), else there is one scene.
struct SceneGraphWs { float* sv; int32_t* si; int32_t* ptr; uint32_t* keys; uint32_t* packs; };   // [N, min(C,100)] x 2, [S + 1], [E, L] x 2
size_t scene_graph_scratch_bytes(int64_t N, int64_t E, int C, int R, int n_scenes, int each);
SceneGraphWs scene_graph_carve(void* scratch, int64_t N, int64_t E, int C, int R, int n_scenes, int each);
int scene_graph_check_args(int C, int R, int mode, int top_k, int each);
int launch_scene_graph_topk(const float* obj_probs, const float* rel, const int64_t* edges, const int64_t* batch_ids,
                            const int32_t* node_ptr, int N, int E, int C, int R, int n_scenes, int mode, int top_k, int each,
                            const SceneGraphWs& ws, int32_t* trip, float* score, int32_t* nvalid, hipStream_t s);
// ptr[q] = first edge of scene q, ptr[n_scenes] = E, for edges grouped by scene in ascending order (scene of an edge: see above)
int launch_scene_edge_ptr(const int64_t* edges, const int64_t* batch_ids, const int32_t* node_ptr, int N, int E, int n_scenes, int32_t* ptr,
                          hipStream_t s);
int launch_exp(const float* x, float* out, size_t n, hipStream_t s);      // out = exp(x) (out may be x): log-probabilities of a single-label model

// the decoded scene graph (graph_decode.hip): per node its n_labels best classes (labels / label_probs [N][n_labels]), per scene the
// asserted (edge, predicate) pairs by (score descending, edge, predicate ascending), capped at max_rel: rels [n_scenes][max_rel][2],
// score [n_scenes][max_rel], n_valid / n_total [n_scenes].  multi: threshold every predicate | arg-max (0 = none) then threshold;
// score_mode 0 rel | 1 fl(fl(s * o) * rel) with the nodes' top-1 probabilities.  Scene of an edge: as launch_scene_graph_topk.
struct GraphDecodeWs { int32_t* ptr; int32_t* cnt; uint32_t* keys; uint8_t* preds; };             // [S + 1], [E], [E, R], [E, R]
size_t graph_decode_scratch_bytes(int64_t E, int R, int n_scenes);
GraphDecodeWs graph_decode_carve(void* scratch, int64_t E, int R, int n_scenes);
int graph_decode_check_args(int C, int R, int multi, int score_mode, int n_labels, int max_rel);
int launch_graph_decode(const float* obj_probs, const float* rel, const int64_t* edges, const int64_t* batch_ids, const int32_t* node_ptr,
                        const float* thr, int N, int E, int C, int R, int n_scenes, int multi, int score_mode, int n_labels, int max_rel,
                        const GraphDecodeWs& ws, int32_t* labels, float* label_probs, int32_t* rels, float* score, int32_t* nvalid,
                        int32_t* ntotal, hipStream_t s);
// out[3 R + 2] += per predicate tp, fp, fn of the same decisions (before the cap) against gt, then nodes, nodes with top-1 == gt;
// gt_rel int64 multi-hot [E, R] (multi) | int64 [E], 0 = none; integer atomics only, safe from concurrent streams
int launch_graph_decode_counts(const float* obj_probs, const float* rel, const int64_t* gt_cls, const int64_t* gt_rel, const float* thr,
                               int N, int E, int C, int R, int multi, unsigned long long* out, hipStream_t s);

// rank arrays of one batch -> += the additive counts vector of evaluate.validation (uint64 [1 + R + 2 (11 + 6 R)]; layout:
// evaluate.fields()); integer atomics only, safe from concurrent streams
int launch_eval_counts(const int32_t* obj_rank3, const int32_t* obj_rank2, const int32_t* rel_rank3, const int32_t* rel_rank2,
                       const int32_t* tri_rank3, const int32_t* tri_rank2, const int32_t* cnt, const int64_t* gt_cls,
                       const int64_t* gt_rel, const int64_t* edges, int N, int E, int R, int n_scenes, unsigned long long* out,
                       hipStream_t s);
// zero-shot split of the triplet recall: out[12] += per branch (3D, 2D) all_n, all_hit@{50,100}, zs_n, zs_hit@{50,100} over the
// rows with a predicate; table uint8 [C*C*R] (1 = zero-shot key (s*C + o)*R + p); R <= 32; integer atomics only
int launch_eval_triplet_split(const int32_t* tri_rank3, const int32_t* tri_rank2, const int32_t* cnt, const int64_t* gt_cls,
                              const int64_t* gt_rel, const int64_t* edges, const uint8_t* table, int E, int C, int R,
                              unsigned long long* out, hipStream_t s);

// the additive metrics vector {scenes, N, E, four fp64 output sums, two top-1 agreement counts}; scratch: 256 * 6 doubles
int launch_scene_checksums(const float* obj3d, const float* obj2d, long N, int C, const float* rel3d, const float* rel2d, long E, int R,
                           int n_scenes, double* out9, double* scratch, hipStream_t s);

// ---- per-object input preparation ----
int launch_prepare_objects(const float* scene, const int32_t* choice, int N, int P, float* obj_points, float* desc,
                           hipStream_t s);
// *mismatches += rows of a DEVICE edge list [2,E] (int64) that differ from a plan's own (src, dst) tables, + nodes whose batch id
// run structure differs from the plan's scene partition (batch_ids may be null)
int launch_check_graph(const int64_t* edges, int64_t n_edges, const int32_t* src, const int32_t* dst, const int64_t* batch_ids,
                       int64_t n_nodes, const int32_t* scene_ptr, int n_scenes, int32_t* mismatches, hipStream_t s);
// per-object point selection (reference dataset_3dssg.py:279-289): stable per-instance index lists + n_sample draws with
// replacement from a counter-based generator (prep.hip); scratch: sample_objects_scratch_ints(n_points, n_obj) int32
size_t sample_objects_scratch_ints(int64_t n_points, int n_obj);
int launch_sample_objects(const int32_t* instances, int64_t n_points, const int32_t* ids, int n_obj, int n_sample, unsigned long long seed,
                          int32_t* id_map, int map_size, int32_t* scratch, int32_t* choice, int32_t* counts, hipStream_t s);
int launch_fc_edges(const int32_t* node_ptr, const int64_t* edge_ptr, int n_scenes, int64_t n_nodes, int64_t n_edges,
                    int64_t* edges, int64_t* batch_ids, hipStream_t s);
// id -> slot map (prep.hip): id_map[0:map_size] = -1; id_map[ids[i]] = i for the ids in range (one thread per entry; unchecked launches:
// the caller's launch check covers them)
void launch_id_map_clear(int32_t* id_map, int map_size, hipStream_t s);
void launch_id_map_set(const int32_t* ids, int n, int32_t* id_map, int map_size, hipStream_t s);

// ---- proximity-pruned edge lists (proximity.hip; the rule is stated in include/vlsat.h) ----
int proximity_lds_boxes();
int launch_instance_boxes(const int32_t* instances, const float* scene_points, int64_t n_points, const int32_t* ids, int n_obj,
                          int32_t* id_map, int map_size, float* boxes, hipStream_t s);
// scratch: thr u64 [N] | row_off i64 [N+1] | row_count i32 [N]; count fills it, fill reads it
size_t proximity_scratch_bytes(int64_t n_nodes);
int launch_proximity_count(const float* boxes, const int32_t* node_ptr, int n_scenes, int64_t n_nodes, float padding, int max_neighbors,
                           void* scratch, int64_t* edge_ptr, int64_t* batch_ids, hipStream_t s);
int launch_proximity_fill(const float* boxes, const int32_t* node_ptr, int n_scenes, int64_t n_nodes, float padding, int max_neighbors,
                          const void* scratch, int64_t n_edges, int64_t capacity, int64_t* edges, hipStream_t s);

// ---- annotation transfer onto a predicted segmentation (label_transfer.hip; the rule is stated in include/vlsat.h) ----
size_t nearest_points_scratch_bytes(int64_t n_query, int64_t n_ref);
// the grid nearest_points searches, for other searches over the same cells (cloud.hip): nn_grid.h describes what comes back
struct NnGridView;
size_t nn_grid_scratch_bytes(int64_t n_ref);
NnGridView launch_nn_grid(const float* ref, int64_t n_ref, float max_sq_dist, void* scratch, hipStream_t s);
int launch_nearest_points(const float* query, int64_t n_query, const float* ref, int64_t n_ref, float max_sq_dist, void* scratch,
                          int32_t* nn_index, float* nn_sqdist, hipStream_t s);
// id_maps: int32 [seg_map_size + gt_map_size] scratch (segment id -> slot, then instance id -> slot)
size_t segment_overlap_scratch_bytes(int32_t seg_map_size, int32_t gt_map_size);
int launch_segment_overlap(const int32_t* pd_segments, const int32_t* nn_index, int64_t n_query, const int32_t* gt_instances, int64_t n_ref,
                           const int32_t* segment_ids, int n_seg, const int32_t* gt_ids, int n_gt, int32_t* id_maps, int seg_map_size,
                           int gt_map_size, int min_seg_size, double corr_thres, double occ_thres, int occ_min_candidates, int32_t* size,
                           int32_t* counts, int32_t* match, int32_t* best, int32_t* second, int32_t* n_candidates, hipStream_t s);

// ---- segments merged into objects along "same part" edges (segment_merge.hip; the rule is stated in include/vlsat.h) ----
int merge_segments_check_args(int64_t N, int64_t E, int C, int R, int n_scenes);
size_t merge_segments_scratch_bytes(int64_t N, int64_t E, int C, int R, int n_scenes);
int launch_merge_segments(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids, const float* weights,
                          int n_nodes, int n_edges, int C, int R, int n_scenes, int same_part, float threshold, int mutual, void* scratch,
                          int32_t* root, int32_t* object, int32_t* n_objects, int32_t* totals, int32_t* member_ptr, int32_t* members,
                          float* out_probs, float* out_weight, int64_t* obj_batch_ids, int32_t* edge_to_pair, int64_t* pair_edges,
                          int32_t* pair_count, float* pair_probs, hipStream_t s);
// the three steps merge_segments shares with fuse_splits (scene_split.hip), defined in segment_merge.hip: a contract-off source.
// Unchecked launches: the caller's launch check covers them.
//   scan     out[0..n] = exclusive scan of in[0..n-1] by one block of 1024; *total = *total2 = out[n] (either may be null); out may be
//            in: a thread reads each element of its own run before writing it
//   members  one wave per object o < totals[0]: the rows n >= obj_root[o] with root[n] == obj_root[o], ascending, into
//            members[member_ptr[o] ..]; bid given: the walk ends with the root's scene
//   pool     one wave per object, members in order: s = fl(s + fl(w p)), W = fl(W + w), out_probs = fl(s / W), out_weight = W
void launch_scan_i32(const int32_t* in, int n, int32_t* out, int32_t* total, int32_t* total2, hipStream_t s);
void launch_members(const int32_t* root, const int32_t* obj_root, const int32_t* member_ptr, const int64_t* bid, const int32_t* totals, int n,
                    int32_t* members, hipStream_t s);
void launch_pool_members(const float* probs, const float* weights, const int32_t* members, const int32_t* member_ptr, const int32_t* totals,
                         int n, int C, float* out_probs, float* out_weight, hipStream_t s);

}  // namespace vlsat
