// Every edge-row nn.Linear of the forward, stated ONCE: one function per launch that returns its GemmArgs complete in shape, pitches, which
// of bias / residual / gathered rows exist, activation, pending ReLU, operand formats and pair words.  engine_forward.hip launches what these
// return (its gemm_resolve adds what needs the handle: weight planes, workspaces, debug switches); edge_pairs_plan (edge_pairs.h) asks the
// planner about the same GemmArgs on placeholder operands; tests/edge_stages_check.cpp prints every field.  No HIP header.
// br: 0 = the 3D branch (chain tensor E3), 1 = the 2D one (E2).  Node-row launches and the STN chain never carry pair words: not here.
#pragma once
#include "gemm_plan.h"

namespace vlsat {

// fp32 mode: which edge-row tensors of the forward being enqueued travel as pair words -- the answer of edge_pairs_plan
struct EdgePairs {
    bool hbig[2] = {false, false}, r1[2] = {false, false}, e3 = false;     // [branch]
    bool kv = false, oe = false;                                            // K | V (attention pair words), Oe (GEMM pair words)
    bool e2 = false;                                                        // E2 as the LayerNorm / conv3 of rel_encoder_2d write it
    const char *why_hbig[2] = {nullptr, nullptr}, *why_r1[2] = {nullptr, nullptr}, *why_e3 = nullptr;      // why not (null: it pairs)
    const char *why_kv = nullptr, *why_oe = nullptr, *why_e2 = nullptr;
    int flash_io() const { return kv ? (oe ? 5 : 4) : 0; }                  // what the attention launch is told (flash_f16x3_pair_pick)
    bool any() const { return hbig[0] || hbig[1] || r1[0] || r1[1] || e3 || kv || oe || e2; }
    // The chain tensor of a branch as conv3 of its relation encoder (on the 2D branch: and the LayerNorm) writes it and as nn_edge.0,
    // proj_edge and the first Linear of the relation head read it
    bool chain(int br) const { return br ? e2 : e3; }
    // ... and as nn_edge.2 writes it.  E2 holds two kinds of content in a layer: nn_edge.2's is also the fp32 residual of the
    // out-projection (a pair word holds about 22 bits), so on the 2D branch it NEVER pairs -- and the query projection, its other
    // reader, reads fp32 and splits it on the fly
    bool nn_edge2_out(int br) const { return br == 0 && e3; }
    bool attn_q_in() const { return false; }
    int attn_kv_out() const { return kv ? 2 : 0; }                          // (GemmArgs::c_pair 2: attention pair words)
};

// E edges, D edge feature width, NPC = 6 D + A the pitch of the node-side projection's rows, R predicate classes; the mode's format codes:
// S of the chain tensors (split_fmt), SA of Q / K|V / O of the edge attention (edge_attn_fmt) -- both 0 in the fp32 mode
struct EdgeDims { int E = 0, D = 512, NPC = 6 * 512 + 256, R = 26, S = 0, SA = 0; };
// the operands of one launch; resid: E2 (out-projection); NP, src, dst: the gathered node rows and their indices (nn_edge.0)
struct EdgeOps {
    const float *A = nullptr, *W = nullptr, *bias = nullptr;
    float* C = nullptr;
    const float *resid = nullptr, *NP = nullptr;
    const int32_t *src = nullptr, *dst = nullptr;
};
// ... and aligned placeholders for them: the planner looks at shapes, flags, which operands exist and their alignment -- never through a pointer
inline EdgeOps edge_ops_placeholder() {
    static float f[4] __attribute__((aligned(16)));
    static int32_t i[1];
    return {f, f, f, f, f, f, i, i};
}

// storage format of an operand: the mode's code (GemmArgs::a_split / c_split) and, fp32 mode, pair words (GemmArgs::a_pair / c_pair)
struct EdgeFmt { int split = 0, pair = 0; };
// A [E, K] . W [N, K]^T (+ bias) -> C [E, N], both at their own width as pitch
inline GemmArgs edge_linear(const EdgeDims& d, const EdgeOps& o, int K, int N, bool bias, int act, EdgeFmt a, EdgeFmt c, int relu_a = 0) {
    GemmArgs g;
    g.A = o.A; g.lda = K; g.W = o.W; g.ldw = K; g.C = o.C; g.ldc = N; g.M = d.E; g.N = N; g.K = K; g.bias = bias ? o.bias : nullptr; g.act = act;
    g.relu_a = relu_a; g.a_split = a.split; g.c_split = c.split; g.a_pair = (int16_t)a.pair; g.c_pair = (int16_t)c.pair;
    return g;
}
// conv2 / conv3 of a relation encoder (+BN folded) on the edge embedding H1 [E, 64 | 64] (A = H1 + 64 br, pitch 128) -> H2 -> E3 / E2
inline GemmArgs stage_conv2(const EdgeDims& d, const EdgeOps& o) {
    GemmArgs g = edge_linear(d, o, 64, 128, true, ACT_RELU, {}, {d.S});
    g.lda = 128;
    return g;
}
inline GemmArgs stage_conv3(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, int br) {
    return edge_linear(d, o, 128, d.D, true, ACT_RELU, {d.S}, {d.S, P.chain(br)});
}
// nn_edge.0 on the edge part of its weight: Hbig = relu(e . we^T + P_i[src] + P_j[dst]); the node columns (with the bias) were made on N
// rows by the node-side projection.  g_f16: they are fp16 half rows (P_j then starts at byte 2 * 2D of the row)
inline GemmArgs nn_edge0_on(const EdgeDims& d, const EdgeOps& o, int relu_a, bool g_f16, bool e_pair, bool hbig_pair) {
    GemmArgs g = edge_linear(d, o, d.D, 2 * d.D, false, ACT_RELU, {d.S, e_pair}, {d.S, hbig_pair}, relu_a);
    g.g0 = o.NP; g.gi0 = o.src; g.g1 = o.NP + (g_f16 ? d.D : 2 * d.D); g.gi1 = o.dst; g.ldg0 = g.ldg1 = d.NPC; g.g_f16 = g_f16;
    return g;
}
inline GemmArgs stage_nn_edge0(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, int br, int relu_a, bool g_f16) {
    return nn_edge0_on(d, o, relu_a, g_f16, P.chain(br), P.hbig[br]);
}
// proj_edge feeds only the gate MLP; gate16: a 16-bit gate kernel reads KP in the chain's format (the fp32 gate kernels read plain fp32)
inline GemmArgs stage_proj_edge(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, int br, int relu_a, bool gate16) {
    return edge_linear(d, o, d.D, d.D, true, ACT_NONE, {d.S, P.chain(br)}, {gate16 ? d.S : 0}, relu_a);
}
inline GemmArgs stage_nn_edge2(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, int br) {       // e <- nn_edge output (pre-activation)
    return edge_linear(d, o, 2 * d.D, d.D, true, ACT_NONE, {d.S, P.hbig[br]}, {d.S, P.nn_edge2_out(br)});
}
// the three Linears of a relation head: e -> R1 -> R2 -> out; the last with a sigmoid (multi_rel_outputs) or none (log_softmax follows)
inline GemmArgs stage_rel_head1(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, int br, int relu_a) {
    return edge_linear(d, o, d.D, 512, true, ACT_RELU, {d.S, P.chain(br)}, {d.S, P.r1[br]}, relu_a);
}
inline GemmArgs stage_rel_head2(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, int br) {
    return edge_linear(d, o, 512, 256, true, ACT_RELU, {d.S, P.r1[br]}, {d.S});
}
inline GemmArgs stage_rel_head3(const EdgeDims& d, const EdgeOps& o, bool sigmoid) {
    return edge_linear(d, o, 256, d.R, true, sigmoid ? ACT_SIGMOID : ACT_NONE, {d.S}, {});
}
// edge cross-attention: query projection of E2 (the split-format attention takes Q pre-scaled), key | value projection of E3,
// out-projection of Oe + residual E2 -- unless the LayerNorm adds it (ln_resid); o16: fp16 half rows for the LayerNorm
inline GemmArgs stage_attn_q(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, float qscale) {
    GemmArgs g = edge_linear(d, o, d.D, d.D, true, ACT_NONE, {d.S, P.attn_q_in()}, {d.SA});
    if (d.SA) g.c_scale = qscale;
    return g;
}
inline GemmArgs stage_attn_kv(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P) {
    return edge_linear(d, o, d.D, 2 * d.D, true, ACT_NONE, {d.S, P.e3}, {d.SA, P.attn_kv_out()});
}
inline GemmArgs stage_attn_out(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P, bool ln_resid, bool o16) {
    GemmArgs g = edge_linear(d, o, d.D, d.D, true, ACT_NONE, {d.SA, P.oe}, {});
    if (!ln_resid) { g.resid = o.resid; g.ldr = d.D; g.r_split = d.S; }
    if (o16) g.c_f16_cols = d.D;
    return g;
}
// triplet_projector_2d (training outputs): its first Linear like nn_edge.0 on fp32 tables, reading E2 as fp32 and without a pending
// ReLU, then 2D -> D into the caller's output
inline GemmArgs stage_triplet0(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P) { return nn_edge0_on(d, o, 0, false, false, P.hbig[1]); }
inline GemmArgs stage_triplet2(const EdgeDims& d, const EdgeOps& o, const EdgePairs& P) {
    return edge_linear(d, o, 2 * d.D, d.D, true, ACT_NONE, {d.S, P.hbig[1]}, {});
}

}  // namespace vlsat
