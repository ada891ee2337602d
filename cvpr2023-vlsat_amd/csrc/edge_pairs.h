// fp32 mode: which edge-row tensors of a forward travel as GEMM PAIR WORDS (gemm_f16s_planes.h: Ah << 16 | Al, the two halves of the
// split-fp16 operand, made once by the writer's epilogue instead of by every reader) -- decided ONCE per forward, here, for every launch
// that touches them.  No HIP header: tests/edge_pairs_check.cpp compiles this with g++ and prints every decision with its reason.
//
// A tensor qualifies only if EVERY launch that writes or reads it in this forward runs, in all its parts (full rounds and tail), on a
// kernel with the pair forms: the split-fp16 8-phase kernel (gemm_p8s_pair_pick) or the split-fp16 persistent kernel
// (gemm_f16s_tiled_pick).  The function asks the planner (plan_gemm) what each launch gets, with the launch's own shape and flags; a
// part on split-K, on an exact kernel or on a twin launch of the paired schedule refuses the tensor, which then stays fp32 for everyone.
// Candidates: Hbig of either branch (nn_edge.0 -> nn_edge.2), R1 of either branch (relation head, first -> second Linear) and the 3D chain
// tensor E3 (relation encoder conv3 / nn_edge.2 -> nn_edge.0, proj_edge, key | value projection, relation head); K | V of the edge
// attention (key | value projection -> split-fp16 attention kernel, as ATTENTION pair words) and, with them, its output Oe (attention
// kernel in one key part -> out-projection, as GEMM pair words; split-key partials and the merge kernel keep fp32).  Q stays fp32 (the
// attention splits it once per block) and KP is read by the gate: fp32.
// The 2D chain tensor E2 holds two kinds of content in a layer.  What the LayerNorm of the edge attention writes (and, before the first
// layer, conv3 of rel_encoder_2d) is read only as a GEMM A operand -- nn_edge.0 and proj_edge of gcn_2ds, after the last layer the first
// Linear of the 2D relation head -- and travels as GEMM pair words (`e2`; the LayerNorm kernel packs with output format 6).  What
// nn_edge.2 of gcn_2ds writes into the same buffer is also the fp32 residual of the out-projection (a pair word holds about 22 bits):
// it stays fp32, and the query projection splits it on the fly.
#pragma once
#include "flash_pick.h"
#include "gemm_plan.h"

namespace vlsat {

struct EdgePairsIn {
    long E = 0;                  // edges of the plan
    int D = 512;                 // edge feature width (nn_edge.0: D -> 2D -> D)
    int G = 512;                 // resident 256-thread blocks at two per CU (gemm_slots)
    int option = 1;              // debug option "edge_pairs": 0 = everything stays fp32 (the forward of the releases before the pair words)
    int option_e2 = 1;           // debug option "edge_pairs_e2": 0 = E2 stays fp32 (the forward of the release before E2 paired)
    bool fp32_mode = true;       // precision mode 0 (prec == prec_edge == 0)
    bool gemm_exact = false, gemm_small_exact = false;     // debug options: exact kernels for the 8-phase / persistent launches
    bool no_dma = false, no_p8 = false, splitk = true;     // debug options "gemm_dma" 0, "gemm_p8" 0, "gemm_splitk"
    int p8_part_min = 0, sk_max_tiles = 64;                // "gemm_p8_part_min", "gemm_splitk_max_tiles"
    bool paired = false;         // paired schedule of one-scene plans: twin launches of two problems
    bool do2d = true;            // the 2D branch runs (key | value projection reads E3)
    bool use_gcn_edge = true;    // proj_edge runs
    bool feature_transform = false, train = false, prob_tap = false;
    int debug_stop = -1;
    // the edge attention of this forward: the split-fp16 kernel runs (fp32 mode, head dim in its list, "flash_exact" off), its V operand
    // read (0 gather | 1 transpose read), the plan's key parts (1: no split keys)
    bool flash_x3 = true;
    int head_dim = 64, flash_tr = 1, fa_parts = 1;
};
struct EdgePairs {
    bool hbig[2] = {false, false}, r1[2] = {false, false}, e3 = false;     // [branch]: 0 = 3D, 1 = 2D
    bool kv = false, oe = false;                                            // K | V (attention pair words), Oe (GEMM pair words)
    bool e2 = false;                                                        // E2 as the LayerNorm / conv3 of rel_encoder_2d write it (nn_edge.2's E2 stays fp32)
    const char *why_hbig[2] = {nullptr, nullptr}, *why_r1[2] = {nullptr, nullptr}, *why_e3 = nullptr;      // why not (null: it pairs)
    const char *why_kv = nullptr, *why_oe = nullptr, *why_e2 = nullptr;
    int flash_io() const { return kv ? (oe ? 5 : 4) : 0; }                  // what the attention launch is told (flash_f16x3_pair_pick)
    bool any() const { return hbig[0] || hbig[1] || r1[0] || r1[1] || e3 || kv || oe || e2; }
};

// an edge-row Linear of the forward as the engine launches it in the fp32 mode, on placeholder operands (the planner looks at shapes,
// flags, which operands exist and their alignment -- never through a pointer)
inline GemmArgs edge_pairs_probe(const EdgePairsIn& in, int N, int K, int add, bool relu_a, int act) {
    static float dummy[4] __attribute__((aligned(16)));
    static uint16_t dummy16[8] __attribute__((aligned(16)));
    static int32_t dummy_i[1];
    static unsigned dummy_u[1];
    GemmArgs a;
    a.A = dummy; a.lda = K; a.W = dummy; a.ldw = K; a.C = dummy; a.ldc = N; a.M = (int)in.E; a.N = N; a.K = K; a.bias = add == 6 ? nullptr : dummy;
    a.act = act; a.relu_a = relu_a;
    if (add & 1) { a.resid = dummy; a.ldr = N; }
    if (add & 6) { a.g0 = a.g1 = dummy; a.gi0 = a.gi1 = dummy_i; a.ldg0 = a.ldg1 = 6 * in.D + 256; }
    a.prec = 0;
    a.f16s = in.gemm_small_exact ? (in.gemm_exact ? 0 : 1) : (in.gemm_exact ? 3 : 2);      // (engine_forward.hip gemm_resolve, edge rows)
    a.Wh16 = a.Wl16 = dummy16;
    a.no_dma = in.no_dma; a.no_p8 = in.no_p8; a.p8_part_min = in.p8_part_min;
    if (in.splitk) {
        a.sk_ws = dummy; a.sk_ws_floats = SPLITK_WS_FLOATS; a.sk_counters = dummy_u; a.sk_n_counters = SPLITK_COUNTERS;
        a.sk_max_tiles = in.sk_max_tiles;
    }
    return a;
}
// nullptr when every part of the launch (launch_gemm's loop: a plan, then the rows it leaves) runs on a kernel with the pair forms
inline const char* edge_pairs_launch(GemmArgs a, int G, int a_pair, int c_pair) {
    if (a.M <= 0) return nullptr;                                    // (an empty launch launches nothing)
    if (a.f16s != 2) return "gemm_exact / gemm_small_exact: a part of the launch runs on an exact fp32 kernel";
    a.a_pair = a_pair; a.c_pair = c_pair;
    if (gemm_invalid(a)) return "the launch is not valid with pair words";
    for (int guard = 0; guard < 64; ++guard) {
        const GemmPlan p = plan_gemm(a, G);
        GemmArgs m = a;
        m.M = p.rows;
        if (p.family == GemmPlan::P8) {
            if (gemm_p8s_pair_pick(m, p.variant) < 0) return "an 8-phase part without a split-fp16 pair form";
        } else if (p.family == GemmPlan::TILED) {
            if (gemm_f16s_tiled_pick(m, p.variant).index < 0) return "a persistent-kernel part stays on the exact fp32 kernel";
        } else {
            return p.family == GemmPlan::SPLITK ? "a part runs on the split-K kernel (exact fp32)" : "a part runs on a kernel without pair forms";
        }
        if (p.rows >= a.M) return nullptr;
        a.M -= p.rows;                                               // the tail: the same problem on the rows left (tail_of)
    }
    return "the launch does not finish planning";
}

inline EdgePairs edge_pairs_plan(const EdgePairsIn& in) {
    EdgePairs r;
    const char* all = nullptr;
    if (!in.option) all = "edge_pairs is 0";
    else if (!in.fp32_mode) all = "not the fp32 precision mode";
    else if (in.E <= 0) all = "no edges";
    else if (in.paired) all = "paired schedule: the twin stages are launches of two problems";
    if (all) {
        r.why_hbig[0] = r.why_hbig[1] = r.why_r1[0] = r.why_r1[1] = r.why_e3 = r.why_kv = r.why_oe = r.why_e2 = all;
        return r;
    }
    const int D = in.D, G = in.G;
    auto first = [](const char* a, const char* b) { return a ? a : b; };
    // Hbig: nn_edge.0 (gathered node rows, ReLU; ReLU-on-A or not, A fp32 or pairs: every form is built) -> nn_edge.2
    const char* hb = first(edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 6, false, ACT_RELU), G, 0, 1),
                           first(edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 6, true, ACT_RELU), G, 1, 1),
                                 edge_pairs_launch(edge_pairs_probe(in, D, 2 * D, 0, false, ACT_NONE), G, 1, 0)));
    r.why_hbig[0] = r.why_hbig[1] = hb;
    r.hbig[0] = !hb;
    r.hbig[1] = !hb && in.do2d;
    if (!r.hbig[1] && !hb) r.why_hbig[1] = "the 2D branch does not run";
    // R1: first Linear of a relation head (D -> 512, ReLU) -> second (512 -> 256)
    const char* r1 = first(edge_pairs_launch(edge_pairs_probe(in, 512, D, 0, true, ACT_RELU), G, 1, 1),
                           first(edge_pairs_launch(edge_pairs_probe(in, 512, D, 0, false, ACT_RELU), G, 0, 1),
                                 edge_pairs_launch(edge_pairs_probe(in, 256, 512, 0, false, ACT_RELU), G, 1, 0)));
    r.why_r1[0] = r.why_r1[1] = r1;
    r.r1[0] = !r1;
    // (the 2D head: its first Linear reads E2, an fp32 tensor, so it still splits its A operand AND packs its output -- measured per launch
    //  at the bench batch, the packing costs that launch what the second Linear then saves: 160.7 + 56.3 -> 167.9 + 49.4 us,
    //  profiles/edge_pairs_ab.txt -- taken out; the 3D head reads E3 as pairs and gains in both launches.  That was measured while E2 was
    //  fp32 for every reader; with E2 paired (below) the first Linear no longer splits its A operand, and R1 of the 2D head has not been
    //  measured again: 7 us, left as it is)
    r.r1[1] = false;
    if (!r1) r.why_r1[1] = in.do2d ? "measured: packing in the first Linear (A = E2, fp32) costs what the second saves" : "the 2D branch does not run";
    // E3: written by conv3 of rel_encoder_3d (128 -> D) and by nn_edge.2 of gcn_3ds; read by nn_edge.0, proj_edge, the key | value projection
    // of the edge attention and the 3D relation head (whose other operand, Hbig / R1, carries the format decided above)
    const char* e3 = nullptr;
    if (in.debug_stop >= 0) e3 = "a debug stop: the caller may read E3";
    else if (in.train) e3 = "training outputs";
    else if (in.feature_transform) e3 = "feature_transform: E3 is copied out of the encoder's fp32 rows";
    else if (in.prob_tap) e3 = "the probability tap";
    if (!e3) e3 = edge_pairs_launch(edge_pairs_probe(in, D, 128, 0, false, ACT_RELU), G, 0, 1);              // conv3
    if (!e3) e3 = edge_pairs_launch(edge_pairs_probe(in, D, 2 * D, 0, false, ACT_NONE), G, r.hbig[0], 1);      // nn_edge.2
    if (!e3) e3 = edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 6, true, ACT_RELU), G, 1, r.hbig[0]);       // nn_edge.0
    if (!e3) e3 = edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 6, false, ACT_RELU), G, 1, r.hbig[0]);
    if (!e3 && in.use_gcn_edge) e3 = first(edge_pairs_launch(edge_pairs_probe(in, D, D, 0, true, ACT_NONE), G, 1, 0),      // proj_edge
                                           edge_pairs_launch(edge_pairs_probe(in, D, D, 0, false, ACT_NONE), G, 1, 0));
    // K | V: key | value projection (D -> 2D) -> the split-fp16 attention kernel; Oe: that kernel in one key part -> out-projection (+ residual)
    const char* kv = nullptr;
    if (!in.do2d) kv = "the 2D branch does not run";
    else if (!in.flash_x3) kv = "the edge attention runs on another kernel (flash_exact, head dim, VALU attention)";
    else if (flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 4).index < 0) kv = flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 4).error;
    if (!kv) kv = edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 0, false, ACT_NONE), G, 0, 2);
    r.why_kv = kv;
    r.kv = !kv;
    const char* oe = kv ? "K and V stay fp32: Oe pairs only with them" : nullptr;
    if (!oe && in.fa_parts > 1) oe = "split keys: the partials and the merge kernel are fp32";
    if (!oe && flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 5, in.fa_parts).index < 0) oe = flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 5, in.fa_parts).error;
    if (!oe) oe = edge_pairs_launch(edge_pairs_probe(in, D, D, 1, false, ACT_NONE), G, 1, 0);
    r.why_oe = oe;
    r.oe = !oe;
    if (!e3 && in.do2d) e3 = edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 0, false, ACT_NONE), G, 1, r.kv ? 2 : 0);   // key | value
    if (!e3) e3 = first(edge_pairs_launch(edge_pairs_probe(in, 512, D, 0, true, ACT_RELU), G, 1, r.r1[0]),                // relation head
                        edge_pairs_launch(edge_pairs_probe(in, 512, D, 0, false, ACT_RELU), G, 1, r.r1[0]));
    r.why_e3 = e3;
    r.e3 = !e3;
    // E2 of the LayerNorm and of conv3 of rel_encoder_2d (128 -> D, C pairs): read by nn_edge.0 (no pending ReLU: the LayerNorm applies
    // it) and proj_edge of gcn_2ds and by the first Linear of the 2D relation head (whose output R1 stays fp32, above)
    const char* e2 = nullptr;
    if (!in.option_e2) e2 = "edge_pairs_e2 is 0";
    else if (!in.do2d) e2 = "the 2D branch does not run";
    else if (in.debug_stop >= 0) e2 = "a debug stop: the caller may read E2";
    else if (in.train) e2 = "training outputs: the first Linear of triplet_projector_2d reads E2 as fp32";
    else if (in.feature_transform) e2 = "feature_transform: E2 is copied out of the encoder's fp32 rows";
    if (!e2) e2 = edge_pairs_launch(edge_pairs_probe(in, D, 128, 0, false, ACT_RELU), G, 0, 1);                           // conv3
    if (!e2) e2 = edge_pairs_launch(edge_pairs_probe(in, 2 * D, D, 6, false, ACT_RELU), G, 1, r.hbig[1]);                 // nn_edge.0
    if (!e2 && in.use_gcn_edge) e2 = edge_pairs_launch(edge_pairs_probe(in, D, D, 0, false, ACT_NONE), G, 1, 0);          // proj_edge
    if (!e2) e2 = edge_pairs_launch(edge_pairs_probe(in, 512, D, 0, false, ACT_RELU), G, 1, r.r1[1]);                     // relation head
    r.why_e2 = e2;
    r.e2 = !e2;
    return r;
}

}  // namespace vlsat
