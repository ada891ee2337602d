// fp32 mode: which edge-row tensors of a forward travel as GEMM PAIR WORDS (gemm_f16s_planes.h: Ah << 16 | Al, the two halves of the
// split-fp16 operand, made once by the writer's epilogue instead of by every reader) -- decided ONCE per forward, here, for every launch
// that touches them.  No HIP header: tests/edge_pairs_check.cpp compiles this with g++ and prints every decision with its reason.
//
// A tensor qualifies only if EVERY launch that writes or reads it in this forward runs, in all its parts (full rounds and tail), on a
// kernel with the pair forms: the split-fp16 8-phase kernel (gemm_p8s_pair_pick) or the split-fp16 persistent kernel
// (gemm_f16s_tiled_pick).  The launches are those of edge_stages.h -- the GemmArgs the forward itself launches, built here on placeholder
// operands -- and the function asks the planner (plan_gemm) what each gets; a part on split-K, on an exact kernel or on a twin launch of
// the paired schedule refuses the tensor, which then stays fp32 for everyone.
// Candidates, in the order edge_pairs_plan decides them: Hbig and R1 of either branch, K | V of the edge attention (as ATTENTION pair
// words) and with them its output Oe, the 3D chain tensor E3, and of the 2D chain tensor E2 what the LayerNorm of the edge attention (its
// output format 6) and conv3 of rel_encoder_2d write -- not what nn_edge.2 writes (EdgePairs::nn_edge2_out).  Q stays fp32 (the attention
// splits it once per block) and KP is read by the gate: fp32.
#pragma once
#include "edge_stages.h"
#include "flash_pick.h"

namespace vlsat {

struct EdgePairsIn {
    long E = 0;                  // edges of the plan
    int D = 512, A = 256;        // edge feature width (nn_edge.0: D -> 2D -> D), DIM_ATTEN (the gathered rows' pitch is 6 D + A)
    int G = 512;                 // resident 256-thread blocks at two per CU (gemm_slots)
    int option = 1;              // debug option "edge_pairs": 0 = everything stays fp32 (the forward of the releases before the pair words)
    int option_e2 = 1;           // debug option "edge_pairs_e2": 0 = E2 stays fp32 (the forward of the release before E2 paired)
    bool fp32_mode = true;       // precision mode 0 (engine.h fp32_mode)
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

// the dims of the forward's edge stages in the fp32 mode (format codes 0), and what gemm_resolve of engine_forward.hip adds to an edge-row
// launch of that mode, on placeholders
inline EdgeDims edge_pairs_dims(const EdgePairsIn& in) { return {(int)in.E, in.D, 6 * in.D + in.A}; }
inline GemmArgs edge_pairs_resolve(const EdgePairsIn& in, GemmArgs a) {
    static uint16_t planes[8] __attribute__((aligned(16)));
    static float ws[4] __attribute__((aligned(16)));
    static unsigned counters[1];
    a.prec = 0;
    a.f16s = gemm_f16s_code(in.gemm_exact, in.gemm_small_exact, false);
    a.Wh16 = a.Wl16 = planes;
    a.no_dma = in.no_dma; a.no_p8 = in.no_p8; a.p8_part_min = in.p8_part_min;
    if (in.splitk) {
        a.sk_ws = ws; a.sk_ws_floats = SPLITK_WS_FLOATS; a.sk_counters = counters; a.sk_n_counters = SPLITK_COUNTERS;
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
    const EdgeDims d = edge_pairs_dims(in);
    const EdgeOps o = edge_ops_placeholder();
    // a stage's launch (edge_stages.h), built under the formats asked about: nullptr, or why a part of it has no pair form
    auto ask = [&](const GemmArgs& a) { return edge_pairs_launch(edge_pairs_resolve(in, a), in.G, a.a_pair, a.c_pair); };
    // ... those formats: the chain tensor, Hbig and R1 of branch br as pairs or not (the fp32 mode gathers fp32 tables, adds the residual
    // in the out-projection and runs the fp32 gate: g_f16, ln_resid, o16 and gate16 are off in every launch below)
    auto fmt = [](int br, bool chain, bool hbig = false, bool r1 = false) {
        EdgePairs q;
        (br ? q.e2 : q.e3) = chain; q.hbig[br] = hbig; q.r1[br] = r1;
        return q;
    };
    auto first = [](const char* a, const char* b) { return a ? a : b; };
    // Hbig: nn_edge.0 writes it (its A, the chain tensor, is decided below: fp32 without a pending ReLU and pairs with one are asked;
    // every form is built), nn_edge.2 reads it.  The launches of the two branches are the same: asked once
    const char* hb = first(ask(stage_nn_edge0(d, o, fmt(0, false, true), 0, 0, false)),
                           first(ask(stage_nn_edge0(d, o, fmt(0, true, true), 0, 1, false)), ask(stage_nn_edge2(d, o, fmt(0, false, true), 0))));
    r.why_hbig[0] = r.why_hbig[1] = hb;
    r.hbig[0] = !hb;
    r.hbig[1] = !hb && in.do2d;
    if (!r.hbig[1] && !hb) r.why_hbig[1] = "the 2D branch does not run";
    // R1: the first Linear of a relation head writes it (A: both forms), the second reads it
    const char* r1 = first(ask(stage_rel_head1(d, o, fmt(0, true, false, true), 0, 1)),
                           first(ask(stage_rel_head1(d, o, fmt(0, false, false, true), 0, 0)), ask(stage_rel_head2(d, o, fmt(0, false, false, true), 0))));
    r.why_r1[0] = r.why_r1[1] = r1;
    r.r1[0] = !r1;
    // (the 2D head: its first Linear reads E2, an fp32 tensor, so it still splits its A operand AND packs its output -- measured per launch
    //  at the bench batch, the packing costs that launch what the second Linear then saves: 160.7 + 56.3 -> 167.9 + 49.4 us,
    //  profiles/edge_pairs_ab.txt -- taken out; the 3D head reads E3 as pairs and gains in both launches.  That was measured while E2 was
    //  fp32 for every reader; with E2 paired (below) the first Linear no longer splits its A operand, and R1 of the 2D head has not been
    //  measured again: 7 us, left as it is)
    r.r1[1] = false;
    if (!r1) r.why_r1[1] = in.do2d ? "measured: packing in the first Linear (A = E2, fp32) costs what the second saves" : "the 2D branch does not run";
    // K | V: the key | value projection writes them (A = E3: fp32 here, as pairs below) for the split-fp16 attention kernel
    const char* kv = nullptr;
    if (!in.do2d) kv = "the 2D branch does not run";
    else if (!in.flash_x3) kv = "the edge attention runs on another kernel (flash_exact, head dim, VALU attention)";
    else if (flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 4).index < 0) kv = flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 4).error;
    EdgePairs q;
    q.kv = true;
    if (!kv) kv = ask(stage_attn_kv(d, o, q));
    r.why_kv = kv;
    r.kv = !kv;
    // Oe: that kernel in one key part writes it, the out-projection (+ residual) reads it
    const char* oe = kv ? "K and V stay fp32: Oe pairs only with them" : nullptr;
    if (!oe && in.fa_parts > 1) oe = "split keys: the partials and the merge kernel are fp32";
    if (!oe && flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 5, in.fa_parts).index < 0) oe = flash_f16x3_pair_pick(in.head_dim, in.flash_tr, 5, in.fa_parts).error;
    q.oe = true;
    if (!oe) oe = ask(stage_attn_out(d, o, q, false, false));
    r.why_oe = oe;
    r.oe = !oe;
    // E3: conv3 of rel_encoder_3d and nn_edge.2 of gcn_3ds write it; nn_edge.0 (pending ReLU or not), proj_edge, the key | value projection
    // and the 3D relation head read it -- the other operand of each in the format decided above
    const char* e3 = nullptr;
    if (in.debug_stop >= 0) e3 = "a debug stop: the caller may read E3";
    else if (in.train) e3 = "training outputs";
    else if (in.feature_transform) e3 = "feature_transform: E3 is copied out of the encoder's fp32 rows";
    else if (in.prob_tap) e3 = "the probability tap";
    q = fmt(0, true, r.hbig[0], r.r1[0]);
    q.kv = r.kv;
    if (!e3) e3 = ask(stage_conv3(d, o, q, 0));
    if (!e3) e3 = ask(stage_nn_edge2(d, o, q, 0));
    if (!e3) e3 = first(ask(stage_nn_edge0(d, o, q, 0, 1, false)), ask(stage_nn_edge0(d, o, q, 0, 0, false)));
    if (!e3 && in.use_gcn_edge) e3 = first(ask(stage_proj_edge(d, o, q, 0, 1, false)), ask(stage_proj_edge(d, o, q, 0, 0, false)));
    if (!e3 && in.do2d) e3 = ask(stage_attn_kv(d, o, q));
    if (!e3) e3 = first(ask(stage_rel_head1(d, o, q, 0, 1)), ask(stage_rel_head1(d, o, q, 0, 0)));
    r.why_e3 = e3;
    r.e3 = !e3;
    // E2 of the LayerNorm and of conv3 of rel_encoder_2d: nn_edge.0 (no pending ReLU: the LayerNorm applies it) and proj_edge of gcn_2ds
    // and the first Linear of the 2D relation head (whose output R1 stays fp32, above) read it
    const char* e2 = nullptr;
    if (!in.option_e2) e2 = "edge_pairs_e2 is 0";
    else if (!in.do2d) e2 = "the 2D branch does not run";
    else if (in.debug_stop >= 0) e2 = "a debug stop: the caller may read E2";
    else if (in.train) e2 = "training outputs: the first Linear of triplet_projector_2d reads E2 as fp32";
    else if (in.feature_transform) e2 = "feature_transform: E2 is copied out of the encoder's fp32 rows";
    q = fmt(1, true, r.hbig[1], r.r1[1]);
    if (!e2) e2 = ask(stage_conv3(d, o, q, 1));
    if (!e2) e2 = ask(stage_nn_edge0(d, o, q, 1, 0, false));
    if (!e2 && in.use_gcn_edge) e2 = ask(stage_proj_edge(d, o, q, 1, 0, false));
    if (!e2) e2 = ask(stage_rel_head1(d, o, q, 1, 0));
    r.why_e2 = e2;
    r.e2 = !e2;
    return r;
}

}  // namespace vlsat
