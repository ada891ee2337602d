// Host-only check of the decision that lets the 2D chain tensor E2 -- as the LayerNorm of the edge attention and conv3 of rel_encoder_2d
// write it -- travel as GEMM pair words (csrc/edge_pairs.h: EdgePairs::e2 / why_e2).  g++ only (optionally ASan + UBSan): no HIP header,
// no library, no device.
//   e2_pairs_check                 one line per plan: "<case> -> E2 pairs|fp32 (<reason>) | Hbig2 0|1 | conv3 <parts> | nn_edge.0 <parts> |
//                                  proj_edge <parts> | head <parts>": for each launch that touches that E2, the kernel family of every part
//                                  plan_gemm gives it (full rounds, then the tail), asked here with the launch's shape and flags, and
//                                  whether that part has the pair form: "p8+", "tiled+", "p8-", "tiled-", "splitk-", "other-", "exact-"
//   e2_pairs_check pack <hex>...   the GEMM pair word of each fp32 bit pattern: "<hex> -> <word>"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "edge_pairs.h"
#include "gemm_f16s_planes.h"

using namespace vlsat;

// the parts of one launch (a stage of csrc/edge_stages.h, as the forward launches it), in this program's own words: plan, take the rows
// the plan covers, plan the rest
static std::string parts(const EdgePairsIn& in, const GemmArgs& stage) {
    GemmArgs a = edge_pairs_resolve(in, stage);
    if (a.M <= 0) return "none";
    if (a.f16s != 2) return "exact-";
    if (gemm_invalid(a)) return "invalid-";
    std::string out;
    for (int guard = 0; guard < 64 && a.M > 0; ++guard) {
        const GemmPlan p = plan_gemm(a, in.G);
        GemmArgs m = a;
        m.M = p.rows;
        if (!out.empty()) out += ",";
        if (p.family == GemmPlan::P8) out += gemm_p8s_pair_pick(m, p.variant) >= 0 ? "p8+" : "p8-";
        else if (p.family == GemmPlan::TILED) out += gemm_f16s_tiled_pick(m, p.variant).index >= 0 ? "tiled+" : "tiled-";
        else out += p.family == GemmPlan::SPLITK ? "splitk-" : "other-";
        if (p.rows <= 0) return out + ",stuck-";
        a.M -= p.rows;
    }
    return out;
}

static void plan_line(const char* name, const EdgePairsIn& in) {
    const EdgePairs r = edge_pairs_plan(in);
    // the launches of the 2D branch that touch that E2, with E2 as pair words and Hbig / R1 as the plan decided them
    const EdgeDims d = edge_pairs_dims(in);
    const EdgeOps o = edge_ops_placeholder();
    EdgePairs q = r;
    q.e2 = true;
    std::printf("%s -> E2 %s | Hbig2 %d | conv3 %s | nn_edge.0 %s | proj_edge %s | head %s\n", name,
                r.e2 ? "pairs" : (std::string("fp32 (") + (r.why_e2 ? r.why_e2 : "?") + ")").c_str(), r.hbig[1] ? 1 : 0,
                parts(in, stage_conv3(d, o, q, 1)).c_str(), parts(in, stage_nn_edge0(d, o, q, 1, 0, false)).c_str(),
                in.use_gcn_edge ? parts(in, stage_proj_edge(d, o, q, 1, 0, false)).c_str() : "none", parts(in, stage_rel_head1(d, o, q, 1, 0)).c_str());
}

int main(int argc, char** argv) {
    if (argc > 2 && !std::strcmp(argv[1], "pack")) {
        for (int i = 2; i < argc; ++i) {
            const uint32_t bits = (uint32_t)std::strtoul(argv[i], nullptr, 16);
            std::printf("%08x -> %08x\n", bits, f16s_pair_pack(f16s_float(bits)));
        }
        return 0;
    }
    EdgePairsIn bench;                                   // the bench batch: 64 scenes x 40 objects, 256 CUs
    bench.E = 64 * 40 * 39; bench.G = 512;
    plan_line("bench batch", bench);
    { EdgePairsIn in = bench; in.do2d = false; plan_line("bench batch, 3D only", in); }
    { EdgePairsIn in = bench; in.debug_stop = 12; plan_line("bench batch, debug stop", in); }
    { EdgePairsIn in = bench; in.train = true; plan_line("bench batch, training outputs", in); }
    { EdgePairsIn in = bench; in.feature_transform = true; plan_line("bench batch, feature_transform", in); }
    { EdgePairsIn in = bench; in.option = 0; plan_line("bench batch, edge_pairs 0", in); }
    { EdgePairsIn in = bench; in.option_e2 = 0; plan_line("bench batch, edge_pairs_e2 0", in); }
    { EdgePairsIn in = bench; in.gemm_exact = true; plan_line("bench batch, gemm_exact 1", in); }
    { EdgePairsIn in = bench; in.gemm_small_exact = true; plan_line("bench batch, gemm_small_exact 1", in); }
    { EdgePairsIn in = bench; in.flash_x3 = false; plan_line("bench batch, flash_exact 1", in); }
    { EdgePairsIn in = bench; in.use_gcn_edge = false; plan_line("bench batch, no proj_edge", in); }
    EdgePairsIn small;                                   // 3 scenes x 16 objects
    small.E = 720; small.G = 512;
    plan_line("E = 720", small);
    { EdgePairsIn in = small; in.p8_part_min = 1; plan_line("E = 720, gemm_p8_part_min 1", in); }
    { EdgePairsIn in = small; in.gemm_exact = true; plan_line("E = 720, gemm_exact 1", in); }
    { EdgePairsIn in = small; in.gemm_small_exact = true; plan_line("E = 720, gemm_small_exact 1", in); }
    { EdgePairsIn in = small; in.flash_x3 = false; plan_line("E = 720, flash_exact 1", in); }
    { EdgePairsIn in = small; in.E = 5 * 4 + 0 + 7 * 6; plan_line("scenes of 5, 1 and 7 objects (E = 62)", in); }
    { EdgePairsIn in = small; in.E = 5 * 4 + 0 + 7 * 6; in.splitk = false; plan_line("scenes of 5, 1 and 7 objects (E = 62), gemm_splitk 0", in); }
    { EdgePairsIn in = small; in.E = 0; plan_line("E = 0", in); }
    { EdgePairsIn in = small; in.E = 72; in.paired = true; plan_line("one scene of 9 objects, paired schedule", in); }
    { EdgePairsIn in; in.E = 200 * 199; in.G = 512; plan_line("one scene of 200 objects", in); }
    return 0;
}
