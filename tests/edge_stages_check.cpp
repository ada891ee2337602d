// Host-only check of csrc/edge_stages.h: every edge-row Linear of the forward as the GemmArgs of its launch.  g++ only (optionally ASan +
// UBSan): no HIP header, no library, no device.
//   edge_stages_check      one line per stage, branch and case that changes a field:
//                          "<stage> <param>=<value> ... -> <field>=<value> ...", every field of the GemmArgs the builders set.
// Dims: D = 512, A = 256 (NP pitch 3328), R = 26, E = 720.  Params: br (0 = 3D, 1 = 2D), S / SA (format codes of the chain tensors / of
// Q, K|V, O), relu (pending ReLU on A), g16 (fp16 gather tables), gate16 (16-bit gate kernel), lnres (the LayerNorm adds the residual),
// o16 (fp16 half rows for the LayerNorm), sig (sigmoid head), pairs: none | all | kv (K|V only) | nokv (all but K|V).
// ops=1: A, W, C and every additive operand the launch has are the ones the caller gave; g1: offset of the second gather table in floats.
#include <cstdio>
#include <string>

#include "edge_stages.h"

using namespace vlsat;

static float mem[8 * 2048] __attribute__((aligned(16)));
static int32_t idx[2][4];
static const EdgeOps o = {mem, mem + 2048, mem + 2 * 2048, mem + 3 * 2048, mem + 4 * 2048, mem + 5 * 2048, idx[0], idx[1]};

static void line(const std::string& name, const GemmArgs& g) {
    const bool ops = g.A == o.A && g.W == o.W && g.C == o.C && (!g.bias || g.bias == o.bias) && (!g.resid || g.resid == o.resid) &&
                     (!g.g0 || (g.g0 == o.NP && g.gi0 == o.src)) && (!g.g1 || g.gi1 == o.dst) && !g.rowscale && g.resid_scale == 1.f;
    std::printf("%s -> M=%d N=%d K=%d lda=%d ldw=%d ldc=%d ops=%d bias=%d resid=%d ldr=%d g=%d ldg0=%d ldg1=%d g1=%ld act=%s relu_a=%d a_split=%d "
                "c_split=%d r_split=%d c_scale=%g c_f16_cols=%d g_f16=%d a_pair=%d c_pair=%d\n",
                name.c_str(), g.M, g.N, g.K, g.lda, g.ldw, g.ldc, ops ? 1 : 0, g.bias ? 1 : 0, g.resid ? 1 : 0, g.ldr, (g.g0 ? 1 : 0) | (g.g1 ? 2 : 0),
                g.ldg0, g.ldg1, g.g1 ? (long)(g.g1 - o.NP) : 0L, g.act == ACT_NONE ? "none" : g.act == ACT_RELU ? "relu" : g.act == ACT_SIGMOID ? "sigmoid" : "?",
                g.relu_a, g.a_split, g.c_split, g.r_split, (double)g.c_scale, g.c_f16_cols, g.g_f16, (int)g.a_pair, (int)g.c_pair);
}
static std::string kv(const char* k, int v) { return std::string(" ") + k + "=" + std::to_string(v); }

int main() {
    const char* pair_names[4] = {"none", "all", "kv", "nokv"};
    for (int S = 0; S < 3; ++S) {
        EdgeDims d;
        d.E = 720; d.D = 512; d.NPC = 6 * 512 + 256; d.R = 26; d.S = S;
        const std::string s = kv("S", S);
        line("conv2" + s, stage_conv2(d, o));
        for (int sig = 0; sig < 2; ++sig) line("head3" + s + kv("sig", sig), stage_rel_head3(d, o, sig != 0));
        for (int pc = 0; pc < 4; ++pc) {
            EdgePairs P;
            const bool rest = pc == 1 || pc == 3;
            P.hbig[0] = P.hbig[1] = P.r1[0] = P.r1[1] = P.e3 = P.e2 = P.oe = rest;
            P.kv = pc == 1 || pc == 2;
            const std::string p = std::string(" pairs=") + pair_names[pc];
            for (int br = 0; br < 2; ++br) {
                const std::string b = kv("br", br) + s;
                line("conv3" + b + p, stage_conv3(d, o, P, br));
                line("nn_edge.2" + b + p, stage_nn_edge2(d, o, P, br));
                line("head2" + b + p, stage_rel_head2(d, o, P, br));
                for (int relu = 0; relu < 2; ++relu) {
                    for (int f = 0; f < 2; ++f) {
                        line("nn_edge.0" + b + kv("relu", relu) + kv("g16", f) + p, stage_nn_edge0(d, o, P, br, relu, f != 0));
                        line("proj_edge" + b + kv("relu", relu) + kv("gate16", f) + p, stage_proj_edge(d, o, P, br, relu, f != 0));
                    }
                    line("head1" + b + kv("relu", relu) + p, stage_rel_head1(d, o, P, br, relu));
                }
            }
            line("triplet0" + s + p, stage_triplet0(d, o, P));
            line("triplet2" + s + p, stage_triplet2(d, o, P));
            for (int SA = 0; SA < 3; ++SA) {
                EdgeDims da = d;
                da.SA = SA;
                const std::string a = s + kv("SA", SA);
                line("attn_q" + a + p, stage_attn_q(da, o, P, 0.25f));
                line("attn_kv" + a + p, stage_attn_kv(da, o, P));
                for (int lnres = 0; lnres < 2; ++lnres)
                    for (int o16 = 0; o16 < 2; ++o16) line("attn_out" + a + kv("lnres", lnres) + kv("o16", o16) + p, stage_attn_out(da, o, P, lnres != 0, o16 != 0));
            }
        }
    }
    return 0;
}
