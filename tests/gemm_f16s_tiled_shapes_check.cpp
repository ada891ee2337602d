// Host-only check of the shape list of tests/test_hip_gemm_f16s_tiled.py against csrc/gemm_plan.h (built with g++ by tests/host_check.py;
// opens no device): what launch_gemm plans for every shape x form at 256 CUs (512 resident slots) when the problem comes from
// vlsat_k_gemm_f16s(..., -1) -- f16s = 2, no split-K workspace, the built-in p8_part_min.  Arguments: the shapes as M,N,K.
// Prints one "launch | ..." line per planned launch, then one "name -> ok ..." line per check; exits 1 at the first failure:
//   families   every launch and tail of every shape is in the TILED family (none on the 8-phase or split-K kernel)
//   siblings   every one of them gets a row of the siblings' list from gemm_f16s_tiled_pick
//   tiles      every one of the five tiles of kGemmTiles is reached
//   twin       at least one shape pairs as a twin (gemm_pair_plan) whose pair takes a sibling, for both ReLU-on-A settings of the second problem
//   refused    N = 26, f16s = 1, no_dma, a single gathered-row operand and an operand format get -1 and a reason
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gemm_plan.h"

using namespace vlsat;

namespace {

alignas(64) float g_buf[64];
alignas(64) uint16_t g_planes[64];
alignas(64) int32_t g_idx[64];
constexpr int G = 512;
const int kForms[5][2] = {{0, 0}, {0, 1}, {1, 0}, {6, 0}, {6, 1}};

GemmArgs problem(int M, int N, int K, int add, int relu_a) {
    GemmArgs a;
    a.A = g_buf; a.lda = K; a.W = g_buf; a.ldw = K; a.C = g_buf; a.ldc = N; a.M = M; a.N = N; a.K = K;
    a.bias = g_buf; a.relu_a = relu_a;
    if (add & 1) { a.resid = g_buf; a.ldr = N; a.resid_scale = 0.5f; }
    if (add & 2) { a.g0 = g_buf; a.gi0 = g_idx; a.ldg0 = 2 * N; }
    if (add & 4) { a.g1 = g_buf; a.gi1 = g_idx; a.ldg1 = 2 * N; }
    a.f16s = 2; a.Wh16 = g_planes; a.Wl16 = g_planes; a.w_exp = 17;
    return a;
}

[[noreturn]] void die(const char* what, int M, int N, int K, int add, int relu) {
    printf("%s -> FAILED at M %d N %d K %d add %d relu_a %d\n", what, M, N, K, add, relu);
    exit(1);
}

}  // namespace

int main(int argc, char** argv) {
    int tiles_seen[kGemmTileCount] = {0, 0, 0, 0, 0}, launches = 0, twins = 0;
    for (int i = 1; i < argc; ++i) {
        int M = 0, N = 0, K = 0;
        if (sscanf(argv[i], "%d,%d,%d", &M, &N, &K) != 3) { printf("arguments -> FAILED %s\n", argv[i]); return 1; }
        for (const auto& form : kForms) {
            GemmArgs a = problem(M, N, K, form[0], form[1]);
            if (gemm_invalid(a)) die("valid", M, N, K, form[0], form[1]);
            while (true) {                                    // launch_gemm's loop
                const GemmPlan p = plan_gemm(a, G);
                if (p.family != GemmPlan::TILED || p.variant < 0) die("families", M, N, K, form[0], form[1]);
                const GemmPick fs = gemm_f16s_tiled_pick(a, p.variant);
                if (fs.index < 0 || kGemmF16sTiledAdds[fs.index] != form[0]) die("siblings", M, N, K, form[0], form[1]);
                const int t = gemm_tile_index(p.bm, p.bn, p.ksl);
                ++tiles_seen[t];
                ++launches;
                printf("launch | M %d N %d K %d add %d relu_a %d: rows %d of %d, tile %d x %d ksl %d x%d, grid %d, sibling row %d\n", M, N, K, form[0],
                       form[1], p.rows, a.M, p.bm, p.bn, p.ksl, p.slot_mult, p.grid, fs.index);
                if (p.rows == a.M) break;
                a = tail_of(a, p.rows);
            }
            // the pair of this problem with a twin of either ReLU-on-A setting
            for (int relu_b = 0; relu_b < 2; ++relu_b) {
                const GemmArgs x = problem(M, N, K, form[0], form[1]), y = problem(M, N, K, form[0], relu_b);
                const GemmPlan p = gemm_pair_plan(x, y, G, false);
                if (p.variant < 0) continue;
                if (p.family != GemmPlan::TILED) die("twin family", M, N, K, form[0], form[1]);
                if (gemm_f16s_tiled_pick(x, p.variant).index < 0 || gemm_f16s_tiled_pick(y, p.variant).index < 0) die("twin", M, N, K, form[0], form[1]);
                ++twins;
            }
        }
    }
    printf("families -> ok %d launches, all TILED\n", launches);
    printf("siblings -> ok %d\n", launches);
    int reached = 0;
    for (int t = 0; t < kGemmTileCount; ++t) reached += tiles_seen[t] > 0;
    if (reached != kGemmTileCount) { printf("tiles -> FAILED %d %d %d %d %d\n", tiles_seen[0], tiles_seen[1], tiles_seen[2], tiles_seen[3], tiles_seen[4]); return 1; }
    printf("tiles -> ok %d of %d (%d %d %d %d %d launches)\n", reached, kGemmTileCount, tiles_seen[0], tiles_seen[1], tiles_seen[2], tiles_seen[3], tiles_seen[4]);
    if (!twins) { printf("twin -> FAILED\n"); return 1; }
    printf("twin -> ok %d pairs\n", twins);

    // what the pick refuses: the exact kernel runs
    int refused = 0;
    {
        GemmArgs a = problem(2560, 26, 512, 0, 0);
        const GemmPick r = gemm_f16s_tiled_pick(a, plan_gemm(a, G).variant);
        refused += r.index < 0 && r.why;
        a = problem(2560, 512, 512, 0, 0); a.f16s = 1;
        const GemmPick r1 = gemm_f16s_tiled_pick(a, plan_gemm(a, G).variant);
        refused += r1.index < 0 && r1.why;
        a = problem(2560, 512, 512, 0, 0); a.no_dma = 1;
        const GemmPick r2 = gemm_f16s_tiled_pick(a, plan_gemm(a, G).variant);
        refused += r2.index < 0 && r2.why;
        a = problem(2560, 512, 512, 2, 0);
        const GemmPick r3 = gemm_f16s_tiled_pick(a, plan_gemm(a, G).variant);
        refused += r3.index < 0 && r3.why;
        a = problem(2560, 512, 512, 0, 0);
        const int variant = plan_gemm(a, G).variant;
        a.c_scale = 2.f;
        const GemmPick r4 = gemm_f16s_tiled_pick(a, variant);
        refused += r4.index < 0 && r4.why;
        const GemmPick r5 = gemm_f16s_tiled_pick(problem(2560, 512, 512, 0, 0), -1);
        refused += r5.index < 0 && r5.why;
    }
    if (refused != 6) { printf("refused -> FAILED %d of 6\n", refused); return 1; }
    printf("refused -> ok %d\n", refused);
    return 0;
}
