// fp32 MFMA GEMM with fused epilogues -- the engine behind every nn.Linear / Conv1d(k=1) of
// the path (reference call sites: network_MMG.py:40,93-98; attention.py:54-58,77;
// network_PointNet.py:329-339; SGFN_MMG/model.py:294,305-306,329-330; clip_adapter/model.py:27-29).
//
// C[M,N] = act(rowscale * (A[M,K] . W[N,K]^T) + bias + resid_scale*resid + g0[gi0] + g1[gi1])
//
// Block = 256 threads = 4 waves in a 2x2 grid; block tile BM x BN, wave tile (BM/2) x (BN/2)
// made of 32x32 MFMA tiles; K streamed in BK=32 slices through double-buffered LDS, one barrier
// per slice.  Default operand pipe (PipeF32Dma, gemm_core.h): the loads of slice t+1 are issued
// before the MFMAs of slice t as `buffer_load_dwordx4 ... lds` straight into the other buffer
// (XOR-swizzled unpadded rows, no VGPR round trip, no ds_write).  ReLU-on-A launches and operands
// beyond 32-bit offsets use the VGPR-staged pipe (PipeF32: global_load -> registers -> ds_write).
//
// PERSISTENT + pipelined across tiles: the grid is (at most) 2 blocks per CU and every block
// walks a list of output tiles.  The slice pipeline does not drain at a tile boundary: the
// first slice of the NEXT tile is prefetched under the last slice of the current one, the
// additive epilogue operands (residual / gathered rows) are loaded straight into the
// accumulators at the start of a tile, and the stores of a finished tile retire under the next
// tile's MFMAs.  With
// K = 512 (16 slices per tile) the per-tile load/store bubble was ~20 % of the tile time
// in the one-tile-per-block version (blocks co-resident on a CU run in lock-step, so their
// bubbles coincide instead of hiding each other).
//
// Tile order is XCD-aware: in round r the 64 blocks resident on XCD x (block id % 8 == x) own
// 64 CONSECUTIVE tiles (N fastest), i.e. whole M-panels, so an A panel is fetched from HBM
// once and re-read from that XCD's L2 by its N-tile neighbours.
//
// Tail: a launch covers only full rounds of the grid; the launcher hands the remaining
// M-panels to a second launch with a smaller tile so the last, mostly idle round of big tiles
// (up to 1 of 6 rounds at cfg 2) becomes a quarter-length round.
//
// Roofline: fp32 MFMA (157.3 TF).  Per 128x128x32 slice a block moves 32 KB from L2 for
// 1.05 MFLOP (~19 GB/s/CU at peak rate): MFMA-issue bound, LDS is 4 ds_read_b128 per 16 MFMAs.
#include "gemm_core.h"
#include "kernels.h"

namespace vlsat {

// the kernel text, once per kernel name: the rows of the variant list, and the split-fp16 siblings of its exact-fp32 rows (fp32 mode)
#define VLSAT_TILED_NAME gemm_f32_kernel
#include "gemm_tiled_kernel.h"
#undef VLSAT_TILED_NAME
#define VLSAT_TILED_NAME gemm_f16s_kernel
#include "gemm_tiled_kernel.h"
#undef VLSAT_TILED_NAME

double gemm_flops(const GemmArgs& a) { return 2.0 * a.M * (double)a.N * a.K; }

// resident 256-thread blocks the persistent grid may use (2 per CU): a constant of the device, cached per device id
static int slots() { return gemm_slots(); }
int gemm_slots() {
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!cache[dev]) {
        int cus = 256;
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount;
        cache[dev] = std::max(8, ((2 * cus) / 8) * 8);
    }
    return cache[dev];
}

// one row of kernel pointers per row of the variant list (gemm_plan.h), in its order: the tiles of kGemmTiles, then the twin form
// (null where the row has none).  Taking the address is what instantiates a kernel.
typedef void (*TiledKernel)(GemmArgs, GemmArgs, int, int);
template <int ADD, int PREC, bool TWIN> constexpr TiledKernel tiled_twin() { if constexpr (TWIN) return gemm_f32_kernel<64, 64, ADD, PREC, 2, true>; else return nullptr; }
#define VLSAT_TILED_KERNELS(ADD, PREC, TWIN)                                                                                         \
    {gemm_f32_kernel<128, 128, ADD, PREC, 1>, gemm_f32_kernel<128, 64, ADD, PREC, 1>, gemm_f32_kernel<64, 128, ADD, PREC, 1>,        \
     gemm_f32_kernel<64, 64, ADD, PREC, 1>, gemm_f32_kernel<64, 64, ADD, PREC, 2>, tiled_twin<ADD, PREC, TWIN>()},
constexpr TiledKernel kTiledKernels[][kGemmTileCount + 1] = {VLSAT_GEMM_TILED_VARIANTS(VLSAT_TILED_KERNELS)};
#undef VLSAT_TILED_KERNELS
static_assert(sizeof kTiledKernels / sizeof kTiledKernels[0] == kGemmTiledCount, "one row of kernels per row of the variant list");
// ... and per row of the siblings' list: the same tiles and the twin form
#define VLSAT_F16S_KERNELS(ADD)                                                                                                       \
    {gemm_f16s_kernel<128, 128, ADD, 17, 1>, gemm_f16s_kernel<128, 64, ADD, 17, 1>, gemm_f16s_kernel<64, 128, ADD, 17, 1>,             \
     gemm_f16s_kernel<64, 64, ADD, 17, 1>, gemm_f16s_kernel<64, 64, ADD, 17, 2>, gemm_f16s_kernel<64, 64, ADD, 17, 2, true>},
constexpr TiledKernel kF16sKernels[][kGemmTileCount + 1] = {VLSAT_GEMM_F16S_TILED_VARIANTS(VLSAT_F16S_KERNELS)};
#undef VLSAT_F16S_KERNELS
static_assert(sizeof kF16sKernels / sizeof kF16sKernels[0] == kGemmF16sTiledCount, "one row of kernels per row of the siblings' list");

// ... and their forms on GEMM pair words (PREC 18 / 19 / 20: gemm_f16s_pair_prec), single launches only
#define VLSAT_F16S_PAIR_KERNELS(ADD, PREC)                                                                                            \
    {gemm_f16s_kernel<128, 128, ADD, PREC, 1>, gemm_f16s_kernel<128, 64, ADD, PREC, 1>, gemm_f16s_kernel<64, 128, ADD, PREC, 1>,       \
     gemm_f16s_kernel<64, 64, ADD, PREC, 1>, gemm_f16s_kernel<64, 64, ADD, PREC, 2>},
// (PREC 21 / 22, attention pair words: the row without additive operands only -- gemm_f16s_pair_built)
template <int ADD, int PREC, int BM, int BN, int KSL> constexpr TiledKernel f16s_attn_kernel() {
    if constexpr (gemm_f16s_pair_built(ADD, PREC)) return gemm_f16s_kernel<BM, BN, ADD, PREC, KSL>; else return nullptr;
}
#define VLSAT_F16S_ATTN_KERNELS(ADD, PREC)                                                                                            \
    {f16s_attn_kernel<ADD, PREC, 128, 128, 1>(), f16s_attn_kernel<ADD, PREC, 128, 64, 1>(), f16s_attn_kernel<ADD, PREC, 64, 128, 1>(), \
     f16s_attn_kernel<ADD, PREC, 64, 64, 1>(), f16s_attn_kernel<ADD, PREC, 64, 64, 2>()},
#define VLSAT_F16S_PAIR_ROW(ADD) {VLSAT_F16S_PAIR_KERNELS(ADD, 18) VLSAT_F16S_PAIR_KERNELS(ADD, 19) VLSAT_F16S_PAIR_KERNELS(ADD, 20) \
                                  VLSAT_F16S_ATTN_KERNELS(ADD, 21) VLSAT_F16S_ATTN_KERNELS(ADD, 22)},
constexpr TiledKernel kF16sPairKernels[][5][kGemmTileCount] = {VLSAT_GEMM_F16S_TILED_VARIANTS(VLSAT_F16S_PAIR_ROW)};
#undef VLSAT_F16S_PAIR_ROW
#undef VLSAT_F16S_PAIR_KERNELS
static_assert(sizeof kF16sPairKernels / sizeof kF16sPairKernels[0] == kGemmF16sTiledCount, "one row of kernels per row of the siblings' list");

// the persistent kernel on the plan's tiles; b: the second problem of a pair (grid.y = 2), which launch_gemm_pair has planned
// (GemmArgs::f16s 2 | 3: the split-fp16 sibling of an exact-fp32 row takes the launch as planned -- gemm_f16s_tiled_pick; a pair when both
//  problems ask for it)
static int launch_tiled(const GemmArgs& a, const GemmPlan& p, hipStream_t s, const GemmArgs* b = nullptr) {
    if (p.variant < 0) return fail(-1, gemm_tiled_pick(a, a.relu_a).why);
    const int tile = b ? kGemmTileCount : gemm_tile_index(p.bm, p.bn, p.ksl);
    int fs = gemm_f16s_tiled_pick(a, p.variant).index;
    if (b && gemm_f16s_tiled_pick(*b, p.variant).index != fs) fs = -1;
    // pair words: only the siblings read and write them -- anything else is an error, never another kernel on the wrong format
    const bool pairs = a.a_pair || a.c_pair || (b && (b->a_pair || b->c_pair));
    if (pairs && (fs < 0 || b)) return fail(-1, "gemm: pair words (a_pair / c_pair) on a launch the split-fp16 persistent kernel does not take");
    const TiledKernel k = pairs ? kF16sPairKernels[fs][gemm_f16s_pair_prec(a.a_pair, a.c_pair) - 18][tile]
                          : fs >= 0 ? kF16sKernels[fs][tile] : kTiledKernels[p.variant][tile];
    if (!k) return fail(-1, "gemm: this pair-word form of the split-fp16 persistent kernel is not built");
    hipLaunchKernelGGL(k, dim3(p.grid, b ? 2 : 1), dim3(256), 0, s, a, b ? *b : a, p.n_tiles, (a.N + p.bn - 1) / p.bn);
    if (a.launches) ++*a.launches;         // a logical GEMM is a main launch plus (usually) a small-tile tail launch
    VLSAT_LAUNCH_CHECK((b ? "gemm_f32 (pair)" : "gemm_f32"));
    return 0;
}

// the launch of a plan on rows [0, m.M) (m.M == p.rows)
static int launch_plan(const GemmArgs& m, const GemmPlan& p, hipStream_t s) {
    if ((m.a_pair || m.c_pair) && p.family != GemmPlan::P8 && p.family != GemmPlan::TILED)
        return fail(-1, "gemm: pair words (a_pair / c_pair) on a launch planned onto a kernel without the form");
    if (p.family == GemmPlan::SPLITK) return launch_gemm_splitk(m, p, s);
    if (p.family == GemmPlan::P8) return launch_gemm_p8(m, p, s);
    return p.family == GemmPlan::RING ? launch_gemm_ring(m, p, s) : launch_tiled(m, p, s);
}

static long long* g_clock_probe = nullptr;       // debug only (vlsat_debug_gemm_clock_probe): process-wide on purpose
void gemm_set_clock_probe(long long* buf) { g_clock_probe = buf; }

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

// two problems, one launch (one-scene plans, round 6): which pairs, and as what, is gemm_pair_plan
int launch_gemm_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t s) {
    if (a.a_pair || a.c_pair || b.a_pair || b.c_pair) return fail(-1, "gemm: pair words on a pair of problems");
    const GemmPlan p = gemm_pair_plan(a, b, slots(), g_clock_probe != nullptr);
    if (p.variant < 0) return 1;
    return p.family == GemmPlan::SPLITK ? launch_gemm_splitk(a, p, s, &b) : launch_tiled(a, p, s, &b);
}

}  // namespace vlsat
