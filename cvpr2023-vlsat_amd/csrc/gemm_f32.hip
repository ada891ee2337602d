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

// ADD (compile time, so the 64 accumulator-init loads per lane are branch-free and batched):
//   bit 0 = residual, bit 1 = gathered rows g0, bit 2 = gathered rows g1.
// PREC: 0 = exact fp32 (PipeF32), 1 / 3 = bf16 / split-bf16 operands (PipeBF16, gemm_core.h).
// KSL: k-slices (of 32) moved per pipeline step.  2 for small single-round problems, which are bound
//      by the global-load round trip per step, not by MFMA issue: half the steps, twice the bytes in flight.
// TWIN: two problems of one shape in one launch, selected by blockIdx.y (see gemm_splitk.hip; single-round 64 x 64 launches only).
template <int BM, int BN, int ADD, int PREC, int KSL, bool TWIN = false>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(GemmArgs pa, GemmArgs pb, int n_tiles, int nbn) {
    const GemmArgs& p = (TWIN && blockIdx.y != 0) ? pb : pa;
    constexpr int TM = BM / 64, TN = BN / 64;
    using Pipe = typename PipeSel<BM, BN, PREC>::type;
    constexpr int SLICE = Pipe::STAGE_BYTES;
    constexpr int STAGE = SLICE * KSL;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int g8 = gridDim.x >> 3, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int KT = p.K / (BK * KSL);
    // (an experiment that started each row panel's k loop at a different slice, against L2 channel camping, measured no
    //  gain in any mode and cost the fp32 kernel 2 %: removed)
    auto kslice = [&](int, int kt) { return kt * (BK * KSL); };

    int round = 0;
    int v = xcd * g8 + slot;                 // tile of round r: (r*8 + xcd)*g8 + slot
    if (v >= n_tiles) return;
    const long long t_start = p.clock_probe ? clock64() : 0, w_start = p.clock_probe ? wall_clock64() : 0;
    int m0 = (v / nbn) * BM, n0 = (v % nbn) * BN;

    f32x16 acc[TM][TN];
    zero_acc<TM, TN>(acc);
    typename Pipe::Regs regs[KSL];
    const typename Pipe::Ctx ctx(p, tid);

#pragma unroll
    for (int ks = 0; ks < KSL; ++ks) Pipe::load(ctx, p, m0, n0, kslice(m0, 0) + ks * BK, regs[ks], tid, smem + ks * SLICE);
#pragma unroll
    for (int ks = 0; ks < KSL; ++ks) Pipe::store(smem + ks * SLICE, regs[ks], tid, p.relu_a);
    __syncthreads();

    // A-panel prefetch of the bf16 LDS-direct pipe (Pipe::PREFETCH): thread -> (line of the stage, part of the line)
    constexpr int PF_TPL = 256 / (BM * KSL) > 0 ? 256 / (BM * KSL) : 1;          // threads per 128-byte line
    const int pf_row = (tid / PF_TPL) % BM, pf_col = ((tid / PF_TPL) / BM) * BK + (tid % PF_TPL) * (32 / PF_TPL);
    const int pf_dist = Pipe::PREFETCH ? (p.prefetch < 0 ? 6 : p.prefetch) : 0;
    float pf_sink = 0.f;                     // destination of every prefetch touch: lives in one register for the whole kernel

    int buf = 0;
    while (true) {
        const int nv = ((round + 1) * 8 + xcd) * g8 + slot;
        const bool next_tile = nv < n_tiles;
        const int nm0 = (nv / nbn) * BM, nn0 = (nv % nbn) * BN;
        for (int kt = 0; kt < KT; ++kt) {
            char* cur = smem + buf * STAGE;
            char* nxt = smem + (buf ^ 1) * STAGE;
            const bool last = kt == KT - 1;
            const bool more = !last || next_tile;
            if (more) {
                const int lm0 = last ? nm0 : m0, ln0 = last ? nn0 : n0, lk = last ? kslice(nm0, 0) : kslice(m0, kt + 1);
#pragma unroll
                for (int ks = 0; ks < KSL; ++ks) Pipe::load(ctx, p, lm0, ln0, lk + ks * BK, regs[ks], tid, nxt + ks * SLICE);
            }
            bool touched = false;
            if (Pipe::PREFETCH && pf_dist > 0) {
                // slice kt + 1 + pf_dist of this block's (tile, k) sequence; it may belong to the next tile
                const int j = kt + 1 + pf_dist;
                const bool same = j < KT;
                if (same || next_tile) {
                    int jj = same ? j : j - KT;
                    jj = jj < KT ? jj : KT - 1;
                    int row = (same ? m0 : nm0) + pf_row;
                    row = row < p.M ? row : p.M - 1;
                    const float* src = p.A + (size_t)row * p.lda + kslice(same ? m0 : nm0, jj) + pf_col;
                    // hidden from hipcc's wait counting on purpose (it would drain it at the next barrier); the register is
                    // tied ("+v") so nothing else is ever allocated to it while a touch is in flight
                    asm volatile("global_load_dword %0, %1, off" : "+v"(pf_sink) : "v"(src) : "memory");
                    touched = true;
                }
            }
            // additive epilogue operands (residual / gathered rows) are loaded straight into the accumulators at the start
            // of a tile (C-in of the first MFMA): no extra registers, and the wait overlaps the co-resident block's MFMAs
            if (ADD != 0 && kt == 0) tile_init<TM, TN, ADD, (PREC == 0 || PREC == 4)>(p, m0, n0, wm, wn, lane, acc);
#pragma unroll
            for (int ks = 0; ks < KSL; ++ks) Pipe::mma(cur + ks * SLICE, wm, wn, acc, lane, p.relu_a);
            if constexpr (Pipe::PREFETCH) {
                // counted wait + raw barrier: __syncthreads() would make hipcc drain every outstanding load, the touch included
                if (touched) Pipe::store_keep1();
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            } else {
                if (more) {
#pragma unroll
                    for (int ks = 0; ks < KSL; ++ks) Pipe::store(nxt + ks * SLICE, regs[ks], tid, p.relu_a);
                }
                __syncthreads();
            }
            if (last) {
                tile_epilogue<TM, TN, (PREC == 0 || PREC == 4)>(p, m0, n0, BM, BN, wm, wn, lane, acc);
                zero_acc<TM, TN>(acc);
            }
            buf ^= 1;
        }
        if (!next_tile) {
            if (p.clock_probe && tid == 0) {       // DVFS probe: shader cycles (s_memtime) vs 100 MHz wall clock per block
                long long* d = p.clock_probe + (size_t)blockIdx.x * 4;
                unsigned hw_id, xcc_id;                       // where the block ran: HW_ID (wave/simd/cu/sh/se), XCC_ID
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
                d[0] = clock64() - t_start; d[1] = wall_clock64() - w_start;
                d[2] = (round + 1) | ((long long)(hw_id & 0xffffu) << 16) | ((long long)(xcc_id & 0xfu) << 32); d[3] = 1;
            }
            break;
        }
        ++round;
        m0 = nm0;
        n0 = nn0;
    }
    if (Pipe::PREFETCH) {                    // no touch may outlive its register
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" ::"v"(pf_sink));
    }
}

double gemm_flops(const GemmArgs& a) { return 2.0 * a.M * (double)a.N * a.K; }

// resident 256-thread blocks the persistent grid may use (2 per CU): a constant of the device, cached per device id
static int slots() {
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

// the persistent kernel on the plan's tiles; b: the second problem of a pair (grid.y = 2), which launch_gemm_pair has planned
static int launch_tiled(const GemmArgs& a, const GemmPlan& p, hipStream_t s, const GemmArgs* b = nullptr) {
    if (p.variant < 0) return fail(-1, gemm_tiled_pick(a, a.relu_a).why);
    const TiledKernel k = kTiledKernels[p.variant][b ? kGemmTileCount : gemm_tile_index(p.bm, p.bn, p.ksl)];
    hipLaunchKernelGGL(k, dim3(p.grid, b ? 2 : 1), dim3(256), 0, s, a, b ? *b : a, p.n_tiles, (a.N + p.bn - 1) / p.bn);
    if (a.launches) ++*a.launches;         // a logical GEMM is a main launch plus (usually) a small-tile tail launch
    VLSAT_LAUNCH_CHECK((b ? "gemm_f32 (pair)" : "gemm_f32"));
    return 0;
}

// the launch of a plan on rows [0, m.M) (m.M == p.rows)
static int launch_plan(const GemmArgs& m, const GemmPlan& p, hipStream_t s) {
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
    const GemmPlan p = gemm_pair_plan(a, b, slots(), g_clock_probe != nullptr);
    if (p.variant < 0) return 1;
    return p.family == GemmPlan::SPLITK ? launch_gemm_splitk(a, p, s, &b) : launch_tiled(a, p, s, &b);
}

}  // namespace vlsat
