// The text of the persistent GEMM kernel (gemm_f32.hip), compiled once per kernel name: gemm_f32.hip defines VLSAT_TILED_NAME
// (gemm_f32_kernel: the rows of VLSAT_GEMM_TILED_VARIANTS; gemm_f16s_kernel: the split-fp16 siblings of its exact-fp32 rows, PREC 17,
// VLSAT_GEMM_F16S_TILED_VARIANTS) and includes this file inside namespace vlsat -- no include guard on purpose.
// PREC 17 (FS): fp32 tensors in and out like PREC 4, the products as three fp16 MFMAs each on the planes Wh16 / Wl16 of the weight
// (PipeSplitDma AFMT 4, gemm_core.h); the accumulator holds the result times 2^w_exp: additive inits enter times 2^w_exp, the epilogue
// multiplies by 2^-w_exp before row scale, bias and activation (powers of two: exact, so the operation order of the exact kernel is kept).
// PREC 21 / 22: C written as ATTENTION pair words (the key | value projection of the edge attention; 22: A read as GEMM pair words).
// PREC 18 / 19 / 20: PREC 17 with C written / A read / both as GEMM pair words (gemm_f16s_planes.h; GemmArgs::c_pair / a_pair) -- the halves
// of the split-fp16 operand, made once by the producer's epilogue instead of by every reader.
// ADD (compile time, so the 64 accumulator-init loads per lane are branch-free and batched):
//   bit 0 = residual, bit 1 = gathered rows g0, bit 2 = gathered rows g1.
// PREC: 0 = exact fp32 (PipeF32), 1 / 3 = bf16 / split-bf16 operands (PipeBF16, gemm_core.h), 4 .. 17 the LDS-direct pipes (PipeSel).
// KSL: k-slices (of 32) moved per pipeline step.  2 for small single-round problems, which are bound
//      by the global-load round trip per step, not by MFMA issue: half the steps, twice the bytes in flight.
// TWIN: two problems of one shape in one launch, selected by blockIdx.y (see gemm_splitk.hip; single-round 64 x 64 launches only).
template <int BM, int BN, int ADD, int PREC, int KSL, bool TWIN = false>
__global__ __launch_bounds__(256, 2) void VLSAT_TILED_NAME(GemmArgs pa, GemmArgs pb, int n_tiles, int nbn) {
    const GemmArgs& p = (TWIN && blockIdx.y != 0) ? pb : pa;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr bool FS = PREC >= 17 && PREC <= 22;      // split-fp16 sibling: acc = result 2^w_exp
    constexpr int CP = PREC == 18 || PREC == 20 ? 1 : PREC >= 21 ? 2 : 0;      // ... that writes C as GEMM (1) / attention (2) pair words (19, 20, 22: reads A as GEMM pair words, PipeSel)
    constexpr bool PLAIN = PREC == 0 || PREC == 4 || FS;      // fp32 tensors, c_scale 1: the format dispatch of tile_init / tile_epilogue folds away
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
            if (ADD != 0 && kt == 0) {
                tile_init<TM, TN, ADD, PLAIN>(p, m0, n0, wm, wn, lane, acc);
                if constexpr (FS) scale_acc<TM, TN>(acc, f16s_pow2(p.w_exp));
            }
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
                if constexpr (FS) scale_acc<TM, TN>(acc, f16s_pow2(-p.w_exp));
                tile_epilogue<TM, TN, PLAIN, CP>(p, m0, n0, BM, BN, wm, wn, lane, acc);
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
