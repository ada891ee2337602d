// The text of the 16-bit edge-attention kernel (flash_attn_bf16.hip includes it once per kernel name; no include guard).  The includer
// defines VLSAT_FLASH_KERNEL_NAME and VLSAT_FLASH_KERNEL_X3:
//   flash_attn_bf16_kernel,  X3 false: the kernels of VLSAT_FLASH_BF16_VARIANTS, each the kernel it was before the split-fp16 form existed
//   flash_attn_f16x3_kernel, X3 true:  the split-fp16 form of the three-term kernel on fp32 tensors (VLSAT_FLASH_F16X3_VARIANTS; the edge
//                            attention of the fp32 precision mode) -- the same LDS image of two 16-bit planes, the same MFMA order (small
//                            terms first), the same softmax, with every operand split as fp16 hi + fp16 lo (split4h: 2^-22 instead of the
//                            bf16 pair's 2^-17) and every product on v_mfma_f32_32x32x16_f16.
// Two names, not an eleventh template argument: the names of the bf16 list's kernels in the library stay what they were.
template <int TERMS, bool TR, int IO, int PVT = 3, int FB_D = 64, int RING = 0, int BQW = 4, int ABL = 0, int QG = 1, int ORD = 0>
__global__ __launch_bounds__(64 * BQW, 2) void VLSAT_FLASH_KERNEL_NAME(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    float* __restrict__ O, int ldq, int ldkv, int ldo, const int4* __restrict__ tiles, int n_tiles,
    float scale_log2e, FlashSplit sp) {
    constexpr bool X3 = VLSAT_FLASH_KERNEL_X3;
    static_assert(!X3 || (TERMS == 3 && (IO == 0 || IO == 4 || IO == 5) && PVT == 3 && RING == 0 && BQW == 4 && ABL == 0 && QG == 1), "split-fp16: the three-term kernel on fp32 tensors or pair words, register-staged");
    // X3, IO 4 / 5 (fp32 mode, "edge_pairs"): K and V arrive as ATTENTION pair words (gemm_f16s_planes.h f16s_attn_pack: hi << 16 | lo of
    // split4h<true>, V already times 2^3 -- written by the key | value projection's epilogue), so staging separates the halves with two byte
    // permutes per plane instead of clamping, converting and subtracting every word once per block of 128 queries; Q stays fp32 (split once
    // per block anyway).  IO 5: O leaves as GEMM pair words for the out-projection (one key part only: split-key partials stay fp32).
    constexpr bool KVP = X3 && IO >= 4, OP = X3 && IO == 5;
    constexpr int IOQ = X3 ? 0 : IO, IOKV = X3 ? (KVP ? 1 : 0) : IO;      // formats load4 / planes_of see (pair words separate like split pairs)
    constexpr int PL = TERMS == 1 ? 1 : 2;
    constexpr int NKS = FB_D / 16, NO = FB_D / 32, NSUB = FB_D / 16;
    constexpr int FB_KPITCH = 2 * FB_D + 16;       // bytes per key row of a K plane (conflict-free ds_read_b128)
    constexpr int FB_KPLANE = FB_KV * FB_KPITCH;
    constexpr int FB_VPLANE = NSUB * FB_VSUB;
    constexpr int FB_OPITCH = FB_D + 4;            // floats per query row of the output transpose
    constexpr bool DMA = RING != 0;           // RING: tile buffers of the LDS-direct K/V ring (0: register-staged double buffer)
    static_assert(!DMA || (TERMS == 1 && IO >= 2 && TR), "LDS-direct K/V staging: half rows, single rounding");
    constexpr bool F16 = IO == 3;                  // IO 3: the half rows hold fp16, QK^T and PV run on the f16 MFMA (precision mode fp16_mixed)
    static_assert(!F16 || (TERMS == 1 && DMA), "fp16 half rows: the LDS-direct single-rounding kernel");
    // X3: the lo part of a value below 2^-3 is a subnormal fp16 (absolute error 2^-25 whatever the value).  For K that is 1e-7 on a score
    // and is left alone.  V is multiplied by VS = 2^3 while staging (exact; the factor leaves with the final 1 / l), which makes the lo parts
    // normal down to |v| = 2^-6 and the domain |V| < 65504 / 2^3 = 8188 (a larger factor buys nothing measurable and costs range: the x4
    // stress weights of the tests reach |V| = 2076); P gets PBIAS = 14 added to its exponent in the subtraction of the running
    // maximum (p <= 2^14: lo normal down to p = 2^-17), a factor the row sum l carries as well, so that it cancels in O / l
    constexpr float VS = X3 ? 8.f : 1.f, VS_INV = 1.f / VS, PBIAS = X3 ? 14.f : 0.f;
    constexpr bool H16 = F16 || X3;                // the operand registers hold fp16: every product on the f16 MFMA
    // (DMA) K image: 64 rows of ROWB = 2 FB_D bytes, unpadded (an LDS-direct load writes lane-linear), 16-byte chunks XOR-swizzled with
    // KSWZ(row) on the global side and on the fragment reads: 64-byte rows (row >> 2) & 3, 128-byte rows (row >> 1) & 7, 256-byte rows row & 15
    constexpr int ROWB = 2 * FB_D, CPR = ROWB / 16, RPI = 1024 / ROWB;          // bytes per K row, chunks per row, rows per load instruction
    static_assert(QG == 1 || (QG == 2 && RING != 0 && FB_D == 64 && (BQW == 2 || BQW == 4)), "two query groups per wave: the LDS-direct variant at head dim 64");
    static_assert(BQW == 4 || (BQW == 8 && RING != 0 && FB_D == 64) || (BQW == 2 && QG == 2), "eight waves: the LDS-direct variant at head dim 64");
    constexpr int KI = FB_KV / RPI / BQW, VI = 2 * NSUB / BQW, LPT = KI + VI;      // load instructions per wave and tile: K, V, both
    constexpr int KBYTES = FB_KV * ROWB;
    constexpr int BUF = DMA ? KBYTES + FB_VPLANE : PL * (FB_KPLANE + FB_VPLANE);
    constexpr int NBUF = DMA ? RING : 2, LA = NBUF - 1;           // (DMA) tiles of look-ahead
    constexpr int SMEM = NBUF * BUF > BQW * QG * 32 * FB_OPITCH * 4 ? NBUF * BUF : BQW * QG * 32 * FB_OPITCH * 4;
    __shared__ __attribute__((aligned(16))) char smem[SMEM];

    const int tile_id = xcd_remap(blockIdx.x, n_tiles);
    const int4 t = tiles[tile_id];
    const int row_base = t.x, n_tok = t.y, q0 = t.z, head = t.w;
    const int n_kv_tiles = (n_tok + FB_KV - 1) / FB_KV;
    // split mode: sp.krange[tile] = {first 32-key tile, end 32-key tile, part, -} (units of 32 keys, see split_keys, plan_graph.h)
    const int4 kr = sp.parts > 1 ? sp.krange[tile_id] : make_int4(0, 2 * n_kv_tiles, 0, 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const size_t col0 = (size_t)head * FB_D;

    const bool wave_active = q0 + wave * QG * 32 < n_tok;     // (QG = 2: a wave whose second group lies past the scene computes it on clamped rows)
    // ---- this lane's query (one per group): d = 16 ks + 8 hi + e, pre-scaled, split into bf16 hi / lo ----
    bf16x8 qhg[QG][NKS], ql[NKS];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        int qrow = q0 + (wave * QG + g) * 32 + li;
        if (qrow >= n_tok) qrow = n_tok - 1;      // clamped rows are computed but never stored
        bf16x8 (&qh)[NKS] = qhg[g];
        const float* qrowp = Q + (size_t)(row_base + qrow) * ldq;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            f32x4 x0 = load4<IOQ>(qrowp, col0 + 8 * hi + 16 * ks), x1 = load4<IOQ>(qrowp, col0 + 8 * hi + 16 * ks + 4);
            if (IOQ == 0) {
                x0 *= scale_log2e;
                x1 *= scale_log2e;
            }
            bf16x4 h0, l0, h1, l1;
            planes_of<IOQ, X3>(x0, h0, l0);
            planes_of<IOQ, X3>(x1, h1, l1);
            qh[ks] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
            ql[ks] = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    }

    f32x16 og[QG][NO];
#pragma unroll
    for (int g = 0; g < QG; ++g)
#pragma unroll
    for (int b = 0; b < NO; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) og[g][b][r] = 0.f;
    float m_rung[QG], l_rung[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) { m_rung[g] = -INFINITY; l_rung[g] = 0.f; }
    // (tried in round 4 and dropped: the row sums of P through the matrix pipe -- one more MFMA per 16 keys with an all-ones A
    //  operand instead of 32 fp32 adds per lane and tile: 735 vs 790 TFLOP/s on the same box, profiles/r04_probes/flash_bf16_dma_ab.txt)

    // ---- staging: K rows (tid>>4) + 16 i, four d per thread; V: wave-instruction = 4 keys x all 64 d, so that a
    //      16-lane write group fills 4 consecutive 32-byte rows of ONE sub-tile (conflict-free ds_write_b64) ----
    //      (FB_D / 4 threads per K row; per thread FB_D / 16 = NKS pieces of K and of V.  V at other head dims: 32 -> a wave
    //      instruction = 8 keys x 32 d (lane groups 0, 1 = sub-tiles of keys 0..3, groups 2, 3 = of keys 4..7); 128 -> two
    //      instructions per 4 keys, sub-tiles 0..3 and 4..7)
    constexpr int TPR = FB_D / 4, RP = 256 / TPR;
    const int krow = tid / TPR, kc4 = (tid % TPR) * 4;
    const int vg = lane >> 4;
    auto vsub_of = [&](int i) { return FB_D == 32 ? (vg & 1) : FB_D == 64 ? vg : vg + 4 * (i & 1); };
    auto vkey_of = [&](int i) {
        return FB_D == 32 ? 8 * wave + 4 * (vg >> 1) + ((lane >> 2) & 3) + 32 * i
             : FB_D == 64 ? 4 * wave + ((lane >> 2) & 3) + 16 * i
                          : 4 * wave + ((lane >> 2) & 3) + 16 * (i >> 1);
    };
    f32x4 rk[NKS], rv[NKS];
    auto load_tile = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < NKS; ++i) {
            int r = kv0 + krow + RP * i;
            r = r < n_tok ? r : n_tok - 1;
            rk[i] = load4<IOKV>(K + (size_t)(row_base + r) * ldkv, col0 + kc4);
            int rv_ = kv0 + vkey_of(i);
            rv_ = rv_ < n_tok ? rv_ : n_tok - 1;
            rv[i] = load4<IOKV>(V + (size_t)(row_base + rv_) * ldkv, col0 + vsub_of(i) * 16 + (lane & 3) * 4);
        }
    };
    auto store_tile = [&](char* buf) {
#pragma unroll
        for (int i = 0; i < NKS; ++i) {
            bf16x4 h, l;
            planes_of<IOKV, X3 && !KVP>(rk[i], h, l);
            char* kp = buf + (krow + RP * i) * FB_KPITCH + kc4 * 2;
            *reinterpret_cast<bf16x4*>(kp) = h;
            if (PL == 2) *reinterpret_cast<bf16x4*>(kp + FB_KPLANE) = l;
            planes_of<IOKV, X3 && !KVP>((X3 && !KVP) ? rv[i] * VS : rv[i], h, l);
            char* vp = buf + PL * FB_KPLANE + vsub_of(i) * FB_VSUB + vkey_of(i) * 32 + (lane & 3) * 8;
            *reinterpret_cast<bf16x4*>(vp) = h;
            if (PL == 2) *reinterpret_cast<bf16x4*>(vp + FB_VPLANE) = l;
        }
    };

    // key range of this block in 64-key tiles (the split table counts 32-key tiles; a part boundary inside a 64-key
    // tile is handled by masking, below)
    const int kt0 = kr.x >> 1, kt1 = (kr.y + 1) >> 1;
    const int key_lo = kr.x * 32, key_hi = kr.y * 32 < n_tok ? kr.y * 32 : n_tok;       // keys [key_lo, key_hi) belong to this block
    // ---- LDS-direct staging (DMA): one tile = LPT loads per wave -- K rows in instructions of RPI rows (a wave takes KI consecutive
    //      ones), V in instructions of 32 keys x 32 B of one [64 keys][16 d] sub-tile (a wave takes VI consecutive halves).  The buffer
    //      descriptors span THIS scene's rows only, so keys past the scene's last token read as zeros (their scores are masked below) ----
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(K + (size_t)row_base * ldkv), 0, DMA ? (int)(unsigned)((size_t)n_tok * ldkv * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V + (size_t)row_base * ldkv), 0, DMA ? (int)(unsigned)((size_t)n_tok * ldkv * 4) : 0, 0x00020000);
    const unsigned ld4 = (unsigned)ldkv * 4u;
    auto kswz_of = [](int row) { return FB_D == 32 ? (row >> 2) & 3 : FB_D == 64 ? (row >> 1) & 7 : row & 15; };
    unsigned vK[4];                                   // (KI <= 4 used; an array bound that depends on the template arguments makes hipcc drop every host stub of this template without a diagnostic)
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        const int row = (wave_u * KI + j) * RPI + lane / CPR;
        vK[j] = (unsigned)row * ld4 + (unsigned)col0 * 2u + (unsigned)(((lane % CPR) ^ kswz_of(row)) << 4);
    }
    const unsigned vV0 = (unsigned)(lane >> 1) * ld4 + (unsigned)col0 * 2u + (unsigned)(lane & 1) * 16u;       // key lane / 2 of a 32-key half, 16-byte half lane & 1
    auto dma_tile = [&](int kv0, char* buf) {
        const unsigned s0 = (unsigned)kv0 * ld4;
#pragma unroll
        for (int j = 0; j < KI; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, buf + (wave_u * KI + j) * 1024, 16, vK[j], s0, 0, 0);
#pragma unroll
        for (int j = 0; j < VI; ++j) {
            const int idx = wave_u * VI + j, sub = idx >> 1, kh = idx & 1;                 // sub-tile, 32-key half of it
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, buf + KBYTES + sub * FB_VSUB + kh * 1024, 16, vV0, s0 + (unsigned)kh * 32u * ld4 + (unsigned)sub * 32u, 0, 0);
        }
    };
    // counted wait: everything but the newest `n` tiles (LPT loads each) has landed
    auto wait_tiles = [&](int n) {
        if (n <= 0) fb_wait_vm<0>();
        else if (n == 1) fb_wait_vm<LPT>();
        else if (n == 2) fb_wait_vm<2 * LPT>();
        else fb_wait_vm<3 * LPT>();
    };
    if (DMA) {
        int issued = 0;
#pragma unroll
        for (int j = 0; j < LA; ++j)
            if (kt0 + j < kt1) { dma_tile((kt0 + j) * FB_KV, smem + j * BUF); ++issued; }
        wait_tiles(issued - 1);
        asm volatile("s_barrier" ::: "memory");
    } else {
        if (kt0 < kt1) {
            load_tile(kt0 * FB_KV);
            store_tile(smem + (kt0 & 1) * BUF);
        }
        __syncthreads();
    }

    // One key tile.  SLOT: the tile's LDS buffer as a compile-time constant where the loop below can provide it (two-buffer
    // configurations: the loop is unrolled by two, so every LDS address of the iteration is lane constant + immediate -- the
    // run-time slot cost ~40 VALU address instructions per tile in a kernel that is VALU-bound, round 5), else -1 = `ring`.
    int ring = 0;                                          // (DMA) buffer of tile kt
    auto tile_step = [&](int kt, auto slotc) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slotc)::value;
        const int buf_i = SLOT >= 0 ? SLOT : (DMA ? ring : (kt & 1));
        const char* sK = smem + buf_i * BUF;
        const char* sV = sK + (DMA ? KBYTES : PL * FB_KPLANE);
        const bool more = kt + 1 < kt1;
        if (DMA) {
            // tile kt + LA goes into the buffer tile kt - 1 was read from: every wave passed the barrier that ended iteration kt - 1
            if (kt + LA < kt1 && !(kExperiments && (sp.ablate & 1))) dma_tile((kt + LA) * FB_KV, smem + (buf_i == 0 ? NBUF - 1 : buf_i - 1) * BUF);
        } else if (more && !(kExperiments && (sp.ablate & 1))) load_tile((kt + 1) * FB_KV);

        if (wave_active) {
            // ---- S^T[key][query] = sum_d K[key][d] * Q[query][d], two blocks of 32 keys (per query group) ----
            f32x16 sg[QG][2];
#pragma unroll
            for (int g = 0; g < QG; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) { sg[g][0][r] = 0.f; sg[g][1][r] = 0.f; }
            {
                // the two 32-key blocks alternate, so consecutive MFMAs never wait for each other's accumulator
                const char* kp = sK + li * FB_KPITCH + 16 * hi;
                const char* kd = sK + li * ROWB;                      // (DMA) row li; rows li and li + 32 share the swizzle
                const int kswz = kswz_of(li);
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bf16x8 kh0 = *reinterpret_cast<const bf16x8*>(DMA ? kd + (((hi + 2 * ks) ^ kswz) << 4) : kp + 32 * ks);
                    const bf16x8 kh1 = *reinterpret_cast<const bf16x8*>(DMA ? kd + 32 * ROWB + (((hi + 2 * ks) ^ kswz) << 4) : kp + 32 * FB_KPITCH + 32 * ks);
                    if (PL == 2) {
                        const bf16x8 kl0 = *reinterpret_cast<const bf16x8*>(kp + FB_KPLANE + 32 * ks);
                        const bf16x8 kl1 = *reinterpret_cast<const bf16x8*>(kp + FB_KPLANE + 32 * FB_KPITCH + 32 * ks);
                        sg[0][0] = mfma_h<H16>(kl0, qhg[0][ks], sg[0][0]);
                        sg[0][1] = mfma_h<H16>(kl1, qhg[0][ks], sg[0][1]);
                        sg[0][0] = mfma_h<H16>(kh0, ql[ks], sg[0][0]);
                        sg[0][1] = mfma_h<H16>(kh1, ql[ks], sg[0][1]);
                    }
                    if ((ABL & 64)) {           // no QK MFMAs (the fragments stay read)
                        asm volatile("" :: "v"(kh0), "v"(kh1));
                        continue;
                    }
#pragma unroll
                    for (int g = 0; g < QG; ++g) {
                        sg[g][0] = mfma_h<H16>(kh0, qhg[g][ks], sg[g][0]);
                        sg[g][1] = mfma_h<H16>(kh1, qhg[g][ks], sg[g][1]);
                    }
                }
            }
            // The first readers of the score registers below are inline-asm VALU instructions, which hipcc's hazard recogniser
            // does not see: the wait states between an MFMA's register write and a VALU read of it (19 for a 16-pass MFMA; the
            // hardware has no interlock there) are inserted by hand.  The asm names the accumulators, so it cannot move above the
            // MFMAs, and everything that reads them is ordered behind it.  (Found by the kernel tests: without it the maxima were
            // taken from stale registers.)
            if (QG == 2) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(sg[0][0]), "+v"(sg[0][1]), "+v"(sg[QG - 1][0]), "+v"(sg[QG - 1][1]));
            else asm volatile("s_nop 15\n\ts_nop 3" : "+v"(sg[0][0]), "+v"(sg[0][1]));
            const int kv0 = kt * FB_KV;
            // ---- online softmax for this lane's query ----
            // The kernel is bound by VALU issue at head dim 64 (round 4 PMC: matrix pipe 35 % busy; per tile and wave 512 MFMA cycles
            // against ~1100 of VALU), so the softmax is written for instruction count (round 5): the maximum of the 32 scores with
            // v_max3_f32 (two new values per instruction; fmaxf costs a canonicalising v_max per MFMA result on top of the max itself:
            // 54 -> 16 instructions), score - m and the row sum as packed fp32 pairs (v_pk_add_f32: 33 + 33 -> 16 + 16); the 32
            // quarter-rate v_exp_f32 stay.
            auto softmax_group = [&](f32x16 (&s)[2], f32x16 (&o)[NO], float& m_run, float& l_run) __attribute__((always_inline)) {
            // keys outside [key_lo, key_hi): beyond the scene's tokens (last tile) or another part's (split mode)
            if (kv0 < key_lo || kv0 + FB_KV > key_hi) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kv0 + 32 * kb + crow32(r, hi);
                        if (key < key_lo || key >= key_hi) s[kb][r] = -INFINITY;
                    }
            }
            float mx;
            {
                float ma = max3f(s[0][0], s[0][1], s[0][2]), mb = max3f(s[1][0], s[1][1], s[1][2]);    // two chains: no max waits for its predecessor
#pragma unroll
                for (int r = 3; r < 15; r += 2) { ma = max3f(ma, s[0][r], s[0][r + 1]); mb = max3f(mb, s[1][r], s[1][r + 1]); }
                mx = max3f(ma, mb, s[0][15]);
                mx = max3f(mx, s[1][15], s[1][15]);
            }
            if (!((ABL & 16))) { float ha, hb; half_swap(mx, ha, hb); mx = max3f(ha, hb, hb); }       // (ablate 16: no cross-half exchanges)
            if ((ABL & 8)) mx = 0.f;                                        // (ablate 8: no maximum at all)
            const float m_new = max3f(m_run, mx, mx);
            // (a part whose first tile is fully masked for this query keeps m = -inf; exp2(-inf - -inf) must not be NaN)
            const float m_use = m_new == -INFINITY ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
            const float m_sub = X3 ? m_use - PBIAS : m_use;                 // (X3: one more rounding of the order of the subtraction's own)
            f32x2 rs2 = {0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    f32x2 x = pk_sub(f32x2{s[kb][r], s[kb][r + 1]}, m_sub);
                    if (!((ABL & 4))) {                                      // (ablate 4: no exponentials)
                        x[0] = __builtin_amdgcn_exp2f(x[0]);
                        x[1] = __builtin_amdgcn_exp2f(x[1]);
                    }
                    rs2 = pk_add(rs2, x);
                    s[kb][r] = x[0];
                    s[kb][r + 1] = x[1];
                }
            float rs = rs2[0] + rs2[1];
            if (!((ABL & 16))) rs = half_sum(rs);
            l_run = l_run * alpha + rs;
            m_run = m_new;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
                for (int b = 0; b < NO; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
            }
            };
            // ---- O^T[d][query] += sum_key V[key][d] * P[key][query]: groups [G0, G1) share every V fragment ----
            auto pv_groups = [&](auto g0c, auto g1c) __attribute__((always_inline)) {
            constexpr int G0 = decltype(g0c)::value, G1 = decltype(g1c)::value;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kb = j >> 1, half = j & 1;
                bf16x8 phg[QG], pl;
#pragma unroll
                for (int g = G0; g < G1; ++g) {
                f32x4 p0, p1;
#pragma unroll
                for (int c = 0; c < 4; ++c) { p0[c] = sg[g][kb][8 * half + c]; p1[c] = sg[g][kb][8 * half + 4 + c]; }
                bf16x4 h0, l0, h1, l1;
                if constexpr (F16) {              // probabilities in [0, 1]: fp16, no clamp needed
                    typedef _Float16 f16x4_p __attribute__((ext_vector_type(4)));
                    h0 = l0 = __builtin_bit_cast(bf16x4, __builtin_convertvector(p0, f16x4_p));
                    h1 = l1 = __builtin_bit_cast(bf16x4, __builtin_convertvector(p1, f16x4_p));
                } else if constexpr (X3) {
                    split4h<false>(p0, h0, l0);
                    split4h<false>(p1, h1, l1);
                } else {
                    split4(p0, h0, l0);
                    split4(p1, h1, l1);
                }
                phg[g] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
                pl = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
                const bf16x8 ph = phg[G0];
                f32x16 (&o)[NO] = og[G0];
                const int k0 = 32 * kb + 16 * half + 4 * hi;          // first key of this lane half's k-slots (then +8)
                bf16x8 vf[NO][PL];
#pragma unroll
                for (int db = 0; db < NO; ++db)
#pragma unroll
                    for (int pln = 0; pln < PL; ++pln) {
                        const char* vb = sV + pln * FB_VPLANE + (2 * db + ((lane >> 4) & 1)) * FB_VSUB;
                        if (TR) {
                            const char* a = vb + (k0 + ((lane & 15) >> 2)) * 32 + (lane & 3) * 8;
                            const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (s16x4 __attribute__((address_space(3)))*)(a));
                            const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (s16x4 __attribute__((address_space(3)))*)(a + 8 * 32));
                            const bf16x4 b0 = __builtin_bit_cast(bf16x4, x0), b1 = __builtin_bit_cast(bf16x4, x1);
                            vf[db][pln] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
                        } else {
                            const unsigned short* g = reinterpret_cast<const unsigned short*>(vb) + (lane & 15);
                            typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
                            u16x8 u;
#pragma unroll
                            for (int e = 0; e < 8; ++e) u[e] = g[(k0 + 8 * (e >> 2) + (e & 3)) * 16];
                            vf[db][pln] = __builtin_bit_cast(bf16x8, u);
                        }
                    }
                // the d-blocks alternate (independent accumulators back to back)
                if (PL == 2) {
#pragma unroll
                    for (int db = 0; db < NO; ++db) o[db] = mfma_h<H16>(vf[db][PL - 1], ph, o[db]);
                    if (PVT == 3) {
#pragma unroll
                        for (int db = 0; db < NO; ++db) o[db] = mfma_h<H16>(vf[db][0], pl, o[db]);
                    }
                }
                if ((ABL & 32)) {               // no PV MFMAs (P converted, V fragments read)
                    asm volatile("" :: "v"(ph), "v"(vf[0][0]), "v"(vf[NO - 1][0]));
                    continue;
                }
#pragma unroll
                for (int g = G0; g < G1; ++g)
#pragma unroll
                for (int db = 0; db < NO; ++db) og[g][db] = mfma_h<H16>(vf[db][0], phg[g], og[g][db]);
            }
            };
            typedef std::integral_constant<int, 0> I0;
            typedef std::integral_constant<int, 1> I1;
            typedef std::integral_constant<int, QG> IQ;
            if constexpr (QG == 2 && ORD == 1) {
                softmax_group(sg[0], og[0], m_rung[0], l_rung[0]);
                pv_groups(I0{}, I1{});
                softmax_group(sg[QG - 1], og[QG - 1], m_rung[QG - 1], l_rung[QG - 1]);
                pv_groups(I1{}, IQ{});
            } else {
#pragma unroll
                for (int g = 0; g < QG; ++g) softmax_group(sg[g], og[g], m_rung[g], l_rung[g]);
                pv_groups(I0{}, IQ{});
            }
        }   // wave_active
        if (DMA) {
            // tile kt + 1 has landed once only the tiles issued after it (kt + 2 .. kt + LA, as far as they exist) are outstanding
            wait_tiles((kExperiments && (sp.ablate & 1)) ? 0 : min(LA - 1, kt1 - kt - 2));
            if ((ABL & 256)) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (ablate 256: no barrier per tile)
            else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            ring = ring == NBUF - 1 ? 0 : ring + 1;
        } else {
            if (more && !(kExperiments && (sp.ablate & 2))) store_tile(smem + ((kt + 1) & 1) * BUF);
            __syncthreads();
        }
    };
    if (DMA && NBUF == 2) {                                 // the first tile of the range sits in buffer 0
        for (int kt = kt0; kt < kt1; kt += 2) {
            tile_step(kt, std::integral_constant<int, 0>{});
            if (kt + 1 < kt1) tile_step(kt + 1, std::integral_constant<int, 1>{});
        }
    } else {
        for (int kt = kt0; kt < kt1; ++kt) tile_step(kt, std::integral_constant<int, -1>{});
    }

    // ---- normalise (or, in split mode, keep un-normalised and record m, l), transpose through LDS
    //      (wave-private [32 q][68]), coalesced store ----
    const bool split = sp.parts > 1;
    if (split) O = sp.o_part + (size_t)kr.z * sp.part_stride;
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const float m_run = m_rung[g], l_run = l_rung[g];
        const float inv_l = X3 ? (split ? 1.f : 1.f / l_run) * VS_INV : (split ? 1.f : 1.f / l_run);
        if (split) {
            const int qr = q0 + (wave * QG + g) * 32 + li;
            if (hi == 0 && qr < n_tok) {
                const size_t i = ((size_t)kr.z * sp.rows + row_base + qr) * sp.heads + head;
                sp.m_part[i] = m_run;
                sp.l_part[i] = l_run;
            }
        }
        float* so = reinterpret_cast<float*>(smem) + (wave * QG + g) * (32 * FB_OPITCH);
#pragma unroll
        for (int b = 0; b < NO; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = og[g][b][r] * inv_l;
                so[li * FB_OPITCH + 32 * b + crow32(r, hi)] = (IO == 1 && !split) ? pack_split(a) : a;   // (split-key partials stay fp32: the merge packs)
            }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < QG; ++g) {
    const float* so = reinterpret_cast<const float*>(smem) + (wave * QG + g) * (32 * FB_OPITCH);
#pragma unroll
    for (int i = 0; i < FB_D / 8; ++i) {
        const int idx = lane + 64 * i;             // 8 FB_D float4 = 32 rows x FB_D / 4
        const int r = idx / (FB_D / 4), c4 = (idx % (FB_D / 4)) * 4;
        const int qr = q0 + (wave * QG + g) * 32 + r;
        if (qr < n_tok) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(so + r * FB_OPITCH + c4);
            float* orow = O + (size_t)(row_base + qr) * ldo;
            if (IO == 3 && !split) {
                typedef _Float16 f16x4_o __attribute__((ext_vector_type(4)));
                f32x4 vc;
#pragma unroll
                for (int c = 0; c < 4; ++c) vc[c] = __builtin_amdgcn_fmed3f(v[c], -65504.f, 65504.f);
                *reinterpret_cast<f16x4_o*>(reinterpret_cast<char*>(orow) + (col0 + c4) * 2) = __builtin_convertvector(vc, f16x4_o);
            } else if (IO == 2 && !split)
                *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(orow) + (col0 + c4) * 2) = __builtin_convertvector(v, bf16x4);
            else if (OP && !split) {        // GEMM pair words: the out-projection's A operand, split here once (f16s_pack2)
                typedef unsigned u32x4_o __attribute__((ext_vector_type(4)));
                u32x4_o w;
#pragma unroll
                for (int c = 0; c < 4; c += 2) {
                    unsigned w0, w1;
                    f16s_pack2(v[c], v[c + 1], w0, w1);
                    w[c] = w0;
                    w[c + 1] = w1;
                }
                *reinterpret_cast<u32x4_o*>(orow + col0 + c4) = w;
            } else
                *reinterpret_cast<f32x4*>(orow + col0 + c4) = v;
        }
    }
    }
}
