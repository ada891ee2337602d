// The text of the 8-phase GEMM kernel (gemm_bf16_p8.hip), compiled once per kernel name: gemm_bf16_p8.hip defines VLSAT_P8_NAME and
// VLSAT_P8_FS (false: gemm_p8_kernel, the rows of VLSAT_GEMM_P8_VARIANTS; true: gemm_p8s_kernel, the split-fp16 form FS below) and includes
// this file inside namespace vlsat { namespace { -- no include guard on purpose.
// CF: storage format of C (0 fp32, 2 half rows of bf16, 3 half rows of FP16 clamped to +-65504 -- the out-projection of the single-rounded edge
// attention, whose only reader is the LayerNorm: round 6).  ABL (timing experiments, results are garbage): bit 0 no LDS-direct
// loads after the prologue, bit 1 no MFMAs, bit 2 no fragment reads, bit 3 no epilogue stores
// F32: exact-fp32 operands (A fp32 rows, W fp32 [N,K], v_mfma_f32_32x32x2_f32, K-tiles of 32): the same LDS image -- 128-byte
// rows, a lane's fragment is the 16-byte chunk 2 ks + hi = four consecutive k (gemm_core.h, K-permutation trick) -- so
// loader, phases, waits and epilogue are shared; a phase is 32 MFMAs of 64 cycles there.  Bias then joins after the
// transposition (8 registers per lane; same fp32 operation order as gemm_f32.hip: bit-identical results).
// MODE 2 (X3): split-bf16, three MFMAs per product.  A = split-pair words (bf16 hi | lo in one 32-bit word, common.h), the
// same 128-byte rows as fp32 (K-tiles of 32), separated with v_perm on the fragment side; a weight half-tile is the hi and
// the lo plane side by side, 128 rows x 64 bytes each (chunks swizzled with (row >> 2) & 3), one LDS-direct load per plane
// -- so a half-tile is still two loads and every counted wait is unchanged.  Term order per accumulator and epilogue order
// as in the older split-bf16 kernels: bit-identical results.
// (round 6, measured and dropped: the g0 rows of a gathered-row tile DEDUPLICATED per 32-row strip -- source-major edge lists name
//  one or two g0 rows per strip; each distinct 256-byte segment fetched once by 16 lanes into the wave's idle transposition
//  buffer, every lane reading its run's values from LDS, bit-identical results -- 213.6 / 218.5 us against 209.5 / 210.6 us for the
//  per-lane gather on the bench batch's indices, 9852-9867 vs 9839-9880 scenes/s per step: the repeated g0 lines were L1 hits
//  already, what the launch pays for is the L2 -> CU traffic of the DISTINCT lines, which the deduplication does not change.
//  profiles/r06_probes/p8_dedup_krot_{kernel,step}_ab.txt)
// FS (the body of gemm_p8s_kernel, below; MODE 2, CF 0): the split-fp16 form of MODE 2 for the fp32 precision mode -- fp32 tensors in and
// out, fp32-grade results on the 16-bit matrix pipe.  The LDS image, K-tiles of 32, loader, phases and counted waits are MODE 2's; the
// differences:
//   * A words are plain fp32.  A fragment is split ONCE, in the phase that read it (a0: phase 1, a1: phase 3), in place -- the 32
//     registers of the fp32 words then hold  Ah = f16(x)  and  Al = f16((x - Ah) 2^11),  x = the word after the optional ReLU-on-A clamped
//     to +-65504 (one v_med3: ReLU is its lower bound).  Times 2^11 the lo part is a normal fp16 number for every |x| >= 2^-13.
//   * the weight planes are fp16: Wh = f16(W 2^k), Wl = f16(W 2^k - Wh), k = GemmArgs::w_exp per weight tensor (gemm_f16s_planes.h) --
//     unscaled, the lo part of a weight of 0.05 is a subnormal fp16.  A third operand Wh 2^-11 (exact: |Wh| >= 2^-3 or zero) is made from
//     the Wh fragment by packed fp16 multiplies.
//   * three v_mfma_f32_32x32x16_f16 per product into one fp32 accumulator, small terms first: (Wh 2^-11).Al, Wl.Ah, Wh.Ah.
//   * additive accumulator inits enter times 2^k; the epilogue multiplies by 2^-k before bias and activation.  Powers of two: exact,
//     so the operation order of the exact-fp32 path is otherwise kept.
//   * pair words (CF = PF of VLSAT_GEMM_P8S_PAIR_VARIANTS; GemmArgs::a_pair / c_pair, gemm_f16s_planes.h): bit 2 -- A holds Ah << 16 | Al, stored
//     by the kernel that wrote the tensor, and the fresh phases separate the halves with byte permutes (f16s_unpack8: one VALU operation per
//     word instead of 3.5; a pending ReLU is a signed max on the word) -- bit 0: the epilogue stores such words (f16s_pack2, after 2^-k, bias
//     and activation); bit 1: the epilogue stores ATTENTION pair words (f16s_attn_pack2: the key | value projection, whose reader is the
//     split-fp16 edge attention).  The MFMA operands are bit for bit those of the fp32 form.
// Domain: |A| <= 65504 (beyond: the operand saturates, results stay finite); weights below 2^-16 of their tensor's maximum lose low bits.
template <int MODE, int ADD, bool RELU, int CF, int ABL = 0>
__global__ __launch_bounds__(512, 2) void VLSAT_P8_NAME(GemmArgs p, int n_tiles, int nbn) {
    constexpr bool FS = VLSAT_P8_FS;
    constexpr bool F32 = MODE == 1, X3 = MODE == 2, H16 = MODE == 3, WORDS = F32 || X3;      // WORDS: 4-byte A elements, K-tiles of 32; H16: MODE 0 on fp16 (GemmArgs::half_f16)
    static_assert(MODE == 3 ? (CF == 0 || CF == 3) : MODE == 0 ? (CF == 0 || CF == 2 || CF == 3) : F32 ? CF == 0 : (CF == 0 || CF == 1 || (FS && (CF == 2 || CF == 4 || CF == 5 || CF == 6))), "output format of the mode");
    static_assert(!FS || (X3 && ABL == 0), "the split-fp16 form is MODE 2 on fp32 tensors or pair words");
    constexpr bool AP = FS && (CF & 4) != 0, CP = FS && (CF & 1) != 0;      // split-fp16 form: A read / C written as GEMM pair words
    constexpr bool CPA = FS && (CF & 2) != 0;                                // ... C written as ATTENTION pair words (the K | V projection)
    __shared__ __attribute__((aligned(16))) char smem[10 * P8_HALF];
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr bool SPREAD = ADD == 0;             // epilogue strips 2 / 3 inside the next tile's first K-tile
    // (ABL bits 8, 9, gathered-row launches: 256 = the init loads in a row-contiguous lane pattern, 512 = no init loads)
    constexpr bool HALF = !FS && (CF == 2 || CF == 3);                // two bytes per element of C
    constexpr int E = HALF ? 4 : 8;            // buffer stores per epilogue strip and lane

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int li = lane & 31, hi = lane >> 5;
    const int g8 = gridDim.x >> 3, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int KT = p.K / (WORDS ? 32 : P8_BK);         // K-tiles of 128 bytes per A row
    auto tile_of_round = [&](int r) { return (r * 8 + xcd) * g8 + slot; };
    if (tile_of_round(0) >= n_tiles) return;

    // ---- LDS-direct loader: lane constants (a wave instruction fills 8 rows x 128 bytes) ----
    const int srow = wave * 8 + (lane >> 3);                                   // LDS row inside a 64-row round
    const unsigned schunk = (unsigned)((lane & 7) ^ ((srow >> 1) & 7));          // logical chunk this lane fetches
    constexpr unsigned EA = WORDS ? 4u : 2u, EW = F32 ? 4u : 2u;              // bytes per A / W element
    constexpr unsigned KA = 128u, KW = X3 ? 64u : 128u;                        // bytes of a K-tile in an A / W row
    const unsigned lda4 = (unsigned)p.lda * 4u, ldw2 = (unsigned)p.ldw * EW;     // row pitches in bytes (half rows keep the fp32 pitch)
    const unsigned vA = (unsigned)srow * lda4 + schunk * 16u;
    // weight rows: 128-byte K-tiles like A (8 rows per wave instruction), or -- X3 -- 64-byte ones (16 rows, one plane)
    const int wrow3 = wave * 16 + (lane >> 2);                                  // X3: LDS row of the half-tile's plane
    const unsigned vW = X3 ? (unsigned)((wrow3 >> 5) * 64 + (wrow3 & 31)) * ldw2 + (unsigned)((lane & 3) ^ ((wrow3 >> 2) & 3)) * 16u
                           : (unsigned)((wave >> 2) * 64 + (wave & 3) * 8 + (lane >> 3)) * ldw2 + schunk * 16u;
    const int na = (int)((size_t)(p.M - 1) * lda4 + (size_t)p.K * EA), nw = (int)(((size_t)(p.N - 1) * p.ldw + p.K) * EW);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, na, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(F32 ? (void*)const_cast<float*>(p.W) : (void*)const_cast<uint16_t*>(FS ? p.Wh16 : p.Whi), 0, nw, 0x00020000);
    const __amdgpu_buffer_rsrc_t rwl = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(FS ? p.Wl16 : X3 ? p.Wlo : p.Whi), 0, nw, 0x00020000);
    char* const sdst = smem + wave * 1024;
    // two wave instructions = one half-tile: rows 0..63 and 64..127 of it
    auto ld2 = [&](const __amdgpu_buffer_rsrc_t& r, char* dst, unsigned v, unsigned s0, unsigned step) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 16, v, s0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst + 8192, 16, v, s0 + step, 0, 0);
    };
    // weight half-tile h at byte offset sw (K-tile included): two 64-row rounds of one plane, or (X3) the two planes
    auto ldw = [&](char* dst, unsigned sw, int h) {
        const unsigned s0 = sw + (unsigned)(h * 32) * ldw2;
        if (X3) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, dst, 16, vW, s0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rwl, dst + 8192, 16, vW, s0, 0, 0);
        } else {
            ld2(rw, dst, vW, s0, 128u * ldw2);
        }
    };
    // half-tile h of the K-tile at byte offsets (sa, sw) into buffer `buf`
    auto stage_a = [&](int buf, int h, unsigned sa) {
        if (!(ABL & 1)) ld2(ra, sdst + (buf * 2 + h) * P8_HALF, vA, sa + (unsigned)(h * 64) * lda4, 128u * lda4);
    };
    auto stage_w = [&](int buf, int h, unsigned sw) {
        if (!(ABL & 1)) ldw(sdst + P8_WBASE + (buf * 2 + h) * P8_HALF, sw, h);
    };

    // ---- staging cursor: the K-tile sequence of this block, across output tiles ----
    // (past the block's last tile the cursor stays on it: the loads keep their rhythm, so every wait is a counted one and
    //  the K loop has no branch; what they fetch is never read)
    struct Cur { int r, kt; unsigned sa, sw; };
    auto locate = [&](Cur& c) {
        const int v = tile_of_round(c.r);
        if (v >= n_tiles) return;
        const int tm = v / nbn, tn = v - tm * nbn;
        c.sa = (unsigned)(tm * P8_BM) * lda4;
        c.sw = (unsigned)(tn * P8_BN) * ldw2;
    };
    auto advance = [&](Cur& c) {
        if (++c.kt == KT) { c.kt = 0; ++c.r; locate(c); }
    };
    // (A/B, GemmArgs::k_rot) column tile tn of a row panel walks its K-tiles starting at tn * k_rot: the blocks that share an A panel
    //  (neighbouring slots of one XCD) then ask L2 for the same lines a K-tile or more apart instead of in the same microsecond
    const int rot = p.k_rot ? ((tile_of_round(0) % nbn) * p.k_rot) % KT : 0;
    auto kti = [&](const Cur& c) { const int j = c.kt + rot; return (unsigned)(j >= KT ? j - KT : j); };
    Cur c1{0, 0, 0u, 0u};
    locate(c1);
    const Cur c0 = c1;
    advance(c1);
    Cur c2 = c1;
    advance(c2);

    // ---- fragment readers: per-lane byte offsets of k-step ks (the chunk XOR is not an add: one register per k-step) ----
    // (X3: fragment i of an A tile is chunk 4 (i >> 1) + 2 hi + (i & 1) -- eight words of k-step i >> 1 in two reads; weight
    //  fragment i is chunk 2 (i & 1) + hi of the 64-byte row of plane i >> 1)
    const int swz = (li >> 1) & 7;
    int offA[4], offW[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const int ca = X3 ? (((ks >> 1) << 2) | (hi << 1) | (ks & 1)) : 2 * ks + hi;
        offA[ks] = (wr * 64 + li) * 128 + ((ca ^ swz) * 16);
        offW[ks] = X3 ? P8_WBASE + (ks >> 1) * 8192 + (wc * 32 + li) * 64 + (((2 * (ks & 1) + hi) ^ ((li >> 2) & 3)) * 16)
                      : P8_WBASE + (wc * 32 + li) * 128 + (((2 * ks + hi) ^ swz) * 16);
    }
    bf16x8 af[2][4], w0[4], w1[4];
    bf16x8 dum[12];                              // (ABL bit 6: the reads land here and nothing waits for them before the MFMAs)
    auto read_a = [&](int buf, int h) {
        if (ABL & 4) return;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(smem + offA[ks] + (buf * 2 + h) * P8_HALF + mt * 4096);
                if (ABL & 64) dum[4 + mt * 4 + ks] = v; else af[mt][ks] = v;
            }
    };
    auto read_w = [&](int buf, int h, bf16x8 (&w)[4]) {
        if (ABL & 4) return;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(smem + offW[ks] + (buf * 2 + h) * P8_HALF);
            if (ABL & 64) dum[ks] = v; else w[ks] = v;
        }
    };
    auto eat = [&]() {
        if (ABL & 64) {
#pragma unroll
            for (int i = 0; i < 12; ++i) asm volatile("" ::"v"(dum[i]));
        }
    };

    f32x16 acc[4][2];
    // bf16: the bias enters as ONE EXTRA k-step at the start of a tile: W' = [b_hi b_mid b_lo 0 ...] (the fp32 bias as three
    // bf16 terms: their fp32 sum is exact) against A' = [1 1 1 0 ...] -- 8 MFMAs per tile instead of 128 bias registers or
    // adds per lane, and it replaces zeroing the accumulators.  The block's columns never change (the launcher makes the tile
    // order keep n0 per block), so the two operand register sets live for the whole kernel.
    const int n0 = (tile_of_round(0) % nbn) * P8_BN;
    bf16x8 wb[2], ones;
    f32x4 biasr[2];                               // fp32: the lane's bias values in the layout AFTER the transposition
    if (!WORDS) {
        // (H16: the same three-term bias on fp16 operands -- the sum of three fp16 terms is exact for |b| in fp16's normal range)
        auto pack3 = [&](float x0, float x1, float x2) {
            if constexpr (H16) {
                const _Float16 z = (_Float16)0.f;
                return __builtin_bit_cast(bf16x8, f16x8{(_Float16)x0, (_Float16)x1, (_Float16)x2, z, z, z, z, z});
            } else {
                const __bf16 z = (__bf16)0.f;
                return bf16x8{(__bf16)x0, (__bf16)x1, (__bf16)x2, z, z, z, z, z};
            }
        };
        auto rnd = [&](float x) { if constexpr (H16) return (float)(_Float16)x; else return (float)(__bf16)x; };
        const float o = hi ? 0.f : 1.f;
        ones = pack3(o, o, o);
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const float b = (p.bias && !hi) ? p.bias[n0 + (wc * 2 + tn) * 32 + li] : 0.f;
            const float b0 = rnd(b), b1 = rnd(b - b0), b2 = rnd(b - b0 - b1);
            wb[tn] = pack3(b0, b1, b2);
            asm volatile("" : "+v"(wb[tn]));     // landed before the pipeline starts: no compiler-inserted wait inside it
        }
    } else {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            biasr[tn] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n0 + (wc * 2 + tn) * 32 + 4 * (lane & 7)) : f32x4{0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+v"(biasr[tn]));
        }
    }
    // quadrant (ah, bh): 2 m-tiles x 1 n-tile x 4 k-steps; INIT: first k-tile of an output tile
    // FRESH (FS): the A fragments of this quadrant were read in this phase and are still fp32 words
    auto mma = [&](int ah, int bh, const bf16x8 (&w)[4], auto initc, auto freshc) {
        constexpr bool INIT = decltype(initc)::value;
        constexpr bool FRESH = decltype(freshc)::value;
        if (ABL & 2) return;
        if (!(ABL & 128)) __builtin_amdgcn_s_setprio(1);
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (F32) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const f32x4 wf = __builtin_bit_cast(f32x4, w[ks]);
#pragma unroll
                for (int sft = 0; sft < 4; ++sft)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        float a = __builtin_bit_cast(f32x4, af[mt][ks])[sft];
                        if (RELU) a = fmaxf(a, 0.f);
                        const f32x16 c0 = (INIT && ADD == 0 && ks == 0 && sft == 0) ? zero : acc[2 * ah + mt][bh];
                        acc[2 * ah + mt][bh] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[sft], a, c0, 0, 0, 0);
                    }
            }
        } else if (FS) {
            // the fragments read in this phase are split first, in place: af[mt][2 ks] = Ah, af[mt][2 ks + 1] = Al of k-step ks (the eight
            // words of a k-step are the two chunks 2 ks, 2 ks + 1; phases 2 and 4 find them split).  No barrier between the split and the
            // MFMAs: the compiler spreads the VALU work of the later fragments under the first MFMAs.
            typedef float f32x8 __attribute__((ext_vector_type(8)));
            if constexpr (FRESH && AP) {          // pair words: the producer made the halves, two byte permutes per register pair separate them
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const f32x4 x0 = __builtin_bit_cast(f32x4, af[mt][2 * ks]), x1 = __builtin_bit_cast(f32x4, af[mt][2 * ks + 1]);
                        f16s_unpack8<RELU>(x0, x1, af[mt][2 * ks], af[mt][2 * ks + 1]);
                    }
            } else if constexpr (FRESH) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const f32x4 x0 = __builtin_bit_cast(f32x4, af[mt][2 * ks]), x1 = __builtin_bit_cast(f32x4, af[mt][2 * ks + 1]);
                        f32x8 x;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            x[c] = __builtin_amdgcn_fmed3f(x0[c], RELU ? 0.f : -65504.f, 65504.f);
                            x[4 + c] = __builtin_amdgcn_fmed3f(x1[c], RELU ? 0.f : -65504.f, 65504.f);
                        }
                        const u32x4 h = __builtin_bit_cast(u32x4, __builtin_convertvector(x, f16x8));
                        // (x - Ah) 2^11 = fma(Ah, -2^11, x 2^11) as ONE mixed-precision fma per word, fp16 operand in, fp16 result out
                        // (v_fma_mixlo / mixhi_f16 on the halves of a register pair; hipcc does not select them from C++: it packs the fp32
                        // form, five operations per pair more): both products are exact in fp32, so is their sum, the only rounding is the
                        // one to fp16.  Plain VALU results: no wait states towards the MFMAs that read them.
                        u32x4 l;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            unsigned r;
                            asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h[c]), "s"(-2048.f), "v"(x[2 * c] * 2048.f));      // 2^F16S_A_SHIFT
                            asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(h[c]), "s"(-2048.f), "v"(x[2 * c + 1] * 2048.f));
                            l[c] = r;
                        }
                        af[mt][2 * ks] = __builtin_bit_cast(bf16x8, h);
                        af[mt][2 * ks + 1] = __builtin_bit_cast(bf16x8, l);
                    }
            }
            // w = {Wh ks0, Wh ks1, Wl ks0, Wl ks1}; term order per accumulator: (Wh 2^-11).Al, Wl.Ah, Wh.Ah
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 ws = __builtin_bit_cast(bf16x8, __builtin_bit_cast(f16x8, w[ks]) * (_Float16)0.00048828125f);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = mfma_h<true>(ws, af[mt][2 * ks + 1], (INIT && ADD == 0 && ks == 0) ? zero : acc[2 * ah + mt][bh]);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = mfma_h<true>(w[2 + ks], af[mt][2 * ks], acc[2 * ah + mt][bh]);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = mfma_h<true>(w[ks], af[mt][2 * ks], acc[2 * ah + mt][bh]);
            }
        } else if (X3) {
            // w = {hi ks0, hi ks1, lo ks0, lo ks1}; term order per accumulator: w_hi.a_lo, w_lo.a_hi, w_hi.a_hi (small terms
            // first, as gemm_core.h PipeSplitDma); the two accumulators take turns so that no MFMA waits for its predecessor
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 ahi[2], alo[2];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    u32x4 x0 = __builtin_bit_cast(u32x4, af[mt][2 * ks]), x1 = __builtin_bit_cast(u32x4, af[mt][2 * ks + 1]);
                    if (RELU) {          // x < 0  <=>  its hi part is negative: sign bit of the word; the whole word becomes +0
#pragma unroll
                        for (int c = 0; c < 4; ++c) { x0[c] = (unsigned)max((int)x0[c], 0); x1[c] = (unsigned)max((int)x1[c], 0); }
                    }
                    u32x4 h, l;
                    h[0] = __builtin_amdgcn_perm(x0[1], x0[0], 0x07060302u); h[1] = __builtin_amdgcn_perm(x0[3], x0[2], 0x07060302u);
                    h[2] = __builtin_amdgcn_perm(x1[1], x1[0], 0x07060302u); h[3] = __builtin_amdgcn_perm(x1[3], x1[2], 0x07060302u);
                    l[0] = __builtin_amdgcn_perm(x0[1], x0[0], 0x05040100u); l[1] = __builtin_amdgcn_perm(x0[3], x0[2], 0x05040100u);
                    l[2] = __builtin_amdgcn_perm(x1[1], x1[0], 0x05040100u); l[3] = __builtin_amdgcn_perm(x1[3], x1[2], 0x05040100u);
                    ahi[mt] = __builtin_bit_cast(bf16x8, h);
                    alo[mt] = __builtin_bit_cast(bf16x8, l);
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[ks], alo[mt], (INIT && ADD == 0 && ks == 0) ? zero : acc[2 * ah + mt][bh], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2 + ks], ahi[mt], acc[2 * ah + mt][bh], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[ks], ahi[mt], acc[2 * ah + mt][bh], 0, 0, 0);
            }
        } else {
            if (INIT) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[2 * ah + mt][bh] = mfma_h<H16>(wb[bh], ones, ADD != 0 ? acc[2 * ah + mt][bh] : zero);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    bf16x8 a = af[mt][ks];
                    if (RELU) a = __builtin_bit_cast(bf16x8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, a), s16x8{0, 0, 0, 0, 0, 0, 0, 0}));
                    acc[2 * ah + mt][bh] = mfma_h<H16>(w[ks], a, acc[2 * ah + mt][bh]);
                }
        }
        if (!(ABL & 128)) __builtin_amdgcn_s_setprio(0);
        eat();
    };

    // ---- epilogue of one 32-row strip (tm) of the wave tile ----
    // Lane (li, hi) holds row li and columns tn*32 + 8g + 4hi .. +3 (gemm_core.h).  The strip is transposed through a
    // wave-private LDS buffer of 32 rows x 128 bytes (16-byte chunks XOR-swizzled with row & 7) so that lane l then holds
    // 16 consecutive bytes of row 8j + (l >> 3), chunk l & 7: one store instruction writes 8 full 128-byte rows.
    char* const tbuf = smem + P8_TBASE + wave * 4096;
    // (half rows: a lane writes 8 bytes; rows li and li + 8 of a 16-lane write group name the same chunk, so the upper eight
    //  rows take the chunk's OTHER half -- 32 distinct banks per group instead of a 2-way conflict (PMC, round 3: 10-12 % of the
    //  LDS cycles of the half-row launches) -- and the reader swaps the halves back for those rows, a register renaming)
    const int t_wr = li * 128 + (HALF ? (hi ^ ((li >> 3) & 1)) * 8 : 0), t_x = (li & 7) << 4;
    const int t_rd = (lane >> 3) * 128 + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);
    const unsigned ldc4 = (unsigned)p.ldc * 4u;
    const unsigned vst = (unsigned)(lane >> 3) * ldc4 + (unsigned)(lane & 7) * 16u;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, (int)(((size_t)(p.M - 1) * p.ldc + p.N) * 4), 0x00020000);
    const float cs = p.c_scale;
    const float fs_up = FS ? __builtin_ldexpf(1.f, p.w_exp) : 1.f, fs_down = FS ? __builtin_ldexpf(1.f, -p.w_exp) : 1.f;
    const float act_lo = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    // ACTV (wave-uniform, picked once per strip): 0 = no output activation and c_scale 1, 1 = ReLU and c_scale 1, 2 = the
    // general form.  The first two are what the forward launches; they drop the max / multiply per element (the compiler
    // needs two v_max per fmaxf on values it cannot prove canonical), and the half-row ReLU runs on packed bf16 pairs.
    const int actv = __builtin_amdgcn_readfirstlane(cs != 1.f ? 2 : p.act == ACT_RELU ? 1 : 0);
    auto relu1 = [](float x) { float y; asm("v_max_f32 %0, 0, %1" : "=v"(y) : "v"(x)); return y; };
    auto epi_t = [&](auto tmc, auto actc, int m0) __attribute__((always_inline)) {
        constexpr int TM = decltype(tmc)::value;
        constexpr int ACTV = decltype(actc)::value;
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef short s16x2 __attribute__((ext_vector_type(2)));
        const unsigned srow = (unsigned)(m0 + wr * 128 + TM * 32) * ldc4 + (unsigned)(n0 + wc * 64) * (HALF ? 2u : 4u);
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = acc[TM][tn][4 * g + c];
                if (!WORDS) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (ACTV == 2) v[c] = fmaxf(v[c], act_lo) * cs;      // (branch-free: ReLU or max with -inf)
                        else if (ACTV == 1 && !HALF) v[c] = relu1(v[c]);
                    }
                }
                if (HALF) {
                    s16x2 w0, w1;
                    if (CF == 3) {
                        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = __builtin_amdgcn_fmed3f(v[c], -65504.f, 65504.f);
                        w0 = __builtin_bit_cast(s16x2, __builtin_convertvector((f32x2{v[0], v[1]}), f16x2));
                        w1 = __builtin_bit_cast(s16x2, __builtin_convertvector((f32x2{v[2], v[3]}), f16x2));
                    } else {
                        w0 = __builtin_bit_cast(s16x2, __builtin_convertvector((f32x2{v[0], v[1]}), bf16x2));
                        w1 = __builtin_bit_cast(s16x2, __builtin_convertvector((f32x2{v[2], v[3]}), bf16x2));
                    }
                    if (ACTV == 1) {          // ReLU after the rounding: the same values (rounding keeps the sign; -0 becomes +0)
                        w0 = __builtin_elementwise_max(w0, s16x2{0, 0});
                        w1 = __builtin_elementwise_max(w1, s16x2{0, 0});
                    }
                    u32x2 w;
                    w.x = __builtin_bit_cast(unsigned, w0);
                    w.y = __builtin_bit_cast(unsigned, w1);
                    *reinterpret_cast<u32x2*>(tbuf + t_wr + (((tn * 4 + g) << 4) ^ t_x)) = w;
                } else {
                    *reinterpret_cast<f32x4*>(tbuf + t_wr + (((2 * g + hi) << 4) ^ t_x)) = v;
                }
            }
            if (!HALF || tn == 1) {          // the buffer holds 32 rows x 128 bytes: both n-tiles (bf16) or one (fp32)
                u32x4 rj[4];                   // (all four reads in flight before the first store waits for its data)
#pragma unroll
                for (int j = 0; j < 4; ++j) rj[j] = *reinterpret_cast<const u32x4*>(tbuf + t_rd + j * 1024);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    u32x4 r = rj[j];
                    if (HALF && (j & 1)) r = u32x4{rj[j][2], rj[j][3], rj[j][0], rj[j][1]};      // rows 8 j + (lane >> 3): halves stored swapped
                    if (WORDS) {               // lane: row 8j + (l >> 3), columns tn*32 + 4 (l & 7) .. +3
                        f32x4 x = __builtin_bit_cast(f32x4, r);
                        if (FS) x *= fs_down;      // (times 2^-k: exact, and a fused multiply-add with the bias rounds once, like the plain add)
                        x += biasr[tn];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (ACTV == 2) {
                                x[c] = fmaxf(x[c], act_lo);
                                if (X3) x[c] *= cs;
                            } else if (ACTV == 1) {
                                x[c] = relu1(x[c]);
                            }
                        }
                        r = __builtin_bit_cast(u32x4, x);
                        if constexpr (CPA) {   // attention pair words: this block's columns are K (below N / 2) or V (times 2^3)
                            const float vs = 2 * n0 >= p.N ? 8.f : 1.f;
#pragma unroll
                            for (int c = 0; c < 4; c += 2) {
                                unsigned w0, w1;
                                f16s_attn_pack2(x[c], x[c + 1], vs, w0, w1);
                                r[c] = w0;
                                r[c + 1] = w1;
                            }
                        } else if constexpr (CP) { // GEMM pair words of the split-fp16 operand (gemm_f16s_planes.h), two elements at a time
#pragma unroll
                            for (int c = 0; c < 4; c += 2) {
                                unsigned w0, w1;
                                f16s_pack2(x[c], x[c + 1], w0, w1);
                                r[c] = w0;
                                r[c + 1] = w1;
                            }
                        } else if constexpr (CF == 1) {  // split pairs (common.h pack_split), two elements at a time
#pragma unroll
                            for (int c = 0; c < 4; c += 2) {
                                const f32x2 v2 = {x[c], x[c + 1]};
                                const bf16x2 h2 = __builtin_convertvector(v2, bf16x2);
                                const bf16x2 l2 = __builtin_convertvector(v2 - __builtin_convertvector(h2, f32x2), bf16x2);
                                const unsigned hb = __builtin_bit_cast(unsigned, h2), lb = __builtin_bit_cast(unsigned, l2);
                                r[c] = __builtin_amdgcn_perm(hb, lb, 0x05040100u);
                                r[c + 1] = __builtin_amdgcn_perm(hb, lb, 0x07060302u);
                            }
                        }
                    }
                    if (!(ABL & 8)) {
                        __builtin_amdgcn_raw_buffer_store_b128(r, rc, vst, srow + (unsigned)(8 * j) * ldc4 + (HALF ? 0u : (unsigned)tn * 128u), 0);
                        // A 128-bit buffer store reads its data registers a few cycles after issue; hipcc pads a following VALU
                        // write of them ONLY when the store has no SGPR soffset (LLVM's hazard rule assumes the register form is
                        // safe) -- on gfx950 it is not: split-pair epilogues, whose pack code reuses the registers at once, stored
                        // garbage in one dword of some lanes until this pad went in (found with the bit-identity test).
                        // (the data registers are named as an input so that they stay allocated across the pad: a side-effecting asm
                        //  orders memory operations only, and `r` is otherwise dead after the store)
                        asm volatile("s_nop 3" ::"v"(r) : "memory");
                    } else
                        asm volatile("" ::"v"(r));
                }
            }
        }
    };
    auto epi = [&](auto tmc, int m0) __attribute__((always_inline)) {     // (not inlined = the accumulators live in scratch)
        if (actv == 0) epi_t(tmc, std::integral_constant<int, 0>{}, m0);
        else if (actv == 1) epi_t(tmc, std::integral_constant<int, 1>{}, m0);
        else epi_t(tmc, std::integral_constant<int, 2>{}, m0);
    };

    // ---- prologue: the six half-tiles whose staging phase lies before the first compute phase ----
    ld2(ra, sdst, vA, c0.sa + kti(c0) * KA, 128u * lda4);                                         // A_0(0)
    ldw(sdst + P8_WBASE, c0.sw + kti(c0) * KW, 0);                                                // W_0(0)
    ldw(sdst + P8_WBASE + P8_HALF, c0.sw + kti(c0) * KW, 1);                                      // W_1(0)
    ld2(ra, sdst + P8_HALF, vA, c0.sa + kti(c0) * KA + 64u * lda4, 128u * lda4);                  // A_1(0)
    ld2(ra, sdst + 2 * P8_HALF, vA, c1.sa + kti(c1) * KA, 128u * lda4);                           // A_0(1)
    ldw(sdst + P8_WBASE + 2 * P8_HALF, c1.sw + kti(c1) * KW, 0);                                  // W_0(1)
    p8_wait_vm<8>();
    p8_barrier();
    if (wr == 1) p8_barrier();                       // the two wave rows run one barrier apart from here on

    // One K-tile = four phases on buffer B; c1 / c2 = the K-tiles one and two ahead.  VAR places the epilogue strips
    // (pm0: row base of the tile they belong to) and sets the counted waits: the half-tile a phase's wait must retire was
    // issued four load parts earlier, with 8 LDS-direct loads and the epilogue stores of the parts since behind it.
    auto ktile = [&](auto bufc, auto varc, int pm0) {
        constexpr int B = decltype(bufc)::value;
        constexpr int VAR = decltype(varc)::value;
        // (a load part is [strip: E stores][2 LDS-direct loads][wait]: the wait of part j lets the loads of parts j-3 .. j
        //  and the stores of those four parts stay in flight; strips sit in L3, L4, F1, F2)
        constexpr int N1 = 8 + (VAR == P8_FIRST ? 3 * E : VAR == P8_SECOND ? E : 0);
        constexpr int N2 = 8 + (VAR == P8_FIRST ? 4 * E : 0);
        constexpr int N4 = 8 + (VAR == P8_FIRST || VAR == P8_LAST ? 2 * E : 0);
        using Init = std::integral_constant<bool, VAR == P8_FIRST || VAR == P8_FIRST0>;
        const unsigned a1 = c1.sa + kti(c1) * KA, w1o = c1.sw + kti(c1) * KW;
        const unsigned a2 = c2.sa + kti(c2) * KA, w2o = c2.sw + kti(c2) * KW;
        // phase 1: quadrant (a0, w0)
        if (VAR == P8_FIRST) {               // (before the fragment reads: the strip's temporaries need their registers)
            epi(std::integral_constant<int, 2>{}, pm0);
            __builtin_amdgcn_sched_barrier(0);
        }
        read_w(B, 0, w0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(B, 0);
        stage_w(B ^ 1, 1, w1o);
        p8_wait_vm<N1>();
        if (!(ABL & 32)) p8_barrier();
        if (!(ABL & 64)) p8_wait_lds();
        __builtin_amdgcn_sched_barrier(0);
        mma(0, 0, w0, Init{}, std::true_type{});
        __builtin_amdgcn_sched_barrier(0);
        if (!(ABL & 48)) p8_barrier();
        // phase 2: quadrant (a0, w1)
        if (VAR == P8_FIRST) {
            epi(std::integral_constant<int, 3>{}, pm0);
            __builtin_amdgcn_sched_barrier(0);
        }
        read_w(B, 1, w1);
        stage_a(B ^ 1, 1, a1);
        p8_wait_vm<N2>();
        if (!(ABL & 32)) p8_barrier();
        if (!(ABL & 64)) p8_wait_lds();
        __builtin_amdgcn_sched_barrier(0);
        mma(0, 1, w1, Init{}, std::false_type{});
        __builtin_amdgcn_sched_barrier(0);
        if (!(ABL & 48)) p8_barrier();
        // phase 3: quadrant (a1, w1)
        if (VAR == P8_LAST) {
            epi(std::integral_constant<int, 0>{}, pm0);
            __builtin_amdgcn_sched_barrier(0);
        }
        read_a(B, 1);
        stage_a(B, 0, a2);
        if (!(ABL & 32)) p8_barrier();
        if (!(ABL & 64)) p8_wait_lds();
        __builtin_amdgcn_sched_barrier(0);
        mma(1, 1, w1, Init{}, std::true_type{});
        __builtin_amdgcn_sched_barrier(0);
        if (!(ABL & 48)) p8_barrier();
        // phase 4: quadrant (a1, w0)
        if (VAR == P8_LAST) {
            epi(std::integral_constant<int, 1>{}, pm0);
            __builtin_amdgcn_sched_barrier(0);
        }
        stage_w(B, 0, w2o);
        p8_wait_vm<N4>();
        if (!(ABL & 32)) p8_barrier();
        if (!(ABL & 64)) p8_wait_lds();
        __builtin_amdgcn_sched_barrier(0);
        mma(1, 0, w0, Init{}, std::false_type{});
        __builtin_amdgcn_sched_barrier(0);
        if (!(ABL & 48)) p8_barrier();
        c1 = c2;
        advance(c2);
    };
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    using Mid = std::integral_constant<int, P8_MID>;

    int pm0 = 0;
    for (int round = 0;; ++round) {
        const int v = tile_of_round(round);
        if (v >= n_tiles) break;
        const int m0 = (v / nbn) * P8_BM;
        if (ADD == 6 && (ABL & 256)) {
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = min(m0 + wr * 128 + tm * 32 + g * 8 + (lane >> 3), p.M - 1);
                    const float* r0 = p.g0 + (size_t)p.gi0[row] * p.ldg0 + n0 + wc * 64 + (lane & 7) * 4;
                    const float* r1 = p.g1 + (size_t)p.gi1[row] * p.ldg1 + n0 + wc * 64 + (lane & 7) * 4;
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) {
                        const f32x4 x = *reinterpret_cast<const f32x4*>(r0 + tn * 32) + *reinterpret_cast<const f32x4*>(r1 + tn * 32);
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[tm][tn][4 * g + c] = x[c];
                    }
                }
        } else if (ADD != 0 && !(ABL & 512))
            tile_init<4, 2, ADD, F32 || FS>(p, m0, n0, wr, wc, lane, acc);   // (PLAIN only for fp32: formats fold away)
        if (FS && ADD != 0) {                        // the accumulators hold 2^k times the sums (the weight planes are scaled)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) acc[tm][tn] *= fs_up;
        }
        if (SPREAD && round > 0) {                   // strips 2 / 3 of the previous tile go out under this tile's first phases
            ktile(B0{}, std::integral_constant<int, P8_FIRST>{}, pm0);
            ktile(B1{}, std::integral_constant<int, P8_SECOND>{}, pm0);
        } else {
            ktile(B0{}, std::integral_constant<int, P8_FIRST0>{}, 0);
            ktile(B1{}, Mid{}, 0);
        }
        for (int kt = 2; kt < KT - 2; kt += 2) {     // (KT is even and >= 4: the launcher checks K % 128 == 0, K >= 256)
            ktile(B0{}, Mid{}, 0);
            ktile(B1{}, Mid{}, 0);
        }
        ktile(B0{}, Mid{}, 0);
        ktile(B1{}, std::integral_constant<int, P8_LAST>{}, m0);
        if (!SPREAD) {                               // additive operands are loaded as accumulator inits of the next tile
            epi(std::integral_constant<int, 2>{}, m0);
            epi(std::integral_constant<int, 3>{}, m0);
        }
        pm0 = m0;
    }
    if (wr == 0) p8_barrier();
    if (SPREAD) {
        epi(std::integral_constant<int, 2>{}, pm0);
        epi(std::integral_constant<int, 3>{}, pm0);
    }
    p8_wait_vm<0>();                                 // no LDS-direct load may outlive the block's LDS allocation
}
