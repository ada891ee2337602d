// Edge gate of the fp32 mode on the 16-bit matrix cores at the shipped 8 x (64, 64, 32) geometry: every product as three fp16 MFMAs
// (v_mfma_f32_32x32x16_f16) with fp32-grade error -- the sibling of edge_gate_kernel (edge_gate.hip) that launch_gate runs for GATE_F32
// when GateArgs::f16s is set.  Algebra and lane model: gate_core.h.  Operand scheme: gemm_f16s_planes.h / gemm_core.h (f16s_split8).
//   * weights: the block makes the planes itself from the fp32 weights (they are tiny): per tensor k = 13 - ceil(log2 max |w|) from an
//     order-independent integer max over the tensor (the same in every block), Wh = f16(w 2^k), Wl = f16(w 2^k - Wh); the third
//     operand Wh 2^-11 is made from the Wh fragment in registers (f16s_w_small);
//   * activations: the kproj row and the hidden vector are split by f16s_split8 (Ah = f16(clamp(a)), Al = f16((a - Ah) 2^11); its
//     lower bound 0 is the ReLU of the hidden layer);
//   * a product is  (Wh 2^-11) . Al + Wl . Ah + Wh . Ah  into ONE fp32 accumulator, in this order;
//   * hidden = relu(acc1 2^-k0 + Gq);  the logit accumulators start at b3 2^k3 and leave times 2^-k3.
// A row's bits depend on its own inputs only: one lane computes one row, and no value crosses rows before gate_store / the max
// aggregation.  So both row maps, every grid size, the twin launch and the fused aggregation give the same bits per row.
// Shape: NW waves share ONE copy of the planes (53.8 KB); NW = 8 is 76 KB per block with the aggregation's wave buffers, two blocks per
// CU = four waves per SIMD at <= 128 VGPRs (the split-bf16 kernel of edge_gate_bf16.hip holds two), which is what hides a unit's
// chain  index -> gathers -> 4 x (12 MFMAs -> hidden -> 6 MFMAs) -> softmax -> LDS passes -> atomics.  The next unit's edge indices
// are loaded while the current unit computes, and the Gq values of a hidden slice ahead of the slice's layer-1 MFMAs.
#include "gate_core.h"
#include "gate_agg.h"

namespace vlsat {

namespace {

constexpr int GS_P0 = 144;      // W0k plane row pitch (64 fp16 + 16 B)
constexpr int GS_P3 = 264;      // W3 plane row pitch (128 fp16 + 8 B), as in edge_gate_bf16.hip
constexpr int GS_W0B = 128 * GS_P0, GS_W3B = 32 * GS_P3;

typedef _Float16 f16x4_gs __attribute__((ext_vector_type(4)));

// bits of max |w| over a tensor of n floats (n % 4 == 0) seen by this thread; folded over the block with an LDS atomic max: integer
// max is associative and commutative, every block gets the same bits
template <int NT>
__device__ __forceinline__ unsigned gate_absmax_bits(const float* w, int n, int tid) {
    unsigned m = 0;
    for (int i = tid * 4; i < n; i += NT * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned a = __float_as_uint(v[c]) & 0x7fffffffu;
            m = a > m ? a : m;
        }
    }
    return m;
}
// w [ROWS][COLS] fp32 -> planes Wh = f16(w scale), Wl = f16(w scale - Wh) (gemm_f16s_planes.h f16s_split), rows of PITCH bytes
template <int ROWS, int COLS, int PITCH, int NT>
__device__ __forceinline__ void gate_stage_f16s(char* sW, const float* w, float scale, int tid) {
    for (int i = tid; i < ROWS * (COLS / 4); i += NT) {
        const int r = i / (COLS / 4), c4 = (i % (COLS / 4)) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + r * COLS + c4);
        f32x4 x;
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = __builtin_amdgcn_fmed3f(v[c] * scale, -65504.f, 65504.f);
        const f16x4_gs h = __builtin_convertvector(x, f16x4_gs);
        const f16x4_gs l = __builtin_convertvector(x - __builtin_convertvector(h, f32x4), f16x4_gs);
        *reinterpret_cast<f16x4_gs*>(sW + r * PITCH + c4 * 2) = h;
        *reinterpret_cast<f16x4_gs*>(sW + ROWS * PITCH + r * PITCH + c4 * 2) = l;
    }
}
// acc += W . A as the three MFMAs of the scheme, small terms first
__device__ __forceinline__ f32x16 gate_mma_f16s(const bf16x8& wh, const bf16x8& wl, const bf16x8& ah, const bf16x8& al, f32x16 acc) {
    acc = mfma_h<true>(f16s_w_small(wh), al, acc);
    acc = mfma_h<true>(wl, ah, acc);
    return mfma_h<true>(wh, ah, acc);
}

// NW: waves of a block (they share the planes).  TWIN: two gates on one edge list in one launch, selected by blockIdx.y (edge_gate.hip)
template <int NW, bool TWIN>
__global__ __launch_bounds__(64 * NW, NW / 2) void edge_gate_f16s_kernel(GateArgs pa, GateArgs pb) {
    const GateArgs& p = (TWIN && blockIdx.y != 0) ? pb : pa;
    constexpr int NT = 64 * NW;
    __shared__ __attribute__((aligned(16))) char smem[2 * (GS_W0B + GS_W3B) + NW * AG_WAVE_BYTES];     // + the fused aggregation's wave buffers (gate_agg.h)
    __shared__ __attribute__((aligned(16))) float sB3[32];        // b3 2^k3
    __shared__ unsigned sMax[2];
    char* sW0 = smem;                          // [2][128][144]
    char* sW3 = smem + 2 * GS_W0B;             // [2][32][264]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li0 = lane & 31, hi0 = lane >> 5;

    if (tid < 2) sMax[tid] = 0u;
    __syncthreads();
    if (p.use_edge) atomicMax(&sMax[0], gate_absmax_bits<NT>(p.w0k, 128 * 64, tid));
    atomicMax(&sMax[1], gate_absmax_bits<NT>(p.w3, 32 * 128, tid));
    __syncthreads();
    const int k0 = f16s_exponent(sMax[0]), k3 = f16s_exponent(sMax[1]);
    const float s0inv = f16s_pow2(-k0), s3inv = f16s_pow2(-k3);
    if (p.use_edge) gate_stage_f16s<128, 64, GS_P0, NT>(sW0, p.w0k, f16s_pow2(k0), tid);
    gate_stage_f16s<32, 128, GS_P3, NT>(sW3, p.w3, f16s_pow2(k3), tid);
    if (tid < 32) sB3[tid] = p.b3[tid] * f16s_pow2(k3);
    __syncthreads();

    // Work unit of a WAVE = 32 rows: row_map 1: 32 consecutive edges of one head (wave unit u: edges 32 (u >> 3) .., head u & 7; edge
    // lists are source-major, so the 32 lanes of a Gq load mostly name the same node row), row_map 0: 4 edges x 8 heads.  A block
    // takes NW consecutive wave units per step.
    const int n_wu = p.row_map ? 8 * ((p.n_edges + 31) / 32) : (p.n_edges + 3) / 4;
    const int n_units = (n_wu + NW - 1) / NW;
    auto edge_of = [&](int g) { const int u = g * NW + wave; return p.row_map ? (u >> 3) * 32 + li0 : u * 4 + (li0 >> 3); };
    int e_raw = edge_of(blockIdx.x < n_units ? (int)blockIdx.x : 0);
    int e = e_raw < p.n_edges ? e_raw : p.n_edges - 1;
    int sn = p.src[e], dn = p.dst[e];
    for (int g = blockIdx.x; g < n_units; g += gridDim.x) {
        asm volatile("" ::: "memory");                    // keep the weight fragments out of LICM's hands (edge_gate.hip)
        // ... and the lane-invariant 64-bit address bases as well: the unit makes its addresses from lane indices the compiler cannot see
        // through, a few integer operations per unit; hoisted, the bases take the registers that the 128 of four waves per SIMD do not have
        int li = li0, hi = hi0;
        asm volatile("" : "+v"(li), "+v"(hi));
        const int h = p.row_map ? (g * NW + wave) & 7 : li & 7;
        const bool valid = e_raw < p.n_edges;
        const int e_cur = e, sn_cur = sn, dn_cur = dn;
        bf16x8 zh[4], zl[4];
        if (p.use_edge) {
            const float* zrow = p.kproj + (size_t)e_cur * 512 + h * 64 + 8 * hi;
            f32x4 z[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = *reinterpret_cast<const f32x4*>(zrow + 16 * (j >> 1) + 4 * (j & 1));
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) f16s_split8(z[2 * ks], z[2 * ks + 1], -65504.f, zh[ks], zl[ks]);
        }
        const float* gq = p.node + (size_t)sn_cur * p.ld_node + p.gq_off + h * 128 + 4 * hi;
        {       // the next unit's indices travel while this one computes
            const int gn = g + (int)gridDim.x < n_units ? g + (int)gridDim.x : g;
            e_raw = edge_of(gn);
            e = e_raw < p.n_edges ? e_raw : p.n_edges - 1;
            sn = p.src[e];
            dn = p.dst[e];
        }
        f32x16 lg[1];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(sB3 + 8 * r4 + 4 * hi);
#pragma unroll
            for (int c = 0; c < 4; ++c) lg[0][r4 * 4 + c] = b[c];
        }
#pragma unroll
        for (int to = 0; to < 4; ++to) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            f32x4 gqv[4];                   // Gq of this slice: issued ahead of the slice's layer-1 MFMAs, which hide the gather
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) gqv[r4] = *reinterpret_cast<const f32x4*>(gq + to * 32 + 8 * r4);
            if (p.use_edge) {               // (USE_GCN_EDGE=false: hidden = relu(Gq), the edge half is absent)
                const char* ap = sW0 + (to * 32 + li) * GS_P0 + 16 * hi;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    acc = gate_mma_f16s(*reinterpret_cast<const bf16x8*>(ap + 32 * ks), *reinterpret_cast<const bf16x8*>(ap + GS_W0B + 32 * ks),
                                        zh[ks], zl[ks], acc);
            }
            // hidden = relu(acc 2^-k0 + Gq[src, h*128 + o]), o = 32 to + 8 r4 + 4 hi + c in register 4 r4 + c; the ReLU is the lower
            // bound of the split.  Registers 8 half .. 8 half + 7 are the layer-2 B operand of step (to, half)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 p0, p1;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    p0[c] = fmaf(acc[8 * half + c], s0inv, gqv[2 * half][c]);
                    p1[c] = fmaf(acc[8 * half + 4 + c], s0inv, gqv[2 * half + 1][c]);
                }
                bf16x8 hh, hl;
                f16s_split8(p0, p1, 0.f, hh, hl);
                const char* wp = sW3 + li * GS_P3 + (to * 32 + 16 * half + 4 * hi) * 2;
                lg[0] = gate_mma_f16s(gate_w3_frag(wp), gate_w3_frag(wp + GS_W3B), hh, hl, lg[0]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[0][r] *= s3inv;
        const float inv = gate_softmax<1, 32>(lg);
        int ho = hi;                       // (the output addresses are made here, not carried through the unit)
        asm volatile("" : "+v"(ho));
        const float* vrow = p.node + (size_t)dn_cur * p.ld_node + p.v_off + h * 32 + 4 * ho;
        if (p.agg) {                       // fused max aggregation: the gated rows are never stored (gate_agg.h)
            gate_aggregate_max(smem + 2 * (GS_W0B + GS_W3B) + wave * AG_WAVE_BYTES, lg[0], inv, vrow, valid ? sn_cur : -1, li, ho, lane, h, p.agg,
                               p.ld_agg);
        } else if (valid) {
            gate_store<1, 32>(lg, inv, vrow, p.gated + (size_t)e_cur * 256 + h * 32 + 4 * ho, p.prob, (size_t)e_cur * 256, 8, h, ho);
        }
    }
}

}  // namespace

int launch_gate_f16s(const GateArgs& a, hipStream_t s, const GateArgs* twin) {
    constexpr int NW = 8;
    const GateArgs& b = twin ? *twin : a;
    const int n_wu = a.row_map ? 8 * ((a.n_edges + 31) / 32) : (a.n_edges + 3) / 4;
    const int n_units = (n_wu + NW - 1) / NW;
    // persistent grid (planes made once per block): two blocks of eight waves per CU
    const int cap = a.grid_cap > 0 ? a.grid_cap : 512;
    const int grid = n_units < cap ? n_units : cap;
    if (twin) hipLaunchKernelGGL((edge_gate_f16s_kernel<NW, true>), dim3(grid, 2), dim3(64 * NW), 0, s, a, b);
    else hipLaunchKernelGGL((edge_gate_f16s_kernel<NW, false>), dim3(grid), dim3(64 * NW), 0, s, a, a);
    VLSAT_LAUNCH_CHECK("edge_gate_f16s");
    return 0;
}

}  // namespace vlsat
