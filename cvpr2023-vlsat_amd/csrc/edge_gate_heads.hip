// Edge gate on the fp32 matrix cores for the head geometries other than the shipped 8 x (64, 64, 32): MODEL.NUM_HEADS in {4, 8, 16}
// and DIM_ATTEN in {128, 256, 512} (reference network_MMG.py:48-50,69-79,96-104) give d_k = 512 / H in {128, 64, 32}, a hidden layer
// of 2 d_k and d_o = DIM_ATTEN / H in {8 .. 128}.  Algebra and lane model: gate_core.h; a wave owns 32 consecutive EDGES of one head
// (source-major edge lists: its Gq loads name one or two node rows), v_mfma_f32_32x32x2_f32 as in edge_gate.hip.
// What the template adds: TO = 2 d_k / 32 hidden slices, d_k / 2 MFMAs per slice, MO = ceil(d_o / 32) logit blocks.  Weights:
// W0k [2 d_k][d_k] and W3 [d_o][2 d_k] in LDS; at d_k = 128 W0k alone is 135 KB, so there the block is 8 waves (one block per CU)
// and W3's fragments come from global memory (64 .. 128 KB, L2-resident; 25 GB/s per CU against the 49 000 MFMA cycles of a wave
// step).  On the VALU kernel of edge_gate.hip (kept for anything else) these geometries took 266 ms per bench step at 4 heads,
// 77 ms at 16, against 1.1 ms at 8.
#include "gate_core.h"

namespace vlsat {

namespace {

template <int DK, int DOX>
__global__ __launch_bounds__(DK == 128 ? 512 : 256, DK == 128 ? 1 : 2) void edge_gate_hd_kernel(GateArgs p, int n_heads) {
    constexpr int HID = 2 * DK, TO = HID / 32, MO = (DOX + 31) / 32, KG = DK / 8;
    constexpr int P0 = DK + 4, P3 = HID + 4;                 // LDS row pitches (floats): 16-byte pad, conflict-free b128 reads
    constexpr bool W3_LDS = DK != 128;
    constexpr bool Z_REGS = !(DK == 128 && DOX > 32);        // else: the row's kproj values are re-read per hidden slice (L1 hits) --
                                                             // 64 of them next to 32 .. 64 logit accumulators do not fit the registers
    constexpr int NT = DK == 128 ? 512 : 256, NW = NT / 64;
    static_assert(DOX % 8 == 0 && (W3_LDS || DOX % 32 == 0), "output channels per head");
    __shared__ __attribute__((aligned(16))) float sW0[HID * P0];
    __shared__ __attribute__((aligned(16))) float sW3[W3_LDS ? MO * 32 * P3 : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int A = n_heads * DOX;                              // row width of gated / prob / the value columns

    gate_stage_f32_rows<HID, HID, DK, P0, NT>(sW0, p.w0k, tid);
    if (W3_LDS) gate_stage_f32_rows<MO * 32, DOX, HID, P3, NT>(sW3, p.w3, tid);
    __syncthreads();

    const long n_wu = (long)((p.n_edges + 31) / 32) * n_heads;          // wave units: (block of 32 edges, head)
    for (long u = blockIdx.x; u * NW < n_wu; u += gridDim.x) {
        asm volatile("" ::: "memory");                        // keep the weight fragments out of LICM's hands (edge_gate.hip)
        const long wu = u * NW + wave;
        if (wu >= n_wu) continue;                             // (no barrier in this loop)
        const int h = (int)(wu % n_heads);
        const int e_raw = (int)(wu / n_heads) * 32 + li;
        const bool valid = e_raw < p.n_edges;
        const int e = valid ? e_raw : p.n_edges - 1;
        const float* zrow = p.kproj + (size_t)e * 512 + h * DK + 4 * hi;
        f32x4 z[Z_REGS ? KG : 1];
        if (Z_REGS && p.use_edge) {
#pragma unroll
            for (int kg = 0; kg < KG; ++kg) z[kg] = *reinterpret_cast<const f32x4*>(zrow + kg * 8);
        }
        const int sn = p.src[e], dn = p.dst[e];
        const float* gq = p.node + (size_t)sn * p.ld_node + p.gq_off + h * HID + 4 * hi;
        f32x16 lg[MO];
        gate_bias<MO, DOX>(lg, p.b3, hi);
#pragma unroll(DK == 128 ? 1 : TO)                        // (d_k = 128: one slice is 64 + 64 MFMAs; unrolled, the scheduler's appetite spills)
        for (int to = 0; to < TO; ++to) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (p.use_edge) {                                 // (USE_GCN_EDGE=false: hidden = relu(Gq), the edge half is absent)
#pragma unroll
                for (int kg = 0; kg < KG; ++kg) {
                    if (!Z_REGS && (kg & 3) == 0) asm volatile("" ::: "memory");     // (at most four re-read groups in flight)
                    const f32x4 a = *reinterpret_cast<const f32x4*>(sW0 + (to * 32 + li) * P0 + kg * 8 + 4 * hi);
                    const f32x4 zk = Z_REGS ? z[Z_REGS ? kg : 0] : *reinterpret_cast<const f32x4*>(zrow + kg * 8);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], zk[s], acc, 0, 0, 0);
                }
            }
            // hidden = relu(acc + Gq[src, h*HID + o]),  o = to*32 + 8*r4 + 4*hi + c; layer-2 A fragment: W3[m][o]
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                if (!W3_LDS) asm volatile("" ::: "memory");                           // (W3 fragments from global: one r4 group at a time)
                const f32x4 gqv = *reinterpret_cast<const f32x4*>(gq + to * 32 + 8 * r4);
                float hid[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) hid[c] = fmaxf(acc[r4 * 4 + c] + gqv[c], 0.f);
#pragma unroll
                for (int mo = 0; mo < MO; ++mo) {
                    const f32x4 w3v = W3_LDS ? *reinterpret_cast<const f32x4*>(sW3 + (mo * 32 + li) * P3 + to * 32 + 8 * r4 + 4 * hi)
                                             : *reinterpret_cast<const f32x4*>(p.w3 + (size_t)(mo * 32 + li) * HID + to * 32 + 8 * r4 + 4 * hi);
#pragma unroll
                    for (int c = 0; c < 4; ++c) lg[mo] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3v[c], hid[c], lg[mo], 0, 0, 0);
                }
            }
        }
        const float inv = gate_softmax<MO, DOX>(lg);
        if (valid)
            gate_store<MO, DOX>(lg, inv, p.node + (size_t)dn * p.ld_node + p.v_off + h * DOX + 4 * hi, p.gated + (size_t)e * A + h * DOX + 4 * hi,
                                p.prob, (size_t)e * A, n_heads, h, hi);
    }
}

template <int DK, int DOX>
int run(const GateArgs& a, int n_heads, hipStream_t s) {
    constexpr int NT = DK == 128 ? 512 : 256, NW = NT / 64;
    const long n_wu = (long)((a.n_edges + 31) / 32) * n_heads, units = (n_wu + NW - 1) / NW;
    const long cap = a.grid_cap > 0 ? a.grid_cap : (DK == 128 ? 256 : 768);      // persistent: weights staged once per block
    hipLaunchKernelGGL((edge_gate_hd_kernel<DK, DOX>), dim3((unsigned)std::min(units, cap)), dim3(NT), 0, s, a, n_heads);
    return 0;
}

}  // namespace

int launch_gate_f32_heads(const GateArgs& a, int n_heads, int dk, int dox, hipStream_t s) {
#define VLSAT_GH(DK, DOX) if (dk == DK && dox == DOX) run<DK, DOX>(a, n_heads, s);
    VLSAT_GATE_HEAD_GEOMETRIES(VLSAT_GH)
#undef VLSAT_GH
    VLSAT_LAUNCH_CHECK("edge_gate_heads");
    return 0;
}

}  // namespace vlsat
