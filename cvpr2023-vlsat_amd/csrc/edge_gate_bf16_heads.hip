// Edge gate on the 16-bit matrix cores for the head geometries other than the shipped 8 x (64, 64, 32): the 16-bit twin of
// edge_gate_heads.hip (work units, MO logit blocks, 8-wave block at d_k = 128) on the operands of edge_gate_bf16.hip (gate_core.h).
// Template: d_k in {32, 64, 128} (d_k / 16 k-steps in layer 1, 2 d_k / 32 hidden slices), d_o = DIM_ATTEN / heads.  Planes of
// W0k [2 d_k][d_k] and W3 [d_o][2 d_k] in LDS (row pitches 2 d_k + 16 and 4 d_k + 8 bytes as in edge_gate_bf16.hip); at d_k = 128
// they take 103 KB per plane set: one 8-wave block per CU, and no split-bf16 variant (two plane sets do not fit) -- gate_select
// keeps that combination on the fp32 template.
#include "gate_core.h"

namespace vlsat {

namespace {

// KS: format of kproj (gate_load_kproj)
template <int TERMS, int KS, int DK, int DOX>
__global__ __launch_bounds__(DK == 128 ? 512 : 256, DK == 128 ? 1 : 2) void edge_gate_bf16_hd_kernel(GateArgs p, int n_heads) {
    constexpr int PL = TERMS == 1 ? 1 : 2;
    constexpr bool F16 = KS == 3;                 // KS 3: fp16 half rows and fp16 operands (precision mode fp16_mixed; TERMS = 1), as in edge_gate_bf16.hip
    constexpr int HID = 2 * DK, TO = HID / 32, MO = (DOX + 31) / 32, NK1 = DK / 16;
    constexpr int P0 = 2 * DK + 16, P3 = 2 * HID + 8;        // plane row pitches in bytes
    constexpr int W0B = HID * P0, W3B = MO * 32 * P3;
    constexpr int NT = DK == 128 ? 512 : 256, NW = NT / 64;
    static_assert(DOX % 8 == 0 && PL * (W0B + W3B) <= 160 * 1024, "gate geometry");
    __shared__ __attribute__((aligned(16))) char smem[PL * (W0B + W3B)];
    char* sW0 = smem;                    // [PL][HID][P0]
    char* sW3 = smem + PL * W0B;         // [PL][MO * 32][P3]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int A = n_heads * DOX;

    gate_stage_planes<PL, F16, HID, HID, DK, P0, NT>(sW0, p.w0k, tid);
    gate_stage_planes<PL, F16, MO * 32, DOX, HID, P3, NT>(sW3, p.w3, tid);
    __syncthreads();

    const long n_wu = (long)((p.n_edges + 31) / 32) * n_heads;          // wave units: (block of 32 edges, head)
    for (long u = blockIdx.x; u * NW < n_wu; u += gridDim.x) {
        asm volatile("" ::: "memory");                    // keep the weight fragments out of LICM's hands (edge_gate.hip)
        const long wu = u * NW + wave;
        if (wu >= n_wu) continue;                         // (no barrier in this loop)
        const int h = (int)(wu % n_heads);
        const int e_raw = (int)(wu / n_heads) * 32 + li;
        const bool valid = e_raw < p.n_edges;
        const int e = valid ? e_raw : p.n_edges - 1;
        bf16x8 zh[NK1], zl[NK1];
        if (p.use_edge) gate_load_kproj<KS, NK1>(p.kproj + (size_t)e * 512, h * DK + 8 * hi, zh, zl);
        const int sn = p.src[e], dn = p.dst[e];
        const float* gq = p.node + (size_t)sn * p.ld_node + p.gq_off + h * HID + 4 * hi;
        f32x16 lg[MO];
        gate_bias<MO, DOX>(lg, p.b3, hi);
#pragma unroll(DK == 128 ? 1 : TO)
        for (int to = 0; to < TO; ++to) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // (USE_GCN_EDGE=false: hidden = relu(Gq), the edge half is absent)
            if (p.use_edge) gate_layer1_16<PL, F16, NK1>(acc, sW0 + (to * 32 + li) * P0 + 16 * hi, W0B, zh, zl);
            float hid[16];
            gate_hidden(acc, gq + to * 32, hid);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                bf16x8 hh, hl;
                gate_hidden_operand<PL, F16>(hid, half, hh, hl);
                gate_layer2_16<PL, F16, MO, P3>(lg, sW3 + li * P3 + (to * 32 + 16 * half + 4 * hi) * 2, W3B, hh, hl);
            }
        }
        const float inv = gate_softmax<MO, DOX>(lg);
        if (valid)
            gate_store<MO, DOX>(lg, inv, p.node + (size_t)dn * p.ld_node + p.v_off + h * DOX + 4 * hi, p.gated + (size_t)e * A + h * DOX + 4 * hi,
                                p.prob, (size_t)e * A, n_heads, h, hi);
    }
}

template <int TERMS, int KS, int DK, int DOX>
int run(const GateArgs& a, int n_heads, hipStream_t s) {
    constexpr int NT = DK == 128 ? 512 : 256, NW = NT / 64;
    const long n_wu = (long)((a.n_edges + 31) / 32) * n_heads, units = (n_wu + NW - 1) / NW;
    const long cap = a.grid_cap > 0 ? a.grid_cap : (DK == 128 ? 256 : 768);      // persistent: the planes are made once per block
    hipLaunchKernelGGL((edge_gate_bf16_hd_kernel<TERMS, KS, DK, DOX>), dim3((unsigned)std::min(units, cap)), dim3(NT), 0, s, a, n_heads);
    return 0;
}

template <int DK, int DOX>
int pick(const GateArgs& a, int n_heads, int terms, int ks, hipStream_t s) {
    if (terms == 3) {
        if constexpr (DK == 128) return fail(-1, "edge_gate_bf16: no split-bf16 kernel at d_k = 128");      // (two plane sets do not fit the LDS; launch_gate has refused it)
        else return ks ? run<3, 1, DK, DOX>(a, n_heads, s) : run<3, 0, DK, DOX>(a, n_heads, s);
    }
    return ks == 3 ? run<1, 3, DK, DOX>(a, n_heads, s) : ks == 2 ? run<1, 2, DK, DOX>(a, n_heads, s) : ks ? run<1, 1, DK, DOX>(a, n_heads, s) : run<1, 0, DK, DOX>(a, n_heads, s);
}

}  // namespace

int launch_gate_16_heads(const GateArgs& a, int n_heads, int dk, int dox, int terms, int kproj_split, hipStream_t s) {
    int r = 0;
#define VLSAT_GH(DK, DOX) if (dk == DK && dox == DOX) r = pick<DK, DOX>(a, n_heads, terms, kproj_split, s);
    VLSAT_GATE_HEAD_GEOMETRIES(VLSAT_GH)
#undef VLSAT_GH
    if (r) return r;
    VLSAT_LAUNCH_CHECK("edge_gate_bf16_heads");
    return 0;
}

}  // namespace vlsat
