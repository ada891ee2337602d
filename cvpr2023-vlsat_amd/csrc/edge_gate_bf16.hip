// Edge gate on the 16-bit matrix cores at the shipped 8 x (64, 64, 32) geometry (BASELINE configs[2]): algebra, lane model, operand
// construction and the hi / lo scheme are in gate_core.h.  Here: W0k / W3 planes in LDS (ds_read_b128 at pitch 144 B, two 8-byte
// reads per W3 operand), made by the block itself from the fp32 weights (they are tiny); one wave = 32 rows per step (72 MFMAs in
// split-bf16, against 192 64-cycle fp32 ones); the unit mapping head = 4 (unit & 1) + wave, the fused aggregation and the twin launch
// of edge_gate.hip.
#include "gate_core.h"
#include "gate_agg.h"

namespace vlsat {

namespace {

constexpr int GB_P0 = 144;      // W0k plane row pitch (64 bf16 + 16 B)
constexpr int GB_P3 = 264;      // W3 plane row pitch (128 bf16 + 8 B: the 32 rows of a ds_read_b64 land on 32 different bank pairs)

// KS: format of kproj (gate_load_kproj)
// TWIN (round 6): two gates on one edge list in one launch, selected by blockIdx.y (edge_gate.hip)
template <int TERMS, int KS, bool TWIN = false>
__global__ __launch_bounds__(256, TERMS == 1 ? 4 : 2) void edge_gate_bf16_kernel(GateArgs pa, GateArgs pb) {
    const GateArgs& p = (TWIN && blockIdx.y != 0) ? pb : pa;
    constexpr int PL = TERMS == 1 ? 1 : 2;
    constexpr bool F16 = KS == 3;                 // KS 3: kproj holds fp16 half rows, the whole gate runs on fp16 operands (precision mode fp16_mixed; TERMS = 1)
    constexpr int W0B = 128 * GB_P0, W3B = 32 * GB_P3;
    __shared__ __attribute__((aligned(16))) char smem[PL * (W0B + W3B) + 4 * AG_WAVE_BYTES];     // + the fused aggregation's wave buffers (gate_agg.h)
    char* sW0 = smem;                    // [PL][128][144]
    char* sW3 = smem + PL * W0B;         // [PL][32][272]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;

    gate_stage_planes<PL, F16, 128, 128, 64, GB_P0, 256>(sW0, p.w0k, tid);
    gate_stage_planes<PL, F16, 32, 32, 128, GB_P3, 256>(sW3, p.w3, tid);
    float b3f[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) b3f[r] = p.b3[crow32(r, hi)];
    __syncthreads();

    // Work unit = 32 consecutive edges x 4 heads: a wave's 32 rows are 32 EDGES of ONE head (head = 4 (unit & 1) + wave).
    // Edge lists are source-major (reference dataset_3dssg.py:264-266), so the 32 lanes of a Gq load mostly name the same
    // node row: one cache line per instruction instead of 32 (row_map = 0: the older 4 edges x 8 heads per wave).
    const int n_units = 2 * ((p.n_edges + 31) / 32);
    for (int g = blockIdx.x; g < n_units; g += gridDim.x) {
        asm volatile("" ::: "memory");                    // keep the weight fragments out of LICM's hands (edge_gate.hip)
        const int e_raw = p.row_map ? (g >> 1) * 32 + li : g * 16 + wave * 4 + (li >> 3);
        const int h = p.row_map ? (g & 1) * 4 + wave : li & 7;
        const bool valid = e_raw < p.n_edges;
        const int e = valid ? e_raw : p.n_edges - 1;
        bf16x8 zh[4], zl[4];
        if (p.use_edge) gate_load_kproj<KS, 4>(p.kproj + (size_t)e * 512, h * 64 + 8 * hi, zh, zl);
        const int sn = p.src[e], dn = p.dst[e];
        const float* gq = p.node + (size_t)sn * p.ld_node + p.gq_off + h * 128 + 4 * hi;
        f32x16 lg[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[0][r] = b3f[r];
#pragma unroll
        for (int to = 0; to < 4; ++to) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // (USE_GCN_EDGE=false: hidden = relu(Gq), the edge half is absent)
            if (p.use_edge) gate_layer1_16<PL, F16, 4>(acc, sW0 + (to * 32 + li) * GB_P0 + 16 * hi, W0B, zh, zl);
            float hid[16];
            gate_hidden(acc, gq + to * 32, hid);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                bf16x8 hh, hl;
                gate_hidden_operand<PL, F16>(hid, half, hh, hl);
                gate_layer2_16<PL, F16, 1, GB_P3>(lg, sW3 + li * GB_P3 + (to * 32 + 16 * half + 4 * hi) * 2, W3B, hh, hl);
            }
        }
        const float inv = gate_softmax<1, 32>(lg);
        if (p.agg) {                       // fused max aggregation: the gated rows are never stored (gate_agg.h)
            gate_aggregate_max(smem + PL * (W0B + W3B) + wave * AG_WAVE_BYTES, lg[0], inv, p.node + (size_t)dn * p.ld_node + p.v_off + h * 32 + 4 * hi,
                               valid ? sn : -1, li, hi, lane, h, p.agg, p.ld_agg);
        } else if (valid) {
            gate_store<1, 32>(lg, inv, p.node + (size_t)dn * p.ld_node + p.v_off + h * 32 + 4 * hi, p.gated + (size_t)e * 256 + h * 32 + 4 * hi,
                              p.prob, (size_t)e * 256, 8, h, hi);
        }
    }
}

}  // namespace

int launch_gate_16(const GateArgs& a, int terms, int kproj_split, hipStream_t s, const GateArgs* twin) {
    const GateArgs& b = twin ? *twin : a;
    const int n_groups = a.row_map ? 2 * ((a.n_edges + 31) / 32) : (a.n_edges + 15) / 16;
    // persistent grid (weights staged once per block): three blocks per CU; the single-rounding kernel holds four (128 VGPRs,
    // 37 KB of LDS) and 1024 measured 0.7 % faster per step than 768 or 1280 with the aggregation fused in
    const int cap = a.grid_cap > 0 ? a.grid_cap : terms == 1 ? 1024 : 768;
    const int grid = n_groups < cap ? n_groups : cap;
#define VLSAT_GB(T, K) do { if (twin) hipLaunchKernelGGL((edge_gate_bf16_kernel<T, K, true>), dim3(grid, 2), dim3(256), 0, s, a, b); \
                            else hipLaunchKernelGGL((edge_gate_bf16_kernel<T, K, false>), dim3(grid), dim3(256), 0, s, a, a); } while (0)
    if (terms == 3) { if (kproj_split) VLSAT_GB(3, 1); else VLSAT_GB(3, 0); }
    else            { if (kproj_split == 3) VLSAT_GB(1, 3); else if (kproj_split == 2) VLSAT_GB(1, 2); else if (kproj_split) VLSAT_GB(1, 1); else VLSAT_GB(1, 0); }       // (3: fp16 half rows)
#undef VLSAT_GB
    VLSAT_LAUNCH_CHECK("edge_gate_bf16");
    return 0;
}

}  // namespace vlsat
