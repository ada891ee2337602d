// Shared code of the edge-gate kernels of MultiHeadedEdgeAttention.forward (reference network_MMG.py:96-104).  This header is the
// one place that describes the gate's algebra and lane model; the kernels say only what differs between them:
//   edge_gate.hip             fp32 MFMA at the shipped 8 x (64, 64, 32), the VALU kernel for any geometry, and launch_gate
//   edge_gate_f16s.hip        the fp32 mode's split-fp16 sibling of the fp32 MFMA kernel (GateArgs::f16s): three fp16 MFMAs per product
//   edge_gate_bf16.hip        bf16 / fp16 MFMA at the shipped geometry
//   edge_gate_heads.hip       fp32 MFMA template for the other head geometries
//   edge_gate_bf16_heads.hip  bf16 / fp16 MFMA template for the other head geometries
//   gate_agg.h                max aggregation fused into the two shipped kernels
// Which of them runs is decided by gate_select (kernels.h) alone.
//
// Reference, with H heads, d_k = 512 / H query / edge channels and d_o = DIM_ATTEN / H output channels per head (head = FAST axis):
//   q = proj_query(x_i).view(E, d_k, H); k = proj_edge(e).view(E, d_k, H)
//   prob = softmax_dim1( Conv1d(2 d_k -> d_o)( ReLU( Conv1d(2 d_k -> 2 d_k)( cat[q, k] ) ) ) )      [E, d_o, H]
//   gated = prob.reshape(E, H d_o) * proj_value(x_j)
// Algebra (weights prepared once in vlsat_finalize_weights):
//   * the q half of layer 1 depends on the SOURCE node only -> Gq[n, h * 2 d_k + o] (bias included) comes from the node-side GEMM
//     and is gathered here;
//   * proj_edge's rows are permuted so that k arrives head-major, kproj[e, h * d_k + c] == k[e, c, h]: the [E, 512] matrix is a
//     contiguous [H E, d_k] matrix of (edge, head) rows;
//   * value and gated are HEAD-MAJOR as well (the engine permutes proj_value's rows and prop.0's columns once), so the four
//     consecutive channels a lane owns per MFMA row group are one float4 load and one float4 store.
// Per (edge, head) row:  hidden = relu(Gq[src] + W0k . kproj_row);  logits = W3 . hidden + b3;  prob = softmax(logits);
//                        gated[e, h * d_o + m] = prob[m] * value[dst[e], h * d_o + m].
// Lane model: both layers are TRANSPOSED 32x32 MFMA products, so that a lane owns ONE row (li = lane & 31) and, of every block of 32
// output channels, the 16 channels crow32(r, hi) = 8 (r >> 2) + 4 hi + (r & 3), hi = lane >> 5:
//   hidden^T[o][row] : A = W0k from LDS, B = the row's kproj values from HBM;
//   logits^T[m][row] : A = W3, B = hidden straight from the layer-1 accumulator registers (no LDS round trip), 32 hidden outputs
//                      at a time, so only one 32x32 accumulator is live next to the MO = ceil(d_o / 32) logit blocks.
// The softmax over the d_o channels is then in-lane work plus one exchange with lane ^ 32.  Rows of W3 past d_o are staged as zeros
// and their channels masked out of the softmax and the stores (a group of four channels is in or out as a whole: d_o % 8 == 0).
// 16-bit kernels (v_mfma_f32_32x32x16_bf16 / _f16): TERMS = 3 keeps every operand as bf16 hi + lo (PL = 2 weight planes, three
// MFMAs per product: lo.hi, hi.lo, hi.hi), TERMS = 1 rounds once (PL = 1).  k-slot (hi, e) of layer-1 step ks is channel
// c = 16 ks + 8 hi + e; k-slot (hi, e) of layer-2 step (to, half) is o = 32 to + 16 half + 8 (e >> 2) + 4 hi + (e & 3), exactly what
// accumulator registers 8 half + e hold.
#pragma once
#include "gemm_core.h"
#include "kernels.h"

namespace vlsat {

// ---- launchers of the five kernels: called by launch_gate (edge_gate.hip) only, which has checked the arguments ----
int launch_gate_valu(const GateArgs& a, int n_heads, int dk, int dox, hipStream_t s);
int launch_gate_f32(const GateArgs& a, hipStream_t s, const GateArgs* twin);
int launch_gate_f16s(const GateArgs& a, hipStream_t s, const GateArgs* twin);      // GATE_F32 with GateArgs::f16s (edge_gate_f16s.hip)
int launch_gate_f32_heads(const GateArgs& a, int n_heads, int dk, int dox, hipStream_t s);
int launch_gate_16(const GateArgs& a, int terms, int kproj_split, hipStream_t s, const GateArgs* twin);
int launch_gate_16_heads(const GateArgs& a, int n_heads, int dk, int dox, int terms, int kproj_split, hipStream_t s);

// four fp32 -> four 16-bit operands: bf16, or (F16: precision mode fp16_mixed) fp16 clamped to its range
template <bool F16>
__device__ __forceinline__ bf16x4 gate_cv4(const f32x4& x) {
    if constexpr (F16) {
        typedef _Float16 f16x4_g __attribute__((ext_vector_type(4)));
        f32x4 y;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = __builtin_amdgcn_fmed3f(x[c], -65504.f, 65504.f);
        return __builtin_bit_cast(bf16x4, __builtin_convertvector(y, f16x4_g));
    } else {
        return __builtin_convertvector(x, bf16x4);
    }
}
// bf16 remainder of x after its rounding h
__device__ __forceinline__ bf16x4 gate_lo4(const f32x4& x, const bf16x4& h) {
    return __builtin_convertvector(x - __builtin_convertvector(h, f32x4), bf16x4);
}
__device__ __forceinline__ bf16x8 gate_cat(const bf16x4& a, const bf16x4& b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
// eight fp32 -> one 16-bit MFMA operand (hi) and, with two planes, its bf16 remainder (lo; else lo = hi)
template <int PL, bool F16>
__device__ __forceinline__ void gate_split8(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
    const bf16x4 h0 = gate_cv4<F16>(x0), h1 = gate_cv4<F16>(x1);
    hi = gate_cat(h0, h1);
    lo = hi;
    if (PL == 2) lo = gate_cat(gate_lo4(x0, h0), gate_lo4(x1, h1));
}

// This row's d_k = 16 NK1 kproj values as layer-1 B operands.  `krow` = kproj + e * 512, `col` = h * d_k + 8 hi.
// KS: format of kproj -- 0 fp32, 1 split-pair words (common.h pack_split: two v_perm_b32 per pair), 2 bf16 half rows, 3 fp16 half
// rows (eight values = one 16-byte load; TERMS = 1, no low part)
template <int KS, int NK1>
__device__ __forceinline__ void gate_load_kproj(const float* krow, int col, bf16x8 (&zh)[NK1], bf16x8 (&zl)[NK1]) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const float* zrow = krow + col;
#pragma unroll
    for (int ks = 0; ks < NK1; ++ks) {
        if (KS >= 2) {
            zh[ks] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(krow) + (col + 16 * ks) * 2);
            zl[ks] = zh[ks];
            continue;
        }
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(zrow + 16 * ks), x1 = *reinterpret_cast<const f32x4*>(zrow + 16 * ks + 4);
        if (KS == 1) {
            const u32x4 a = __builtin_bit_cast(u32x4, x0), b = __builtin_bit_cast(u32x4, x1);
            u32x4 hh, ll;
            hh[0] = __builtin_amdgcn_perm(a[1], a[0], 0x07060302u); hh[1] = __builtin_amdgcn_perm(a[3], a[2], 0x07060302u);
            hh[2] = __builtin_amdgcn_perm(b[1], b[0], 0x07060302u); hh[3] = __builtin_amdgcn_perm(b[3], b[2], 0x07060302u);
            ll[0] = __builtin_amdgcn_perm(a[1], a[0], 0x05040100u); ll[1] = __builtin_amdgcn_perm(a[3], a[2], 0x05040100u);
            ll[2] = __builtin_amdgcn_perm(b[1], b[0], 0x05040100u); ll[3] = __builtin_amdgcn_perm(b[3], b[2], 0x05040100u);
            zh[ks] = __builtin_bit_cast(bf16x8, hh);
            zl[ks] = __builtin_bit_cast(bf16x8, ll);
        } else {
            gate_split8<2, false>(x0, x1, zh[ks], zl[ks]);
        }
    }
}

// Weight staging by a block of NT threads: w [n_valid][COLS] fp32 -> ROWS rows in LDS, rows past N_VALID zero.
// fp32 rows of PITCH floats ...
template <int ROWS, int N_VALID, int COLS, int PITCH, int NT>
__device__ __forceinline__ void gate_stage_f32_rows(float* sW, const float* w, int tid) {
    for (int i = tid; i < ROWS * (COLS / 4); i += NT) {
        const int r = i / (COLS / 4), c4 = (i % (COLS / 4)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (N_VALID == ROWS || r < N_VALID) v = *reinterpret_cast<const f32x4*>(w + r * COLS + c4);
        *reinterpret_cast<f32x4*>(sW + r * PITCH + c4) = v;
    }
}
// ... or PL planes (hi, lo) of 16-bit values, rows of PITCH bytes, the planes ROWS * PITCH bytes apart
template <int PL, bool F16, int ROWS, int N_VALID, int COLS, int PITCH, int NT>
__device__ __forceinline__ void gate_stage_planes(char* sW, const float* w, int tid) {
    for (int i = tid; i < ROWS * (COLS / 4); i += NT) {
        const int r = i / (COLS / 4), c4 = (i % (COLS / 4)) * 4;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (N_VALID == ROWS || r < N_VALID) x = *reinterpret_cast<const f32x4*>(w + r * COLS + c4);
        const bf16x4 h = gate_cv4<F16>(x);
        *reinterpret_cast<bf16x4*>(sW + r * PITCH + c4 * 2) = h;
        if (PL == 2) *reinterpret_cast<bf16x4*>(sW + ROWS * PITCH + r * PITCH + c4 * 2) = gate_lo4(x, h);
    }
}

// acc += A . B on 16-bit operands: one MFMA, or the three of the hi / lo scheme (al, bl unused with one plane)
template <int PL, bool F16>
__device__ __forceinline__ f32x16 gate_mma(const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl, f32x16 acc) {
    if (PL == 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    return mfma_h<F16>(ah, bh, acc);
}
// layer 1 of one hidden slice on the 16-bit planes: acc = W0k[32 to + li][:] . kproj_row; `ap` = the lane's row of the hi plane + 16 hi
template <int PL, bool F16, int NK1>
__device__ __forceinline__ void gate_layer1_16(f32x16& acc, const char* ap, int plane_bytes, const bf16x8 (&zh)[NK1], const bf16x8 (&zl)[NK1]) {
#pragma unroll
    for (int ks = 0; ks < NK1; ++ks) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap + 32 * ks);
        bf16x8 al = ah;
        if (PL == 2) al = *reinterpret_cast<const bf16x8*>(ap + plane_bytes + 32 * ks);
        acc = gate_mma<PL, F16>(ah, al, zh[ks], zl[ks], acc);
    }
}
// hidden = relu(acc + Gq[src, h * 2 d_k + o]), o = 32 to + 8 r4 + 4 hi + c in register 4 r4 + c; `gq` points at o = 32 to + 4 hi
__device__ __forceinline__ void gate_hidden(const f32x16& acc, const float* gq, float (&hid)[16]) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
        const f32x4 gqv = *reinterpret_cast<const f32x4*>(gq + 8 * r4);
#pragma unroll
        for (int c = 0; c < 4; ++c) hid[r4 * 4 + c] = fmaxf(acc[r4 * 4 + c] + gqv[c], 0.f);
    }
}
// ... and its registers 8 half .. 8 half + 7 as the layer-2 B operand of step (to, half)
template <int PL, bool F16>
__device__ __forceinline__ void gate_hidden_operand(const float (&hid)[16], int half, bf16x8& hh, bf16x8& hl) {
    f32x4 p0, p1;
#pragma unroll
    for (int c = 0; c < 4; ++c) { p0[c] = hid[8 * half + c]; p1[c] = hid[8 * half + 4 + c]; }
    gate_split8<PL, F16>(p0, p1, hh, hl);
}
// layer-2 A operand from a 16-bit W3 plane: W3[m][o .. o + 3] and the same + 8, `wp` = &plane[m][o], o = 32 to + 16 half + 4 hi
__device__ __forceinline__ bf16x8 gate_w3_frag(const char* wp) {
    return gate_cat(*reinterpret_cast<const bf16x4*>(wp), *reinterpret_cast<const bf16x4*>(wp + 16));
}
// layer 2 of step (to, half) on the 16-bit planes for MO logit blocks; `wp` = &hi plane[li][32 to + 16 half + 4 hi], rows of P3 bytes
template <int PL, bool F16, int MO, int P3>
__device__ __forceinline__ void gate_layer2_16(f32x16 (&lg)[MO], const char* wp, int plane_bytes, const bf16x8& hh, const bf16x8& hl) {
#pragma unroll
    for (int mo = 0; mo < MO; ++mo) {
        const bf16x8 wh = gate_w3_frag(wp + mo * 32 * P3);
        bf16x8 wl = wh;
        if (PL == 2) wl = gate_w3_frag(wp + mo * 32 * P3 + plane_bytes);
        lg[mo] = gate_mma<PL, F16>(wh, wl, hh, hl, lg[mo]);
    }
}

// logits start at b3[m], m = 32 mo + 8 r4 + 4 hi + c (zero past d_o)
template <int MO, int DOX>
__device__ __forceinline__ void gate_bias(f32x16 (&lg)[MO], const float* b3, int hi) {
#pragma unroll
    for (int mo = 0; mo < MO; ++mo)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (mo * 32 + 8 * r4 < DOX) b = *reinterpret_cast<const f32x4*>(b3 + mo * 32 + 8 * r4 + 4 * hi);
#pragma unroll
            for (int c = 0; c < 4; ++c) lg[mo][r4 * 4 + c] = b[c];
        }
}
// softmax over the d_o channels m = 32 mo + crow32(r, hi) (+ the other 16 of each block in lane ^ 32): lg <- exp(lg - max), returns
// 1 / sum.  The maximum starts from channel 0 (always valid); a start from -inf gives the same bits -- fmaxf(-inf, x) is x, and a
// NaN logit makes every probability of the row NaN either way.
template <int MO, int DOX>
__device__ __forceinline__ float gate_softmax(f32x16 (&lg)[MO]) {
    float mx = lg[0][0];
#pragma unroll
    for (int mo = 0; mo < MO; ++mo)
#pragma unroll
        for (int r = mo ? 0 : 1; r < 16; ++r)
            if (mo * 32 + 8 * (r >> 2) < DOX) mx = fmaxf(mx, lg[mo][r]);
    mx = half_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int mo = 0; mo < MO; ++mo)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (mo * 32 + 8 * (r >> 2) < DOX) {
                lg[mo][r] = __expf(lg[mo][r] - mx);
                sum += lg[mo][r];
            }
    sum = half_sum(sum);
    return 1.f / sum;
}
// gated row = prob * value: `vrow` / `grow` point at channel 4 hi of the head's d_o values / gated channels; the lane's channels
// 32 mo + 8 r4 + 4 hi + c, c = 0..3, are one float4 per r4.  `prob` (test tap, may be null) is in the reference's [E, d_o, H]
// order, prob_row = e * H d_o.
template <int MO, int DOX>
__device__ __forceinline__ void gate_store(const f32x16 (&lg)[MO], float inv, const float* vrow, float* grow, float* prob, size_t prob_row,
                                           int n_heads, int h, int hi) {
#pragma unroll
    for (int mo = 0; mo < MO; ++mo)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            if (mo * 32 + 8 * r4 >= DOX) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(vrow + mo * 32 + 8 * r4);
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = lg[mo][r4 * 4 + c] * inv * v[c];
            *reinterpret_cast<f32x4*>(grow + mo * 32 + 8 * r4) = o;
        }
    if (prob) {
#pragma unroll
        for (int mo = 0; mo < MO; ++mo)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (mo * 32 + 8 * (r >> 2) < DOX) prob[prob_row + (mo * 32 + crow32(r, hi)) * n_heads + h] = lg[mo][r] * inv;
    }
}
}  // namespace vlsat
