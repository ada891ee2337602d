// Scene-graph Recall@K / mR@K of the reference's evaluate_triplet_recallk / evaluate_triplet_mrecallk
// (src/utils/eval_utils_recall.py, called per scene by process_val2 / process_val3, SGFN_MMG/model_in21k.py:439-500):
// PredCls (conf = r_k) and SGCls (conf = fl(fl(s_i * o_j) * r_k), the reference's two einsums, no FMA), each with the
// graph constraint (topk_each = 1) and without (topk_each = 100), at K = 20, 50, 100.
// The reference sorts the 160 x 160 x 26 = 665 600-entry product of every edge and keeps a running global top-K; all a hit needs
// is a COUNT: edge e hits at K when some correct entry c of e is one of its topk_each candidates and fewer than K candidates of
// the scene are strictly greater than c (ties at the boundary resolve optimistically, as in tri_rank_kernel).  With T_K = the K-th
// largest candidate of the scene that is c >= T_K; the candidate condition is c >= max of e for GC and implied by c >= T_K for NGC
// (K <= topk_each).  The conditions are monotone in c, so only an edge's best correct entry g_e matters:
//   PredCls  g = max_{k in gt} r_k                      SGCls  g = fl(fl(s_gt * o_gt) * max_{k in gt} r_k)
// Three launches after the per-node sort of eval_ranks.hip, values compared as order-preserving 32-bit keys (never indices; key,
// bisection and tie rule: select_core.h):
//   launch_scene_edge_ptr  (scene_graph.hip) edge offsets of every scene (edges arrive grouped by scene in ascending order)
//   recall_edge_kernel one wave per edge: its gt mask, g keys, sorted predicate keys and -- SGCls NGC -- its top 100 products.
//                      An entry at sorted position (i, j, k) of (s, o, r) is dominated by (i+1)(j+1)(k+1) - 1 others, so the top
//                      100 lie in the 1 365 triples with (i+1)(j+1)(k+1) <= 100 (k < 32): evaluated, the 100th largest selected by
//                      bisection on the key bits, the rest sorted by counting.  The 665 600 products are never formed.
//   recall_scene_kernel one block per (scene, variant): T_20 / T_50 / T_100 by bisection over the per-edge sorted lists (a binary
//                      search per list and trial), then the hits, counted in LDS and written as the scene's int64 row.
// No atomics on global memory, no fill of the output: every field of every row is written by exactly one block.
// Integer / latency-bound work: no MFMA.
#include "common.h"
#include "kernels.h"
#include "select_core.h"

namespace vlsat {

namespace {

constexpr int RK_TOP = 100;                      // topk_each of the NGC variants = the largest K
constexpr int RK_MAX_R = 32;
constexpr int RK_SCENE_THREADS = 1024;

constexpr int RK_NT = tri_count(RK_TOP, RK_MAX_R);   // 1 365
constexpr int RK_PER = (RK_NT + 63) / 64;        // triples per lane
__constant__ TriTable<RK_TOP, RK_MAX_R> c_tri = make_tri<RK_TOP, RK_MAX_R>();

}  // namespace

// one wave per edge, 4 edges per block
__global__ __launch_bounds__(256) void recall_edge_kernel(const float* __restrict__ probs, const float* __restrict__ sorted, int Ks,
                                                          const float* __restrict__ rel, const int64_t* __restrict__ gt_cls,
                                                          const int64_t* __restrict__ gt_rel, const int64_t* __restrict__ edges, int N,
                                                          int E, int C, int R, int do_sg, int do_ngc, uint32_t* __restrict__ gtmask,
                                                          uint32_t* __restrict__ gkey_p, uint32_t* __restrict__ plist,
                                                          uint32_t* __restrict__ gkey_s, uint32_t* __restrict__ mkey_s,
                                                          uint32_t* __restrict__ slist) {
    __shared__ float s_rs[4][RK_MAX_R];           // the edge's predicate scores, descending
    __shared__ float s_a[4][RK_TOP], s_b[4][RK_TOP];
    __shared__ uint32_t s_top[4][RK_TOP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, e = blockIdx.x * 4 + w;
    const bool live = e < E;                       // (no early return: the block synchronises twice)
    int a = 0, b = 0;
    unsigned mask = 0;
    float gr = 0.f;
    if (live) {
        a = clampi(edges[2 * (size_t)e], 0, N - 1);
        b = clampi(edges[2 * (size_t)e + 1], 0, N - 1);
        const float rv = lane < R ? rel[(size_t)e * R + lane] : -INFINITY;
        const bool is_gt = lane < R && gt_rel[(size_t)e * R + lane] == 1;
        mask = (unsigned)__ballot(is_gt);
        const int rk = rank_desc_in_wave(rv, lane, R);
        gr = wave_max(is_gt ? rv : -INFINITY);    // best gt predicate score (-inf: no gt relation)
        if (lane < R) {
            s_rs[w][rk] = rv;
            plist[(size_t)e * R + rk] = fkey(rv);
        }
        if (lane == 0) {
            gtmask[e] = mask;
            gkey_p[e] = mask ? fkey(gr) : 0u;
        }
        if (do_sg)
            for (int i = lane; i < Ks; i += 64) {
                s_a[w][i] = sorted[(size_t)a * Ks + i];
                s_b[w][i] = sorted[(size_t)b * Ks + i];
            }
    }
    __syncthreads();
    if (!do_sg) return;                            // (uniform)
    if (live && lane == 0) {
        mkey_s[e] = fkey(__fmul_rn(__fmul_rn(s_a[w][0], s_b[w][0]), s_rs[w][0]));
        const float gs = __fmul_rn(probs[(size_t)a * C + clampi(gt_cls[a], 0, C - 1)], probs[(size_t)b * C + clampi(gt_cls[b], 0, C - 1)]);
        gkey_s[e] = mask ? fkey(__fmul_rn(gs, gr)) : 0u;
    }
    if (!do_ngc) return;
    uint32_t v[RK_PER];
#pragma unroll
    for (int t = 0; t < RK_PER; ++t) {
        const int idx = lane + 64 * t;
        uint32_t key = 0;
        if (live && idx < RK_NT) {
            const uint32_t tr = c_tri.v[idx];
            const int i = tr & 0xff, j = (tr >> 8) & 0xff, k = tr >> 16;
            if (i < Ks && j < Ks && k < R) key = fkey(__fmul_rn(__fmul_rn(s_a[w][i], s_b[w][j]), s_rs[w][k]));
        }
        v[t] = key;
    }
    const uint32_t T = wave_kth_largest(v, RK_TOP);                // the 100th largest key (0 when the edge has fewer than 100 entries)
    // the (< 100) keys above T, compacted in lane order
    int mine = 0;
#pragma unroll
    for (int t = 0; t < RK_PER; ++t) mine += v[t] > T;
    int off = wave_scan_incl(mine, lane);
    const int above = __shfl(off, 63);
    off -= mine;
#pragma unroll
    for (int t = 0; t < RK_PER; ++t)
        if (v[t] > T) s_top[w][off++] = v[t];
    __syncthreads();
    if (!live) return;
    uint32_t* out = slist + (size_t)e * RK_TOP;
    for (int i = lane; i < RK_TOP; i += 64) {
        if (i < above) {
            const uint32_t x = s_top[w][i];
            int rank = 0;
            for (int q = 0; q < above; ++q) {
                const uint32_t y = s_top[w][q];
                rank += y > x || (y == x && q < i);
            }
            out[rank] = x;
        } else {
            out[i] = T;                            // ties of T fill the list up to 100
        }
    }
}

// block (scene s, variant v); row layout of counts_out: see launch_eval_recallk
__global__ __launch_bounds__(RK_SCENE_THREADS) void recall_scene_kernel(const int32_t* __restrict__ ptr, const uint32_t* __restrict__ gtmask,
                                                                       const uint32_t* __restrict__ gkey_p, const uint32_t* __restrict__ plist,
                                                                       const uint32_t* __restrict__ gkey_s, const uint32_t* __restrict__ mkey_s,
                                                                       const uint32_t* __restrict__ slist, int E, int R, int vmask,
                                                                       long long* __restrict__ out) {
    constexpr int NW = RK_SCENE_THREADS / 64;
    __shared__ unsigned s_cnt[3 + 3 * RK_MAX_R];  // hit@K, class_hit@K[R]
    __shared__ unsigned s_gt[1 + RK_MAX_R];       // gt_edges, gt_per_class[R]
    __shared__ int s_red[3][NW];
    const int s = blockIdx.x, v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int F = 1 + R + 4 * (3 + 3 * R);
    for (int i = tid; i < 3 + 3 * RK_MAX_R; i += blockDim.x) s_cnt[i] = 0;
    for (int i = tid; i < 1 + RK_MAX_R; i += blockDim.x) s_gt[i] = 0;
    const int e0 = clampi(ptr[s], 0, E), e1 = max(e0, clampi(ptr[s + 1], 0, E));
    const bool on = (vmask >> v) & 1;
    const uint32_t* list = v < 2 ? plist : v == 2 ? mkey_s : slist;
    const int stride = v < 2 ? R : v == 2 ? 1 : RK_TOP;
    const int len = v == 1 ? R : v == 3 ? RK_TOP : 1;
    const uint32_t* gk = v < 2 ? gkey_p : gkey_s;
    const bool gc = v == 0 || v == 2;
    const int Ks[3] = {20, 50, 100};
    uint32_t key[3] = {0u, 0u, 0u};               // T_K; 0 = the scene has fewer than K candidates
    if (on) {
        for (int bit = 31; bit >= 0; --bit) {
            uint32_t trial[3];
            int c[3] = {0, 0, 0};
#pragma unroll
            for (int q = 0; q < 3; ++q) trial[q] = key[q] | (1u << bit);
            for (int e = e0 + tid; e < e1; e += blockDim.x) {
                const uint32_t* p = list + (size_t)e * stride;
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] += count_ge(p, len, trial[q]);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                c[q] = wave_sum_i(c[q]);
                if (lane == 0) s_red[q][wv] = c[q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                int tot = 0;
                for (int i = 0; i < NW; ++i) tot += s_red[q][i];
                if (tot >= Ks[q]) key[q] = trial[q];
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int e = e0 + tid; e < e1; e += blockDim.x) {
        const unsigned m = gtmask[e];
        if (!m) continue;
        if (v == 0) {
            atomicAdd(&s_gt[0], 1u);
            for (unsigned x = m; x; x &= x - 1) atomicAdd(&s_gt[1 + __ffs(x) - 1], 1u);
        }
        if (!on) continue;
        const uint32_t g = gk[e];
        if (gc && g < list[(size_t)e * stride]) continue;          // not the edge's top entry: no candidate
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (g < key[q]) continue;
            atomicAdd(&s_cnt[q], 1u);
            for (unsigned x = m; x; x &= x - 1) atomicAdd(&s_cnt[3 + q * R + __ffs(x) - 1], 1u);
        }
    }
    __syncthreads();
    long long* row = out + (size_t)s * F;
    if (v == 0)
        for (int i = tid; i < 1 + R; i += blockDim.x) row[i] = s_gt[i];
    long long* vr = row + 1 + R + v * (3 + 3 * R);
    for (int i = tid; i < 3 + 3 * R; i += blockDim.x) vr[i] = s_cnt[i];
}

size_t eval_recallk_scratch_bytes(int64_t N, int64_t E, int C, int R, int n_scenes) {
    const int64_t Ks = C < RK_TOP ? C : RK_TOP;
    return align_up((size_t)N * Ks * sizeof(float), 256) + align_up((size_t)(n_scenes + 1) * sizeof(int32_t), 256) +
           4 * align_up((size_t)E * sizeof(uint32_t), 256) + align_up((size_t)E * R * sizeof(uint32_t), 256) +
           align_up((size_t)E * RK_TOP * sizeof(uint32_t), 256);
}

int launch_eval_recallk(const float* obj_probs, const float* rel, const int64_t* gt_cls, const int64_t* gt_rel, const int64_t* edges,
                        const int64_t* batch_ids, int N, int E, int C, int R, int n_scenes, int vmask, void* scratch,
                        long long* counts, hipStream_t s) {
    if (R <= 0 || R > RK_MAX_R || C <= 0 || C > 1024) return fail(-1, "eval_recallk: 1..1024 object and 1..32 relation classes");
    if (n_scenes < 0 || N < 0 || E < 0 || (E > 0 && N <= 0)) return fail(-1, "eval_recallk: bad sizes");
    if (vmask & ~15) return fail(-1, "eval_recallk: variants_mask has bits above 15");
    if (n_scenes == 0) return 0;
    const int Ks = C < RK_TOP ? C : RK_TOP;
    char* p = static_cast<char*>(scratch);
    float* sorted = reinterpret_cast<float*>(p);                 p += align_up((size_t)N * Ks * sizeof(float), 256);
    int32_t* ptr = reinterpret_cast<int32_t*>(p);                p += align_up((size_t)(n_scenes + 1) * sizeof(int32_t), 256);
    uint32_t* gtmask = reinterpret_cast<uint32_t*>(p);           p += align_up((size_t)E * sizeof(uint32_t), 256);
    uint32_t* gkey_p = reinterpret_cast<uint32_t*>(p);           p += align_up((size_t)E * sizeof(uint32_t), 256);
    uint32_t* gkey_s = reinterpret_cast<uint32_t*>(p);           p += align_up((size_t)E * sizeof(uint32_t), 256);
    uint32_t* mkey_s = reinterpret_cast<uint32_t*>(p);           p += align_up((size_t)E * sizeof(uint32_t), 256);
    uint32_t* plist = reinterpret_cast<uint32_t*>(p);            p += align_up((size_t)E * R * sizeof(uint32_t), 256);
    uint32_t* slist = reinterpret_cast<uint32_t*>(p);
    const int do_sg = (vmask & 12) != 0, do_ngc = (vmask & 8) != 0;
    const int rp = launch_scene_edge_ptr(edges, batch_ids, nullptr, N, E, n_scenes, ptr, s);
    if (rp) return rp;
    if (E > 0) {
        if (do_sg) {
            const int rc = launch_sort_probs(obj_probs, N, C, Ks, sorted, s);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(recall_edge_kernel, dim3((E + 3) / 4), dim3(256), 0, s, obj_probs, sorted, Ks, rel, gt_cls, gt_rel, edges, N, E,
                           C, R, do_sg, do_ngc, gtmask, gkey_p, plist, gkey_s, mkey_s, slist);
        VLSAT_LAUNCH_CHECK("recallk edge");
    }
    hipLaunchKernelGGL(recall_scene_kernel, dim3(n_scenes, 4), dim3(RK_SCENE_THREADS), 0, s, ptr, gtmask, gkey_p, plist, gkey_s, mkey_s,
                       slist, E, R, vmask, counts);
    VLSAT_LAUNCH_CHECK("recallk scene");
    return 0;
}

}  // namespace vlsat
