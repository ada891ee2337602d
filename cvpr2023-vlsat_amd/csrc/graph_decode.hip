// The decoded scene graph: per node its n_labels most probable classes, per scene the predicates the model ASSERTS -- the decision
// rule the reference's evaluation states and never applies to an output (src/utils/eva_utils_acc.py:42-63, 176-181: a multi-label
// edge predicts "none" exactly when no predicate reaches the confidence threshold; get_gt :19-22: class 0 of a single-label edge is
// "none").  No labels are read by the decode; the counts kernel compares the same decisions with ground truth.
//   multi_label = 1   predicate k of edge e is asserted iff rel[e, k] >= thr[k] (fp32 compare, equality passes)
//   multi_label = 0   k* = lowest index of the row maximum; asserted iff k* != 0 and rel[e, k*] >= thr[k*]
//   score_mode 0      score(e, k) = rel[e, k];   score_mode 1: fl(fl(s * o) * rel[e, k]), s / o the top-1 probabilities of the two
//                     nodes (two roundings, no FMA: the convention of scene_graph.hip and eval_recall.hip)
//   gd_node_kernel    one wave per node: n_labels rounds of a wave-wide arg-max (value descending, class ascending)
//   gd_edge_kernel    32 lanes per edge, lane = predicate: the COMPACTION pass -- the asserted predicates of an edge, ordered by
//                     (score descending, predicate ascending), as order-preserving keys (select_core.h; 0 = "not asserted") into
//                     the edge's slots, and their number
//   gd_scene_kernel   one block per scene: n_total by a block sum; when the cap bites, the max_rel-th largest key by bisection on
//                     the key bits over the per-edge sorted lists (asserted pairs only); a gather of the keys above it plus the
//                     first ones equal to it in (edge, predicate) order, by two block scans; a bitonic sort of <= 4096 rows in LDS
//                     on (key, edge, predicate); one write of every field of the scene, rows past n_valid included.
// The kept rows are the first n_valid of the scene's asserted pairs under the total order (score descending, edge ascending,
// predicate ascending): fully determined.  No global atomics, no fill, no host synchronisation, no allocation in the decode.
//   gd_counts_kernel  the same decisions before the cap against ground truth: per predicate tp, fp, fn, then nodes and nodes whose
//                     top-1 class is the gt class, added to a uint64 vector -- wave sums, one LDS atomic per counter and wave, one
//                     64-bit global atomic per counter and block: exact and order-independent.
// Integer / latency-bound work: no MFMA.
#include "common.h"
#include "decode_core.h"
#include "kernels.h"
#include "select_core.h"

namespace vlsat {

namespace {

constexpr int GD_MAX_R = 32;
constexpr int GD_MAX_C = 1024;
constexpr int GD_MAX_LABELS = 8;
constexpr int GD_MAX_REL = 4096;                 // largest max_rel: rows of the LDS sort
constexpr int GD_SCENE_THREADS = 1024;
constexpr int GD_PER_LANE = GD_MAX_C / 64;       // classes per lane of the node wave

// the decision of lane k (< 32) about predicate k of its edge; r = rel[e, k] (any value for k >= R); all 32 lanes of the group call
__device__ __forceinline__ bool gd_asserted(float r, int k, int R, const float* __restrict__ thr, int multi) {
    const bool in = k < R;
    const bool pass = in && r >= thr[in ? k : 0];
    if (multi) return pass;
    const int bi = gd_pick(r, k, R);               // arg-max of the row, lowest index among equals (every lane calls: shuffles)
    return pass && k == bi && k != 0;
}

}  // namespace

// labels[n, 0:K] / lp[n, 0:K] = the K largest entries of probs[n, :] in descending order (equal values in ascending class order);
// one wave per node, K <= min(C, 8) rounds of a wave arg-max over the classes each lane holds in registers
__global__ __launch_bounds__(256) void gd_node_kernel(const float* __restrict__ probs, int N, int C, int K, int32_t* __restrict__ labels,
                                                      float* __restrict__ lp) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                            // (a whole wave: nothing below synchronises the block)
    float v[GD_PER_LANE];
    unsigned avail = 0;
#pragma unroll
    for (int t = 0; t < GD_PER_LANE; ++t) {
        const int c = lane + 64 * t;
        v[t] = c < C ? probs[(size_t)n * C + c] : 0.f;
        avail |= (unsigned)(c < C) << t;
    }
    for (int r = 0; r < K; ++r) {
        float bv = 0.f;
        int bi = INT32_MAX;                        // INT32_MAX: this lane has no class left
#pragma unroll
        for (int t = 0; t < GD_PER_LANE; ++t)
            if (((avail >> t) & 1) && (bi == INT32_MAX || v[t] > bv)) {
                bv = v[t];
                bi = lane + 64 * t;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != INT32_MAX && (bi == INT32_MAX || ov > bv || (ov == bv && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi != INT32_MAX && (bi & 63) == lane) avail &= ~(1u << (bi >> 6));
        if (lane == 0) {
            labels[(size_t)n * K + r] = bi;
            lp[(size_t)n * K + r] = bv;
        }
    }
}

// 32 lanes per edge, 8 edges per block.  top[n * ldt] = top-1 probability of node n (score_mode 1: the label_probs just written).
// keys[e * R + j], preds[e * R + j], j < cnt[e]: the asserted predicates of edge e by (score descending, predicate ascending)
__global__ __launch_bounds__(256) void gd_edge_kernel(const float* __restrict__ rel, const int64_t* __restrict__ edges,
                                                      const float* __restrict__ thr, const float* __restrict__ top, int ldt, int N, int E,
                                                      int R, int multi, int score_mode, uint32_t* __restrict__ keys,
                                                      uint8_t* __restrict__ preds, int32_t* __restrict__ cnt) {
    const int k = threadIdx.x & 31, e = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = e < E;
    const size_t el = live ? e : 0, row = el * R;  // (a dead group reads edge 0 and writes nothing: the shuffles want every lane)
    const float r = k < R ? rel[row + k] : 0.f;
    const bool on = gd_asserted(r, k, R, thr, multi);
    float sc = r;
    if (score_mode == 1) {
        const int a = clampi(edges[2 * el], 0, N - 1), b = clampi(edges[2 * el + 1], 0, N - 1);
        sc = __fmul_rn(__fmul_rn(top[(size_t)a * ldt], top[(size_t)b * ldt]), r);
    }
    const uint32_t key = on ? fkey(sc) : 0u;
    int rank = 0, n = 0;
    for (int q = 0; q < R; ++q) {
        const uint32_t kq = __shfl(key, q, 32);
        n += kq != 0;
        rank += kq > key || (kq == key && q < k);  // (only asserted lanes use their rank: key != 0 there)
    }
    if (!live) return;
    if (on) {
        keys[row + rank] = key;
        preds[row + rank] = (uint8_t)k;
    }
    if (k == 0) cnt[e] = n;
}

// block = scene; thread = edge while selecting, = row while sorting and writing.  A row of the sort is
// key << 32 | ~(edge << 5 | predicate): descending rows = (score descending, edge ascending, predicate ascending); 0 = padding.
__global__ __launch_bounds__(GD_SCENE_THREADS) void gd_scene_kernel(const int32_t* __restrict__ ptr, const uint32_t* __restrict__ keys,
                                                                   const uint8_t* __restrict__ preds, const int32_t* __restrict__ cnt,
                                                                   int E, int R, int K, int32_t* __restrict__ rels,
                                                                   float* __restrict__ score, int32_t* __restrict__ nvalid,
                                                                   int32_t* __restrict__ ntotal) {
    constexpr int NW = GD_SCENE_THREADS / 64;
    __shared__ unsigned long long s_row[GD_MAX_REL];
    __shared__ int s_red[NW];
    __shared__ long long s_scan[NW];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int e0 = clampi(ptr[s], 0, E), e1 = max(e0, clampi(ptr[s + 1], 0, E));
    int c = 0;
    for (int e = e0 + tid; e < e1; e += GD_SCENE_THREADS) c += cnt[e];
    const int total = block_sum<GD_SCENE_THREADS>(c, s_red);               // n_total (the launcher bounds E * R by INT32_MAX)
    const int Kk = total < K ? total : K;          // n_valid
    int P = 1;                                     // rows of the sort: the power of two >= Kk
    while (P < Kk) P <<= 1;
    if (Kk > 0) {                                  // (uniform)
        // the Kk largest keys (all of them when the cap does not bite: no bisection); equal keys of one edge lie in ascending
        // predicate order, so the (edge, slot) order of the ties is (edge, predicate) order
        select_topk_lists<GD_SCENE_THREADS>(keys, R, [&](int e) { return cnt[e]; }, e0, e1, Kk, total > K, s_red, s_scan, [&](int pos, int e, int j) {
            const size_t i = (size_t)e * R + j;
            s_row[pos] = ((unsigned long long)keys[i] << 32) | (0xFFFFFFFFu - (((uint32_t)e << 5) | preds[i]));
        });
        for (int i = Kk + tid; i < P; i += GD_SCENE_THREADS) s_row[i] = 0;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)           // bitonic sort, descending (rows are pairwise distinct)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += GD_SCENE_THREADS) {
                    const int x = i ^ j;
                    if (x > i) {
                        const unsigned long long a = s_row[i], b = s_row[x];
                        if (((i & k) == 0) ? a < b : a > b) {
                            s_row[i] = b;
                            s_row[x] = a;
                        }
                    }
                }
                __syncthreads();
            }
    }
    if (tid == 0) {
        nvalid[s] = Kk;
        ntotal[s] = total;
    }
    int32_t* orow = rels + (size_t)s * K * 2;
    float* osc = score + (size_t)s * K;
    for (int i = tid; i < K; i += GD_SCENE_THREADS) {
        if (i < Kk) {
            const unsigned long long x = s_row[i];
            const uint32_t id = 0xFFFFFFFFu - (uint32_t)x;
            orow[2 * i] = (int32_t)(id >> 5);
            orow[2 * i + 1] = (int32_t)(id & 31);
            osc[i] = unkey((uint32_t)(x >> 32));
        } else {                                   // rows past n_valid
            orow[2 * i] = orow[2 * i + 1] = -1;
            osc[i] = 0.f;
        }
    }
}

// out[3 k + {0, 1, 2}] += tp, fp, fn of predicate k; out[3 R] += nodes; out[3 R + 1] += nodes whose arg-max class (lowest index
// among equals) is gt_cls.  gt_rel: int64 multi-hot [E, R] (multi) | int64 [E], 0 = none (single label: row 0 stays zero).
// Blocks [0, nbe) walk the edges (32 lanes per edge, lane = predicate), the others the nodes (one wave per node).
__global__ __launch_bounds__(256) void gd_counts_kernel(const float* __restrict__ probs, const float* __restrict__ rel,
                                                        const int64_t* __restrict__ gt_cls, const int64_t* __restrict__ gt_rel,
                                                        const float* __restrict__ thr, int N, int E, int C, int R, int multi, int nbe,
                                                        unsigned long long* __restrict__ out) {
    __shared__ unsigned s_h[3 * GD_MAX_R + 2];
    const int n_out = 3 * R + 2;
    for (int i = threadIdx.x; i < n_out; i += 256) s_h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x < nbe) {
        const int k = threadIdx.x & 31;
        unsigned tp = 0, fp = 0, fn = 0;
        for (int e0 = blockIdx.x * 8; e0 < E; e0 += nbe * 8) {     // (uniform trip count: every lane takes part in the shuffles)
            const int e = e0 + (threadIdx.x >> 5);
            const bool live = e < E;
            const size_t el = live ? e : 0, row = el * R;
            const bool on = gd_asserted(k < R ? rel[row + k] : 0.f, k, R, thr, multi) && live;
            const bool gt = live && k < R && (multi ? gt_rel[row + k] == 1 : (k != 0 && gt_rel[el] == k));
            tp += on && gt;
            fp += on && !gt;
            fn += gt && !on;
        }
        tp += __shfl_xor(tp, 32);                  // the two edges of a wave
        fp += __shfl_xor(fp, 32);
        fn += __shfl_xor(fn, 32);
        if (lane < R) {
            if (tp) atomicAdd(s_h + 3 * lane, tp);
            if (fp) atomicAdd(s_h + 3 * lane + 1, fp);
            if (fn) atomicAdd(s_h + 3 * lane + 2, fn);
        }
    } else {
        int nodes = 0, hit = 0;
        for (int n = ((int)blockIdx.x - nbe) * 4 + (threadIdx.x >> 6); n < N; n += ((int)gridDim.x - nbe) * 4) {
            float bv;
            const int bi = gd_top1(probs + (size_t)n * C, C, lane, bv);
            ++nodes;
            hit += gt_cls[n] == bi;
        }
        if (lane == 0) {
            if (nodes) atomicAdd(s_h + 3 * R, (unsigned)nodes);
            if (hit) atomicAdd(s_h + 3 * R + 1, (unsigned)hit);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_out; i += 256)
        if (s_h[i]) atomicAdd(out + i, (unsigned long long)s_h[i]);
}

int graph_decode_check_args(int C, int R, int multi, int score_mode, int n_labels, int max_rel) {
    if (R <= 0 || R > GD_MAX_R || C <= 0 || C > GD_MAX_C) return fail(-1, "graph_decode: 1..1024 object and 1..32 relation classes");
    if (multi != 0 && multi != 1) return fail(-1, "graph_decode: multi_label 0 | 1");
    if (score_mode != 0 && score_mode != 1) return fail(-1, "graph_decode: score_mode 0 (rel) or 1 (triplet)");
    if (n_labels < 1 || n_labels > GD_MAX_LABELS || n_labels > C) return fail(-1, "graph_decode: n_labels must be in 1..8 (and at most n_obj_class)");
    if (max_rel < 1 || max_rel > GD_MAX_REL) return fail(-1, "graph_decode: max_rel must be in 1..4096");
    return 0;
}

size_t graph_decode_scratch_bytes(int64_t E, int R, int n_scenes) {
    return align_up((size_t)(n_scenes + 1) * sizeof(int32_t), 256) + align_up((size_t)E * sizeof(int32_t), 256) +
           align_up((size_t)E * R * sizeof(uint32_t), 256) + align_up((size_t)E * R, 256);
}

GraphDecodeWs graph_decode_carve(void* scratch, int64_t E, int R, int n_scenes) {
    char* p = static_cast<char*>(scratch);
    GraphDecodeWs w;
    w.ptr = reinterpret_cast<int32_t*>(p);     p += align_up((size_t)(n_scenes + 1) * sizeof(int32_t), 256);
    w.cnt = reinterpret_cast<int32_t*>(p);     p += align_up((size_t)E * sizeof(int32_t), 256);
    w.keys = reinterpret_cast<uint32_t*>(p);   p += align_up((size_t)E * R * sizeof(uint32_t), 256);
    w.preds = reinterpret_cast<uint8_t*>(p);
    return w;
}

int launch_graph_decode(const float* obj_probs, const float* rel, const int64_t* edges, const int64_t* batch_ids, const int32_t* node_ptr,
                        const float* thr, int N, int E, int C, int R, int n_scenes, int multi, int score_mode, int n_labels, int max_rel,
                        const GraphDecodeWs& ws, int32_t* labels, float* label_probs, int32_t* rels, float* score, int32_t* nvalid,
                        int32_t* ntotal, hipStream_t s) {
    const int rc = graph_decode_check_args(C, R, multi, score_mode, n_labels, max_rel);
    if (rc) return rc;
    if (n_scenes < 0 || N < 0 || E < 0 || (E > 0 && N <= 0)) return fail(-1, "graph_decode: bad sizes");
    if (E > (1 << 26) || (int64_t)E * R > INT32_MAX) return fail(-1, "graph_decode: at most 2^26 edges and 2^31 - 1 (edge, predicate) pairs");
    if (N > 0) {
        hipLaunchKernelGGL(gd_node_kernel, dim3((N + 3) / 4), dim3(256), 0, s, obj_probs, N, C, n_labels, labels, label_probs);
        VLSAT_LAUNCH_CHECK("graph_decode node");
    }
    if (n_scenes == 0) return 0;
    const int rp = launch_scene_edge_ptr(edges, batch_ids, node_ptr, N, E, n_scenes, ws.ptr, s);
    if (rp) return rp;
    if (E > 0) {
        hipLaunchKernelGGL(gd_edge_kernel, dim3((E + 7) / 8), dim3(256), 0, s, rel, edges, thr, label_probs, n_labels, N, E, R, multi,
                           score_mode, ws.keys, ws.preds, ws.cnt);
        VLSAT_LAUNCH_CHECK("graph_decode edge");
    }
    hipLaunchKernelGGL(gd_scene_kernel, dim3(n_scenes), dim3(GD_SCENE_THREADS), 0, s, ws.ptr, ws.keys, ws.preds, ws.cnt, E, R, max_rel, rels,
                       score, nvalid, ntotal);
    VLSAT_LAUNCH_CHECK("graph_decode scene");
    return 0;
}

int launch_graph_decode_counts(const float* obj_probs, const float* rel, const int64_t* gt_cls, const int64_t* gt_rel, const float* thr,
                               int N, int E, int C, int R, int multi, unsigned long long* out, hipStream_t s) {
    if (R <= 0 || R > GD_MAX_R || C <= 0 || C > GD_MAX_C) return fail(-1, "graph_decode_counts: 1..1024 object and 1..32 relation classes");
    if (multi != 0 && multi != 1) return fail(-1, "graph_decode_counts: multi_label 0 | 1");
    if (N < 0 || E < 0) return fail(-1, "graph_decode_counts: bad sizes");
    const int nbe = E > 0 ? (E + 7) / 8 < 1024 ? (E + 7) / 8 : 1024 : 0;
    const int nbn = N > 0 ? (N + 3) / 4 < 256 ? (N + 3) / 4 : 256 : 0;
    if (nbe + nbn == 0) return 0;
    hipLaunchKernelGGL(gd_counts_kernel, dim3(nbe + nbn), dim3(256), 0, s, obj_probs, rel, gt_cls, gt_rel, thr, N, E, C, R, multi, nbe, out);
    VLSAT_LAUNCH_CHECK("graph_decode counts");
    return 0;
}

}  // namespace vlsat
