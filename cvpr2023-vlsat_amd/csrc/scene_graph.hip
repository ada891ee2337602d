// The predicted scene graph: per scene the top_k (subject, predicate, object) triplets the model believes in, WITH their indices --
// the list the reference builds inside evaluate_triplet_recallk (src/utils/eval_utils_recall.py:24-60, 75-96: the running global
// top-K all_topk_id / all_topk_conf_matrix, unravelled into pred_triplets) and never returns.  No labels are read.
//   triplet mode  conf(e; i, j, k) = fl(fl(s_i * o_j) * r_k), s = obj_probs[from], o = obj_probs[to], r = rel_probs[e] (two
//                 roundings, no FMA: the reference's two einsums, as eval_recall.hip scores them)
//   rels mode     conf(e; k) = r_k, subject / object class reported as -1
// The candidates of a scene are, per edge, its L = min(topk_each, #entries) largest entries.  eval_recall.hip selects the same
// candidates as values only; here every value carries its class triple (key, bisection and tie rule: select_core.h):
//   launch_sort_probs       (eval_ranks.hip) per node the min(C, 100) largest probabilities, descending, with their class indices
//                           (stable by class)
//   sg_scene_ptr_kernel     edge offsets of every scene (edges arrive grouped by scene in ascending order)
//   sg_edge_kernel          one wave per edge: predicates sorted with indices; triplet mode: the products over the dominance table
//                           (an entry at sorted position (i, j, k) is dominated by (i+1)(j+1)(k+1) - 1 others, so the L largest lie
//                           among the positions with (i+1)(j+1)(k+1) <= L), the L-th largest key by bisection on the key bits,
//                           the keys above it plus as many equal to it as are needed, ordered by counting -> L slots of
//                           (order-preserving key, packed class triple), descending.  The C x C x R products are never formed.
//   sg_scene_kernel         one block per scene: the top_k-th largest key by bisection over the per-edge sorted lists, a gather of
//                           the slots above it plus the first slots equal to it (edge order, then slot order), a sort of <= top_k
//                           rows in LDS by (score descending; edge, subject class, object class, predicate ascending), one write.
// Every output field of every scene is written by exactly one block: no global atomics, no fill, no host synchronisation, no
// allocation.  Which of several candidates EQUAL to a boundary value are kept depends on the scene's own inputs only.
// Integer / latency-bound work: no MFMA.
#include "common.h"
#include "kernels.h"
#include "select_core.h"

namespace vlsat {

namespace {

constexpr int SG_EACH = 100;                     // largest topk_each: the bound of the dominance table
constexpr int SG_MAX_R = 32;
constexpr int SG_MAX_K = 1024;                   // largest top_k = threads of the scene block (one row per thread)
constexpr int SG_SCENE_THREADS = 1024;

constexpr int SG_NT = tri_count(SG_EACH, SG_MAX_R);   // 1 365
constexpr int SG_PER = (SG_NT + 63) / 64;        // table entries per lane
__constant__ TriTable<SG_EACH, SG_MAX_R> c_tri = make_tri<SG_EACH, SG_MAX_R>();

// class triple of a slot: subject class (10 bits) | object class (10 bits) | predicate (5 bits); ascending = (sub, obj, pred) ascending
__device__ __forceinline__ uint32_t sg_pack(int sub, int obj, int pred) { return ((uint32_t)sub << 15) | ((uint32_t)obj << 5) | (uint32_t)pred; }

// slots per edge: min(topk_each, #entries of an edge)
int sg_slots(int C, int R, int mode, int each) {
    const int64_t entries = mode == 1 ? (int64_t)R : (int64_t)C * C * R;
    return (int)(entries < each ? entries : each);
}

}  // namespace

// ptr[q] = first edge of scene q, ptr[n_scenes] = E (thread t = E closes the list).  The scene of an edge is that of its first
// node: batch_ids[node], or -- node_ptr given -- the scene whose node range holds it, or 0.
__global__ __launch_bounds__(256) void sg_scene_ptr_kernel(const int64_t* __restrict__ edges, const int64_t* __restrict__ batch_ids,
                                                           const int32_t* __restrict__ node_ptr, int N, int E, int n_scenes,
                                                           int32_t* __restrict__ ptr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t > E) return;
    auto scene = [&](int e) {
        const int a = clampi(edges[2 * (size_t)e], 0, N - 1);
        if (batch_ids) return clampi(batch_ids[a], 0, n_scenes - 1);
        if (!node_ptr) return 0;
        int lo = 0, hi = n_scenes;                                 // #{q <= n_scenes: node_ptr[q] <= a} - 1
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (node_ptr[mid] <= a) lo = mid; else hi = mid - 1;
        }
        return lo < n_scenes ? lo : n_scenes - 1;
    };
    const int s0 = t > 0 ? scene(t - 1) : -1, s1 = t < E ? scene(t) : n_scenes;
    for (int q = s0 + 1; q <= s1; ++q) ptr[q] = t;
}

__global__ __launch_bounds__(256) void sg_exp_kernel(const float* x, float* out, size_t n) {      // (out may be x)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = log_prob_exp(x[i]);
}

// one wave per edge, 4 edges per block; L = slots per edge (1 <= L <= 100; rels mode: L <= R)
__global__ __launch_bounds__(256) void sg_edge_kernel(const float* __restrict__ sv, const int32_t* __restrict__ si, int Ks,
                                                      const float* __restrict__ rel, const int64_t* __restrict__ edges, int N, int E, int R,
                                                      int mode, int L, uint32_t* __restrict__ keys, uint32_t* __restrict__ packs) {
    __shared__ float s_rs[4][SG_MAX_R];            // the edge's predicate scores, descending, and their classes
    __shared__ int s_ri[4][SG_MAX_R];
    __shared__ float s_a[4][SG_EACH], s_b[4][SG_EACH];
    __shared__ int s_ai[4][SG_EACH], s_bi[4][SG_EACH];
    __shared__ uint32_t s_key[4][SG_EACH], s_pk[4][SG_EACH];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, e = blockIdx.x * 4 + w;
    const bool live = e < E;                       // (no early return: the block synchronises twice)
    if (live) {
        const float rv = lane < R ? rel[(size_t)e * R + lane] : -INFINITY;
        const int rk = rank_desc_in_wave(rv, lane, R);
        if (lane < R) {
            s_rs[w][rk] = rv;
            s_ri[w][rk] = lane;
        }
        if (mode == 0) {
            const int a = clampi(edges[2 * (size_t)e], 0, N - 1), b = clampi(edges[2 * (size_t)e + 1], 0, N - 1);
            for (int i = lane; i < Ks; i += 64) {
                s_a[w][i] = sv[(size_t)a * Ks + i];
                s_ai[w][i] = si[(size_t)a * Ks + i];
                s_b[w][i] = sv[(size_t)b * Ks + i];
                s_bi[w][i] = si[(size_t)b * Ks + i];
            }
        }
    }
    __syncthreads();
    uint32_t* okey = keys + (size_t)(live ? e : 0) * L;
    uint32_t* opk = packs + (size_t)(live ? e : 0) * L;
    if (mode == 1) {                               // (uniform) the L largest predicates
        if (live && lane < L) {
            okey[lane] = fkey(s_rs[w][lane]);
            opk[lane] = (uint32_t)s_ri[w][lane];
        }
        return;
    }
    if (L == 1) {                                  // (uniform) graph constraint: the entry at sorted position (0, 0, 0)
        if (live && lane == 0) {
            okey[0] = fkey(__fmul_rn(__fmul_rn(s_a[w][0], s_b[w][0]), s_rs[w][0]));
            opk[0] = sg_pack(s_ai[w][0], s_bi[w][0], s_ri[w][0]);
        }
        return;
    }
    uint32_t v[SG_PER];
#pragma unroll
    for (int t = 0; t < SG_PER; ++t) {
        const int idx = lane + 64 * t;
        uint32_t key = 0;
        if (live && idx < SG_NT) {
            const uint32_t tr = c_tri.v[idx];
            const int i = tr & 0xff, j = (tr >> 8) & 0xff, k = tr >> 16;
            if (i < Ks && j < Ks && k < R && (i + 1) * (j + 1) * (k + 1) <= L)
                key = fkey(__fmul_rn(__fmul_rn(s_a[w][i], s_b[w][j]), s_rs[w][k]));
        }
        v[t] = key;
    }
    const uint32_t T = wave_kth_largest(v, L);     // the L-th largest key (at least L table positions are in range, so T > 0)
    // the (< L) entries above T, then entries equal to T until L are gathered, both in lane order
    int mine = 0;                                  // #above | #equal << 16
#pragma unroll
    for (int t = 0; t < SG_PER; ++t) mine += (v[t] > T) + ((v[t] == T) << 16);
    int off = wave_scan_incl(mine, lane);
    const int above = __shfl(off, 63) & 0xffff, need = L - above;
    off -= mine;
    int oa = off & 0xffff, oq = off >> 16;
#pragma unroll
    for (int t = 0; t < SG_PER; ++t) {
        const uint32_t key = v[t];
        int pos = -1;
        if (key > T) pos = oa++;
        else if (key == T && key != 0) {
            if (oq < need) pos = above + oq;
            ++oq;
        }
        if (pos >= 0 && pos < L) {
            const uint32_t tr = c_tri.v[lane + 64 * t];
            s_key[w][pos] = key;
            s_pk[w][pos] = sg_pack(s_ai[w][tr & 0xff], s_bi[w][(tr >> 8) & 0xff], s_ri[w][tr >> 16]);
        }
    }
    __syncthreads();
    if (!live) return;
    for (int i = lane; i < L; i += 64) {           // order by (key descending, class triple ascending): the triples are distinct
        const uint32_t x = s_key[w][i], px = s_pk[w][i];
        int rank = 0;
        for (int q = 0; q < L; ++q) {
            const uint32_t y = s_key[w][q];
            rank += y > x || (y == x && s_pk[w][q] < px);
        }
        okey[rank] = x;
        opk[rank] = px;
    }
}

// block = scene; thread = edge while selecting, = output row while sorting and writing
__global__ __launch_bounds__(SG_SCENE_THREADS) void sg_scene_kernel(const int32_t* __restrict__ ptr, const uint32_t* __restrict__ keys,
                                                                   const uint32_t* __restrict__ packs, int E, int L, int K, int mode,
                                                                   int32_t* __restrict__ trip, float* __restrict__ score,
                                                                   int32_t* __restrict__ nvalid) {
    constexpr int NW = SG_SCENE_THREADS / 64;
    __shared__ uint32_t s_k[SG_MAX_K], s_e[SG_MAX_K], s_p[SG_MAX_K];
    __shared__ int s_red[NW];
    __shared__ long long s_scan[NW];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int e0 = clampi(ptr[s], 0, E), e1 = max(e0, clampi(ptr[s + 1], 0, E));
    const long long total = (long long)(e1 - e0) * L;
    const int Kk = total < K ? (int)total : K;     // n_valid
    if (Kk > 0)                                    // (uniform) the Kk largest slots of the scene, unordered
        select_topk_lists<SG_SCENE_THREADS>(keys, L, [&](int) { return L; }, e0, e1, Kk, true, s_red, s_scan, [&](int pos, int e, int j) {
            s_k[pos] = keys[(size_t)e * L + j];
            s_e[pos] = (uint32_t)e;
            s_p[pos] = packs[(size_t)e * L + j];
        });
    __syncthreads();
    if (tid == 0) nvalid[s] = Kk;
    if (tid >= K) return;
    int32_t* orow = trip + (size_t)s * K * 4;
    float* osc = score + (size_t)s * K;
    if (tid >= Kk) {                               // rows past n_valid
        orow[4 * tid] = orow[4 * tid + 1] = orow[4 * tid + 2] = orow[4 * tid + 3] = -1;
        osc[tid] = 0.f;
        return;
    }
    const uint32_t x = s_k[tid], ex = s_e[tid], px = s_p[tid];
    int rank = 0;                                  // (score descending; edge, subject class, object class, predicate ascending): rows are distinct
    for (int q = 0; q < Kk; ++q) {
        const uint32_t y = s_k[q], ey = s_e[q];
        rank += y > x || (y == x && (ey < ex || (ey == ex && s_p[q] < px)));
    }
    int32_t* o = orow + 4 * (size_t)rank;
    o[0] = (int32_t)ex;
    o[1] = mode == 1 ? -1 : (int32_t)(px >> 15);
    o[2] = mode == 1 ? -1 : (int32_t)((px >> 5) & 1023);
    o[3] = (int32_t)(px & 31);
    osc[rank] = unkey(x);
}

size_t scene_graph_scratch_bytes(int64_t N, int64_t E, int C, int R, int n_scenes, int each) {
    const int64_t Ks = C < SG_EACH ? C : SG_EACH;
    const int L = sg_slots(C, R, 0, each);
    return 2 * align_up((size_t)N * Ks * sizeof(float), 256) + align_up((size_t)(n_scenes + 1) * sizeof(int32_t), 256) +
           2 * align_up((size_t)E * L * sizeof(uint32_t), 256);
}

SceneGraphWs scene_graph_carve(void* scratch, int64_t N, int64_t E, int C, int R, int n_scenes, int each) {
    const int64_t Ks = C < SG_EACH ? C : SG_EACH;
    const int L = sg_slots(C, R, 0, each);
    char* p = static_cast<char*>(scratch);
    SceneGraphWs w;
    w.sv = reinterpret_cast<float*>(p);        p += align_up((size_t)N * Ks * sizeof(float), 256);
    w.si = reinterpret_cast<int32_t*>(p);      p += align_up((size_t)N * Ks * sizeof(float), 256);
    w.ptr = reinterpret_cast<int32_t*>(p);     p += align_up((size_t)(n_scenes + 1) * sizeof(int32_t), 256);
    w.keys = reinterpret_cast<uint32_t*>(p);   p += align_up((size_t)E * L * sizeof(uint32_t), 256);
    w.packs = reinterpret_cast<uint32_t*>(p);
    return w;
}

int scene_graph_check_args(int C, int R, int mode, int top_k, int each) {
    if (R <= 0 || R > SG_MAX_R || C <= 0 || C > 1024) return fail(-1, "scene_graph_topk: 1..1024 object and 1..32 relation classes");
    if (mode != 0 && mode != 1) return fail(-1, "scene_graph_topk: mode 0 (triplet) or 1 (rels)");
    if (top_k < 1 || top_k > SG_MAX_K) return fail(-1, "scene_graph_topk: top_k must be in 1..1024");
    if (each < 1 || each > SG_EACH) return fail(-1, "scene_graph_topk: topk_each must be in 1..100");
    return 0;
}

int launch_exp(const float* x, float* out, size_t n, hipStream_t s) {
    if (!n) return 0;
    hipLaunchKernelGGL(sg_exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, n);
    VLSAT_LAUNCH_CHECK("scene_graph exp");
    return 0;
}

int launch_scene_edge_ptr(const int64_t* edges, const int64_t* batch_ids, const int32_t* node_ptr, int N, int E, int n_scenes, int32_t* ptr,
                          hipStream_t s) {
    hipLaunchKernelGGL(sg_scene_ptr_kernel, dim3(E / 256 + 1), dim3(256), 0, s, edges, batch_ids, node_ptr, N, E, n_scenes, ptr);
    VLSAT_LAUNCH_CHECK("scene_graph scene_ptr");
    return 0;
}

int launch_scene_graph_topk(const float* obj_probs, const float* rel, const int64_t* edges, const int64_t* batch_ids,
                            const int32_t* node_ptr, int N, int E, int C, int R, int n_scenes, int mode, int top_k, int each,
                            const SceneGraphWs& ws, int32_t* trip, float* score, int32_t* nvalid, hipStream_t s) {
    const int rc = scene_graph_check_args(C, R, mode, top_k, each);
    if (rc) return rc;
    if (n_scenes < 0 || N < 0 || E < 0 || (E > 0 && N <= 0)) return fail(-1, "scene_graph_topk: bad sizes");
    if (n_scenes == 0) return 0;
    const int Ks = C < SG_EACH ? C : SG_EACH;
    const int L = sg_slots(C, R, mode, each);
    const int rp = launch_scene_edge_ptr(edges, batch_ids, node_ptr, N, E, n_scenes, ws.ptr, s);
    if (rp) return rp;
    if (E > 0) {
        if (mode == 0) {
            const int rs = launch_sort_probs(obj_probs, N, C, Ks, ws.sv, s, ws.si);
            if (rs) return rs;
        }
        hipLaunchKernelGGL(sg_edge_kernel, dim3((E + 3) / 4), dim3(256), 0, s, ws.sv, ws.si, Ks, rel, edges, N, E, R, mode, L, ws.keys,
                           ws.packs);
        VLSAT_LAUNCH_CHECK("scene_graph edge");
    }
    hipLaunchKernelGGL(sg_scene_kernel, dim3(n_scenes), dim3(SG_SCENE_THREADS), 0, s, ws.ptr, ws.keys, ws.packs, E, L, top_k, mode, trip,
                       score, nvalid);
    VLSAT_LAUNCH_CHECK("scene_graph scene");
    return 0;
}

}  // namespace vlsat
