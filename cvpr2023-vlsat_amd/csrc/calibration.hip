// Score histograms for choosing thresholds and judging calibration (include/vlsat_calib.h): one pass over a batch's outputs gives
// the tp / fp / fn of EVERY threshold k / bins of the decode (graph_decode.hip), the reliability table of the object head and its
// confusion matrix.  Integer counts only; the bin rule is calib_core.h's, the two picks are decode_core.h's.
//   sh_kernel, edge blocks   32 lanes per edge, lane = predicate, as gd_counts_kernel: the single-label pick is then the decode's
//                            own gd_pick.  A block owns a GROUP of G consecutive predicates -- as many as have their two rows of
//                            bins + 1 32-bit counters in the block's LDS (64 KiB: 32 predicates at 16 bins, 7 at 1024, 1 at 4096)
//                            -- and walks a persistent chunk of the edges; block b = (chunk, group), group fastest, so the blocks
//                            that read the same rows are launched next to each other.  Every group pulls the whole row-major
//                            matrix through the caches: groups x 31 MB at the 64-scene batch, still small.
//                            Contention: a lane sees one predicate for the whole walk, and most scores of one predicate fall into
//                            the same one or two columns, so the lane keeps (key, run length) in registers and touches LDS only
//                            when the key changes: the common case and the all-equal worst case both cost a handful of LDS
//                            atomics per lane, and a wave instruction never has more than two lanes on one address (the two
//                            edges of a wave).  One flush per block: 64-bit global atomic adds of the non-zero counters.
//   sh_kernel, node blocks   one wave per node: gd_top1, then one 64-bit global atomic per table.
// Every sum is an integer: the tables do not depend on scheduling, and several streams may add into one table.
// Integer / latency-bound work: no MFMA.
#include "../../include/vlsat_calib.h"
#include "calib_core.h"
#include "common.h"
#include "decode_core.h"

namespace vlsat {

namespace {

constexpr int SH_MAX_R = 32;
constexpr int SH_MAX_C = 1024;
constexpr int SH_THREADS = 512;
constexpr int SH_EDGES = SH_THREADS / 32;          // edges of one block iteration
constexpr int SH_LDS_WORDS = 16384;                // 64 KiB of 32-bit counters
constexpr int SH_BLOCKS = 512;                     // edge blocks of a launch, about: two per CU at 64 KiB each
constexpr int SH_NODE_BLOCKS = 64;

int sh_group(int R, int bins) {                    // predicates per block
    const int g = SH_LDS_WORDS / (2 * (bins + 1));
    return g < R ? g : R;
}

int sh_chunks(int64_t E, int R, int bins) {        // edge chunks (blocks per group)
    const int G = sh_group(R, bins), groups = (R + G - 1) / G;
    const int64_t want = (E + SH_EDGES - 1) / SH_EDGES;
    const int cap = SH_BLOCKS / groups > 1 ? SH_BLOCKS / groups : 1;
    return (int)(want < cap ? want : cap);
}

}  // namespace

// rel_table [R, 2, bins + 1], obj_table [2, bins + 1], confusion [C, C]: see include/vlsat_calib.h.  Blocks [0, nbe) walk the edges
// (nbe = chunks * groups; 0 when rel_table is NULL), the others the nodes.  Dynamic LDS: G * 2 * (bins + 1) counters.
__global__ __launch_bounds__(SH_THREADS) void sh_kernel(const float* __restrict__ probs, const float* __restrict__ rel,
                                                        const int64_t* __restrict__ gt_cls, const int64_t* __restrict__ gt_rel, int N,
                                                        int E, int C, int R, int multi, int bins, int G, int groups, int nbe,
                                                        unsigned long long* __restrict__ rel_table,
                                                        unsigned long long* __restrict__ obj_table,
                                                        unsigned long long* __restrict__ confusion) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_h[];
    const int W = bins + 1;
    if ((int)blockIdx.x < nbe) {
        const int g = (int)blockIdx.x % groups, chunk = (int)blockIdx.x / groups, chunks = nbe / groups;
        const int k0 = g * G, kn = (R - k0 < G ? R - k0 : G);              // this block's predicates [k0, k0 + kn)
        const int n_ctr = kn * 2 * W;
        for (int i = threadIdx.x; i < n_ctr; i += SH_THREADS) s_h[i] = 0;
        __syncthreads();
        const int k = threadIdx.x & 31, j = k - k0;
        const bool mine = j >= 0 && j < kn;                                // (k < R follows)
        unsigned key = 0xFFFFFFFFu, run = 0;                               // the lane's current counter and what it owes it
        for (int e0 = chunk * SH_EDGES; e0 < E; e0 += chunks * SH_EDGES) { // (uniform trip count: gd_pick wants every lane)
            const int e = e0 + ((int)threadIdx.x >> 5);
            const bool live = e < E;
            const size_t el = live ? e : 0, row = el * R;
            float p = 0.f;
            bool ok = true;
            if (!multi) {                                                  // the whole row takes part in the pick
                p = k < R ? rel[row + k] : 0.f;
                ok = k == gd_pick(p, k, R) && k != 0;
            } else if (mine) {
                p = rel[row + k];
            }
            if (mine && live) {
                const bool hot = multi ? gt_rel[row + k] == 1 : gt_rel[el] == k && k != 0;
                const unsigned nk = (unsigned)((j * 2 + (int)hot) * W + calib_bin(p, bins, ok));
                if (nk != key) {
                    if (run) atomicAdd(s_h + key, run);
                    key = nk;
                    run = 0;
                }
                ++run;
            }
        }
        if (run) atomicAdd(s_h + key, run);
        __syncthreads();
        unsigned long long* out = rel_table + (size_t)k0 * 2 * W;          // the LDS layout is the table's, k0 predicates in
        for (int i = threadIdx.x; i < n_ctr; i += SH_THREADS)
            if (s_h[i]) atomicAdd(out + i, (unsigned long long)s_h[i]);
        return;
    }
    const int lane = threadIdx.x & 63, nbn = (int)gridDim.x - nbe;
    for (int n = ((int)blockIdx.x - nbe) * (SH_THREADS / 64) + ((int)threadIdx.x >> 6); n < N; n += nbn * (SH_THREADS / 64)) {
        float bv;
        const int bi = gd_top1(probs + (size_t)n * C, C, lane, bv);
        const int64_t gt = gt_cls[n];
        if (lane == 0 && gt >= 0 && gt < C) {                              // a node without a valid class is in neither table
            if (obj_table) atomicAdd(obj_table + (size_t)(gt == bi) * W + calib_bin(bv, bins, true), 1ull);
            if (confusion) atomicAdd(confusion + (size_t)gt * C + bi, 1ull);
        }
    }
}

int score_hist_check_args(int64_t N, int64_t E, int C, int R, int multi, int bins) {
    if (R <= 0 || R > SH_MAX_R || C <= 0 || C > SH_MAX_C) return fail(-1, "score_hist: 1..1024 object and 1..32 relation classes");
    if (multi != 0 && multi != 1) return fail(-1, "score_hist: multi_label 0 | 1");
    if (!calib_bins_ok(bins)) return fail(-1, "score_hist: bins must be a power of two in 16..4096");
    if (N < 0 || E < 0 || N > INT32_MAX) return fail(-1, "score_hist: bad sizes");
    if (E > (1 << 26) || E * R > INT32_MAX) return fail(-1, "score_hist: at most 2^26 edges and 2^31 - 1 (edge, predicate) pairs");
    return 0;
}

void score_hist_geometry(int R, int bins, int* edges_per_iteration, int* edges_per_sweep) {
    *edges_per_iteration = SH_EDGES;
    *edges_per_sweep = sh_chunks((int64_t)1 << 26, R, bins) * SH_EDGES;
}

int launch_score_hist(const float* obj_probs, const float* rel, const int64_t* gt_cls, const int64_t* gt_rel, int N, int E, int C, int R,
                      int multi, int bins, unsigned long long* rel_table, unsigned long long* obj_table, unsigned long long* confusion,
                      hipStream_t s) {
    const int rc = score_hist_check_args(N, E, C, R, multi, bins);
    if (rc) return rc;
    const int G = sh_group(R, bins), groups = (R + G - 1) / G;
    const int nbe = rel_table && E > 0 ? sh_chunks(E, R, bins) * groups : 0;
    const int per = SH_THREADS / 64;
    const int nbn = (obj_table || confusion) && N > 0 ? ((N + per - 1) / per < SH_NODE_BLOCKS ? (N + per - 1) / per : SH_NODE_BLOCKS) : 0;
    if (nbe + nbn == 0) return 0;
    const size_t lds = nbe ? (size_t)G * 2 * (bins + 1) * sizeof(unsigned) : 0;
    hipLaunchKernelGGL(sh_kernel, dim3(nbe + nbn), dim3(SH_THREADS), lds, s, obj_probs, rel, gt_cls, gt_rel, N, E, C, R, multi, bins, G,
                       groups, nbe, rel_table, obj_table, confusion);
    VLSAT_LAUNCH_CHECK("score_hist");
    return 0;
}

}  // namespace vlsat

using namespace vlsat;

extern "C" {

void vlsat_score_hist_geometry(int32_t n_rel_class, int32_t bins, int32_t* edges_per_iteration, int32_t* edges_per_sweep) {
    int a = 0, b = 0;
    if (n_rel_class >= 1 && n_rel_class <= SH_MAX_R && calib_bins_ok(bins)) score_hist_geometry(n_rel_class, bins, &a, &b);
    if (edges_per_iteration) *edges_per_iteration = a;
    if (edges_per_sweep) *edges_per_sweep = b;
}

int vlsat_score_hist(const float* obj_probs, const float* rel_probs, const int64_t* gt_class, const int64_t* gt_rel, int32_t n_nodes,
                     int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t multi_label, int32_t bins, int64_t* rel_table,
                     int64_t* obj_table, int64_t* confusion, void* stream) {
    if (score_hist_check_args(n_nodes, n_edges, n_obj_class, n_rel_class, multi_label, bins)) return VLSAT_EINVAL;
    if (n_nodes > 0 && (obj_table || confusion) && (!obj_probs || !gt_class)) return fail(VLSAT_EINVAL, "score_hist: null node argument");
    if (n_edges > 0 && rel_table && (!rel_probs || !gt_rel)) return fail(VLSAT_EINVAL, "score_hist: null edge argument");
    return launch_score_hist(obj_probs, rel_probs, gt_class, gt_rel, n_nodes, n_edges, n_obj_class, n_rel_class, multi_label, bins,
                             reinterpret_cast<unsigned long long*>(rel_table), reinterpret_cast<unsigned long long*>(obj_table),
                             reinterpret_cast<unsigned long long*>(confusion), static_cast<hipStream_t>(stream));
}

}  // extern "C"
