// Clusters cut at concave junctions (include/vlsat_convex.h states the rule; prep.convex_clusters_host restates it in numpy with equal
// bits): the table entries of vlsat_cloud_knn whose two normals open towards each other mark both their ends as boundary, the other
// oriented points are clustered over the table, and the boundary points are handed back to the cluster of their nearest labelled
// neighbour, one ring per round.  The arithmetic and the scratch layout are convex_core.h's, the union-find is union_find.h's, the
// scans are wave_core.h's and launch_scan_i32 (segment_merge.hip).
//
// Launches of vlsat_convex_clusters, V points, K entries per row, R absorption rounds:
//   cx_init_kernel        state[v] = 0 / 1 / 3 (not eligible / oriented / no usable normal); parent, size, boundary, cluster_size cleared
//   cx_evidence_kernel    THE HOT PATH with the next, V x K entries, one thread each: the K lanes of a row read the same x_i, n_i and
//                         state[i] (one address: a broadcast), the j side is a gather of 24 bytes that the table's locality keeps in L2;
//                         a concave entry stores boundary[i] = boundary[j] = 1 -- plain stores, the same value from everybody
//   cx_link_kernel        a launch of its own: boundary[] must be COMPLETE before anybody is called core.  uf_unite over the links
//   cx_root_kernel        root[v] by plain loads (-1 for a point that is not core), state 2 for the boundary points, core points per root
//                         by one add per distinct root of a wave
//   R x cx_absorb_kernel  one thread per point, no cross-lane operation; a labelled point copies its label and leaves.  Round 1 reads
//                         the labels of rule 4 from root[] and size[] (cx_label0), round r > 1 the buffer round r - 1 wrote: two buffers
//   cx_kept_kernel, scan_i32_kernel, cx_number_kernel     the kept roots numbered 1 .. S by lowest point
//   cx_label_kernel       labels, state 4 for the cores of a dissolved component, members per cluster by one add per distinct label of a wave
// The launch boundary is the only cross-block ordering.  Everything read from device memory is checked before it is used as an index.
// build.py compiles THIS file with -ffp-contract=off (PER_SOURCE_FLAGS): c rounds every product and sum on its own.
#include "../../include/vlsat_convex.h"
#include "common.h"
#include "convex_core.h"
#include "kernels.h"
#include "union_find.h"
#include "wave_core.h"

namespace vlsat {

constexpr int CX_THREADS = PLANE_THREADS;

__global__ __launch_bounds__(CX_THREADS) void cx_init_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                             const int32_t* __restrict__ mask, int n_points, int32_t* __restrict__ state,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ size,
                                                             int32_t* __restrict__ boundary, int32_t* __restrict__ cluster_size,
                                                             int32_t* __restrict__ n_clusters) {
    const int v = blockIdx.x * CX_THREADS + threadIdx.x;
    if (v == 0) *n_clusters = 0;
    if (v >= n_points) return;
    const size_t o = (size_t)v * 3;
    const bool eligible = mask[v] != 0 && plane_point_valid(points[o], points[o + 1], points[o + 2]);
    const bool oriented = eligible && convex_normal_usable(normals[o], normals[o + 1], normals[o + 2]);
    state[v] = !eligible ? CONVEX_OUT : oriented ? CONVEX_CORE : CONVEX_NO_NORMAL;
    parent[v] = v;
    size[v] = 0;
    boundary[v] = 0;
    cluster_size[v] = 0;
}

__global__ __launch_bounds__(CX_THREADS) void cx_evidence_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                                 const int32_t* __restrict__ nbr, const float* __restrict__ nbr_sqdist,
                                                                 const int32_t* __restrict__ state, int n_points, int k, float tau,
                                                                 int32_t* __restrict__ boundary) {
    const int64_t e = (int64_t)blockIdx.x * CX_THREADS + threadIdx.x;
    if (e >= (int64_t)n_points * k) return;
    const int i = (int)(e / k), j = nbr[e];
    if (j < 0 || j >= n_points || j == i) return;
    if (state[i] != CONVEX_CORE || state[j] != CONVEX_CORE) return;                // (oriented: nobody is boundary yet)
    const float q = nbr_sqdist[e];
    if (!convex_sqdist_ok(q)) return;
    const size_t oi = (size_t)i * 3, oj = (size_t)j * 3;
    const float xi[3] = {points[oi], points[oi + 1], points[oi + 2]}, ni[3] = {normals[oi], normals[oi + 1], normals[oi + 2]};
    const float xj[3] = {points[oj], points[oj + 1], points[oj + 2]}, nj[3] = {normals[oj], normals[oj + 1], normals[oj + 2]};
    if (!convex_concave(convex_c(xi, ni, xj, nj), tau, q)) return;
    boundary[i] = 1;
    boundary[j] = 1;
}

__device__ __forceinline__ bool cx_core(const int32_t* __restrict__ state, const int32_t* __restrict__ boundary, int v) {
    return state[v] == CONVEX_CORE && boundary[v] == 0;
}

__global__ __launch_bounds__(CX_THREADS) void cx_link_kernel(const int32_t* __restrict__ nbr, const float* __restrict__ nbr_sqdist,
                                                             const int32_t* __restrict__ state, const int32_t* __restrict__ boundary,
                                                             int n_points, int k, float link_sq_dist, int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * CX_THREADS + threadIdx.x;
    if (e >= (int64_t)n_points * k) return;
    const int i = (int)(e / k), j = nbr[e];
    if (j < 0 || j >= n_points || j == i || !(nbr_sqdist[e] <= link_sq_dist)) return;
    if (!cx_core(state, boundary, i) || !cx_core(state, boundary, j)) return;
    uf_unite(parent, i, j);
}

// root[v] of a core point by plain loads of the finished forest, -1 for everybody else; the boundary points get their state; the core
// points of a component by one add per distinct root of a wave (the counting of oc_root_kernel)
__global__ __launch_bounds__(CX_THREADS) void cx_root_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ boundary,
                                                             int n_points, int32_t* __restrict__ state, int32_t* __restrict__ root,
                                                             int32_t* __restrict__ size) {
    const int v = blockIdx.x * CX_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int r = -1;
    bool todo = false;
    if (v < n_points) {
        const bool oriented = state[v] == CONVEX_CORE;
        todo = oriented && boundary[v] == 0;
        if (todo) {
            r = uf_root(parent, v, n_points);
            if (r < 0 || r >= n_points) r = v;
        }
        root[v] = r;
        if (oriented && !todo) state[v] = CONVEX_BOUNDARY;
    }
    for (;;) {
        const unsigned long long pending = __ballot(todo);
        if (!pending) break;
        const int leader = __ffsll((long long)pending) - 1;
        const int r0 = __shfl(r, leader);
        const bool mine = todo && r == r0;
        const unsigned long long group = __ballot(mine);
        if (lane == leader) atomicAdd(size + r0, (int)__popcll(group));
        if (mine) todo = false;
    }
}

// rule 4: the label of v before the first round -- its root when it is a core of a kept component, else -1
__device__ __forceinline__ int cx_label0(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_points, int min_points, int v) {
    const int r = root[v];
    return r >= 0 && r < n_points && size[r] >= min_points ? r : -1;
}

// the label of v at the end of the round before: src, or rule 4 when there was none (src == nullptr)
__device__ __forceinline__ int cx_label(const int32_t* __restrict__ src, const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                        int n_points, int min_points, int v) {
    return src ? src[v] : cx_label0(root, size, n_points, min_points, v);
}

__global__ __launch_bounds__(CX_THREADS) void cx_absorb_kernel(const int32_t* __restrict__ nbr, const int32_t* __restrict__ state,
                                                               const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                               const int32_t* __restrict__ src, int n_points, int k, int min_points,
                                                               int32_t* __restrict__ dst) {
    const int v = blockIdx.x * CX_THREADS + threadIdx.x;
    if (v >= n_points) return;
    int label = cx_label(src, root, size, n_points, min_points, v);
    if (label < 0 && state[v] != CONVEX_OUT) {
        const int32_t* row = nbr + (size_t)v * k;
        for (int s = 0; s < k; ++s) {
            const int j = row[s];
            if (j < 0 || j >= n_points || j == v) continue;
            const int lj = cx_label(src, root, size, n_points, min_points, j);
            if (lj >= 0) {
                label = lj;
                break;
            }
        }
    }
    dst[v] = label;
}

__device__ __forceinline__ int cx_kept(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_points, int min_points, int v) {
    return v < n_points && root[v] == v && size[v] >= min_points;
}

__global__ __launch_bounds__(CX_THREADS) void cx_kept_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_points,
                                                             int min_points, int32_t* __restrict__ block_kept) {
    __shared__ int s_red[CX_THREADS / 64];
    const int total = block_sum<CX_THREADS>(cx_kept(root, size, n_points, min_points, blockIdx.x * CX_THREADS + threadIdx.x), s_red);
    if (threadIdx.x == 0) block_kept[blockIdx.x] = total;
}

__global__ __launch_bounds__(CX_THREADS) void cx_number_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_points,
                                                               int min_points, const int32_t* __restrict__ block_kept,
                                                               int32_t* __restrict__ num) {
    __shared__ int s_wave[CX_THREADS / 64];
    const int v = blockIdx.x * CX_THREADS + threadIdx.x;
    const int kept = cx_kept(root, size, n_points, min_points, v);
    int total;
    const int at = block_kept[blockIdx.x] + block_scan_excl<CX_THREADS>(kept, s_wave, total);
    if (v >= n_points) return;
    num[v] = kept && at >= 0 && at < n_points ? at + 1 : 0;
}

__global__ __launch_bounds__(CX_THREADS) void cx_label_kernel(const int32_t* __restrict__ last, const int32_t* __restrict__ root,
                                                              const int32_t* __restrict__ size, const int32_t* __restrict__ num, int n_points,
                                                              int min_points, int32_t* __restrict__ labels, int32_t* __restrict__ state,
                                                              int32_t* __restrict__ cluster_size) {
    const int v = blockIdx.x * CX_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int n = 0;
    if (v < n_points) {
        const int label = cx_label(last, root, size, n_points, min_points, v);
        n = label >= 0 && label < n_points ? num[label] : 0;
        if (n < 0 || n > n_points) n = 0;                                          // (cannot happen: num is 0 or a rank below V)
        labels[v] = n;
        if (root[v] >= 0 && cx_label0(root, size, n_points, min_points, v) < 0) state[v] = CONVEX_DISSOLVED;
    }
    bool todo = n > 0;
    for (;;) {
        const unsigned long long pending = __ballot(todo);
        if (!pending) break;
        const int leader = __ffsll((long long)pending) - 1;
        const int n0 = __shfl(n, leader);
        const bool mine = todo && n == n0;
        const unsigned long long group = __ballot(mine);
        if (lane == leader) atomicAdd(cluster_size + (n0 - 1), (int)__popcll(group));
        if (mine) todo = false;
    }
}

static unsigned cx_blocks(int64_t n) { return (unsigned)((n + CX_THREADS - 1) / CX_THREADS); }

}  // namespace vlsat

using namespace vlsat;

extern "C" {

size_t vlsat_convex_clusters_scratch_bytes(int64_t n_points) {
    if (!convex_sizes_ok(n_points, 1)) return 0;
    return convex_layout(n_points).bytes;
}

int vlsat_convex_clusters(const float* points, const float* normals, const int32_t* nbr, const float* nbr_sqdist, const int32_t* mask,
                          int64_t n_points, int32_t k, float link_sq_dist, float concavity, int32_t min_points, int32_t absorb_rounds,
                          void* scratch, int32_t* labels, int32_t* n_clusters, int32_t* cluster_size, int32_t* state, void* stream) {
    if (!convex_sizes_ok(n_points, k)) return fail(VLSAT_EINVAL, "convex_clusters: 1 .. 2^24 points and 1 .. 32 neighbours");
    if (link_sq_dist != link_sq_dist) return fail(VLSAT_EINVAL, "convex_clusters: link_sq_dist is NaN");
    if (!(concavity >= 0.0f && concavity <= 1.0f)) return fail(VLSAT_EINVAL, "convex_clusters: concavity must be in [0, 1]");
    if (min_points < 1) return fail(VLSAT_EINVAL, "convex_clusters: min_points must be at least 1");
    if (absorb_rounds < 0 || absorb_rounds > CONVEX_MAX_ROUNDS) return fail(VLSAT_EINVAL, "convex_clusters: absorb_rounds must be in 0 .. 64");
    if (!points || !normals || !nbr || !nbr_sqdist || !mask || !scratch || !labels || !n_clusters || !cluster_size || !state)
        return fail(VLSAT_EINVAL, "convex_clusters: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int V = (int)n_points, K = (int)k, M = (int)min_points;
    const ConvexLayout l = convex_layout(n_points);
    char* base = static_cast<char*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(base + l.parent);
    int32_t* root = reinterpret_cast<int32_t*>(base + l.root);
    int32_t* size = reinterpret_cast<int32_t*>(base + l.size);
    int32_t* boundary = reinterpret_cast<int32_t*>(base + l.boundary);
    int32_t* label[2] = {reinterpret_cast<int32_t*>(base + l.label_a), reinterpret_cast<int32_t*>(base + l.label_b)};
    int32_t* num = reinterpret_cast<int32_t*>(base + l.num);
    int32_t* block_kept = reinterpret_cast<int32_t*>(base + l.block_kept);
    const dim3 block(CX_THREADS), per_point(cx_blocks(V)), per_entry(cx_blocks((int64_t)V * K));
    hipLaunchKernelGGL(cx_init_kernel, per_point, block, 0, s, points, normals, mask, V, state, parent, size, boundary, cluster_size, n_clusters);
    hipLaunchKernelGGL(cx_evidence_kernel, per_entry, block, 0, s, points, normals, nbr, nbr_sqdist, (const int32_t*)state, V, K, concavity,
                       boundary);
    hipLaunchKernelGGL(cx_link_kernel, per_entry, block, 0, s, nbr, nbr_sqdist, (const int32_t*)state, (const int32_t*)boundary, V, K,
                       link_sq_dist, parent);
    hipLaunchKernelGGL(cx_root_kernel, per_point, block, 0, s, (const int32_t*)parent, (const int32_t*)boundary, V, state, root, size);
    const int32_t* last = nullptr;                                                 // the labels of rule 4 live in root[] and size[]
    for (int r = 0; r < (int)absorb_rounds; ++r) {
        hipLaunchKernelGGL(cx_absorb_kernel, per_point, block, 0, s, nbr, (const int32_t*)state, (const int32_t*)root, (const int32_t*)size, last, V,
                           K, M, label[r & 1]);
        last = label[r & 1];
    }
    hipLaunchKernelGGL(cx_kept_kernel, per_point, block, 0, s, (const int32_t*)root, (const int32_t*)size, V, M, block_kept);
    launch_scan_i32(block_kept, (int)per_point.x, block_kept, n_clusters, nullptr, s);           // in place; the total is S <= V
    hipLaunchKernelGGL(cx_number_kernel, per_point, block, 0, s, (const int32_t*)root, (const int32_t*)size, V, M, (const int32_t*)block_kept, num);
    hipLaunchKernelGGL(cx_label_kernel, per_point, block, 0, s, last, (const int32_t*)root, (const int32_t*)size, (const int32_t*)num, V, M, labels,
                       state, cluster_size);
    VLSAT_LAUNCH_CHECK("convex_clusters");
    return 0;
}

}  // extern "C"
