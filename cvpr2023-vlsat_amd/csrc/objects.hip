// A cloud segmented into objects without a trained model (include/vlsat_objects.h states both rules; prep.cloud_planes_host and
// prep.cloud_clusters_host restate them in numpy with equal bits): the structural planes of the room are found by scoring drawn
// three-point planes against every remaining point and removed, and what is left is clustered over the neighbour table of
// vlsat_cloud_knn.  The arithmetic and the scratch layouts are plane_core.h's, the union-find is union_find.h's, the scans are
// wave_core.h's and launch_scan_i32 (segment_merge.hip).
//
// Launches of vlsat_cloud_planes, V points, H hypotheses, P rounds:
//   op_init_kernel        alive[i] = the point is finite, plane_id[i] = 0; planes, plane_counts, n_planes and the state cleared
//   P x  op_count_kernel        alive points per block of 256
//        scan_i32_kernel        ONE block: the exclusive scan of those counts in place; the total n goes to state[N]
//        op_scatter_kernel      the block's own exclusive scan on top of its offset: the alive list, ascending
//        op_hypotheses_kernel   one thread per hypothesis: three drawn ranks, the plane in fp64, rounded to fp32; clears its two counters
//        op_score_kernel<HPT>   THE HOT PATH, n x H scores: see below
//        op_select_kernel       ONE block: the largest key among the eligible hypotheses; writes row r, or raises the done flag
//        op_apply_kernel        the winner's inliers get plane_id = r + 1 and die
// All P rounds are enqueued.  state[DONE] is raised by op_select_kernel when a round stops (n < 3, or nothing eligible); it is read
// by the kernels of LATER launches only, which return at once -- the launch boundary is the only cross-block ordering, there is no
// cooperative launch, no spin-wait and nothing is read back.
//
// op_score_kernel: a block of 256 threads, each thread HPT (1, 2 or 4) hypotheses in registers with two private integer counters
// each.  The block walks tiles of 1024 alive points (grid-stride over blockIdx.x; blockIdx.y is the hypothesis group), stages them in
// LDS as float4 through the alive list, and every lane then reads the SAME point: one ds_read_b128 broadcast, free of bank conflicts,
// per point and thread.  The inner loop has no cross-lane operation; at the end one integer atomicAdd per block, hypothesis and
// counter.  below = n - inliers - above is never counted: a NaN score is neither an inlier nor above, so it lands there.
// Integer sums: the counts do not depend on the order of the blocks.  build.py compiles THIS file with -ffp-contract=off
// (PER_SOURCE_FLAGS): the plane and the score round every product and sum on their own.
//
// Launches of vlsat_cloud_clusters: oc_init_kernel, oc_link_kernel (one thread per table entry), oc_root_kernel (roots by plain
// loads, sizes by one add per distinct root of a wave), oc_kept_kernel, scan_i32_kernel, oc_number_kernel, oc_label_kernel.
// Everything read from device memory is checked before it is used as an index.
#include "../../include/vlsat_objects.h"
#include "common.h"
#include "kernels.h"
#include "plane_core.h"
#include "union_find.h"
#include "wave_core.h"

namespace vlsat {

constexpr int OP_THREADS = PLANE_THREADS;
constexpr int OP_TILE = 1024;                            // alive points in LDS at a time: 16 KB
constexpr int OP_MAX_BLOCKS = 2048;                      // of the score kernel: 8 per CU
// state words of vlsat_cloud_planes
enum { OP_DONE = 0, OP_N = 1, OP_WIN = 2 };

__global__ __launch_bounds__(OP_THREADS) void op_init_kernel(const float* __restrict__ points, int n_points, int max_planes,
                                                             int32_t* __restrict__ alive, int32_t* __restrict__ plane_id,
                                                             float* __restrict__ planes, int32_t* __restrict__ plane_counts,
                                                             int32_t* __restrict__ n_planes, int32_t* __restrict__ state) {
    const int i = blockIdx.x * OP_THREADS + threadIdx.x;
    if (i < max_planes * 4) planes[i] = 0.0f;
    if (i < max_planes * 3) plane_counts[i] = 0;
    if (i < 8) state[i] = 0;
    if (i == 0) *n_planes = 0;
    if (i >= n_points) return;
    alive[i] = plane_point_valid(points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]);
    plane_id[i] = 0;
}

__global__ __launch_bounds__(OP_THREADS) void op_count_kernel(const int32_t* __restrict__ alive, int n_points,
                                                              int32_t* __restrict__ block_alive) {
    __shared__ int s_red[OP_THREADS / 64];
    const int i = blockIdx.x * OP_THREADS + threadIdx.x;
    const int total = block_sum<OP_THREADS>(i < n_points && alive[i] != 0, s_red);
    if (threadIdx.x == 0) block_alive[blockIdx.x] = total;
}

__global__ __launch_bounds__(OP_THREADS) void op_scatter_kernel(const int32_t* __restrict__ alive, int n_points,
                                                                const int32_t* __restrict__ block_alive, const int32_t* __restrict__ state,
                                                                int32_t* __restrict__ alive_list) {
    __shared__ int s_wave[OP_THREADS / 64];
    if (state[OP_DONE]) return;                                       // (uniform: written by an earlier launch)
    const int i = blockIdx.x * OP_THREADS + threadIdx.x;
    const int mine = i < n_points && alive[i] != 0;
    int total;
    const int at = block_alive[blockIdx.x] + block_scan_excl<OP_THREADS>(mine, s_wave, total);
    if (mine && at >= 0 && at < n_points) alive_list[at] = i;
}

// the alive point of rank `rank` into p[3]; false when the list names no point (it never does)
__device__ __forceinline__ bool op_load_rank(const float* __restrict__ points, const int32_t* __restrict__ alive_list, int n_points, uint32_t rank,
                                             float* p) {
    const int32_t i = rank < (uint32_t)n_points ? alive_list[rank] : -1;
    if (i < 0 || i >= n_points) return false;
    p[0] = points[(size_t)i * 3];
    p[1] = points[(size_t)i * 3 + 1];
    p[2] = points[(size_t)i * 3 + 2];
    return true;
}

__global__ __launch_bounds__(OP_THREADS) void op_hypotheses_kernel(const float* __restrict__ points, const int32_t* __restrict__ alive_list,
                                                                   int n_points, int n_hyp, int round, unsigned long long seed,
                                                                   const int32_t* __restrict__ state, float4* __restrict__ hyp,
                                                                   int32_t* __restrict__ hyp_ok, int32_t* __restrict__ counts,
                                                                   unsigned long long* __restrict__ best) {
    if (state[OP_DONE]) return;
    const int n = state[OP_N];
    if (n < 3 || n > n_points) return;                                // (op_select_kernel raises the flag)
    const int h = blockIdx.x * OP_THREADS + threadIdx.x;
    if (h == 0) *best = 0ull;
    if (h >= n_hyp) return;
    const unsigned long long k0 = ((unsigned long long)round * (unsigned long long)n_hyp + (unsigned long long)h) * 3ull;
    float a[3], b[3], c[3];
    bool ok = op_load_rank(points, alive_list, n_points, plane_draw(seed, k0, (uint32_t)n), a);
    ok = op_load_rank(points, alive_list, n_points, plane_draw(seed, k0 + 1, (uint32_t)n), b) && ok;
    ok = op_load_rank(points, alive_list, n_points, plane_draw(seed, k0 + 2, (uint32_t)n), c) && ok;
    Plane pl;
    pl.nx = pl.ny = pl.nz = pl.d = 0.0f;
    if (ok) ok = plane_from_points(a, b, c, pl);
    hyp[h] = make_float4(pl.nx, pl.ny, pl.nz, pl.d);
    hyp_ok[h] = ok;
    counts[2 * h] = 0;
    counts[2 * h + 1] = 0;
}

template <int HPT>
__global__ __launch_bounds__(OP_THREADS) void op_score_kernel(const float* __restrict__ points, const int32_t* __restrict__ alive_list,
                                                              int n_points, int n_hyp, float dist, const int32_t* __restrict__ state,
                                                              const float4* __restrict__ hyp, const int32_t* __restrict__ hyp_ok,
                                                              int32_t* __restrict__ counts) {
    __shared__ float4 s_pt[OP_TILE];
    if (state[OP_DONE]) return;
    const int n = state[OP_N];
    if (n < 3 || n > n_points) return;
    const int tid = threadIdx.x;
    float4 pl[HPT];
    int inl[HPT], abv[HPT];
    bool live[HPT], any = false;
#pragma unroll
    for (int j = 0; j < HPT; ++j) {
        const int h = (blockIdx.y * HPT + j) * OP_THREADS + tid;
        live[j] = h < n_hyp && hyp_ok[h] != 0;
        pl[j] = live[j] ? hyp[h] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        inl[j] = abv[j] = 0;
        any = any || live[j];
    }
    const int n_tiles = (n + OP_TILE - 1) / OP_TILE;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int base = tile * OP_TILE, cnt = min(OP_TILE, n - base);
        __syncthreads();                                              // the tile before this one has been read by every wave
        for (int t = tid; t < cnt; t += OP_THREADS) {
            const int32_t i = alive_list[base + t];
            const bool in = i >= 0 && i < n_points;
            const size_t o = in ? (size_t)i * 3 : 0;
            const float nan = __uint_as_float(0x7fc00000u);           // a rank without a point (there is none) scores NaN: below
            s_pt[t] = make_float4(in ? points[o] : nan, in ? points[o + 1] : nan, in ? points[o + 2] : nan, 0.0f);
        }
        __syncthreads();
        if (any) {
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {
                const float4 q = s_pt[t];                             // every lane the same address: a broadcast
#pragma unroll
                for (int j = 0; j < HPT; ++j) {
                    const float s = plane_score(pl[j].x, pl[j].y, pl[j].z, pl[j].w, q.x, q.y, q.z);
                    inl[j] += plane_inlier(s, dist);
                    abv[j] += plane_above(s, dist);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < HPT; ++j) {
        const int h = (blockIdx.y * HPT + j) * OP_THREADS + tid;
        if (!live[j]) continue;
        if (inl[j]) atomicAdd(counts + 2 * h, inl[j]);
        if (abv[j]) atomicAdd(counts + 2 * h + 1, abv[j]);
    }
}

__global__ __launch_bounds__(OP_THREADS) void op_select_kernel(const float4* __restrict__ hyp, const int32_t* __restrict__ hyp_ok,
                                                               const int32_t* __restrict__ counts, int n_points, int n_hyp, int round,
                                                               int min_inliers, int outside_ppm, int32_t* __restrict__ state,
                                                               float* __restrict__ planes, int32_t* __restrict__ plane_counts,
                                                               int32_t* __restrict__ n_planes) {
    __shared__ unsigned long long s_best[OP_THREADS / 64];
    if (state[OP_DONE]) return;
    const int n = state[OP_N];
    if (n < 3 || n > n_points) {                                      // rule 1: fewer than three alive points end the rounds
        if (threadIdx.x == 0) state[OP_DONE] = 1;
        return;
    }
    unsigned long long key = 0ull;
    for (int h = threadIdx.x; h < n_hyp; h += OP_THREADS) {
        if (!hyp_ok[h]) continue;
        const int32_t inliers = counts[2 * h], above = counts[2 * h + 1];
        if (inliers < 0 || above < 0 || inliers + above > n) continue;                       // (cannot happen: both are counts over n points)
        if (!plane_eligible(inliers, above, n, min_inliers, outside_ppm)) continue;
        const unsigned long long k = plane_key(inliers, h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 0; w < OP_THREADS / 64; ++w) key = s_best[w] > key ? s_best[w] : key;
    const int h = plane_key_hypothesis(key);
    if (key == 0ull || h < 0 || h >= n_hyp) {                         // nothing eligible: the rounds end
        state[OP_DONE] = 1;
        state[OP_WIN] = -1;
        return;
    }
    const float4 p = hyp[h];
    const int32_t inliers = counts[2 * h], above = counts[2 * h + 1];
    planes[round * 4] = p.x;
    planes[round * 4 + 1] = p.y;
    planes[round * 4 + 2] = p.z;
    planes[round * 4 + 3] = p.w;
    plane_counts[round * 3] = inliers;
    plane_counts[round * 3 + 1] = above;
    plane_counts[round * 3 + 2] = n - inliers - above;
    *n_planes = round + 1;
    state[OP_WIN] = h;
}

__global__ __launch_bounds__(OP_THREADS) void op_apply_kernel(const float* __restrict__ points, const int32_t* __restrict__ alive_list,
                                                              int n_points, int n_hyp, int round, float dist,
                                                              const int32_t* __restrict__ state, const float4* __restrict__ hyp,
                                                              int32_t* __restrict__ alive, int32_t* __restrict__ plane_id) {
    if (state[OP_DONE]) return;
    const int n = state[OP_N], h = state[OP_WIN];
    if (n < 3 || n > n_points || h < 0 || h >= n_hyp) return;
    const float4 p = hyp[h];
    for (int t = blockIdx.x * OP_THREADS + threadIdx.x; t < n; t += gridDim.x * OP_THREADS) {
        const int32_t i = alive_list[t];
        if (i < 0 || i >= n_points) continue;
        const float s = plane_score(p.x, p.y, p.z, p.w, points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]);
        if (plane_inlier(s, dist)) {
            plane_id[i] = round + 1;
            alive[i] = 0;
        }
    }
}

// ---- clusters ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OP_THREADS) void oc_init_kernel(int n_points, int32_t* __restrict__ parent, int32_t* __restrict__ size,
                                                             int32_t* __restrict__ cluster_size, int32_t* __restrict__ n_clusters) {
    const int v = blockIdx.x * OP_THREADS + threadIdx.x;
    if (v == 0) *n_clusters = 0;
    if (v >= n_points) return;
    parent[v] = v;
    size[v] = 0;
    cluster_size[v] = 0;
}

__global__ __launch_bounds__(OP_THREADS) void oc_link_kernel(const int32_t* __restrict__ nbr, const float* __restrict__ nbr_sqdist,
                                                             const int32_t* __restrict__ mask, int n_points, int k, float max_sq_dist,
                                                             int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * OP_THREADS + threadIdx.x;
    if (e >= (int64_t)n_points * k) return;
    const int i = (int)(e / k), j = nbr[e];
    if (j < 0 || j >= n_points || j == i || !(nbr_sqdist[e] <= max_sq_dist)) return;
    if (mask[i] == 0 || mask[j] == 0) return;
    uf_unite(parent, i, j);
}

// root[v] by plain loads of the finished forest; the size of a component by one add per distinct root of a wave: the lanes of the first
// pending lane's root are counted by a ballot and retire together
__global__ __launch_bounds__(OP_THREADS) void oc_root_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ mask, int n_points,
                                                             int32_t* __restrict__ root, int32_t* __restrict__ size) {
    const int v = blockIdx.x * OP_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int r = -1;
    if (v < n_points) {
        r = uf_root(parent, v, n_points);
        if (r < 0 || r >= n_points) r = v;
        root[v] = r;
    }
    bool todo = v < n_points && mask[v] != 0;
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

__device__ __forceinline__ int oc_kept(const int32_t* __restrict__ root, const int32_t* __restrict__ size, const int32_t* __restrict__ mask,
                                       int n_points, int min_points, int v) {
    return v < n_points && mask[v] != 0 && root[v] == v && size[v] >= min_points;
}

__global__ __launch_bounds__(OP_THREADS) void oc_kept_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                             const int32_t* __restrict__ mask, int n_points, int min_points,
                                                             int32_t* __restrict__ block_kept) {
    __shared__ int s_red[OP_THREADS / 64];
    const int total = block_sum<OP_THREADS>(oc_kept(root, size, mask, n_points, min_points, blockIdx.x * OP_THREADS + threadIdx.x), s_red);
    if (threadIdx.x == 0) block_kept[blockIdx.x] = total;
}

__global__ __launch_bounds__(OP_THREADS) void oc_number_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                               const int32_t* __restrict__ mask, int n_points, int min_points,
                                                               const int32_t* __restrict__ block_kept, int32_t* __restrict__ num,
                                                               int32_t* __restrict__ cluster_size) {
    __shared__ int s_wave[OP_THREADS / 64];
    const int v = blockIdx.x * OP_THREADS + threadIdx.x;
    const int kept = oc_kept(root, size, mask, n_points, min_points, v);
    int total;
    const int at = block_kept[blockIdx.x] + block_scan_excl<OP_THREADS>(kept, s_wave, total);
    if (v >= n_points) return;
    const bool ok = kept && at >= 0 && at < n_points;
    num[v] = ok ? at + 1 : 0;
    if (ok) cluster_size[at] = size[v];
}

__global__ __launch_bounds__(OP_THREADS) void oc_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ num,
                                                              const int32_t* __restrict__ mask, int n_points, int32_t* __restrict__ labels) {
    const int v = blockIdx.x * OP_THREADS + threadIdx.x;
    if (v >= n_points) return;
    const int r = root[v];
    labels[v] = mask[v] != 0 && r >= 0 && r < n_points ? num[r] : 0;
}

static unsigned op_blocks(int64_t n) { return (unsigned)((n + OP_THREADS - 1) / OP_THREADS); }

template <int HPT>
static void launch_score(const float* points, const int32_t* alive_list, int V, int H, float dist, const int32_t* state, const float4* hyp,
                         const int32_t* hyp_ok, int32_t* counts, hipStream_t s) {
    const unsigned groups = (unsigned)((H + OP_THREADS * HPT - 1) / (OP_THREADS * HPT));
    const unsigned tiles = (unsigned)((V + OP_TILE - 1) / OP_TILE), cap = OP_MAX_BLOCKS / groups;
    hipLaunchKernelGGL(op_score_kernel<HPT>, dim3(tiles < cap ? tiles : cap, groups), dim3(OP_THREADS), 0, s, points, alive_list, V, H, dist, state,
                       hyp, hyp_ok, counts);
}

}  // namespace vlsat

using namespace vlsat;

extern "C" {

size_t vlsat_cloud_planes_scratch_bytes(int64_t n_points, int32_t n_hyp) {
    if (!plane_sizes_ok(n_points, n_hyp, 1)) return 0;
    return plane_layout(n_points, n_hyp).bytes;
}

int vlsat_cloud_planes(const float* points, int64_t n_points, int32_t n_hyp, int32_t max_planes, float dist, int32_t min_inliers,
                       int32_t outside_ppm, uint64_t seed, void* scratch, int32_t* plane_id, float* planes, int32_t* plane_counts,
                       int32_t* n_planes, void* stream) {
    if (n_points < 3 || n_points > PLANE_MAX_POINTS) return fail(VLSAT_EINVAL, "cloud_planes: 3 .. 2^24 points");
    if (n_hyp < 1 || n_hyp > PLANE_MAX_HYP) return fail(VLSAT_EINVAL, "cloud_planes: 1 .. 4096 hypotheses");
    if (max_planes < 1 || max_planes > PLANE_MAX_PLANES) return fail(VLSAT_EINVAL, "cloud_planes: 1 .. 32 planes");
    if (!(dist > 0.0f && dist < INFINITY)) return fail(VLSAT_EINVAL, "cloud_planes: dist must be > 0 and finite");
    if (min_inliers < PLANE_MIN_INLIERS) return fail(VLSAT_EINVAL, "cloud_planes: min_inliers must be at least 3");
    if (outside_ppm < 0 || outside_ppm > PLANE_MAX_PPM) return fail(VLSAT_EINVAL, "cloud_planes: outside_ppm must be in 0 .. 500000");
    if (!points || !scratch || !plane_id || !planes || !plane_counts || !n_planes) return fail(VLSAT_EINVAL, "cloud_planes: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int V = (int)n_points, H = (int)n_hyp, P = (int)max_planes;
    const PlaneLayout l = plane_layout(n_points, n_hyp);
    char* base = static_cast<char*>(scratch);
    int32_t* state = reinterpret_cast<int32_t*>(base + l.state);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(base + l.best);
    float4* hyp = reinterpret_cast<float4*>(base + l.hyp);
    int32_t* hyp_ok = reinterpret_cast<int32_t*>(base + l.hyp_ok);
    int32_t* counts = reinterpret_cast<int32_t*>(base + l.counts);
    int32_t* alive = reinterpret_cast<int32_t*>(base + l.alive);
    int32_t* alive_list = reinterpret_cast<int32_t*>(base + l.alive_list);
    int32_t* block_alive = reinterpret_cast<int32_t*>(base + l.block_alive);
    const unsigned blocks = op_blocks(V), apply_blocks = blocks < (unsigned)OP_MAX_BLOCKS ? blocks : (unsigned)OP_MAX_BLOCKS;
    hipLaunchKernelGGL(op_init_kernel, dim3(blocks), dim3(OP_THREADS), 0, s, points, V, P, alive, plane_id, planes, plane_counts, n_planes, state);
    for (int r = 0; r < P; ++r) {
        hipLaunchKernelGGL(op_count_kernel, dim3(blocks), dim3(OP_THREADS), 0, s, (const int32_t*)alive, V, block_alive);
        launch_scan_i32(block_alive, (int)blocks, block_alive, state + OP_N, nullptr, s);       // in place; state[N] = the total <= V
        hipLaunchKernelGGL(op_scatter_kernel, dim3(blocks), dim3(OP_THREADS), 0, s, (const int32_t*)alive, V, (const int32_t*)block_alive,
                           (const int32_t*)state, alive_list);
        hipLaunchKernelGGL(op_hypotheses_kernel, dim3(op_blocks(H)), dim3(OP_THREADS), 0, s, points, (const int32_t*)alive_list, V, H, r,
                           (unsigned long long)seed, (const int32_t*)state, hyp, hyp_ok, counts, best);
        if (H <= OP_THREADS)
            launch_score<1>(points, alive_list, V, H, dist, state, hyp, hyp_ok, counts, s);
        else if (H <= 2 * OP_THREADS)
            launch_score<2>(points, alive_list, V, H, dist, state, hyp, hyp_ok, counts, s);
        else
            launch_score<4>(points, alive_list, V, H, dist, state, hyp, hyp_ok, counts, s);
        hipLaunchKernelGGL(op_select_kernel, dim3(1), dim3(OP_THREADS), 0, s, (const float4*)hyp, (const int32_t*)hyp_ok, (const int32_t*)counts, V,
                           H, r, (int)min_inliers, (int)outside_ppm, state, planes, plane_counts, n_planes);
        hipLaunchKernelGGL(op_apply_kernel, dim3(apply_blocks), dim3(OP_THREADS), 0, s, points, (const int32_t*)alive_list, V, H, r, dist,
                           (const int32_t*)state, (const float4*)hyp, alive, plane_id);
    }
    VLSAT_LAUNCH_CHECK("cloud_planes");
    return 0;
}

size_t vlsat_cloud_clusters_scratch_bytes(int64_t n_points) {
    if (!cluster_sizes_ok(n_points, 1)) return 0;
    return cluster_layout(n_points).bytes;
}

int vlsat_cloud_clusters(const int32_t* nbr, const float* nbr_sqdist, const int32_t* mask, int64_t n_points, int32_t k, float max_sq_dist,
                         int32_t min_points, void* scratch, int32_t* labels, int32_t* n_clusters, int32_t* cluster_size, void* stream) {
    if (!cluster_sizes_ok(n_points, k)) return fail(VLSAT_EINVAL, "cloud_clusters: 1 .. 2^24 points and 1 .. 32 neighbours");
    if (max_sq_dist != max_sq_dist) return fail(VLSAT_EINVAL, "cloud_clusters: max_sq_dist is NaN");
    if (min_points < 1) return fail(VLSAT_EINVAL, "cloud_clusters: min_points must be at least 1");
    if (!nbr || !nbr_sqdist || !mask || !scratch || !labels || !n_clusters || !cluster_size)
        return fail(VLSAT_EINVAL, "cloud_clusters: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int V = (int)n_points, K = (int)k;
    const ClusterLayout l = cluster_layout(n_points);
    char* base = static_cast<char*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(base + l.parent);
    int32_t* root = reinterpret_cast<int32_t*>(base + l.root);
    int32_t* size = reinterpret_cast<int32_t*>(base + l.size);
    int32_t* num = reinterpret_cast<int32_t*>(base + l.num);
    int32_t* block_kept = reinterpret_cast<int32_t*>(base + l.block_kept);
    const dim3 block(OP_THREADS), per_point(op_blocks(V)), per_entry(op_blocks((int64_t)V * K));
    hipLaunchKernelGGL(oc_init_kernel, per_point, block, 0, s, V, parent, size, cluster_size, n_clusters);
    hipLaunchKernelGGL(oc_link_kernel, per_entry, block, 0, s, nbr, nbr_sqdist, mask, V, K, max_sq_dist, parent);
    hipLaunchKernelGGL(oc_root_kernel, per_point, block, 0, s, (const int32_t*)parent, mask, V, root, size);
    hipLaunchKernelGGL(oc_kept_kernel, per_point, block, 0, s, (const int32_t*)root, (const int32_t*)size, mask, V, (int)min_points, block_kept);
    launch_scan_i32(block_kept, (int)per_point.x, block_kept, n_clusters, nullptr, s);           // in place; the total is S <= V
    hipLaunchKernelGGL(oc_number_kernel, per_point, block, 0, s, (const int32_t*)root, (const int32_t*)size, mask, V, (int)min_points,
                       (const int32_t*)block_kept, num, cluster_size);
    hipLaunchKernelGGL(oc_label_kernel, per_point, block, 0, s, (const int32_t*)root, (const int32_t*)num, mask, V, labels);
    VLSAT_LAUNCH_CHECK("cloud_clusters");
    return 0;
}

}  // extern "C"
