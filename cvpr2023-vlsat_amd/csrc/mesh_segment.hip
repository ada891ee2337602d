// An unlabelled mesh over-segmented into segments (include/vlsat_segment.h states the rule; prep.segment_mesh_host restates it in
// numpy with the same operations): smoothness-constrained region growing -- connected components of the edges whose normals agree --
// then R rounds in which every small component joins its best neighbour, then dense numbering.  The weight, the key packing, the round
// count and the scratch layout are segment_core.h's.  The union-find is union_find.h's (a tree's root is its lowest vertex); a launch
// boundary is the only cross-block ordering.
//
// Launches, V vertices, M edges, R = seg_rounds(min_verts):
//   ms_init_kernel           parent[v] = v, seg_size[v] = 0, n_segments = 0
//   ms_link_kernel           (M > 0) one thread per edge: w <= max_weight unites the ends
//   ms_flatten_kernel        root[v] = the end of v's parent walk (reads parent, writes nothing anyone reads in this launch);
//                            size[v] = 0, key[v] = none
//   R x  ms_count_kernel     size[root[v]] += 1, one add per distinct root of a wave; parent[v] = root[v]: every tree has depth 1 again
//        ms_choose_kernel    (M > 0) one thread per edge between two components: atomicMin of (w, other root) on the key of each SMALL end;
//                            root[] is the flattened state of the previous launch, nothing here changes it
//        ms_hook_kernel      (M > 0) a small root with a key unites with its target
//        ms_flatten_kernel   (M > 0)
//   ms_count_kernel          the final sizes
//   ms_flag_count_kernel     per tile of 1024 vertices the number of kept roots (root[v] == v and size >= min_verts)
//   scan_i32_kernel          exclusive scan of the tile counts (at most 2^14 of them: one block); the total is S
//   ms_number_kernel         per tile: num[v] = 1 + tile's first + rank inside the tile for a kept root, else 0; seg_size[num - 1] = size
//   ms_label_kernel          labels[v] = num[root[v]]
// With M == 0 no round can change anything and only the counts are run: 7 launches; otherwise 8 + 4 R.
// Nothing depends on the order blocks run in: minima define roots and choices, sums are integer.  The hot root (a floor holds a third of
// all vertices) is read by many and written by none once it is the lowest vertex of its component (union_find.h); its size takes one add
// per wave and distinct root.
// build.py compiles THIS file with -ffp-contract=off (PER_SOURCE_FLAGS): seg_weight rounds every product and sum on its own.
//
// vlsat_segment_cloud (include/vlsat_cloud.h) runs the same launches over a cloud's neighbour table: the edge loader and the weight are
// template parameters of ms_link_kernel and ms_choose_kernel (MsEdgeList | MsNbrTable, signed | unsigned), and vlsat_segment_mesh
// instantiates what it always ran.
#include "../../include/vlsat_cloud.h"
#include "../../include/vlsat_segment.h"
#include "cloud_core.h"
#include "common.h"
#include "kernels.h"
#include "segment_core.h"
#include "union_find.h"
#include "wave_core.h"

namespace vlsat {

constexpr int MS_THREADS = 256;
constexpr int MS_PER_THREAD = SEG_NUMBER_TILE / MS_THREADS;
static_assert(MS_PER_THREAD * MS_THREADS == SEG_NUMBER_TILE, "a numbering tile is a whole number of vertices per thread");

// Where the edges come from -- a template parameter of the two kernels that read them: an explicit list (a mesh), or the neighbour
// table of a cloud, whose edge e joins point e / K and nbr[e] (a -1 entry fails seg_edge_ok like any end out of range).
struct MsEdge { int a, b; bool ok; };
__device__ __forceinline__ MsEdge ms_checked(int a, int b, int n_verts) {
    MsEdge r;
    r.ok = seg_edge_ok(a, b, n_verts);
    r.a = r.ok ? a : 0;
    r.b = r.ok ? b : 0;
    return r;
}
struct MsEdgeList {
    const int32_t* edges;
    __device__ __forceinline__ MsEdge load(int n_verts, int64_t e) const { return ms_checked(edges[(size_t)e * 2], edges[(size_t)e * 2 + 1], n_verts); }
};
struct MsNbrTable {
    const int32_t* nbr;
    int k;
    __device__ __forceinline__ MsEdge load(int n_verts, int64_t e) const { return ms_checked((int)(e / k), nbr[e], n_verts); }
};
// UNSIGNED: the weight of unoriented normals, fl(1 - |d|) (cloud_core.h); else seg_weight.
template <bool UNSIGNED>
__device__ __forceinline__ float ms_weight(const float* __restrict__ normals, int a, int b) {
    const float* na = normals + (size_t)a * 3;
    const float* nb = normals + (size_t)b * 3;
    if (UNSIGNED) return cloud_unsigned_weight(na[0], na[1], na[2], nb[0], nb[1], nb[2]);
    return seg_weight(na[0], na[1], na[2], nb[0], nb[1], nb[2]);
}

__global__ __launch_bounds__(MS_THREADS) void ms_init_kernel(int n_verts, int32_t* __restrict__ parent, int32_t* __restrict__ seg_size,
                                                             int32_t* __restrict__ n_segments) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v == 0) *n_segments = 0;
    if (v >= n_verts) return;
    parent[v] = v;
    seg_size[v] = 0;
}

template <class Edges, bool UNSIGNED>
__global__ __launch_bounds__(MS_THREADS) void ms_link_kernel(const float* __restrict__ normals, const Edges edges, int n_verts,
                                                             int64_t n_edges, float max_weight, int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const MsEdge ed = edges.load(n_verts, e);
    if (!ed.ok || !(ms_weight<UNSIGNED>(normals, ed.a, ed.b) <= max_weight)) return;
    uf_unite(parent, ed.a, ed.b);
}

__global__ __launch_bounds__(MS_THREADS) void ms_flatten_kernel(const int32_t* __restrict__ parent, int n_verts, int32_t* __restrict__ root,
                                                                int32_t* __restrict__ size, unsigned long long* __restrict__ key) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= n_verts) return;
    root[v] = uf_root(parent, v, n_verts);
    size[v] = 0;
    key[v] = SEG_NO_KEY;
}

// One add per distinct root of a wave: the lanes of the first pending lane's root are counted by a ballot and retire together.
__global__ __launch_bounds__(MS_THREADS) void ms_count_kernel(const int32_t* __restrict__ root, int n_verts, int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ size) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    bool todo = v < n_verts;
    int r = todo ? root[v] : -1;
    if (todo && (r < 0 || r >= n_verts)) { r = -1; todo = false; }
    if (todo) parent[v] = r;
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

template <class Edges, bool UNSIGNED>
__global__ __launch_bounds__(MS_THREADS) void ms_choose_kernel(const float* __restrict__ normals, const Edges edges, int n_verts,
                                                               int64_t n_edges, int min_verts, const int32_t* __restrict__ root,
                                                               const int32_t* __restrict__ size, unsigned long long* __restrict__ key) {
    const int64_t e = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const MsEdge ed = edges.load(n_verts, e);
    if (!ed.ok) return;
    const int ra = root[ed.a], rb = root[ed.b];
    if (ra == rb || ra < 0 || rb < 0 || ra >= n_verts || rb >= n_verts) return;
    const bool small_a = size[ra] < min_verts, small_b = size[rb] < min_verts;
    if (!small_a && !small_b) return;
    const float w = ms_weight<UNSIGNED>(normals, ed.a, ed.b);         // symmetric: the edge stands for both of its directions
    if (small_a) atomicMin(key + ra, seg_key(w, rb));
    if (small_b) atomicMin(key + rb, seg_key(w, ra));
}

__global__ __launch_bounds__(MS_THREADS) void ms_hook_kernel(int n_verts, int min_verts, const int32_t* __restrict__ root,
                                                             const int32_t* __restrict__ size, const unsigned long long* __restrict__ key,
                                                             int32_t* __restrict__ parent) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= n_verts || root[v] != v || size[v] >= min_verts) return;
    const unsigned long long k = key[v];
    if (k == SEG_NO_KEY) return;
    const int target = seg_key_root(k);
    if (target < 0 || target >= n_verts) return;
    uf_unite(parent, v, target);
}

// ---- dense numbering: per-tile counts, a scan of the counts, then apply --------------------------------------------------------------
__device__ __forceinline__ bool ms_kept(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_verts, int min_verts, int v) {
    return v < n_verts && root[v] == v && size[v] >= min_verts;
}

__global__ __launch_bounds__(MS_THREADS) void ms_flag_count_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_verts,
                                                                   int min_verts, int32_t* __restrict__ block_count) {
    __shared__ int wave_sum[MS_THREADS / 64];
    const int v0 = blockIdx.x * SEG_NUMBER_TILE + threadIdx.x * MS_PER_THREAD;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < MS_PER_THREAD; ++k) mine += ms_kept(root, size, n_verts, min_verts, v0 + k);
    const int total = block_sum<MS_THREADS>(mine, wave_sum);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(MS_THREADS) void ms_number_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int n_verts,
                                                               int min_verts, const int32_t* __restrict__ block_first, int32_t* __restrict__ num,
                                                               int32_t* __restrict__ seg_size) {
    __shared__ int wave_sum[MS_THREADS / 64];
    const int v0 = blockIdx.x * SEG_NUMBER_TILE + threadIdx.x * MS_PER_THREAD;
    bool kept[MS_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < MS_PER_THREAD; ++k) { kept[k] = ms_kept(root, size, n_verts, min_verts, v0 + k); mine += kept[k]; }
    int total;
    int at = block_first[blockIdx.x] + block_scan_excl<MS_THREADS>(mine, wave_sum, total);
#pragma unroll
    for (int k = 0; k < MS_PER_THREAD; ++k) {
        const int v = v0 + k;
        if (v >= n_verts) break;
        if (kept[k] && at >= 0 && at < n_verts) {
            num[v] = at + 1;
            seg_size[at] = size[v];
            ++at;
        } else {
            num[v] = 0;
        }
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ num, int n_verts,
                                                              int32_t* __restrict__ labels) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= n_verts) return;
    const int r = root[v];
    labels[v] = r >= 0 && r < n_verts ? num[r] : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int segment_mesh_check_args(int64_t V, int64_t M) {
    if (!seg_sizes_ok(V, M)) return fail(VLSAT_EINVAL, "segment_mesh: 1 .. 2^24 vertices and 0 .. 2^31 - 1 edges");
    return 0;
}

template <class Edges, bool UNSIGNED>
static int launch_segment(const char* what, const float* normals, const Edges edges, int64_t n_verts, int64_t n_edges, float max_weight, int min_verts,
                               void* scratch, int32_t* labels, int32_t* n_segments, int32_t* seg_size, hipStream_t s) {
    const int V = (int)n_verts;
    const int64_t M = n_edges;
    const SegScratch lay = seg_scratch_layout(n_verts);
    char* p = static_cast<char*>(scratch);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(p + lay.key);
    int32_t* parent = reinterpret_cast<int32_t*>(p + lay.parent);
    int32_t* root = reinterpret_cast<int32_t*>(p + lay.root);
    int32_t* size = reinterpret_cast<int32_t*>(p + lay.size);
    int32_t* num = reinterpret_cast<int32_t*>(p + lay.num);
    int32_t* block_count = reinterpret_cast<int32_t*>(p + lay.block_count);
    int32_t* block_first = reinterpret_cast<int32_t*>(p + lay.block_first);

    const dim3 block(MS_THREADS), per_vertex((unsigned)((V + MS_THREADS - 1) / MS_THREADS)),
        per_edge((unsigned)((M + MS_THREADS - 1) / MS_THREADS)), per_tile((unsigned)lay.tiles);
    hipLaunchKernelGGL(ms_init_kernel, per_vertex, block, 0, s, V, parent, seg_size, n_segments);
    if (M > 0) hipLaunchKernelGGL((ms_link_kernel<Edges, UNSIGNED>), per_edge, block, 0, s, normals, edges, V, M, max_weight, parent);
    hipLaunchKernelGGL(ms_flatten_kernel, per_vertex, block, 0, s, (const int32_t*)parent, V, root, size, key);
    const int rounds = M > 0 ? seg_rounds(min_verts) : 0;              // without an edge no component has a neighbour
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(ms_count_kernel, per_vertex, block, 0, s, (const int32_t*)root, V, parent, size);
        hipLaunchKernelGGL((ms_choose_kernel<Edges, UNSIGNED>), per_edge, block, 0, s, normals, edges, V, M, min_verts, (const int32_t*)root, (const int32_t*)size, key);
        hipLaunchKernelGGL(ms_hook_kernel, per_vertex, block, 0, s, V, min_verts, (const int32_t*)root, (const int32_t*)size,
                           (const unsigned long long*)key, parent);
        hipLaunchKernelGGL(ms_flatten_kernel, per_vertex, block, 0, s, (const int32_t*)parent, V, root, size, key);
    }
    hipLaunchKernelGGL(ms_count_kernel, per_vertex, block, 0, s, (const int32_t*)root, V, parent, size);
    hipLaunchKernelGGL(ms_flag_count_kernel, per_tile, block, 0, s, (const int32_t*)root, (const int32_t*)size, V, min_verts, block_count);
    launch_scan_i32(block_count, (int)lay.tiles, block_first, n_segments, nullptr, s);
    hipLaunchKernelGGL(ms_number_kernel, per_tile, block, 0, s, (const int32_t*)root, (const int32_t*)size, V, min_verts,
                       (const int32_t*)block_first, num, seg_size);
    hipLaunchKernelGGL(ms_label_kernel, per_vertex, block, 0, s, (const int32_t*)root, (const int32_t*)num, V, labels);
    VLSAT_LAUNCH_CHECK(what);
    return 0;
}

}  // namespace vlsat

using namespace vlsat;

extern "C" {

size_t vlsat_segment_mesh_scratch_bytes(int64_t n_verts, int64_t n_edges) {
    if (!seg_sizes_ok(n_verts, n_edges)) return 0;
    return seg_scratch_layout(n_verts).bytes;
}

int vlsat_segment_mesh(const float* normals, const int32_t* edges, int64_t n_verts, int64_t n_edges, float max_weight, int32_t min_verts,
                       void* scratch, int32_t* labels, int32_t* n_segments, int32_t* seg_size, void* stream) {
    if (segment_mesh_check_args(n_verts, n_edges)) return VLSAT_EINVAL;
    if (max_weight != max_weight) return fail(VLSAT_EINVAL, "segment_mesh: max_weight is NaN");
    if (!normals || !scratch || !labels || !n_segments || !seg_size) return fail(VLSAT_EINVAL, "segment_mesh: null argument");
    if (n_edges > 0 && !edges) return fail(VLSAT_EINVAL, "segment_mesh: null edge list");
    return launch_segment<MsEdgeList, false>("segment_mesh", normals, MsEdgeList{edges}, n_verts, n_edges, max_weight, min_verts, scratch, labels,
                                             n_segments, seg_size, static_cast<hipStream_t>(stream));
}

// include/vlsat_cloud.h: the same rules over the directed pairs (e / K, nbr[e]), e < V K
int vlsat_segment_cloud(const float* normals, const int32_t* nbr, int64_t n_points, int32_t k, float max_weight, int32_t min_verts,
                        int32_t unsigned_dot, void* scratch, int32_t* labels, int32_t* n_segments, int32_t* seg_size, void* stream) {
    if (!cloud_sizes_ok(n_points, k)) return fail(VLSAT_EINVAL, "segment_cloud: 1 .. 2^24 points and 1 .. 32 neighbours");
    if (max_weight != max_weight) return fail(VLSAT_EINVAL, "segment_cloud: max_weight is NaN");
    if (!normals || !nbr || !scratch || !labels || !n_segments || !seg_size) return fail(VLSAT_EINVAL, "segment_cloud: null argument");
    const int64_t n_edges = n_points * k;                              // at most 2^29
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MsNbrTable table{nbr, (int)k};
    if (unsigned_dot)
        return launch_segment<MsNbrTable, true>("segment_cloud", normals, table, n_points, n_edges, max_weight, min_verts, scratch, labels,
                                                n_segments, seg_size, s);
    return launch_segment<MsNbrTable, false>("segment_cloud", normals, table, n_points, n_edges, max_weight, min_verts, scratch, labels,
                                             n_segments, seg_size, s);
}

}  // extern "C"
