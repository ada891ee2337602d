// Segments of an over-segmentation merged into objects along "same part" edges: connected components of the link graph, pooled node
// probabilities, and the edge list folded onto the objects.  The rule is stated in include/vlsat.h (vlsat_merge_segments);
// metrics.merge_segments_host restates it in numpy with the same operations.
//
// Launches (every launch boundary is the only cross-block ordering this file relies on; inside a launch blocks meet only in device-scope
// integer atomics):
//   sm_clear_kernel          parent[n] = n, counters and every output to their "past the end" value
//   sm_table_clear_kernel    the open-addressing table (64-bit keys, capacity = the power of two >= 2 E: at most half full)
//   sm_link_insert_kernel    mutual only: key (a, b) of every edge that passes the threshold
//   sm_union_kernel          every link unites its two rows (union_find.h: a tree's root is its lowest row)
//   sm_flatten_kernel        root[n], is_root[n]
//   scan_i32_kernel          exclusive scan (one block; a thread owns a contiguous run: wave_core.h) -> dense object numbers, M
//   sm_object_kernel         object[n], member counts, obj_batch_ids, n_objects
//   scan_i32_kernel          -> member_ptr
//   sm_members_kernel        one wave per object: the rows from its root to the end of its scene, compacted in order by ballot prefixes
//   sm_pool_kernel           one wave per object, lanes over classes, members in order: s = fl(s + fl(w p)), W = fl(W + w), fl(s / W)
//   sm_pair_insert_kernel    key (object[a], object[b]) of every edge between two objects; atomicMin of the edge row per key
//   sm_pair_flag_kernel      an edge is the representative of its pair when it is that minimum
//   scan_i32_kernel          -> pair numbers in the order of the representatives, E'
//   sm_pair_emit_kernel      one thread per (edge, predicate): atomicMax on the float bits (values >= 0), counts, pair_edges
// Nothing here depends on the order blocks run in: minima define roots and pair order, maxima the pair probabilities, the member order
// the sums.  build.py compiles THIS file with -ffp-contract=off (PER_SOURCE_FLAGS) so that the pooled sum rounds w * p and the addition
// separately.
#include "common.h"
#include "kernels.h"
#include "union_find.h"
#include "wave_core.h"

namespace vlsat {

constexpr int SM_THREADS = 256;
constexpr int SM_SCAN_THREADS = 1024;
constexpr unsigned long long SM_EMPTY = ~0ull;          // never a key: both halves of a key are below 2^31
constexpr int SM_NONE = 0x7fffffff;

__device__ __forceinline__ unsigned sm_hash(unsigned long long k, unsigned mask) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k & mask;
}
// the slot of `key`, claiming an empty one when it is new; -1 when the table is full (it never is: capacity >= 2 E)
__device__ __forceinline__ int sm_table_insert(unsigned long long* __restrict__ keys, unsigned mask, unsigned long long key) {
    unsigned slot = sm_hash(key, mask);
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(keys + slot, SM_EMPTY, key);
        if (prev == SM_EMPTY || prev == key) return (int)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}
// (a launch after the inserts: plain loads)
__device__ __forceinline__ bool sm_table_has(const unsigned long long* __restrict__ keys, unsigned mask, unsigned long long key) {
    unsigned slot = sm_hash(key, mask);
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long k = keys[slot];
        if (k == key) return true;
        if (k == SM_EMPTY) return false;
        slot = (slot + 1) & mask;
    }
    return false;
}

struct SmEdge { int a, b; bool ok; };                   // ok: both rows in range, a != b, same scene
__device__ __forceinline__ SmEdge sm_edge(const int64_t* __restrict__ edges, const int64_t* __restrict__ bid, int n_nodes, int64_t e) {
    const int64_t a = edges[e * 2], b = edges[e * 2 + 1];
    SmEdge r;
    r.ok = a >= 0 && b >= 0 && a < n_nodes && b < n_nodes && a != b;
    r.a = r.ok ? (int)a : 0;
    r.b = r.ok ? (int)b : 0;
    if (r.ok && bid) r.ok = bid[r.a] == bid[r.b];
    return r;
}

__global__ __launch_bounds__(SM_THREADS) void sm_clear_kernel(int n_nodes, int n_edges, int C, int R, int n_scenes, int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ cnt, int32_t* __restrict__ slot_of,
                                                              int32_t* __restrict__ root, int32_t* __restrict__ object,
                                                              int32_t* __restrict__ n_objects, int32_t* __restrict__ totals,
                                                              int32_t* __restrict__ members, float* __restrict__ obj_probs,
                                                              float* __restrict__ obj_weight, int64_t* __restrict__ obj_bid,
                                                              int32_t* __restrict__ edge_to_pair, int64_t* __restrict__ pair_edges,
                                                              int32_t* __restrict__ pair_count, float* __restrict__ pair_probs) {
    const int64_t stride = (int64_t)gridDim.x * SM_THREADS, t0 = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    for (int64_t i = t0; i < n_nodes; i += stride) {
        parent[i] = (int)i; cnt[i] = 0; root[i] = -1; object[i] = -1; members[i] = -1; obj_weight[i] = 0.0f; obj_bid[i] = -1;
    }
    for (int64_t i = t0; i < (int64_t)n_nodes * C; i += stride) obj_probs[i] = 0.0f;
    for (int64_t i = t0; i < n_edges; i += stride) {
        slot_of[i] = -1; edge_to_pair[i] = -1; pair_edges[i * 2] = -1; pair_edges[i * 2 + 1] = -1; pair_count[i] = 0;
    }
    for (int64_t i = t0; i < (int64_t)n_edges * R; i += stride) pair_probs[i] = 0.0f;
    for (int64_t i = t0; i < n_scenes; i += stride) n_objects[i] = 0;
    if (t0 < 2) totals[t0] = 0;
}

__global__ __launch_bounds__(SM_THREADS) void sm_table_clear_kernel(unsigned long long* __restrict__ keys, int32_t* __restrict__ slot_min,
                                                                    int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; i < cap; i += (int64_t)gridDim.x * SM_THREADS) {
        keys[i] = SM_EMPTY;
        slot_min[i] = SM_NONE;
    }
}

// ---- links and components ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_THREADS) void sm_link_insert_kernel(const float* __restrict__ rel_probs, const int64_t* __restrict__ edges,
                                                                    const int64_t* __restrict__ bid, int n_nodes, int n_edges, int R,
                                                                    int same_part, float threshold, unsigned long long* __restrict__ keys,
                                                                    unsigned mask) {
    const int64_t e = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const SmEdge ed = sm_edge(edges, bid, n_nodes, e);
    if (!ed.ok || !(rel_probs[e * R + same_part] >= threshold)) return;
    sm_table_insert(keys, mask, ((unsigned long long)(unsigned)ed.a << 32) | (unsigned)ed.b);
}

template <bool MUTUAL>
__global__ __launch_bounds__(SM_THREADS) void sm_union_kernel(const float* __restrict__ rel_probs, const int64_t* __restrict__ edges,
                                                              const int64_t* __restrict__ bid, int n_nodes, int n_edges, int R, int same_part,
                                                              float threshold, const unsigned long long* __restrict__ keys, unsigned mask,
                                                              int32_t* __restrict__ parent) {
    const int64_t e = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const SmEdge ed = sm_edge(edges, bid, n_nodes, e);
    if (!ed.ok || !(rel_probs[e * R + same_part] >= threshold)) return;
    if (MUTUAL && !sm_table_has(keys, mask, ((unsigned long long)(unsigned)ed.b << 32) | (unsigned)ed.a)) return;
    uf_unite(parent, ed.a, ed.b);
}

__global__ __launch_bounds__(SM_THREADS) void sm_flatten_kernel(const int32_t* __restrict__ parent, int n_nodes, int32_t* __restrict__ root,
                                                                int32_t* __restrict__ flag) {
    const int n = blockIdx.x * SM_THREADS + threadIdx.x;
    if (n >= n_nodes) return;
    const int r = uf_root(parent, n, n_nodes);
    root[n] = r;
    flag[n] = r == n;
}

// out[0..n] = exclusive scan of in[0..n-1]; *total = *total2 = out[n] (either may be null).  One block; out may be in.
__global__ __launch_bounds__(SM_SCAN_THREADS) void scan_i32_kernel(const int32_t* in, int n, int32_t* out, int32_t* __restrict__ total,
                                                                   int32_t* __restrict__ total2) {
    __shared__ int s_wave[SM_SCAN_THREADS / 64];
    const RunScan<int> r = block_run_scan<SM_SCAN_THREADS>(in, n, s_wave);
    int acc = r.before;
    for (int i = r.b; i < r.e; ++i) { const int v = in[i]; out[i] = acc; acc += v; }
    if (threadIdx.x == 0) { out[n] = r.total; if (total) *total = r.total; if (total2) *total2 = r.total; }
}

__global__ __launch_bounds__(SM_THREADS) void sm_object_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ num,
                                                               const int64_t* __restrict__ bid, int n_nodes, int n_scenes,
                                                               int32_t* __restrict__ object, int32_t* __restrict__ cnt,
                                                               int32_t* __restrict__ obj_root, int64_t* __restrict__ obj_bid,
                                                               int32_t* __restrict__ n_objects) {
    const int n = blockIdx.x * SM_THREADS + threadIdx.x;
    if (n >= n_nodes) return;
    const int r = root[n], o = num[r];
    if (o < 0 || o >= n_nodes) return;
    object[n] = o;
    atomicAdd(cnt + o, 1);
    if (r == n) {
        const int64_t s = bid ? bid[n] : 0;
        obj_root[o] = n;
        obj_bid[o] = s;
        if (s >= 0 && s < n_scenes) atomicAdd(n_objects + s, 1);
    }
}

// ---- members and pooled probabilities: one wave per object (fuse_splits of scene_split.hip runs the same two kernels: there root[n]
// is the first row of n's instance id and bid is null, so "root[n] == r" selects the rows of the object and no scene ends the walk) ----
__global__ __launch_bounds__(SM_THREADS) void sm_members_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ obj_root,
                                                                const int32_t* __restrict__ member_ptr, const int64_t* __restrict__ bid,
                                                                const int32_t* __restrict__ totals, int n_nodes, int32_t* __restrict__ members) {
    const int o = blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= n_nodes || o >= totals[0]) return;
    const int r = obj_root[o];
    if (r < 0 || r >= n_nodes) return;
    const int64_t scene = bid ? bid[r] : 0;
    int pos = member_ptr[o];
    const int end = member_ptr[o + 1];
    for (int n0 = r; n0 < n_nodes && pos < end; n0 += 64) {           // members lie in [r, end of r's scene); all of them found: stop
        const int n = n0 + lane;
        const bool in = n < n_nodes, mine = in && root[n] == r;
        const bool other = in && bid && bid[n] != scene;
        const unsigned long long m = __ballot(mine);
        const int p = pos + (int)__popcll(m & ((1ull << lane) - 1));
        if (mine && p >= 0 && p < end && p < n_nodes) members[p] = n;
        pos += (int)__popcll(m);
        if (__ballot(other)) break;
    }
}

__global__ __launch_bounds__(SM_THREADS) void sm_pool_kernel(const float* __restrict__ obj_probs, const float* __restrict__ weights,
                                                             const int32_t* __restrict__ members, const int32_t* __restrict__ member_ptr,
                                                             const int32_t* __restrict__ totals, int n_nodes, int C,
                                                             float* __restrict__ out_probs, float* __restrict__ out_weight) {
    const int o = blockIdx.x * (SM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= n_nodes || o >= totals[0]) return;
    const int m0 = max(member_ptr[o], 0), m1 = min(member_ptr[o + 1], n_nodes);
    float W = 0.0f;
    for (int k = m0; k < m1; ++k) {
        const int i = members[k];
        if (i < 0 || i >= n_nodes) continue;
        W = __fadd_rn(W, weights ? weights[i] : 1.0f);
    }
    for (int c = lane; c < C; c += 64) {
        float s = 0.0f;
        for (int k = m0; k < m1; ++k) {
            const int i = members[k];
            if (i < 0 || i >= n_nodes) continue;
            s = __fadd_rn(s, __fmul_rn(weights ? weights[i] : 1.0f, obj_probs[(size_t)i * C + c]));
        }
        out_probs[(size_t)o * C + c] = __fdiv_rn(s, W);
    }
    if (lane == 0) out_weight[o] = W;
}

// ---- merged edges -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_THREADS) void sm_pair_insert_kernel(const int64_t* __restrict__ edges, const int64_t* __restrict__ bid,
                                                                    const int32_t* __restrict__ object, int n_nodes, int n_edges,
                                                                    unsigned long long* __restrict__ keys, int32_t* __restrict__ slot_min,
                                                                    unsigned mask, int32_t* __restrict__ slot_of) {
    const int64_t e = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const SmEdge ed = sm_edge(edges, bid, n_nodes, e);
    if (!ed.ok) return;
    const int oa = object[ed.a], ob = object[ed.b];
    if (oa < 0 || ob < 0 || oa == ob) return;
    const int slot = sm_table_insert(keys, mask, ((unsigned long long)(unsigned)oa << 32) | (unsigned)ob);
    if (slot < 0) return;
    atomicMin(slot_min + slot, (int)e);
    slot_of[e] = slot;
}

__global__ __launch_bounds__(SM_THREADS) void sm_pair_flag_kernel(const int32_t* __restrict__ slot_of, const int32_t* __restrict__ slot_min,
                                                                  int n_edges, int32_t* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const int slot = slot_of[e];
    flag[e] = slot >= 0 && slot_min[slot] == (int)e;
}

__global__ __launch_bounds__(SM_THREADS) void sm_pair_emit_kernel(const float* __restrict__ rel_probs, const int64_t* __restrict__ edges,
                                                                  const int32_t* __restrict__ object, const int32_t* __restrict__ slot_of,
                                                                  const int32_t* __restrict__ slot_min, const int32_t* __restrict__ num,
                                                                  int n_edges, int R, int32_t* __restrict__ edge_to_pair,
                                                                  int64_t* __restrict__ pair_edges, int32_t* __restrict__ pair_count,
                                                                  unsigned* __restrict__ pair_probs) {
    const int64_t t = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (t >= (int64_t)n_edges * R) return;
    const int64_t e = t / R;
    const int r = (int)(t - e * R);
    const int slot = slot_of[e];
    if (slot < 0) return;
    const int rep = slot_min[slot];
    if (rep < 0 || rep >= n_edges) return;
    const int p = num[rep];
    if (p < 0 || p >= n_edges) return;
    atomicMax(pair_probs + (size_t)p * R + r, __float_as_uint(rel_probs[t]));       // values >= 0: the bit order is the value order
    if (r != 0) return;
    edge_to_pair[e] = p;
    atomicAdd(pair_count + p, 1);
    if (rep == (int)e) {                                              // (slot_of[e] >= 0: both rows were checked by sm_edge)
        pair_edges[(size_t)p * 2] = object[edges[e * 2]];
        pair_edges[(size_t)p * 2 + 1] = object[edges[e * 2 + 1]];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// (the three launchers below leave the launch check to their caller, which names the entry point)
void launch_scan_i32(const int32_t* in, int n, int32_t* out, int32_t* total, int32_t* total2, hipStream_t s) {
    hipLaunchKernelGGL(scan_i32_kernel, dim3(1), dim3(SM_SCAN_THREADS), 0, s, in, n, out, total, total2);
}
static dim3 sm_waves(int n) { return dim3((unsigned)((n + SM_THREADS / 64 - 1) / (SM_THREADS / 64))); }
void launch_members(const int32_t* root, const int32_t* obj_root, const int32_t* member_ptr, const int64_t* bid, const int32_t* totals, int n,
                    int32_t* members, hipStream_t s) {
    hipLaunchKernelGGL(sm_members_kernel, sm_waves(n), dim3(SM_THREADS), 0, s, root, obj_root, member_ptr, bid, totals, n, members);
}
void launch_pool_members(const float* probs, const float* weights, const int32_t* members, const int32_t* member_ptr, const int32_t* totals,
                         int n, int C, float* out_probs, float* out_weight, hipStream_t s) {
    hipLaunchKernelGGL(sm_pool_kernel, sm_waves(n), dim3(SM_THREADS), 0, s, probs, weights, members, member_ptr, totals, n, C, out_probs, out_weight);
}

static int64_t sm_capacity(int64_t E) {
    int64_t cap = 64;
    while (cap < 2 * E) cap <<= 1;
    return cap;
}

int merge_segments_check_args(int64_t N, int64_t E, int C, int R, int n_scenes) {
    if (N < 0 || E < 0 || n_scenes < 0) return fail(-1, "merge_segments: negative size");
    if (C < 1 || C > 1024 || R < 1 || R > 32) return fail(-1, "merge_segments: 1..1024 object and 1..32 relation classes");
    if (E > (1 << 26) || E * R > 0x7fffffff || N * C > 0x7fffffff) return fail(-1, "merge_segments: too many nodes or edges");
    return 0;
}

// scratch: keys u64 [cap] | slot_min i32 [cap] | parent i32 [N] | cnt i32 [N] | obj_root i32 [N] | slot_of i32 [E] | flag i32 [max(N,E)] |
//          num i32 [max(N,E) + 1]
size_t merge_segments_scratch_bytes(int64_t N, int64_t E, int C, int R, int n_scenes) {
    (void)C; (void)R; (void)n_scenes;
    const size_t n = (size_t)N, e = (size_t)E, cap = (size_t)sm_capacity(E), big = n > e ? n : e;
    return cap * 8 + align_up(cap * 4, 16) + 3 * align_up(n * 4, 16) + align_up(e * 4, 16) + align_up(big * 4, 16) + align_up((big + 1) * 4, 16);
}

int launch_merge_segments(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int64_t* batch_ids, const float* weights,
                          int n_nodes, int n_edges, int C, int R, int n_scenes, int same_part, float threshold, int mutual, void* scratch,
                          int32_t* root, int32_t* object, int32_t* n_objects, int32_t* totals, int32_t* member_ptr, int32_t* members,
                          float* out_probs, float* out_weight, int64_t* obj_batch_ids, int32_t* edge_to_pair, int64_t* pair_edges,
                          int32_t* pair_count, float* pair_probs, hipStream_t s) {
    const int N = n_nodes, E = n_edges;
    const int64_t cap = sm_capacity(E);
    const unsigned mask = (unsigned)(cap - 1);
    const size_t big = (size_t)std::max(N, E);
    char* p = static_cast<char*>(scratch);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(p);  p += (size_t)cap * 8;
    int32_t* slot_min = reinterpret_cast<int32_t*>(p);                    p += align_up((size_t)cap * 4, 16);
    int32_t* parent = reinterpret_cast<int32_t*>(p);                      p += align_up((size_t)N * 4, 16);
    int32_t* cnt = reinterpret_cast<int32_t*>(p);                         p += align_up((size_t)N * 4, 16);
    int32_t* obj_root = reinterpret_cast<int32_t*>(p);                    p += align_up((size_t)N * 4, 16);
    int32_t* slot_of = reinterpret_cast<int32_t*>(p);                     p += align_up((size_t)E * 4, 16);
    int32_t* flag = reinterpret_cast<int32_t*>(p);                        p += align_up(big * 4, 16);
    int32_t* num = reinterpret_cast<int32_t*>(p);

    auto blocks = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + SM_THREADS - 1) / SM_THREADS, 4096))); };
    auto exact = [](int64_t n) { return dim3((unsigned)((n + SM_THREADS - 1) / SM_THREADS)); };
    const dim3 block(SM_THREADS);
    const int64_t most = std::max<int64_t>(std::max<int64_t>((int64_t)N * C, (int64_t)E * R), n_scenes);
    hipLaunchKernelGGL(sm_clear_kernel, blocks(most), block, 0, s, N, E, C, R, n_scenes, parent, cnt, slot_of, root, object, n_objects, totals,
                       members, out_probs, out_weight, obj_batch_ids, edge_to_pair, pair_edges, pair_count, pair_probs);
    if (N == 0) {                                                     // no node: no object, no pair; member_ptr = [0]
        launch_scan_i32(cnt, 0, member_ptr, nullptr, nullptr, s);
        VLSAT_LAUNCH_CHECK("merge_segments");
        return 0;
    }
    if (E > 0) {
        if (mutual) {
            hipLaunchKernelGGL(sm_table_clear_kernel, blocks(cap), block, 0, s, keys, slot_min, cap);
            hipLaunchKernelGGL(sm_link_insert_kernel, exact(E), block, 0, s, rel_probs, edges, batch_ids, N, E, R, same_part, threshold, keys, mask);
            hipLaunchKernelGGL(sm_union_kernel<true>, exact(E), block, 0, s, rel_probs, edges, batch_ids, N, E, R, same_part, threshold,
                               (const unsigned long long*)keys, mask, parent);
        } else {
            hipLaunchKernelGGL(sm_union_kernel<false>, exact(E), block, 0, s, rel_probs, edges, batch_ids, N, E, R, same_part, threshold,
                               (const unsigned long long*)keys, mask, parent);
        }
    }
    hipLaunchKernelGGL(sm_flatten_kernel, exact(N), block, 0, s, (const int32_t*)parent, N, root, flag);
    launch_scan_i32(flag, N, num, totals, nullptr, s);
    hipLaunchKernelGGL(sm_object_kernel, exact(N), block, 0, s, (const int32_t*)root, (const int32_t*)num, batch_ids, N, n_scenes, object, cnt,
                       obj_root, obj_batch_ids, n_objects);
    launch_scan_i32(cnt, N, member_ptr, nullptr, nullptr, s);
    launch_members(root, obj_root, member_ptr, batch_ids, totals, N, members, s);
    launch_pool_members(obj_probs, weights, members, member_ptr, totals, N, C, out_probs, out_weight, s);
    if (E > 0) {
        hipLaunchKernelGGL(sm_table_clear_kernel, blocks(cap), block, 0, s, keys, slot_min, cap);
        hipLaunchKernelGGL(sm_pair_insert_kernel, exact(E), block, 0, s, edges, batch_ids, (const int32_t*)object, N, E, keys, slot_min, mask, slot_of);
        hipLaunchKernelGGL(sm_pair_flag_kernel, exact(E), block, 0, s, (const int32_t*)slot_of, (const int32_t*)slot_min, E, flag);
        launch_scan_i32(flag, E, num, totals + 1, nullptr, s);
        hipLaunchKernelGGL(sm_pair_emit_kernel, exact((int64_t)E * R), block, 0, s, rel_probs, edges, (const int32_t*)object, (const int32_t*)slot_of,
                           (const int32_t*)slot_min, (const int32_t*)num, E, R, edge_to_pair, pair_edges, pair_count,
                           reinterpret_cast<unsigned*>(pair_probs));
    }
    VLSAT_LAUNCH_CHECK("merge_segments");
    return 0;
}

}  // namespace vlsat
