// Proximity-pruned edge lists on the device: the sparse alternative to the fully connected list of prep.hip for large scenes.
//
//   boxes  f32 [N,6] = lo.xyz, hi.xyz   unpadded axis-aligned box of ALL points of an instance (instance_boxes below; the reference
//                                       pads the same box by 0.2 per side, src/dataset/dataset_3dssg.py:286-288)
//   cand(i,j)   i != j, same scene, padded boxes intersect strictly on the three axes:
//                   lo_i[a] - padding < hi_j[a] + padding   and   lo_j[a] - padding < hi_i[a] + padding      (one fp32 op per side)
//               an instance without points has lo = +inf, hi = -inf and is never a candidate
//   d(i,j)      g_a = max(0, max(lo_i[a] - hi_j[a], lo_j[a] - hi_i[a]));  d = (g_x g_x + g_y g_y) + g_z g_z, fp32, round to nearest,
//               no contraction: d(i,j) and d(j,i) are the same bits
//   key_i(j)    (bits(d) << 32) | local index of j         (d >= 0: the order of the bits is the order of the values)
//   keep_i(j)   key_i(j) is among the max_neighbors smallest keys of i's candidates
//   edge (i,j)  cand(i,j) and (no cap  or  keep_i(j)  or  keep_j(i))     -- symmetric; out-degree may exceed max_neighbors
// Order: scenes in node order, source-major, targets ascending = the fully connected order with the dropped pairs removed.
//
// Passes (one wave per source node, lanes stride over the targets of its scene; no global atomics, O(N + E) memory, O(sum n_s^2) work):
//   prox_threshold_kernel   thr[i] = the max_neighbors-th smallest key of row i, by bisection on the key bits (all ones when the row
//                           has fewer candidates) -- skipped without a cap
//   prox_rows_kernel<0>     row_count[i] by ballot + popcount, batch_ids[i]
//   prox_scan_kernel        exclusive scan -> row_off[N+1], edge_ptr[S+1]
//   prox_rows_kernel<1>     the same predicate again; lanes compact with ballot prefixes, so a row's targets come out ascending
// A block stages the boxes of the scenes its rows belong to in LDS (structure of arrays) when they are at most PROX_LDS_BOXES, and
// reads them from global memory otherwise; the arithmetic is the same function in both branches.
#include "common.h"
#include "kernels.h"
#include "select_core.h"
#include "wave_core.h"

namespace vlsat {

constexpr int PROX_LDS_BOXES = 1024;      // boxes a block stages (24 KiB of LDS); larger spans are read from global memory
constexpr int PROX_ROWS = 8;              // source nodes per block (4 waves, 2 rows each)
constexpr int PROX_THREADS = 256;
constexpr unsigned long long PROX_ALL = ~0ull;

int proximity_lds_boxes() { return PROX_LDS_BOXES; }

// ---- per-instance boxes -------------------------------------------------------------------------------------------------------
// min / max are order independent, so integer atomics on the order-preserving key of the float (select_core.h fkey: unsigned order =
// float order, -0 < +0) give the exact result.
__global__ void prox_map_set_kernel(const int32_t* __restrict__ ids, int n_obj, int32_t* __restrict__ id_map, int map_size,
                                    unsigned* __restrict__ codes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_obj) return;
    if (ids[i] >= 0 && ids[i] < map_size) id_map[ids[i]] = i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        codes[(size_t)i * 6 + a] = fkey(INFINITY);
        codes[(size_t)i * 6 + 3 + a] = fkey(-INFINITY);
    }
}
constexpr int BOX_CHUNK = 4096;           // points per block
// TABLE: the block reduces into an LDS table [n_obj][6] first and sends one atomic per touched entry; otherwise (more objects than
// the table holds) every point sends its own.  Both are min / max of the same values.
template <bool TABLE>
__global__ __launch_bounds__(256) void prox_boxes_kernel(const int32_t* __restrict__ inst, const float* __restrict__ pts, int64_t n_points,
                                                         const int32_t* __restrict__ id_map, int map_size, int n_obj,
                                                         unsigned* __restrict__ codes) {
    __shared__ unsigned tab[TABLE ? PROX_LDS_BOXES * 6 : 1];
    const unsigned lo0 = fkey(INFINITY), hi0 = fkey(-INFINITY);
    if (TABLE) {
        for (int t = threadIdx.x; t < n_obj * 6; t += 256) tab[t] = (t % 6) < 3 ? lo0 : hi0;
        __syncthreads();
    }
    const int64_t base = (int64_t)blockIdx.x * BOX_CHUNK;
    for (int c = threadIdx.x; c < BOX_CHUNK; c += 256) {
        const int64_t i = base + c;
        if (i >= n_points) break;
        const int id = inst[i];
        if (id < 0 || id >= map_size) continue;
        const int slot = id_map[id];
        if (slot < 0 || slot >= n_obj) continue;
        unsigned* dst = TABLE ? tab + slot * 6 : codes + (size_t)slot * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned v = fkey(pts[i * 3 + a]);
            atomicMin(dst + a, v);
            atomicMax(dst + 3 + a, v);
        }
    }
    if (TABLE) {
        __syncthreads();
        for (int t = threadIdx.x; t < n_obj * 6; t += 256) {
            const unsigned v = tab[t];
            if ((t % 6) < 3) { if (v != lo0) atomicMin(codes + t, v); }
            else if (v != hi0) atomicMax(codes + t, v);
        }
    }
}
__global__ void prox_boxes_decode_kernel(unsigned* __restrict__ codes, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) codes[i] = __float_as_uint(unkey(codes[i]));
}

int launch_instance_boxes(const int32_t* instances, const float* scene_points, int64_t n_points, const int32_t* ids, int n_obj,
                          int32_t* id_map, int map_size, float* boxes, hipStream_t s) {
    if (n_obj <= 0) return 0;
    if (n_points < 0 || n_points > 0x7fffffff || map_size <= 0) return fail(-1, "instance_boxes: bad sizes");
    unsigned* codes = reinterpret_cast<unsigned*>(boxes);
    launch_id_map_clear(id_map, map_size, s);
    hipLaunchKernelGGL(prox_map_set_kernel, dim3((n_obj + 255) / 256), dim3(256), 0, s, ids, n_obj, id_map, map_size, codes);
    if (n_points > 0) {
        const unsigned blocks = (unsigned)((n_points + BOX_CHUNK - 1) / BOX_CHUNK);
        if (n_obj <= PROX_LDS_BOXES)
            hipLaunchKernelGGL(prox_boxes_kernel<true>, dim3(blocks), dim3(256), 0, s, instances, scene_points, n_points, id_map, map_size,
                               n_obj, codes);
        else
            hipLaunchKernelGGL(prox_boxes_kernel<false>, dim3(blocks), dim3(256), 0, s, instances, scene_points, n_points, id_map, map_size,
                               n_obj, codes);
    }
    const int64_t n = (int64_t)n_obj * 6;
    hipLaunchKernelGGL(prox_boxes_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, codes, n);
    VLSAT_LAUNCH_CHECK("instance_boxes");
    return 0;
}

// ---- the pair rule ------------------------------------------------------------------------------------------------------------
struct Box { float lo[3], hi[3]; };

// STAGED: from the block's LDS copy (structure of arrays, index relative to the staged span); else from global memory
template <bool STAGED>
__device__ __forceinline__ Box load_box(const float* __restrict__ boxes, const float* __restrict__ lds, int base, int j) {
    Box b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = STAGED ? lds[a * PROX_LDS_BOXES + (j - base)] : boxes[(size_t)j * 6 + a];
        b.hi[a] = STAGED ? lds[(3 + a) * PROX_LDS_BOXES + (j - base)] : boxes[(size_t)j * 6 + 3 + a];
    }
    return b;
}

__device__ __forceinline__ bool prox_cand(const Box& p, const Box& q, float padding) {
    bool c = true;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        c = c && (p.lo[a] - padding < q.hi[a] + padding) && (q.lo[a] - padding < p.hi[a] + padding);
    return c;
}

// squared gap between two boxes; every product and sum is rounded on its own (numpy restates d bit for bit).  This toolchain's
// __fmul_rn / __fadd_rn are plain operators, and under the library's -ffp-contract=fast the backend fuses them whatever a pragma
// says, so build.py compiles THIS file with -ffp-contract=off (PER_SOURCE_FLAGS).
__device__ __forceinline__ unsigned prox_dist_bits(const Box& p, const Box& q) {
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = fmaxf(0.0f, fmaxf(__fsub_rn(p.lo[a], q.hi[a]), __fsub_rn(q.lo[a], p.hi[a])));
    const float xx = __fmul_rn(g[0], g[0]), yy = __fmul_rn(g[1], g[1]), zz = __fmul_rn(g[2], g[2]);
    return __float_as_uint(__fadd_rn(__fadd_rn(xx, yy), zz));
}

__device__ __forceinline__ unsigned long long prox_key(unsigned dist_bits, int local) {
    return ((unsigned long long)dist_bits << 32) | (unsigned)local;
}

// largest s in [0, n_scenes) with node_ptr[s] <= i  (the scene of node i; empty scenes own no node)
__device__ __forceinline__ int scene_of(const int32_t* __restrict__ node_ptr, int n_scenes, int i) {
    int lo = 0, hi = n_scenes - 1;
    while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (node_ptr[m] <= i) lo = m; else hi = m - 1; }
    return lo;
}

// The span of nodes a block needs (the scenes of its first and last row) and, when it fits, its copy in LDS.  Returns whether staged.
__device__ __forceinline__ bool prox_stage(const float* __restrict__ boxes, const int32_t* __restrict__ node_ptr, int n_scenes, int n_nodes,
                                           int row0, float* lds, int& base) {
    const int row1 = min(row0 + PROX_ROWS, n_nodes) - 1;
    const int s0 = scene_of(node_ptr, n_scenes, row0), s1 = scene_of(node_ptr, n_scenes, row1);
    base = max(node_ptr[s0], 0);
    const int end = min(node_ptr[s1 + 1], n_nodes);
    if (end - base > PROX_LDS_BOXES) return false;
    for (int t = threadIdx.x; t < end - base; t += PROX_THREADS) {
#pragma unroll
        for (int a = 0; a < 6; ++a) lds[a * PROX_LDS_BOXES + t] = boxes[(size_t)(base + t) * 6 + a];
    }
    __syncthreads();
    return true;
}

// ---- threshold: the K-th smallest key of every row ---------------------------------------------------------------------------------
template <bool STAGED>
__device__ __forceinline__ void prox_threshold_row(const float* __restrict__ boxes, const float* __restrict__ lds, int base, int i, int a0, int a1,
                                                   float padding, int K, unsigned long long* __restrict__ thr) {
    const int lane = threadIdx.x & 63;
    const Box bi = load_box<STAGED>(boxes, lds, base, i);
    // bits of a key that can be set: 31 of the distance (d >= 0), and the bits of the largest local index
    const int idx_bits = 32 - __builtin_clz((unsigned)max(a1 - a0 - 1, 1));
    auto count_le = [&](unsigned long long t) {
        int n = 0;
        for (int j0 = a0; j0 < a1; j0 += 64) {
            const int j = j0 + lane;
            bool in = false;
            if (j < a1 && j != i) {
                const Box bj = load_box<STAGED>(boxes, lds, base, j);
                in = prox_cand(bi, bj, padding) && prox_key(prox_dist_bits(bi, bj), j - a0) <= t;
            }
            n += (int)__popcll(__ballot(in));
        }
        return n;
    };
    unsigned long long t = PROX_ALL;
    if (count_le(PROX_ALL) >= K) {                       // smallest t with #{key <= t} >= K, built from the top bit down
        t = 0;
        for (int b = 62; b >= 0; --b) {
            if (b < 32 && b >= idx_bits) continue;       // (no key has these bits set)
            const unsigned long long below = t | ((1ull << b) - 1);
            if (count_le(below) < K) t |= 1ull << b;
        }
    }
    if (lane == 0) thr[i] = t;
}

__global__ __launch_bounds__(PROX_THREADS) void prox_threshold_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ node_ptr,
                                                                      int n_scenes, int n_nodes, float padding, int K,
                                                                      unsigned long long* __restrict__ thr) {
    __shared__ float lds[6 * PROX_LDS_BOXES];
    const int row0 = blockIdx.x * PROX_ROWS, wave = threadIdx.x >> 6;
    int base;
    const bool staged = prox_stage(boxes, node_ptr, n_scenes, n_nodes, row0, lds, base);
    for (int r = wave; r < PROX_ROWS; r += PROX_THREADS / 64) {
        const int i = row0 + r;
        if (i >= n_nodes) break;
        const int s = scene_of(node_ptr, n_scenes, i);
        const int a0 = max(node_ptr[s], 0), a1 = min(node_ptr[s + 1], n_nodes);
        if (staged) prox_threshold_row<true>(boxes, lds, base, i, a0, a1, padding, K, thr);
        else prox_threshold_row<false>(boxes, lds, base, i, a0, a1, padding, K, thr);
    }
}

// ---- count (FILL = 0) and fill (FILL = 1) ------------------------------------------------------------------------------------------
template <bool STAGED, bool FILL>
__device__ __forceinline__ void prox_row(const float* __restrict__ boxes, const float* __restrict__ lds, int base, int i, int a0, int a1,
                                         float padding, const unsigned long long* __restrict__ thr, int32_t* __restrict__ row_count,
                                         const int64_t* __restrict__ row_off, int64_t capacity, int64_t* __restrict__ edges) {
    const int lane = threadIdx.x & 63;
    const Box bi = load_box<STAGED>(boxes, lds, base, i);
    const unsigned long long thr_i = thr ? thr[i] : PROX_ALL;
    int64_t pos = FILL ? row_off[i] : 0;
    int n = 0;
    for (int j0 = a0; j0 < a1; j0 += 64) {
        const int j = j0 + lane;
        bool emit = false;
        if (j < a1 && j != i) {
            const Box bj = load_box<STAGED>(boxes, lds, base, j);
            emit = prox_cand(bi, bj, padding);
            if (emit && thr) {
                const unsigned d = prox_dist_bits(bi, bj);
                emit = prox_key(d, j - a0) <= thr_i || prox_key(d, i - a0) <= thr[j];
            }
        }
        const unsigned long long m = __ballot(emit);
        if (FILL) {
            const int64_t p = pos + (int64_t)__popcll(m & ((1ull << lane) - 1));
            if (emit && p < capacity) {                  // (the host checked count <= capacity; this keeps a wrong count in bounds)
                edges[p] = i;
                edges[capacity + p] = j;
            }
            pos += (int64_t)__popcll(m);
        } else {
            n += (int)__popcll(m);
        }
    }
    if (!FILL && lane == 0) row_count[i] = n;
}

template <bool FILL>
__global__ __launch_bounds__(PROX_THREADS) void prox_rows_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ node_ptr, int n_scenes,
                                                                 int n_nodes, float padding, const unsigned long long* __restrict__ thr,
                                                                 int32_t* __restrict__ row_count, const int64_t* __restrict__ row_off,
                                                                 int64_t capacity, int64_t* __restrict__ edges, int64_t* __restrict__ batch_ids) {
    __shared__ float lds[6 * PROX_LDS_BOXES];
    const int row0 = blockIdx.x * PROX_ROWS, wave = threadIdx.x >> 6;
    int base;
    const bool staged = prox_stage(boxes, node_ptr, n_scenes, n_nodes, row0, lds, base);
    for (int r = wave; r < PROX_ROWS; r += PROX_THREADS / 64) {
        const int i = row0 + r;
        if (i >= n_nodes) break;
        const int s = scene_of(node_ptr, n_scenes, i);
        const int a0 = max(node_ptr[s], 0), a1 = min(node_ptr[s + 1], n_nodes);
        if (!FILL && (threadIdx.x & 63) == 0) batch_ids[i] = s;
        if (staged) prox_row<true, FILL>(boxes, lds, base, i, a0, a1, padding, thr, row_count, row_off, capacity, edges);
        else prox_row<false, FILL>(boxes, lds, base, i, a0, a1, padding, thr, row_count, row_off, capacity, edges);
    }
}

// row_off[0..N] = exclusive scan of row_count, edge_ptr[s] = row_off[node_ptr[s]].  One block; a thread owns a contiguous run.
__global__ __launch_bounds__(256) void prox_scan_kernel(const int32_t* __restrict__ row_count, int n_nodes, const int32_t* __restrict__ node_ptr,
                                                        int n_scenes, int64_t* __restrict__ row_off, int64_t* __restrict__ edge_ptr) {
    __shared__ int64_t s_wave[256 / 64];
    const int tid = threadIdx.x;
    const RunScan<int64_t> r = block_run_scan<256>(row_count, n_nodes, s_wave);
    int64_t acc = r.before;
    for (int i = r.b; i < r.e; ++i) { row_off[i] = acc; acc += row_count[i]; }
    if (tid == 0) row_off[n_nodes] = r.total;
    __syncthreads();                                     // (row_off of this block's writes is read below)
    for (int s = tid; s <= n_scenes; s += 256) edge_ptr[s] = row_off[min(max(node_ptr[s], 0), n_nodes)];
}

// scratch: thr u64 [N] | row_off i64 [N+1] | row_count i32 [N]
size_t proximity_scratch_bytes(int64_t n_nodes) {
    const size_t n = (size_t)(n_nodes > 0 ? n_nodes : 0);
    return n * 8 + (n + 1) * 8 + n * 4;
}
static unsigned long long* prox_thr(void* scratch) { return static_cast<unsigned long long*>(scratch); }
static int64_t* prox_row_off(void* scratch, int64_t n) { return static_cast<int64_t*>(scratch) + n; }
static int32_t* prox_row_count(void* scratch, int64_t n) { return reinterpret_cast<int32_t*>(static_cast<int64_t*>(scratch) + 2 * n + 1); }

int launch_proximity_count(const float* boxes, const int32_t* node_ptr, int n_scenes, int64_t n_nodes, float padding, int max_neighbors,
                           void* scratch, int64_t* edge_ptr, int64_t* batch_ids, hipStream_t s) {
    if (n_scenes <= 0 || n_nodes < 0 || n_nodes > 0x7fffffff) return fail(-1, "proximity_count: bad sizes");
    if (!(padding >= 0.0f)) return fail(-1, "proximity_count: padding must be >= 0");
    const int N = (int)n_nodes;
    if (N == 0) {
        VLSAT_HIP_CHECK(hipMemsetAsync(edge_ptr, 0, (size_t)(n_scenes + 1) * sizeof(int64_t), s));
        return 0;
    }
    const bool cap = max_neighbors > 0;
    const dim3 grid((N + PROX_ROWS - 1) / PROX_ROWS), block(PROX_THREADS);
    if (cap) hipLaunchKernelGGL(prox_threshold_kernel, grid, block, 0, s, boxes, node_ptr, n_scenes, N, padding, max_neighbors, prox_thr(scratch));
    hipLaunchKernelGGL(prox_rows_kernel<false>, grid, block, 0, s, boxes, node_ptr, n_scenes, N, padding,
                       cap ? prox_thr(scratch) : (const unsigned long long*)nullptr, prox_row_count(scratch, N),
                       (const int64_t*)nullptr, (int64_t)0, (int64_t*)nullptr, batch_ids);
    hipLaunchKernelGGL(prox_scan_kernel, dim3(1), dim3(256), 0, s, prox_row_count(scratch, N), N, node_ptr, n_scenes, prox_row_off(scratch, N),
                       edge_ptr);
    VLSAT_LAUNCH_CHECK("proximity_count");
    return 0;
}

int launch_proximity_fill(const float* boxes, const int32_t* node_ptr, int n_scenes, int64_t n_nodes, float padding, int max_neighbors,
                          const void* scratch, int64_t n_edges, int64_t capacity, int64_t* edges, hipStream_t s) {
    if (n_scenes <= 0 || n_nodes < 0 || n_nodes > 0x7fffffff || n_edges < 0 || capacity < 0) return fail(-1, "proximity_fill: bad sizes");
    if (n_edges > capacity)
        return fail(-1, "proximity_fill: " + std::to_string(n_edges) + " edges counted, capacity " + std::to_string(capacity));
    const int N = (int)n_nodes;
    if (N == 0 || n_edges == 0) return 0;
    void* sc = const_cast<void*>(scratch);
    const dim3 grid((N + PROX_ROWS - 1) / PROX_ROWS), block(PROX_THREADS);
    hipLaunchKernelGGL(prox_rows_kernel<true>, grid, block, 0, s, boxes, node_ptr, n_scenes, N, padding,
                       max_neighbors > 0 ? prox_thr(sc) : (const unsigned long long*)nullptr, (int32_t*)nullptr, prox_row_off(sc, N), capacity,
                       edges, (int64_t*)nullptr);
    VLSAT_LAUNCH_CHECK("proximity_fill");
    return 0;
}

}  // namespace vlsat
