// A scan split into sub-scenes, and the per-split predictions fused back into one graph per scan.  The three rules are stated in
// include/vlsat_split.h (vlsat_split_seeds, vlsat_split_groups, vlsat_fuse_splits); prep.split_seeds_host / prep.split_groups_host /
// metrics.fuse_splits_host restate them in numpy with the same operations.  The C entry points are at the end of this file.
//
// Seeds (reference data_processing/gen_data.py:69-85).  One init launch, then per seed two launches:
//   ss_update_kernel     dmin2[v] = min(dmin2[v], dx*dx + dy*dy) to the newest seed in fp64; per 1024-vertex block the number of selectable
//                        vertices (dmin2 > distance^2), a plain store
//   ss_pick_kernel       one block: scans the block counts (wave_core.h: a run of them per thread), takes the rank (the counter-based
//                        draw, or ranks[k]), finds the block that holds it and the vertex inside that block (a block scan of the
//                        selectable flags: ascending vertex order), appends the seed
// The number of seeds is data dependent; the caller passes a cap and that many iterations are enqueued.  Once no vertex is selectable
// the pick kernel raises a done flag in device memory and every later launch returns at its first instruction: no read-back per seed, no
// cooperative launch, no barrier or spin-wait between blocks -- the launch boundary is the only cross-block ordering.
//
// Groups (:109-122).  sg_hit_kernel keeps the seeds' boxes in LDS (tiles of SG_TILE), tests every vertex against every box in fp64 and
// sets bit (group, segment slot) by atomicOr (after a relaxed load: most bits are set already); sg_count_kernel counts a group's bits.
//
// Fusion.  Rows of several splits that carry the same instance id are one object; objects are numbered by ascending id through an
// id -> slot table (presence flags, exclusive scan); scan, members and pooled probabilities BY the kernels of segment_merge.hip
// (launch_scan_i32, launch_members, launch_pool_members: one wave per object, rows ascending, fl(s + fl(w p)), fl(s / W)); an edge
// sets bit (a, b) of an [N, ceil(N / 32)] table, the pairs of a source object are counted by popcount, scanned, and an edge's pair
// number is base[a] + the set bits below b: pairs come out sorted by (a, b) with no sort; pair probabilities by atomicMax on the float bits (values >= 0).
// Nothing depends on the order blocks run in.  Integer atomics only.  build.py compiles THIS file with -ffp-contract=off
// (PER_SOURCE_FLAGS): the squared distance and the pooled sum round every product and sum on their own.
#include <algorithm>

#include "../../include/vlsat_split.h"
#include "common.h"
#include "kernels.h"
#include "wave_core.h"

namespace vlsat {

constexpr int SS_THREADS = 256;
constexpr int SS_CHUNK = 1024;                          // vertices per block of the update kernel = threads of the pick kernel
constexpr int SS_PICK_THREADS = 1024;
constexpr int SG_TILE = 512;                            // seed boxes in LDS at a time: 512 * 6 doubles = 24 KB
constexpr int FS_THREADS = 256;
constexpr int FS_NONE = 0x7fffffff;
// state words of vlsat_split_seeds
enum { SS_COUNT = 0, SS_STATUS = 1, SS_DONE = 2, SS_CUR = 3 };

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// splitmix64 of (seed, k), the top 32 bits scaled to n: the generator of vlsat_sample_objects (prep.hip)
__device__ __forceinline__ unsigned ss_draw(unsigned long long seed, unsigned long long k, unsigned n) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (k + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(((z >> 32) * (unsigned long long)n) >> 32);
}

__global__ void ss_init_kernel(int64_t n_points, unsigned long long seed, const int64_t* __restrict__ ranks, int64_t n_ranks, int max_seeds,
                               int32_t* __restrict__ seeds, int32_t* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int status = 0;
    int64_t first = 0;
    if (ranks) {
        if (n_ranks < 1) status = 2;
        else {
            first = ranks[0];
            if (first < 0 || first >= n_points) status = 1;
        }
    } else {
        first = ss_draw(seed, 0, (unsigned)n_points);
    }
    if (!status && max_seeds < 1) status = 3;
    state[SS_STATUS] = status;
    state[SS_DONE] = status != 0;
    state[SS_COUNT] = status ? 0 : 1;
    state[SS_CUR] = status ? 0 : (int)first;
    if (!status) seeds[0] = (int)first;
}

__global__ __launch_bounds__(SS_THREADS) void ss_update_kernel(const float* __restrict__ points, int64_t n_points, double d2_max, int first,
                                                               const int32_t* __restrict__ state, double* __restrict__ dmin2,
                                                               int32_t* __restrict__ block_cnt) {
    __shared__ int wave_cnt[SS_THREADS / 64];
    if (state[SS_DONE]) return;                                       // (uniform: written by an earlier launch)
    const int cur = state[SS_CUR];
    const double sx = (double)points[(size_t)cur * 3], sy = (double)points[(size_t)cur * 3 + 1];
    const int64_t base = (int64_t)blockIdx.x * SS_CHUNK;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < SS_CHUNK / SS_THREADS; ++j) {
        const int64_t v = base + j * SS_THREADS + threadIdx.x;
        bool sel = false;
        if (v < n_points) {
            const float x = points[v * 3], y = points[v * 3 + 1], z = points[v * 3 + 2];
            const double dx = (double)x - sx, dy = (double)y - sy;
            const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
            double m;
            if (first) m = finite3(x, y, z) ? d : __longlong_as_double(0x7ff8000000000000ll);     // NaN: never selectable
            else { m = dmin2[v]; m = d < m ? d : m; }                 // (NaN stays NaN: the comparison is false)
            dmin2[v] = m;
            sel = m > d2_max;
        }
        mine += (int)__popcll(__ballot(sel));                         // (every lane of the wave holds the wave's count)
    }
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < SS_THREADS / 64; ++w) s += wave_cnt[w];
        block_cnt[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(SS_PICK_THREADS) void ss_pick_kernel(const double* __restrict__ dmin2, int64_t n_points, double d2_max,
                                                                  const int32_t* __restrict__ block_cnt, int n_blocks, int draw_index,
                                                                  unsigned long long seed, const int64_t* __restrict__ ranks, int64_t n_ranks,
                                                                  int max_seeds, int32_t* __restrict__ seeds, int32_t* __restrict__ state) {
    __shared__ long long s_wave[SS_PICK_THREADS / 64];
    __shared__ int wave_cnt[SS_PICK_THREADS / 64];
    __shared__ long long s_rank;
    __shared__ int s_block, s_in_block, s_stop;
    if (state[SS_DONE]) return;
    const int tid = threadIdx.x;
    const RunScan<long long> r = block_run_scan<SS_PICK_THREADS>(block_cnt, n_blocks, s_wave);   // a run of blocks per thread
    if (tid == 0) {
        const long long n = r.total;
        int stop = 0, status = 0;
        long long rank = 0;
        if (n == 0) stop = 1;                                         // no vertex is selectable: the seeds are complete
        else if (state[SS_COUNT] >= max_seeds) { stop = 1; status = 3; }
        else if (ranks) {
            if (draw_index >= n_ranks) { stop = 1; status = 2; }
            else {
                rank = ranks[draw_index];
                if (rank < 0 || rank >= n) { stop = 1; status = 1; }
            }
        } else {
            rank = ss_draw(seed, (unsigned long long)draw_index, (unsigned)n);
        }
        s_rank = rank;
        s_stop = stop;
        s_block = -1;
        if (stop) { state[SS_DONE] = 1; state[SS_STATUS] = status; }
    }
    __syncthreads();
    if (s_stop) return;
    const long long rank = s_rank;
    if (rank >= r.before && rank < r.before + r.sum) {                // the rank lies in this thread's run of blocks
        long long acc = r.before;
        for (int b = r.b; b < r.e; ++b) {
            const int c = block_cnt[b];
            if (rank < acc + c) { s_block = b; s_in_block = (int)(rank - acc); break; }
            acc += c;
        }
    }
    __syncthreads();
    const int blk = s_block;
    if (blk < 0) return;                                              // (cannot happen: 0 <= rank < the total)
    const int64_t v = (int64_t)blk * SS_CHUNK + tid;
    const bool sel = v < n_points && dmin2[v] > d2_max;
    int n_sel;
    const int before = block_scan_excl<SS_PICK_THREADS>((int)sel, wave_cnt, n_sel);       // selectable vertices of the block before v
    if (sel && before == s_in_block) {
        const int k = state[SS_COUNT];
        seeds[k] = (int)v;
        state[SS_CUR] = (int)v;
        state[SS_COUNT] = k + 1;
    }
}

// ---- groups -------------------------------------------------------------------------------------------------------------------------
__global__ void sg_clear_kernel(int32_t* __restrict__ id_map, int map_size, unsigned* __restrict__ mask, int64_t n_words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < map_size; i += stride) id_map[i] = -1;
    for (int64_t i = t0; i < n_words; i += stride) mask[i] = 0u;
}

__global__ __launch_bounds__(256) void sg_hit_kernel(const float* __restrict__ points, const int32_t* __restrict__ segments, int64_t n_points,
                                                     const int32_t* __restrict__ id_map, int map_size, const int32_t* __restrict__ seeds,
                                                     int n_seeds, double bbox, int words, unsigned* __restrict__ mask) {
    __shared__ double box[SG_TILE * 6];                               // lo.xyz, hi.xyz of the tile's seeds
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int k0 = 0; k0 < n_seeds; k0 += SG_TILE) {
        const int kn = min(SG_TILE, n_seeds - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < kn * 3; i += 256) {
            const int k = i / 3, a = i - k * 3;
            const int sv = seeds[k0 + k];
            const bool ok = sv >= 0 && sv < n_points;
            const double p = ok ? (double)points[(size_t)sv * 3 + a] : __longlong_as_double(0x7ff8000000000000ll);
            box[k * 6 + a] = __dsub_rn(p, bbox);
            box[k * 6 + 3 + a] = __dadd_rn(p, bbox);
        }
        __syncthreads();
        for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_points; v += stride) {
            const int id = segments[v];
            const int slot = (id >= 0 && id < map_size) ? id_map[id] : -1;
            if (slot < 0) continue;
            const double x = (double)points[v * 3], y = (double)points[v * 3 + 1], z = (double)points[v * 3 + 2];
            const unsigned bit = 1u << (slot & 31);
            for (int k = 0; k < kn; ++k) {
                const double* b = box + k * 6;
                if (x > b[0] && x < b[3] && y > b[1] && y < b[4] && z > b[2] && z < b[5]) {
                    unsigned* w = mask + (size_t)(k0 + k) * words + (slot >> 5);
                    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void sg_count_kernel(const unsigned* __restrict__ mask, int n_seeds, int words, int min_seg,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ keep) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n_seeds) return;
    int c = 0;
    for (int w = lane; w < words; w += 64) c += __popc(mask[(size_t)k * words + w]);
    c = wave_sum_i(c);
    if (lane == 0) { counts[k] = c; keep[k] = c >= min_seg; }
}

// ---- fusion -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FS_THREADS) void fs_clear_kernel(int n, int e, int C, int R, int map_size, int64_t bit_words, int32_t* __restrict__ first,
                                                              int32_t* __restrict__ rows, int32_t* __restrict__ cnt, unsigned* __restrict__ bits,
                                                              int32_t* __restrict__ root, int32_t* __restrict__ object, int32_t* __restrict__ n_objects,
                                                              int32_t* __restrict__ totals, int32_t* __restrict__ members,
                                                              float* __restrict__ out_probs, float* __restrict__ out_weight,
                                                              int64_t* __restrict__ obj_bid, int32_t* __restrict__ obj_ids,
                                                              int32_t* __restrict__ edge_to_pair, int64_t* __restrict__ pair_edges,
                                                              int32_t* __restrict__ pair_count, float* __restrict__ pair_probs) {
    const int64_t stride = (int64_t)gridDim.x * FS_THREADS, t0 = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
    for (int64_t i = t0; i < map_size; i += stride) { first[i] = FS_NONE; rows[i] = 0; }
    for (int64_t i = t0; i < bit_words; i += stride) bits[i] = 0u;
    for (int64_t i = t0; i < n; i += stride) {
        cnt[i] = 0; root[i] = -1; object[i] = -1; members[i] = -1; out_weight[i] = 0.0f; obj_bid[i] = -1; obj_ids[i] = -1;
    }
    for (int64_t i = t0; i < (int64_t)n * C; i += stride) out_probs[i] = 0.0f;
    for (int64_t i = t0; i < e; i += stride) { edge_to_pair[i] = -1; pair_edges[i * 2] = -1; pair_edges[i * 2 + 1] = -1; pair_count[i] = 0; }
    for (int64_t i = t0; i < (int64_t)e * R; i += stride) pair_probs[i] = 0.0f;
    if (t0 < 2) totals[t0] = 0;
    if (t0 == 0) n_objects[0] = 0;
}

__global__ __launch_bounds__(FS_THREADS) void fs_first_kernel(const int32_t* __restrict__ row_instance, int n, int map_size,
                                                              int32_t* __restrict__ first, int32_t* __restrict__ rows) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int id = row_instance[i];
    if (id < 0 || id >= map_size) return;
    atomicMin(first + id, i);
    atomicAdd(rows + id, 1);
}

__global__ __launch_bounds__(FS_THREADS) void fs_flag_kernel(const int32_t* __restrict__ first, int map_size, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (i < map_size) flag[i] = first[i] != FS_NONE;
}

__global__ __launch_bounds__(FS_THREADS) void fs_object_kernel(const int32_t* __restrict__ row_instance, int n, int map_size,
                                                               const int32_t* __restrict__ first, const int32_t* __restrict__ rows,
                                                               const int32_t* __restrict__ num, int32_t* __restrict__ root,
                                                               int32_t* __restrict__ object, int32_t* __restrict__ cnt,
                                                               int32_t* __restrict__ obj_root, int64_t* __restrict__ obj_bid,
                                                               int32_t* __restrict__ obj_ids) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int id = row_instance[i];
    if (id < 0 || id >= map_size) return;
    const int o = num[id], r = first[id];
    if (o < 0 || o >= n || r < 0 || r >= n) return;
    root[i] = r;
    object[i] = o;
    if (r == i) { cnt[o] = rows[id]; obj_root[o] = i; obj_bid[o] = 0; obj_ids[o] = id; }
}

struct FsPair { int a, b; bool ok; };                   // ok: both rows in range, both with an object, two different objects
__device__ __forceinline__ FsPair fs_pair(const int64_t* __restrict__ edges, const int32_t* __restrict__ object, int n, int64_t e) {
    const int64_t ra = edges[e * 2], rb = edges[e * 2 + 1];
    FsPair p;
    p.ok = ra >= 0 && rb >= 0 && ra < n && rb < n;
    p.a = p.ok ? object[ra] : -1;
    p.b = p.ok ? object[rb] : -1;
    p.ok = p.ok && p.a >= 0 && p.b >= 0 && p.a < n && p.b < n && p.a != p.b;
    return p;
}

__global__ __launch_bounds__(FS_THREADS) void fs_pair_mark_kernel(const int64_t* __restrict__ edges, const int32_t* __restrict__ object, int n, int n_edges,
                                                                  int words, unsigned* __restrict__ bits) {
    const int64_t e = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const FsPair p = fs_pair(edges, object, n, e);
    if (!p.ok) return;
    unsigned* w = bits + (size_t)p.a * words + (p.b >> 5);
    const unsigned bit = 1u << (p.b & 31);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
}

// one wave per source object: its number of distinct targets (objects past M have none)
__global__ __launch_bounds__(FS_THREADS) void fs_row_count_kernel(const unsigned* __restrict__ bits, int n, int words, int32_t* __restrict__ row_cnt) {
    const int a = blockIdx.x * (FS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n) return;
    int c = 0;
    for (int w = lane; w < words; w += 64) c += __popc(bits[(size_t)a * words + w]);
    c = wave_sum_i(c);
    if (lane == 0) row_cnt[a] = c;
}

__global__ __launch_bounds__(FS_THREADS) void fs_pair_index_kernel(const int64_t* __restrict__ edges, const int32_t* __restrict__ object,
                                                                   const unsigned* __restrict__ bits, const int32_t* __restrict__ base, int n,
                                                                   int n_edges, int words, int32_t* __restrict__ edge_to_pair,
                                                                   int64_t* __restrict__ pair_edges, int32_t* __restrict__ pair_count) {
    const int64_t e = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const FsPair p = fs_pair(edges, object, n, e);
    if (!p.ok) return;
    const unsigned* row = bits + (size_t)p.a * words;
    int below = 0;
    for (int w = 0; w < (p.b >> 5); ++w) below += __popc(row[w]);
    below += __popc(row[p.b >> 5] & ((1u << (p.b & 31)) - 1u));
    const int q = base[p.a] + below;
    if (q < 0 || q >= n_edges) return;                                // (cannot happen: distinct pairs <= edges)
    edge_to_pair[e] = q;
    atomicAdd(pair_count + q, 1);
    pair_edges[(size_t)q * 2] = p.a;                                  // (every edge of the pair writes the same two values)
    pair_edges[(size_t)q * 2 + 1] = p.b;
}

__global__ __launch_bounds__(FS_THREADS) void fs_pair_emit_kernel(const float* __restrict__ rel_probs, const int32_t* __restrict__ edge_to_pair,
                                                                  int n_edges, int R, unsigned* __restrict__ pair_probs) {
    const int64_t t = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
    if (t >= (int64_t)n_edges * R) return;
    const int64_t e = t / R;
    const int q = edge_to_pair[e];
    if (q < 0 || q >= n_edges) return;
    atomicMax(pair_probs + (size_t)q * R + (t - e * R), __float_as_uint(rel_probs[t]));       // values >= 0: the bit order is the value order
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static dim3 ss_blocks(int64_t n, int threads) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + threads - 1) / threads, 4096))); }

// scratch of the seeds: dmin2 f64 [V] | block_cnt i32 [ceil(V / 1024)]
static size_t split_seeds_scratch_bytes(int64_t V) {
    if (V < 1 || V > 0x7fffffff) return 0;
    return align_up((size_t)V * 8, 16) + align_up((size_t)((V + SS_CHUNK - 1) / SS_CHUNK) * 4, 16);
}

static int launch_split_seeds(const float* points, int64_t V, double distance, unsigned long long seed, const int64_t* ranks, int64_t n_ranks,
                              int max_seeds, void* scratch, int32_t* seeds, int32_t* state, hipStream_t s) {
    const int n_blocks = (int)((V + SS_CHUNK - 1) / SS_CHUNK);
    double* dmin2 = static_cast<double*>(scratch);
    int32_t* block_cnt = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + align_up((size_t)V * 8, 16));
    const double d2 = distance * distance;
    hipLaunchKernelGGL(ss_init_kernel, dim3(1), dim3(64), 0, s, V, seed, ranks, n_ranks, max_seeds, seeds, state);
    for (int k = 0; k < max_seeds; ++k) {
        hipLaunchKernelGGL(ss_update_kernel, dim3(n_blocks), dim3(SS_THREADS), 0, s, points, V, d2, k == 0, (const int32_t*)state, dmin2, block_cnt);
        hipLaunchKernelGGL(ss_pick_kernel, dim3(1), dim3(SS_PICK_THREADS), 0, s, (const double*)dmin2, V, d2, (const int32_t*)block_cnt, n_blocks,
                           k + 1, seed, ranks, n_ranks, max_seeds, seeds, state);
    }
    VLSAT_LAUNCH_CHECK("split_seeds");
    return 0;
}

static int launch_split_groups(const float* points, const int32_t* segments, int64_t V, const int32_t* segment_ids, int n_seg, int32_t* id_map,
                               int map_size, const int32_t* seeds, int n_seeds, double bbox, int min_seg, uint32_t* mask, int32_t* counts,
                               int32_t* keep, hipStream_t s) {
    const int words = (n_seg + 31) / 32;
    const int64_t n_words = (int64_t)n_seeds * words;
    hipLaunchKernelGGL(sg_clear_kernel, ss_blocks(std::max<int64_t>(map_size, n_words), 256), dim3(256), 0, s, id_map, map_size, mask, n_words);
    if (n_seg > 0) launch_id_map_set(segment_ids, n_seg, id_map, map_size, s);
    if (n_seeds > 0 && n_seg > 0 && V > 0)
        hipLaunchKernelGGL(sg_hit_kernel, ss_blocks(V, 256), dim3(256), 0, s, points, segments, V, (const int32_t*)id_map, map_size, seeds, n_seeds, bbox,
                           words, mask);
    if (n_seeds > 0)
        hipLaunchKernelGGL(sg_count_kernel, dim3((n_seeds + 3) / 4), dim3(256), 0, s, (const unsigned*)mask, n_seeds, words, min_seg, counts, keep);
    VLSAT_LAUNCH_CHECK("split_groups");
    return 0;
}

static int fuse_splits_check_args(int64_t N, int64_t E, int C, int R, int map_size) {
    if (N < 0 || E < 0) return fail(VLSAT_EINVAL, "fuse_splits: negative size");
    if (C < 1 || C > 1024 || R < 1 || R > 32) return fail(VLSAT_EINVAL, "fuse_splits: 1..1024 object and 1..32 relation classes");
    if (map_size < 1 || map_size > (1 << 24)) return fail(VLSAT_EINVAL, "fuse_splits: map_size must be in 1..2^24");
    if (N > 16384) return fail(VLSAT_EINVAL, "fuse_splits: at most 16384 rows per call (the pair table is N * N bits)");
    if (E > (1 << 26) || E * R > 0x7fffffff || N * C > 0x7fffffff) return fail(VLSAT_EINVAL, "fuse_splits: too many rows or edges");
    return 0;
}

// scratch: first i32 [map] | rows i32 [map] | flag i32 [max(map, N)] | num i32 [max(map, N) + 1] | cnt i32 [N] | obj_root i32 [N] |
//          base i32 [N + 1] | bits u32 [N * ceil(N / 32)]
static size_t fuse_splits_scratch_bytes(int64_t N, int64_t E, int map_size) {
    (void)E;
    const size_t n = (size_t)N, m = (size_t)map_size, big = n > m ? n : m, words = (n + 31) / 32;
    return 2 * align_up(m * 4, 16) + align_up(big * 4, 16) + align_up((big + 1) * 4, 16) + 2 * align_up(n * 4, 16) + align_up((n + 1) * 4, 16) +
           align_up(n * words * 4, 16);
}

static int launch_fuse_splits(const float* probs, const float* rel_probs, const int64_t* edges, const int32_t* row_instance, const float* weights,
                              int N, int E, int C, int R, int map_size, void* scratch, int32_t* root, int32_t* object, int32_t* n_objects,
                              int32_t* totals, int32_t* member_ptr, int32_t* members, float* out_probs, float* out_weight, int64_t* obj_bid,
                              int32_t* edge_to_pair, int64_t* pair_edges, int32_t* pair_count, float* pair_probs, int32_t* obj_ids, hipStream_t s) {
    const size_t n = (size_t)N, m = (size_t)map_size, big = n > m ? n : m;
    const int words = (N + 31) / 32;
    const int64_t bit_words = (int64_t)N * words;
    char* p = static_cast<char*>(scratch);
    int32_t* first = reinterpret_cast<int32_t*>(p);     p += align_up(m * 4, 16);
    int32_t* rows = reinterpret_cast<int32_t*>(p);      p += align_up(m * 4, 16);
    int32_t* flag = reinterpret_cast<int32_t*>(p);      p += align_up(big * 4, 16);
    int32_t* num = reinterpret_cast<int32_t*>(p);       p += align_up((big + 1) * 4, 16);
    int32_t* cnt = reinterpret_cast<int32_t*>(p);       p += align_up(n * 4, 16);
    int32_t* obj_root = reinterpret_cast<int32_t*>(p);  p += align_up(n * 4, 16);
    int32_t* base = reinterpret_cast<int32_t*>(p);      p += align_up((n + 1) * 4, 16);
    unsigned* bits = reinterpret_cast<unsigned*>(p);

    auto exact = [](int64_t k) { return dim3((unsigned)((k + FS_THREADS - 1) / FS_THREADS)); };
    const dim3 block(FS_THREADS);
    const int64_t most = std::max<int64_t>(std::max<int64_t>((int64_t)N * C, (int64_t)E * R), std::max<int64_t>(map_size, bit_words));
    hipLaunchKernelGGL(fs_clear_kernel, ss_blocks(most, FS_THREADS), block, 0, s, N, E, C, R, map_size, bit_words, first, rows, cnt, bits, root, object,
                       n_objects, totals, members, out_probs, out_weight, obj_bid, obj_ids, edge_to_pair, pair_edges, pair_count, pair_probs);
    if (N == 0) {                                                     // no row: no object, no pair; member_ptr = [0]
        launch_scan_i32(cnt, 0, member_ptr, nullptr, nullptr, s);
        VLSAT_LAUNCH_CHECK("fuse_splits");
        return 0;
    }
    hipLaunchKernelGGL(fs_first_kernel, exact(N), block, 0, s, row_instance, N, map_size, first, rows);
    hipLaunchKernelGGL(fs_flag_kernel, exact(map_size), block, 0, s, (const int32_t*)first, map_size, flag);
    launch_scan_i32(flag, map_size, num, totals, n_objects, s);
    hipLaunchKernelGGL(fs_object_kernel, exact(N), block, 0, s, row_instance, N, map_size, (const int32_t*)first, (const int32_t*)rows,
                       (const int32_t*)num, root, object, cnt, obj_root, obj_bid, obj_ids);
    launch_scan_i32(cnt, N, member_ptr, nullptr, nullptr, s);
    // members: root[i] == obj_root[o] exactly when object[i] == o (fs_object_kernel writes both or neither, and distinct ids have
    // distinct first rows), so the kernel of segment_merge.hip without scenes lists the rows of an object
    launch_members(root, obj_root, member_ptr, nullptr, totals, N, members, s);
    launch_pool_members(probs, weights, members, member_ptr, totals, N, C, out_probs, out_weight, s);
    const dim3 waves((unsigned)((N + FS_THREADS / 64 - 1) / (FS_THREADS / 64)));
    if (E > 0) {
        hipLaunchKernelGGL(fs_pair_mark_kernel, exact(E), block, 0, s, edges, (const int32_t*)object, N, E, words, bits);
        hipLaunchKernelGGL(fs_row_count_kernel, waves, block, 0, s, (const unsigned*)bits, N, words, flag);
        launch_scan_i32(flag, N, base, totals + 1, nullptr, s);
        hipLaunchKernelGGL(fs_pair_index_kernel, exact(E), block, 0, s, edges, (const int32_t*)object, (const unsigned*)bits, (const int32_t*)base, N, E,
                           words, edge_to_pair, pair_edges, pair_count);
        hipLaunchKernelGGL(fs_pair_emit_kernel, exact((int64_t)E * R), block, 0, s, rel_probs, (const int32_t*)edge_to_pair, E, R,
                           reinterpret_cast<unsigned*>(pair_probs));
    }
    VLSAT_LAUNCH_CHECK("fuse_splits");
    return 0;
}

}  // namespace vlsat

using namespace vlsat;

extern "C" {

size_t vlsat_split_seeds_scratch_bytes(int64_t n_points) { return split_seeds_scratch_bytes(n_points); }

int vlsat_split_seeds(const float* points, int64_t n_points, double distance, uint64_t seed, const int64_t* ranks, int64_t n_ranks,
                      int32_t max_seeds, void* scratch, int32_t* seeds, int32_t* state, void* stream) {
    if (n_points < 1 || n_points > 0x7fffffff) return fail(VLSAT_EINVAL, "split_seeds: 1 .. 2^31 - 1 points");
    if (!(distance > 0.0) || !(distance * distance < 1e300)) return fail(VLSAT_EINVAL, "split_seeds: distance must be positive and finite");
    if (max_seeds < 1 || max_seeds > 65536) return fail(VLSAT_EINVAL, "split_seeds: max_seeds must be in 1..65536");
    if (n_ranks < 0) return fail(VLSAT_EINVAL, "split_seeds: negative n_ranks");
    if (!points || !scratch || !seeds || !state) return fail(VLSAT_EINVAL, "split_seeds: null argument");
    return launch_split_seeds(points, n_points, distance, seed, ranks, n_ranks, max_seeds, scratch, seeds, state, static_cast<hipStream_t>(stream));
}

int vlsat_split_groups(const float* points, const int32_t* segments, int64_t n_points, const int32_t* segment_ids, int32_t n_seg, int32_t* id_map,
                       int32_t map_size, const int32_t* seeds, int32_t n_seeds, double bbox_distance, int32_t min_seg_per_group, uint32_t* mask,
                       int32_t* counts, int32_t* keep, void* stream) {
    if (n_points < 0 || n_points > 0x7fffffff || n_seg < 0 || n_seeds < 0) return fail(VLSAT_EINVAL, "split_groups: negative size or too many points");
    if (map_size < 1) return fail(VLSAT_EINVAL, "split_groups: map_size must be positive");
    if (bbox_distance != bbox_distance) return fail(VLSAT_EINVAL, "split_groups: bbox_distance is NaN");
    if ((int64_t)n_seeds * ((n_seg + 31) / 32) > 0x7fffffff) return fail(VLSAT_EINVAL, "split_groups: the bit table is too large");
    if (!id_map || (n_points > 0 && (!points || !segments)) || (n_seg > 0 && !segment_ids) || (n_seeds > 0 && (!seeds || !counts || !keep)) ||
        (n_seeds > 0 && n_seg > 0 && !mask))
        return fail(VLSAT_EINVAL, "split_groups: null argument");
    return launch_split_groups(points, segments, n_points, segment_ids, n_seg, id_map, map_size, seeds, n_seeds, bbox_distance, min_seg_per_group,
                               mask, counts, keep, static_cast<hipStream_t>(stream));
}

size_t vlsat_fuse_splits_scratch_bytes(int64_t n_rows, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t map_size) {
    if (fuse_splits_check_args(n_rows, n_edges, n_obj_class, n_rel_class, map_size)) return 0;
    return std::max<size_t>(16, fuse_splits_scratch_bytes(n_rows, n_edges, map_size));
}

int vlsat_fuse_splits(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int32_t* row_instance, const float* weights,
                      int32_t n_rows, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t map_size, void* scratch, int32_t* root,
                      int32_t* object, int32_t* n_objects, int32_t* totals, int32_t* member_ptr, int32_t* members, float* fused_probs,
                      float* obj_weight, int64_t* obj_batch_ids, int32_t* edge_to_pair, int64_t* pair_edges, int32_t* pair_count, float* pair_probs,
                      int32_t* obj_ids, void* stream) {
    if (fuse_splits_check_args(n_rows, n_edges, n_obj_class, n_rel_class, map_size)) return VLSAT_EINVAL;
    if (!scratch || !totals || !member_ptr || !n_objects) return fail(VLSAT_EINVAL, "fuse_splits: null output or scratch");
    if (n_rows > 0 && (!obj_probs || !row_instance || !root || !object || !members || !fused_probs || !obj_weight || !obj_batch_ids || !obj_ids))
        return fail(VLSAT_EINVAL, "fuse_splits: null row argument");
    if (n_edges > 0 && (!rel_probs || !edges || !edge_to_pair || !pair_edges || !pair_count || !pair_probs))
        return fail(VLSAT_EINVAL, "fuse_splits: null edge argument");
    return launch_fuse_splits(obj_probs, rel_probs, edges, row_instance, weights, n_rows, n_edges, n_obj_class, n_rel_class, map_size, scratch, root,
                              object, n_objects, totals, member_ptr, members, fused_probs, obj_weight, obj_batch_ids, edge_to_pair, pair_edges,
                              pair_count, pair_probs, obj_ids, static_cast<hipStream_t>(stream));
}

}  // extern "C"
