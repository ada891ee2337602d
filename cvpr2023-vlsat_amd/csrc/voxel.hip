// A point cloud resampled on a voxel grid (include/vlsat_voxel.h states the rule; prep.voxel_downsample_host restates it in numpy with
// equal bits): one representative per occupied cell, numbered in input order, and the map from every point to its representative.  The
// arithmetic is voxel_core.h's.
//
// Launches of vlsat_voxel_assign, V points:
//   voxel_clear_kernel    one thread per table slot: key = all ones (empty), first = INT_MAX, count = 0; thread 0 clears the error flag
//   voxel_insert_kernel   one thread per point: the key claimed by a 64-bit compare-and-swap from the empty value, linear probing from
//                         a multiplicative hash, at most `slots` steps (then the error flag is raised and the point has no voxel: the
//                         loop never spins); first by atomicMin, count by atomicAdd; the slot is remembered per point.  Which slot a
//                         key lands in varies from run to run; first and count are a minimum and a sum over a set, which do not.
//   voxel_heads_kernel    point i is a head when first[slot] == i and count >= min_count; heads per block of 256 points
//   scan_i32_kernel       (launch_scan_i32, segment_merge.hip) ONE block: the exclusive scan of the per-block counts in place, a run
//                         of them per thread; the total is M.  Every count is a sum of 0 / 1 flags over the points i < V of a block, so
//                         the total is at most V
//   voxel_number_kernel   the block's own exclusive scan on top of its offset: a head gets its number m and writes first_point[m],
//                         voxel_count[m] and head_number[i]
//   voxel_map_kernel      every point: the number of its slot's head, or -1
// Launches of vlsat_voxel_reduce, M voxels:
//   voxel_zero_kernel, voxel_accumulate_kernel (one thread per point: 64-bit integer atomicAdd per coordinate, 32-bit per colour
//   channel; neighbouring lanes of a wave that hold the same voxel are summed first and issue one atomic), voxel_finalise_kernel (one
//   thread per voxel).
// A plain three-launch scan; no cooperative launch, no spin-wait, no look-back that waits on another block, no host synchronisation
// and no allocation.  Everything read from device memory is checked before it is used as an index.  build.py compiles THIS file with
// -ffp-contract=off (PER_SOURCE_FLAGS).
#include "../../include/vlsat_voxel.h"
#include "common.h"
#include "kernels.h"
#include "voxel_core.h"
#include "wave_core.h"

namespace vlsat {

constexpr int VX_THREADS = VOXEL_THREADS;
constexpr int VX_WAVE = 64;

struct __attribute__((aligned(16))) VoxelSlot {
    unsigned long long key;
    int32_t first;
    int32_t count;
};
static_assert(sizeof(VoxelSlot) == 16, "voxel_layout counts 16 bytes per slot");

__global__ __launch_bounds__(VX_THREADS) void voxel_clear_kernel(VoxelSlot* __restrict__ table, uint32_t slots, int32_t* __restrict__ n_voxels) {
    const uint32_t s = blockIdx.x * VX_THREADS + threadIdx.x;
    if (s == 0) n_voxels[1] = 0;
    if (s >= slots) return;
    VoxelSlot empty;
    empty.key = VOXEL_EMPTY;
    empty.first = INT32_MAX;
    empty.count = 0;
    table[s] = empty;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_insert_kernel(const float* __restrict__ points, int n_points, float ox, float oy, float oz,
                                                                  float inv, VoxelSlot* table, int log2_slots,
                                                                  int32_t* __restrict__ slot_of_point, int32_t* n_voxels) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= n_points) return;
    const unsigned long long key =
        voxel_key(points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2], ox, oy, oz, inv);
    int32_t mine = -1;
    if (key != VOXEL_EMPTY) {
        const uint32_t slots = 1u << log2_slots, mask = slots - 1u;
        uint32_t h = voxel_hash(key, log2_slots) & mask;
        for (uint32_t step = 0; step < slots; ++step) {
            unsigned long long seen = __atomic_load_n(&table[h].key, __ATOMIC_RELAXED);
            if (seen == VOXEL_EMPTY) seen = atomicCAS(&table[h].key, VOXEL_EMPTY, key);
            if (seen == VOXEL_EMPTY || seen == key) {
                mine = (int32_t)h;
                break;
            }
            h = (h + 1u) & mask;
        }
        if (mine >= 0) {
            atomicMin(&table[mine].first, i);
            atomicAdd(&table[mine].count, 1);
        } else {
            atomicMax(&n_voxels[1], 1);                               // the table is full: cannot happen with slots >= 2 V, and is reported
        }
    }
    slot_of_point[i] = mine;
}

// 1 when point i opens a kept voxel; `count` is its voxel's then
__device__ __forceinline__ int voxel_is_head(const VoxelSlot* __restrict__ table, uint32_t slots, const int32_t* __restrict__ slot_of_point,
                                             int i, int n_points, int min_count, int32_t& count) {
    count = 0;
    if (i >= n_points) return 0;
    const int32_t s = slot_of_point[i];
    if (s < 0 || (uint32_t)s >= slots) return 0;
    count = table[s].count;
    return table[s].first == i && count >= min_count;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_heads_kernel(const VoxelSlot* __restrict__ table, uint32_t slots,
                                                                 const int32_t* __restrict__ slot_of_point, int n_points, int min_count,
                                                                 int32_t* __restrict__ block_heads) {
    __shared__ int s_red[VX_THREADS / 64];
    int32_t count;
    const int head = voxel_is_head(table, slots, slot_of_point, blockIdx.x * VX_THREADS + threadIdx.x, n_points, min_count, count);
    const int total = block_sum<VX_THREADS>(head, s_red);
    if (threadIdx.x == 0) block_heads[blockIdx.x] = total;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_number_kernel(const VoxelSlot* __restrict__ table, uint32_t slots,
                                                                  const int32_t* __restrict__ slot_of_point, int n_points, int min_count,
                                                                  const int32_t* __restrict__ block_heads, int32_t* __restrict__ head_number,
                                                                  int32_t* __restrict__ first_point, int32_t* __restrict__ voxel_count) {
    __shared__ int s_wave[VX_THREADS / 64];
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    int32_t count;
    const int head = voxel_is_head(table, slots, slot_of_point, i, n_points, min_count, count);
    int total;
    const int m = block_heads[blockIdx.x] + block_scan_excl<VX_THREADS>(head, s_wave, total);
    if (i >= n_points) return;
    const bool ok = head && m >= 0 && m < n_points;
    head_number[i] = ok ? m : -1;
    if (ok) {
        first_point[m] = i;
        voxel_count[m] = count;
    }
}

__global__ __launch_bounds__(VX_THREADS) void voxel_map_kernel(const VoxelSlot* __restrict__ table, uint32_t slots,
                                                               const int32_t* __restrict__ slot_of_point,
                                                               const int32_t* __restrict__ head_number, int n_points,
                                                               int32_t* __restrict__ voxel_of_point) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= n_points) return;
    const int32_t s = slot_of_point[i];
    int32_t m = -1;
    if (s >= 0 && (uint32_t)s < slots) {
        const int32_t f = table[s].first;
        if (f >= 0 && f < n_points) m = head_number[f];               // -1 when the voxel was dropped: its first point is no head
    }
    voxel_of_point[i] = m;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_zero_kernel(long long* __restrict__ point_sum, long long* __restrict__ normal_sum,
                                                                uint32_t* __restrict__ color_sum, int rows3) {
    const int e = blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= rows3) return;
    point_sum[e] = 0;
    if (normal_sum) normal_sum[e] = 0;
    if (color_sum) color_sum[e] = 0;
}

__device__ __forceinline__ void voxel_add(long long* p, long long q) { atomicAdd((unsigned long long*)p, (unsigned long long)q); }

// sums over the lanes of a wave that follow this one and hold the same voxel: after the loop a lane that opens a run (its predecessor
// holds another voxel) has the sum of the whole run.  `reach` = how many lanes after this one belong to its run.
template <class T>
__device__ __forceinline__ T voxel_run_sum(T v, int reach, int longest) {
    for (int d = 1; d <= longest; d <<= 1) {
        const T o = __shfl_down(v, d, VX_WAVE);
        if (reach >= d) v += o;
    }
    return v;
}

// One thread per point.  Neighbours in the file are often neighbours in space, so the lanes of a wave that stand side by side and hold
// the same voxel are summed in registers first and the lane that opens the run issues the atomics.  Integer sums: the result is the
// same whatever is summed first.
__global__ __launch_bounds__(VX_THREADS) void voxel_accumulate_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                                      const uint8_t* __restrict__ colors,
                                                                      const int32_t* __restrict__ voxel_of_point, int n_points, int n_voxels,
                                                                      long long* point_sum, long long* normal_sum, uint32_t* color_sum) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    int32_t m = -1;
    if (i < n_points) {
        m = voxel_of_point[i];
        if (m < 0 || m >= n_voxels) m = -1;
    }
    const size_t in = (size_t)max(min(i, n_points - 1), 0) * 3, out = (size_t)max(m, 0) * 3;
    long long qp[3] = {0, 0, 0}, qn[3] = {0, 0, 0};
    uint32_t qc[3] = {0, 0, 0};
    if (m >= 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            qp[c] = voxel_quantise(points[in + c], VOXEL_POINT_SCALE);
            if (normals) qn[c] = voxel_quantise_normal(normals[in + c]);
            if (colors) qc[c] = colors[in + c];
        }
    }
    const int lane = threadIdx.x & (VX_WAVE - 1);
    const int32_t before = __shfl_up(m, 1, VX_WAVE);
    const bool opens = lane == 0 || before != m;
    const unsigned long long heads = __ballot(opens);
    const unsigned long long later = lane == VX_WAVE - 1 ? 0ull : heads >> (lane + 1);              // bit d - 1: lane + d opens a run
    const int reach = later ? __ffsll((long long)later) - 1 : VX_WAVE - 1 - lane;
    int longest = reach;
#pragma unroll
    for (int d = 1; d < VX_WAVE; d <<= 1) longest = max(longest, __shfl_xor(longest, d, VX_WAVE));
    if (longest > 0) {                                                   // wave-uniform: a wave without two equal neighbours skips it
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            qp[c] = voxel_run_sum(qp[c], reach, longest);
            if (normals) qn[c] = voxel_run_sum(qn[c], reach, longest);
            if (colors) qc[c] = voxel_run_sum(qc[c], reach, longest);
        }
    }
    const bool issue = m >= 0 && opens;
    if (!issue) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        voxel_add(point_sum + out + c, qp[c]);
        if (normals) voxel_add(normal_sum + out + c, qn[c]);
        if (colors) atomicAdd(color_sum + out + c, qc[c]);
    }
}

__global__ __launch_bounds__(VX_THREADS) void voxel_finalise_kernel(const long long* __restrict__ point_sum,
                                                                    const long long* __restrict__ normal_sum,
                                                                    const uint32_t* __restrict__ color_sum,
                                                                    const int32_t* __restrict__ voxel_count, int n_voxels,
                                                                    float* __restrict__ out_points, float* __restrict__ out_normals,
                                                                    uint8_t* __restrict__ out_colors) {
    const int m = blockIdx.x * VX_THREADS + threadIdx.x;
    if (m >= n_voxels) return;
    const int32_t count = max(voxel_count[m], 1);
    const size_t o = (size_t)m * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out_points[o + c] = voxel_mean(point_sum[o + c], count);
    if (normal_sum) {
        float nx, ny, nz;
        voxel_normal(normal_sum[o], normal_sum[o + 1], normal_sum[o + 2], nx, ny, nz);
        out_normals[o] = nx;
        out_normals[o + 1] = ny;
        out_normals[o + 2] = nz;
    }
    if (color_sum) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out_colors[o + c] = voxel_color(color_sum[o + c], count);
    }
}

static unsigned vx_blocks(int64_t n) { return (unsigned)((n + VX_THREADS - 1) / VX_THREADS); }

}  // namespace vlsat

using namespace vlsat;

extern "C" {

size_t vlsat_voxel_scratch_bytes(int64_t n_points) {
    if (!voxel_sizes_ok(n_points)) return 0;
    return voxel_layout(n_points).bytes;
}

int vlsat_voxel_assign(const float* points, int64_t n_points, float voxel, float ox, float oy, float oz, int32_t min_count, void* scratch,
                       int32_t* voxel_of_point, int32_t* first_point, int32_t* voxel_count, int32_t* n_voxels, void* stream) {
    if (!voxel_sizes_ok(n_points)) return fail(VLSAT_EINVAL, "voxel_assign: 1 .. 2^24 points");
    float inv = 0.0f;
    if (!voxel_inverse(voxel, inv)) return fail(VLSAT_EINVAL, "voxel_assign: voxel must be > 0 and finite, and so must 1 / voxel in fp32");
    if (!(fabsf(ox) < INFINITY && fabsf(oy) < INFINITY && fabsf(oz) < INFINITY)) return fail(VLSAT_EINVAL, "voxel_assign: the origin must be finite");
    if (min_count < 1) return fail(VLSAT_EINVAL, "voxel_assign: min_count must be at least 1");
    if (!points || !scratch || !voxel_of_point || !first_point || !voxel_count || !n_voxels)
        return fail(VLSAT_EINVAL, "voxel_assign: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int V = (int)n_points, log2_slots = voxel_log2_slots(n_points);
    const uint32_t slots = 1u << log2_slots;
    const VoxelLayout l = voxel_layout(n_points);
    char* base = static_cast<char*>(scratch);
    VoxelSlot* table = reinterpret_cast<VoxelSlot*>(base + l.table);
    int32_t* slot_of_point = reinterpret_cast<int32_t*>(base + l.slot_of_point);
    int32_t* head_number = reinterpret_cast<int32_t*>(base + l.head_number);
    int32_t* block_heads = reinterpret_cast<int32_t*>(base + l.block_heads);
    const unsigned blocks = vx_blocks(V);
    hipLaunchKernelGGL(voxel_clear_kernel, dim3(vx_blocks(slots)), dim3(VX_THREADS), 0, s, table, slots, n_voxels);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3(blocks), dim3(VX_THREADS), 0, s, points, V, ox, oy, oz, inv, table, log2_slots, slot_of_point,
                       n_voxels);
    hipLaunchKernelGGL(voxel_heads_kernel, dim3(blocks), dim3(VX_THREADS), 0, s, table, slots, slot_of_point, V, (int)min_count, block_heads);
    launch_scan_i32(block_heads, (int)blocks, block_heads, n_voxels, nullptr, s);   // in place; n_voxels[0] = the total <= V
    hipLaunchKernelGGL(voxel_number_kernel, dim3(blocks), dim3(VX_THREADS), 0, s, table, slots, slot_of_point, V, (int)min_count, block_heads,
                       head_number, first_point, voxel_count);
    hipLaunchKernelGGL(voxel_map_kernel, dim3(blocks), dim3(VX_THREADS), 0, s, table, slots, slot_of_point, head_number, V, voxel_of_point);
    VLSAT_LAUNCH_CHECK("voxel_assign");
    return 0;
}

int vlsat_voxel_reduce(const float* points, const float* normals, const uint8_t* colors, const int32_t* voxel_of_point,
                       const int32_t* voxel_count, int64_t n_points, int64_t n_voxels, void* scratch, float* out_points, float* out_normals,
                       uint8_t* out_colors, void* stream) {
    if (!voxel_sizes_ok(n_points)) return fail(VLSAT_EINVAL, "voxel_reduce: 1 .. 2^24 points");
    if (n_voxels < 0 || n_voxels > n_points) return fail(VLSAT_EINVAL, "voxel_reduce: n_voxels must be in [0, n_points]");
    if (!points || !voxel_of_point || !voxel_count || !scratch) return fail(VLSAT_EINVAL, "voxel_reduce: null argument");
    if (n_voxels == 0) return 0;
    if (!out_points || (normals && !out_normals) || (colors && !out_colors))
        return fail(VLSAT_EINVAL, "voxel_reduce: an input without the output it is averaged into");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int V = (int)n_points, M = (int)n_voxels;
    const VoxelLayout l = voxel_layout(n_points);
    char* base = static_cast<char*>(scratch);
    long long* point_sum = reinterpret_cast<long long*>(base + l.point_sum);
    long long* normal_sum = normals ? reinterpret_cast<long long*>(base + l.normal_sum) : nullptr;
    uint32_t* color_sum = colors ? reinterpret_cast<uint32_t*>(base + l.color_sum) : nullptr;
    hipLaunchKernelGGL(voxel_zero_kernel, dim3(vx_blocks((int64_t)M * 3)), dim3(VX_THREADS), 0, s, point_sum, normal_sum, color_sum, M * 3);
    hipLaunchKernelGGL(voxel_accumulate_kernel, dim3(vx_blocks(V)), dim3(VX_THREADS), 0, s, points, normals, colors, voxel_of_point, V, M,
                       point_sum, normal_sum, color_sum);
    hipLaunchKernelGGL(voxel_finalise_kernel, dim3(vx_blocks(M)), dim3(VX_THREADS), 0, s, point_sum, normal_sum, color_sum, voxel_count, M,
                       out_points, out_normals, out_colors);
    VLSAT_LAUNCH_CHECK("voxel_reduce");
    return 0;
}

}  // extern "C"
