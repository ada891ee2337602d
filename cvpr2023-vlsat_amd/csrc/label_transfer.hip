// Annotation transfer onto a predicted segmentation (the rule is stated in include/vlsat.h; reference data_processing/gen_data.py:196-349).
//
// nearest_points   for every query the reference point with the smallest key (bits(d2) << 32) | index among those with d2 <= max_sq_dist,
//                  d2 = (dx dx + dy dy) + dz dz in fp32, every operation rounded on its own (this file is compiled with -ffp-contract=off,
//                  like proximity.hip, so numpy float32 restates d2 bit for bit).  Exact: a uniform grid over the finite reference points
//                  with cell edge >= sqrt(max_sq_dist) (1/64 wider, see nn_params_kernel) and a search of the 27 cells around the query.
//   nn_bbox_kernel     bounding box of the finite points: wave reduction, then integer atomics on the order-preserving key of select_core.h
//   nn_params_kernel   one thread: cell edge, cells per axis (at most NN_AXIS_CELLS each, NN_MAX_CELLS in all: the edge grows until they fit)
//   nn_zero_kernel     counts[0 .. n_cells] = 0
//   nn_hist_kernel     cell of every point (kept), counts[cell] += 1 (int32 atomics)
//   nn_scan_kernel     one block: exclusive scan -> start[0 .. n_cells], cursor = start
//   nn_fill_kernel     sorted[atomicAdd(cursor[cell])] = (x, y, z, index) -- the order inside a cell varies from run to run
//   nn_query_kernel    one thread per query: min of the 64-bit key over the 27 cells -- a function of the points alone, not of that order
// segment_overlap  contingency table predicted segment x annotated instance by int32 atomics (order free), then one wave per segment: best
//                  and second count, number of candidates, and the decision in fp64.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "nn_grid.h"
#include "select_core.h"
#include "wave_core.h"

namespace vlsat {

constexpr int NN_THREADS = 256;
constexpr int NN_SCAN_THREADS = 1024, NN_SCAN_PER = 4;
constexpr unsigned long long NN_NONE = ~0ull;

__global__ void nn_init_kernel(unsigned* __restrict__ box) {
    if (threadIdx.x < 3) box[threadIdx.x] = fkey(INFINITY);
    else if (threadIdx.x < 6) box[threadIdx.x] = fkey(-INFINITY);
}

__global__ __launch_bounds__(NN_THREADS) void nn_bbox_kernel(const float* __restrict__ ref, int n_ref, unsigned* __restrict__ box) {
    unsigned lo[3] = {fkey(INFINITY), fkey(INFINITY), fkey(INFINITY)};
    unsigned hi[3] = {fkey(-INFINITY), fkey(-INFINITY), fkey(-INFINITY)};
    for (int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; i < n_ref; i += (int64_t)gridDim.x * NN_THREADS) {
        const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
        if (!nn_finite3(x, y, z)) continue;
        const unsigned c[3] = {fkey(x), fkey(y), fkey(z)};
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(box + a, lo[a]); atomicMax(box + 3 + a, hi[a]); }
    }
}

// The cell edge h.  Two points with d2 <= max_sq_dist differ by at most sqrt(max_sq_dist) (1 + 2^-22) on an axis (the rounded product
// dx dx is at most d2).  h = sqrt(max_sq_dist) (1 + 2^-6) makes that at most 0.985 cells; a cell coordinate below NN_AXIS_CELLS is off
// by less than 2^-12 after its two roundings and that of 1 / h; so the integer cells of the two points differ by at most one, and the
// 27 cells around a query hold every point that can be its answer.  A larger h keeps that.  h grows (x 1.25 a step) until every axis has
// at most NN_AXIS_CELLS cells and the grid NN_MAX_CELLS; when it cannot (an extent that overflows), one cell holds everything.
__global__ void nn_params_kernel(const unsigned* __restrict__ box, float max_sq_dist, NnGrid* __restrict__ g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    NnGrid r;
    r.inv_h = 0.0f;
    r.n_cells = 1;
    float ext[3];
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = unkey(box[a]), hi = unkey(box[3 + a]);
        any = any && lo <= hi;
        r.lo[a] = lo <= hi ? lo : 0.0f;
        r.n[a] = 1;
        ext[a] = hi - lo;
    }
    if (any) {
        float h = sqrtf(max_sq_dist) * 1.015625f;
        const float ext_max = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
        // max_sq_dist = 0 (or next to it): any edge does, but not one below 1e-18 -- a product dx dx that underflows to zero passes
        // d2 <= 0 with |dx| up to 2^-74, and the cells must be far wider than that
        if (!(h >= 1e-18f)) h = fmaxf(ext_max / (float)NN_AXIS_CELLS, 1e-18f);
        for (int it = 0; it < 512 && isfinite(h) && h > 0.0f; ++it) {
            const float inv = 1.0f / h;
            bool ok = isfinite(inv) && inv > 0.0f;
            int n[3] = {1, 1, 1};
            double cells = 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float t = ext[a] * inv;
                ok = ok && t >= 0.0f && t < (float)NN_AXIS_CELLS;
                if (ok) n[a] = (int)t + 1;
                cells *= (double)n[a];
            }
            if (ok && cells <= (double)NN_MAX_CELLS) {
                r.inv_h = inv;
                r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2];
                r.n_cells = n[0] * n[1] * n[2];
                break;
            }
            h *= 1.25f;
        }
    }
    *g = r;
}

__global__ __launch_bounds__(NN_THREADS) void nn_zero_kernel(const NnGrid* __restrict__ g, int32_t* __restrict__ counts) {
    const int n = min(g->n_cells, NN_MAX_CELLS) + 1;
    for (int i = blockIdx.x * NN_THREADS + threadIdx.x; i < n; i += gridDim.x * NN_THREADS) counts[i] = 0;
}

__device__ __forceinline__ int nn_cell_of(const NnGrid& g, float x, float y, float z) {
    const int cx = nn_cell_axis(x, g.lo[0], g.inv_h, g.n[0]), cy = nn_cell_axis(y, g.lo[1], g.inv_h, g.n[1]),
              cz = nn_cell_axis(z, g.lo[2], g.inv_h, g.n[2]);
    return (cz * g.n[1] + cy) * g.n[0] + cx;
}

__global__ __launch_bounds__(NN_THREADS) void nn_hist_kernel(const float* __restrict__ ref, int n_ref, const NnGrid* __restrict__ gp,
                                                             int32_t* __restrict__ cell, int32_t* __restrict__ counts) {
    const NnGrid g = *gp;
    for (int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; i < n_ref; i += (int64_t)gridDim.x * NN_THREADS) {
        const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
        int c = -1;                                                   // a non-finite point is in no cell: never returned
        if (nn_finite3(x, y, z)) {
            c = nn_cell_of(g, x, y, z);
            if (c >= 0 && c < g.n_cells && c < NN_MAX_CELLS) atomicAdd(counts + c, 1); else c = -1;
        }
        cell[i] = c;
    }
}

// counts[0 .. n_cells) -> start[0 .. n_cells] (exclusive), cursor[c] = start[c] (cursor may be counts).  One block walks the array in
// tiles of NN_SCAN_THREADS x NN_SCAN_PER with a running total.
__global__ __launch_bounds__(NN_SCAN_THREADS) void nn_scan_kernel(const NnGrid* __restrict__ gp, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ start) {
    __shared__ int s_wave[NN_SCAN_THREADS / 64];
    const int n = min(gp->n_cells, NN_MAX_CELLS);
    const int tid = threadIdx.x;
    int carry = 0;                                                    // the total of the tiles before this one, in every thread
    for (int base = 0; base < n; base += NN_SCAN_THREADS * NN_SCAN_PER) {
        const int i0 = base + tid * NN_SCAN_PER;
        int v[NN_SCAN_PER], sum = 0, tile;
#pragma unroll
        for (int k = 0; k < NN_SCAN_PER; ++k) { v[k] = i0 + k < n ? counts[i0 + k] : 0; sum += v[k]; }
        int acc = carry + block_scan_excl<NN_SCAN_THREADS>(sum, s_wave, tile);
#pragma unroll
        for (int k = 0; k < NN_SCAN_PER; ++k) {
            if (i0 + k < n) { start[i0 + k] = acc; counts[i0 + k] = acc; }
            acc += v[k];
        }
        carry += tile;
    }
    if (tid == 0) start[n] = carry;
}

__global__ __launch_bounds__(NN_THREADS) void nn_fill_kernel(const float* __restrict__ ref, int n_ref, const int32_t* __restrict__ cell,
                                                             int32_t* __restrict__ cursor, float4* __restrict__ sorted) {
    for (int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; i < n_ref; i += (int64_t)gridDim.x * NN_THREADS) {
        const int c = cell[i];
        if (c < 0) continue;
        const int p = atomicAdd(cursor + c, 1);
        if (p >= 0 && p < n_ref) sorted[p] = make_float4(ref[i * 3], ref[i * 3 + 1], ref[i * 3 + 2], __int_as_float((int)i));
    }
}

__global__ __launch_bounds__(NN_THREADS) void nn_query_kernel(const float* __restrict__ query, int n_query, int n_ref, float max_sq_dist,
                                                              const NnGrid* __restrict__ gp, const int32_t* __restrict__ start,
                                                              const float4* __restrict__ sorted, int32_t* __restrict__ nn_index,
                                                              float* __restrict__ nn_sqdist) {
    const int64_t q = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (q >= n_query) return;
    const NnGrid g = *gp;
    const float x = query[q * 3], y = query[q * 3 + 1], z = query[q * 3 + 2];
    unsigned long long best = NN_NONE;
    if (nn_finite3(x, y, z)) {
        const int cx = nn_cell_axis(x, g.lo[0], g.inv_h, g.n[0]), cy = nn_cell_axis(y, g.lo[1], g.inv_h, g.n[1]),
                  cz = nn_cell_axis(z, g.lo[2], g.inv_h, g.n[2]);
        for (int kz = max(cz - 1, 0); kz <= min(cz + 1, g.n[2] - 1); ++kz)
            for (int ky = max(cy - 1, 0); ky <= min(cy + 1, g.n[1] - 1); ++ky) {
                // the cells cx-1 .. cx+1 of a row are neighbours in memory: one run of the sorted points
                const int c0 = (kz * g.n[1] + ky) * g.n[0] + max(cx - 1, 0), c1 = (kz * g.n[1] + ky) * g.n[0] + min(cx + 1, g.n[0] - 1);
                if (c0 < 0 || c1 >= g.n_cells || c1 >= NN_MAX_CELLS) continue;
                const int p0 = max(start[c0], 0), p1 = min(start[c1 + 1], n_ref);
                for (int p = p0; p < p1; ++p) {
                    const float4 r = sorted[p];
                    const float dx = __fsub_rn(x, r.x), dy = __fsub_rn(y, r.y), dz = __fsub_rn(z, r.z);
                    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                    if (d2 <= max_sq_dist) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(r.w);
                        best = key < best ? key : best;
                    }
                }
            }
    }
    nn_index[q] = best == NN_NONE ? -1 : (int32_t)(best & 0xffffffffull);
    nn_sqdist[q] = best == NN_NONE ? INFINITY : __uint_as_float((unsigned)(best >> 32));
}

__global__ void nn_none_kernel(int n_query, int32_t* __restrict__ nn_index, float* __restrict__ nn_sqdist) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n_query) { nn_index[q] = -1; nn_sqdist[q] = INFINITY; }
}

// scratch: sorted float4 [n_ref] | grid (64 bytes) | box u32 [8] | cell i32 [n_ref] | counts = cursor i32 [NN_MAX_CELLS + 1] | start i32 [NN_MAX_CELLS + 1]
size_t nn_grid_scratch_bytes(int64_t n_ref) {
    const size_t g = (size_t)(n_ref > 0 ? n_ref : 0);
    return g * 16 + 64 + 32 + align_up(g * 4, 16) + 2 * align_up((size_t)(NN_MAX_CELLS + 1) * 4, 16);
}

// The grid over ref[0 .. n_ref), 1 <= n_ref <= 2^31 - 1, built inside `scratch` (nn_grid_scratch_bytes): seven launches, no check of
// its own -- the caller's VLSAT_LAUNCH_CHECK covers them.
NnGridView launch_nn_grid(const float* ref, int64_t n_ref, float max_sq_dist, void* scratch, hipStream_t s) {
    const int G = (int)n_ref;
    char* p = static_cast<char*>(scratch);
    float4* sorted = reinterpret_cast<float4*>(p);            p += (size_t)G * 16;
    NnGrid* grid = reinterpret_cast<NnGrid*>(p);               p += 64;
    unsigned* box = reinterpret_cast<unsigned*>(p);            p += 32;
    int32_t* cell = reinterpret_cast<int32_t*>(p);             p += align_up((size_t)G * 4, 16);
    int32_t* counts = reinterpret_cast<int32_t*>(p);           p += align_up((size_t)(NN_MAX_CELLS + 1) * 4, 16);
    int32_t* start = reinterpret_cast<int32_t*>(p);
    const dim3 rgrid((unsigned)std::min<int64_t>((n_ref + NN_THREADS - 1) / NN_THREADS, 2048));
    hipLaunchKernelGGL(nn_init_kernel, dim3(1), dim3(64), 0, s, box);
    hipLaunchKernelGGL(nn_bbox_kernel, rgrid, dim3(NN_THREADS), 0, s, ref, G, box);
    hipLaunchKernelGGL(nn_params_kernel, dim3(1), dim3(64), 0, s, box, max_sq_dist, grid);
    hipLaunchKernelGGL(nn_zero_kernel, dim3(1024), dim3(NN_THREADS), 0, s, grid, counts);
    hipLaunchKernelGGL(nn_hist_kernel, rgrid, dim3(NN_THREADS), 0, s, ref, G, grid, cell, counts);
    hipLaunchKernelGGL(nn_scan_kernel, dim3(1), dim3(NN_SCAN_THREADS), 0, s, grid, counts, start);
    hipLaunchKernelGGL(nn_fill_kernel, rgrid, dim3(NN_THREADS), 0, s, ref, G, cell, counts, sorted);
    return NnGridView{sorted, grid, cell, start};
}

size_t nearest_points_scratch_bytes(int64_t n_query, int64_t n_ref) {
    (void)n_query;
    return nn_grid_scratch_bytes(n_ref);
}

int launch_nearest_points(const float* query, int64_t n_query, const float* ref, int64_t n_ref, float max_sq_dist, void* scratch,
                          int32_t* nn_index, float* nn_sqdist, hipStream_t s) {
    if (n_query < 0 || n_ref < 0 || n_query > 0x7fffffff || n_ref > 0x7fffffff) return fail(-1, "nearest_points: bad sizes");
    if (!(max_sq_dist >= 0.0f)) return fail(-1, "nearest_points: max_sq_dist must be >= 0 (it is a squared distance)");
    if (n_query == 0) return 0;
    const int Q = (int)n_query, G = (int)n_ref;
    const dim3 qgrid((unsigned)((n_query + NN_THREADS - 1) / NN_THREADS));
    if (G == 0) {
        hipLaunchKernelGGL(nn_none_kernel, qgrid, dim3(NN_THREADS), 0, s, Q, nn_index, nn_sqdist);
        VLSAT_LAUNCH_CHECK("nearest_points");
        return 0;
    }
    const NnGridView g = launch_nn_grid(ref, n_ref, max_sq_dist, scratch, s);
    hipLaunchKernelGGL(nn_query_kernel, qgrid, dim3(NN_THREADS), 0, s, query, Q, G, max_sq_dist, g.grid, g.start, g.sorted, nn_index, nn_sqdist);
    VLSAT_LAUNCH_CHECK("nearest_points");
    return 0;
}

// ---- segment x instance overlap ------------------------------------------------------------------------------------------------
__global__ void ov_clear_kernel(int32_t* __restrict__ maps, int64_t n_maps, int32_t* __restrict__ size, int n_seg, int32_t* __restrict__ counts,
                                int64_t n_counts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n_maps; i += stride) maps[i] = -1;
    for (int64_t i = t0; i < n_seg; i += stride) size[i] = 0;
    for (int64_t i = t0; i < n_counts; i += stride) counts[i] = 0;
}
__global__ void ov_map_set_kernel(const int32_t* __restrict__ seg_ids, int n_seg, int32_t* __restrict__ seg_map, int seg_map_size,
                                  const int32_t* __restrict__ gt_ids, int n_gt, int32_t* __restrict__ gt_map, int gt_map_size) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seg && seg_ids[i] >= 0 && seg_ids[i] < seg_map_size) seg_map[seg_ids[i]] = i;
    if (i < n_gt && gt_ids[i] >= 0 && gt_ids[i] < gt_map_size) gt_map[gt_ids[i]] = i;
}
__global__ __launch_bounds__(NN_THREADS) void ov_table_kernel(const int32_t* __restrict__ pd_segments, const int32_t* __restrict__ nn_index,
                                                              int n_query, const int32_t* __restrict__ gt_instances, int n_ref,
                                                              const int32_t* __restrict__ seg_map, int seg_map_size, int n_seg,
                                                              const int32_t* __restrict__ gt_map, int gt_map_size, int n_gt,
                                                              int32_t* __restrict__ size, int32_t* __restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; i < n_query; i += (int64_t)gridDim.x * NN_THREADS) {
        const int seg = pd_segments[i];
        if (seg < 0 || seg >= seg_map_size) continue;
        const int s = seg_map[seg];
        if (s < 0 || s >= n_seg) continue;
        atomicAdd(size + s, 1);                                       // every point of the segment, with or without a correspondence
        const int k = nn_index[i];
        if (k < 0 || k >= n_ref) continue;
        const int inst = gt_instances[k];
        if (inst < 0 || inst >= gt_map_size) continue;
        const int g = gt_map[inst];
        if (g < 0 || g >= n_gt) continue;                             // an instance without a label, or labelled 'none'
        atomicAdd(counts + (size_t)s * n_gt + g, 1);
    }
}

// One wave per segment.  Best = largest count, ties to the lower instance id: the max of (count << 32) | ~id.  Second = the largest count
// of the other instances.
__global__ __launch_bounds__(NN_THREADS) void ov_decide_kernel(const int32_t* __restrict__ size, const int32_t* __restrict__ counts,
                                                               const int32_t* __restrict__ gt_ids, int n_seg, int n_gt, int min_seg_size,
                                                               double corr_thres, double occ_thres, int occ_min_candidates,
                                                               int32_t* __restrict__ match, int32_t* __restrict__ best,
                                                               int32_t* __restrict__ second, int32_t* __restrict__ n_candidates) {
    const int s = blockIdx.x * (NN_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n_seg) return;
    unsigned long long k1 = 0;                                        // (no instance: count 0)
    int slot1 = -1, c2 = 0, nc = 0;
    for (int g = lane; g < n_gt; g += 64) {
        const int c = counts[(size_t)s * n_gt + g];
        if (c <= 0) continue;
        ++nc;
        const unsigned long long k = ((unsigned long long)(unsigned)c << 32) | (unsigned)~gt_ids[g];
        if (k > k1) { c2 = max(c2, (int)(k1 >> 32)); k1 = k; slot1 = g; }
        else c2 = max(c2, c);
    }
    unsigned long long kmax = k1;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(kmax, o);
        kmax = t > kmax ? t : kmax;
        nc += __shfl_xor(nc, o);
    }
    const bool winner = kmax != 0 && k1 == kmax;                      // instance ids are distinct: one lane at most
    int sec = winner ? c2 : (int)(k1 >> 32);
    for (int o = 32; o > 0; o >>= 1) sec = max(sec, __shfl_xor(sec, o));
    const unsigned long long wm = __ballot(winner);
    const int slot = wm ? __shfl(slot1, __ffsll((long long)wm) - 1) : -1;
    if (lane != 0) return;
    const int sz = size[s], cb = (int)(kmax >> 32);
    bool accept = false;
    if (sz > min_seg_size && cb > 0 && sz > 0) {
        const double r1 = (double)cb / (double)sz, r2 = (double)sec / (double)sz;
        const double occ = nc >= occ_min_candidates ? r2 / r1 : 0.0;
        accept = r1 > corr_thres && occ < occ_thres;
    }
    match[s] = accept ? slot : -1;
    best[s] = cb;
    second[s] = sec;
    n_candidates[s] = nc;
}

size_t segment_overlap_scratch_bytes(int32_t seg_map_size, int32_t gt_map_size) {
    return ((size_t)(seg_map_size > 0 ? seg_map_size : 0) + (size_t)(gt_map_size > 0 ? gt_map_size : 0)) * 4;
}

int launch_segment_overlap(const int32_t* pd_segments, const int32_t* nn_index, int64_t n_query, const int32_t* gt_instances, int64_t n_ref,
                           const int32_t* segment_ids, int n_seg, const int32_t* gt_ids, int n_gt, int32_t* id_maps, int seg_map_size,
                           int gt_map_size, int min_seg_size, double corr_thres, double occ_thres, int occ_min_candidates, int32_t* size,
                           int32_t* counts, int32_t* match, int32_t* best, int32_t* second, int32_t* n_candidates, hipStream_t s) {
    if (n_query < 0 || n_ref < 0 || n_query > 0x7fffffff || n_ref > 0x7fffffff || n_seg < 0 || n_gt < 0 || seg_map_size <= 0 || gt_map_size <= 0)
        return fail(-1, "segment_overlap: bad sizes");
    if ((int64_t)n_seg * n_gt > 0x7fffffff) return fail(-1, "segment_overlap: the table of counts has more than 2^31 - 1 entries");
    if (corr_thres != corr_thres || occ_thres != occ_thres) return fail(-1, "segment_overlap: a threshold is NaN");
    if (n_seg == 0) return 0;
    int32_t* seg_map = id_maps;
    int32_t* gt_map = id_maps + seg_map_size;
    const int64_t n_maps = (int64_t)seg_map_size + gt_map_size, n_counts = (int64_t)n_seg * n_gt;
    const int64_t most = std::max(std::max(n_maps, n_counts), (int64_t)n_seg);
    hipLaunchKernelGGL(ov_clear_kernel, dim3((unsigned)std::min<int64_t>((most + 255) / 256, 2048)), dim3(256), 0, s, id_maps, n_maps, size, n_seg,
                       counts, n_counts);
    hipLaunchKernelGGL(ov_map_set_kernel, dim3((unsigned)((std::max(n_seg, n_gt) + 255) / 256)), dim3(256), 0, s, segment_ids, n_seg, seg_map,
                       seg_map_size, gt_ids, n_gt, gt_map, gt_map_size);
    if (n_query > 0)
        hipLaunchKernelGGL(ov_table_kernel, dim3((unsigned)std::min<int64_t>((n_query + NN_THREADS - 1) / NN_THREADS, 2048)), dim3(NN_THREADS), 0, s,
                           pd_segments, nn_index, (int)n_query, gt_instances, (int)n_ref, seg_map, seg_map_size, n_seg, gt_map, gt_map_size,
                           n_gt, size, counts);
    hipLaunchKernelGGL(ov_decide_kernel, dim3((unsigned)((n_seg + NN_THREADS / 64 - 1) / (NN_THREADS / 64))), dim3(NN_THREADS), 0, s, size,
                       counts, gt_ids, n_seg, n_gt, min_seg_size, corr_thres, occ_thres, occ_min_candidates, match, best, second,
                       n_candidates);
    VLSAT_LAUNCH_CHECK("segment_overlap");
    return 0;
}

}  // namespace vlsat
