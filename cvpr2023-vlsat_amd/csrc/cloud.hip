// A point cloud without faces made ready for the segmenter (include/vlsat_cloud.h states the rules; prep.knn_points_host and
// prep.cloud_normals_host restate them in numpy with the same operations): the K nearest neighbours of every point, then a normal and
// a flatness measure per point from that neighbourhood.  The arithmetic is cloud_core.h's; the grid is label_transfer.hip's
// (launch_nn_grid: bbox, params, zero, hist, scan, fill -- cell edge >= sqrt(max_sq_dist) (1 + 2^-6), so the 27 cells around a point
// hold every candidate).
//
// Launches of vlsat_cloud_knn, V points:
//   the grid's seven
//   cloud_pad_kernel      one thread per point: a point in no cell (a non-finite coordinate) gets count 0 and a padded row
//   cloud_knn_kernel<CAP> one thread per SORTED slot, CAP = 8 / 16 / 32 >= K: the lanes of a wave stand in the same or in neighbouring
//                         cells and read the same runs of `sorted`.  The CAP best keys live in registers: an ascending list, a new key
//                         enters at the end behind the guard key < worst and sinks through an unrolled compare-exchange chain -- every
//                         index is a compile-time constant, so nothing goes to scratch memory.  The first K of the CAP smallest are the
//                         K smallest.  The minimum over a set does not depend on the order the set is walked in: the order of points
//                         inside a cell varies from run to run, the result does not.
// vlsat_cloud_normals: cloud_normals_kernel, one thread per point, fp64, every operation rounded on its own.
// Plain stores only here (the grid build has the integer atomics); no cooperative launch, no spin-wait, no host synchronisation and no
// allocation.  build.py compiles THIS file with -ffp-contract=off (PER_SOURCE_FLAGS).
#include "../../include/vlsat_cloud.h"
#include "cloud_core.h"
#include "common.h"
#include "kernels.h"
#include "nn_grid.h"

namespace vlsat {

constexpr int CK_THREADS = 256;

__global__ __launch_bounds__(CK_THREADS) void cloud_pad_kernel(const int32_t* __restrict__ cell, int n_points, int K, int32_t* __restrict__ nbr,
                                                               float* __restrict__ nbr_sqdist, int32_t* __restrict__ nbr_count) {
    const int i = blockIdx.x * CK_THREADS + threadIdx.x;
    if (i >= n_points || cell[i] >= 0) return;
    nbr_count[i] = 0;
    for (int k = 0; k < K; ++k) {
        nbr[(size_t)i * K + k] = -1;
        nbr_sqdist[(size_t)i * K + k] = INFINITY;
    }
}

template <int CAP>
__global__ __launch_bounds__(CK_THREADS) void cloud_knn_kernel(int n_points, int K, float max_sq_dist, const NnGrid* __restrict__ gp,
                                                               const int32_t* __restrict__ start, const float4* __restrict__ sorted,
                                                               int32_t* __restrict__ nbr, float* __restrict__ nbr_sqdist,
                                                               int32_t* __restrict__ nbr_count) {
    const NnGrid g = *gp;
    const int n_cells = min(max(g.n_cells, 1), NN_MAX_CELLS);
    const int n_sorted = min(max(start[n_cells], 0), n_points);
    const int p = blockIdx.x * CK_THREADS + threadIdx.x;
    if (p >= n_sorted) return;
    const float4 me = sorted[p];
    const int i = __float_as_int(me.w);
    if (i < 0 || i >= n_points) return;
    unsigned long long best[CAP];
#pragma unroll
    for (int k = 0; k < CAP; ++k) best[k] = CLOUD_NO_KEY;
    const int cx = nn_cell_axis(me.x, g.lo[0], g.inv_h, g.n[0]), cy = nn_cell_axis(me.y, g.lo[1], g.inv_h, g.n[1]),
              cz = nn_cell_axis(me.z, g.lo[2], g.inv_h, g.n[2]);
    for (int kz = max(cz - 1, 0); kz <= min(cz + 1, g.n[2] - 1); ++kz)
        for (int ky = max(cy - 1, 0); ky <= min(cy + 1, g.n[1] - 1); ++ky) {
            // the cells cx-1 .. cx+1 of a row are neighbours in memory: one run of the sorted points
            const int c0 = (kz * g.n[1] + ky) * g.n[0] + max(cx - 1, 0), c1 = (kz * g.n[1] + ky) * g.n[0] + min(cx + 1, g.n[0] - 1);
            if (c0 < 0 || c1 >= n_cells) continue;
            const int p0 = max(start[c0], 0), p1 = min(start[c1 + 1], n_sorted);
            for (int q = p0; q < p1; ++q) {
                const float4 r = sorted[q];
                const int j = __float_as_int(r.w);
                const float d2 = cloud_d2(me.x, me.y, me.z, r.x, r.y, r.z);
                if (j != i && d2 <= max_sq_dist) cloud_insert<CAP>(best, cloud_key(d2, j));
            }
        }
    int count = 0;
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
        if (k < K) {
            const bool have = best[k] != CLOUD_NO_KEY;
            count += have;
            nbr[(size_t)i * K + k] = have ? cloud_key_index(best[k]) : -1;
            nbr_sqdist[(size_t)i * K + k] = have ? cloud_key_d2(best[k]) : INFINITY;
        }
    }
    nbr_count[i] = count;
}

struct CloudRowMembers {
    const float* points;
    const int32_t* row;
    int n_points;
    __device__ __forceinline__ bool operator()(int k, double& x, double& y, double& z) const {
        const int j = row[k];
        if (j < 0 || j >= n_points) return false;                    // an entry that names no point is no member
        x = (double)points[(size_t)j * 3];
        y = (double)points[(size_t)j * 3 + 1];
        z = (double)points[(size_t)j * 3 + 2];
        return true;
    }
};

__global__ __launch_bounds__(CK_THREADS) void cloud_normals_kernel(const float* __restrict__ points, const int32_t* __restrict__ nbr,
                                                                   const int32_t* __restrict__ nbr_count, int n_points, int K, int min_points,
                                                                   int use_viewpoint, double vx, double vy, double vz,
                                                                   float* __restrict__ normals, float* __restrict__ curvature) {
    const int i = blockIdx.x * CK_THREADS + threadIdx.x;
    if (i >= n_points) return;
    const CloudRowMembers members{points, nbr + (size_t)i * K, n_points};
    const int listed = min(max(nbr_count[i], 0), K);
    const CloudNormal n = cloud_point_normal(members, listed, (double)points[(size_t)i * 3], (double)points[(size_t)i * 3 + 1],
                                             (double)points[(size_t)i * 3 + 2], min_points, use_viewpoint != 0, vx, vy, vz);
    normals[(size_t)i * 3] = __double2float_rn(n.x);
    normals[(size_t)i * 3 + 1] = __double2float_rn(n.y);
    normals[(size_t)i * 3 + 2] = __double2float_rn(n.z);
    curvature[i] = __double2float_rn(n.curvature);
}

template <int CAP>
static void launch_knn(int V, int K, float max_sq_dist, const NnGridView& g, int32_t* nbr, float* nbr_sqdist, int32_t* nbr_count, hipStream_t s) {
    hipLaunchKernelGGL(cloud_knn_kernel<CAP>, dim3((unsigned)((V + CK_THREADS - 1) / CK_THREADS)), dim3(CK_THREADS), 0, s, V, K, max_sq_dist,
                       g.grid, g.start, g.sorted, nbr, nbr_sqdist, nbr_count);
}

}  // namespace vlsat

using namespace vlsat;

extern "C" {

size_t vlsat_cloud_knn_scratch_bytes(int64_t n_points, int32_t k) {
    if (!cloud_sizes_ok(n_points, k)) return 0;
    return nn_grid_scratch_bytes(n_points);
}

int vlsat_cloud_knn(const float* points, int64_t n_points, int32_t k, float max_sq_dist, void* scratch, int32_t* nbr, float* nbr_sqdist,
                    int32_t* nbr_count, void* stream) {
    if (!cloud_sizes_ok(n_points, k)) return fail(VLSAT_EINVAL, "cloud_knn: 1 .. 2^24 points and 1 .. 32 neighbours");
    if (!(max_sq_dist >= 0.0f)) return fail(VLSAT_EINVAL, "cloud_knn: max_sq_dist must be >= 0 (it is a squared distance)");
    if (!points || !scratch || !nbr || !nbr_sqdist || !nbr_count) return fail(VLSAT_EINVAL, "cloud_knn: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int V = (int)n_points, K = (int)k;
    const NnGridView g = launch_nn_grid(points, n_points, max_sq_dist, scratch, s);
    hipLaunchKernelGGL(cloud_pad_kernel, dim3((unsigned)((V + CK_THREADS - 1) / CK_THREADS)), dim3(CK_THREADS), 0, s, g.cell, V, K, nbr,
                       nbr_sqdist, nbr_count);
    switch (cloud_knn_capacity(K)) {
        case 8: launch_knn<8>(V, K, max_sq_dist, g, nbr, nbr_sqdist, nbr_count, s); break;
        case 16: launch_knn<16>(V, K, max_sq_dist, g, nbr, nbr_sqdist, nbr_count, s); break;
        default: launch_knn<32>(V, K, max_sq_dist, g, nbr, nbr_sqdist, nbr_count, s); break;
    }
    VLSAT_LAUNCH_CHECK("cloud_knn");
    return 0;
}

int vlsat_cloud_normals(const float* points, const int32_t* nbr, const int32_t* nbr_count, int64_t n_points, int32_t k, int32_t min_points,
                        int32_t use_viewpoint, double vx, double vy, double vz, float* normals, float* curvature, void* stream) {
    if (!cloud_sizes_ok(n_points, k)) return fail(VLSAT_EINVAL, "cloud_normals: 1 .. 2^24 points and 1 .. 32 neighbours");
    if (min_points < CLOUD_MIN_POINTS) return fail(VLSAT_EINVAL, "cloud_normals: min_points must be at least 3");
    if (use_viewpoint && !(vx == vx && vy == vy && vz == vz)) return fail(VLSAT_EINVAL, "cloud_normals: the viewpoint is NaN");
    if (!points || !nbr || !nbr_count || !normals || !curvature) return fail(VLSAT_EINVAL, "cloud_normals: null argument");
    const int V = (int)n_points;
    hipLaunchKernelGGL(cloud_normals_kernel, dim3((unsigned)((V + CK_THREADS - 1) / CK_THREADS)), dim3(CK_THREADS), 0,
                       static_cast<hipStream_t>(stream), points, nbr, nbr_count, V, (int)k, (int)min_points, (int)use_viewpoint, vx, vy, vz,
                       normals, curvature);
    VLSAT_LAUNCH_CHECK("cloud_normals");
    return 0;
}

}  // extern "C"
