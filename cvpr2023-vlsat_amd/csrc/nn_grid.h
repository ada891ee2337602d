// The uniform grid of label_transfer.hip as seen by its users (nearest_points there, the kNN kernel of cloud.hip): the grid's
// parameters, the cell of a coordinate, and the views into the scratch block that launch_nn_grid (kernels.h) fills.  The build itself
// -- bbox, params, zero, hist, scan, fill -- exists once, in label_transfer.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlsat {

constexpr int NN_AXIS_CELLS = 1024;            // cells per axis: keeps the rounding of a cell coordinate below 1/64 of a cell (nn_params_kernel)
constexpr int NN_MAX_CELLS = 1 << 21;          // cells in all (the histogram and its scan are this long at most)

struct NnGrid {
    float lo[3];
    float inv_h;
    int n[3];
    int n_cells;
};

// What launch_nn_grid built inside the caller's scratch block: the finite points in cell order as (x, y, z, bits of the index) -- the
// order inside a cell varies from run to run --, the grid's parameters, the cell of every point (-1: in no cell) and the first sorted
// slot of every cell (start[n_cells] = the number of sorted points).
struct NnGridView {
    const float4* sorted;
    const NnGrid* grid;
    const int32_t* cell;
    const int32_t* start;
};

__device__ __forceinline__ bool nn_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// cell coordinate on one axis: monotone in x, clamped to [0, n).  A NaN product (an overflowed difference times inv_h = 0) gives 0.
__device__ __forceinline__ int nn_cell_axis(float x, float lo, float inv_h, int n) {
    const float t = (x - lo) * inv_h;
    if (!(t >= 0.0f)) return 0;
    return min((int)fminf(t, (float)(NN_AXIS_CELLS - 1)), n - 1);
}

}  // namespace vlsat
