// Sums and prefix sums of one integer per thread over a wave and over a block, for the selection kernels (select_core.h) and the
// geometry kernels (segment_merge.hip, scene_split.hip, mesh_segment.hip, voxel.hip, label_transfer.hip, proximity.hip).  Device only.
// Integer addition: the result does not depend on the order of the partial sums, so every user is bit-exact by construction.
// The block functions take their LDS from the caller (THREADS / 64 entries), are uniform calls (every thread of the block, THREADS =
// blockDim.x, a multiple of 64) and end with the barrier that makes a second call on the same LDS safe.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlsat {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// inclusive scan over the wave (int: one count, or two 16-bit counts; long long: two 32-bit counts)
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T x = __shfl_up(v, o);
        if (lane >= o) v += x;
    }
    return v;
}

// sum over the block, in every thread; s_red: THREADS / 64 ints of LDS
template <int THREADS>
__device__ __forceinline__ int block_sum(int c, int* s_red) {
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    int tot = 0;
    for (int i = 0; i < THREADS / 64; ++i) tot += s_red[i];
    __syncthreads();
    return tot;
}

// exclusive prefix of v over the block in thread order; total = the block's sum, in every thread.  The wave's scan, the waves' totals
// through LDS, then the sum of the earlier waves.  s_wave: THREADS / 64 entries of LDS
template <int THREADS, class T>
__device__ __forceinline__ T block_scan_excl(T v, T* s_wave, T& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T incl = wave_scan_incl(v, lane);
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) {
        const T s = s_wave[i];
        if (i < wv) before += s;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}

// One block scans in[0 .. n): thread tid owns the contiguous run [b, e) = [min(tid per, n), min(b + per, n)), per = ceil(n / THREADS)
// (empty past the end), sums it, and learns the sum of the runs before it and of all runs.  The caller writes what it writes: a thread
// that reads in[i] before it stores to out[i] may have out == in, because no other thread touches its run.
template <class T>
struct RunScan {
    int b, e;               // the run
    T sum, before, total;   // of the run, of in[0 .. b), of in[0 .. n)
};
template <int THREADS, class T, class In>
__device__ __forceinline__ RunScan<T> block_run_scan(const In* in, int n, T* s_wave) {
    const int per = (n + THREADS - 1) / THREADS;
    RunScan<T> r;
    r.b = (int)min((int64_t)threadIdx.x * per, (int64_t)n);
    r.e = (int)min((int64_t)r.b + per, (int64_t)n);
    r.sum = 0;
    for (int i = r.b; i < r.e; ++i) r.sum += in[i];
    r.before = block_scan_excl<THREADS>(r.sum, s_wave, r.total);
    return r;
}

}  // namespace vlsat
