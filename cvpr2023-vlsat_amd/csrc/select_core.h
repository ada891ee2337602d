// The selection code shared by the post-forward kernels (eval_recall.hip, scene_graph.hip, graph_decode.hip; the key also by
// proximity.hip and label_transfer.hip).  Every function here is bit-exact by contract: it decides ties, caps and integer ranks.
//
//   key        fkey(x) = bits(x) ^ (sign ? all ones : the sign bit): unsigned order = float order (no NaN; -0 < +0), and every
//              real value has a key > 0, so 0 pads a list or marks "no entry".  For x >= 0 that is bits | sign bit.
//   threshold  the K-th largest of a multiset of keys is the largest T with #{key >= T} >= K, built from the top bit down: 32
//              trials, each a count.  T = 0 when there are fewer than K keys.
//   ties       the keys > T are all kept (fewer than K of them); of the keys == T the first K - #{key > T} in the order the
//              caller enumerates them (lane order in a wave; (list, slot) order over lists).
// The integer helpers compile for the host as well (tests/select_host_check.cpp); the wave and block code is device only (its sums
// and scans are wave_core.h's).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "wave_core.h"
#define VLSAT_HD __host__ __device__ __forceinline__
#else
#define VLSAT_HD inline
#endif

namespace vlsat {

VLSAT_HD uint32_t f32_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
#endif
}
VLSAT_HD float bits_f32(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    memcpy(&x, &u, sizeof x);
    return x;
#endif
}

VLSAT_HD uint32_t fkey(float x) {
    const uint32_t u = f32_bits(x);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
VLSAT_HD float unkey(uint32_t k) { return bits_f32((k >> 31) ? k ^ 0x80000000u : ~k); }

VLSAT_HD int clampi(int64_t x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : (int)x; }

// #{entries >= t} of a descending list of len entries
VLSAT_HD int count_ge(const uint32_t* __restrict__ p, int len, uint32_t t) {
    if (len == 0 || p[0] < t) return 0;            // (most lists, once the trial is near the top: one load)
    int lo = 1, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] >= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Dominance triples.  With three lists sorted descending, the product at sorted position (i, j, k) is dominated by
// (i+1)(j+1)(k+1) - 1 others, so the TOP largest products lie among the positions with (i+1)(j+1)(k+1) <= TOP (k < MAX_R).
// Entry = i | j << 8 | k << 16.
constexpr int tri_count(int top, int max_r) {
    int n = 0;
    for (int a = 1; a <= top; ++a)
        for (int b = 1; a * b <= top; ++b)
            for (int c = 1; c <= max_r && a * b * c <= top; ++c) ++n;
    return n;
}
template <int TOP, int MAX_R>
struct TriTable {
    static constexpr int N = tri_count(TOP, MAX_R);
    uint32_t v[N];
};
template <int TOP, int MAX_R>
constexpr TriTable<TOP, MAX_R> make_tri() {
    TriTable<TOP, MAX_R> t{};
    int n = 0;
    for (int a = 1; a <= TOP; ++a)
        for (int b = 1; a * b <= TOP; ++b)
            for (int c = 1; c <= MAX_R && a * b * c <= TOP; ++c) t.v[n++] = (uint32_t)((a - 1) | ((b - 1) << 8) | ((c - 1) << 16));
    return t;
}
static_assert(tri_count(100, 32) == 1365, "the table of topk_each = 100 and 32 predicates");

#if defined(__HIPCC__)

// position of lane's value among the values of lanes 0 .. R-1 in descending order, equal values to the lower lane
__device__ __forceinline__ int rank_desc_in_wave(float rv, int lane, int R) {
    int rk = 0;
    for (int q = 0; q < R; ++q) {
        const float x = __shfl(rv, q);
        rk += x > rv || (x == rv && q < lane);
    }
    return rk;
}

// the L-th largest of the wave's 64 * PER keys (0 when fewer than L are non-zero)
template <int PER>
__device__ __forceinline__ uint32_t wave_kth_largest(const uint32_t (&v)[PER], int L) {
    uint32_t T = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t trial = T | (1u << bit);
        int c = 0;
#pragma unroll
        for (int t = 0; t < PER; ++t) c += v[t] >= trial;
        if (wave_sum_i(c) >= L) T = trial;
    }
    return T;
}

// The Kk largest keys over the descending lists of edges [e0, e1) (list of e: keys + e * stride, len_of(e) entries), by one block
// of THREADS (thread = edge, chunks of THREADS edges): the threshold T by bisection (bisect = false: every key is kept, T = 0), the
// count above it, and the gather -- sink(pos, e, j) for slot j of edge e at output position pos < Kk: the keys above T in
// (edge, slot) order, then the first Kk - above keys equal to T in (edge, slot) order.  Positions come from a packed block scan
// (#above | #equal << 32) with a running base across the chunks.  Uniform call; 1 <= Kk <= the number of keys.
// s_red / s_scan: THREADS / 64 entries of LDS each.
template <int THREADS, typename LenOf, typename Sink>
__device__ __forceinline__ void select_topk_lists(const uint32_t* __restrict__ keys, int stride, LenOf len_of, int e0, int e1, int Kk, bool bisect,
                                                  int* s_red, long long* s_scan, Sink sink) {
    const int tid = threadIdx.x;
    uint32_t T = 0;
    if (bisect)
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t trial = T | (1u << bit);
            int c = 0;
            for (int e = e0 + tid; e < e1; e += THREADS) c += count_ge(keys + (size_t)e * stride, len_of(e), trial);
            if (block_sum<THREADS>(c, s_red) >= Kk) T = trial;
        }
    int c = 0;
    if (T != 0xFFFFFFFFu)
        for (int e = e0 + tid; e < e1; e += THREADS) c += count_ge(keys + (size_t)e * stride, len_of(e), T + 1);
    const int above = block_sum<THREADS>(c, s_red), need = Kk - above;         // above <= Kk
    long long base = 0;                            // #above | #equal << 32 of the edges before this chunk
    for (int c0 = e0; c0 < e1; c0 += THREADS) {
        const int e = c0 + tid;
        int g = 0, q = 0;
        if (e < e1) {
            const uint32_t* p = keys + (size_t)e * stride;
            const int len = len_of(e);
            g = T != 0xFFFFFFFFu ? count_ge(p, len, T + 1) : 0;
            q = count_ge(p, len, T) - g;
        }
        const long long mine = (long long)g | ((long long)q << 32);
        long long all;
        const long long off = base + block_scan_excl<THREADS>(mine, s_scan, all);
        const int oa = (int)(off & 0xffffffffll);
        const long long oq = off >> 32;
        for (int j = 0; j < g; ++j)
            if (oa + j < Kk) sink(oa + j, e, j);
        for (int j = 0; j < q && oq + j < need; ++j) {
            const int pos = above + (int)(oq + j);
            if (pos < Kk) sink(pos, e, g + j);
        }
        base += all;
    }
}

#endif  // __HIPCC__

}  // namespace vlsat
