// The lock-free union-find of segment_merge.hip and mesh_segment.hip over parent[0 .. n), parent[v] = v at the start.  Device only.
//   - A parent only ever decreases (hooks put the larger root under the smaller, path halving writes by atomicMin), so parent[v] <= v,
//     every walk ends, and the root of a tree is its lowest row: the components do not depend on the order the threads ran in.
//   - A CAS is only ever aimed at the LARGER of two roots, which then stops being a root for good.  Nobody retries a CAS on a hot root
//     (a floor that holds a third of all vertices): it is read by many and written by none once it is the lowest row of its component.
//   - A find that raced with a hook returns a stale root, which is still an ancestor: the CAS of the caller then fails and it walks on,
//     strictly downwards.
// Inside a launch threads meet only in these device-scope atomics; uf_root reads with plain loads in a LATER launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlsat {

__device__ __forceinline__ int uf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v as far as this thread can see it
__device__ __forceinline__ int uf_find(int32_t* __restrict__ parent, int v) {
    int curr = uf_load(parent + v);
    if (curr == v) return v;
    int prev = v, next;
    while ((next = uf_load(parent + curr)) < curr) {
        atomicMin(parent + prev, next);                               // path halving
        prev = curr;
        curr = next;
    }
    return curr;
}

__device__ __forceinline__ void uf_unite(int32_t* __restrict__ parent, int a, int b) {
    int ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        if (ra < rb) { const int t = ra; ra = rb; rb = t; }           // ra > rb: hook ra under rb
        const int old = atomicCAS(parent + ra, ra, rb);
        if (old == ra) break;
        ra = uf_find(parent, old);                                    // ra had been hooked meanwhile (old < ra)
        rb = uf_find(parent, rb);
    }
}

// the root of v once every union is done (a launch later); n bounds the walk and is a belt: parent[r] <= r ends it
__device__ __forceinline__ int uf_root(const int32_t* __restrict__ parent, int v, int n) {
    int r = v;
    for (int step = 0; step < n; ++step) {
        const int p = parent[r];
        if (p >= r || p < 0) break;
        r = p;
    }
    return r;
}

}  // namespace vlsat
