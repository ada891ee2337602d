/*
 * vlsat_segment.h -- the part of libvlsat_hip.so's C ABI that over-segments an unlabelled mesh into segments (csrc/mesh_segment.hip):
 * the per-vertex instance id every other entry point takes as given.  Conventions, error codes and vlsat_last_error() are those of
 * vlsat.h; the symbols are exported from the same library and bound by lib.py from its registry row HEADERS["segment"].
 *
 * Why.  prepare_scan, split_scan, transfer_labels and merge_graph all start from a segmentation someone else made: the annotators'
 * objectId, or the output of an outside tool (the reference's data_processing/gen_data.py:188 reads an inseg.ply that ships with
 * neither project).  The rule below is smoothness-constrained region growing plus small-segment absorption: an over-segmentation,
 * which vlsat_merge_segments then fuses into objects along "same part" edges.  It is NOT the Felzenszwalb-Huttenlocher ordering of
 * the mesh segmentators behind 3RScan's segs.v2.json: that visits edges one by one in weight order and has no exact parallel form.
 * prep.segment_mesh_host restates the rule in numpy with the same operations: labels, count and sizes are equal.
 *
 * The call takes device pointers, is asynchronous on `stream` (no host synchronisation, no allocation, no runtime fill), returns 0
 * or a negative VLSAT_E* code and sets vlsat_last_error; every limit is checked before anything is launched.  Integer vector
 * atomics and plain stores only; no cooperative launch, no barrier and no spin-wait between blocks -- a launch boundary is the only
 * cross-block ordering.  No result depends on scheduling.
 */
#ifndef VLSAT_SEGMENT_H
#define VLSAT_SEGMENT_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------- the rule --------
 *
 * Inputs: normals f32 [V,3] (unit length is the caller's business: the rule only takes dot products); edges int32 [M,2], undirected,
 *   for a mesh the three sides of every triangle; max_weight f32 (not NaN); min_verts int32.  1 <= V <= 2^24, 0 <= M < 2^31.
 *   Duplicates need no removal.  An edge with an end outside [0, V) or with a == b is ignored.
 *
 * 1. Weight.  d = fl(fl(fl(ax*bx) + fl(ay*by)) + fl(az*bz)) in fp32, every product and sum rounded on its own; w = fl(1 - d) clamped
 *    to [0, 2]; a NaN d gives w = 2.  w is symmetric in a and b.  (csrc/segment_core.h holds the function, for the kernels and for a
 *    host program alike.)
 * 2. Link.  Edges with w <= max_weight link their ends.  Components are the connected components of the links; a component's root is
 *    its lowest vertex index.
 * 3. Absorb.  R = ceil(log2(min_verts)) rounds (0 when min_verts <= 1).  In each round sizes are counted from the current roots; a
 *    component is small when size < min_verts; every small component takes the minimum key over all directed edges (a, b) with a
 *    inside it and root(b) != root(a) -- edges above max_weight take part -- where key = (uint64(bits(w)) << 32) | root(b): the
 *    lowest weight, and on a tie the lower target root (bits(w) is monotone because w >= 0); every small component that has a key is
 *    united with its target.  Union is a set operation: mutual choices and chains need no special case and the result does not depend
 *    on order.  After r rounds a component that is still small and still has an outgoing edge holds at least 2^r former components,
 *    so R rounds reach the fixed point and nothing is read back to decide when to stop.
 * 4. Drop.  A component still smaller than min_verts is an island without neighbours: its vertices get id 0, the dataset's
 *    "unlabelled", which prepare_scan skips.
 * 5. Number.  The kept components are numbered 1..S in the order of their lowest vertex.
 *
 * Outputs: labels int32 [V]; n_segments int32 [1] = S; seg_size int32 [V]: seg_size[s - 1] = the number of vertices of segment s,
 *   entries past S hold 0.  Every entry of every output is written by the call.
 * scratch: vlsat_segment_mesh_scratch_bytes(V, M) bytes (24 per vertex and 8 per 1024 vertices, rounded up; nothing per edge: a weight
 *   is recomputed where it is used; 0 = arguments out of range), 16-byte aligned.
 * The call enqueues 8 + 4 R launches (7 when M == 0: no component has a neighbour), whatever the mesh looks like. */
size_t vlsat_segment_mesh_scratch_bytes(int64_t n_verts, int64_t n_edges);
int vlsat_segment_mesh(const float* normals, const int32_t* edges, int64_t n_verts, int64_t n_edges, float max_weight, int32_t min_verts,
                       void* scratch, int32_t* labels /* [V] */, int32_t* n_segments /* [1] */, int32_t* seg_size /* [V] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_SEGMENT_H */
