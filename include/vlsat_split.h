/*
 * vlsat_split.h -- the part of libvlsat_hip.so's C ABI that splits a scan into sub-scenes and fuses the per-split predictions back
 * into one graph per scan (csrc/scene_split.hip).  Conventions, error codes and vlsat_last_error() are those of vlsat.h; the symbols
 * are exported from the same library and bound by lib.py from its registry row HEADERS["split"].
 *
 * Why.  The reference trains and evaluates on SUB-SCENES: every entry of relationships_*.json is scan + "_" + split
 * (src/dataset/dataset_3dssg.py:238-240), and a split is the group of segments its generate_groups collects around a seed point
 * (data_processing/gen_data.py:56-183; the BBOX method :108-122 is the one stated here).  prep.split_seeds_host,
 * prep.split_groups_host and metrics.fuse_splits_host restate the three rules in numpy with the same operations: every index, mask,
 * count and every bit of the pooled probabilities is equal.
 *
 * All calls take device pointers, are asynchronous on `stream` (no host synchronisation, no allocation, no runtime fill), return 0
 * or a negative VLSAT_E* code and set vlsat_last_error.  Integer vector atomics and plain stores only; no cooperative launch, no
 * barrier and no spin-wait between blocks -- a launch boundary is the only cross-block ordering.  No result depends on scheduling.
 */
#ifndef VLSAT_SPLIT_H
#define VLSAT_SPLIT_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------- seeds (gen_data.py:69-85) --------
 *
 * points f32 [V,3], V >= 1.  distance > 0 (reference default 1.0); D2 = distance * distance in fp64.
 *   draw(k, n) = the counter-based generator of vlsat_sample_objects: x = seed + 0x9E3779B97F4A7C15 (k + 1) mod 2^64, the splitmix64
 *     finaliser of x, its top 32 bits scaled to n: ((z >> 32) * n) >> 32.  It is NOT numpy's stream.  With ranks (int64 [n_ranks])
 *     draw(k, n) = ranks[k]: a recorded run of the reference replays exactly.
 *   Seed 0 is the vertex at index draw(0, V), whatever its coordinates.
 *   dmin2[v] = the minimum over the seeds so far of dx*dx + dy*dy, dx = (double)x_v - (double)x_seed ..., in fp64, every operation
 *     rounded on its own (no fused multiply-add); z is ignored.  The reference compares sqrt(...) > distance on the same fp64 values;
 *     the squared form differs from it only within an ulp of the threshold.
 *   selectable = the v with dmin2[v] > D2 (strict, fp64), in ascending index order.  A vertex with a non-finite coordinate (x, y or z) is
 *     never selectable: its dmin2 is NaN and the comparison is false, as numpy's is.  (When seed 0 is a vertex with a non-finite x or y,
 *     every distance is NaN and it stays the only seed.)
 *   While selectable is not empty, seed k = selectable[draw(k, len(selectable))], k = 1, 2, ...
 * seeds int32 [max_seeds] receives the K seed indices in creation order (entries past K are not written).
 * state int32 [4] = {K, status, done, last seed}.  status: 0 complete; 1 a rank was negative or >= n; 2 the ranks ran out while vertices
 *   were still selectable; 3 max_seeds was reached while vertices were still selectable.  done = 1 in every one of these cases.
 * max_seeds (1..65536) is the caller's bound on K: two seeds are more than `distance` apart, so a cell of side distance / sqrt(2) of
 *   the xy bounding box holds at most one (prep.split_seed_cap).  The call enqueues one init launch and max_seeds x (update, pick):
 *   update refreshes dmin2 against the newest seed and writes per-block counts of selectable vertices; pick (one block) scans the
 *   counts, takes the rank, locates the vertex and appends it.  When nothing is selectable, pick sets `done` in device memory and every
 *   later launch returns at once.  The caller reads `state` back once; nothing is read back per seed.
 * scratch: vlsat_split_seeds_scratch_bytes(V) bytes (8 per vertex + 4 per 1024 vertices; 0 = V out of range), 16-byte aligned. */
size_t vlsat_split_seeds_scratch_bytes(int64_t n_points);
int vlsat_split_seeds(const float* points, int64_t n_points, double distance, uint64_t seed, const int64_t* ranks /* or NULL */,
                      int64_t n_ranks, int32_t max_seeds, void* scratch, int32_t* seeds /* [max_seeds] */, int32_t* state /* [4] */,
                      void* stream);

/* -------- groups (gen_data.py:109-122) --------
 *
 * points f32 [V,3]; segments int32 [V] (segment id per vertex); segment_ids int32 [S], distinct, each in [0, map_size): slot s is
 *   segment_ids[s] (id_map: int32 [map_size] scratch, as in vlsat_instance_boxes; vertices of other ids are ignored); seeds int32 [K]
 *   vertex indices; bbox_distance (reference default 0.75); min_seg_per_group (5).
 *   lo = (double)p - bbox_distance, hi = (double)p + bbox_distance per axis, p the seed's vertex (one fp64 operation each).
 *   Group k holds slot s iff some vertex of segment s lies strictly inside the box on all three axes: lo < (double)v < hi, fp64.
 *     A vertex on a face is outside; a non-finite vertex is in no box; a seed with a non-finite coordinate has an empty group.
 *   The reference takes np.unique of the filtered labels, so segment id 0 (unlabelled / background) counts like any other id when the
 *     caller lists it in segment_ids -- scan.split_scan lists it; prepare_scan later ignores ids without a label.
 * mask uint32 [K, W], W = ceil(S / 32): bit (s & 31) of word s >> 5 of row k.  counts int32 [K] = set bits of the row;
 *   keep int32 [K] = counts >= min_seg_per_group (the reference drops the smaller groups).  Every word is written by the call. */
int vlsat_split_groups(const float* points, const int32_t* segments, int64_t n_points, const int32_t* segment_ids, int32_t n_seg,
                       int32_t* id_map, int32_t map_size, const int32_t* seeds, int32_t n_seeds, double bbox_distance,
                       int32_t min_seg_per_group, uint32_t* mask /* [K, W] */, int32_t* counts /* [K] */, int32_t* keep /* [K] */,
                       void* stream);

/* -------- fusion: the rows of a batch of splits folded into one graph per scan --------
 *
 * Inputs: obj_probs f32 [N,C]; rel_probs f32 [E,R], finite and non-negative (no -0); edges int64 [E,2] row pairs in any order;
 *   row_instance int32 [N], the scan-level instance id of each row; weights f32 [N], positive, or NULL (all 1).
 * Objects = the distinct ids in [0, map_size), ascending: object m is the m-th smallest id, obj_ids[m] that id.  A row whose id lies
 *   outside [0, map_size) belongs to no object (root = object = -1) and its edges are dropped.  root[n] = the lowest row with n's id;
 *   object[n] = m.  n_objects[0] = totals[0] = M; totals[1] = E'; obj_batch_ids[m] = 0 (one scan per call).
 * Members: member_ptr int32 [N+1], members int32 [N]: CSR, the rows of object m in ascending row order (member_ptr[o] = the number of
 *   rows with an object for o > M).
 * Pooled probabilities: over the rows i of m in ascending row order, from 0:  s = fl(s + fl(w_i * p_ic)),  W = fl(W + w_i),
 *   fused_probs[m,c] = fl(s / W) -- fp32, every operation rounded on its own.  obj_weight[m] = W.
 * Pairs: an edge (ra, rb) with both rows in range and object[ra] = a != b = object[rb] (both >= 0) folds onto the ordered pair (a, b);
 *   a self pair (a == b: a self loop, or two rows of one instance) and an out-of-range index are dropped (edge_to_pair = -1).  Pairs
 *   are numbered by (a, b) ascending.  edge_to_pair int32 [E]; pair_edges int64 [E,2] = (a, b); pair_count int32 [E] = occurrences
 *   folded, whatever split they come from; pair_probs f32 [E,R] = the maximum over the occurrences (exact: a maximum has no order).
 * Rows past M / E' hold zero; index tables (members past the end, obj_batch_ids, obj_ids, pair_edges) hold -1.  Every field of every
 *   output is written by the call.  The outputs have the layout of vlsat_merge_segments, plus obj_ids int32 [N].
 * Limits: N <= 16384 (the pair table is N x N bits), C 1..1024, R 1..32, E <= 2^26, E * R < 2^31, N * C < 2^31, map_size 1..2^24; anything
 *   else is VLSAT_EINVAL.  scratch: vlsat_fuse_splits_scratch_bytes(...) bytes (0 = arguments out of range), 16-byte aligned. */
size_t vlsat_fuse_splits_scratch_bytes(int64_t n_rows, int64_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t map_size);
int vlsat_fuse_splits(const float* obj_probs, const float* rel_probs, const int64_t* edges, const int32_t* row_instance, const float* weights,
                      int32_t n_rows, int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t map_size, void* scratch,
                      int32_t* root /* [N] */, int32_t* object /* [N] */, int32_t* n_objects /* [1] */, int32_t* totals /* [2] */,
                      int32_t* member_ptr /* [N+1] */, int32_t* members /* [N] */, float* fused_probs /* [N,C] */, float* obj_weight /* [N] */,
                      int64_t* obj_batch_ids /* [N] */, int32_t* edge_to_pair /* [E] */, int64_t* pair_edges /* [E,2] */,
                      int32_t* pair_count /* [E] */, float* pair_probs /* [E,R] */, int32_t* obj_ids /* [N] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_SPLIT_H */
