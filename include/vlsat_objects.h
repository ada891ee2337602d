/*
 * vlsat_objects.h -- the part of libvlsat_hip.so's C ABI that takes a point cloud to OBJECT-level instances without a trained model
 * (csrc/objects.hip): the room's structural planes (floor, walls, ceiling) are found and removed, and what is left is clustered by
 * Euclidean proximity over the neighbour table of vlsat_cloud_knn.  Conventions, error codes and vlsat_last_error() are those of
 * vlsat.h; the symbols are exported from the same library and bound by lib.py from its registry row HEADERS["objects"].
 *
 * Why.  vlsat_segment_mesh and vlsat_segment_cloud over-segment: a table top and each of its sides are separate segments, and the only
 * way back to objects is merging along "same part" edges, a relation the 26-name list of the published checkpoints does not have.
 * prep.cloud_planes_host and prep.cloud_clusters_host restate the rules below in numpy with the same operations in the same order:
 * every output is an integer count or a value with one stated rounding, and is equal bit for bit.
 *
 * Every call takes device pointers, is asynchronous on `stream` (no host synchronisation, no allocation), returns 0 or a negative
 * VLSAT_E* code and sets vlsat_last_error; every limit is checked before anything is launched.  Integer vector atomics and plain
 * stores only; no cooperative launch, no spin-wait, no float atomics, no loop whose length depends on the data beyond the stated
 * bounds.  No result depends on scheduling: two runs are bit-equal.
 */
#ifndef VLSAT_OBJECTS_H
#define VLSAT_OBJECTS_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------- structural planes --------
 *
 * Inputs: points f32 [V,3], 3 <= V <= 2^24; n_hyp H in 1 .. 4096; max_planes P in 1 .. 32; dist f32 > 0 and finite; min_inliers >= 3;
 *   outside_ppm in 0 .. 500000; seed u64.  A point is valid when its three coordinates are finite.  At the start alive = valid.
 * For round r = 0 .. P-1:
 *   1. The alive list is the alive points in ascending index, n its length.  n < 3: stop.
 *   2. Hypothesis h (0 <= h < H) takes the alive points of ranks draw((r H + h) 3 + j, n), j = 0, 1, 2: points a, b, c.  draw(k, n) is
 *      the generator of vlsat_sample_objects and vlsat_split_seeds: x = seed + 0x9E3779B97F4A7C15 (k + 1) mod 2^64, z = the splitmix64
 *      finaliser of x, draw = ((z >> 32) n) >> 32.
 *   3. The plane, in fp64, every difference, product, sum, quotient and square root rounded on its own (IEEE, to nearest even):
 *      u = b - a, v = c - a, m = u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), l2 = fl(fl(mx mx + my my) + mz mz).  The
 *      hypothesis is VOID unless l2 > 0 and finite (repeated draws and collinear triples fall out here).  n = m / sqrt(l2), each
 *      component divided; the component of largest magnitude is made positive, ties to the lower axis (rule 7 of vlsat_cloud.h without
 *      a viewpoint); d = -fl(fl(nx ax + ny ay) + nz az).  (nx, ny, nz, d) are then rounded to fp32.
 *   4. The score of every alive point, in fp32, every operation rounded on its own: s = fl(fl(fl(fl(nx x) + fl(ny y)) + fl(nz z)) + d).
 *      inlier: |s| <= dist; above: s > dist; below: the rest -- a NaN s counts as below.  The three counts are int32.
 *   5. A hypothesis that is not void is ELIGIBLE when inliers >= min_inliers and min(above, below) <= (int64(n) outside_ppm) / 1000000
 *      (integer division).  The second condition is what makes a plane structural: almost the whole remaining cloud lies on one side
 *      of a floor or a wall, which is not true of a table top.
 *   6. The winner is the eligible hypothesis of the largest key (inliers << 32) | (0xFFFFFFFF - h): most inliers, ties to the lower
 *      h.  Nothing eligible: stop.  Otherwise the winner's inliers get plane_id = r + 1 and die, and row r of planes and of
 *      plane_counts is written.  There is no refit: the stated plane is exactly the one that was scored.
 * Outputs: plane_id int32 [V] (0 = no plane; an invalid point is never alive and has 0); planes f32 [P,4] = (nx, ny, nz, d) and
 *   plane_counts int32 [P,3] = (inliers, above, below) per found plane, unused rows zero; n_planes int32 [1].  Every entry of every
 *   output is written by the call.
 * Launches: one that clears the outputs and marks the valid points, then per round seven: alive points per block of 256, the scan of
 *   those counts (one block), the scatter into the alive list, the H planes (one thread each; it also clears the counts), the score
 *   (below), the choice of the winner (one block) and the death of its inliers.  All P rounds are enqueued; a flag in device memory
 *   turns the kernels of the rounds after a stop into immediate returns (the idiom of vlsat_split_seeds).  The only host wait is the
 *   caller's read of n_planes.
 * The score is the hot path, V x H evaluations per round: a block of 256 threads keeps one, two or four hypotheses per thread in
 *   registers, with two private integer counters each; the block streams tiles of its share of the alive list through LDS and every
 *   lane reads the same point (a broadcast, free of bank conflicts); there is no cross-lane operation in the inner loop and one integer
 *   atomicAdd per block, hypothesis and counter at the end.  Integer sums: the counts do not depend on the order.
 * scratch: vlsat_cloud_planes_scratch_bytes(V, H) bytes (8 per point, 4 per block of 256 points, 28 per hypothesis; 0 = arguments
 *   out of range), 256-byte aligned. */
size_t vlsat_cloud_planes_scratch_bytes(int64_t n_points, int32_t n_hyp);
int vlsat_cloud_planes(const float* points, int64_t n_points, int32_t n_hyp, int32_t max_planes, float dist, int32_t min_inliers,
                       int32_t outside_ppm, uint64_t seed, void* scratch, int32_t* plane_id /* [V] */, float* planes /* [P,4] */,
                       int32_t* plane_counts /* [P,3] */, int32_t* n_planes /* [1] */, void* stream);

/* -------- clusters --------
 *
 * Inputs: nbr int32 [V,K] and nbr_sqdist f32 [V,K] as vlsat_cloud_knn wrote them (any table will do), 1 <= V <= 2^24, 1 <= K <= 32;
 *   mask int32 [V], a non-zero entry means the point is eligible; max_sq_dist f32, not NaN -- a SQUARED distance; min_points >= 1.
 * Edges: the pairs (i, nbr[i][k]) with both ends eligible, the entry inside [0, V) and not i, and nbr_sqdist[i][k] <= max_sq_dist.
 *   Each pair stands for both directions.  The eligible points fall into connected components; the root of one is its lowest point.  A
 *   component of fewer than min_points points gets 0, the rest are numbered 1 .. S by lowest point.  A point that is not eligible
 *   gets 0 and belongs to no component.
 * Outputs: labels int32 [V]; n_clusters int32 [1]; cluster_size int32 [V], entries 0 .. S-1 hold the sizes of clusters 1 .. S, the
 *   rest are 0.  Every entry is written.
 * Launches: init, link (one thread per table entry; the lock-free union-find of the segmenter), roots and sizes, kept roots per block
 *   of 256, the scan of those counts, numbering, labels: 7.
 * scratch: vlsat_cloud_clusters_scratch_bytes(V) bytes (16 per point, 4 per block of 256; 0 = out of range), 256-byte aligned. */
size_t vlsat_cloud_clusters_scratch_bytes(int64_t n_points);
int vlsat_cloud_clusters(const int32_t* nbr, const float* nbr_sqdist, const int32_t* mask, int64_t n_points, int32_t k, float max_sq_dist,
                         int32_t min_points, void* scratch, int32_t* labels /* [V] */, int32_t* n_clusters /* [1] */,
                         int32_t* cluster_size /* [V] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_OBJECTS_H */
