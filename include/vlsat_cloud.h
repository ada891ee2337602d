/*
 * vlsat_cloud.h -- the part of libvlsat_hip.so's C ABI that takes a point cloud WITHOUT faces to the segmenter (csrc/cloud.hip, and
 * vlsat_segment_cloud in csrc/mesh_segment.hip): the K nearest neighbours of every point, a normal and a flatness measure per point
 * from that neighbourhood, and the rules of vlsat_segment.h run over the neighbour table.  Conventions, error codes and
 * vlsat_last_error() are those of vlsat.h; the symbols are exported from the same library and bound by lib.py from its registry row
 * HEADERS["cloud"].
 *
 * Why.  vlsat_segment_mesh reads mesh edges and vertex normals, both of which come from triangles.  A fused RGB-D or LiDAR cloud, or a
 * reconstruction saved without its face element, has neither.  prep.knn_points_host and prep.cloud_normals_host restate the rules below
 * in numpy with the same operations in the same order: every output is equal bit for bit.
 *
 * Every call takes device pointers, is asynchronous on `stream` (no host synchronisation, no allocation), returns 0 or a negative
 * VLSAT_E* code and sets vlsat_last_error; every limit is checked before anything is launched.  Integer vector atomics and plain
 * stores only; no cooperative launch and no spin-wait.  No result depends on scheduling.
 */
#ifndef VLSAT_CLOUD_H
#define VLSAT_CLOUD_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------- neighbours --------
 *
 * Inputs: points f32 [V,3], 1 <= V <= 2^24; 1 <= K <= 32; max_sq_dist f32 >= 0, not NaN -- a SQUARED distance, as in
 *   vlsat_nearest_points.  A point is valid when its three coordinates are finite.
 * For a valid point i a candidate is every valid j != i with d2 <= max_sq_dist, d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) in fp32
 *   with dx = fl(xi - xj), every operation rounded on its own: the d2 of vlsat_nearest_points.  Coincident points are candidates of each
 *   other.  The neighbours of i are the K smallest keys (uint64(bits(d2)) << 32) | j, ascending: nearest first, ties to the lower index.
 * Outputs: nbr int32 [V,K] padded with -1; nbr_sqdist f32 [V,K] padded with +inf; nbr_count int32 [V].  An invalid point has count 0
 *   and is nobody's neighbour.  Every entry of every output is written by the call.
 * The search runs over the uniform grid vlsat_nearest_points builds (cell edge >= sqrt(max_sq_dist) (1 + 2^-6), the 27 cells around a
 *   point); the order of points inside a cell varies from run to run, the K smallest keys of a set do not.  Cost grows with the number
 *   of points within a cell edge of each point: choose max_sq_dist for the sampling density, not for the room.
 * scratch: vlsat_cloud_knn_scratch_bytes(V, K) bytes (the grid's: 20 per point and 16 MiB for the cells; 0 = arguments out of range),
 *   16-byte aligned.  The call enqueues 9 launches. */
size_t vlsat_cloud_knn_scratch_bytes(int64_t n_points, int32_t k);
int vlsat_cloud_knn(const float* points, int64_t n_points, int32_t k, float max_sq_dist, void* scratch, int32_t* nbr /* [V,K] */,
                    float* nbr_sqdist /* [V,K] */, int32_t* nbr_count /* [V] */, void* stream);

/* -------- normal and flatness --------
 *
 * Inputs: points as above; nbr, nbr_count as vlsat_cloud_knn wrote them (any table will do: a count is clamped to [0, K] and an entry
 *   outside [0, V) is no member); min_points >= 3; a viewpoint (vx, vy, vz), not NaN, used when use_viewpoint != 0.
 * Everything is fp64, every product, sum, difference, quotient and square root rounded on its own (IEEE, to nearest even).
 *   1. The members of point i are the point itself and then its neighbours in list order; n is their number.
 *   2. With n < min_points there is no estimate: normal (0, 0, 0), curvature 1.0.
 *   3. Centroid: the left-fold sum of the members, divided by n.
 *   4. Covariance (not divided by n): a_xx, a_xy, a_xz, a_yy, a_yz, a_zz are left-fold sums, from 0, of the products of the members'
 *      differences to the centroid.  A trace fl(fl(a_xx + a_yy) + a_zz) that is not > 0 (coincident members, or a NaN): no estimate.
 *   5. Six cyclic Jacobi sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index, V = I at the start.  A pair whose a_pq
 *      is exactly 0 is skipped.  Otherwise theta = (a_qq - a_pp) / (2 a_pq); t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with
 *      sgn(+-0) = +1; c = 1 / sqrt(t^2 + 1); s = t c; then a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0,
 *      (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq), and for every row k of V (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq).
 *      Six is not a guess: on the neighbourhoods of a 3 x 3 m room with three boxes sampled at 0.1 (radius 0.15, K = 12) the largest
 *      relative off-diagonal norm sqrt(2 sum a_pq^2) / |A|_F after 2 / 3 / 4 / 5 sweeps was 1.2e-2 / 1.3e-8 / 1.3e-33 / 1.7e-139,
 *      measured in fp64 on the host: convergence is quadratic and the fifth sweep is already beyond fp64; the sixth is margin.
 *   6. The normal is the column of V of the smallest diagonal entry, ties to the lower index.  It is not renormalised: V is orthonormal
 *      to rounding.  curvature = max(lambda_min, 0) / fl(fl(l0 + l1) + l2): the surface variation, in [0, 1/3].
 *   7. Sign.  With a viewpoint: d = fl(fl(nx tx + ny ty) + nz tz), t = viewpoint - point; d < 0 flips the normal, d > 0 keeps it.
 *      Without one, or when d is neither: the component of largest magnitude is made positive, ties to the lower axis.
 * Outputs, rounded to fp32: normals [V,3], curvature [V].  Every entry is written.  No scratch; one launch.
 * Bit equality with a host restatement rests on fp64 division and square root being correctly rounded on the device, which the
 * gfx950 code generator's IEEE expansions of both are; tests/test_hip_cloud.py compares every bit. */
int vlsat_cloud_normals(const float* points, const int32_t* nbr, const int32_t* nbr_count, int64_t n_points, int32_t k, int32_t min_points,
                        int32_t use_viewpoint, double vx, double vy, double vz, float* normals /* [V,3] */, float* curvature /* [V] */,
                        void* stream);

/* -------- segments of a cloud --------
 *
 * Rules 2-5 of vlsat_segment.h apply unchanged over the pairs (e / K, nbr[e]) for e < V K, each standing for both of its directions
 * as a mesh edge does.  A -1 entry is an ignored edge, as an end outside [0, V) or a == b already is.
 * Weight: unsigned_dot == 0 uses rule 1 of vlsat_segment.h.  unsigned_dot != 0 is for normals whose sign means nothing (a PCA normal
 *   without a viewpoint): w = fl(1 - |d|) clamped to [0, 2], d as in rule 1; a NaN d gives 2.
 * A zero normal weighs exactly 1 against everyone under both weights: such a point links to nobody (max_weight < 1) and is absorbed
 *   by rule 3.  prep / scan.segment_cloud use that to keep crease points (curvature above a bound) from chaining two faces together.
 * Outputs as vlsat_segment_mesh.  scratch: vlsat_segment_mesh_scratch_bytes(V, V K) bytes.  8 + 4 R launches. */
int vlsat_segment_cloud(const float* normals, const int32_t* nbr, int64_t n_points, int32_t k, float max_weight, int32_t min_verts,
                        int32_t unsigned_dot, void* scratch, int32_t* labels /* [V] */, int32_t* n_segments /* [1] */,
                        int32_t* seg_size /* [V] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_CLOUD_H */
