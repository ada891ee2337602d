/*
 * vlsat_convex.h -- the part of libvlsat_hip.so's C ABI that clusters a point cloud by LOCAL CONVEXITY (csrc/convex.hip): bodies that
 * touch are cut where their surfaces meet in a concave junction.  Conventions, error codes and vlsat_last_error() are those of vlsat.h;
 * the symbols are exported from the same library and bound by lib.py from its registry row HEADERS["convex"].
 *
 * Why.  vlsat_cloud_clusters (vlsat_objects.h) joins whatever touches: with floor and walls removed, a desk and all it carries are one
 * cluster.  The surfaces of one body meet in convex creases, and two bodies resting on each other meet in a concave one (Stein et al.,
 * "Object Partitioning using Local Convexity", CVPR 2014).  Cutting only the concave table entries does not separate them when the
 * normals are estimated: fitted normals turn gradually across a junction, and some short entry always passes the tolerance.  So the
 * points that show concave evidence are ERODED, the rest is clustered, and the eroded points are handed back to the nearest cluster.
 * prep.convex_clusters_host restates the rule below in numpy with the same operations in the same order; every output is an integer and
 * is equal bit for bit.
 *
 * The call takes device pointers, is asynchronous on `stream` (no host synchronisation, no allocation), returns 0 or a negative
 * VLSAT_E* code and sets vlsat_last_error; every limit is checked before anything is launched and a refused call leaves the outputs
 * untouched.  Integer vector atomics and plain stores only; no cooperative launch, no spin-wait, no float atomics.  No result depends
 * on scheduling: two runs are bit-equal.
 */
#ifndef VLSAT_CONVEX_H
#define VLSAT_CONVEX_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Inputs: points f32 [V,3] and normals f32 [V,3]; nbr int32 [V,K] and nbr_sqdist f32 [V,K] as vlsat_cloud_knn wrote them (any table
 *   will do); mask int32 [V]; 1 <= V <= 2^24, 1 <= K <= 32; link_sq_dist f32, not NaN -- a SQUARED distance; concavity tau f32 in
 *   [0, 1], the sine of the tolerated concave angle; min_points >= 1; 0 <= absorb_rounds <= 64; no null pointer.  Anything else:
 *   VLSAT_EINVAL before any launch.  Every fp32 operation below is rounded on its own (IEEE, to nearest even).
 *   1. A point is ELIGIBLE when its mask is non-zero and its three coordinates are finite.  It is ORIENTED when it is eligible and its
 *      normal is finite and not (0, 0, 0) (a -0 is a 0).  Normals are taken as given: turning them to one side, and unit length, are
 *      the caller's business.
 *   2. Evidence.  Table entry (i, k) with j = nbr[i][k] COUNTS when j is in [0, V), j != i, both ends are oriented, and
 *      q = nbr_sqdist[i][k] is finite and >= 0 -- whatever the link distance is.  d = x_j - x_i per component,
 *      a = fl(fl(fl(n_ix dx) + fl(n_iy dy)) + fl(n_iz dz)), b the same with n_j, c = fl(a - b).  The entry is CONCAVE when c > 0 and
 *      fl(c c) > fl(fl(tau tau) q); a NaN fails both comparisons and is not concave.  A concave entry marks BOTH its ends as boundary.
 *      c is the same bit pattern seen from either end: from j every difference, product and sum changes its sign and nothing else,
 *      a and b change places, and fl(-b - -a) = fl(a - b).  Only a c that is zero may differ, in its sign (x + -x is +0 from both
 *      ends), which no comparison sees; so an entry and its mirror (j, i) at the same q are concave together.  (For unit normals
 *      c / |d| is the difference of the cosines of the two normals against the line that joins the points: positive when the
 *      surfaces open towards each other.)
 *   3. Core and links.  A point is CORE when it is oriented and not boundary.  The entries that name another point inside [0, V) with
 *      both ends core and q <= link_sq_dist are links; each stands for both directions.  The cores fall into connected components;
 *      the root of one is its lowest point.  A component of fewer than min_points core points is DISSOLVED.
 *   4. Boundary points, eligible points without a usable normal and the points of dissolved components are UNLABELLED; the cores of a
 *      kept component carry its root as their label.
 *   5. Absorption.  For round r = 1 .. absorb_rounds every unlabelled eligible point looks along its row in table order (nearest
 *      first) and takes the label of the first entry that is inside [0, V), not the point itself, and carried a label at the END of
 *      round r - 1 (round 0: rule 4).  All points update at once: two label buffers.  A point with no such entry keeps waiting.  What
 *      is still unlabelled after the last round gets 0.
 *   6. The kept roots are numbered 1 .. S by lowest point.  cluster_size[0 .. S-1] counts ALL final members of clusters 1 .. S, the
 *      absorbed ones included; the rest are 0.
 *   7. state: 0 not eligible, 1 core of a kept component, 2 boundary, 3 eligible without a usable normal, 4 core of a dissolved
 *      component.  An absorbed point keeps its state.
 * Outputs: labels int32 [V]; n_clusters int32 [1]; cluster_size int32 [V]; state int32 [V].  Every entry of every output is written.
 * Launches, all enqueued, no host wait: init (eligible, oriented; the outputs cleared), evidence (one thread per table entry: the
 *   K lanes of a row read the same x_i and n_i, the j side is a gather of 24 bytes; boundary[i] = boundary[j] = 1 by plain stores,
 *   the same value from everybody), link (one thread per entry, in a launch of its own because it needs the evidence COMPLETE; the
 *   lock-free union-find of the segmenter), roots and sizes (one integer add per distinct root of a wave), one launch per absorption
 *   round (one thread per point, labelled points leave at once), kept roots per block of 256, the scan of those counts (one block),
 *   numbering, labels and sizes: 8 + absorb_rounds.
 * scratch: vlsat_convex_clusters_scratch_bytes(V) bytes (28 per point, 4 per block of 256; 0 = out of range), 256-byte aligned. */
size_t vlsat_convex_clusters_scratch_bytes(int64_t n_points);
int vlsat_convex_clusters(const float* points /* [V,3] */, const float* normals /* [V,3] */, const int32_t* nbr /* [V,K] */,
                          const float* nbr_sqdist /* [V,K] */, const int32_t* mask /* [V] */, int64_t n_points, int32_t k,
                          float link_sq_dist, float concavity, int32_t min_points, int32_t absorb_rounds, void* scratch,
                          int32_t* labels /* [V] */, int32_t* n_clusters /* [1] */, int32_t* cluster_size /* [V] */,
                          int32_t* state /* [V] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_CONVEX_H */
