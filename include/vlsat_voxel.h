/*
 * vlsat_voxel.h -- the part of libvlsat_hip.so's C ABI that resamples a point cloud on a voxel grid before it is segmented
 * (csrc/voxel.hip): one representative point per occupied cell, and a map from every input point to its cell's representative.
 * Conventions, error codes and vlsat_last_error() are those of vlsat.h; the symbols are exported from the same library and bound by
 * lib.py from its registry row HEADERS["voxel"].
 *
 * Why.  vlsat_cloud_knn takes K neighbours within one radius and the segmenter counts points, which presumes ONE sampling distance.  A
 * fused RGB-D or LiDAR cloud is dense where many frames overlapped: there the K nearest neighbours lie within the sensor noise, the
 * normals are fitted to that noise and the surface shatters into segments.  A voxel grid in front evens the density out.
 * prep.voxel_downsample_host restates the rule below in numpy: every output is equal bit for bit.
 *
 * Every call takes device pointers, is asynchronous on `stream` (no host synchronisation, no allocation), returns 0 or a negative
 * VLSAT_E* code and sets vlsat_last_error; every limit is checked before anything is launched.  Integer vector atomics and plain
 * stores only; no cooperative launch, no spin-wait, every loop bounded.  No result depends on scheduling: two runs are bit-equal.
 */
#ifndef VLSAT_VOXEL_H
#define VLSAT_VOXEL_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------- the rule --------
 *
 * Inputs: points f32 [V,3], 1 <= V <= 2^24; voxel f32 > 0, finite: the edge of a cell; origin (ox, oy, oz) f32, finite: a corner of
 *   the grid.  The origin anchors the grid to the FRAME, not to the cloud's bounding box: two clouds in one frame share cells.
 *   min_count >= 1.  Optionally normals f32 [V,3] and colors u8 [V,3].
 * 1. Cell.  inv = fl(1.0f / voxel), computed once on the host in fp32; the call is refused when inv is not finite and positive.  Per
 *    axis t = floor(fl(fl(x - o) inv)), the subtraction and the product each rounded on their own in fp32.  A point is IN RANGE when on
 *    every axis |x| < 32768 and |t| < 2^20, written as comparisons a NaN fails (so a non-finite coordinate is out of range).  A point
 *    out of range belongs to no voxel.  Key: (tz + 2^20) << 42 | (ty + 2^20) << 21 | (tx + 2^20).
 * 2. Voxels.  Per distinct key: count = the number of its points, first = its lowest point index.  The voxels with count >= min_count
 *    are kept and numbered 0 .. M-1 by ascending first: the numbering follows the input order and depends on nothing else.
 *    voxel_of_point[i] is that number, or -1 for a point out of range or in a dropped voxel.
 * 3. Position.  Per coordinate q = llrint((double)x 2^24) (half to even; the product is exact), S = the sum of q over the voxel's
 *    points in int64 (|q| < 2^39, at most 2^24 points: no overflow), output (float)((double)S / (double)count 2^-24), every
 *    conversion and the quotient rounded to nearest even.  Integer sums do not depend on order: the result is exact and free of
 *    scheduling.
 * 4. Normals: the same sums with the scale 2^20; a component that is not finite or has |n| >= 32768 adds 0.  The three sums go to
 *    fp64 (x, y, z), l = sqrt(fl(fl(x x + y y) + z z)) with every operation rounded on its own, output (float)(x / l) etc., or
 *    (0, 0, 0) when l == 0 (the normals cancel, or none counted).
 * 5. Colours: per channel (2 S + count) / (2 count) in integers, S the sum of the channel: the mean, halves rounded up.
 * 6. Any other per-point integer field (an instance id) takes its value at `first`; that is a gather through first_point, left to the
 *    caller.
 *
 * -------- the calls --------
 *
 * vlsat_voxel_assign: rules 1 and 2.  Outputs: voxel_of_point int32 [V]; first_point int32 [V] and voxel_count int32 [V], of which the
 *   first M entries are written; n_voxels int32 [2]: M, and an error flag that is 0 unless the hash table overflowed (it holds 2 V
 *   slots or more for at most V keys, so it cannot: the flag is what keeps the probe loop bounded -- it ends after `slots` steps and
 *   the point is then treated as out of range).  The caller reads both after the stream has drained.
 *   Launches: clear, insert (an open-addressing table: the key claimed by a 64-bit compare-and-swap from the all-ones empty value,
 *   linear probing, first by atomic min, count by atomic add; which slot a key lands in varies from run to run and reaches no
 *   output), count / scan / apply of the head flags (point i is a head when first == i and count >= min_count; a plain three-launch
 *   exclusive scan in index order), and one pass that gives every point the number of its head: 6 launches.
 * vlsat_voxel_reduce: rules 3 to 5 for the M = n_voxels voxels vlsat_voxel_assign found, from its voxel_of_point and voxel_count
 *   (an entry of voxel_of_point outside [0, M) is no member; a count below 1 is read as 1).  normals / colors may be null, and
 *   then so may out_normals / out_colors.  Outputs: out_points f32 [M,3], out_normals f32 [M,3], out_colors u8 [M,3].  n_voxels == 0:
 *   nothing is launched.  Launches: zero the sums, accumulate (64-bit integer atomic adds per coordinate, 32-bit for a colour
 *   channel; neighbouring lanes of a wave that hold the same voxel are summed first, which changes no integer sum), finalise (one thread per voxel): 3 launches.
 * scratch: vlsat_voxel_scratch_bytes(V) bytes for both calls, the same block, 256-byte aligned: 16 bytes per table slot (the least
 *   power of two >= 2 V of them), 8 bytes per point for the slot and head maps, 60 bytes per point for the sums.  0 = V out of range. */
size_t vlsat_voxel_scratch_bytes(int64_t n_points);
int vlsat_voxel_assign(const float* points, int64_t n_points, float voxel, float ox, float oy, float oz, int32_t min_count, void* scratch,
                       int32_t* voxel_of_point /* [V] */, int32_t* first_point /* [V] */, int32_t* voxel_count /* [V] */,
                       int32_t* n_voxels /* [2] */, void* stream);
int vlsat_voxel_reduce(const float* points, const float* normals /* or null */, const uint8_t* colors /* or null */,
                       const int32_t* voxel_of_point, const int32_t* voxel_count, int64_t n_points, int64_t n_voxels, void* scratch,
                       float* out_points /* [M,3] */, float* out_normals /* [M,3] or null */, uint8_t* out_colors /* [M,3] or null */,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_VOXEL_H */
