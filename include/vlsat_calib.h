/*
 * vlsat_calib.h -- the part of libvlsat_hip.so's C ABI that histograms a batch's scores against ground truth, for choosing the decode's
 * per-predicate thresholds and for judging the calibration of the object head (csrc/calibration.hip).  Conventions, error codes and
 * vlsat_last_error() are those of vlsat.h; the symbols are exported from the same library and bound by lib.py from its registry row
 * HEADERS["calib"].
 *
 * Why.  vlsat_graph_decode_counts gives the tp / fp / fn of the decode at ONE threshold vector, so a sweep over thresholds costs one
 * pass over the validation set per candidate.  A histogram of the predicate scores, split by ground truth, over a power-of-two number
 * of bins holds the counts of EVERY threshold k / bins at once, and exactly: for fp32 p >= 0 the product p * bins is exact, so
 * floor(p * bins) >= k if and only if p >= k / bins, which is the decode's own comparison (equality passes).
 * metrics.score_histograms_host restates the rule in PyTorch; evaluate.operating_points derives the curves on the host.
 *
 * The call takes device pointers, is asynchronous on `stream` (no host synchronisation, no allocation, no scratch, no runtime fill),
 * returns 0 or a negative VLSAT_E* code and sets vlsat_last_error; every limit is checked before anything is launched.  Integer
 * vector atomics only: the tables are ADDED to (zero them once), do not depend on scheduling, and may be added to from several streams.
 */
#ifndef VLSAT_CALIB_H
#define VLSAT_CALIB_H

#include "vlsat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------- the bin rule --------
 *
 * bins: a power of two in 16..4096.  A table row has bins + 1 columns.
 *   column(p, eligible) = min(bins - 1, (int)floor(p * bins))   when the cell is eligible and p >= 0 (fp32 compare: -0 passes);
 *                         p * bins is ONE fp32 multiply, exact because bins is a power of two; +inf and every p > 1 land in bins - 1;
 *                       = bins, the "never asserted" column, for every other cell: NaN, p < 0, not eligible.
 *   (csrc/calib_core.h holds the function, for the kernels and for a host program alike.)
 *
 * Inputs as vlsat_graph_decode_counts: obj_probs f32 [N, C]; rel_probs f32 [E, R] predicate probabilities (already exponentiated for
 *   a single-label model); gt_class int64 [N]; gt_rel int64 multi-hot [E, R] (multi_label = 1) or int64 [E], 0 = none (multi_label = 0).
 *   hot(e, r): gt_rel[e, r] == 1 (multi-label) | r != 0 and gt_rel[e] == r (single label) -- the ground truth of the decode counts.
 *   eligible(e, r): multi-label: always.  Single label: r is the lowest index of the row maximum of rel_probs[e, :] and r != 0 -- the
 *   one predicate the decode can assert for the edge.
 *
 * The three tables, int64, each may be NULL (skipped; the others are unchanged by that):
 *   rel_table [R, 2, bins + 1]   rel_table[r, hot(e, r), column(rel_probs[e, r], eligible(e, r))] += 1 for every edge e and predicate r:
 *                                E * R cells in all.
 *   obj_table [2, bins + 1]      per node n with a valid class: top1 = the lowest index of the row maximum of obj_probs[n, :];
 *                                obj_table[top1 == gt_class[n], column(obj_probs[n, top1], eligible)] += 1.
 *   confusion [C, C]             confusion[gt_class[n], top1] += 1.
 *   A node whose gt_class is outside [0, C) is counted in NEITHER node table (vlsat_graph_decode_counts counts it as a node that is wrong).
 *
 * Derived counts.  At threshold k / bins, k in 0..bins - 1, the decode asserts exactly the cells in columns k..bins - 1, so
 *   tp(r, k) = sum over b in k..bins - 1 of rel_table[r, 1, b]
 *   fp(r, k) = sum over b in k..bins - 1 of rel_table[r, 0, b]
 *   fn(r, k) = (sum over ALL bins + 1 columns of rel_table[r, 1, :]) - tp(r, k)
 * equal the tp / fp / fn of vlsat_graph_decode_counts with thresholds[r] = k / bins, bit for bit.
 *
 * Limits: R 1..32, C 1..1024, N >= 0, E <= 2^26, E * R < 2^31; anything else is VLSAT_EINVAL.  N = 0 / E = 0 (or the tables of that
 *   side NULL) launch nothing for that side. */
int vlsat_score_hist(const float* obj_probs, const float* rel_probs, const int64_t* gt_class, const int64_t* gt_rel, int32_t n_nodes,
                     int32_t n_edges, int32_t n_obj_class, int32_t n_rel_class, int32_t multi_label, int32_t bins,
                     int64_t* rel_table /* [R, 2, bins + 1] or NULL */, int64_t* obj_table /* [2, bins + 1] or NULL */,
                     int64_t* confusion /* [C, C] or NULL */, void* stream);

/* How the edge kernel cuts its work, for tests that want sizes on either side of a boundary: a block takes *edges_per_iteration edges
 * per step of its loop, and all blocks of one predicate group together cover *edges_per_sweep edges before any of them takes a second
 * step.  Both are 0 for arguments out of range. */
void vlsat_score_hist_geometry(int32_t n_rel_class, int32_t bins, int32_t* edges_per_iteration, int32_t* edges_per_sweep);

#ifdef __cplusplus
}
#endif

#endif /* VLSAT_CALIB_H */
