/* hnsw_mi355x_dbscan_screen.h -- exact DBSCAN behind a two-sided matrix-core screen, an extension of hnsw_mi355x_exact_range_screen.h
 * in a header of its own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its
 * message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the
 * stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswxd_: the seven other headers keep their sets of hnswgpu_*,
 * hnswhdb_*, hnswhds_*, hnswhdp_*, hnswdbs_*, hnswxs_* and hnswxr_* symbols as they are.  The ctypes binding of these entries is
 * generated from THIS file.                                                                                                         */
#ifndef HNSW_MI355X_DBSCAN_SCREEN_H
#define HNSW_MI355X_DBSCAN_SCREEN_H

#include "hnsw_mi355x_exact_range_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hnswdbs_exact(_device) of hnsw_mi355x_dbscan.h, argument for argument, and one more: for every input that call accepts, these
 * write byte for byte what it writes -- labels, core flags, counts, anchors, the number of clusters -- and they refuse what it
 * refuses, in its words (min_samples == 0, a NaN eps, HNSWGPU_STORAGE_F16, HNSWGPU_ARITH_SIMD8, a NULL out_label or out_n_clusters);
 * a refused call writes nothing, out_stats included.  Only the cost differs: the existing call runs every (point, point) pair
 * through the f32 chain twice; these run every pair twice through the matrix cores and the chain on a thin band of pairs.
 *   screen    DistL2, DistDot, DistCosine: the inner products of (tile of stored points as queries, slab of rows) on the matrix cores
 *             in f32, each turned into the LOWER BOUND lb of hnsw_mi355x_exact_screen.h and into an UPPER BOUND ub -- never below the
 *             f32 distance the exact arithmetic gives for the pair, proved in the same range of norms from the same error term.
 *             ub <= eps: the pair is a hit without the chain.  lb > eps: a miss without it.  Every other pair -- lb <= eps < ub, or
 *             a pair outside the proved range, which has no upper bound -- is undecided.
 *   count     the sure hits are counted in the screen; the undecided pairs go through the exact chain and count where v <= eps.
 *   link      core points unite over their sure hits in the screen; the chain runs on the undecided pairs with a core row, and on
 *             every pair that is no miss between a point that is NOT core and a core row: the anchor is the core row of the smallest
 *             {distance bits, position}, which needs the bits.  A point that is not core has fewer than min_samples such pairs.
 *   fallback  a call whose pairs for the chain outgrow the buffer (2 Mi pairs per chunk of 16 MB of padded points and pass) is
 *             answered by the code of hnswdbs_exact itself, whole.
 *   stats     out_stats (host memory in both forms, four words, may be NULL): [0] points answered through the screen, [1] points
 *             answered by the existing path because the buffer was outgrown, [2] points not screened at all -- a distance without
 *             a screen (DistL1, DistHellinger, DistJeffreys, DistJensenShannon), fewer than 256 points, rows too long for a tile of
 *             queries in LDS (d above 1120): the whole call then runs the existing path.  The three add up to the number of points.
 *             [3] pairs that went through the exact chain, both passes together ([1] != 0: those counted before the fallback).
 *   cost      the answers never depend on which path ran or on timing: counts are integer sums, unions a set, anchors an integer
 *             minimum.  Faster than hnswdbs_exact where the chain dominated it (100 000 x 128 DistL2); expect little or a loss on
 *             short rows (d = 25: the epilogue dominates) and on rows of more than 544 elements (one wavefront per workgroup);
 *             RESULTS.md "DBSCAN" has the figures.  A fallback costs the existing call plus the screening up to the overflow.
 *   memory    the 25 bytes a point of hnswdbs_exact, and at most 16 MB of padded points, 16 MB of candidates and the n f32 of row
 *             norms that the screened k-NN keeps with the replica, from the replica's pool.
 * Legal from several host threads at once (the handle's lock is taken shared).  The host form uploads the index on first use; the
 * device form wants a resident replica (HNSWGPU_ERR_DEVICE otherwise) and waits for `stream` before it returns.                     */
int hnswxd_exact(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* out_label, uint8_t* out_core, uint32_t* out_count,
                 uint32_t* out_anchor, uint64_t* out_n_clusters, uint64_t* out_stats);
int hnswxd_exact_device(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* d_out_label, uint8_t* d_out_core,
                        uint32_t* d_out_count, uint32_t* d_out_anchor, uint64_t* out_n_clusters, uint64_t* out_stats, void* stream);

/* Diagnostic (host buffers, DistL2 / DistDot / DistCosine, nq * n up to 2^24): out_lb[q * n + f] and out_ub[q * n + f] = the two
 * bounds the screen kernel gives (row q of queries, the point of flat id f), written by that kernel with a store epilogue.  Outside
 * the proved range lb is +0 and ub is +inf.  The band between the two is what the exact chain sees: an unsound bound would hide until
 * a distance sits at eps, this makes it testable directly.                                                                         */
int hnswxd_bounds_matrix(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, float* out_lb, float* out_ub);

/* Out of scope: using dist(i, j) = dist(j, i) to halve the tiles; F16 storage; filters; the four distances without a screen; the CSR
 * forms.  Hnsw.dbscan and every other caller stay on hnswdbs_exact.                                                                  */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_DBSCAN_SCREEN_H */
