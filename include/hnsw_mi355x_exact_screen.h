/* hnsw_mi355x_exact_screen.h -- exhaustive exact k-NN behind a matrix-core screen, an extension of hnsw_mi355x_dbscan.h in a header of
 * its own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its message in
 * hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the stream
 * contract of hnsw_mi355x.h.  The entries carry the prefix hnswxs_: the five other headers
 * keep their sets of hnswgpu_*, hnswhdb_*, hnswhds_*, hnswhdp_* and hnswdbs_* symbols as they are.  The ctypes binding of these entries is
 * generated from THIS file.                                                                                                         */
#ifndef HNSW_MI355X_EXACT_SCREEN_H
#define HNSW_MI355X_EXACT_SCREEN_H

#include "hnsw_mi355x_dbscan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------- 1. the screened exact k-NN ---------------------- */
/* hnswgpu_exact_search_batch(_device) of hnsw_mi355x.h, argument for argument, and one more: for every input that call accepts,
 * these write byte for byte what it writes -- ids, f32 distance bits, p_ids, counts, the tie order, the zeros behind the counts --
 * and they refuse what it refuses, in its words (HNSWGPU_STORAGE_F16, HNSWGPU_ARITH_SIMD8, knbn == 0 or above 4096, a NULL buffer,
 * a dimension that is not the index's, an unsorted host filter).  Only the cost differs.
 *   screen    DistL2, DistDot, DistCosine: the inner products of (tile of queries, slab of rows) on the matrix cores in f32, each
 *             turned into a LOWER BOUND of the f32 distance the exact arithmetic gives for the pair (the bound covers the matrix
 *             cores' rounding, whatever their internal order, and the exact chain's own).  Per query the C = knbn + 54 rows of
 *             smallest bound are kept.
 *   rerank    those C rows in the exact arithmetic; the knbn smallest by (distance, DataId, dump order).
 *   certify   the answer is the exact call's when fewer than C rows were eligible, or when the C-th bound is greater, as an f32,
 *             than the knbn-th exact distance: every row left out then lies strictly behind the cut.
 *   fallback  a query that is not certified is answered by the code of hnswgpu_exact_search_batch itself.
 *   stats     out_stats (host memory in both forms, may be NULL): [0] queries certified by the screen, [1] queries answered by the
 *             existing path because the certificate refused, [2] queries not screened at all -- a distance without a screen
 *             (DistL1, DistHellinger, DistJeffreys, DistJensenShannon), knbn + 54 above 4096, fewer than 256 points, rows too long
 *             for a tile of queries in LDS (d above 1120): the whole call then runs the existing path.  The three add up to nq.
 *   memory    at most 320 MB of scratch from the replica's pool, n f32 of row norms kept with the replica; a fallback takes the
 *             existing call's scratch besides.
 * Legal from several host threads at once (the handle's lock is taken shared).  The host form uploads the index on first use; the
 * device form wants a resident replica (HNSWGPU_ERR_DEVICE otherwise) and waits for `stream` before it returns.                     */
int hnswxs_exact_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                        const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dists,
                                        uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts, uint64_t* out_stats);
int hnswxs_exact_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                               const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids,
                                               float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                                               uint64_t* out_stats, void* stream);

/* ------------------------------------------------------------------------------- 2. the bound itself (diagnostic) ---------------- */
/* out_lb[q * n + r] (host memory, nq x n f32) = the screen kernel's lower bound for (query q, the point at position r of the dump
 * order), from the kernel itself with a store epilogue: never NaN, never below +0, and +0 for every pair outside the range in
 * which the bound is proved (a squared norm outside [2^-40, 2^40] or NaN, a screen value that is not finite).  For small shapes.
 *   refused   HNSWGPU_ERR_ARG: nq * n above 2^24; a distance without a screen; d above 1120; a NULL buffer with nq > 0; a dimension
 *             that is not the index's; HNSWGPU_STORAGE_F16; HNSWGPU_ARITH_SIMD8.  An index without a point: HNSWGPU_OK, nothing
 *             written.                                                                                                             */
int hnswxs_screen_matrix(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, float* out_lb);

/* The queries by stored point behind this screen: hnsw_mi355x_exact_graph_screen.h (hnswxg_*).
 * Out of scope: a set of filters; DBSCAN's passes; F16 storage; sharding.                                                          */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_EXACT_SCREEN_H */
