/* hnsw_mi355x_exact_range_screen.h -- exact range search behind a matrix-core screen, an extension of hnsw_mi355x_exact_screen.h in a
 * header of its own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its
 * message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the
 * stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswxr_: the six other headers keep their sets of hnswgpu_*,
 * hnswhdb_*, hnswhds_*, hnswhdp_*, hnswdbs_* and hnswxs_* symbols as they are.  The ctypes binding of these entries is generated
 * from THIS file.                                                                                                                   */
#ifndef HNSW_MI355X_EXACT_RANGE_SCREEN_H
#define HNSW_MI355X_EXACT_RANGE_SCREEN_H

#include "hnsw_mi355x_exact_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hnswgpu_exact_range_search_batch(_device) of hnsw_mi355x.h, argument for argument, and one more: for every input that call
 * accepts, these write byte for byte what it writes -- the CSR offsets (always complete), ids, f32 distance bits, p_ids, the order
 * within a query -- and they refuse what it refuses, in its words (HNSWGPU_STORAGE_F16, HNSWGPU_ARITH_SIMD8, a NULL buffer, a
 * dimension that is not the index's, an unsorted host filter).  The capacity rule is that call's: answers that need more than cap
 * slots return HNSWGPU_ERR_CAPACITY with its message, the offsets complete and no out slot touched; cap == 0 with NULL out arrays
 * counts only.  Only the cost differs: the existing call runs every (query, row) pair through the f32 chain twice, to count and to
 * fill; these run every pair once through the matrix cores and the chain on the candidates alone.
 *   screen    DistL2, DistDot, DistCosine: the inner products of (tile of queries, slab of rows) on the matrix cores in f32, each
 *             turned into the LOWER BOUND of hnsw_mi355x_exact_screen.h -- never above the f32 distance the exact arithmetic gives
 *             for the pair unless that distance is NaN, and +0 outside the range in which that is proved.  A pair whose bound is at
 *             or below the query's radius (a plain f32 comparison: a NaN radius has no candidate) is a candidate; every answer is
 *             one.  No certificate is needed: a pair that is no candidate is no answer.
 *   rerank    every candidate in the exact arithmetic; those with distance <= radius are the answers.
 *   sort      per query by (distance, DataId, dump order), as the existing call sorts.  The order in which candidates and answers
 *             arrive reaches no output: two calls give the same bytes.
 *   fallback  a call whose candidates outgrow a chunk's buffer (2 Mi pairs) or whose answers outgrow the key buffer (8 Mi) is
 *             answered by the code of hnswgpu_exact_range_search_batch itself, whole.
 *   stats     out_stats (host memory in both forms, may be NULL): [0] queries answered through the screen, [1] queries answered by
 *             the existing path because a buffer was outgrown, [2] queries not screened at all -- a distance without a screen
 *             (DistL1, DistHellinger, DistJeffreys, DistJensenShannon), fewer than 256 points, rows too long for a tile of queries
 *             in LDS (d above 1120), an index whose filter bitmap alone breaks the scratch bound: the whole call then runs the
 *             existing path.  The three add up to nq.
 *   memory    fixed, whatever nq and n are: at most the 320 MB of the screened exact k-NN from the replica's pool plus the sort's
 *             temporary storage, and the n f32 of row norms that the screened k-NN keeps with the replica too; a fallback takes
 *             the existing call's scratch instead.  The host form stages queries in blocks of 64 MB like the existing call.
 * Legal from several host threads at once (the handle's lock is taken shared).  The host form uploads the index on first use; the
 * device form wants a resident replica (HNSWGPU_ERR_DEVICE otherwise) and waits for `stream` before it returns.                     */
int hnswxr_exact_range_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, const float* radii,
                                    const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t cap, uint64_t* out_offsets,
                                    uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint64_t* out_stats);
int hnswxr_exact_range_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                           const float* d_radii, const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t cap,
                                           uint64_t* d_out_offsets, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer,
                                           int32_t* d_out_rank, uint64_t* out_stats, void* stream);

/* Out of scope: DBSCAN's passes; the queries by stored point; a set of filters; F16 storage; sharding; recovery from an outgrown
 * buffer chunk by chunk.                                                                                                            */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_EXACT_RANGE_SCREEN_H */
