/* hnsw_mi355x_exact_long.h -- the screened exact k-NN for long rows, an extension of hnsw_mi355x_dbscan_screen.h in a header of its
 * own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its message in
 * hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the stream
 * contract of hnsw_mi355x.h.  The entries carry the prefix hnswxl_: the eight other headers keep their sets of hnswgpu_*, hnswhdb_*,
 * hnswhds_*, hnswhdp_*, hnswdbs_*, hnswxs_*, hnswxr_* and hnswxd_* symbols as they are.  The ctypes binding of these entries is
 * generated from THIS file.                                                                                                         */
#ifndef HNSW_MI355X_EXACT_LONG_H
#define HNSW_MI355X_EXACT_LONG_H

#include "hnsw_mi355x_dbscan_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------- 1. the screened exact k-NN, rows up to 4096 ----- */
/* hnswxs_exact_search_batch(_device) of hnsw_mi355x_exact_screen.h, argument for argument, out_stats included, and its contract word
 * for word: for every input hnswgpu_exact_search_batch accepts, these write byte for byte what it writes, and they refuse what it
 * refuses, in its words.  Screen, rerank, certificate, fallback, stats and memory are described there.  What differs is the screen
 * kernel behind rows of more than 256 elements (d rounded up to a multiple of 32):
 *   up to 256      the kernel of hnswxs_exact_search_batch: a tile's queries resident in LDS, four wavefronts.
 *   288 .. 4096    a kernel that keeps neither operand resident: 32 elements of 128 queries and of 64 rows stream through LDS per
 *                  step, and a wavefront's accumulators live across the whole row.  Its LDS does not depend on d, so every such d
 *                  runs four wavefronts; hnswxs_* runs two from 288, one from 576 and does not screen from 1121.
 *   above 4096     not screened: the whole call runs the existing path (stats word 2).
 * Beyond 1120 elements the bound's error term has a coefficient of its own, (4d + 96) 2^-24 (DistL2), (d + 64) 2^-24 (DistDot),
 * (2d + 96) 2^-24 (DistCosine); up to 1120 it is that of hnsw_mi355x_exact_screen.h.  A wider term costs candidates, never answers.    */
int hnswxl_exact_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                        const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dists,
                                        uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts, uint64_t* out_stats);
int hnswxl_exact_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                               const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids,
                                               float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                                               uint64_t* out_stats, void* stream);

/* ------------------------------------------------------------------------------- 2. the bound itself (diagnostic) ---------------- */
/* hnswxs_screen_matrix, argument for argument: out_lb[q * n + r] (host memory, nq x n f32) = the lower bound for (query q, the point
 * at position r of the dump order) -- ALWAYS from the streaming kernel with a store epilogue, for every d from 1 to 4096.
 *   refused   HNSWGPU_ERR_ARG: d above 4096 ("rows too long"); otherwise as hnswxs_screen_matrix refuses.                             */
int hnswxl_screen_matrix(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, float* out_lb);

/* The queries by stored point behind this kernel: hnsw_mi355x_exact_graph_screen.h (hnswxg_*).
 * Out of scope: the range search and DBSCAN behind this kernel; a set of filters; F16 storage; sharding.                            */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_EXACT_LONG_H */
