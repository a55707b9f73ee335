/* hnsw_mi355x_exact_graph_screen.h -- the exact k-NN graph of the stored points behind the matrix-core screen, an extension of
 * hnsw_mi355x_exact_long.h in a header of its own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an
 * HNSWGPU_* status and leaves its message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM
 * buffers and a HIP stream under the stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswxg_: the nine other headers
 * keep their sets of hnswgpu_*, hnswhdb_*, hnswhds_*, hnswhdp_*, hnswdbs_*, hnswxs_*, hnswxr_*, hnswxd_* and hnswxl_* symbols as they
 * are.  The ctypes binding of these entries is generated from THIS file.                                                            */
#ifndef HNSW_MI355X_EXACT_GRAPH_SCREEN_H
#define HNSW_MI355X_EXACT_GRAPH_SCREEN_H

#include "hnsw_mi355x_exact_long.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------- 1. the screened exact graph --------------------- */
/* hnswgpu_exact_graph_batch(_device) of hnsw_mi355x.h, argument for argument, plus out_stats, and its contract word for word: for
 * every input that call accepts, these write byte for byte what it writes -- ids, f32 distance bits, p_ids, counts, the order of
 * ties, zeros behind the counts -- and they refuse what it refuses, in its words and in its order (unknown ids with their count and
 * nothing written, out_stats included; F16 storage; HNSWGPU_ARITH_SIMD8; knbn == 0 or above 4096; np != nb_point with NULL ids; an
 * unsorted host filter).  Opt-in: no other entry calls them.
 *   how       The screen of hnswxs_ / hnswxl_exact_search_batch with the query operand taken from the replica's own rows: a tile
 *             holds the named points' flat ids, the screen kernel gathers each point's first d elements from its index row (zeros
 *             behind them), its plain f32 norm is the replica's row norm, and no copy of a query is written to scratch.  A point is
 *             left out of its own row BY IDENTITY inside the screen -- its DataId rank lies beside its threshold --, never by id,
 *             distance or bound: exact copies and the other points of a repeated DataId stay candidates, and a point need not pass
 *             the filter to be queried.  The rerank reads the point's row again, runs the exact chain on the k + 54 candidates and
 *             certifies the answer; a point it cannot certify is answered by hnswgpu_exact_graph_batch's own kernels into its row.
 *   routing   d rounded up to a multiple of 32: up to 256 the resident screen of hnswxs_*, four wavefronts; above, up to 4096, the
 *             streaming screen of hnswxl_* with its coefficient beyond 1120 elements.  A distance without a screen (DistL2, DistDot
 *             and DistCosine have one), knbn + 54 above 4096, fewer than 256 points, rows above 4096 elements: not screened, the whole
 *             call runs the existing path.
 *   out_stats host memory in both forms, may be NULL: three uint64_t -- points certified by the screen, points handed to the existing
 *             path by the certificate, points not screened at all.  They sum to np.  Written when the call succeeds.
 *   memory    the screen's lists and the fallback list in a pooled block of at most 320 MB; the replica's row norms (4 n bytes, made
 *             by the first screened call of any kind); a host call stages its answers in chunks of at most 64 MB.                    */
int hnswxg_exact_graph_batch(const hnswgpu_index* idx, const uint64_t* point_ids, uint64_t np, uint64_t k, const uint64_t* allowed_ids,
                             uint64_t n_allowed, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank,
                             uint32_t* out_counts, uint64_t* out_stats);
int hnswxg_exact_graph_batch_device(const hnswgpu_index* idx, const uint64_t* d_point_ids, uint64_t np, uint64_t k,
                                    const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids, float* d_out_dists,
                                    uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, uint64_t* out_stats, void* stream);

/* ------------------------------------------------------------------------------- 2. the bound itself (diagnostic) ---------------- */
/* out_lb[i * n + r] (host memory, np x n f32) = the lower bound that the screen kernel of the call above gives the pair (named point i,
 * the point at position r of the dump order), the point's own pair written like any other.  point_ids: host memory, NULL = every
 * point (np must be nb_point), row i being position i of the ascending (DataId, dump order) order.
 *   refused   HNSWGPU_ERR_ARG: as hnswxs_screen_matrix refuses (F16 storage, HNSWGPU_ARITH_SIMD8, a distance without a screen, np * n
 *             above 2^24 pairs); rows above 4096 elements ("rows too long"); an id that names no point.                               */
int hnswxg_screen_matrix(const hnswgpu_index* idx, const uint64_t* point_ids, uint64_t np, float* out_lb);

/* Out of scope: halving the work by symmetry; a set of filters; F16 storage; sharding; the symmetric graph, the recall ground truth
 * and the HDBSCAN entries behind this call.                                                                                         */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_EXACT_GRAPH_SCREEN_H */
