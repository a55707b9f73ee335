/* hnsw_mi355x_exact_range_long.h -- the screened exact range search for long rows, an extension of hnsw_mi355x_exact_graph_screen.h in a
 * header of its own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its
 * message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the
 * stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswxrl_: the ten other headers keep their sets of hnswgpu_*,
 * hnswhdb_*, hnswhds_*, hnswhdp_*, hnswdbs_*, hnswxs_*, hnswxr_*, hnswxd_*, hnswxl_* and hnswxg_* symbols as they are.  The ctypes
 * binding of these entries is generated from THIS file.                                                                             */
#ifndef HNSW_MI355X_EXACT_RANGE_LONG_H
#define HNSW_MI355X_EXACT_RANGE_LONG_H

#include "hnsw_mi355x_exact_graph_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hnswxr_exact_range_search_batch(_device) of hnsw_mi355x_exact_range_screen.h, argument for argument, out_stats included, and its
 * contract word for word: for every input hnswgpu_exact_range_search_batch accepts, these write byte for byte what it writes, and
 * they refuse what it refuses, in its words and in its order; the capacity rule is that call's.  Screen, rerank, sort, fallback,
 * stats and memory are described there.  Opt-in: no other entry calls them.  What differs is the screen kernel behind rows of more
 * than 256 elements (d rounded up to a multiple of 32):
 *   up to 256      the kernel of hnswxr_exact_range_search_batch: a tile's queries resident in LDS, four wavefronts; the same bytes
 *                  and the same stats as that call.
 *   288 .. 4096    a kernel that keeps neither operand resident: 32 elements of 128 queries and of 128 rows stream through LDS per
 *                  step, a wavefront's four accumulator tiles live across the whole row, and the test against the radius is that
 *                  of hnswxr_*.  Its LDS does not depend on d, so every such d runs four wavefronts; hnswxr_* runs two from 288,
 *                  one from 576 and does not screen from 1121.
 *   above 4096     not screened: the whole call runs the existing path (stats word 2).
 * Beyond 1120 elements the bound's error term has the coefficient of hnsw_mi355x_exact_long.h, (4d + 96) 2^-24 (DistL2), (d + 64)
 * 2^-24 (DistDot), (2d + 96) 2^-24 (DistCosine); up to 1120 it is that of hnsw_mi355x_exact_screen.h.  A wider term costs
 * candidates, never answers: a pair that is no candidate is no answer.  The chunk of query tiles that shares the 16 MB of padded
 * queries shrinks with d (eight tiles of 128 at d = 4096).                                                                          */
int hnswxrl_exact_range_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, const float* radii,
                                     const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t cap, uint64_t* out_offsets,
                                     uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint64_t* out_stats);
int hnswxrl_exact_range_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                            const float* d_radii, const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t cap,
                                            uint64_t* d_out_offsets, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer,
                                            int32_t* d_out_rank, uint64_t* out_stats, void* stream);

/* Out of scope: DBSCAN behind this kernel; a set of filters; F16 storage; sharding; moving any existing caller to these entries.    */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_EXACT_RANGE_LONG_H */
