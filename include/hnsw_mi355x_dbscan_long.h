/* hnsw_mi355x_dbscan_long.h -- the screened exact DBSCAN for long rows, an extension of hnsw_mi355x_exact_range_long.h in a header of
 * its own.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its message in
 * hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the stream
 * contract of hnsw_mi355x.h.  The entries carry the prefix hnswxdl_: the eleven other headers keep their sets of hnswgpu_*, hnswhdb_*,
 * hnswhds_*, hnswhdp_*, hnswdbs_*, hnswxs_*, hnswxr_*, hnswxd_*, hnswxl_*, hnswxg_* and hnswxrl_* symbols as they are.  The ctypes
 * binding of these entries is generated from THIS file.                                                                             */
#ifndef HNSW_MI355X_DBSCAN_LONG_H
#define HNSW_MI355X_DBSCAN_LONG_H

#include "hnsw_mi355x_exact_range_long.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hnswxd_exact(_device) of hnsw_mi355x_dbscan_screen.h, argument for argument, out_stats included, and its contract word for word:
 * for every input hnswdbs_exact accepts, these write byte for byte what it writes -- labels, core flags, counts, anchors, the number
 * of clusters -- and they refuse what it refuses, in its words and in its order; a refused call writes nothing.  Screen, count, link,
 * fallback, stats and memory are described there.  Opt-in: no other entry calls them.  What differs is the screen kernel behind rows
 * of more than 256 elements (d rounded up to a multiple of 32):
 *   up to 256      the kernel of hnswxd_exact: a tile's points resident in LDS, four wavefronts; the same bytes and the same stats
 *                  as that call.
 *   288 .. 4096    a kernel that keeps neither operand resident: 32 elements of 128 points as queries and of 128 rows stream through
 *                  LDS per step, a wavefront's four accumulator tiles live across the whole row, and the two-sided test, the counts,
 *                  the unions and the candidate buffer are those of hnswxd_*.  Its LDS does not depend on d, so every such d runs
 *                  four wavefronts; hnswxd_* runs two from 288, one from 576 and does not screen from 1121.
 *   above 4096     not screened: the whole call runs the existing path (stats word 2), as for a distance without a screen, fewer
 *                  than 256 points or an index beyond the scratch budget.
 * Beyond 1120 elements both bounds' error term has the coefficient of hnsw_mi355x_exact_long.h, (4d + 96) 2^-24 (DistL2), (d + 64)
 * 2^-24 (DistDot), (2d + 96) 2^-24 (DistCosine); up to 1120 it is that of hnsw_mi355x_exact_screen.h.  The upper bound is proved
 * with it for d up to 4096.  A wider term costs pairs for the exact chain, never answers.  The chunk of points
 * that shares the 16 MB of padded queries shrinks with d (eight tiles of 128 at d = 4096).
 *   cost           the padded points of a tile are read again, from L2, for every block of 128 rows, and every pair is screened
 *                  twice (count, link).  Expect a gain over hnswdbs_exact that grows with d where the band is thin; expect little
 *                  where most pairs are undecided -- rows far from the origin relative to eps: the error term is a multiple of
 *                  |q|^2 + |x|^2 -- since those pairs run the chain as before, and a loss where the buffer is outgrown (the
 *                  existing call plus the screening up to the overflow).  RESULTS.md "DBSCAN, long rows" says what was measured.  */
int hnswxdl_exact(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* out_label, uint8_t* out_core, uint32_t* out_count,
                  uint32_t* out_anchor, uint64_t* out_n_clusters, uint64_t* out_stats);
int hnswxdl_exact_device(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* d_out_label, uint8_t* d_out_core,
                         uint32_t* d_out_count, uint32_t* d_out_anchor, uint64_t* out_n_clusters, uint64_t* out_stats, void* stream);

/* hnswxd_bounds_matrix argument for argument (host buffers, DistL2 / DistDot / DistCosine, nq * n up to 2^24): the two bounds of the
 * STREAMED kernel, whatever d is, from 1 to 4096; longer rows are refused ("rows too long").  Outside the proved range lb is +0 and
 * ub is +inf.                                                                                                                      */
int hnswxdl_bounds_matrix(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, float* out_lb, float* out_ub);

/* Out of scope: using dist(i, j) = dist(j, i) to halve the tiles; gathering the queries from the replica's own rows; F16 storage;
 * filters; the CSR forms.  Hnsw.dbscan, HDBSCAN and every other caller stay on their entries.                                       */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_DBSCAN_LONG_H */
