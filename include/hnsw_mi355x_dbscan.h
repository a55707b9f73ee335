/* hnsw_mi355x_dbscan.h -- DBSCAN(eps, min_samples) on the device, an extension of hnsw_mi355x_hdbscan_predict.h in a header of its
 * own: exact over the points of an uploaded index, the vectors never leaving HBM and no neighbour list ever built, and over any
 * neighbour lists a caller already has, in CSR.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an
 * HNSWGPU_* status and leaves its message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM
 * buffers and a HIP stream under the stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswdbs_: the four other headers
 * keep their sets of hnswgpu_*, hnswhdb_*, hnswhds_* and hnswhdp_* symbols as they are.  The ctypes binding of these entries is
 * generated from THIS file.                                                                                                       */
#ifndef HNSW_MI355X_DBSCAN_H
#define HNSW_MI355X_DBSCAN_H

#include "hnsw_mi355x_hdbscan_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------- 1. the contract, both forms ------------------- */
/* Vertices are POSITIONS: vertex i is the point at position i of the ascending (DataId, dump order) order, the row numbering of
 * hnswgpu_symmetric_graph.  N(i) is a set of pairs (j, w), j a vertex and w an f32, defined per form below.
 *   count     count[i] = |N(i)| (the CSR form: + add_self).
 *   core      core[i] iff count[i] >= min_samples.
 *   join      two core points i, j are joined iff j is in N(i) or i is in N(j).  A cluster is a connected component of the core
 *             points under these joins.  Clusters are numbered 0 .. c - 1 by their smallest core position, ascending.
 *   core pt   its label is its cluster, its anchor is itself.
 *   other pt  a point i that is not core looks only at its OWN set: its candidates are the (j, w) of N(i) with core[j], its anchor
 *             is the candidate of smallest key (dist_order_bits(w) << 32) | j -- the order of the exact k-NN key: by value, -0 as
 *             +0, a tie by position --, its label is the anchor's.  Without a candidate the label is -1 (noise) and the anchor is
 *             UINT32_MAX.
 *   exact     Everything is integers and ordered f32 comparisons: the answer is a function of the input alone, and two calls give
 *             the same bytes.
 *   outputs   out_label (i32[n]) is required when n > 0; out_core (u8[n], 0 or 1), out_count (u32[n]) and out_anchor (u32[n]) may
 *             be NULL, each on its own.  *out_n_clusters (u64) is host memory in both forms.  Nothing is written behind slot n - 1.
 *             On any error no out slot is touched.
 *   refused   HNSWGPU_ERR_ARG, nothing written: min_samples == 0; eps NaN; n above 2^31 - 1; a NULL out_label with n > 0; a NULL
 *             out_n_clusters.  A negative eps is legal: nothing is within it, every point is noise when min_samples >= 1 + add_self.
 *   small     n == 0: *out_n_clusters = 0, HNSWGPU_OK, nothing else written, no device needed.                                    */

/* ------------------------------------------------------------------------------- 2. exact, over the points of the index -------- */
/* N(i) = { (j, v) : v = dist(point i as the query, row j) and v <= eps }, the IEEE f32 comparison of hnswgpu_exact_range_search_batch:
 * the bits of v are those of hnswgpu_exact_search_batch for the point's vector brought as a query, a NaN never matches, -0 equals +0.
 * The point itself is a row like any other: there is no exclusion by identity, exact copies and repeated DataIds are ordinary points.
 * For DistJeffreys and DistJensenShannon the two directions of a pair differ in their bits, so a pair may be within eps one way only:
 * the join rule's "or" covers that (the union mode of hnswgpu_symmetric_graph reads a pair the same way), and a point that is not
 * core reads its own direction only.
 *   refused   besides section 1: HNSWGPU_ARITH_SIMD8, HNSWGPU_STORAGE_F16 (in the exact range search's words).
 *   memory    25 n + n / 8 bytes (parent, count, best, the two core arrays, the roots' flags and their scan), one chunk of tiled
 *             queries of at most 64 MB and rocPRIM's temporary storage of one scan of n + 1 words; the host form: 8 n bytes of
 *             staged labels and anchors besides.  No list of neighbours exists at any time.
 * Two passes over the same pair evaluations, one kernel template: the stored rows are tiled as queries, 16 to a wavefront, against
 * slabs of rows, one row per lane (the exact range search's loop).  The count pass adds a ballot's popcount per (query, 64 rows) and
 * ends in one integer atomic per (query, slab).  One kernel sets the core flags by position and a core bitmap by row.  The link
 * pass skips every 64 rows without a core row within eps of a query; a core query unites with the core rows it hits (a lock-free
 * union-find, the larger root under the smaller), a query that is not core lowers its best key by an integer atomic min.  Then the
 * trees are compressed, the flags "core and its own root" are scanned -- the last word is c -- and one kernel writes the answer.
 * Integer atomics only, no grid-wide sync; read back: c.  Legal from several host threads at once (the handle's lock is taken shared).
 * The host form uploads the index on first use; the device form wants a resident replica (HNSWGPU_ERR_DEVICE otherwise).          */
int hnswdbs_exact(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* out_label, uint8_t* out_core, uint32_t* out_count,
                  uint32_t* out_anchor, uint64_t* out_n_clusters);
int hnswdbs_exact_device(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* d_out_label, uint8_t* d_out_core,
                         uint32_t* d_out_count, uint32_t* d_out_anchor, uint64_t* out_n_clusters, void* stream);

/* ------------------------------------------------------------------------------- 3. over any CSR graph -------------------------- */
/* For neighbour lists that exist already, by position: the outputs of hnswgpu_symmetric_graph_device as they stand, or a range
 * search's answer with its ids turned into positions.  No index is needed.  Row i is entries offsets[i] .. offsets[i + 1] - 1.
 *   N(i)      entry e of row i, naming j = cols[e], is in N(i) iff dists == NULL or dists[e] <= eps (the same ordered comparison);
 *             its w is dists[e], +0 when dists is NULL.  Self entries and repeated entries count as they stand.
 *   add_self  0 or 1 (anything else: HNSWGPU_ERR_ARG), added to every count: 1 for k-NN rows that never name their own point, 0 for
 *             range answers that do.
 *   directed  The rule for a point that is not core is DIRECTED: such an i that only a core j's row names, and that does not name j
 *             itself, is noise.  A symmetric CSR gives the textbook behaviour.
 *   refused   besides section 1, what hnswgpu_csr_components refuses, in its words: NULL offsets with n > 0, offsets[0] != 0,
 *             descending offsets, offsets[n] >= 2^32, NULL cols with entries, a col >= n.  The host form checks on the host; the
 *             device form by kernel, one word read back BEFORE any kernel follows a col: a bad graph is HNSWGPU_ERR_ARG, never a fault.
 *   memory    25 n bytes and the scan's temporary storage; the host form: the graph and 8 n bytes of staged answers besides.
 * One thread per entry: the counts (its row by a binary search in the offsets), the core flags, the unions over the entries whose two
 * ends are core, the atomic min of the others' keys; then section 2's finish, the same code.                                      */
int hnswdbs_csr(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists, float eps, uint64_t min_samples,
                uint32_t add_self, int32_t* out_label, uint8_t* out_core, uint32_t* out_count, uint32_t* out_anchor, uint64_t* out_n_clusters);
int hnswdbs_csr_device(int device, uint64_t n, const uint64_t* d_offsets, const uint32_t* d_cols, const float* d_dists, float eps,
                       uint64_t min_samples, uint32_t add_self, int32_t* d_out_label, uint8_t* d_out_core, uint32_t* d_out_count,
                       uint32_t* d_out_anchor, uint64_t* out_n_clusters, void* stream);

/* Out of scope: using dist(i, j) == dist(j, i) to halve the work; filters or a subset of the points; labels by DataId; an
 * approximate form through the graph search (section 3 serves it by composition: hnswgpu_symmetric_graph_device, then hnswdbs_csr_device);
 * OPTICS; sharding over GPUs; F16 storage; the SIMD-order arithmetic.                                                             */

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_DBSCAN_H */
