/* hnsw_mi355x_hdbscan_predict.h -- HDBSCAN's third stage on the device, an extension of hnsw_mi355x_hdbscan_select.h in a header of
 * its own: new points are assigned to the clusters of a condensed tree that hnswhdb_forest / hnswhdb_graph wrote and hnswhds_select
 * (or the first stage itself) selected from -- what users of the `hdbscan` package know as approximate_predict -- without anything
 * being clustered again.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its
 * message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM buffers and a HIP stream under the
 * stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswhdp_: the three other headers keep their sets of hnswgpu_*,
 * hnswhdb_* and hnswhds_* symbols as they are.  The ctypes binding of these entries is generated from THIS file.                  */
#ifndef HNSW_MI355X_HDBSCAN_PREDICT_H
#define HNSW_MI355X_HDBSCAN_PREDICT_H

#include "hnsw_mi355x_hdbscan_select.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------- 1. the stored points' core distances --------- */
/* out_core[v], v a POSITION (hnswgpu_symmetric_graph), is exactly the core distance that hnswgpu_graph_spanning_forest -- and so
 * hnswhdb_graph -- uses with the same knbn, ef and core_k: the stored f32 bits of slot min(core_k, counts[v]) - 1 of row v of D, D
 * the exact graph of the stored points for ef == 0 and the graph search for ef >= 1; +0 for an empty row or core_k == 0.
 *   refused   what that call refuses, in its words: knbn == 0, core_k > knbn, nb_point x knbn above 2^30, F16 storage,
 *             HNSWGPU_ARITH_SIMD8 with ef == 0, knbn above 4096 with ef == 0; a NULL out_core on an index with a point.
 *   small     An index without a point: HNSWGPU_OK, nothing written, no device needed.
 *   memory    D staged (17 n knbn + 4 n bytes) and n words.
 * The host form uploads the index on first use; the device form wants a resident replica (HNSWGPU_ERR_DEVICE otherwise).          */
int hnswhdp_core_distances(const hnswgpu_index* idx, uint64_t knbn, uint64_t ef, uint64_t core_k, float* out_core);
int hnswhdp_core_distances_device(const hnswgpu_index* idx, uint64_t knbn, uint64_t ef, uint64_t core_k, float* d_out_core, void* stream);

/* ------------------------------------------------------------------------------- 2. assignment from neighbour rows ------------- */
/*   input     nq rows of knbn slots: nbr_pos (u32 positions of stored points), nbr_dist (f32) and counts[q] <= knbn, the slots of
 *             row q that are used; core_k; core (f32[n], entry 1's answer); the tree as hnswhdb_* / hnswhds_select wrote it: K
 *             per-cluster slots (cluster_parent, cluster_birth_w, selected) and n per-vertex slots (point_cluster, point_w);
 *             cluster_selection_epsilon (eps) as it was given to the selection; optionally cluster_death_lambda (f64[K],
 *             hnswhds_select's output).  No index is needed.
 *   order     Weights compare by dist_order_bits: as values, -0 as +0, every NaN behind +inf (all NaNs equal).  lambda(w) is
 *             hnsw_mi355x_hdbscan.h's: 1.0 / (double)w; +0 for +inf and NaN; +inf for w <= 0, -0 included.
 *   core(q)   the bits of slot min(core_k, counts[q]) - 1 of row q of nbr_dist, +0 if that is slot -1.
 *   mr(q, s)  for slot s with position j = nbr_pos[q][s]: the largest of nbr_dist[q][s], core(q), core[j], in this order of
 *             arguments; a tie keeps the earlier one (hnswgpu_graph_spanning_forest's rule for the bits that survive).
 *   nearest   s* minimises the u64 key (order bits of mr(q, s)) << 32 | s over the used slots.  nearest[q] = nbr_pos[q][s*],
 *             w[q] = the bits of mr(q, s*), lambda_q = lambda(w[q]).
 *   empty row counts[q] == 0: nearest = UINT32_MAX, w = +inf, lambda_q = +0, cluster = 0, label -1, prob 0; the score by the
 *             score rule with c = 0.
 *   cluster   c0 = point_cluster[nearest], lambda_j = lambda(point_w[nearest]).  If lambda_j <= lambda_q, cluster[q] = c0.
 *             Otherwise c = c0, and while c != 0 and lambda(cluster_birth_w[c]) >= lambda_q: c = cluster_parent[c]; cluster[q] = c.
 *             (Both comparisons are those of the hdbscan package's _find_cluster_and_probability.)
 *   label     maxlambda(c) is hnsw_mi355x_hdbscan_select.h's: the largest lambda over the rows of c -- vertices by point_w, child
 *             clusters by birth --, 0 without rows.  If selected is exactly {0}: label 0 iff lambda_q >= thr, with thr =
 *             1.0 / (double)eps for eps > 0, else maxlambda(0) (that header's rule 5).  Otherwise the label of the nearest member
 *             of selected among cluster[q] and its ancestors, or -1.  Labels number the selected clusters by ascending index: they
 *             are the labels of the stored points.
 *   prob      0 for label -1; for the labelled cluster L it is 1 if maxlambda(L) == 0 or lambda_q >= maxlambda(L), otherwise
 *             (float)(lambda_q / maxlambda(L)).
 *   score     only with cluster_death_lambda: for c = cluster[q] and d = cluster_death_lambda[c], 0 if d == 0 or lambda_q >= d;
 *             1 if d = +inf; otherwise (float)((d - lambda_q) / d), two separate f64 operations, no FMA (GLOSH, as for a stored
 *             point).  With K == 0 (then n == 0 and every row is empty) there is no cluster 0: the score is 0.
 *   outputs   out_labels (i32[nq]) is required; out_prob (f32), out_score (f32), out_nearest (u32), out_w (f32) and out_cluster
 *             (u32), nq slots each, may be NULL, each on its own.  Nothing is written behind slot nq - 1.
 *   refused   HNSWGPU_ERR_ARG, no out slot touched: eps NaN or < 0; core_k > knbn; knbn == 0 with nq >= 1; n, K or nq above
 *             2^31 - 1; nq x knbn above 2^31 - 1; K == 0 with n >= 1; a NULL array that is needed (core, point_cluster and point_w
 *             with n >= 1; the three cluster arrays with K >= 1; the three row arrays and out_labels with nq >= 1); out_score
 *             without cluster_death_lambda; cluster_parent[0] != UINT32_MAX; cluster_parent[c] >= c for any c >= 1;
 *             point_cluster[v] >= K; counts[q] > knbn; nbr_pos >= n in a used slot.  The host form checks on the host first.  The
 *             device form checks by kernel BEFORE ANY TRAVERSAL OR GATHER, one word read back: a bad index is never dereferenced, a
 *             malformed parent array can neither fault nor loop.
 *   small     nq == 0 writes nothing and needs no device.
 *   memory    28 K + 24 nq bytes of scratch (the host form: its inputs besides) and rocPRIM's temporary storage of one scan of
 *             K + 1 words.
 * One kernel checks and raises maxlambda (integer atomic max on the f64 bits); the table "label of the nearest selected
 * ancestor-or-self" is made once per call by pointer doubling, rounds counted on the host, and one scan; then 16 lanes per query
 * read the row, gather core[], keep the smallest key and fold it across lanes, and the group's first lane climbs: every step goes to
 * a strictly smaller cluster index, so a walk has at most depth(cluster tree) steps.  The key holds the slot: the answer does not
 * depend on the group's width.  Read back: the check word.  Legal from several host threads at once.
 * Deviations from the hdbscan package's approximate_predict:
 *   - A query whose cluster[q] is a descendant of a selected cluster gets that cluster's label; the package answers -1 unless the
 *     cluster it finds is itself selected.
 *   - maxlambda is taken of the labelled cluster, not of the found one.
 *   - core(q) is the distance to the query's core_k-th stored neighbour; the package reads slot min_samples of a query for
 *     2 * min_samples neighbours.
 * Out of scope: soft clustering (membership vectors), filtered prediction, sharding, F16 storage, labels by DataId, mcs = 1.      */
int hnswhdp_assign(int device, uint64_t nq, uint64_t knbn, const uint32_t* nbr_pos, const float* nbr_dist, const uint32_t* counts,
                   uint64_t core_k, uint64_t n, const float* core, uint64_t K,
                   const uint32_t* cluster_parent, const float* cluster_birth_w, const uint32_t* point_cluster, const float* point_w,
                   const uint8_t* selected, float cluster_selection_epsilon, const double* cluster_death_lambda,
                   int32_t* out_labels, float* out_prob, float* out_score, uint32_t* out_nearest, float* out_w, uint32_t* out_cluster);
/* The same with every array in HBM of `device`, on HIP stream `stream`, waited for.                                               */
int hnswhdp_assign_device(int device, uint64_t nq, uint64_t knbn, const uint32_t* d_nbr_pos, const float* d_nbr_dist,
                          const uint32_t* d_counts, uint64_t core_k, uint64_t n, const float* d_core, uint64_t K,
                          const uint32_t* d_cluster_parent, const float* d_cluster_birth_w, const uint32_t* d_point_cluster,
                          const float* d_point_w, const uint8_t* d_selected, float cluster_selection_epsilon,
                          const double* d_cluster_death_lambda,
                          int32_t* d_out_labels, float* d_out_prob, float* d_out_score, uint32_t* d_out_nearest, float* d_out_w,
                          uint32_t* d_out_cluster, void* stream);

/* ------------------------------------------------------------------------------- 3. prediction for new vectors ------------------ */
/* Row q of the neighbours is the answer of hnswgpu_search_batch(queries, knbn, ef) under the handle's settings, bit for bit -- with
 * ef == 0 that of hnswgpu_exact_search_batch without a filter --, each entry's p_id turned into its position as
 * hnswgpu_symmetric_graph defines it; the rest is entry 2 on the staged rows, the same kernels, nothing leaving HBM in between.  n is
 * hnswgpu_nb_point(idx); core, point_cluster and point_w have that many slots.
 *   refused   what the search (ef >= 1) or the exact search (ef == 0) refuses, in its words; what entry 2 refuses; F16 storage.
 *   small     nq == 0 writes nothing.  An index without a point: every row is empty (label -1, the other outputs as entry 2 gives
 *             them for empty rows).
 *   memory    the staged rows (21 nq knbn + 4 nq bytes; the host form: the queries besides), the search's own, and entry 2's.
 * The host form uploads the index on first use; the device form wants a resident replica (HNSWGPU_ERR_DEVICE otherwise).  The
 * handle's lock is taken shared: legal beside searches.                                                                          */
int hnswhdp_predict(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t knbn, uint64_t ef, uint64_t core_k,
                    const float* core, uint64_t K,
                    const uint32_t* cluster_parent, const float* cluster_birth_w, const uint32_t* point_cluster, const float* point_w,
                    const uint8_t* selected, float cluster_selection_epsilon, const double* cluster_death_lambda,
                    int32_t* out_labels, float* out_prob, float* out_score, uint32_t* out_nearest, float* out_w, uint32_t* out_cluster);
int hnswhdp_predict_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t knbn, uint64_t ef,
                           uint64_t core_k, const float* d_core, uint64_t K,
                           const uint32_t* d_cluster_parent, const float* d_cluster_birth_w, const uint32_t* d_point_cluster,
                           const float* d_point_w, const uint8_t* d_selected, float cluster_selection_epsilon,
                           const double* d_cluster_death_lambda,
                           int32_t* d_out_labels, float* d_out_prob, float* d_out_score, uint32_t* d_out_nearest, float* d_out_w,
                           uint32_t* d_out_cluster, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_HDBSCAN_PREDICT_H */
