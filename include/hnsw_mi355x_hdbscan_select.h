/* hnsw_mi355x_hdbscan_select.h -- HDBSCAN's second stage on the device, an extension of hnsw_mi355x_hdbscan.h in a header of its own:
 * from a condensed tree that hnswhdb_forest / hnswhdb_graph wrote, the selection of clusters under allow_single_cluster,
 * cluster_selection_epsilon and max_cluster_size, the flat labels and probabilities, and the GLOSH outlier scores -- without the
 * dendrogram and the condensed tree being made again.  Same library (libhnsw_mi355x.so), same conventions: every entry returns an
 * HNSWGPU_* status and leaves its message in hnswgpu_last_error(); the host form takes host buffers, the `_device` form takes HBM
 * buffers and a HIP stream under the stream contract of hnsw_mi355x.h.  The entries carry the prefix hnswhds_: the two other headers
 * keep their sets of hnswgpu_* and hnswhdb_* symbols as they are.  The ctypes binding of these entries is generated from THIS
 * file.                                                                                                                          */
#ifndef HNSW_MI355X_HDBSCAN_SELECT_H
#define HNSW_MI355X_HDBSCAN_SELECT_H

#include "hnsw_mi355x_hdbscan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- HDBSCAN: selection options and GLOSH from a condensed tree --- */
/*   input     The six arrays that an hnswhdb_* call wrote: K per-cluster slots (cluster_parent, cluster_birth_w, cluster_size,
 *             stability) and n per-vertex slots (point_cluster, point_w).  method is HNSWGPU_SELECT_EOM or HNSWGPU_SELECT_LEAF;
 *             allow_single_cluster is 0 or 1; cluster_selection_epsilon (eps) is a weight, >= 0, +inf legal; max_cluster_size
 *             0 means no limit.  lambda(w) is hnsw_mi355x_hdbscan.h's: 1.0 / (double)w; +0 for +inf and NaN; +inf for w <= 0, -0
 *             included.  Weights compare by value, NaN counts as +inf and -0 as +0.
 *   per cluster  kids(c): its children.  size(c) = cluster_size[c], with no special case for cluster 0.  maxlambda(c): the largest
 *             lambda over the rows of c -- the vertices with point_cluster == c, by point_w, and the child clusters, by their
 *             birth --, 0 without rows.  lambda_v = lambda(point_w[v]).
 *   1 winners HNSWGPU_SELECT_EOM, bottom-up: sub(c) is the sum of S over kids(c).  c is a CANDIDATE iff c != 0 or
 *             allow_single_cluster.  A candidate WINS iff stability[c] >= sub(c) and (max_cluster_size == 0 or size(c) <=
 *             max_cluster_size).  S(c) = stability[c] if c wins, else sub(c).  A cluster other than 0 has no child or two: its sub
 *             is one commutative f64 add.  sub(0) may have thousands of terms: thread t of 256 adds S of the children of 0 whose
 *             index is t modulo 256, in ascending index, and the 256 sums are folded in a fixed tree -- a function of the input
 *             alone: the same bytes from call to call, and |sub - exact| <= children 2^-53 exact.
 *             HNSWGPU_SELECT_LEAF: c != 0 wins iff it has no child; cluster 0 wins iff allow_single_cluster and K == 1;
 *             max_cluster_size is ignored, as in scikit-learn.
 *   2 E       the winners without a winning proper ancestor.
 *   3 epsilon applied when eps > 0 and E != {0}.  A member c with birth_w(c) < eps climbs: with p = parent(c), if p == 0 it ends
 *             at 0 when allow_single_cluster, else at c itself; otherwise it ends at p if birth_w(p) > eps; otherwise it goes on
 *             from p.  A member with birth_w(c) >= eps stays.  F is the set of ends; E' is the members of F without a proper
 *             ancestor in F.  With eps == 0 (-0 too) E' = E.
 *   4 numbering  selected[c] iff c is in E'.  Labels number E' by ascending cluster index.  *out_n_labels = |E'|.
 *   5 labels  If E' = {0}: vertex v gets label 0 iff lambda_v >= thr, with thr = 1.0 / (double)eps if eps > 0, else
 *             maxlambda(0) -- for every vertex, whatever its point_cluster.  Otherwise the label is that of the nearest member of
 *             E' among point_cluster[v] and its ancestors, or -1.  prob[v] is 0 for -1; for the labelled cluster q it is 1 if
 *             maxlambda(q) == 0 or lambda_v >= maxlambda(q), otherwise (float)(lambda_v / maxlambda(q)).
 *   6 GLOSH   death(c) = max(maxlambda(c), death(d) for d in kids(c)): exact, written to out_cluster_death_lambda, independent of
 *             the options.  With c = point_cluster[v]: score[v] is 0 if death(c) == 0 or lambda_v >= death(c); 1 if death(c) =
 *             +inf; otherwise (float)((death(c) - lambda_v) / death(c)): two separate f64 operations, no FMA.
 *   outputs   out_labels (i32[n]) and out_n_labels are required; out_selected (u8[K]), out_prob (f32[n]), out_outlier_score
 *             (f32[n]) and out_cluster_death_lambda (f64[K]) may be NULL, each on its own.  Nothing is written behind slot K - 1
 *             or n - 1.
 *   refused   HNSWGPU_ERR_ARG, no out slot touched: an unknown method; allow_single_cluster > 1; eps NaN or < 0; n or K above
 *             2^31 - 1; K == 0 with n >= 1; a NULL array that is needed; cluster_parent[0] != UINT32_MAX; cluster_parent[c] >= c
 *             for any c >= 1; a cluster other than 0 with one child, or more than two; point_cluster[v] >= K; a stability that is
 *             NaN or < 0.  The host form checks on the host first.  The device form checks by kernel BEFORE ANY TRAVERSAL: a bad
 *             index is never dereferenced, a malformed parent array can neither fault nor loop.
 *   small     n == 0 writes only *out_n_labels = 0 and needs no device.
 *   same bytes  With allow_single_cluster = 0, eps = 0 and max_cluster_size = 0, on the arrays an hnswhdb_* call wrote, selected,
 *             labels, the bits of prob and the label count are byte for byte that call's own, for both methods.
 *   memory    89 K + 12 n bytes of scratch (the host form: the six arrays besides, 20 K + 8 n) and rocPRIM's temporary storage of
 *             one scan of K + 1 words.
 * One thread per cluster or vertex; the children's S and death climb the cluster tree in one launch over arrival counters, nobody
 * waiting; cluster 0 is decided by one block; "highest ancestor-or-self with a flag" and the epsilon climb are pointer doubling,
 * rounds counted on the host; integer atomics only.  Read back: the check word, then the label count.  Needs no index; legal from
 * several host threads at once.
 * Deviations from scikit-learn 1.7:
 *   - cluster 0's size is cluster_size[0], which is n; sklearn uses the sum of its child clusters' sizes: the two differ only where
 *     max_cluster_size and allow_single_cluster meet.
 *   - HNSWGPU_SELECT_LEAF with allow_single_cluster and K == 1 selects cluster 0; sklearn's code sets that and then clears it again.
 *   - E' is an antichain by construction; sklearn's epsilon_search can return nested clusters when a birth weight equals eps
 *     exactly, and then labels by iteration order.
 * Out of scope: soft clustering, approximate_predict for new points, mcs = 1, labels by DataId, F16 storage, sharding.          */
int hnswhds_select(int device, uint64_t n, uint64_t K,
                   const uint32_t* cluster_parent, const float* cluster_birth_w, const uint32_t* cluster_size, const double* stability,
                   const uint32_t* point_cluster, const float* point_w,
                   uint32_t method, uint32_t allow_single_cluster, float cluster_selection_epsilon, uint64_t max_cluster_size,
                   uint8_t* out_selected, int32_t* out_labels, float* out_prob, float* out_outlier_score,
                   double* out_cluster_death_lambda, uint64_t* out_n_labels);
/* The same with every array in HBM of `device`, on HIP stream `stream`, waited for; out_n_labels stays a host pointer.  Composes
 * with hnswhdb_forest_device / hnswhdb_graph_device on the arrays they wrote: nothing leaves HBM in between.                    */
int hnswhds_select_device(int device, uint64_t n, uint64_t K,
                          const uint32_t* d_cluster_parent, const float* d_cluster_birth_w, const uint32_t* d_cluster_size,
                          const double* d_stability, const uint32_t* d_point_cluster, const float* d_point_w,
                          uint32_t method, uint32_t allow_single_cluster, float cluster_selection_epsilon, uint64_t max_cluster_size,
                          uint8_t* d_out_selected, int32_t* d_out_labels, float* d_out_prob, float* d_out_outlier_score,
                          double* d_out_cluster_death_lambda, uint64_t* out_n_labels, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_HDBSCAN_SELECT_H */
