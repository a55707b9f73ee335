/* hnsw_mi355x_hdbscan.h -- HDBSCAN on the device, an extension of the C ABI of hnsw_mi355x.h in a header of its own: the condensed
 * tree of a forest's single-linkage dendrogram, the stabilities of its clusters, their selection and the flat labels.  Same library
 * (libhnsw_mi355x.so), same conventions: every entry returns an HNSWGPU_* status and leaves its message in hnswgpu_last_error();
 * host forms take host buffers, `_device` forms take HBM buffers and a HIP stream under the stream contract of hnsw_mi355x.h.  The
 * entries carry the prefix hnswhdb_: hnsw_mi355x.h keeps its own set of hnswgpu_* symbols as it is.  The ctypes binding of these
 * entries is generated from THIS file, as that of the others is from hnsw_mi355x.h.                                              */
#ifndef HNSW_MI355X_HDBSCAN_H
#define HNSW_MI355X_HDBSCAN_H

#include "hnsw_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- HDBSCAN: condensed tree, stabilities, flat clusters --- */
/* HDBSCAN (Campello, Moulavi, Sander 2013) from a forest in merge order: the condensed tree of the dendrogram of hnsw_mi355x.h, the stability
 * of every cluster, the selected clusters, and a label and a probability per vertex -- on the device, the dendrogram never leaving HBM.
 *   input     m edges over the vertices 0 .. n - 1, ends a[e], b[e], f32 weights w[e], in merge order, and min_cluster_size (mcs).
 *             The weights must not descend under the order of hnsw_mi355x.h's spanning forest (by value, -0 equal to +0, every NaN
 *             behind +inf).  The dendrogram is hnswgpu_forest_dendrogram's: node x < n is a vertex, node n + e the cluster made by edge e,
 *             with left, right, size.  par[x] is the node whose left or right is x; a node without a parent is a DENDROGRAM ROOT.
 *             A node is BIG iff size >= mcs.
 *   lambda    lambda(w) = 1.0 / (double)w for finite w > 0; +0 for w = +inf or NaN; +inf for w <= 0, -0 included.  Lambda is
 *             therefore non-increasing along the merge order.
 *   clusters  Cluster 0 is the root: born at lambda = 0, of size n, never selected (there is no allow_single_cluster).  The
 *             dendrogram roots are joined under cluster 0 at weight +inf: if exactly one of them is big it CONTINUES cluster 0; if
 *             two or more are big each is a HEAD, a child cluster of 0 born at weight +inf; a small dendrogram root's vertices
 *             leave cluster 0 at weight +inf.  A big node x with a parent is a head iff both children of par[x] are big (a true
 *             split); otherwise it continues the cluster of par[x].  Heads are numbered 1 .. K - 1 by descending node id, so a
 *             parent cluster always has the smaller index; the numbering is unique.  K <= max(1, 2 floor(n / mcs) - 1) =
 *             hnswhdb_max_clusters(n, mcs): callers size the per-cluster arrays with it.
 *   cluster   cluster_parent[c] (UINT32_MAX for cluster 0); cluster_birth_w[c], the stored f32 bits of the split edge's weight
 *             (+inf for cluster 0 and its children); cluster_size[c]; stability[c], f64; selected[c], u8.
 *   vertex    with t the highest small ancestor-or-self of v: point_cluster[v] is the cluster of par[t], or 0 if t is a dendrogram
 *             root; point_w[v] is the stored bits of w[par[t] - n], or +inf bits if t is a dendrogram root.
 *   stability The rows of cluster C are its points (size 1, lambda of point_w) and its child clusters (their size, lambda of their
 *             birth).  A row's term is 0 when lambda_row == lambda_birth(C) (this covers inf - inf), else (lambda_row -
 *             lambda_birth(C)) * (double)size: three separate correctly rounded f64 operations, no FMA.  stability[C] is the f64 sum of
 *             the terms; all are >= 0, no NaN arises.  The order of summation is this library's own, a function of the input alone:
 *             two calls return the same bytes (and |stability[C] - exact sum| <= rows(C) 2^-53 exact sum).
 *   selection method = HNSWGPU_SELECT_EOM: S(C) = max(stability[C], sum of S over the children); C WINS iff stability[C] >= that
 *             sum (ties go to the parent, as in sklearn; a cluster without a child always wins); selected[C] iff C != 0, C wins
 *             and no proper ancestor other than 0 wins.  method = HNSWGPU_SELECT_LEAF: selected[C] iff C != 0 and C has no child.
 *   labels    Selected clusters are numbered 0 .. L - 1 by ascending cluster index.  labels[v] (i32) is the label of the selected
 *             ancestor-or-self of point_cluster[v], or -1 if there is none.  maxlambda(C) is the maximum lambda over the rows of C
 *             (exact).  prob[v] (f32) is 0 if labels[v] = -1; 1 if maxlambda = 0 or lambda_v >= maxlambda; otherwise
 *             (float)(lambda_v / maxlambda), maxlambda taken of the labelled cluster.  *out_n_clusters = K, *out_n_labels = L.
 *             Nothing is written behind slot K - 1 of a per-cluster array.  out_labels and the two counts are required; every
 *             other out array may be NULL.
 *   refused   HNSWGPU_ERR_ARG, no out slot touched: mcs < 2 or mcs > 2^31 - 1; an unknown method; a NULL array that is needed;
 *             weights that descend; everything hnswgpu_forest_dendrogram refuses (n > 2^31 - 1, too many edges, a bad end, a
 *             self-loop, a cycle).  The host form checks ends, self-loops and weights on the host first.
 *   small     n == 0 writes only the two counts (0, 0) and needs no device.  m == 0 with n >= 1: K = 1, every vertex in cluster 0
 *             at +inf, all labels -1.
 *   memory    the dendrogram's, then 20 (n + m) + 40 n + 109 K' bytes with K' = hnswhdb_max_clusters (node parents,
 *             chains, head flags and their scan; points; rows twice; clusters) and rocPRIM's temporary storage of one sort of
 *             n + K rows and one scan of n + m words.
 * Chains of the dendrogram are found by the lock-free union-find of the graph sections of hnsw_mi355x.h (no walk of O(depth)); the rows are sorted by
 * cluster and summed in a fixed shape; the selection climbs the cluster tree in one launch over arrival counters, nobody waiting;
 * integer atomics only.  Read back: the dendrogram's word, then the descent flag with K, then L.  Needs no index; legal from
 * several host threads at once.
 * Out of scope: allow_single_cluster, cluster_selection_epsilon, max_cluster_size, mcs = 1, GLOSH outlier scores, soft clustering,
 * labels by DataId, F16 storage, sharding.                                                                                      */
#define HNSWGPU_SELECT_EOM 0
#define HNSWGPU_SELECT_LEAF 1
/* max(1, 2 floor(n / min_cluster_size) - 1); 0 for min_cluster_size == 0.  Pure: needs no device.                               */
uint64_t hnswhdb_max_clusters(uint64_t n, uint64_t min_cluster_size);
int hnswhdb_forest(int device, uint64_t n, uint64_t m, const uint32_t* a, const uint32_t* b, const float* w,
                           uint64_t min_cluster_size, uint32_t method,
                           int32_t* out_labels, float* out_prob, uint32_t* out_point_cluster, float* out_point_w,
                           uint32_t* out_cluster_parent, float* out_cluster_birth_w, uint32_t* out_cluster_size,
                           double* out_stability, uint8_t* out_selected, uint64_t* out_n_clusters, uint64_t* out_n_labels);
/* The same with every array in HBM of `device`, on HIP stream `stream`, waited for; the two counts stay host pointers.  Ends and
 * self-loops are checked by the dendrogram's kernel, the weights by one of this call's: a bad input is HNSWGPU_ERR_ARG, never a fault. */
int hnswhdb_forest_device(int device, uint64_t n, uint64_t m, const uint32_t* d_a, const uint32_t* d_b, const float* d_w,
                                  uint64_t min_cluster_size, uint32_t method,
                                  int32_t* d_out_labels, float* d_out_prob, uint32_t* d_out_point_cluster, float* d_out_point_w,
                                  uint32_t* d_out_cluster_parent, float* d_out_cluster_birth_w, uint32_t* d_out_cluster_size,
                                  double* d_out_stability, uint8_t* d_out_selected, uint64_t* out_n_clusters, uint64_t* out_n_labels,
                                  void* stream);
/* hnswgpu_graph_dendrogram followed by the clusters of its dendrogram, which never leaves HBM in between: HDBSCAN of the indexed
 * points over the k-NN graph, core_k the mutual-reachability parameter (sklearn's min_samples counts the point itself: core_k =
 * min_samples - 1).  Vertices are POSITIONS.  Its refusals are hnswgpu_graph_dendrogram's in the same words -- except that out_a,
 * out_b, out_w, out_left, out_right and out_size are OPTIONAL here (NULL allowed, each on its own) --, followed by the new ones
 * above.  Where given, those six and *out_n_edges are byte for byte what hnswgpu_graph_dendrogram writes with the same arguments
 * (max(n - 1, 0) slots).  An empty index: the three counts are 0, HNSWGPU_OK, nothing else written.  On any error no out slot is
 * touched.  Takes the handle's lock shared; host buffers; uploads the index on first use.                                      */
int hnswhdb_graph(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k,
                          uint64_t min_cluster_size, uint32_t method,
                          uint32_t* out_a, uint32_t* out_b, float* out_w, uint32_t* out_left, uint32_t* out_right, uint32_t* out_size,
                          int32_t* out_labels, float* out_prob, uint32_t* out_point_cluster, float* out_point_w,
                          uint32_t* out_cluster_parent, float* out_cluster_birth_w, uint32_t* out_cluster_size,
                          double* out_stability, uint8_t* out_selected, uint64_t* out_n_clusters, uint64_t* out_n_labels,
                          uint64_t* out_n_edges);
/* The same with every array in HBM, on HIP stream `stream`, waited for; the three counts stay host pointers.  The index must be
 * uploaded (else HNSWGPU_ERR_DEVICE).                                                                                          */
int hnswhdb_graph_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k,
                                 uint64_t min_cluster_size, uint32_t method,
                                 uint32_t* d_out_a, uint32_t* d_out_b, float* d_out_w, uint32_t* d_out_left, uint32_t* d_out_right,
                                 uint32_t* d_out_size,
                                 int32_t* d_out_labels, float* d_out_prob, uint32_t* d_out_point_cluster, float* d_out_point_w,
                                 uint32_t* d_out_cluster_parent, float* d_out_cluster_birth_w, uint32_t* d_out_cluster_size,
                                 double* d_out_stability, uint8_t* d_out_selected, uint64_t* out_n_clusters, uint64_t* out_n_labels,
                                 uint64_t* out_n_edges, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HNSW_MI355X_HDBSCAN_H */
