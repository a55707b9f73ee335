"""Host-side mirror of the reference's interface for the search path, on top of the C ABI.

Same names and argument meaning as the Rust crate (so the parity tests read like the crate's tests):

    hnsw_rs::hnsw::Hnsw<f32, D>        -> Hnsw(max_nb_connection, max_elements, max_layer, ef_construction, "DistL2")
        .insert / .parallel_insert                      src/hnsw.rs:1069, :1224
        .search(data, knbn, ef)                         src/hnsw.rs:1597
        .parallel_search(datas, knbn, ef)               src/hnsw.rs:1612
    hnsw_rs::api::AnnT                 -> .search_neighbours / .parallel_search_neighbours / .file_dump
                                                        src/api.rs:13-38
    hnsw_rs::hnswio::HnswIo            -> HnswIo(directory, basename).load_hnsw("DistL2")
                                                        src/hnswio.rs:317, :431
    hnsw_rs::hnsw::Neighbour           -> Neighbour(d_id, distance, p_id=(layer, rank))   src/hnsw.rs:98-107

All searches run on the MI355X through libhnsw_mi355x.so; nothing here computes a distance.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native as N

Neighbour = namedtuple("Neighbour", ["d_id", "distance", "p_id"])  # p_id = (layer, rank)


def _recall(got, exact):
    """(by distance, by id) of the answers `got` against the exact answers `exact` (Hnsw.recall_flat has the definition)"""
    total = int(exact.counts.sum())
    if total == 0:
        return 1.0, 1.0
    by_dist = by_id = 0
    for q in range(len(exact.counts)):
        ce, cg = int(exact.counts[q]), int(got.counts[q])
        if ce == 0:
            continue
        by_dist += int(np.count_nonzero(got.dists[q, :cg] <= exact.dists[q, ce - 1]))
        by_id += len(np.intersect1d(got.ids[q, :cg], exact.ids[q, :ce]))
    return by_dist / total, by_id / total


def _pack_filter_set(datas, filters, filter_of):
    """The arguments of the filter-set calls, checked and packed: the (nq, d) f32 matrix, the filters' ids behind one another
    with their CSR offsets, one u32 filter index per query (filter_of=None: one filter per query in order)."""
    datas = np.ascontiguousarray(datas, dtype=np.float32)
    if datas.ndim != 2:
        raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
    nq, d = datas.shape
    filters = [np.ascontiguousarray(f, dtype=np.uint64).reshape(-1) for f in filters]
    if filter_of is None:
        if len(filters) != nq:
            raise HnswError(N.ERR_ARG, f"filter_of=None means one filter per query: {len(filters)} filters for {nq} queries")
        filter_of = np.arange(nq, dtype=np.uint32)
    else:
        fo = np.asarray(filter_of)
        if fo.shape != (nq,):
            raise HnswError(N.ERR_ARG, "filter_of must hold one filter index per query")
        if nq and (fo.min() < 0 or fo.max() > 0xFFFFFFFF):
            raise HnswError(N.ERR_ARG, "filter_of holds an index that names no filter")
        filter_of = np.ascontiguousarray(fo, dtype=np.uint32)
    offsets = np.zeros(len(filters) + 1, np.uint64)
    if filters:
        np.cumsum([len(f) for f in filters], out=offsets[1:])
    flat = np.concatenate(filters) if filters else np.zeros(0, np.uint64)
    if len(flat) == 0:
        flat = np.zeros(1, np.uint64)  # (never read: every filter is empty)
    return datas, flat, offsets, filter_of


class HnswError(RuntimeError):
    """anyhow::Error analogue: carries the status code of the failing C-ABI call."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _check(rc):
    if rc != N.OK:
        raise HnswError(rc, N.last_error())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class BatchResult:
    """Flat form of Vec<Vec<Neighbour>>: row i holds counts[i] valid entries, ascending distance.
    status (filtered search only): 1 where the reference panics on the query (src/hnsw.rs:973), else 0."""

    def __init__(self, ids, dists, layers, ranks, counts, status=None):
        self.ids, self.dists, self.layers, self.ranks, self.counts = ids, dists, layers, ranks, counts
        self.status = status

    def to_neighbours(self):
        out = []
        for i in range(len(self.counts)):
            c = int(self.counts[i])
            out.append([Neighbour(int(self.ids[i, j]), float(self.dists[i, j]),
                                  (int(self.layers[i, j]), int(self.ranks[i, j]))) for j in range(c)])
        return out


class RangeResult:
    """The answers of a range search in CSR form: query q owns the slots offsets[q] .. offsets[q + 1] of ids, dists, layers and
    ranks, ascending by (distance, origin id).  An approximate range search (Hnsw.range_search_flat) also gives, per query, .ef
    (the ef at which it settled) and .flags (bit 0: saturated -- the result set was full and inside the ball at ef_max); its answers
    are in the search's own order."""

    def __init__(self, offsets, ids, dists, layers, ranks, ef=None, flags=None):
        self.offsets, self.ids, self.dists, self.layers, self.ranks = offsets, ids, dists, layers, ranks
        self.ef, self.flags = ef, flags

    @property
    def counts(self):
        return np.diff(self.offsets)

    def of(self, q):
        """(ids, dists, layers, ranks) of query q: views, not copies"""
        a, b = int(self.offsets[q]), int(self.offsets[q + 1])
        return self.ids[a:b], self.dists[a:b], self.layers[a:b], self.ranks[a:b]

    def to_neighbours(self):
        out = []
        for q in range(len(self.offsets) - 1):
            ids, dists, layers, ranks = self.of(q)
            out.append([Neighbour(int(ids[j]), float(dists[j]), (int(layers[j]), int(ranks[j]))) for j in range(len(ids))])
        return out


class GraphCsrResult:
    """An undirected k-NN graph of the indexed points in CSR form (Hnsw.symmetric_knn_graph_flat).  Vertices are POSITIONS in the
    ascending (DataId, dump order) order -- DataIds may repeat, positions do not.  Row i owns the slots offsets[i] .. offsets[i + 1]
    of pos (the neighbours' positions), ids (their DataIds), dists (the stored f32 distances), layers and ranks (their p_ids),
    ascending by (distance, position)."""

    def __init__(self, offsets, pos, ids, dists, layers, ranks):
        self.offsets, self.pos, self.ids, self.dists, self.layers, self.ranks = offsets, pos, ids, dists, layers, ranks

    @property
    def counts(self):
        return np.diff(self.offsets)

    def of(self, i):
        """(pos, ids, dists, layers, ranks) of row i: views, not copies"""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.pos[a:b], self.ids[a:b], self.dists[a:b], self.layers[a:b], self.ranks[a:b]

    def to_neighbours(self):
        out = []
        for i in range(len(self.offsets) - 1):
            _pos, ids, dists, layers, ranks = self.of(i)
            out.append([Neighbour(int(ids[j]), float(dists[j]), (int(layers[j]), int(ranks[j]))) for j in range(len(ids))])
        return out


class ComponentsResult:
    """The connected components of a graph (Hnsw.knn_graph_components, csr_components): labels[v] is the component of vertex v,
    components numbered 0 .. n_components - 1 by their smallest vertex, ascending; sizes[c] is the number of vertices of c."""

    def __init__(self, labels, sizes, n_components):
        self.labels, self.sizes, self.n_components = labels, sizes, n_components


def _cut(max_dist):
    """the one f32 behind the max_dist pointer (the caller keeps it alive over the call), or None"""
    return None if max_dist is None else np.array([max_dist], np.float32)


def csr_components(offsets, cols, dists=None, max_dist=None, device=0):
    """The connected components of ANY graph given in CSR (offsets u64[n + 1], cols u32[offsets[n]]), labelled on `device`: every
    entry (r, c) joins r and c, whichever row names it, so a directed CSR gets its weakly connected components.  With max_dist an
    entry counts iff its f32 in dists is <= max_dist (a NaN never is).  Returns a ComponentsResult."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    if dists is not None:
        dists = np.ascontiguousarray(dists, dtype=np.float32)
        if len(dists) != len(cols):
            raise HnswError(N.ERR_ARG, f"dists has {len(dists)} entries, cols has {len(cols)}")
    if len(offsets) == 0 or int(offsets[-1]) > len(cols):
        raise HnswError(N.ERR_ARG, "offsets must hold n + 1 entries, the last one at most len(cols)")
    n = len(offsets) - 1
    labels, sizes, c = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.uint64)
    cut = _cut(max_dist)
    if dists is not None and len(dists) == 0:
        dists = np.zeros(1, np.float32)  # (never read: there is no entry)
    _check(N.lib().hnswgpu_csr_components(device, n, _p(offsets), _p(cols) if len(cols) else None, _p(dists), _p(cut), _p(labels), _p(sizes), _p(c)))
    return ComponentsResult(labels, sizes[:int(c[0])].copy(), int(c[0]))


class DbscanResult:
    """DBSCAN(eps, min_samples) as include/hnsw_mi355x_dbscan.h defines it (Hnsw.dbscan, csr_dbscan), indexed by POSITION like
    ComponentsResult: labels (i32, the cluster, -1: noise), core (bool), counts (u32, the size of the point's set), anchors (u32: a
    core point itself, otherwise the nearest core point of its own set, UINT32_MAX for noise); clusters are numbered
    0 .. n_clusters - 1 by their smallest core position, ascending."""

    def __init__(self, labels, core, counts, anchors, n_clusters):
        self.labels, self.core, self.counts, self.anchors, self.n_clusters = labels, core, counts, anchors, n_clusters


def _dbscan_params(eps, min_samples):
    if np.isnan(np.float32(eps)):
        raise HnswError(N.ERR_ARG, "eps is NaN")
    if int(min_samples) < 1:
        raise HnswError(N.ERR_ARG, "min_samples must be > 0")
    return float(np.float32(eps)), int(min_samples)


def _dbscan_arrays(n):
    return np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.uint64)


def csr_dbscan(offsets, cols, dists=None, eps=float("inf"), min_samples=1, add_self=False, device=0):
    """DBSCAN over ANY neighbour lists given in CSR by position (offsets u64[n + 1], cols u32[offsets[n]]), on `device`: entry e of
    row i is in the set of i iff dists is None or dists[e] <= eps (a NaN never is); add_self adds the point itself to every count
    (k-NN rows that never name their own point).  A point that is not core reads its OWN row only.  Returns a DbscanResult."""
    eps, min_samples = _dbscan_params(eps, min_samples)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    if dists is not None:
        dists = np.ascontiguousarray(dists, dtype=np.float32)
        if len(dists) != len(cols):
            raise HnswError(N.ERR_ARG, f"dists has {len(dists)} entries, cols has {len(cols)}")
    if len(offsets) == 0 or int(offsets[-1]) > len(cols):
        raise HnswError(N.ERR_ARG, "offsets must hold n + 1 entries, the last one at most len(cols)")
    n = len(offsets) - 1
    labels, core, counts, anchors, c = _dbscan_arrays(n)
    if dists is not None and len(dists) == 0:
        dists = np.zeros(1, np.float32)  # (never read: there is no entry)
    _check(N.lib().hnswdbs_csr(device, n, _p(offsets), _p(cols) if len(cols) else None, _p(dists), eps, min_samples, 1 if add_self else 0,
                               _p(labels), _p(core), _p(counts), _p(anchors), _p(c)))
    return DbscanResult(labels, core.astype(bool), counts, anchors, int(c[0]))


class SpanningForestResult:
    """The minimum spanning forest of a graph (Hnsw.knn_graph_spanning_forest, csr_spanning_forest): n_edges edges, edge e joining
    vertices a[e] < b[e] with weight weights[e] (f32, the bits as the graph stores them), ascending by (weight, a, b).  Read in this
    order the edges are the merges of the single-linkage hierarchy; labels_at cuts it at a radius."""

    def __init__(self, a, b, weights, n_edges, n_vertices=None):
        self.a, self.b, self.weights, self.n_edges = a, b, weights, n_edges
        self.n_vertices = n_vertices if n_vertices is not None else (int(max(a.max(), b.max())) + 1 if n_edges else 0)

    def labels_at(self, max_dist=None):
        """The components of the forest edges whose weight is <= max_dist (None: every edge, a NaN weight included; otherwise an
        ordered f32 comparison, which a NaN never passes), as a ComponentsResult: a host union-find, components numbered by
        their smallest position."""
        n = self.n_vertices
        keep = np.ones(self.n_edges, bool) if max_dist is None else (self.weights[:self.n_edges] <= np.float32(max_dist))
        parent = list(range(n))

        def find(v):
            while parent[v] != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v
        for x, y in zip(self.a[:self.n_edges][keep].tolist(), self.b[:self.n_edges][keep].tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
        labels, sizes, number = np.zeros(n, np.uint32), [], {}
        for v in range(n):
            r = find(v)
            if r not in number:  # (r == v: a root is the smallest vertex of its tree)
                number[r] = len(sizes)
                sizes.append(0)
            labels[v] = number[r]
            sizes[number[r]] += 1
        return ComponentsResult(labels, np.array(sizes, np.uint32), len(sizes))

    def dendrogram(self, device=0):
        """The single-linkage dendrogram of this forest's edges in their order (forest_dendrogram), with the edges and weights
        carried along: a DendrogramResult."""
        m = self.n_edges
        d = forest_dendrogram(self.n_vertices, self.a[:m], self.b[:m], device)
        return DendrogramResult(d.left, d.right, d.sizes, m, self.n_vertices, self.a[:m], self.b[:m], self.weights[:m])

    def hdbscan(self, min_cluster_size, method="eom", device=0, allow_single_cluster=False, cluster_selection_epsilon=0.0, max_cluster_size=None,
                outlier_scores=False):
        """HDBSCAN's clusters of this forest's edges in their order (forest_hdbscan, its options included): an HdbscanResult."""
        m = self.n_edges
        return forest_hdbscan(self.n_vertices, self.a[:m], self.b[:m], self.weights[:m], min_cluster_size, method, device, allow_single_cluster,
                              cluster_selection_epsilon, max_cluster_size, outlier_scores)


class DendrogramResult:
    """The single-linkage dendrogram of a forest (forest_dendrogram, SpanningForestResult.dendrogram, Hnsw.knn_graph_dendrogram):
    merge e joins the clusters left[e] and right[e] into cluster n_vertices + e of sizes[e] vertices.  Cluster ids are scipy's: an
    id below n_vertices is that vertex alone.  a, b, weights: the forest's edges where the call had them, else None."""

    def __init__(self, left, right, sizes, n_edges, n_vertices, a=None, b=None, weights=None):
        self.left, self.right, self.sizes, self.n_edges, self.n_vertices = left, right, sizes, n_edges, n_vertices
        self.a, self.b, self.weights = a, b, weights

    def linkage(self):
        """scipy's linkage matrix, float64[n_edges, 4]: left, right, weight, size.  (scipy itself accepts it when the forest is
        connected and the weights ascend, which a minimum spanning forest's do.)"""
        if self.weights is None:
            raise HnswError(N.ERR_ARG, "linkage() needs the merges' heights: this dendrogram was made without weights")
        m = self.n_edges
        z = np.empty((m, 4), np.float64)
        z[:, 0], z[:, 1], z[:, 2], z[:, 3] = self.left[:m], self.right[:m], self.weights[:m], self.sizes[:m]
        return z

    def roots(self):
        """The ids of the clusters that are nobody's child, ascending: one per component of the forest."""
        m = self.n_edges
        child = np.zeros(self.n_vertices + m, bool)
        child[self.left[:m]] = True
        child[self.right[:m]] = True
        return np.flatnonzero(~child).astype(np.uint32)


def forest_dendrogram(n, a, b, device=0):
    """The dendrogram of the forest whose edge e joins vertices a[e] and b[e] of 0 .. n - 1, built on `device`: the edges' order is
    the merge order.  Refuses (HnswError, ERR_ARG) an end >= n, a self-loop, more than n - 1 edges and a cycle.  Returns a
    DendrogramResult without a, b and weights."""
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1)
    if len(a) != len(b):
        raise HnswError(N.ERR_ARG, f"a has {len(a)} entries, b has {len(b)}")
    m = len(a)
    left, right, sizes = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    _check(N.lib().hnswgpu_forest_dendrogram(device, n, m, _p(a) if m else None, _p(b) if m else None, _p(left) if m else None,
                                             _p(right) if m else None, _p(sizes) if m else None))
    return DendrogramResult(left, right, sizes, m, n)


def _lambda_of(w):
    """HDBSCAN's lambda of f32 weights, f64: 1 / w; 0 for +inf and NaN; +inf for w <= 0"""
    w = np.asarray(w, np.float32)
    lam = np.zeros(w.shape, np.float64)
    pos = np.isfinite(w) & (w > 0)
    lam[pos] = 1.0 / w[pos].astype(np.float64)
    lam[w <= 0] = np.inf
    return lam


class HdbscanResult:
    """HDBSCAN's answer (forest_hdbscan, SpanningForestResult.hdbscan, Hnsw.hdbscan), as include/hnsw_mi355x_hdbscan.h defines it.  Per
    vertex: labels (i32, -1: noise), probabilities (f32), point_cluster and point_w (the cluster of the condensed tree that the
    vertex leaves, and the f32 weight at which it does).  Per cluster of the condensed tree, n_clusters of them, cluster 0 the
    root: cluster_parent (0xFFFFFFFF for cluster 0), cluster_birth_w, cluster_size, stability (f64), selected (bool).  n_labels
    selected clusters, numbered by ascending cluster index.  forest (a SpanningForestResult) and dendrogram (a DendrogramResult)
    are there where the call produced them (Hnsw.hdbscan), else None.  outlier_scores (f32 per vertex, GLOSH) and
    cluster_death_lambda (f64 per cluster) are there on results that went through select(), else None."""

    def __init__(self, labels, probabilities, point_cluster, point_w, cluster_parent, cluster_birth_w, cluster_size, stability, selected,
                 n_clusters, n_labels, forest=None, dendrogram=None, outlier_scores=None, cluster_death_lambda=None):
        self.labels, self.probabilities, self.point_cluster, self.point_w = labels, probabilities, point_cluster, point_w
        self.cluster_parent, self.cluster_birth_w, self.cluster_size = cluster_parent, cluster_birth_w, cluster_size
        self.stability, self.selected, self.n_clusters, self.n_labels = stability, selected, n_clusters, n_labels
        self.forest, self.dendrogram = forest, dendrogram
        self.outlier_scores, self.cluster_death_lambda = outlier_scores, cluster_death_lambda
        self.knn_params = None  # Hnsw.hdbscan: the (knbn, ef, core_k) it ran with, what Hnsw.hdbscan_predict defaults to

    def select(self, method="eom", allow_single_cluster=False, cluster_selection_epsilon=0.0, max_cluster_size=None, device=0):
        """The selection made again on this result's condensed tree, on `device`, without the tree being made again
        (include/hnsw_mi355x_hdbscan_select.h): method "eom" or "leaf"; allow_single_cluster: cluster 0 may be selected;
        cluster_selection_epsilon: a weight, selected clusters born below it climb to the ancestor born above it;
        max_cluster_size: None, or the largest size an excess-of-mass winner may have.  Returns a new HdbscanResult over the same
        tree arrays with selected, labels, probabilities and n_labels of its own, outlier_scores (GLOSH) and
        cluster_death_lambda."""
        code = _hdbscan_method(method)
        if max_cluster_size is None:
            max_size = 0
        elif max_cluster_size != int(max_cluster_size) or not 1 <= max_cluster_size < 1 << 64:
            raise HnswError(N.ERR_ARG, f"max_cluster_size = {max_cluster_size}: None, or a size of 1 or more")
        else:
            max_size = int(max_cluster_size)
        n, k = len(self.labels), int(self.n_clusters)
        tree = [np.ascontiguousarray(x[:k], dtype=t) for x, t in ((self.cluster_parent, np.uint32), (self.cluster_birth_w, np.float32),
                                                                  (self.cluster_size, np.uint32), (self.stability, np.float64))]
        points = [np.ascontiguousarray(self.point_cluster[:n], dtype=np.uint32), np.ascontiguousarray(self.point_w[:n], dtype=np.float32)]
        selected, death = np.zeros(max(k, 1), np.uint8), np.zeros(max(k, 1), np.float64)
        labels, prob, score = np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        n_labels = np.zeros(1, np.uint64)
        _check(N.lib().hnswhds_select(device, n, k, *[_p(x) if len(x) else None for x in tree + points], code, int(bool(allow_single_cluster)),
                                      float(cluster_selection_epsilon), max_size, _p(selected), _p(labels), _p(prob), _p(score), _p(death),
                                      _p(n_labels)))
        res = HdbscanResult(labels[:n].copy(), prob[:n].copy(), self.point_cluster, self.point_w, self.cluster_parent, self.cluster_birth_w,
                            self.cluster_size, self.stability, selected[:k].astype(bool), k, int(n_labels[0]), self.forest, self.dendrogram,
                            score[:n].copy(), death[:k].copy())
        res.knn_params = self.knn_params
        return res

    def condensed_tree(self):
        """The condensed tree as rows (parent, child, lambda, child_size) in sklearn's CONDENSED_dtype layout ('parent' and 'child'
        intp, 'value' f64, 'cluster_size' intp): cluster c is numbered n + c; first the clusters 1 .. n_clusters - 1 as children of
        their parents, then the vertices."""
        n, k = len(self.labels), self.n_clusters
        dtype = np.dtype([("parent", np.intp), ("child", np.intp), ("value", np.float64), ("cluster_size", np.intp)])
        rows = np.zeros(max(k - 1, 0) + n, dtype)
        c = np.arange(1, max(k, 1))
        rows["parent"][:len(c)] = n + self.cluster_parent[1:k].astype(np.intp)
        rows["child"][:len(c)] = n + c
        rows["value"][:len(c)] = _lambda_of(self.cluster_birth_w[1:k])
        rows["cluster_size"][:len(c)] = self.cluster_size[1:k]
        rows["parent"][len(c):] = n + self.point_cluster.astype(np.intp)
        rows["child"][len(c):] = np.arange(n)
        rows["value"][len(c):] = _lambda_of(self.point_w)
        rows["cluster_size"][len(c):] = 1
        return rows


class PredictResult:
    """The assignment of nq new points to the clusters of an HdbscanResult (hdbscan_assign, Hnsw.hdbscan_predict), as
    include/hnsw_mi355x_hdbscan_predict.h defines it.  Per query: labels (i32, the stored points' labels, -1: noise), probabilities
    (f32), outlier_scores (f32, GLOSH; None unless the result holds cluster_death_lambda), nearest (u32, the POSITION of the nearest
    stored point under mutual reachability, 0xFFFFFFFF for a query without a neighbour), weights (f32, that mutual-reachability
    distance) and clusters (u32, the cluster of the condensed tree the query falls into)."""

    def __init__(self, labels, probabilities, outlier_scores, nearest, weights, clusters):
        self.labels, self.probabilities, self.outlier_scores = labels, probabilities, outlier_scores
        self.nearest, self.weights, self.clusters = nearest, weights, clusters


class _PredictArrays:
    """the tree arguments and the out arrays of one hnswhdp_assign / hnswhdp_predict call over nq queries"""

    def __init__(self, result, core, nq, cluster_selection_epsilon):
        n, k = len(result.labels), int(result.n_clusters)
        self.n, self.k, self.nq, self.eps = n, k, nq, float(cluster_selection_epsilon)
        core = np.ascontiguousarray(core, dtype=np.float32).reshape(-1)
        if len(core) != n:
            raise HnswError(N.ERR_ARG, f"core has {len(core)} entries, the result has {n} vertices")
        self.inputs = [core, np.ascontiguousarray(result.cluster_parent[:k], dtype=np.uint32),
                       np.ascontiguousarray(result.cluster_birth_w[:k], dtype=np.float32),
                       np.ascontiguousarray(result.point_cluster[:n], dtype=np.uint32), np.ascontiguousarray(result.point_w[:n], dtype=np.float32),
                       np.ascontiguousarray(result.selected[:k], dtype=np.uint8)]
        death = result.cluster_death_lambda
        self.death = None if death is None else np.ascontiguousarray(death[:k] if k else np.zeros(1), dtype=np.float64)  # (K == 0: never read)
        m = max(nq, 1)
        self.labels, self.prob = np.full(m, -1, np.int32), np.zeros(m, np.float32)
        self.score = None if self.death is None else np.zeros(m, np.float32)
        self.nearest, self.w, self.cluster = np.zeros(m, np.uint32), np.zeros(m, np.float32), np.zeros(m, np.uint32)

    def tree(self):
        """(core, K, cluster_parent, cluster_birth_w, point_cluster, point_w, selected, eps, death): a call's arguments between core_k
        / n and the outputs"""
        core, parent, birth, pc, pw, sel = [_p(x) if len(x) else None for x in self.inputs]
        return (core, self.k, parent, birth, pc, pw, sel, self.eps, None if self.death is None else _p(self.death))

    def outputs(self):
        return (_p(self.labels), _p(self.prob), None if self.score is None else _p(self.score), _p(self.nearest), _p(self.w), _p(self.cluster))

    def result(self):
        nq = self.nq
        return PredictResult(self.labels[:nq].copy(), self.prob[:nq].copy(), None if self.score is None else self.score[:nq].copy(),
                             self.nearest[:nq].copy(), self.w[:nq].copy(), self.cluster[:nq].copy())


def hdbscan_assign(result, core, nbr_pos, nbr_dist, counts, core_k, cluster_selection_epsilon=0.0, device=0):
    """New points assigned to the clusters of `result` (an HdbscanResult) from their neighbour rows, on `device`, no index needed
    (include/hnsw_mi355x_hdbscan_predict.h, hnswhdp_assign): nbr_pos (nq, knbn) u32 POSITIONS of stored points, nbr_dist (nq, knbn)
    f32 and counts (nq) the used slots of each row; core (n) the stored points' core distances (Hnsw.core_distances) and core_k the
    slot of a row that is the query's own; cluster_selection_epsilon as the selection had it.  Returns a PredictResult."""
    nbr_pos = np.ascontiguousarray(nbr_pos, dtype=np.uint32)
    nbr_dist = np.ascontiguousarray(nbr_dist, dtype=np.float32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    if nbr_pos.ndim != 2 or nbr_pos.shape != nbr_dist.shape or len(counts) != nbr_pos.shape[0]:
        raise HnswError(N.ERR_ARG, "nbr_pos and nbr_dist must be (nq, knbn) matrices of one shape, counts (nq)")
    nq, knbn = nbr_pos.shape
    o = _PredictArrays(result, core, nq, cluster_selection_epsilon)
    rows = [_p(x) if x.size else None for x in (nbr_pos, nbr_dist, counts)]
    _check(N.lib().hnswhdp_assign(device, nq, knbn, *rows, core_k, o.n, *o.tree(), *o.outputs()))
    return o.result()


_METHODS = {"eom": "HNSWGPU_SELECT_EOM", "leaf": "HNSWGPU_SELECT_LEAF"}


def _select_behind(result, method, device, allow_single_cluster, cluster_selection_epsilon, max_cluster_size, outlier_scores):
    """what the hdbscan calls return: `result` as it is under the default options, else its select()"""
    if not allow_single_cluster and cluster_selection_epsilon == 0 and max_cluster_size is None and not outlier_scores:
        return result
    return result.select(method, allow_single_cluster, cluster_selection_epsilon, max_cluster_size, device)


def _hdbscan_method(method):
    if method not in _METHODS:
        raise HnswError(N.ERR_ARG, f"method must be 'eom' or 'leaf', not {method!r}")
    return N.HDBSCAN_HEADER.constants[_METHODS[method]]


class _HdbscanArrays:
    """the out arrays of one hdbscan call over n vertices"""

    def __init__(self, n, min_cluster_size):
        if min_cluster_size != int(min_cluster_size) or not 2 <= min_cluster_size <= 0x7FFFFFFF:
            raise HnswError(N.ERR_ARG, f"min_cluster_size = {min_cluster_size}: it must be in 2 .. 2^31 - 1")
        k = max(int(N.lib().hnswhdb_max_clusters(n, int(min_cluster_size))), 1)
        self.labels, self.prob = np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.float32)
        self.point_cluster, self.point_w = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float32)
        self.parent, self.birth, self.size = np.zeros(k, np.uint32), np.zeros(k, np.float32), np.zeros(k, np.uint32)
        self.stability, self.selected = np.zeros(k, np.float64), np.zeros(k, np.uint8)
        self.n_clusters, self.n_labels = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        self.n = n

    def pointers(self):
        return (_p(self.labels), _p(self.prob), _p(self.point_cluster), _p(self.point_w), _p(self.parent), _p(self.birth), _p(self.size),
                _p(self.stability), _p(self.selected), _p(self.n_clusters), _p(self.n_labels))

    def result(self, forest=None, dendrogram=None):
        n, k = self.n, int(self.n_clusters[0])
        return HdbscanResult(self.labels[:n].copy(), self.prob[:n].copy(), self.point_cluster[:n].copy(), self.point_w[:n].copy(),
                             self.parent[:k].copy(), self.birth[:k].copy(), self.size[:k].copy(), self.stability[:k].copy(),
                             self.selected[:k].astype(bool), k, int(self.n_labels[0]), forest, dendrogram)


def forest_hdbscan(n, a, b, weights, min_cluster_size, method="eom", device=0, allow_single_cluster=False, cluster_selection_epsilon=0.0,
                   max_cluster_size=None, outlier_scores=False):
    """HDBSCAN's clusters of the forest whose edge e joins vertices a[e] and b[e] of 0 .. n - 1 with weight weights[e] (f32), on
    `device`: the edges' order is the merge order and the weights must not descend.  method: "eom" (excess of mass) or "leaf".
    Refuses (HnswError, ERR_ARG) what forest_dendrogram refuses, weights that descend and a min_cluster_size outside 2 .. 2^31 - 1.
    Returns an HdbscanResult.  allow_single_cluster, cluster_selection_epsilon, max_cluster_size and outlier_scores are
    HdbscanResult.select's: at their defaults the answer is hnswhdb_forest's own, otherwise select() runs behind it."""
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if len(a) != len(b) or len(a) != len(w):
        raise HnswError(N.ERR_ARG, f"a has {len(a)} entries, b has {len(b)}, weights has {len(w)}")
    m, code = len(a), _hdbscan_method(method)
    o = _HdbscanArrays(n, min_cluster_size)
    _check(N.lib().hnswhdb_forest(device, n, m, _p(a) if m else None, _p(b) if m else None, _p(w) if m else None, int(min_cluster_size), code,
                                          *o.pointers()))
    return _select_behind(o.result(), method, device, allow_single_cluster, cluster_selection_epsilon, max_cluster_size, outlier_scores)


def csr_spanning_forest(offsets, cols, dists=None, device=0):
    """The minimum spanning forest of ANY graph given in CSR (offsets u64[n + 1], cols u32[offsets[n]], dists f32 per entry or None:
    every weight 0), taken on `device`: every entry (r, c) is the undirected pair {r, c}, self-loops are ignored, a repeated pair
    has the min of its weights.  Weights are ordered by value, -0 equal to +0, every NaN behind +inf; ties go by (lo, hi).  Returns
    a SpanningForestResult."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    if dists is not None:
        dists = np.ascontiguousarray(dists, dtype=np.float32)
        if len(dists) != len(cols):
            raise HnswError(N.ERR_ARG, f"dists has {len(dists)} entries, cols has {len(cols)}")
        if len(dists) == 0:
            dists = None  # (there is no entry)
    if len(offsets) == 0 or int(offsets[-1]) > len(cols):
        raise HnswError(N.ERR_ARG, "offsets must hold n + 1 entries, the last one at most len(cols)")
    n = len(offsets) - 1
    slots = max(n - 1, 1)
    a, b, w, m = np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.float32), np.zeros(1, np.uint64)
    _check(N.lib().hnswgpu_csr_spanning_forest(device, n, _p(offsets), _p(cols) if len(cols) else None, _p(dists), _p(a), _p(b), _p(w), _p(m)))
    m = int(m[0])
    return SpanningForestResult(a[:m].copy(), b[:m].copy(), w[:m].copy(), m, n)


class Hnsw:
    """Hnsw<f32, D>: owns a hnswgpu_index handle (flat host graph + its HBM replica)."""

    def __init__(self, max_nb_connection=16, max_elements=0, max_layer=16, ef_construction=200, dist="DistL2",
                 _handle=None):
        self._lib = N.lib()
        self._h = _handle
        self._pending = None
        if _handle is None:
            if max_nb_connection > 256:
                # the reference prints and calls process::exit(1) (src/hnsw.rs:784-787); we raise instead
                raise HnswError(N.ERR_ARG, "error max_nb_connection must be less equal than 256")
            self._params = N.BuildParams(max_nb_connection, ef_construction, max_layer, N.DIST[dist], 1.0, 0, 0, 0, 0, 0, 0, 0)
            self._dist = dist
        else:
            self._dist = N.DIST_NAME[self._lib.hnswgpu_dist(self._h)]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.hnswgpu_free_index(h)

    # ---- construction-time setters (src/hnsw.rs:845-905) --------------------------------
    def set_extend_candidates(self, flag):
        self._params.extend_candidates = int(bool(flag))

    def set_keeping_pruned(self, flag):
        self._params.keep_pruned = int(bool(flag))

    def modify_level_scale(self, scale_modification):
        self._params.level_scale_factor = min(1.0, max(0.2, float(scale_modification)))

    def set_build_options(self, nthreads=None, fast_arithmetic=None, gpu_device=None, gpu_window=None):
        """Extension: 1 thread = deterministic serial insert; fast_arithmetic = SIMD-order sums; gpu_device >= 0 =
        GPU-assisted construction (the insertions' searches on the device, window by window; gpu_window = 1: one point
        at a time, the serial insertion exactly)."""
        if nthreads is not None:
            self._params.nthreads = int(nthreads)
        if fast_arithmetic is not None:
            self._params.fast_arithmetic = int(bool(fast_arithmetic))
        if gpu_device is not None:
            self._params.gpu_assist = int(gpu_device >= 0)
            self._params.gpu_device = max(0, int(gpu_device))
        if gpu_window is not None:
            self._params.gpu_window = int(gpu_window)

    # ---- insertion (host construction; src/hnsw.rs:1069-1238) ---------------------------
    def parallel_insert(self, data, ids=None):
        """data: (n, d) f32 matrix; ids: origin ids (default: continue from the number of points).  The first call
        builds the index; later calls -- also on an index reloaded from a dump -- keep inserting into it."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.ndim != 2:
            raise HnswError(N.ERR_ARG, "data must be a (n, d) matrix")
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            idp = _p(ids)
        if self._h is not None:
            nthreads = self._params.nthreads if hasattr(self, "_params") else 0
            gpu = self._params.gpu_device if hasattr(self, "_params") and self._params.gpu_assist else -1
            if gpu >= 0:
                _check(self._lib.hnswgpu_insert_gpu(self._h, _p(data), data.shape[0], data.shape[1], idp, nthreads, gpu,
                                                    self._params.gpu_window))
            else:
                _check(self._lib.hnswgpu_insert(self._h, _p(data), data.shape[0], data.shape[1], idp, nthreads))
            return
        h = C.c_void_p()
        _check(self._lib.hnswgpu_build(_p(data), data.shape[0], data.shape[1], idp, C.byref(self._params),
                                       C.byref(h)))
        self._h = h.value

    def insert_serial(self, data, ids=None):
        """for (v, id) in data: hnsw.insert((v, id)) -- deterministic serial insertion."""
        if not hasattr(self, "_params"):  # reloaded index
            data = np.ascontiguousarray(data, dtype=np.float32)
            idp = _p(np.ascontiguousarray(ids, dtype=np.uint64)) if ids is not None else None
            _check(self._lib.hnswgpu_insert(self._h, _p(data), data.shape[0], data.shape[1], idp, 1))
            return
        saved = self._params.nthreads
        self._params.nthreads = 1
        try:
            self.parallel_insert(data, ids)
        finally:
            self._params.nthreads = saved

    # ---- getters -------------------------------------------------------------------------
    def get_nb_point(self):
        return self._lib.hnswgpu_nb_point(self._h) if self._h else 0

    def get_max_level_observed(self):
        return self._lib.hnswgpu_max_level_observed(self._h) if self._h else 0

    def get_layer_nb_point(self, layer):
        return self._lib.hnswgpu_layer_nb_point(self._h, layer) if self._h else 0

    def get_distance_name(self):
        return self._dist

    def get_description(self):
        d = N.Description()
        _check(self._lib.hnswgpu_get_description(self._h, C.byref(d)))
        return d

    def get_entry_point(self):
        o, l, r = C.c_uint64(), C.c_uint8(), C.c_int32()
        _check(self._lib.hnswgpu_entry_point(self._h, C.byref(o), C.byref(l), C.byref(r)))
        return o.value, (l.value, r.value)

    def get_neighbours(self, layer, rank, l, cap=512):
        ids = np.zeros(cap, np.uint64)
        layers = np.zeros(cap, np.uint8)
        ranks = np.zeros(cap, np.int32)
        dists = np.zeros(cap, np.float32)
        n = self._lib.hnswgpu_neighbours(self._h, layer, rank, l, cap, _p(ids), _p(layers), _p(ranks), _p(dists))
        if n < 0:
            raise HnswError(N.ERR_ARG, N.last_error())
        n = min(n, cap)
        return ids[:n], layers[:n], ranks[:n], dists[:n]

    # ---- device residency ------------------------------------------------------------------
    def upload(self, device=0):
        """Replicate vectors + neighbour lists into the HBM of HIP device `device`."""
        if self._h is None:
            raise HnswError(N.ERR_EMPTY, "index is empty")
        _check(self._lib.hnswgpu_upload(self._h, device))

    # ---- search -------------------------------------------------------------------------
    def parallel_search_flat(self, datas, knbn, ef, out=None):
        """Hnsw::parallel_search on a (nq, d) matrix; returns a BatchResult (flat arrays).  `out`: a BatchResult of an earlier
        call of the same shape whose arrays are written again (a caller in steady state: fresh arrays cost a page fault per
        4 KB while the answers are unpacked)."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        if datas.ndim != 2:
            raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
        nq, d = datas.shape
        if out is not None:
            ids, dists, layers, ranks, counts = out.ids, out.dists, out.layers, out.ranks, out.counts
            if ids.shape != (nq, knbn) or counts.shape != (nq,):
                raise HnswError(N.ERR_ARG, "out was made for another shape")
        else:
            ids = np.zeros((nq, knbn), np.uint64)
            dists = np.zeros((nq, knbn), np.float32)
            layers = np.zeros((nq, knbn), np.uint8)
            ranks = np.zeros((nq, knbn), np.int32)
            counts = np.zeros(nq, np.uint32)
        if self._h is None:  # empty index => empty answers (src/hnsw.rs:1498-1503)
            return BatchResult(ids, dists, layers, ranks, counts)
        _check(self._lib.hnswgpu_search_batch(self._h, _p(datas), nq, d, knbn, ef, _p(ids), _p(dists), _p(layers),
                                              _p(ranks), _p(counts)))
        return BatchResult(ids, dists, layers, ranks, counts)

    def parallel_search_sharded_flat(self, datas, knbn, ef, devices):
        """Hnsw::parallel_search with the batch sharded over the GPUs `devices` of this process (graph replicated,
        contiguous balanced blocks, answers gathered into one result; a device may be named more than once)."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        nq, d = datas.shape
        ids = np.zeros((nq, knbn), np.uint64)
        dists = np.zeros((nq, knbn), np.float32)
        layers = np.zeros((nq, knbn), np.uint8)
        ranks = np.zeros((nq, knbn), np.int32)
        counts = np.zeros(nq, np.uint32)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        _check(self._lib.hnswgpu_search_batch_sharded(self._h, _p(dev), len(dev), _p(datas), nq, d, knbn, ef, _p(ids), _p(dists),
                                                      _p(layers), _p(ranks), _p(counts)))
        return BatchResult(ids, dists, layers, ranks, counts)

    def parallel_search_filter_flat(self, datas, knbn, ef, allowed_ids):
        """Hnsw::search_filter(data, knbn, ef, Some(&allowed_ids)) for every row of `datas` (src/hnsw.rs:1487-1580);
        allowed_ids = the SORTED id vector of `impl FilterT for Vec<usize>` (src/filter.rs:11-15).  Rows on which the
        reference panics come back with count 0 and status 1."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        if datas.ndim != 2:
            raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
        allowed = np.ascontiguousarray(allowed_ids, dtype=np.uint64)
        nq, d = datas.shape
        ids = np.zeros((nq, knbn), np.uint64)
        dists = np.zeros((nq, knbn), np.float32)
        layers = np.zeros((nq, knbn), np.uint8)
        ranks = np.zeros((nq, knbn), np.int32)
        counts = np.zeros(nq, np.uint32)
        status = np.zeros(nq, np.uint8)
        if self._h is None:
            return BatchResult(ids, dists, layers, ranks, counts, status)
        _check(self._lib.hnswgpu_search_batch_filtered(self._h, _p(datas), nq, d, knbn, ef, _p(allowed), len(allowed), _p(ids),
                                                       _p(dists), _p(layers), _p(ranks), _p(counts), _p(status)))
        return BatchResult(ids, dists, layers, ranks, counts, status)

    def parallel_search_filters_flat(self, datas, knbn, ef, filters, filter_of=None):
        """Hnsw::search_filter(datas[q], knbn, ef, Some(&filters[filter_of[q]])) for every row q: a set of filters for the batch,
        each query naming its own.  filters: a sequence of SORTED id arrays (an empty one allows nothing); filter_of: one index
        into it per query, or None for one filter per query in order (len(filters) == nq).  Rows on which the reference panics
        come back with count 0 and status 1."""
        datas, flat, offsets, filter_of = _pack_filter_set(datas, filters, filter_of)
        nq, d = datas.shape
        ids = np.zeros((nq, knbn), np.uint64)
        dists = np.zeros((nq, knbn), np.float32)
        layers = np.zeros((nq, knbn), np.uint8)
        ranks = np.zeros((nq, knbn), np.int32)
        counts = np.zeros(nq, np.uint32)
        status = np.zeros(nq, np.uint8)
        if self._h is None:  # empty index => empty answers (src/hnsw.rs:1498-1503)
            return BatchResult(ids, dists, layers, ranks, counts, status)
        _check(self._lib.hnswgpu_search_batch_filter_set(self._h, _p(datas), nq, d, knbn, ef, _p(flat), _p(offsets), len(offsets) - 1,
                                                         _p(filter_of), _p(ids), _p(dists), _p(layers), _p(ranks), _p(counts),
                                                         _p(status)))
        return BatchResult(ids, dists, layers, ranks, counts, status)

    def search_filter(self, data, knbn, ef, allowed_ids):
        """Vec<Neighbour> of Hnsw::search_filter with a sorted id vector; raises where the reference panics."""
        data = np.ascontiguousarray(data, dtype=np.float32).reshape(1, -1)
        r = self.parallel_search_filter_flat(data, knbn, ef, allowed_ids)
        if r.status[0]:
            raise HnswError(N.ERR_REF_PANIC, "the reference panics on this query (return_points emptied by the filter, src/hnsw.rs:973)")
        return r.to_neighbours()[0]

    def parallel_search(self, datas, knbn, ef):
        """Vec<Vec<Neighbour>> in input order (src/hnsw.rs:1612-1635)."""
        return self.parallel_search_flat(datas, knbn, ef).to_neighbours()

    def search(self, data, knbn, ef):
        """Vec<Neighbour> (src/hnsw.rs:1597)."""
        data = np.ascontiguousarray(data, dtype=np.float32).reshape(1, -1)
        return self.parallel_search(data, knbn, ef)[0]

    # ---- exhaustive exact k-NN (an extension: the reference gets its ground truth from files or a CPU loop) ----------
    def exact_search_flat(self, datas, knbn, allowed_ids=None):
        """The knbn nearest of ALL points (all layers) for every row of `datas`, by exhaustive search on the device, in the
        arithmetic of the index's own search: the min(knbn, eligible) smallest by (distance as f32, origin id ascending),
        in that order.  allowed_ids: None, or the SORTED id vector of a filter (ids naming no point are ignored; an
        empty vector gives counts of 0).  knbn up to 4096.  Returns a BatchResult."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        if datas.ndim != 2:
            raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
        nq, d = datas.shape
        ids = np.zeros((nq, knbn), np.uint64)
        dists = np.zeros((nq, knbn), np.float32)
        layers = np.zeros((nq, knbn), np.uint8)
        ranks = np.zeros((nq, knbn), np.int32)
        counts = np.zeros(nq, np.uint32)
        if self._h is None:
            return BatchResult(ids, dists, layers, ranks, counts)
        allowed, n_allowed = None, 0
        if allowed_ids is not None:
            n_allowed = len(allowed_ids)
            # (an empty filter still is a filter: a non-null pointer, zero ids)
            allowed = np.ascontiguousarray(allowed_ids, dtype=np.uint64) if n_allowed else np.zeros(1, np.uint64)
        _check(self._lib.hnswgpu_exact_search_batch(self._h, _p(datas), nq, d, knbn, _p(allowed), n_allowed, _p(ids), _p(dists),
                                                    _p(layers), _p(ranks), _p(counts)))
        return BatchResult(ids, dists, layers, ranks, counts)

    def exact_search(self, datas, knbn, allowed_ids=None):
        """exact_search_flat as Vec<Vec<Neighbour>> in input order."""
        return self.exact_search_flat(datas, knbn, allowed_ids).to_neighbours()

    def exact_search_filters_flat(self, datas, knbn, filters, filter_of=None):
        """exact_search_flat for a set of filters, each query naming its own: row q is exact_search_flat(datas[q], knbn,
        filters[filter_of[q]]) -- the ground truth of parallel_search_filters_flat, whose `filters` / `filter_of` these are."""
        datas, flat, offsets, filter_of = _pack_filter_set(datas, filters, filter_of)
        nq, d = datas.shape
        ids = np.zeros((nq, knbn), np.uint64)
        dists = np.zeros((nq, knbn), np.float32)
        layers = np.zeros((nq, knbn), np.uint8)
        ranks = np.zeros((nq, knbn), np.int32)
        counts = np.zeros(nq, np.uint32)
        if self._h is None:
            return BatchResult(ids, dists, layers, ranks, counts)
        _check(self._lib.hnswgpu_exact_search_batch_filter_set(self._h, _p(datas), nq, d, knbn, _p(flat), _p(offsets), len(offsets) - 1,
                                                               _p(filter_of), _p(ids), _p(dists), _p(layers), _p(ranks), _p(counts)))
        return BatchResult(ids, dists, layers, ranks, counts)

    def exact_search_filters(self, datas, knbn, filters, filter_of=None):
        """exact_search_filters_flat as Vec<Vec<Neighbour>> in input order."""
        return self.exact_search_filters_flat(datas, knbn, filters, filter_of).to_neighbours()

    # ---- exhaustive exact range search (an extension, like the exact k-NN) ------------------------------------------
    def exact_range_search_flat(self, datas, radius, allowed_ids=None):
        """Every point within `radius` (a scalar, or one value per row of `datas`) of every row of `datas`, by exhaustive
        search on the device in the arithmetic of the index's own search: the eligible points with distance <= radius as
        f32 values, ascending by (distance, origin id).  allowed_ids as in exact_search_flat.  Returns a RangeResult.
        One call with a guessed capacity, one more with the exact total when the guess was too small."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        if datas.ndim != 2:
            raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
        nq, d = datas.shape
        radii = np.asarray(radius, dtype=np.float32)
        if radii.ndim == 0:
            radii = np.full(nq, radii, np.float32)
        if radii.shape != (nq,):
            raise HnswError(N.ERR_ARG, "radius must be a scalar or hold one radius per query")
        radii = np.ascontiguousarray(radii)
        offsets = np.zeros(nq + 1, np.uint64)

        def empty(cap):
            return np.zeros(cap, np.uint64), np.zeros(cap, np.float32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        if self._h is None:
            return RangeResult(offsets, *empty(0))
        allowed, n_allowed = None, 0
        if allowed_ids is not None:
            n_allowed = len(allowed_ids)
            allowed = np.ascontiguousarray(allowed_ids, dtype=np.uint64) if n_allowed else np.zeros(1, np.uint64)
        cap = max(1024, 32 * nq)
        for attempt in range(2):
            ids, dists, layers, ranks = empty(cap)
            rc = self._lib.hnswgpu_exact_range_search_batch(self._h, _p(datas), nq, d, _p(radii), _p(allowed), n_allowed, cap, _p(offsets),
                                                            _p(ids), _p(dists), _p(layers), _p(ranks))
            if rc != N.ERR_CAPACITY or attempt == 1:
                break
            cap = int(offsets[nq])
        _check(rc)
        total = int(offsets[nq])
        return RangeResult(offsets, ids[:total], dists[:total], layers[:total], ranks[:total])

    def exact_range_search(self, datas, radius, allowed_ids=None):
        """exact_range_search_flat as Vec<Vec<Neighbour>> in input order."""
        return self.exact_range_search_flat(datas, radius, allowed_ids).to_neighbours()

    # ---- approximate range search through the graph (an extension) --------------------------------------------------
    def range_search_flat(self, datas, radius, ef_first, ef_max, allowed_ids=None):
        """Every point within `radius` (a scalar, or one value per row of `datas`) that the index's own search finds: per query
        the search with knbn = ef = ef_first, 2 ef_first, ... (clamped to ef_max), restarted until its result set reaches past the
        ball, returns fewer than ef entries or ef_max is reached; the answer is the prefix with distance <= radius of that one
        search, bit for bit (ids, f32 distances, p_ids, the search's order).  allowed_ids: the SORTED id vector of a filter
        (then ef_first >= 2).  Returns a RangeResult with .ef and .flags (bit 0: saturated, raise ef_max).  One call with a
        guessed capacity, one more with the exact total when the guess was too small."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        if datas.ndim != 2:
            raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
        nq, d = datas.shape
        radii = np.asarray(radius, dtype=np.float32)
        if radii.ndim == 0:
            radii = np.full(nq, radii, np.float32)
        if radii.shape != (nq,):
            raise HnswError(N.ERR_ARG, "radius must be a scalar or hold one radius per query")
        radii = np.ascontiguousarray(radii)
        offsets = np.zeros(nq + 1, np.uint64)
        ef, flags = np.zeros(nq, np.uint32), np.zeros(nq, np.uint8)

        def empty(cap):
            return np.zeros(cap, np.uint64), np.zeros(cap, np.float32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        allowed, n_allowed = None, 0
        if allowed_ids is not None:
            n_allowed = len(allowed_ids)
            allowed = np.ascontiguousarray(allowed_ids, dtype=np.uint64) if n_allowed else np.zeros(1, np.uint64)
        if self._h is None:
            if not 1 <= ef_first <= ef_max <= 4096 or (allowed is not None and ef_first < 2):
                raise HnswError(N.ERR_ARG, "1 <= ef_first <= ef_max <= 4096 (ef_first >= 2 with a filter)")
            return RangeResult(offsets, *empty(0), ef, flags)
        cap = max(1024, 32 * nq)
        for attempt in range(2):
            ids, dists, layers, ranks = empty(cap)
            rc = self._lib.hnswgpu_range_search_batch(self._h, _p(datas), nq, d, _p(radii), ef_first, ef_max, _p(allowed), n_allowed, cap,
                                                      _p(offsets), _p(ids), _p(dists), _p(layers), _p(ranks), _p(ef), _p(flags))
            if rc != N.ERR_CAPACITY or attempt == 1:
                break
            cap = int(offsets[nq])
        _check(rc)
        total = int(offsets[nq])
        return RangeResult(offsets, ids[:total], dists[:total], layers[:total], ranks[:total], ef, flags)

    def range_search(self, datas, radius, ef_first, ef_max, allowed_ids=None):
        """range_search_flat as Vec<Vec<Neighbour>> in input order."""
        return self.range_search_flat(datas, radius, ef_first, ef_max, allowed_ids).to_neighbours()

    def range_recall_flat(self, datas, radius, ef_first, ef_max, allowed_ids=None):
        """(recall by id, share of saturated queries) of range_search_flat against exact_range_search_flat: the hits found (ids
        of a query's answer that are in its exact answer) over the hits that exist; 1.0 when none exists."""
        got = self.range_search_flat(datas, radius, ef_first, ef_max, allowed_ids)
        exact = self.exact_range_search_flat(datas, radius, allowed_ids)
        nq = len(exact.offsets) - 1
        found = sum(len(np.intersect1d(got.of(q)[0], exact.of(q)[0])) for q in range(nq))
        total = int(exact.offsets[nq])
        saturated = float(np.count_nonzero(got.flags & 1)) / nq if nq else 0.0
        return (found / total if total else 1.0), saturated

    # ---- queries by stored point: the k-NN graph of the indexed points (an extension) --------------------------------
    def _graph_call(self, entry, knbn, point_ids, *middle):
        """one of the two graph entries: point_ids (DataIds; None = every point, row i being the point at position i of the
        ascending (DataId, dump order) order), the entry's own arguments, the five output arrays"""
        pts = None
        if point_ids is not None:
            pts = np.ascontiguousarray(point_ids, dtype=np.uint64).reshape(-1)
        np_ = self.get_nb_point() if pts is None else len(pts)
        ids = np.zeros((np_, knbn), np.uint64)
        dists = np.zeros((np_, knbn), np.float32)
        layers = np.zeros((np_, knbn), np.uint8)
        ranks = np.zeros((np_, knbn), np.int32)
        counts = np.zeros(np_, np.uint32)
        if self._h is None:
            if np_ != 0:
                raise HnswError(N.ERR_ARG, f"{np_} of the {np_} point_ids name no point of the index")
            return BatchResult(ids, dists, layers, ranks, counts)
        if pts is not None and np_ == 0:
            pts = np.zeros(1, np.uint64)  # (no point named still is a list of points: a non-null pointer, zero ids)
        _check(entry(self._h, _p(pts), np_, knbn, *middle, _p(ids), _p(dists), _p(layers), _p(ranks), _p(counts)))
        return BatchResult(ids, dists, layers, ranks, counts)

    def knn_graph_flat(self, knbn, ef, point_ids=None):
        """The approximate k-NN graph: for every named point (DataIds; None = every point of the index) its knbn neighbours
        by the index's own search -- the answer of parallel_search_flat(the point's stored vector, knbn + 1, ef) without the
        entry that is the point itself (by p_id: exact copies and other points of its DataId stay), or without its last entry
        when the point is not in its own answer.  The stored vectors never leave the device.  An id that no point carries
        raises (ERR_ARG); an id that several points carry names the first in dump order.  Returns a BatchResult."""
        return self._graph_call(self._lib.hnswgpu_graph_search_batch, knbn, point_ids, ef)

    def exact_knn_graph_flat(self, knbn, point_ids=None, allowed_ids=None):
        """The exact k-NN graph: for every named point the min(knbn, candidates) smallest by (distance as f32, origin id,
        dump order) among all OTHER points -- or, with allowed_ids (the SORTED id vector of a filter, as in exact_search_flat),
        among the allowed points other than itself.  The point is excluded by identity: its exact copies come back at distance
        0.  knbn up to 4096.  Returns a BatchResult."""
        allowed, n_allowed = None, 0
        if allowed_ids is not None:
            n_allowed = len(allowed_ids)
            allowed = np.ascontiguousarray(allowed_ids, dtype=np.uint64) if n_allowed else np.zeros(1, np.uint64)
        return self._graph_call(self._lib.hnswgpu_exact_graph_batch, knbn, point_ids, _p(allowed), n_allowed)

    # ---- the k-NN graph of the indexed points made undirected, in CSR (an extension) ----------------------------------
    def symmetric_knn_graph_flat(self, knbn, ef=None, mode="union"):
        """The k-NN graph of every indexed point made undirected on the device.  The directed graph is exact_knn_graph_flat(knbn)
        (ef=None) or knn_graph_flat(knbn, ef), every point, bit for bit; mode "union": row i holds j iff either names the other,
        "mutual": iff both do.  An entry's distance is the stored f32 of its own row's edge when there is one, else of the other
        row's (for DistJeffreys and DistJensenShannon the two directions differ in their bits).  Returns a GraphCsrResult.  One
        call with a guessed capacity, one more with the exact total when the guess was too small."""
        modes = {"union": N.HEADER.constants["HNSWGPU_SYM_UNION"], "mutual": N.HEADER.constants["HNSWGPU_SYM_MUTUAL"]}
        if mode not in modes:
            raise HnswError(N.ERR_ARG, f"mode must be 'union' or 'mutual', not {mode!r}")
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact graph)")
        n = self.get_nb_point()
        offsets = np.zeros(n + 1, np.uint64)

        def empty(cap):
            return (np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.float32), np.zeros(cap, np.uint8),
                    np.zeros(cap, np.int32))
        if self._h is None:
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            return GraphCsrResult(offsets, *empty(0))
        cap = max(1024, 2 * n * min(knbn, max(n - 1, 1)) if modes[mode] == 0 else n * min(knbn, max(n - 1, 1)))
        for attempt in range(2):
            pos, ids, dists, layers, ranks = empty(cap)
            rc = self._lib.hnswgpu_symmetric_graph(self._h, knbn, 0 if ef is None else ef, modes[mode], cap, _p(offsets), _p(pos), _p(ids),
                                                   _p(dists), _p(layers), _p(ranks))
            if rc != N.ERR_CAPACITY or attempt == 1:
                break
            cap = int(offsets[n])
        _check(rc)
        total = int(offsets[n])
        return GraphCsrResult(offsets, pos[:total], ids[:total], dists[:total], layers[:total], ranks[:total])

    def symmetric_knn_graph(self, knbn, ef=None, mode="union"):
        """symmetric_knn_graph_flat as Vec<Vec<Neighbour>>, row i being the point at position i."""
        return self.symmetric_knn_graph_flat(knbn, ef, mode).to_neighbours()

    def knn_graph_components(self, knbn, ef=None, mode="union", max_dist=None):
        """The connected components of the graph symmetric_knn_graph_flat(knbn, ef, mode) would build, labelled on the device without
        building it.  Vertices are POSITIONS (the rows of that graph).  With max_dist the directed graph is cut first: an entry i -> j
        counts iff its stored f32 distance is <= max_dist (a NaN never is); "union" then joins i and j iff either direction is left,
        "mutual" iff both are.  Returns a ComponentsResult."""
        modes = {"union": N.HEADER.constants["HNSWGPU_SYM_UNION"], "mutual": N.HEADER.constants["HNSWGPU_SYM_MUTUAL"]}
        if mode not in modes:
            raise HnswError(N.ERR_ARG, f"mode must be 'union' or 'mutual', not {mode!r}")
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact graph)")
        if max_dist is not None and np.isnan(np.float32(max_dist)):
            raise HnswError(N.ERR_ARG, "max_dist is NaN")
        n = self.get_nb_point()
        labels, sizes, c = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.uint64)
        if self._h is None:
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            return ComponentsResult(labels, sizes, 0)
        cut = _cut(max_dist)
        _check(self._lib.hnswgpu_graph_components(self._h, knbn, 0 if ef is None else ef, modes[mode], _p(cut), _p(labels), _p(sizes), _p(c)))
        return ComponentsResult(labels, sizes[:int(c[0])].copy(), int(c[0]))

    def dbscan(self, eps, min_samples):
        """Exact DBSCAN(eps, min_samples) of the indexed points on the device, without a neighbour list: the set of point i is every
        stored point j (itself included) with dist(point i as the query, j) <= eps, the bits of hnswgpu_exact_search_batch.  Vertices
        are POSITIONS (the rows of symmetric_knn_graph_flat).  Returns a DbscanResult."""
        eps, min_samples = _dbscan_params(eps, min_samples)
        labels, core, counts, anchors, c = _dbscan_arrays(self.get_nb_point())
        if self._h is None:
            return DbscanResult(labels, core.astype(bool), counts, anchors, 0)
        _check(self._lib.hnswdbs_exact(self._h, eps, min_samples, _p(labels), _p(core), _p(counts), _p(anchors), _p(c)))
        return DbscanResult(labels, core.astype(bool), counts, anchors, int(c[0]))

    def knn_graph_spanning_forest(self, knbn, ef=None, mode="union", core_k=0):
        """The minimum spanning forest of the graph symmetric_knn_graph_flat(knbn, ef, mode) would build, taken on the device without
        building it.  Vertices are POSITIONS.  "union": a pair weighs the min of its directions in the directed graph; "mutual": the
        max of the two.  core_k >= 1: mutual-reachability weights, max(pair, core(a), core(b)) with core(v) the distance to v's
        core_k-th neighbour in the directed graph (the last one of a shorter row).  Returns a SpanningForestResult whose
        labels_at(r) equals knn_graph_components(knbn, ef, mode, max_dist=r) when core_k == 0."""
        modes = {"union": N.HEADER.constants["HNSWGPU_SYM_UNION"], "mutual": N.HEADER.constants["HNSWGPU_SYM_MUTUAL"]}
        if mode not in modes:
            raise HnswError(N.ERR_ARG, f"mode must be 'union' or 'mutual', not {mode!r}")
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact graph)")
        if core_k < 0:
            raise HnswError(N.ERR_ARG, "core_k must be >= 0")
        n = self.get_nb_point()
        slots = max(n - 1, 1)
        a, b, w, m = np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.float32), np.zeros(1, np.uint64)
        if self._h is None:
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            if core_k > knbn:
                raise HnswError(N.ERR_ARG, "core_k is above knbn")
            return SpanningForestResult(a[:0], b[:0], w[:0], 0, 0)
        _check(self._lib.hnswgpu_graph_spanning_forest(self._h, knbn, 0 if ef is None else ef, modes[mode], core_k, _p(a), _p(b), _p(w), _p(m)))
        m = int(m[0])
        return SpanningForestResult(a[:m].copy(), b[:m].copy(), w[:m].copy(), m, n)

    def knn_graph_dendrogram(self, knbn, ef=None, mode="union", core_k=0):
        """knn_graph_spanning_forest(knbn, ef, mode, core_k) and the single-linkage dendrogram of that forest in one call, the forest
        staying on the device in between.  Returns a DendrogramResult whose a, b and weights are that forest's, byte for byte."""
        modes = {"union": N.HEADER.constants["HNSWGPU_SYM_UNION"], "mutual": N.HEADER.constants["HNSWGPU_SYM_MUTUAL"]}
        if mode not in modes:
            raise HnswError(N.ERR_ARG, f"mode must be 'union' or 'mutual', not {mode!r}")
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact graph)")
        if core_k < 0:
            raise HnswError(N.ERR_ARG, "core_k must be >= 0")
        n = self.get_nb_point()
        slots = max(n - 1, 1)
        a, b, w, m = np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.float32), np.zeros(1, np.uint64)
        left, right, sizes = np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.uint32)
        if self._h is None:
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            if core_k > knbn:
                raise HnswError(N.ERR_ARG, "core_k is above knbn")
            return DendrogramResult(left[:0], right[:0], sizes[:0], 0, 0, a[:0], b[:0], w[:0])
        _check(self._lib.hnswgpu_graph_dendrogram(self._h, knbn, 0 if ef is None else ef, modes[mode], core_k, _p(a), _p(b), _p(w), _p(left),
                                                  _p(right), _p(sizes), _p(m)))
        m = int(m[0])
        return DendrogramResult(left[:m].copy(), right[:m].copy(), sizes[:m].copy(), m, n, a[:m].copy(), b[:m].copy(), w[:m].copy())

    def hdbscan(self, min_cluster_size, knbn, ef=None, mode="union", core_k=None, method="eom", allow_single_cluster=False,
                cluster_selection_epsilon=0.0, max_cluster_size=None, outlier_scores=False):
        """HDBSCAN of the indexed points in one call: knn_graph_dendrogram(knbn, ef, mode, core_k), the condensed tree of that
        dendrogram for min_cluster_size, the stabilities, the selection ("eom": excess of mass, "leaf": the leaves) and the labels,
        the forest and the dendrogram staying on the device throughout.  Vertices are POSITIONS.  core_k=None means
        min(min_cluster_size - 1, knbn): sklearn's default min_samples = min_cluster_size, which counts the point itself.  Returns
        an HdbscanResult whose forest and dendrogram are knn_graph_dendrogram's, byte for byte.  allow_single_cluster,
        cluster_selection_epsilon, max_cluster_size and outlier_scores are HdbscanResult.select's: at their defaults the answer is
        hnswhdb_graph's own, otherwise select() runs behind it (on device 0; result.select(..., device=) chooses another)."""
        modes = {"union": N.HEADER.constants["HNSWGPU_SYM_UNION"], "mutual": N.HEADER.constants["HNSWGPU_SYM_MUTUAL"]}
        if mode not in modes:
            raise HnswError(N.ERR_ARG, f"mode must be 'union' or 'mutual', not {mode!r}")
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact graph)")
        code = _hdbscan_method(method)
        n = self.get_nb_point()
        o = _HdbscanArrays(n, min_cluster_size)
        if core_k is None:
            core_k = max(min(int(min_cluster_size) - 1, knbn), 0)
        if core_k < 0:
            raise HnswError(N.ERR_ARG, "core_k must be >= 0")
        slots = max(n - 1, 1)
        a, b, w, m = np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.float32), np.zeros(1, np.uint64)
        left, right, sizes = np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.uint32)
        if self._h is None:
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            if core_k > knbn:
                raise HnswError(N.ERR_ARG, "core_k is above knbn")
            res = o.result(SpanningForestResult(a[:0], b[:0], w[:0], 0, 0), DendrogramResult(left[:0], right[:0], sizes[:0], 0, 0, a[:0], b[:0], w[:0]))
            res.knn_params = (knbn, ef, core_k)
            return _select_behind(res, method, 0, allow_single_cluster, cluster_selection_epsilon, max_cluster_size, outlier_scores)
        _check(self._lib.hnswhdb_graph(self._h, knbn, 0 if ef is None else ef, modes[mode], core_k, int(min_cluster_size), code, _p(a), _p(b),
                                               _p(w), _p(left), _p(right), _p(sizes), *o.pointers(), _p(m)))
        m = int(m[0])
        a, b, w = a[:m].copy(), b[:m].copy(), w[:m].copy()
        res = o.result(SpanningForestResult(a, b, w, m, n), DendrogramResult(left[:m].copy(), right[:m].copy(), sizes[:m].copy(), m, n, a, b, w))
        res.knn_params = (knbn, ef, core_k)
        return _select_behind(res, method, 0, allow_single_cluster, cluster_selection_epsilon, max_cluster_size, outlier_scores)

    def core_distances(self, knbn, ef=None, core_k=0):
        """The stored points' core distances, f32 per POSITION: exactly what knn_graph_spanning_forest and hdbscan use with the same
        knbn, ef and core_k -- the distance to a point's core_k-th neighbour in the directed graph (the last one of a shorter row),
        0 for core_k == 0 (hnswhdp_core_distances)."""
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact graph)")
        if core_k < 0:
            raise HnswError(N.ERR_ARG, "core_k must be >= 0")
        n = self.get_nb_point()
        core = np.zeros(max(n, 1), np.float32)
        if self._h is None:
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            if core_k > knbn:
                raise HnswError(N.ERR_ARG, "core_k is above knbn")
            return core[:0]
        _check(self._lib.hnswhdp_core_distances(self._h, knbn, 0 if ef is None else ef, core_k, _p(core)))
        return core[:n]

    def hdbscan_predict(self, result, datas, knbn=None, ef=None, core_k=None, core=None, cluster_selection_epsilon=0.0):
        """The (nq, d) new vectors `datas` assigned to the clusters of `result`, an HdbscanResult of this index's points -- what the
        hdbscan package calls approximate_predict -- in one call on the device: the search for each vector's knbn neighbours
        (ef=None: the exact search), their positions, and hdbscan_assign on those rows (hnswhdp_predict).  core_k and ef default to
        what Hnsw.hdbscan ran with (result.knn_params), knbn to 2 (core_k + 1); core=None calls core_distances with that call's knbn,
        ef and core_k first.  cluster_selection_epsilon as the selection had it.  Returns a PredictResult."""
        datas = np.ascontiguousarray(datas, dtype=np.float32)
        if datas.ndim != 2:
            raise HnswError(N.ERR_ARG, "datas must be a (nq, d) matrix")
        ran = result.knn_params
        if core_k is None:
            if ran is None:
                raise HnswError(N.ERR_ARG, "core_k=None needs a result of Hnsw.hdbscan (result.knn_params)")
            core_k = ran[2]
        if ef is None and ran is not None:
            ef = ran[1]
        if ef is not None and ef < 1:
            raise HnswError(N.ERR_ARG, "ef must be >= 1 (ef=None: the exact search)")
        if knbn is None:
            knbn = 2 * (core_k + 1)
        if core is None:
            if ran is None:
                raise HnswError(N.ERR_ARG, "core=None needs a result of Hnsw.hdbscan (result.knn_params)")
            core = self.core_distances(ran[0], ran[1], ran[2])
        nq, d = datas.shape
        o = _PredictArrays(result, core, nq, cluster_selection_epsilon)
        if o.n != self.get_nb_point():
            raise HnswError(N.ERR_ARG, f"the result has {o.n} vertices, the index {self.get_nb_point()} points")
        if self._h is None:  # no point: every row is empty
            if knbn < 1:
                raise HnswError(N.ERR_ARG, "knbn must be > 0")
            _check(self._lib.hnswhdp_assign(0, nq, knbn, _p(np.zeros((max(nq, 1), knbn), np.uint32)), _p(np.zeros((max(nq, 1), knbn), np.float32)),
                                            _p(np.zeros(max(nq, 1), np.uint32)), min(core_k, knbn), 0, *o.tree(), *o.outputs()))
            return o.result()
        _check(self._lib.hnswhdp_predict(self._h, _p(datas) if nq else None, nq, d, knbn, 0 if ef is None else ef, core_k, *o.tree(), *o.outputs()))
        return o.result()

    def knn_graph_recall(self, knbn, ef, point_ids=None):
        """The recall by id of knn_graph_flat against exact_knn_graph_flat over the named points: the share of the exact
        graph's edges whose id the approximate graph has in the same row."""
        return _recall(self.knn_graph_flat(knbn, ef, point_ids), self.exact_knn_graph_flat(knbn, point_ids))[1]

    def recall_flat(self, datas, knbn, ef, allowed_ids=None):
        """The two recalls the reference's examples print (examples/ann-sift1m-128-euclidean.rs:172-186), for this index's
        own search (filtered by allowed_ids if given) against the exact answer: (by distance, by id).
        By distance: answers with d <= the exact knbn-th distance (the last exact one when fewer are eligible), compared
        as f32; by id: answers whose id is among the exact ones; both over the number of exact answers."""
        exact = self.exact_search_flat(datas, knbn, allowed_ids)
        got = self.parallel_search_flat(datas, knbn, ef) if allowed_ids is None else \
            self.parallel_search_filter_flat(datas, knbn, ef, allowed_ids)
        return _recall(got, exact)

    def recall_filters_flat(self, datas, knbn, ef, filters, filter_of=None):
        """recall_flat for a set of filters, each query naming its own: parallel_search_filters_flat against
        exact_search_filters_flat, (by distance, by id).  A row on which the reference panics (status 1, count 0) has found
        nothing."""
        exact = self.exact_search_filters_flat(datas, knbn, filters, filter_of)
        got = self.parallel_search_filters_flat(datas, knbn, ef, filters, filter_of)
        return _recall(got, exact)

    # AnnT (src/api.rs:13-38)
    def search_neighbours(self, data, knbn, ef_s):
        return self.search(data, knbn, ef_s)

    def parallel_search_neighbours(self, data, knbn, ef_s):
        return self.parallel_search(data, knbn, ef_s)

    def file_dump(self, path, file_basename):
        """Writes <basename>.hnsw.graph / .hnsw.data into directory `path`; returns the basename."""
        if self._h is None:
            raise HnswError(N.ERR_EMPTY, "entry point not initialized")
        _check(self._lib.hnswgpu_file_dump(self._h, str(path).encode(), file_basename.encode()))
        return file_basename

    def last_search_kernel_ms(self):
        ms = C.c_double()
        _check(self._lib.hnswgpu_last_search_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def set_strict_ties(self, on=True):
        """Extension: replay tie-affected queries with a literal emulation of the reference's heaps."""
        _check(self._lib.hnswgpu_set_strict_ties(self._h, int(bool(on))))

    def set_arithmetic(self, arithmetic="scalar"):
        """Extension: "simd8" = distances of the following searches summed in the order of the crate's simdeez_f build."""
        _check(self._lib.hnswgpu_set_arithmetic(self._h, ARITH[arithmetic]))

    def set_storage(self, storage="f32"):
        """Extension: how the replicas hold the vectors in HBM.  "f16" = rows stored as IEEE binary16 (half the bytes) where every
        stored element is representable (round_to_f16 the data BEFORE building: the library only verifies); the answers of every
        search are those of the same index at "f32", bit for bit.  Raises HnswError(ERR_ARG) naming the first offending point."""
        _check(self._lib.hnswgpu_set_storage(self._h, STORAGE[storage]))

    def get_storage(self):
        return STORAGE_NAME[self._lib.hnswgpu_get_storage(self._h)]

    def device_bytes(self, device=0):
        """Bytes of the replica resident on `device` (upload first; a change of storage or an insert makes it stale)."""
        n = C.c_uint64()
        _check(self._lib.hnswgpu_device_bytes(self._h, int(device), C.byref(n)))
        return n.value

    def last_tie_count(self):
        n = C.c_uint32()
        _check(self._lib.hnswgpu_last_tie_count(self._h, C.byref(n)))
        return n.value

    def last_kernel_ms(self):
        ms, n = C.c_double(), C.c_uint32()
        _check(self._lib.hnswgpu_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @property
    def handle(self):
        return self._h


class HnswIo:
    """HnswIo::new(directory, basename) (src/hnswio.rs:317)."""

    def __init__(self, directory, basename):
        self.dir, self.basename = str(directory), basename

    def get_basename(self):
        return self.basename

    def load_hnsw(self, dist=None):
        """load_hnsw::<f32, D>() (src/hnswio.rs:431-524).  dist=None accepts the dump's own distance."""
        h = C.c_void_p()
        code = N.DIST[dist] if dist is not None else -1
        rc = N.lib().hnswgpu_load_dump(self.dir.encode(), self.basename.encode(), code, C.byref(h))
        if rc != N.OK:
            raise HnswError(rc, N.last_error())
        return Hnsw(_handle=h.value)


class DataMap:
    """hnsw_rs::datamap::DataMap (src/datamap.rs): the vectors of a dump by DataId, memory-mapped, graph not loaded."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def from_hnswdump(directory, file_name):
        h = C.c_void_p()
        _check(N.lib().hnswgpu_datamap_open(str(directory).encode(), file_name.encode(), C.byref(h)))
        return DataMap(h.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.lib().hnswgpu_datamap_close(h)

    def get_data(self, dataid):
        """Option<&[f32]>: a read-only view into the mapping, or None.  The view keeps this DataMap (and with it the mapping)
        alive: it may outlive every other reference to the object."""
        p = N.lib().hnswgpu_datamap_get_data(self._h, int(dataid))
        if not p:
            return None
        d = self.get_dimension()
        buf = (C.c_float * d).from_address(p)
        buf._datamap = self  # the ctypes object is the array's base: the mapping cannot be unmapped under the view
        a = np.ctypeslib.as_array(buf)
        a.flags.writeable = False
        return a

    def get_nb_data(self):
        return N.lib().hnswgpu_datamap_nb_data(self._h)

    def get_dimension(self):
        return N.lib().hnswgpu_datamap_dimension(self._h)

    def get_distname(self):
        return N.lib().hnswgpu_datamap_distname(self._h).decode()

    def get_data_typename(self):
        return N.lib().hnswgpu_datamap_typename(self._h).decode()

    def check_data_type(self, type_name):
        return type_name.rsplit("::", 1)[-1] == self.get_data_typename().rsplit("::", 1)[-1]

    def get_dataid_iter(self):
        n = self.get_nb_data()
        out = np.zeros(n, np.uint64)
        N.lib().hnswgpu_datamap_ids(self._h, _p(out), n)
        return out.tolist()


def load_description(graph_file_path):
    """load_description (src/hnswio.rs:937-1042) of a <basename>.hnsw.graph file."""
    d = N.Description()
    _check(N.lib().hnswgpu_load_description(str(graph_file_path).encode(), C.byref(d)))
    return d


ARITH = {"scalar": N.HEADER.constants["HNSWGPU_ARITH_SCALAR"], "simd8": N.HEADER.constants["HNSWGPU_ARITH_SIMD8"]}
STORAGE = {"f32": N.HEADER.constants["HNSWGPU_STORAGE_F32"], "f16": N.HEADER.constants["HNSWGPU_STORAGE_F16"]}
STORAGE_NAME = {v: k for k, v in STORAGE.items()}


def round_to_f16(x):
    """x rounded to the nearest IEEE binary16 and widened back: contiguous f32 that Hnsw.set_storage("f16") accepts."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32))


def f16_representable(x):
    """(number of elements of x that binary16 cannot hold exactly -- NaN counts --, flat index of the first or None)."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    first = C.c_uint64(0)
    bad = N.lib().hnswgpu_f16_representable(_p(a), a.size, C.byref(first))
    return bad, (first.value if bad else None)


EVAL_VARIANT = {"plain": 0, "deep": N.HEADER.constants["HNSWGPU_EVAL_DEEP"], "pipe": N.HEADER.constants["HNSWGPU_EVAL_PIPE"],
                "r128": N.HEADER.constants["HNSWGPU_EVAL_R128"],
                "deep+r128": N.HEADER.constants["HNSWGPU_EVAL_DEEP"] | N.HEADER.constants["HNSWGPU_EVAL_R128"]}


def eval_distance_matrix(dist, queries, rows, batch, arithmetic="scalar", storage="f32", variant="plain"):
    """out[q][r] = Distance<f32>::eval(queries[q], rows[r]) on the device, by the search kernel's own distance routine with
    the rows taken in batches of `batch` (1..64) -- the lane-group branches the search takes for that many neighbours.
    arithmetic: "scalar" (the crate's default build) or "simd8" (the summation order of its simdeez_f build).
    storage: "f16" = the rows (representable ones only) narrowed to binary16 before the kernel reads them (scalar arithmetic).
    variant: "plain", or the row loop a search kernel's expansion compiles -- "deep" (strict, ef <= 128), "pipe" (strict, ef 129..256),
    "r128" / "deep+r128" (the fixed row stride of DistL2 / f32 / 97 <= d <= 128, lean / strict); scalar arithmetic."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    r = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.zeros((q.shape[0], r.shape[0]), np.float32)
    if variant != "plain":
        if arithmetic != "scalar":
            raise HnswError(N.ERR_ARG, "the variants of the row loop exist in the scalar arithmetic only")
        _check(N.lib().hnswgpu_eval_distance_matrix_variant(N.DIST[dist], STORAGE[storage], EVAL_VARIANT[variant], _p(q), q.shape[0], _p(r),
                                                            r.shape[0], q.shape[1], batch, _p(out)))
        return out
    if storage != "f32":
        if arithmetic != "scalar":
            raise HnswError(N.ERR_ARG, "half-precision rows are read in the scalar arithmetic only")
        _check(N.lib().hnswgpu_eval_distance_matrix_storage(N.DIST[dist], STORAGE[storage], _p(q), q.shape[0], _p(r), r.shape[0], q.shape[1],
                                                            batch, _p(out)))
        return out
    _check(N.lib().hnswgpu_eval_distance_matrix_arith(N.DIST[dist], ARITH[arithmetic], _p(q), q.shape[0], _p(r), r.shape[0], q.shape[1],
                                                      batch, _p(out)))
    return out


def eval_distances(dist, a, b):
    """Distance<f32>::eval for the pairs (a[i], b[i]) on the device, by the search kernel's own distance routine."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    out = np.zeros(a.shape[0], np.float32)
    _check(N.lib().hnswgpu_eval_distances(N.DIST[dist], _p(a), _p(b), a.shape[0], a.shape[1], _p(out)))
    return out


def reload_env():
    """The HNSWGPU_* tuning / test hooks are read from the environment once per process; call this after changing them."""
    _check(N.lib().hnswgpu_reload_env())
