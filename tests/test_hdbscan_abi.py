"""The HDBSCAN entries (hnswhdb_max_clusters, hnswhdb_forest / _device, hnswhdb_graph / _device,
csrc/condensed_tree.hip) as far as a box without a GPU can see them: the ABI, every refusal that is answered before a device is
needed, the calls that need none -- and the contract of include/hnsw_mi355x_hdbscan.h restated in Python: `hdbscan_model`, a sequential pass
over the dendrogram of tests/test_dendrogram_abi.py.  tests/test_gpu_hdbscan.py imports it to build its expected answers, never from
the code under test.  Here the model is checked on a hand-made forest whose every output is written out, on the bound on K, and, where
scikit-learn is installed, against sklearn's own tree_to_labels.  CPU only."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_dendrogram_abi import dendrogram

ENTRIES = ("hnswhdb_forest", "hnswhdb_forest_device", "hnswhdb_graph", "hnswhdb_graph_device")
INF_BITS, NONE = 0x7F800000, 0xFFFFFFFF
EOM, LEAF = 0, 1
METHOD_CODE = {"eom": EOM, "leaf": LEAF}
# sentinels of the out arrays
LABEL, PROB, PCLUSTER, PW, CPARENT, CBIRTH, CSIZE, SEL, COUNT = -77, 0x7FC00123, 0xB1B1B1B1, 0x7FC00456, 0xD2D2D2D2, 0x7FC00789, 0xE3E3E3E3, 0xF4, 0x7777
STAB = 0x7FF8000000ABCDEF                                      # (a NaN's bits)


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
def bits_of(w):
    return np.ascontiguousarray(w, np.float32).view(np.uint32)


def order_bits(w):
    """the order of the spanning forest's weights: by value, -0 equal to +0, every NaN behind +inf"""
    w = np.float32(w)
    b = int(np.array(w, np.float32).view(np.uint32))
    if np.isnan(w):
        return 0xFFFFFFFF
    if b == 0x80000000:
        b = 0
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


@functools.lru_cache(maxsize=None)
def lam_of(bits):
    """lambda of a weight's stored bits"""
    w = np.array(bits, np.uint32).view(np.float32)[()]
    if np.isnan(w) or int(bits) == INF_BITS:
        return 0.0
    if w <= 0:
        return math.inf
    return 1.0 / float(w)


def term(l_row, l_birth, size):
    return 0.0 if l_row == l_birth else (l_row - l_birth) * float(size)


def max_clusters(n, mcs):
    return max(1, 2 * (n // mcs) - 1)


class Model:
    pass


def hdbscan_model(n, a, b, w, mcs, method="eom"):
    """The definitions of include/hnsw_mi355x_hdbscan.h read one after the other.  None when the forest is refused (a cycle,
    weights that descend).  Otherwise an object with K, L, cluster_parent, cluster_birth_w (bits), cluster_size, stability (math.fsum
    of the terms: the exactly rounded sum), terms (the f64 terms per cluster), selected, labels, prob (f32), point_cluster, point_w
    (bits), max_lambda, and decisions: per cluster with children other than 0, (stability, sum of S over the children, rows in its
    subtree)."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    wb = [int(x) for x in bits_of(w)]
    m = len(a)
    if any(order_bits(np.array(wb[e - 1], np.uint32).view(np.float32)) > order_bits(np.array(wb[e], np.uint32).view(np.float32)) for e in range(1, m)):
        return None
    d = dendrogram(n, list(zip(a, b)))
    if d is None:
        return None
    left, right, sizes = (x.tolist() for x in d)
    nodes = n + m
    size = [1] * n + sizes
    par = [-1] * nodes
    for e in range(m):
        par[left[e]] = par[right[e]] = n + e
    big = [s >= mcs for s in size]
    big_roots = [x for x in range(nodes) if par[x] < 0 and big[x]]
    head = [False] * nodes
    for x in range(nodes):
        if big[x]:
            head[x] = len(big_roots) >= 2 if par[x] < 0 else (big[left[par[x] - n]] and big[right[par[x] - n]])
    heads = [x for x in range(nodes - 1, -1, -1) if head[x]]
    index = {x: i + 1 for i, x in enumerate(heads)}
    K = 1 + len(heads)
    cluster = [None] * nodes                                   # of the big nodes; a parent's id is above its children's
    for x in range(nodes - 1, -1, -1):
        if big[x]:
            cluster[x] = index[x] if head[x] else (0 if par[x] < 0 else cluster[par[x]])
    cparent, cbirth, csize = [NONE] + [0] * (K - 1), [INF_BITS] * K, [n] + [0] * (K - 1)
    for x in heads:
        c = index[x]
        csize[c] = size[x]
        cparent[c] = 0 if par[x] < 0 else cluster[par[x]]
        cbirth[c] = INF_BITS if par[x] < 0 else wb[par[x] - n]
    top = list(range(nodes))                                   # the highest small ancestor-or-self of a small node
    for x in range(nodes - 1, -1, -1):
        if not big[x] and par[x] >= 0 and not big[par[x]]:
            top[x] = top[par[x]]
    pc, pw = [0] * n, [INF_BITS] * n
    for v in range(n):
        t = top[v]
        if par[t] >= 0:
            pc[v], pw[v] = cluster[par[t]], wb[par[t] - n]
    lam_birth = [lam_of(x) for x in cbirth]
    terms, maxlam, kids = [[] for _ in range(K)], [0.0] * K, [[] for _ in range(K)]
    for v in range(n):
        terms[pc[v]].append(term(lam_of(pw[v]), lam_birth[pc[v]], 1))
        maxlam[pc[v]] = max(maxlam[pc[v]], lam_of(pw[v]))
    for c in range(1, K):
        terms[cparent[c]].append(term(lam_birth[c], lam_birth[cparent[c]], csize[c]))
        maxlam[cparent[c]] = max(maxlam[cparent[c]], lam_birth[c])
        kids[cparent[c]].append(c)
    stab = [math.inf if any(math.isinf(t) for t in ts) else math.fsum(ts) for ts in terms]
    S, wins, rows_under, decisions = [0.0] * K, [False] * K, [len(ts) for ts in terms], {}
    for c in range(K - 1, 0, -1):
        assert len(kids[c]) in (0, 2), "a cluster other than 0 has no child or two"
        sub = S[kids[c][0]] + S[kids[c][1]] if kids[c] else 0.0
        if kids[c]:
            rows_under[c] += rows_under[kids[c][0]] + rows_under[kids[c][1]]
            decisions[c] = (stab[c], sub, rows_under[c])
        wins[c] = not kids[c] if method == "leaf" else stab[c] >= sub
        S[c] = max(stab[c], sub)
    selected, under_winner, sel_of = [False] * K, [False] * K, [-1] * K
    for c in range(1, K):
        p = cparent[c]
        assert p < c, "a parent cluster has the smaller index"
        under_winner[c] = p != 0 and (wins[p] or under_winner[p])
        selected[c] = wins[c] and not under_winner[c]
        sel_of[c] = c if selected[c] else (sel_of[p] if p != 0 else -1)
    label_of, L = {}, 0
    for c in range(K):
        if selected[c]:
            label_of[c] = L
            L += 1
    labels, prob = [-1] * n, [0.0] * n
    for v in range(n):
        q = sel_of[pc[v]]
        if q < 0:
            continue
        labels[v] = label_of[q]
        lv = lam_of(pw[v])
        prob[v] = 1.0 if maxlam[q] == 0 or lv >= maxlam[q] else lv / maxlam[q]
    r = Model()
    r.K, r.L, r.n, r.m = K, L, n, m
    r.cluster_parent, r.cluster_birth_w, r.cluster_size = np.array(cparent, np.uint32), np.array(cbirth, np.uint32), np.array(csize, np.uint32)
    r.stability, r.terms, r.selected = np.array(stab, np.float64), terms, np.array(selected, np.uint8)
    r.labels, r.prob = np.array(labels, np.int32), np.array(prob, np.float64).astype(np.float32)
    r.point_cluster, r.point_w = np.array(pc, np.uint32), np.array(pw, np.uint32)
    r.max_lambda, r.decisions, r.kids = maxlam, decisions, kids
    return r


def has_margins(model):
    """every excess-of-mass decision of the model is further from a tie than any order of summation can move the two sides"""
    for c, (own, sub, rows) in model.decisions.items():
        if not abs(own - sub) > 4 * rows * 2.0 ** -53 * max(own, sub):
            return False
    return True


def same_partition(x, y):
    pairs = {}
    for i, j in zip(x, y):
        if (i < 0) != (j < 0):
            return False
        if i >= 0 and pairs.setdefault(int(i), int(j)) != int(j):
            return False
    return len(set(pairs.values())) == len(pairs)


HAND_A = [0, 1, 3, 4, 2, 5, 7, 8, 9]
HAND_B = [1, 2, 4, 5, 3, 6, 8, 9, 10]
HAND_W = [0.25, 0.25, 0.5, 0.5, 1.0, 2.0, 2.0, 2.0, 4.0]


def test_model_on_a_hand_made_forest():
    """12 vertices.  {0, 1, 2} closes at 0.25 (node 13), {3, 4, 5} at 0.5 (node 15), the two join at 1 (node 16), vertex 6 joins them
    at 2 (node 17).  {7, 8, 9} closes at 2 (node 19), vertex 10 joins it at 4 (node 20).  Vertex 11 stays alone."""
    r = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3)
    # two big dendrogram roots, 20 and 17: clusters 1 and 2, children of 0.  Below 17 node 16 continues (its sibling 6 is small) and
    # splits truly into 15 and 13: clusters 3 and 4.  Node 19 continues 20.
    assert (r.K, r.L) == (5, 3)
    assert r.cluster_parent.tolist() == [NONE, 0, 0, 2, 2]
    assert r.cluster_birth_w.view(np.float32).tolist() == [math.inf, math.inf, math.inf, 1.0, 1.0]
    assert r.cluster_size.tolist() == [12, 4, 7, 3, 3]
    assert r.point_cluster.tolist() == [4, 4, 4, 3, 3, 3, 2, 1, 1, 1, 1, 0]
    assert r.point_w.view(np.float32).tolist() == [0.25, 0.25, 0.25, 0.5, 0.5, 0.5, 2.0, 2.0, 2.0, 2.0, 4.0, math.inf]
    # cluster 1: three points at lambda 1/2 and one at 1/4 over a birth at 0.  Cluster 2: one point at 1/2 and two children of three
    # born at 1.  Cluster 3: three points at 2 over 1.  Cluster 4: three points at 4 over 1.
    assert r.stability.tolist() == [0.0, 1.75, 6.5, 3.0, 9.0]
    assert r.decisions == {2: (6.5, 12.0, 9)}                 # 6.5 < 3 + 9: cluster 2 loses to its children
    assert r.selected.tolist() == [0, 1, 0, 1, 1]
    assert r.labels.tolist() == [2, 2, 2, 1, 1, 1, -1, 0, 0, 0, 0, -1]
    assert r.prob.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.5, 0.0]
    assert r.max_lambda == [0.0, 0.5, 1.0, 2.0, 4.0]
    leaf = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3, "leaf")
    assert leaf.selected.tolist() == [0, 1, 0, 1, 1] and leaf.labels.tolist() == r.labels.tolist()
    # mcs = 4: the two triples are small now and leave cluster 2 at weight 1, {7, 8, 9} leaves cluster 1 at weight 4
    r = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 4)
    assert (r.K, r.L) == (3, 2) and r.cluster_parent.tolist() == [NONE, 0, 0] and r.cluster_size.tolist() == [12, 4, 7]
    assert r.point_cluster.tolist() == [2] * 7 + [1] * 4 + [0]
    assert r.point_w.view(np.float32).tolist() == [1.0] * 6 + [2.0] + [4.0] * 4 + [math.inf]
    assert r.stability.tolist() == [0.0, 1.0, 6.5] and r.selected.tolist() == [0, 1, 1]
    assert r.labels.tolist() == [1] * 7 + [0] * 4 + [-1] and r.prob.tolist() == [1.0] * 6 + [0.5] + [1.0] * 4 + [0.0]
    # mcs = 7: one big dendrogram root, 17, which continues cluster 0: no cluster but the root, all noise
    r = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 7)
    assert (r.K, r.L) == (1, 0) and r.labels.tolist() == [-1] * 12 and r.point_cluster.tolist() == [0] * 12
    assert r.point_w.view(np.float32).tolist() == [2.0] * 7 + [math.inf] * 5  # {0 .. 5} is small: it leaves with vertex 6, at weight 2
    assert r.stability.tolist() == [3.5]
    # a parent that wins: the same forest with the two triples' own merges close to the join at 1
    w = [0.5, 0.5, 0.5, 0.5, 1.0, 8.0, 8.0, 8.0, 8.0]
    r = hdbscan_model(12, HAND_A, HAND_B, w, 3)
    assert r.stability.tolist() == [0.0, 0.5, 6.125, 3.0, 3.0] and r.decisions == {2: (6.125, 6.0, 9)}
    assert r.selected.tolist() == [0, 1, 1, 0, 0] and r.labels.tolist() == [1] * 7 + [0] * 4 + [-1]
    assert hdbscan_model(12, HAND_A, HAND_B, w, 3, "leaf").selected.tolist() == [0, 1, 0, 1, 1]
    # refused: a cycle, weights that descend (equal weights, and -0 after +0, do not)
    assert hdbscan_model(3, [0, 1, 2], [1, 2, 0], [1, 1, 1], 2) is None
    assert hdbscan_model(3, [0, 1], [1, 2], [2, 1], 2) is None
    assert hdbscan_model(3, [0, 1], [1, 2], [0.0, -0.0], 2) is not None and hdbscan_model(3, [0, 1], [1, 2], [np.inf, np.nan], 2) is not None
    assert hdbscan_model(3, [0, 1], [1, 2], [np.nan, np.inf], 2) is None


def balanced_pairs(pairs):
    """2 * pairs vertices (pairs a power of two): the pairs (2 i, 2 i + 1) first, then pairs of pairs, and so on: every merge above
    the pairs is a true split at mcs = 2.  Weights 1, 2, 4, .. by level."""
    n, a, b, w = 2 * pairs, [], [], []
    width, level = 2, 0
    while width <= n:
        for s in range(0, n, width):
            a.append(s + width // 2 - 1)
            b.append(s + width // 2)
            w.append(float(2 ** level))
        width *= 2
        level += 1
    return n, a, b, w


def test_model_keeps_the_bound_on_the_number_of_clusters(native):
    L = native.lib()
    for n, mcs, want in ((0, 2, 1), (1, 2, 1), (3, 2, 1), (4, 2, 3), (12, 3, 7), (12, 5, 3), (12, 7, 1), (100, 2, 99), ((1 << 31) - 1, 2, (1 << 31) - 3)):
        assert max_clusters(n, mcs) == want and L.hnswhdb_max_clusters(n, mcs) == want, (n, mcs)
    assert L.hnswhdb_max_clusters(10, 0) == 0 and L.hnswhdb_max_clusters(10, 1) == 19
    for pairs in (2, 4, 16, 64):                               # at equality: a balanced binary cluster tree over the pairs
        n, a, b, w = balanced_pairs(pairs)
        r = hdbscan_model(n, a, b, w, 2)
        assert r.K == max_clusters(n, 2) == 2 * pairs - 1, pairs
        assert r.K <= L.hnswhdb_max_clusters(n, 2)
    for pairs in (1, 5, 33):                                   # pairs that stay apart: every pair a child of cluster 0
        n = 2 * pairs
        r = hdbscan_model(n, range(0, n, 2), range(1, n, 2), [1.0] * pairs, 2)
        assert r.K == (1 if pairs == 1 else 1 + pairs) and r.K <= max_clusters(n, 2), pairs
    rng = np.random.default_rng(5)
    for _ in range(60):
        n = int(rng.integers(1, 80))
        v = rng.permutation(n)
        e = [(int(v[i]), int(v[rng.integers(0, i)])) for i in range(1, n) if rng.random() < 0.9]
        w = np.sort(rng.integers(1, 6, len(e))).astype(np.float32)
        for mcs in (2, 3, 5):
            r = hdbscan_model(n, [x for x, _ in e], [y for _, y in e], w, mcs)
            assert 1 <= r.K <= max_clusters(n, mcs), (n, mcs, r.K)
            assert r.L == int(r.selected.sum()) and set(r.labels.tolist()) <= set(range(-1, r.L))


def blob_mst(rng, n, blobs):
    """a float32 minimum spanning tree of Gaussian blobs in the plane, ascending: (n, a, b, w), or None when two weights are equal"""
    from scipy.sparse.csgraph import minimum_spanning_tree
    from scipy.spatial.distance import pdist, squareform
    X = np.concatenate([rng.normal(rng.normal(0, 6, 2), rng.uniform(.3, 1.5), (max(1, n // blobs), 2)) for _ in range(blobs)]).astype(np.float32)
    n = len(X)
    if n < 2:
        return None
    T = minimum_spanning_tree(squareform(pdist(X)).astype(np.float32)).tocoo()
    o = np.argsort(T.data, kind="stable")
    a, b, w = T.row[o].astype(np.uint32), T.col[o].astype(np.uint32), T.data[o].astype(np.float32)
    if len(w) != n - 1 or len(np.unique(w)) < len(w) or not (w > 0).all():
        return None
    return n, a, b, w


def test_model_gives_sklearns_partition():
    tree = pytest.importorskip("sklearn.cluster._hdbscan._tree")
    pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(1)
    done = 0
    for trial in range(60):
        got = blob_mst(rng, int(rng.integers(2, 160)), int(rng.integers(1, 6)))
        mcs = int(rng.integers(2, 12))
        if got is None:
            continue
        n, a, b, w = got
        left, right, size = dendrogram(n, list(zip(a.tolist(), b.tolist())))
        H = np.zeros(n - 1, dtype=tree.HIERARCHY_dtype)
        H["left_node"], H["right_node"], H["value"], H["cluster_size"] = left, right, w.astype(np.float64), size
        for method in ("eom", "leaf"):
            theirs = tree.tree_to_labels(H, mcs, method, False, 0.0, None)[0]
            mine = hdbscan_model(n, a, b, w, mcs, method)
            assert same_partition(mine.labels, theirs), (trial, n, mcs, method)
        done += 1
    assert done >= 40


# ----------------------------------------------------------------------------------------------------- the ABI
class Outs:
    """out arrays at their sentinels: n vertices, `slots` clusters"""

    def __init__(self, n, slots):
        self.labels, self.prob = np.full(n, LABEL, np.int32), np.full(n, PROB, np.uint32)
        self.pc, self.pw = np.full(n, PCLUSTER, np.uint32), np.full(n, PW, np.uint32)
        self.cparent, self.cbirth, self.csize = np.full(slots, CPARENT, np.uint32), np.full(slots, CBIRTH, np.uint32), np.full(slots, CSIZE, np.uint32)
        self.stab, self.sel = np.full(slots, STAB, np.uint64), np.full(slots, SEL, np.uint8)
        self.k, self.l = np.full(1, COUNT, np.uint64), np.full(1, COUNT + 1, np.uint64)

    def arrays(self):
        return {"labels": self.labels, "prob": self.prob, "pc": self.pc, "pw": self.pw, "cparent": self.cparent, "cbirth": self.cbirth,
                "csize": self.csize, "stab": self.stab, "sel": self.sel, "n_clusters": self.k, "n_labels": self.l}

    def untouched(self, vertices_from=0, clusters_from=0):
        v, c = vertices_from, clusters_from
        return bool((self.labels[v:] == LABEL).all() and (self.prob[v:] == PROB).all() and (self.pc[v:] == PCLUSTER).all() and (self.pw[v:] == PW).all()
                    and (self.cparent[c:] == CPARENT).all() and (self.cbirth[c:] == CBIRTH).all() and (self.csize[c:] == CSIZE).all()
                    and (self.stab[c:] == STAB).all() and (self.sel[c:] == SEL).all()
                    and (v or c or (self.k[0] == COUNT and self.l[0] == COUNT + 1)))


ORDER = ("labels", "prob", "pc", "pw", "cparent", "cbirth", "csize", "stab", "sel", "n_clusters", "n_labels")


def test_header_declares_the_five_symbols(native):
    N = _N()
    protos = N.HDBSCAN_HEADER.prototypes
    assert sorted(protos) == sorted(ENTRIES + ("hnswhdb_max_clusters",)) == sorted(N.HDBSCAN_SYMBOLS)
    assert not set(protos) & set(N.SYMBOLS)                     # hnsw_mi355x.h keeps its own set as it is
    for name, (res, args, _names, text) in protos.items():     # bound with the signature generated from the header's text
        fn = getattr(native.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), text
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if " T hnswhdb_" in l} == set(protos)    # and nothing exported without a prototype
    pkg = os.path.join(os.path.dirname(native.LIB_PATH), "hnsw_mi355x_hdbscan.h")             # the package's own copy is the tree's
    assert os.path.exists(pkg) and open(pkg).read() == open(N.HDBSCAN_HEADER_PATH).read()
    assert protos["hnswhdb_max_clusters"][0] is C.c_uint64 and protos["hnswhdb_max_clusters"][2] == ["n", "min_cluster_size"]
    outs = ["labels", "prob", "point_cluster", "point_w", "cluster_parent", "cluster_birth_w", "cluster_size", "stability", "selected"]
    counts = ["out_n_clusters", "out_n_labels"]
    six = ["a", "b", "w", "left", "right", "size"]
    assert protos[ENTRIES[0]][2] == ["device", "n", "m", "a", "b", "w", "min_cluster_size", "method"] + ["out_" + x for x in outs] + counts
    assert protos[ENTRIES[1]][2] == (["device", "n", "m", "d_a", "d_b", "d_w", "min_cluster_size", "method"] + ["d_out_" + x for x in outs] + counts
                                     + ["stream"])
    assert protos[ENTRIES[2]][2] == (["idx", "k", "ef", "mode", "core_k", "min_cluster_size", "method"] + ["out_" + x for x in six + outs] + counts
                                     + ["out_n_edges"])
    assert protos[ENTRIES[3]][2] == (["idx", "k", "ef", "mode", "core_k", "min_cluster_size", "method"] + ["d_out_" + x for x in six + outs] + counts
                                     + ["out_n_edges", "stream"])
    for name in ENTRIES:
        assert protos[name][0] is C.c_int
    assert N.HDBSCAN_HEADER.constants["HNSWGPU_SELECT_EOM"] == EOM and N.HDBSCAN_HEADER.constants["HNSWGPU_SELECT_LEAF"] == LEAF
    text = open(N.HDBSCAN_HEADER_PATH).read()
    assert '#include "hnsw_mi355x.h"' in text
    doc = text[text.index("HDBSCAN: condensed tree"):text.index("int hnswhdb_graph_device")]
    for word in ("merge order", "DENDROGRAM ROOT", "BIG", "-0 included", "CONTINUES", "HEAD", "descending node id", "2 floor(n / mcs) - 1",
                 "UINT32_MAX", "highest small ancestor-or-self", "inf - inf", "no FMA", "the same bytes", "ties go to the parent",
                 "HNSWGPU_SELECT_LEAF", "ascending cluster index", "maxlambda", "behind slot K - 1", "weights that descend", "byte for byte",
                 "Out of scope", "allow_single_cluster", "cluster_selection_epsilon", "max_cluster_size", "GLOSH", "soft clustering", "DataId",
                 "F16 storage", "sharding", "several host threads"):
        assert word in doc, word
    assert hasattr(native.Hnsw, "hdbscan") and callable(native.forest_hdbscan) and hasattr(native.SpanningForestResult, "hdbscan")
    assert hasattr(native.HdbscanResult, "condensed_tree")


def test_forest_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    ea, eb, ew = np.array([0, 1, 2], np.uint32), np.array([1, 2, 3], np.uint32), np.array([1, 2, 3], np.float32)
    o = Outs(4, 3)

    def host(n=4, m=3, a=ea, b=eb, w=ew, mcs=2, method=EOM, **kw):
        arrays = {**o.arrays(), **kw}
        return L.hnswhdb_forest(0, n, m, _p(a), _p(b), _p(w), mcs, method, *[_p(arrays[x]) for x in ORDER])

    def dev(n=4, m=3, a=ea, b=eb, w=ew, mcs=2, method=EOM, **kw):
        arrays = {**o.arrays(), **kw}
        return L.hnswhdb_forest_device(0, n, m, _p(a), _p(b), _p(w), mcs, method, *[_p(arrays[x]) for x in ORDER], None)

    def refused(call, word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), kw.keys()
    for call in (host, dev):                                   # what either form sees without reading an array
        refused(call, "2^31", n=1 << 31, m=1)
        refused(call, "at most n - 1", m=4)
        refused(call, "at most n - 1", n=3)
        refused(call, "at most n - 1", n=0, m=1)
        refused(call, "at most n - 1", m=1 << 40)
        for name in ("a", "b", "w"):
            refused(call, "null a, b or w", **{name: None})
        for mcs in (0, 1, 1 << 31, 1 << 40, (1 << 64) - 1):
            refused(call, "min_cluster_size", mcs=mcs)
        for method in (2, 7, 0xFFFFFFFF):
            refused(call, "unknown method", method=method)
        refused(call, "null out_labels", labels=None)
        refused(call, "out_n_clusters or out_n_labels", n_clusters=None)
        refused(call, "out_n_clusters or out_n_labels", n_labels=None)
        refused(call, "2^31", n=1 << 31, m=1 << 31, a=None, mcs=0)    # several faults at once: the dendrogram's first, in its order
        refused(call, "null a, b or w", a=None, mcs=1)
    # the ends and the weights: the host form reads its arrays on the host (the device form's kernels need a device)
    refused(host, "not below n", a=np.array([0, 4, 2], np.uint32))
    refused(host, "not below n", b=np.array([1, 2, 0xFFFFFFFF], np.uint32))
    refused(host, "itself", a=np.array([0, 2, 2], np.uint32))
    refused(host, "descend", w=np.array([1, 3, 2], np.float32))
    refused(host, "descend at edge 1", w=np.array([1, 0.5, 0.25], np.float32))
    refused(host, "descend", w=np.array([1, np.nan, np.inf], np.float32))
    refused(host, "descend", w=np.array([0.0, -1.0, 2.0], np.float32))
    refused(host, "not below n", a=np.array([0, 4, 2], np.uint32), w=np.array([3, 2, 1], np.float32))    # the ends first
    # a cycle is the device's to find: without one the call says so, with one it is refused like the rest
    rc = host(a=np.array([0, 1, 0], np.uint32), b=np.array([1, 2, 2], np.uint32))
    assert rc == (N.ERR_ARG if L.hnswgpu_device_count() > 0 else N.ERR_DEVICE), (rc, N.last_error())
    assert o.untouched()
    for bad in (dict(n=3, a=[0, 1, 2], b=[1, 2, 0], weights=[1, 1, 1]), dict(n=3, a=[0], b=[3], weights=[1]), dict(n=3, a=[1], b=[1], weights=[1]),
                dict(n=3, a=[0, 1], b=[1], weights=[1, 1]), dict(n=3, a=[0, 1], b=[1, 2], weights=[2, 1]),
                dict(n=3, a=[0, 1], b=[1, 2], weights=[1, 2], min_cluster_size=1), dict(n=3, a=[0, 1], b=[1, 2], weights=[1, 2], method="best")):
        with pytest.raises(native.HnswError) as err:           # the Python function hands the refusals on
            native.forest_hdbscan(**{"min_cluster_size": 2, **bad})
        assert err.value.code == N.ERR_ARG


def test_no_vertex_needs_no_device(native):
    N = _N()
    L = native.lib()
    o = Outs(4, 3)
    for form in ("host", "device"):
        o.k[0], o.l[0] = COUNT, COUNT + 1
        args = (0, 0, 0, None, None, None, 5, LEAF, None, None, None, None, None, None, None, None, None, _p(o.k), _p(o.l))
        rc = L.hnswhdb_forest(*args) if form == "host" else L.hnswhdb_forest_device(*args, None)
        assert rc == N.OK and o.k[0] == 0 and o.l[0] == 0, form
        o.k[0], o.l[0] = COUNT, COUNT + 1
        assert o.untouched()
    got = native.forest_hdbscan(0, [], [], [], 2)
    assert got.n_clusters == 0 and got.n_labels == 0 and len(got.labels) == 0 and got.labels.dtype == np.int32 and len(got.stability) == 0
    assert got.condensed_tree().shape == (0,)


def test_index_entries_answer_every_refusal_before_a_device_is_needed(native):
    """the dendrogram call's refusals with its words -- its six arrays are optional here --, then the new ones"""
    from test_dendrogram_abi import _Outs, _small
    N = _N()
    L = native.lib()
    X, h = _small(native)
    d, o = _Outs(49), Outs(50, 49)
    base = dict(idx=h.handle, k=3, ef=0, mode=0, core_k=0, mcs=5, method=EOM, a=d.a, b=d.b, w=d.w, left=d.left, right=d.right, size=d.size, count=d.count)

    def args(kw):
        kw = {**base, **o.arrays(), **kw}
        return [kw["idx"], kw["k"], kw["ef"], kw["mode"], kw["core_k"], kw["mcs"], kw["method"]] + [_p(kw[x]) for x in ("a", "b", "w", "left", "right",
                                                                                                                         "size") + ORDER] + [_p(kw["count"])]

    def host(**kw):
        return L.hnswhdb_graph(*args(kw))

    def dev(**kw):
        return L.hnswhdb_graph_device(*args(kw), None)

    def dendro(**kw):
        kw = {**base, **kw}
        return L.hnswgpu_graph_dendrogram(kw["idx"], kw["k"], kw["ef"], kw["mode"], kw["core_k"], *[_p(kw[x]) for x in ("a", "b", "w", "left", "right",
                                                                                                                        "size", "count")])
    big = (1 << 30) // 50 + 1
    for call in (host, dev):
        for kw in (dict(idx=None), dict(count=None), dict(k=0), dict(mode=2), dict(k=big), dict(k=1 << 40), dict(core_k=4), dict(core_k=1 << 63),
                   dict(k=4097), dict(k=0, ef=32), dict(mode=7, ef=32), dict(core_k=4, ef=32), dict(k=0, mcs=0), dict(count=None, labels=None)):
            assert dendro(**kw) == N.ERR_ARG
            words = N.last_error()
            rc = call(**kw)
            assert rc == N.ERR_ARG and N.last_error() == words, (kw.keys(), rc, N.last_error(), words)
            assert o.untouched() and d.untouched(), kw.keys()
        for kw, word in ((dict(mcs=0), "min_cluster_size"), (dict(mcs=1), "min_cluster_size"), (dict(mcs=1 << 31), "min_cluster_size"),
                         (dict(method=2), "unknown method"), (dict(labels=None), "null out_labels"),
                         (dict(n_clusters=None), "out_n_clusters or out_n_labels"), (dict(n_labels=None), "out_n_clusters or out_n_labels")):
            rc = call(**kw)
            assert rc == N.ERR_ARG and word in N.last_error(), (kw.keys(), rc, N.last_error())
            assert o.untouched() and d.untouched(), kw.keys()
    for bad in (dict(knbn=0), dict(knbn=3, mode="both"), dict(knbn=3, ef=0), dict(knbn=3, core_k=4), dict(knbn=3, core_k=-1), dict(knbn=3, method="x"),
                dict(knbn=3, min_cluster_size=1)):
        with pytest.raises(native.HnswError) as err:           # the Python method hands the refusals on
            h.hdbscan(**{"min_cluster_size": 5, **bad})
        assert err.value.code == N.ERR_ARG


def test_an_empty_index_has_no_cluster_and_needs_no_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    for method in ("eom", "leaf"):
        res = e.hdbscan(5, 5, None, "union", None, method)
        assert res.n_clusters == 0 and res.n_labels == 0 and len(res.labels) == 0 and res.forest.n_edges == 0 and res.dendrogram.n_edges == 0
    e.parallel_insert(np.zeros((0, 8), np.float32))            # (a handle exists from the first insertion on)
    counts = np.full(3, COUNT, np.uint64)
    none = [None] * 15
    for form in ("host", "device"):
        counts[:] = COUNT
        a = [e.handle, 5, 0, 0, 2, 5, EOM] + none + [_p(counts[0:1]), _p(counts[1:2]), _p(counts[2:3])]
        rc = L.hnswhdb_graph(*a) if form == "host" else L.hnswhdb_graph_device(*a, None)
        assert rc == N.OK and counts.tolist() == [0, 0, 0], (form, rc, N.last_error())
        a[5] = 1                                               # still refused
        counts[:] = COUNT
        rc = L.hnswhdb_graph(*a) if form == "host" else L.hnswhdb_graph_device(*a, None)
        assert rc == N.ERR_ARG and counts.tolist() == [COUNT] * 3


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    from test_dendrogram_abi import _small
    N = _N()
    L = native.lib()
    X, h = _small(native)
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_hdbscan.py checks the answers)
        got = native.forest_hdbscan(12, HAND_A, HAND_B, HAND_W, 3)
        assert got.labels.tolist() == [2, 2, 2, 1, 1, 1, -1, 0, 0, 0, 0, -1] and got.stability.tolist() == [0.0, 1.75, 6.5, 3.0, 9.0]
        got = native.forest_hdbscan(3, [], [], [], 2)
        assert got.n_clusters == 1 and got.labels.tolist() == [-1, -1, -1]
        got = h.hdbscan(5, 3)
        assert got.n_clusters >= 1 and len(got.labels) == 50
        return
    for call in (lambda: native.forest_hdbscan(12, HAND_A, HAND_B, HAND_W, 3), lambda: native.forest_hdbscan(3, [], [], [], 2), lambda: h.hdbscan(5, 3)):
        with pytest.raises(native.HnswError) as e:
            call()
        assert e.value.code == N.ERR_DEVICE
    o = Outs(12, 7)
    a, b, w = np.array(HAND_A, np.uint32), np.array(HAND_B, np.uint32), np.array(HAND_W, np.float32)
    rc = L.hnswhdb_forest_device(0, 12, 9, _p(a), _p(b), _p(w), 3, EOM, *[_p(o.arrays()[x]) for x in ORDER], None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()


def test_condensed_tree_rows_of_a_result(native):
    """HdbscanResult.condensed_tree on the hand-made forest's answer, built from the model: sklearn's layout, clusters numbered n + c"""
    r = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3)
    res = native.HdbscanResult(r.labels, r.prob, r.point_cluster, r.point_w.view(np.float32), r.cluster_parent, r.cluster_birth_w.view(np.float32),
                               r.cluster_size, r.stability, r.selected.astype(bool), r.K, r.L)
    t = res.condensed_tree()
    assert t.dtype.names == ("parent", "child", "value", "cluster_size") and len(t) == 4 + 12
    assert t["parent"].tolist() == [12, 12, 14, 14] + [16, 16, 16, 15, 15, 15, 14, 13, 13, 13, 13, 12]
    assert t["child"].tolist() == [13, 14, 15, 16] + list(range(12))
    assert t["value"].tolist() == [0.0, 0.0, 1.0, 1.0] + [4.0, 4.0, 4.0, 2.0, 2.0, 2.0, 0.5, 0.5, 0.5, 0.5, 0.25, 0.0]
    assert t["cluster_size"].tolist() == [4, 7, 3, 3] + [1] * 12
    try:
        from sklearn.cluster._hdbscan._tree import CONDENSED_dtype
    except ImportError:
        return
    assert t.dtype == CONDENSED_dtype
