"""The prediction stage of HDBSCAN (hnswhdp_core_distances, hnswhdp_assign, hnswhdp_predict and their _device forms,
csrc/cluster_predict.hip) as far as a box without a GPU can see it: the ABI, every refusal -- the host forms answer all of them before
a device is needed --, the calls that need none, and section 2 of include/hnsw_mi355x_hdbscan_predict.h restated in Python:
`predict_model`, over the fields of `hdbscan_model` / `select_model` (imported).  tests/test_gpu_hdbscan_predict.py imports it to
build its expected answers, never from the code under test.  Here the model is checked on a hand-made case whose every output is
written out, and on a property of three blobs.  CPU only."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from test_hdbscan_abi import HAND_A, HAND_B, HAND_W, NONE, Model, bits_of, hdbscan_model, lam_of
from test_hdbscan_select_abi import model_of_arrays, select_model

ENTRIES = ("hnswhdp_core_distances", "hnswhdp_core_distances_device", "hnswhdp_assign", "hnswhdp_assign_device", "hnswhdp_predict",
           "hnswhdp_predict_device")
INF_BITS = 0x7F800000
# sentinels of the out arrays
LABEL, PROB, SCORE, NEAREST, WEIGHT, CLUSTER = -77, 0x7FC00123, 0x7FC00321, 0xABCD0001, 0x7FC00456, 0xABCD0002


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
def order_of(bits):
    """dist_order_bits of a weight's stored bits: by value, -0 as +0, every NaN behind +inf"""
    b = int(bits)
    if math.isnan(float(np.array(b, np.uint32).view(np.float32)[()])):
        return 0xFFFFFFFF
    if b == 0x80000000:
        b = 0
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def later(w, other):
    """the later of two weights' bits; a tie keeps the earlier argument"""
    return other if order_of(other) > order_of(w) else w


def predict_model(tree, selected, eps, death, core, nbr_pos, nbr_dist, counts, core_k):
    """Section 2 of include/hnsw_mi355x_hdbscan_predict.h, query by query.  tree: a model with K, n, cluster_parent, cluster_birth_w
    (bits), point_cluster, point_w (bits), max_lambda; selected: u8[K]; death: f64[K] or None; core: u32 bits [n]; nbr_pos (nq, k)
    u32, nbr_dist (nq, k) u32 bits, counts (nq).  Returns an object with labels (i32), prob (f32), score (f32, or None), nearest
    (u32), w (u32 bits), cluster (u32)."""
    K = tree.K
    parent, birth = [int(x) for x in tree.cluster_parent], [int(x) for x in tree.cluster_birth_w]
    pc, pw, maxlam = [int(x) for x in tree.point_cluster], [int(x) for x in tree.point_w], tree.max_lambda
    selected = [int(x) for x in selected]
    eps = float(np.float32(eps))
    single = K >= 1 and selected[0] == 1 and sum(1 for s in selected if s) == 1
    label_of, sel_of = {}, [-1] * K
    for c in range(K):
        if selected[c]:
            label_of[c] = len(label_of)
        sel_of[c] = c if selected[c] else (sel_of[parent[c]] if c != 0 else -1)
    nq = len(counts)
    labels, prob, score = [-1] * nq, [0.0] * nq, [0.0] * nq
    nearest, weight, cluster = [NONE] * nq, [INF_BITS] * nq, [0] * nq
    for q in range(nq):
        cnt = int(counts[q])
        lam_q, c = 0.0, 0
        if cnt:
            slot = min(int(core_k), cnt) - 1
            core_q = int(nbr_dist[q][slot]) if slot >= 0 else 0
            best = None
            for s in range(cnt):
                j = int(nbr_pos[q][s])
                mr = later(later(int(nbr_dist[q][s]), core_q), int(core[j]))
                key = (order_of(mr) << 32) | s
                if best is None or key < best[0]:
                    best = (key, j, mr)
            nearest[q], weight[q] = best[1], best[2]
            lam_q = lam_of(weight[q])
            c = pc[nearest[q]]
            if not lam_of(pw[nearest[q]]) <= lam_q:
                while c != 0 and lam_of(birth[c]) >= lam_q:
                    c = parent[c]
            cluster[q] = c
        if death is not None and K:
            d = float(death[c])
            if d == 0 or lam_q >= d:
                score[q] = 0.0
            elif math.isinf(d):
                score[q] = 1.0
            else:
                score[q] = (d - lam_q) / d
        if not cnt:
            continue
        if single:
            thr = 1.0 / eps if eps > 0 else maxlam[0]
            L = 0 if lam_q >= thr else -1
        else:
            L = sel_of[c]
        if L < 0:
            continue
        labels[q] = label_of[L]
        prob[q] = 1.0 if maxlam[L] == 0 or lam_q >= maxlam[L] else lam_q / maxlam[L]
    r = Model()
    r.labels, r.prob = np.array(labels, np.int32), np.array(prob, np.float64).astype(np.float32)
    r.score = None if death is None else np.array(score, np.float64).astype(np.float32)
    r.nearest, r.w, r.cluster = np.array(nearest, np.uint32), np.array(weight, np.uint32), np.array(cluster, np.uint32)
    return r


# the hand-made case: the 12-vertex forest of tests/test_hdbscan_abi.py, rows of knbn = 3 slots, core_k = 2
INF = math.inf
HAND_CORE = [0, 0, 0, 0, 0, 0, 2.0, 0, 0, 0, 4.0, 0]
HAND_ROWS = [                                                  # (positions, distances): the count is their length
    ([3], [0.5]),                                              # 0  lambda_j = 2 = lambda_q: no climb
    ([3], [0.25]),                                             # 1  lambda_j = 2 < lambda_q = 4: no climb
    ([3], [1.0]),                                              # 2  lambda_j = 2 > lambda_q = 1 = the birth of 3: the climb goes on, to 2
    ([0], [0.5]),                                              # 3  lambda_j = 4 > 2; the birth of 4, 1, is below 2: a climb of 0 steps
    ([0], [2.0]),                                              # 4  lambda_q = 1/2: 4 -> 2, one step
    ([0], [INF]),                                              # 5  lambda_q = 0: 4 -> 2 -> 0, two steps
    ([], []),                                                  # 6  the empty row
    ([7, 0, 1], [2.0, 2.0, 2.0]),                              # 7  every slot at mr = 2: slot 0 wins
    ([0, 7, 1], [1.0, 2.0, 2.0]),                              # 8  core(q) = 2 lifts slot 0 to the others' mr: slot 0 wins
    ([3, 5], [-0.0, 0.0]),                                     # 9  -0, core(q) = +0, core[3] = +0 tie: the first argument's bits stay
    ([6], [0.5]),                                              # 10 core[6] = 2 is the largest of the three
    ([10, 7], [1.0, 3.0]),                                     # 11 core(q) = 3 and core[10] = 4: slot 1, at 3, is nearer than slot 0, at 4
]


def hand_rows(k=3):
    nq = len(HAND_ROWS)
    pos, dist, counts = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    for q, (p, d) in enumerate(HAND_ROWS):
        pos[q, :len(p)], dist[q, :len(d)], counts[q] = p, d, len(p)
    return pos, dist.view(np.uint32), counts


def hand_case(mcs=3, **select):
    """(tree, selection) of the hand-made forest"""
    base = hdbscan_model(12, HAND_A, HAND_B, HAND_W, mcs)
    return base, select_model(base, **select)


def f32(x):
    return float(np.float32(x))


def test_model_on_the_hand_made_case():
    """K = 5: clusters 1 = {7 .. 10} and 2 = {0 .. 6} under 0, 3 = {3, 4, 5} and 4 = {0, 1, 2} under 2, born at weight 1; maxlambda
    [0, 1/2, 1, 2, 4]; death [4, 1/2, 4, 2, 4]; selected {1, 3, 4} with labels 0, 1, 2"""
    base, sel = hand_case()
    assert sel.selected.tolist() == [0, 1, 0, 1, 1] and sel.death.tolist() == [4.0, 0.5, 4.0, 2.0, 4.0]
    pos, dist, counts = hand_rows()
    core = bits_of(HAND_CORE)
    r = predict_model(base, sel.selected, 0.0, sel.death, core, pos, dist, counts, 2)
    assert r.nearest.tolist() == [3, 3, 3, 0, 0, 0, NONE, 7, 0, 3, 6, 7]
    assert r.w.view(np.float32).tolist()[:9] == [0.5, 0.25, 1.0, 0.5, 2.0, INF, INF, 2.0, 2.0]
    assert r.w.tolist()[9:] == [0x80000000] + bits_of([2.0, 3.0]).tolist()
    assert r.cluster.tolist() == [3, 3, 2, 4, 2, 0, 0, 1, 2, 3, 2, 1]
    assert r.labels.tolist() == [1, 1, -1, 2, -1, -1, -1, 0, -1, 1, -1, 0]
    assert r.prob.tolist() == [1.0, 1.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, f32((1 / 3.0) / 0.5)]
    assert r.score.tolist() == [0.0, 0.0, 0.75, 0.5, 0.875, 1.0, 1.0, 0.0, 0.875, 0.0, 0.875, f32((0.5 - 1 / 3.0) / 0.5)]
    assert predict_model(base, sel.selected, 0.0, None, core, pos, dist, counts, 2).score is None
    # core_k = 0: no core(q); row 8's slot 0 stays at 1 and row 11's slot 1 at 3 against core[10] = 4
    r0 = predict_model(base, sel.selected, 0.0, sel.death, core, pos, dist, counts, 0)
    assert r0.w.view(np.float32).tolist()[8] == 1.0 and r0.cluster.tolist()[8] == 2 and r0.nearest.tolist()[11] == 7
    # selected {1, 2} (the selection under eps = 1.5): a query that lands in 3 or 4, which lost, gets the label of 2
    base, sel = hand_case(eps=1.5)
    assert sel.selected.tolist() == [0, 1, 1, 0, 0]
    r = predict_model(base, sel.selected, 1.5, sel.death, core, pos, dist, counts, 2)
    assert r.cluster.tolist() == [3, 3, 2, 4, 2, 0, 0, 1, 2, 3, 2, 1]
    assert r.labels.tolist() == [1, 1, 1, 1, 1, -1, -1, 0, 1, 1, 1, 0]
    assert r.prob.tolist() == [1.0, 1.0, 1.0, 1.0, 0.5, 0.0, 0.0, 1.0, 0.5, 1.0, 0.5, f32((1 / 3.0) / 0.5)]
    # selected = {0}: mcs = 7, K = 1, maxlambda(0) = 1/2.  eps = 0: thr = 1/2; eps = 4: thr = 1/4
    base, sel = hand_case(7, allow_single_cluster=True)
    assert sel.selected.tolist() == [1] and base.max_lambda == [0.5]
    r = predict_model(base, sel.selected, 0.0, sel.death, core, pos, dist, counts, 2)
    assert r.cluster.tolist() == [0] * 12
    assert r.labels.tolist() == [0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, -1]
    assert r.prob.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0]
    r = predict_model(base, sel.selected, 4.0, sel.death, core, pos, dist, counts, 2)
    assert r.labels.tolist() == [0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0]
    assert r.prob.tolist()[11] == f32((1 / 3.0) / 0.5) and r.prob.tolist()[5] == 0.0


# ----------------------------------------------------------------------------------------------------- three blobs
def blobs_and_shell(seed=0):
    """the shape of tests/test_gpu_hdbscan.py's blobs_and_noise: three tight blobs of 60 points and 20 points on shells around them"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, 8), np.float32)
    centres[0, 0], centres[1, 1], centres[2, 2] = 20, 20, 20
    blobs = [c + rng.normal(0, 0.05, (60, 8)) for c in centres]
    dirs = rng.normal(0, 1, (20, 8))
    noise = centres[rng.integers(0, 3, 20)] + dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(1, 2, (20, 1))
    return np.ascontiguousarray(np.concatenate(blobs + [noise]), np.float32)


def blob_queries(X):
    """the three blob means, and a point 100 blob diameters away from everything"""
    means = [X[60 * i:60 * i + 60].mean(axis=0) for i in range(3)]
    diameter = max(float(np.linalg.norm(X[60 * i:60 * i + 60] - means[i], axis=1).max()) for i in range(3)) * 2
    far = np.zeros(8, np.float32)
    far[3] = 20 + 100 * diameter
    return np.ascontiguousarray(np.stack(means + [far]), np.float32)


def exact_rows(X, Q, k, exclude_self=False):
    """numpy's exact k-NN rows of Q among X by f64 Euclidean distance, rounded to f32: (pos, dist bits, counts)"""
    d = np.sqrt(((Q[:, None, :].astype(np.float64) - X[None, :, :].astype(np.float64)) ** 2).sum(-1))
    if exclude_self:
        np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(d, order, 1).astype(np.float32)
    return order.astype(np.uint32), np.ascontiguousarray(dist).view(np.uint32), np.full(len(Q), k, np.uint32)


def assert_blob_property(labels, prob, score, train_labels):
    """each blob mean gets its blob's training label with probability > 0; the far point gets -1, or a score above every mean's"""
    for i in range(3):
        blob = set(train_labels[60 * i:60 * i + 60].tolist()) - {-1}
        assert len(blob) == 1 and labels[i] == blob.pop() and prob[i] > 0, (i, labels, prob)
    assert labels[3] == -1 or score[3] > max(score[:3]), (labels, score)


def prim(w):
    """a minimum spanning tree of the complete graph under the symmetric weights w (n, n), Prim from vertex 0: (a, b, weight) in
    ascending weight"""
    n = len(w)
    inside, best, link = np.zeros(n, bool), w[0].copy(), np.zeros(n, np.int64)
    inside[0] = True
    edges = []
    for _ in range(n - 1):
        v = int(np.argmin(np.where(inside, np.inf, best)))
        edges.append((int(link[v]), v, best[v]))
        inside[v] = True
        closer = ~inside & (w[v] < best)
        best[closer], link[closer] = w[v][closer], v
    edges.sort(key=lambda e: e[2])
    return (np.array([e[0] for e in edges], np.uint32), np.array([e[1] for e in edges], np.uint32), np.array([e[2] for e in edges], np.float32))


def test_model_assigns_blob_means_to_their_blobs():
    X = blobs_and_shell()
    n, k, core_k, mcs = len(X), 10, 9, 10
    pos, dist, counts = exact_rows(X, X, k, exclude_self=True)
    core = dist[:, core_k - 1].copy()
    # the mutual-reachability minimum spanning tree of the complete graph, ascending
    d = np.sqrt(((X[:, None, :].astype(np.float64) - X[None, :, :].astype(np.float64)) ** 2).sum(-1)).astype(np.float32)
    cf = core.view(np.float32)
    base = hdbscan_model(n, *prim(np.maximum(d, np.maximum(cf[:, None], cf[None, :]))), mcs)
    sel = select_model(base)
    assert sel.L == 3
    Q = blob_queries(X)
    qpos, qdist, qcounts = exact_rows(X, Q, 2 * (core_k + 1))
    r = predict_model(base, sel.selected, 0.0, sel.death, core, qpos, qdist, qcounts, core_k)
    assert_blob_property(r.labels, r.prob, r.score, sel.labels)


# ----------------------------------------------------------------------------------------------------- the ABI
class PredictOuts:
    """out arrays of nq slots at their sentinels"""
    NAMES = ("labels", "prob", "score", "nearest", "w", "cluster")

    def __init__(self, nq):
        self.labels = np.full(nq, LABEL, np.int32)
        self.prob, self.score, self.nearest = np.full(nq, PROB, np.uint32), np.full(nq, SCORE, np.uint32), np.full(nq, NEAREST, np.uint32)
        self.w, self.cluster = np.full(nq, WEIGHT, np.uint32), np.full(nq, CLUSTER, np.uint32)

    def arrays(self):
        return {x: getattr(self, x) for x in self.NAMES}

    def untouched(self, start=0, names=NAMES):
        sent = dict(zip(self.NAMES, (LABEL, PROB, SCORE, NEAREST, WEIGHT, CLUSTER)))
        return all(bool((getattr(self, x)[start:] == sent[x]).all()) for x in names)


TREE_ORDER = ("core", "K", "parent", "birth", "pc", "pw", "sel", "eps", "death")


def tree_args(base, sel, core, eps=0.0, death=True):
    """the arguments of a call between n and the outputs, as a dict of arrays and scalars"""
    return {"core": np.ascontiguousarray(core, np.uint32), "K": base.K, "parent": np.ascontiguousarray(base.cluster_parent, np.uint32),
            "birth": np.ascontiguousarray(base.cluster_birth_w, np.uint32), "pc": np.ascontiguousarray(base.point_cluster, np.uint32),
            "pw": np.ascontiguousarray(base.point_w, np.uint32), "sel": np.ascontiguousarray(sel.selected, np.uint8), "eps": eps,
            "death": np.ascontiguousarray(sel.death, np.float64) if death else None}


def _arg(x):
    return _p(x) if isinstance(x, np.ndarray) or x is None else x


def test_header_declares_the_six_symbols(native):
    N = _N()
    protos = N.PREDICT_HEADER.prototypes
    assert sorted(protos) == sorted(ENTRIES) == sorted(N.PREDICT_SYMBOLS)
    assert not set(protos) & (set(N.SYMBOLS) | set(N.HDBSCAN_SYMBOLS) | set(N.SELECT_SYMBOLS))    # the other headers keep their sets
    for name, (res, args, _names, text) in protos.items():     # bound with the signature generated from the header's text
        fn = getattr(native.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), text
        assert res is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if " T hnswhdp_" in l} == set(protos)    # and nothing exported without a prototype
    pkg = os.path.join(os.path.dirname(native.LIB_PATH), "hnsw_mi355x_hdbscan_predict.h")     # the package's own copy is the tree's
    assert os.path.exists(pkg) and open(pkg).read() == open(N.PREDICT_HEADER_PATH).read()
    tree = ["cluster_parent", "cluster_birth_w", "point_cluster", "point_w", "selected"]
    outs = ["labels", "prob", "score", "nearest", "w", "cluster"]
    rows = ["nbr_pos", "nbr_dist", "counts"]
    assert protos["hnswhdp_core_distances"][2] == ["idx", "knbn", "ef", "core_k", "out_core"]
    assert protos["hnswhdp_core_distances_device"][2] == ["idx", "knbn", "ef", "core_k", "d_out_core", "stream"]
    assert protos["hnswhdp_assign"][2] == (["device", "nq", "knbn"] + rows + ["core_k", "n", "core", "K"] + tree
                                           + ["cluster_selection_epsilon", "cluster_death_lambda"] + ["out_" + x for x in outs])
    assert protos["hnswhdp_assign_device"][2] == (["device", "nq", "knbn"] + ["d_" + x for x in rows] + ["core_k", "n", "d_core", "K"]
                                                  + ["d_" + x for x in tree] + ["cluster_selection_epsilon", "d_cluster_death_lambda"]
                                                  + ["d_out_" + x for x in outs] + ["stream"])
    assert protos["hnswhdp_predict"][2] == (["idx", "queries", "nq", "d", "knbn", "ef", "core_k", "core", "K"] + tree
                                            + ["cluster_selection_epsilon", "cluster_death_lambda"] + ["out_" + x for x in outs])
    assert protos["hnswhdp_predict_device"][2] == (["idx", "d_queries", "nq", "d", "knbn", "ef", "core_k", "d_core", "K"] + ["d_" + x for x in tree]
                                                   + ["cluster_selection_epsilon", "d_cluster_death_lambda"] + ["d_out_" + x for x in outs]
                                                   + ["stream"])
    text = open(N.PREDICT_HEADER_PATH).read()
    assert '#include "hnsw_mi355x_hdbscan_select.h"' in text
    for word in ("min(core_k, counts[v]) - 1", "min(core_k, counts[q]) - 1", "a tie keeps the earlier one", "<< 32 | s", "UINT32_MAX",
                 "lambda_j <= lambda_q", ">= lambda_q", "thr =", "ascending index", "no FMA", "BEFORE ANY TRAVERSAL OR GATHER",
                 "neither fault nor loop", "needs no device", "bit for bit", "Deviations from the hdbscan package", "Out of scope",
                 "several host threads", "strictly smaller cluster index"):
        assert word in text, word
    assert hasattr(native.Hnsw, "core_distances") and hasattr(native.Hnsw, "hdbscan_predict") and hasattr(native, "hdbscan_assign")
    assert hasattr(native, "PredictResult")


def _assign_call(L, form, o, rows, t, nq=None, k=3, core_k=2, n=12, device=0, **kw):
    pos, dist, counts = rows
    a = {**t, "pos": pos, "dist": dist, "counts": counts, **o.arrays(), **kw}
    args = ([device, len(counts) if nq is None else nq, k, _p(a["pos"]), _p(a["dist"]), _p(a["counts"]), core_k, n]
            + [_arg(a[x]) for x in TREE_ORDER] + [_p(a[x]) for x in PredictOuts.NAMES])
    return L.hnswhdp_assign(*args) if form == "host" else L.hnswhdp_assign_device(*args, None)


def test_the_assign_forms_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    base, sel = hand_case()
    rows, o = hand_rows(), PredictOuts(12)
    good = tree_args(base, sel, bits_of(HAND_CORE))

    def refused(form, word, **kw):
        rc = _assign_call(L, form, o, rows, {**good, **{x: kw.pop(x) for x in list(kw) if x in TREE_ORDER}}, **kw)
        assert rc == N.ERR_ARG, (form, word, rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), word

    def changed(name, at, value, src=None):
        x = (good[name] if src is None else src).copy()
        x.reshape(-1)[at] = value
        return x
    for form in ("host", "device"):                            # what either form sees without reading an array
        for eps in (math.nan, -1.0, -math.inf, -1e-30):
            refused(form, "cluster_selection_epsilon", eps=eps)
        refused(form, "core_k", core_k=4)
        refused(form, "knbn must be > 0", k=0, core_k=0)
        refused(form, "2^31", n=1 << 31)
        refused(form, "2^31", K=1 << 31)
        refused(form, "2^31", nq=1 << 31)
        refused(form, "2^31", nq=1 << 30, k=3)
        refused(form, "K = 0", K=0)
        for name in ("pos", "dist", "counts"):
            refused(form, "null nbr_pos", **{name: None})
        for name in ("core", "pc", "pw"):
            refused(form, "null core", **{name: None})
        for name in ("parent", "birth", "sel"):
            refused(form, "null cluster_parent", **{name: None})
        refused(form, "null out_labels", labels=None)
        refused(form, "out_score without", death=None)
        refused(form, "cluster_selection_epsilon", eps=-1.0, core_k=9, parent=None)    # several at once: in the order of the list
    # the tree and the rows themselves: the host form reads them on the host (the device form's kernel needs a device)
    refused("host", "cluster_parent[0]", parent=changed("parent", 0, 0))
    refused("host", "not below c", parent=changed("parent", 3, 3))
    refused("host", "not below c", parent=changed("parent", 1, NONE))
    refused("host", "not below c", parent=np.array([NONE, 2, 1, 2, 2], np.uint32))    # a 2-cycle
    refused("host", "point_cluster", pc=changed("pc", 11, 5))
    refused("host", "counts[q]", counts=changed(None, 4, 4, rows[2]))
    refused("host", "nbr_pos", pos=changed(None, 0, 12, rows[0]))
    refused("host", "nbr_pos", pos=changed(None, 7 * 3 + 2, NONE, rows[0]))
    # an unused slot may hold anything
    if L.hnswgpu_device_count() == 0:
        rc = _assign_call(L, "host", o, rows, good, pos=changed(None, 1, NONE, rows[0]))
        assert rc == N.ERR_DEVICE and o.untouched()


def test_no_query_needs_no_device(native):
    N = _N()
    L = native.lib()
    base, sel = hand_case()
    o = PredictOuts(4)
    good = tree_args(base, sel, bits_of(HAND_CORE))
    none = (np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32))
    for form in ("host", "device"):
        assert _assign_call(L, form, o, none, good) == N.OK, N.last_error()
        assert _assign_call(L, form, o, none, good, k=0, core_k=0) == N.OK, N.last_error()
        assert _assign_call(L, form, o, none, {x: (None if isinstance(v, np.ndarray) else v) for x, v in good.items()}, labels=None) == N.OK
        assert o.untouched()
    got = native.hdbscan_assign(native.forest_hdbscan(0, [], [], [], 2), np.zeros(0, np.float32), np.zeros((0, 4), np.uint32), np.zeros((0, 4), np.float32),
                                np.zeros(0, np.uint32), 2)
    assert len(got.labels) == 0 and got.outlier_scores is None and len(got.nearest) == 0 and len(got.weights) == 0 and len(got.clusters) == 0


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    base, sel = hand_case()
    rows, o = hand_rows(), PredictOuts(12)
    good = tree_args(base, sel, bits_of(HAND_CORE))
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_hdbscan_predict.py checks more)
        assert _assign_call(L, "host", o, rows, good) == N.OK
        want = predict_model(base, sel.selected, 0.0, sel.death, good["core"], *rows, 2)
        assert o.labels.tolist() == want.labels.tolist() and o.cluster.tolist() == want.cluster.tolist()
        return
    for form in ("host", "device"):
        rc = _assign_call(L, form, o, rows, good)
        assert rc == N.ERR_DEVICE and N.last_error() and o.untouched(), form


def _tiny_index(native, n=5):
    h = native.Hnsw(8, 100, 16, 32, "DistL2")
    if n:
        h.insert_serial(np.arange(n * 4, dtype=np.float32).reshape(n, 4))
    return h


def test_index_forms_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    h = _tiny_index(native)
    core = np.full(5, PROB, np.uint32)
    for form in ("host", "device"):
        def cd(k, ef, core_k, out=core, idx=h.handle):
            a = (idx, k, ef, core_k, _p(out))
            return L.hnswhdp_core_distances(*a) if form == "host" else L.hnswhdp_core_distances_device(*a, None)
        for a, word in (((0, 0, 0), "knbn must be > 0"), ((3, 0, 4), "core_k = 4 is above knbn = 3"), ((1 << 30, 0, 0), "2^30"),
                        ((5000, 0, 0), "knbn above 4096"), ((3, 0, 0, None), "null out_core")):
            assert cd(*a) == N.ERR_ARG and word in N.last_error(), (form, a, N.last_error())
        assert cd(3, 0, 0, core, None) == N.ERR_ARG
        h.set_arithmetic("simd8")
        assert cd(3, 0, 1) == N.ERR_ARG and "SIMD8" in N.last_error()
        h.set_arithmetic("scalar")
        h.set_storage("f16")
        for ef in (0, 16):
            assert cd(3, ef, 1) == N.ERR_ARG and "F16" in N.last_error()
        h.set_storage("f32")
        assert (core == PROB).all()
    # the same words as the spanning forest's
    a, b, w, m = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros(1, np.uint64)
    for k, ef, core_k in ((0, 0, 0), (3, 0, 4)):
        assert L.hnswgpu_graph_spanning_forest(h.handle, k, ef, 0, core_k, _p(a), _p(b), _p(w), _p(m)) == N.ERR_ARG
        words = N.last_error()
        assert L.hnswhdp_core_distances(h.handle, k, ef, core_k, _p(core)) == N.ERR_ARG and N.last_error() == words
    # predict: a tree over the 5 points, K = 1
    tree = model_of_arrays([NONE], [INF_BITS], [5], [0.0], [0] * 5, bits_of([1.0] * 5))
    sel = Model()
    sel.selected, sel.death = np.zeros(1, np.uint8), np.array([1.0])
    good = tree_args(tree, sel, np.zeros(5, np.uint32))
    Q = np.zeros((3, 4), np.float32)
    o = PredictOuts(3)

    def predict(form, nq=3, d=4, k=2, ef=8, core_k=1, q=Q, idx=h.handle, **kw):
        a = {**good, **o.arrays(), **kw}
        args = [idx, _p(q), nq, d, k, ef, core_k] + [_arg(a[x]) for x in TREE_ORDER] + [_p(a[x]) for x in PredictOuts.NAMES]
        return L.hnswhdp_predict(*args) if form == "host" else L.hnswhdp_predict_device(*args, None)
    for form in ("host", "device"):
        for kw, word in ((dict(eps=math.nan), "cluster_selection_epsilon"), (dict(core_k=3), "core_k"), (dict(k=0, core_k=0), "knbn must be > 0"),
                         (dict(K=0), "K = 0"), (dict(nq=1 << 31), "2^31"), (dict(q=None), "null buffer"), (dict(core=None), "null core"),
                         (dict(sel=None), "null cluster_parent"), (dict(labels=None), "null out_labels"), (dict(death=None), "out_score without"),
                         (dict(ef=0, d=5), "dimension"), (dict(ef=0, k=5000, core_k=0), "knbn above 4096"), (dict(idx=None), "null argument")):
            assert predict(form, **kw) == N.ERR_ARG and word in N.last_error(), (form, kw, N.last_error())
            assert o.untouched()
        h.set_arithmetic("simd8")
        assert predict(form, ef=0) == N.ERR_ARG and "SIMD8" in N.last_error()
        h.set_arithmetic("scalar")
        h.set_storage("f16")
        for ef in (0, 8):
            assert predict(form, ef=ef) == N.ERR_ARG and "F16" in N.last_error() and o.untouched()
        h.set_storage("f32")
        assert predict(form, nq=0, q=None, labels=None) == N.OK
    assert predict("host", parent=np.array([0], np.uint32)) == N.ERR_ARG and "cluster_parent[0]" in N.last_error()
    assert predict("host", pc=np.array([0, 0, 1, 0, 0], np.uint32)) == N.ERR_ARG and "point_cluster" in N.last_error()
    assert o.untouched()
    if L.hnswgpu_device_count() == 0:
        assert predict("host") == N.ERR_DEVICE and o.untouched()
        assert predict("device") == N.ERR_DEVICE and "upload" in N.last_error() and o.untouched()
        assert L.hnswhdp_core_distances(h.handle, 3, 0, 1, _p(core)) == N.ERR_DEVICE
        assert L.hnswhdp_core_distances_device(h.handle, 3, 0, 1, _p(core), None) == N.ERR_DEVICE and "upload" in N.last_error()
        assert (core == PROB).all()


def test_an_empty_index_has_no_core_distance_and_needs_no_device(native):
    N = _N()
    L = native.lib()
    core = np.full(2, PROB, np.uint32)
    h = native.Hnsw(8, 10, 16, 32, "DistL2")
    assert len(h.core_distances(5, None, 3)) == 0 and h.core_distances(5, 16, 0).dtype == np.float32
    for bad in (dict(knbn=0), dict(knbn=3, core_k=4), dict(knbn=3, ef=0), dict(knbn=3, core_k=-1)):
        try:
            h.core_distances(**bad)
        except native.HnswError as e:
            assert e.code == N.ERR_ARG, bad
        else:
            raise AssertionError(bad)
    res = h.hdbscan(5, 5)
    assert res.knn_params == (5, None, 4)
    assert native.forest_hdbscan(0, [], [], [], 2).knn_params is None and res.select(allow_single_cluster=True).knn_params == (5, None, 4)
    h.parallel_insert(np.zeros((0, 8), np.float32))             # (a handle exists from the first insertion on)
    for form in ("host", "device"):
        a = (h.handle, 5, 0, 3, _p(core))
        assert (L.hnswhdp_core_distances(*a) if form == "host" else L.hnswhdp_core_distances_device(*a, None)) == N.OK, N.last_error()
        a = (h.handle, 5, 0, 6, None)                           # still refused
        assert (L.hnswhdp_core_distances(*a) if form == "host" else L.hnswhdp_core_distances_device(*a, None)) == N.ERR_ARG
    assert (core == PROB).all() and len(h.core_distances(5, None, 3)) == 0
