"""The selection stage of HDBSCAN (hnswhds_select / _device, csrc/cluster_select.hip) as far as a box without a GPU can see it: the
ABI, every refusal -- the host form answers all of them before a device is needed --, the call that needs none, and the contract of
include/hnsw_mi355x_hdbscan_select.h restated in Python: `select_model`, rules 1 - 6 read one after the other over the fields of
`hdbscan_model` (tests/test_hdbscan_abi.py, imported).  tests/test_gpu_hdbscan_select.py imports it to build its expected answers,
never from the code under test.  Here the model is checked on the hand-made forests whose answers are written out, and, where
scikit-learn is installed, against sklearn's own tree_to_labels under every combination of the options.  CPU only."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_dendrogram_abi import dendrogram
from test_hdbscan_abi import EOM, HAND_A, HAND_B, HAND_W, LEAF, NONE, Model, blob_mst, hdbscan_model, lam_of, same_partition

ENTRIES = ("hnswhds_select", "hnswhds_select_device")
# sentinels of the out arrays
SEL, LABEL, PROB, SCORE, DEATH, COUNT = 0xF4, -77, 0x7FC00123, 0x7FC00321, 0x7FF8000000ABCDEF, 0x7777


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
def weight_value(bits):
    """a weight by value: a NaN counts as +inf (-0 equals +0 under a comparison as it is)"""
    w = float(np.array(bits, np.uint32).view(np.float32)[()])
    return math.inf if math.isnan(w) else w


def select_model(base, method="eom", allow_single_cluster=False, eps=0.0, max_cluster_size=0, stability=None):
    """Rules 1 - 6 of include/hnsw_mi355x_hdbscan_select.h over the condensed tree of `base` (an hdbscan_model), sequentially.
    stability: another set of stabilities than the tree's own.  Returns an object with selected (u8), labels (i32), prob (f32),
    score (f32), death (f64), L, and, for the tests' own conditions: root (stability[0], sub(0) as the exactly rounded sum, the number
    of children of 0) and nested (F held a cluster together with a proper ancestor)."""
    K, n = base.K, base.n
    parent, size = [int(x) for x in base.cluster_parent], [int(x) for x in base.cluster_size]
    stab = [float(x) for x in (base.stability if stability is None else stability)]
    birth = [weight_value(b) for b in base.cluster_birth_w]
    kids, maxlam = base.kids, base.max_lambda
    pc, lam_v = [int(c) for c in base.point_cluster], [lam_of(int(b)) for b in base.point_w]
    eps = float(np.float32(eps))

    def fits(c):
        return max_cluster_size == 0 or size[c] <= max_cluster_size
    # 1: the winners
    S, wins, sub0 = [0.0] * K, [False] * K, 0.0
    for c in range(K - 1, -1, -1):
        if c == 0:
            sub = sub0 = math.fsum(S[d] for d in kids[0])
        else:
            assert len(kids[c]) in (0, 2)
            sub = S[kids[c][0]] + S[kids[c][1]] if kids[c] else 0.0
        if method == "leaf":
            wins[c] = (not kids[c]) if c != 0 else (bool(allow_single_cluster) and K == 1)
        else:
            wins[c] = (c != 0 or bool(allow_single_cluster)) and stab[c] >= sub and fits(c)
        S[c] = stab[c] if wins[c] else sub
    # 2: E, the winners without a winning proper ancestor
    under = [False] * K
    for c in range(1, K):
        under[c] = wins[parent[c]] or under[parent[c]]
    E = [c for c in range(K) if wins[c] and not under[c]]
    # 3: epsilon
    F, nested = set(E), False
    if eps > 0 and E != [0]:
        F = set()
        for c in E:
            end = c
            if birth[c] < eps:
                cur = c
                while True:
                    p = parent[cur]
                    if p == 0:
                        end = 0 if allow_single_cluster else cur
                        break
                    if birth[p] > eps:
                        end = p
                        break
                    cur = p
            F.add(end)

    def ancestors(c):
        while c != 0:
            c = parent[c]
            yield c
    Eprime = [c for c in sorted(F) if not any(a in F for a in ancestors(c))]
    nested = len(Eprime) != len(F)
    # 4: numbering
    selected = [0] * K
    label_of = {}
    for c in Eprime:
        selected[c] = 1
        label_of[c] = len(label_of)
    # 5: labels and probabilities
    labels, prob = [-1] * n, [0.0] * n
    sel_of = [-1] * K
    for c in range(K):
        sel_of[c] = c if selected[c] else (sel_of[parent[c]] if c != 0 else -1)
    for v in range(n):
        if Eprime == [0]:
            thr = 1.0 / eps if eps > 0 else maxlam[0]
            q = 0 if lam_v[v] >= thr else -1
        else:
            q = sel_of[pc[v]]
        if q < 0:
            continue
        labels[v] = label_of[q]
        prob[v] = 1.0 if maxlam[q] == 0 or lam_v[v] >= maxlam[q] else lam_v[v] / maxlam[q]
    # 6: GLOSH
    death = list(maxlam)
    for c in range(K - 1, 0, -1):
        death[parent[c]] = max(death[parent[c]], death[c])
    score = [0.0] * n
    for v in range(n):
        d = death[pc[v]]
        if d == 0 or lam_v[v] >= d:
            score[v] = 0.0
        elif math.isinf(d):
            score[v] = 1.0
        else:
            score[v] = (d - lam_v[v]) / d
    r = Model()
    r.K, r.n, r.L = K, n, len(Eprime)
    r.selected, r.labels = np.array(selected, np.uint8), np.array(labels, np.int32)
    r.prob, r.score = np.array(prob, np.float64).astype(np.float32), np.array(score, np.float64).astype(np.float32)
    r.death = np.array(death, np.float64)
    r.root, r.nested, r.E, r.wins = (stab[0], sub0, len(kids[0])), nested, E, wins
    return r


def model_of_arrays(parent, birth_bits, size, stability, point_cluster, point_w_bits):
    """a condensed tree given by its six arrays (what an hnswhdb_* call wrote) as select_model reads one: kids and max_lambda are
    worked out here, by the header's definitions"""
    r = Model()
    r.K, r.n = len(parent), len(point_cluster)
    r.cluster_parent, r.cluster_birth_w, r.cluster_size = np.asarray(parent, np.uint32), np.asarray(birth_bits, np.uint32), np.asarray(size, np.uint32)
    r.stability, r.point_cluster, r.point_w = np.asarray(stability, np.float64), np.asarray(point_cluster, np.uint32), np.asarray(point_w_bits, np.uint32)
    r.kids, r.max_lambda = [[] for _ in range(r.K)], [0.0] * r.K
    for c in range(1, r.K):
        p = int(r.cluster_parent[c])
        r.kids[p].append(c)
        r.max_lambda[p] = max(r.max_lambda[p], lam_of(int(r.cluster_birth_w[c])))
    for v in range(r.n):
        c = int(r.point_cluster[v])
        r.max_lambda[c] = max(r.max_lambda[c], lam_of(int(r.point_w[v])))
    return r


def root_has_margin(model):
    """cluster 0's decision is further from a tie than the device's order of summation can move sub(0)"""
    own, sub, children = model.root
    return own == sub == 0 or abs(own - sub) > 4 * children * 2.0 ** -53 * max(own, sub)


def _selected(r):
    return np.flatnonzero(r.selected).tolist()


def test_model_on_the_hand_made_forests():
    """the forest of tests/test_hdbscan_abi.py at mcs = 3: K = 5, cluster 1 = {7 .. 10} and cluster 2 = {0 .. 6} under 0, clusters
    3 = {3, 4, 5} and 4 = {0, 1, 2} under 2, born at weight 1; stabilities [0, 1.75, 6.5, 3, 9]"""
    base = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3)
    default = [2, 2, 2, 1, 1, 1, -1, 0, 0, 0, 0, -1]
    for method in ("eom", "leaf"):                              # the defaults: the first stage's own answer
        own, r = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3, method), select_model(base, method)
        assert r.selected.tolist() == own.selected.tolist() and r.labels.tolist() == own.labels.tolist() and r.L == own.L
        assert r.prob.tobytes() == own.prob.tobytes()
    r = select_model(base)
    assert _selected(r) == [1, 3, 4] and r.labels.tolist() == default
    r = select_model(base, eps=1.5)                             # 3 and 4, born at 1 < 1.5, climb to 2, a child of 0: they end there
    assert _selected(r) == [1, 2] and r.labels.tolist() == [1] * 7 + [0] * 4 + [-1] and not r.nested
    r = select_model(base, eps=1.0)                             # equal to the births of 3 and 4: strict <, nothing moves
    assert _selected(r) == [1, 3, 4] and r.labels.tolist() == default
    r = select_model(base, max_cluster_size=3)                  # cluster 1 holds four
    assert _selected(r) == [3, 4] and r.labels.tolist() == [1, 1, 1, 0, 0, 0] + [-1] * 6
    r = select_model(base, max_cluster_size=2)
    assert _selected(r) == [] and r.labels.tolist() == [-1] * 12 and r.L == 0
    r = select_model(base, allow_single_cluster=True)           # stability[0] = 0 loses against 1.75 + 12
    assert _selected(r) == [1, 3, 4] and r.labels.tolist() == default and r.root == (0.0, 13.75, 2)
    assert r.death.tolist() == [4.0, 0.5, 4.0, 2.0, 4.0]
    assert r.score.tolist() == [0, 0, 0, 0, 0, 0, 0.875, 0, 0, 0, 0.5, 1.0]
    for kw in (dict(eps=1.5), dict(max_cluster_size=2), dict(method="leaf"), dict(allow_single_cluster=True, eps=7.0)):
        other = select_model(base, **kw)                        # death and the scores do not depend on the options
        assert other.death.tolist() == r.death.tolist() and other.score.tobytes() == r.score.tobytes()
    r = select_model(base, stability=[14.0, 1.75, 6.5, 3.0, 9.0], allow_single_cluster=True)    # a made-up stability[0] that wins
    assert _selected(r) == [0] and r.L == 1                     # maxlambda(0) = 0: every vertex at lambda >= 0
    assert r.labels.tolist() == [0] * 12 and r.prob.tolist() == [1.0] * 12
    r = select_model(base, allow_single_cluster=True, eps=math.inf)    # every climb ends at 0; thr = 1 / inf = 0
    assert _selected(r) == [0] and r.labels.tolist() == [0] * 12
    r = select_model(base, allow_single_cluster=True, eps=1.5)  # 3 and 4 end at 2, born at +inf > 1.5: cluster 0 is not reached
    assert _selected(r) == [1, 2] and r.labels.tolist() == [1] * 7 + [0] * 4 + [-1]
    # the second weights: cluster 2 wins at the defaults
    w = [.5, .5, .5, .5, 1, 8, 8, 8, 8]
    base = hdbscan_model(12, HAND_A, HAND_B, w, 3)
    assert _selected(select_model(base)) == [1, 2]
    assert _selected(select_model(base, max_cluster_size=6)) == [1, 3, 4]
    assert _selected(select_model(base, max_cluster_size=3)) == [3, 4]
    # mcs = 7: K = 1
    base = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 7)
    assert base.K == 1 and base.max_lambda == [0.5]
    assert _selected(select_model(base)) == [] and _selected(select_model(base, "leaf")) == []
    want = [0] * 7 + [-1] * 5                                   # lambda = 0.5 >= maxlambda(0) = 0.5
    for kw in (dict(), dict(eps=2.0), dict(eps=4.0), dict(method="leaf"), dict(method="leaf", eps=2.0)):    # thr 0.5, 0.5, 0.25
        r = select_model(base, allow_single_cluster=True, **kw)
        assert _selected(r) == [0] and r.labels.tolist() == want and r.L == 1, kw
    r = select_model(base, allow_single_cluster=True, max_cluster_size=11)    # cluster 0 holds twelve
    assert _selected(r) == [] and r.labels.tolist() == [-1] * 12
    assert _selected(select_model(base, "leaf", allow_single_cluster=True, max_cluster_size=11)) == [0]    # leaf ignores the size


# ----------------------------------------------------------------------------------------------------- against scikit-learn
def _sklearn_cases():
    """150 seeded trees; per tree both methods, allow_single_cluster off and on, four eps, three max_cluster_size"""
    rng = np.random.default_rng(7)
    for trial in range(150):
        got = blob_mst(rng, int(rng.integers(2, 200)), int(rng.integers(1, 7)))
        mcs = int(rng.integers(2, 12))
        if got is None:
            continue
        yield (trial, mcs) + got


@pytest.mark.filterwarnings("ignore::DeprecationWarning")      # (numpy's, raised inside scikit-learn's own code)
def test_model_gives_sklearns_partition_under_every_option():
    tree = pytest.importorskip("sklearn.cluster._hdbscan._tree")
    pytest.importorskip("scipy.sparse.csgraph")
    kept, skipped, crashed = {}, 0, 0
    for trial, mcs, n, a, b, w in _sklearn_cases():
        left, right, size = dendrogram(n, list(zip(a.tolist(), b.tolist())))
        H = np.zeros(n - 1, dtype=tree.HIERARCHY_dtype)
        H["left_node"], H["right_node"], H["value"], H["cluster_size"] = left, right, w.astype(np.float64), size
        base = hdbscan_model(n, a, b, w, mcs)
        # eps is kept away from every weight
        epss = (0.0, float(np.median(w)) * 1.0001, float(np.quantile(w, 0.9)) * 1.0001, 2.0 * float(w.max()))
        for method in ("eom", "leaf"):
            for allow in (False, True):
                for eps in epss:
                    for max_size in (None, max(mcs, n // 3), n // 2 + 1):
                        mine = select_model(base, method, allow, eps, max_size or 0)
                        # the stated deviations: cluster 0's size, n here and the sum of its child clusters' sizes there, where
                        # max_cluster_size tells the two apart under allow_single_cluster; leaf with allow_single_cluster and K == 1
                        theirs_0 = int(sum(base.cluster_size[d] for d in base.kids[0]))
                        deviates = ((method == "eom" and allow and max_size is not None and (n <= max_size) != (theirs_0 <= max_size))
                                    or (method == "leaf" and allow and base.K == 1))
                        if n < mcs or deviates or mine.nested:
                            skipped += 1
                            continue
                        try:
                            theirs = tree.tree_to_labels(H, mcs, method, allow, eps, max_size)[0]
                        except KeyError:                        # sklearn's own, in _do_labelling: a single non-root cluster
                            assert allow
                            crashed += 1
                            continue
                        assert same_partition(mine.labels, theirs), (trial, n, mcs, method, allow, eps, max_size)
                        key = (method, allow, eps > 0, max_size is not None)
                        kept[key] = kept.get(key, 0) + 1
    print(f"[sklearn] compared {sum(kept.values())}, skipped {skipped}, sklearn KeyError {crashed}, least per combination {min(kept.values())}")
    assert len(kept) == 16 and min(kept.values()) >= 100, kept


# ----------------------------------------------------------------------------------------------------- the ABI
class SelectOuts:
    """out arrays at their sentinels: n vertices, `slots` clusters"""

    def __init__(self, n, slots):
        self.sel, self.labels = np.full(slots, SEL, np.uint8), np.full(n, LABEL, np.int32)
        self.prob, self.score = np.full(n, PROB, np.uint32), np.full(n, SCORE, np.uint32)
        self.death, self.l = np.full(slots, DEATH, np.uint64), np.full(1, COUNT, np.uint64)

    def arrays(self):
        return {"sel": self.sel, "labels": self.labels, "prob": self.prob, "score": self.score, "death": self.death, "n_labels": self.l}

    def untouched(self, vertices_from=0, clusters_from=0):
        v, c = vertices_from, clusters_from
        return bool((self.sel[c:] == SEL).all() and (self.labels[v:] == LABEL).all() and (self.prob[v:] == PROB).all()
                    and (self.score[v:] == SCORE).all() and (self.death[c:] == DEATH).all() and (v or c or self.l[0] == COUNT))


OUT_ORDER = ("sel", "labels", "prob", "score", "death", "n_labels")
IN_ORDER = ("parent", "birth", "size", "stab", "pc", "pw")


def tree_arrays(base, stability=None):
    """the six input arrays of a call, from a model"""
    return {"parent": np.ascontiguousarray(base.cluster_parent, np.uint32), "birth": np.ascontiguousarray(base.cluster_birth_w, np.uint32),
            "size": np.ascontiguousarray(base.cluster_size, np.uint32),
            "stab": np.ascontiguousarray(base.stability if stability is None else stability, np.float64),
            "pc": np.ascontiguousarray(base.point_cluster, np.uint32), "pw": np.ascontiguousarray(base.point_w, np.uint32)}


def test_header_declares_the_two_symbols(native):
    N = _N()
    protos = N.SELECT_HEADER.prototypes
    assert sorted(protos) == sorted(ENTRIES) == sorted(N.SELECT_SYMBOLS)
    assert not set(protos) & (set(N.SYMBOLS) | set(N.HDBSCAN_SYMBOLS))    # the two other headers keep their sets as they are
    for name, (res, args, _names, text) in protos.items():     # bound with the signature generated from the header's text
        fn = getattr(native.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), text
        assert res is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if " T hnswhds_" in l} == set(protos)    # and nothing exported without a prototype
    pkg = os.path.join(os.path.dirname(native.LIB_PATH), "hnsw_mi355x_hdbscan_select.h")      # the package's own copy is the tree's
    assert os.path.exists(pkg) and open(pkg).read() == open(N.SELECT_HEADER_PATH).read()
    ins = ["cluster_parent", "cluster_birth_w", "cluster_size", "stability", "point_cluster", "point_w"]
    opts = ["method", "allow_single_cluster", "cluster_selection_epsilon", "max_cluster_size"]
    outs = ["selected", "labels", "prob", "outlier_score", "cluster_death_lambda"]
    assert protos[ENTRIES[0]][2] == ["device", "n", "K"] + ins + opts + ["out_" + x for x in outs] + ["out_n_labels"]
    assert protos[ENTRIES[1]][2] == ["device", "n", "K"] + ["d_" + x for x in ins] + opts + ["d_out_" + x for x in outs] + ["out_n_labels", "stream"]
    assert protos[ENTRIES[0]][1][11] is C.c_float and protos[ENTRIES[0]][1][12] is C.c_uint64
    text = open(N.SELECT_HEADER_PATH).read()
    assert '#include "hnsw_mi355x_hdbscan.h"' in text
    for word in ("CANDIDATE", "WINS", "t modulo 256", "the same bytes", "children 2^-53", "proper ancestor", "birth_w(c) < eps", "birth_w(p) > eps",
                 "-0 too", "ascending cluster index", "thr = 1.0 / (double)eps", "whatever its point_cluster", "death(c)", "no FMA",
                 "BEFORE ANY TRAVERSAL", "neither fault nor loop", "needs no device", "byte for byte", "Deviations from scikit-learn",
                 "antichain", "Out of scope", "several host threads"):
        assert word in text, word
    assert hasattr(native.HdbscanResult, "select")


def test_the_host_form_answers_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    base = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3)
    good = tree_arrays(base)
    o = SelectOuts(12, 5)

    def args(n, K, method, allow, eps, max_size, kw):
        arrays = {**good, **o.arrays(), **kw}
        return [0, n, K] + [_p(arrays[x]) for x in IN_ORDER] + [method, allow, eps, max_size] + [_p(arrays[x]) for x in OUT_ORDER]

    def host(n=12, K=5, method=EOM, allow=0, eps=0.0, max_size=0, **kw):
        return L.hnswhds_select(*args(n, K, method, allow, eps, max_size, kw))

    def dev(n=12, K=5, method=EOM, allow=0, eps=0.0, max_size=0, **kw):
        return L.hnswhds_select_device(*args(n, K, method, allow, eps, max_size, kw), None)

    def refused(call, word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (call.__name__, kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), kw.keys()

    def changed(name, at, value):
        x = good[name].copy()
        x[at] = value
        return {name: x}
    for call in (host, dev):                                   # what either form sees without reading an array
        for method in (2, 7, 0xFFFFFFFF):
            refused(call, "unknown method", method=method)
        for allow in (2, 0xFFFFFFFF):
            refused(call, "allow_single_cluster", allow=allow)
        for eps in (math.nan, -1.0, -math.inf, -1e-30):
            refused(call, "cluster_selection_epsilon", eps=eps)
        refused(call, "2^31", n=1 << 31)
        refused(call, "2^31", K=1 << 31)
        refused(call, "2^31", K=1 << 40)
        refused(call, "K = 0", K=0)
        for name in IN_ORDER[:4]:
            refused(call, "null cluster_parent", **{name: None})
        for name in IN_ORDER[4:]:
            refused(call, "null point_cluster", **{name: None})
        refused(call, "null out_labels", labels=None)
        refused(call, "null out_n_labels", n_labels=None)
        refused(call, "unknown method", method=5, allow=3, parent=None)    # several at once: in the order of the list
    # the tree itself: the host form reads its arrays on the host (the device form's kernels need a device)
    refused(host, "cluster_parent[0]", **changed("parent", 0, 0))
    refused(host, "not below c", **changed("parent", 3, 3))
    refused(host, "not below c", **changed("parent", 1, NONE))
    refused(host, "not below c", **changed("parent", 2, 4))
    refused(host, "one child", **changed("parent", 4, 0))      # cluster 2 keeps one child
    six = {"parent": np.array([NONE, 0, 0, 2, 2, 2], np.uint32), "birth": np.zeros(6, np.uint32), "size": np.ones(6, np.uint32),
           "stab": np.zeros(6, np.float64)}
    refused(host, "more than two", K=6, **six)                 # cluster 2 has three
    refused(host, "point_cluster", **changed("pc", 11, 5))
    refused(host, "point_cluster", **changed("pc", 0, NONE))
    refused(host, "stability", **changed("stab", 2, math.nan))
    refused(host, "stability", **changed("stab", 0, -1.0))
    refused(host, "stability", **changed("stab", 4, -math.inf))
    with pytest.raises(native.HnswError) as err:               # the Python method hands the refusals on
        native.forest_hdbscan(0, [], [], [], 2).select(cluster_selection_epsilon=-1.0)
    assert err.value.code == N.ERR_ARG
    res = native.HdbscanResult(base.labels, base.prob, base.point_cluster, base.point_w.view(np.float32), base.cluster_parent,
                               base.cluster_birth_w.view(np.float32), base.cluster_size, base.stability, base.selected.astype(bool), base.K, base.L)
    assert res.outlier_scores is None and res.cluster_death_lambda is None
    for bad in (dict(method="best"), dict(cluster_selection_epsilon=math.nan), dict(max_cluster_size=0), dict(max_cluster_size=2.5)):
        with pytest.raises(native.HnswError) as err:
            res.select(**bad)
        assert err.value.code == N.ERR_ARG, bad


def test_no_vertex_needs_no_device(native):
    N = _N()
    L = native.lib()
    o = SelectOuts(4, 3)
    for form in ("host", "device"):
        for K in (0, 5):
            o.l[0] = COUNT
            a = [0, 0, K] + [None] * 6 + [LEAF, 1, 2.5, 7] + [None] * 5 + [_p(o.l)]
            rc = L.hnswhds_select(*a) if form == "host" else L.hnswhds_select_device(*a, None)
            assert rc == N.OK and o.l[0] == 0, (form, K, N.last_error())
            o.l[0] = COUNT
            assert o.untouched()
    got = native.forest_hdbscan(0, [], [], [], 2).select(allow_single_cluster=True)
    assert got.n_labels == 0 and len(got.labels) == 0 and len(got.outlier_scores) == 0 and len(got.cluster_death_lambda) == 0


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    base = hdbscan_model(12, HAND_A, HAND_B, HAND_W, 3)
    t, o = tree_arrays(base), SelectOuts(12, 5)
    a = [0, 12, 5] + [_p(t[x]) for x in IN_ORDER] + [EOM, 1, 1.5, 0] + [_p(o.arrays()[x]) for x in OUT_ORDER]
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_hdbscan_select.py checks more)
        assert L.hnswhds_select(*a) == N.OK
        want = select_model(base, "eom", True, 1.5)
        assert o.labels.tolist() == want.labels.tolist() and o.sel.tolist() == want.selected.tolist() and o.l[0] == want.L
        return
    for form in ("host", "device"):
        rc = L.hnswhds_select(*a) if form == "host" else L.hnswhds_select_device(*a, None)
        assert rc == N.ERR_DEVICE and N.last_error() and o.untouched(), form


def test_the_default_path_makes_no_call_of_the_selection_stage(native, monkeypatch):
    """the options at their defaults leave today's path: nothing of hnswhds_* is called; any other value calls select"""
    import hnsw_rs_amd.api as api
    calls = []
    real = api.HdbscanResult.select
    monkeypatch.setattr(api.HdbscanResult, "select", lambda self, *a, **kw: calls.append((a, kw)) or real(self, *a, **kw))
    got = native.forest_hdbscan(0, [], [], [], 2)
    assert calls == [] and got.outlier_scores is None and got.cluster_death_lambda is None
    native.SpanningForestResult(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, 0).hdbscan(2)
    native.Hnsw(8, 10, 16, 32, "DistL2").hdbscan(5, 5)
    native.forest_hdbscan(0, [], [], [], 2, cluster_selection_epsilon=-0.0)
    assert calls == []
    for kw in (dict(allow_single_cluster=True), dict(cluster_selection_epsilon=0.5), dict(max_cluster_size=4), dict(outlier_scores=True)):
        calls.clear()
        got = native.forest_hdbscan(0, [], [], [], 2, **kw)
        assert len(calls) == 1 and got.outlier_scores is not None, kw
        calls.clear()
        native.Hnsw(8, 10, 16, 32, "DistL2").hdbscan(5, 5, **kw)
        assert len(calls) == 1, kw
