"""DBSCAN on the device (hnswdbs_exact / _device, hnswdbs_csr / _device, csrc/dbscan.hip) as far as a box without a GPU can see it:
the ABI, every refusal that is answered before a device is needed, the calls that need none -- and section 1 of
include/hnsw_mi355x_dbscan.h restated sequentially over explicit sets: `dbscan_model`.  tests/test_gpu_dbscan.py imports it to build
its expected answers, never from the code under test.  Here the model is checked against an independent textbook DBSCAN (queue
expansion) on small symmetric inputs, and on three hand-made cases whose every output is written out.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

from test_hdbscan_predict_abi import order_of

ENTRIES = ("hnswdbs_exact", "hnswdbs_exact_device", "hnswdbs_csr", "hnswdbs_csr_device")
NONE = 0xFFFFFFFF
# sentinels of the out arrays
LABEL, CORE, COUNT, ANCHOR, CLUSTERS = -77, 0xA5, 0xABCD0001, 0xABCD0002, 0x7777


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
class DbscanAnswer:
    def __init__(self, labels, core, counts, anchors, n_clusters):
        self.labels, self.core, self.counts, self.anchors, self.n_clusters = labels, core, counts, anchors, n_clusters


def dbscan_model(N, min_samples, add_self=0):
    """Section 1 of include/hnsw_mi355x_dbscan.h, point by point.  N[i]: the set of vertex i as a sequence of (j, w), w an f32
    (repeated pairs count as they stand).  Returns a DbscanAnswer: labels i32, core u8, counts u32, anchors u32, n_clusters."""
    n = len(N)
    counts = [len(N[i]) + add_self for i in range(n)]
    core = [counts[i] >= min_samples for i in range(n)]
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    for i in range(n):
        for j, _ in N[i]:
            j = int(j)
            if core[i] and core[j]:                              # j in N(i): that is "j in N(i) or i in N(j)" over all i
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    number = {}
    for i in range(n):                                          # ascending: a cluster is met first at its smallest core position
        if core[i] and find(i) not in number:
            number[find(i)] = len(number)
    labels, anchors = [], []
    for i in range(n):
        if core[i]:
            labels.append(number[find(i)])
            anchors.append(i)
            continue
        keys = [(order_of(np.array(w, np.float32).view(np.uint32)[()]) << 32) | int(j) for j, w in N[i] if core[int(j)]]
        if not keys:
            labels.append(-1)
            anchors.append(NONE)
        else:
            a = min(keys) & 0xFFFFFFFF
            labels.append(number[find(a)])
            anchors.append(a)
    return DbscanAnswer(np.array(labels, np.int32).reshape(n), np.array(core, np.uint8).reshape(n), np.array(counts, np.uint32).reshape(n),
                        np.array(anchors, np.uint32).reshape(n), len(number))


def sets_of_matrix(D, eps):
    """N(i) = {(j, D[i, j]) : D[i, j] <= eps} as f32 values: a NaN on either side is no member, -0 equals +0"""
    D = np.asarray(D, np.float32)
    with np.errstate(invalid="ignore"):
        hit = D <= np.float32(eps)
    return [[(int(j), D[i, j]) for j in np.nonzero(hit[i])[0]] for i in range(D.shape[0])]


def sets_of_csr(offsets, cols, dists, eps):
    """section 3: entry e of row i is in N(i) iff dists is None or dists[e] <= eps; its w is dists[e], +0 without dists"""
    out = []
    for i in range(len(offsets) - 1):
        row = []
        for e in range(int(offsets[i]), int(offsets[i + 1])):
            w = np.float32(0.0) if dists is None else np.float32(dists[e])
            with np.errstate(invalid="ignore"):
                if dists is None or bool(w <= np.float32(eps)):
                    row.append((int(cols[e]), w))
        out.append(row)
    return out


def textbook_dbscan(region, n, min_samples):
    """Ester et al. 1996 by queue expansion over region(p) -> list of points (p included); labels with -1 for noise.  Independent
    of dbscan_model: no union-find, no keys."""
    UNDEF, NOISE = -2, -1
    labels, c = [UNDEF] * n, 0
    for p in range(n):
        if labels[p] != UNDEF:
            continue
        nb = region(p)
        if len(nb) < min_samples:
            labels[p] = NOISE
            continue
        labels[p] = c
        queue = list(nb)
        while queue:
            q = queue.pop(0)
            if labels[q] == NOISE:
                labels[q] = c
            if labels[q] != UNDEF:
                continue
            labels[q] = c
            nq = region(q)
            if len(nq) >= min_samples:
                queue.extend(nq)
        c += 1
    return labels


@pytest.mark.parametrize("seed", range(12))
def test_model_agrees_with_the_textbook_on_symmetric_inputs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 90))
    centres = rng.random((3, 2)) * 6
    X = np.concatenate([centres[rng.integers(0, 3, n - n // 4)] + rng.normal(0, 0.35, (n - n // 4, 2)), rng.random((n // 4, 2)) * 8]).astype(np.float32)
    D = np.abs(X[:, None, :] - X[None, :, :]).sum(-1, dtype=np.float32)
    D = np.maximum(D, D.T)                                      # symmetric, bit for bit
    eps, ms = np.float32((0.5, 0.8, 1.2)[seed % 3]), (2, 4, 6, 3)[seed % 4]
    sets = sets_of_matrix(D, eps)
    m = dbscan_model(sets, ms)
    t = textbook_dbscan(lambda p: [j for j, _ in sets[p]], n, ms)
    core = np.array([len(s) >= ms for s in sets])
    assert np.array_equal(m.core.astype(bool), core) and np.array_equal(m.counts, [len(s) for s in sets])
    pairs = {(int(m.labels[i]), t[i]) for i in range(n) if core[i]}                       # the same partition of the core points
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) == m.n_clusters
    for i in range(n):
        if core[i]:
            assert m.anchors[i] == i and m.labels[i] >= 0
            continue
        assert (m.labels[i] == -1) == (t[i] == -1), i                                    # the same noise
        near = {int(m.labels[j]) for j, _ in sets[i] if core[j]}
        if m.labels[i] == -1:
            assert not near and m.anchors[i] == NONE
        else:                                                                            # a border point: one of its core neighbours'
            assert int(m.labels[i]) in near and core[m.anchors[i]] and m.labels[m.anchors[i]] == m.labels[i]
            assert dict(pairs)[int(m.labels[i])] in {t[j] for j, _ in sets[i] if core[j]}
    firsts = [int(np.nonzero((m.labels == c) & core)[0][0]) for c in range(m.n_clusters)]
    assert firsts == sorted(firsts)                                                      # numbered by smallest core position


def _line(x, eps):
    x = np.asarray(x, np.float32)
    return sets_of_matrix(np.abs(x[:, None] - x[None, :]), eps)


def _same(m, labels, core, counts, anchors, c):
    assert m.labels.tolist() == labels and m.core.tolist() == core and m.counts.tolist() == counts and m.anchors.tolist() == anchors
    assert m.n_clusters == c and m.labels.dtype == np.int32 and m.core.dtype == np.uint8 and m.counts.dtype == m.anchors.dtype == np.uint32


def test_model_on_hand_made_cases():
    # 1. two triples and a lone point on a line, eps 1, min_samples 3: the middles are core, the ends border, the lone point noise
    _same(dbscan_model(_line([0, 1, 2, 10, 20, 21, 22], 1.0), 3), [0, 0, 0, -1, 1, 1, 1], [0, 1, 0, 0, 0, 1, 0], [2, 3, 2, 1, 2, 3, 2],
          [1, 1, 1, NONE, 5, 5, 5], 2)
    _same(dbscan_model(_line([0, 1, 2, 10, 20, 21, 22], np.nextafter(np.float32(1), np.float32(0))), 2), [-1] * 7, [0] * 7, [1] * 7, [NONE] * 7, 0)
    _same(dbscan_model(_line([0, 1, 2, 10, 20, 21, 22], 1.0), 1), [0, 0, 0, 1, 2, 2, 2], [1] * 7, [2, 3, 2, 1, 2, 3, 2], list(range(7)), 3)
    # 2. the point at 2 is at exactly eps = 2 from the only core point of either cluster (0 and 4, four points each within 2; it
    # has three itself): the tie goes to the smaller position -- x = 0's cluster in this order ...
    x = [-1.5, -1, 0, 2, 4, 5, 5.5]
    _same(dbscan_model(_line(x, 2.0), 4), [0, 0, 0, 0, 1, 1, 1], [0, 0, 1, 0, 1, 0, 0], [3, 3, 4, 3, 4, 3, 3], [2, 2, 2, 2, 4, 4, 4], 2)
    # ... and x = 4's cluster in the other: the arrays read the same, the point at 2 has changed sides
    r = dbscan_model(_line(x[::-1], 2.0), 4)
    _same(r, [0, 0, 0, 0, 1, 1, 1], [0, 0, 1, 0, 1, 0, 0], [3, 3, 4, 3, 4, 3, 3], [2, 2, 2, 2, 4, 4, 4], 2)
    assert x[::-1][r.anchors[3]] == 4 and x[2] == 0
    # 3. explicit directed sets, add_self 1, min_samples 4: repeated and self entries count; 4 sees -0 and +0 as one distance and
    # takes position 0; 2 names the core point 3, which names only itself: a cluster of its own with 2 on its border; 5 names only
    # 2, which is not core: noise, like the empty 6
    z = np.float32
    sets = [[(1, z(.5)), (1, z(.5)), (0, z(0))], [(0, z(.25)), (1, z(.1)), (1, z(.1))], [(3, z(1))], [(3, z(0)), (3, z(0)), (3, z(0))],
            [(1, z(-0.0)), (0, z(0.0))], [(2, z(.1))], []]
    _same(dbscan_model(sets, 4, 1), [0, 0, 1, 1, 0, -1, -1], [1, 1, 0, 1, 0, 0, 0], [4, 4, 2, 4, 3, 2, 1], [0, 1, 3, 3, 0, NONE, NONE], 2)
    offs, cols = [0, 3, 6, 7, 10, 12, 13, 13], [1, 1, 0, 0, 1, 1, 3, 3, 3, 3, 1, 0, 2]
    d = np.array([.5, .5, 0, .25, .1, .1, 1, 0, 0, 0, -0.0, 0.0, .1], np.float32)
    got = sets_of_csr(offs, cols, d, np.inf)
    assert [[(j, float(w)) for j, w in row] for row in got] == [[(j, float(w)) for j, w in row] for row in sets]
    assert [len(r) for r in sets_of_csr(offs, cols, d, 0.25)] == [1, 3, 0, 3, 2, 1, 0]
    assert [len(r) for r in sets_of_csr(offs, cols, None, -1.0)] == [3, 3, 1, 3, 2, 1, 0]         # without dists eps is not read
    assert dbscan_model([], 1).n_clusters == 0


# ----------------------------------------------------------------------------------------------------- the ABI
def _small(native, n=50, d=8, f16=False):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
    if f16:
        X = native.round_to_f16(X)
    h = native.Hnsw(8, n, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(X)
    return X, h


def test_header_declares_the_four_symbols(native):
    N = _N()
    protos = N.DBSCAN_HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.DBSCAN_SYMBOLS) == ENTRIES
    assert len(N.SYMBOLS) == 102                               # the first header keeps its set
    for name in ENTRIES:
        assert protos[name][0] is C.c_int and getattr(native.lib(), name) is not None
        assert name not in N.SYMBOLS and name not in N.PREDICT_SYMBOLS
    outs = ["out_label", "out_core", "out_count", "out_anchor"]
    assert protos[ENTRIES[0]][2] == ["idx", "eps", "min_samples", *outs, "out_n_clusters"]
    assert protos[ENTRIES[1]][2] == ["idx", "eps", "min_samples", *["d_" + x for x in outs], "out_n_clusters", "stream"]
    assert protos[ENTRIES[2]][2] == ["device", "n", "offsets", "cols", "dists", "eps", "min_samples", "add_self", *outs, "out_n_clusters"]
    assert protos[ENTRIES[3]][2] == ["device", "n", "d_offsets", "d_cols", "d_dists", "eps", "min_samples", "add_self", *["d_" + x for x in outs],
                                     "out_n_clusters", "stream"]
    assert protos[ENTRIES[0]][1][1] is C.c_float and protos[ENTRIES[0]][1][2] is C.c_uint64 and protos[ENTRIES[2]][1][7] is C.c_uint32
    text = open(N.DBSCAN_HEADER_PATH).read()
    for word in ("POSITIONS", "smallest core position", "dist_order_bits", "UINT32_MAX", "no out slot is touched", "2^31 - 1", "negative eps",
                 "no exclusion by identity", "DistJeffreys", "DIRECTED", "add_self", "hnswgpu_csr_components", "Out of scope", "OPTICS"):
        assert word in text, word
    assert hasattr(native.Hnsw, "dbscan") and callable(native.csr_dbscan)
    r = native.DbscanResult(np.zeros(2, np.int32), np.ones(2, bool), np.ones(2, np.uint32), np.arange(2, dtype=np.uint32), 1)
    assert r.n_clusters == 1 and r.labels.tolist() == [0, 0] and r.anchors.tolist() == [0, 1]


def test_package_copy_of_the_header_equals_the_tree(native):
    N = _N()
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_dbscan.h")
    assert N.DBSCAN_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_dbscan.h"), "rb").read() == open(tree, "rb").read()


class _Outs:
    """out arrays at their sentinels"""

    def __init__(self, n):
        n = max(n, 1)
        self.label, self.core = np.full(n, LABEL, np.int32), np.full(n, CORE, np.uint8)
        self.count, self.anchor, self.c = np.full(n, COUNT, np.uint32), np.full(n, ANCHOR, np.uint32), np.full(1, CLUSTERS, np.uint64)

    def arrays_untouched(self):
        return bool((self.label == LABEL).all() and (self.core == CORE).all() and (self.count == COUNT).all() and (self.anchor == ANCHOR).all())

    def untouched(self):
        return self.arrays_untouched() and self.c[0] == CLUSTERS


def test_exact_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    o = _Outs(50)

    def host(idx=h.handle, eps=0.5, ms=3, label=o.label, c=o.c):
        return L.hnswdbs_exact(idx, eps, ms, _p(label), _p(o.core), _p(o.count), _p(o.anchor), _p(c))

    def dev(idx=h.handle, eps=0.5, ms=3, label=o.label, c=o.c):
        return L.hnswdbs_exact_device(idx, eps, ms, _p(label), _p(o.core), _p(o.count), _p(o.anchor), _p(c), None)

    for call in (host, dev):
        def refused(word, **kw):
            rc = call(**kw)
            assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
            assert word in N.last_error(), (word, N.last_error())
            assert o.untouched(), kw.keys()
        refused("null", idx=None)
        refused("min_samples", ms=0)
        refused("NaN", eps=float("nan"))
        refused("out_label", label=None)
        refused("out_n_clusters", c=None)
        refused("min_samples", ms=0, eps=float("nan"))         # two faults at once: min_samples is looked at first
        h.set_arithmetic("simd8")
        try:
            refused("SIMD8")
        finally:
            h.set_arithmetic("scalar")
    Xh, hh = _small(native, f16=True)
    hh.set_storage("f16")
    for call in (host, dev):
        rc = call(idx=hh.handle)
        assert rc == N.ERR_ARG and "HNSWGPU_STORAGE_F16" in N.last_error() and "HNSWGPU_STORAGE_F32" in N.last_error(), N.last_error()
    assert o.untouched()
    for bad in (dict(eps=float("nan"), min_samples=3), dict(eps=1.0, min_samples=0)):
        with pytest.raises(native.HnswError) as err:           # the Python method hands the refusals on
            h.dbscan(**bad)
        assert err.value.code == N.ERR_ARG


def test_csr_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    offs, cols = np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32)
    dists = np.array([0.5, 0.25], np.float32)
    o = _Outs(3)

    def host(n=3, of=offs, co=cols, di=dists, eps=1.0, ms=2, add=0, label=o.label, c=o.c):
        return L.hnswdbs_csr(0, n, _p(of), _p(co), _p(di), eps, ms, add, _p(label), _p(o.core), _p(o.count), _p(o.anchor), _p(c))

    def dev(n=3, of=offs, co=cols, di=dists, eps=1.0, ms=2, add=0, label=o.label, c=o.c):
        return L.hnswdbs_csr_device(0, n, _p(of), _p(co), _p(di), eps, ms, add, _p(label), _p(o.core), _p(o.count), _p(o.anchor), _p(c), None)

    def refused(call, word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), kw.keys()
    for call in (host, dev):                                   # what either form sees without reading an array
        refused(call, "min_samples", ms=0)
        refused(call, "NaN", eps=float("nan"))
        refused(call, "NaN", eps=float("nan"), di=None)
        refused(call, "add_self", add=2)
        refused(call, "add_self", add=0xFFFFFFFF)
        refused(call, "out_label", label=None)
        refused(call, "out_n_clusters", c=None)
        refused(call, "2^31", n=1 << 31)
        refused(call, "2^31", n=(1 << 63) + 5)
        refused(call, "offsets", of=None)
        refused(call, "min_samples", ms=0, c=None)             # two faults at once
    # the graph itself, in hnswgpu_csr_components' words: the host form reads its arrays (the device form's validation kernels need
    # a device: tests/test_gpu_dbscan.py)
    refused(host, "offsets[0] is not 0", of=np.array([1, 1, 2, 2], np.uint64))
    refused(host, "the offsets descend", of=np.array([0, 2, 1, 2], np.uint64))
    refused(host, "is not below n", co=np.array([1, 3], np.uint32))
    refused(host, "is not below n", co=np.array([0xFFFFFFFF, 0], np.uint32))
    refused(host, "is 2^32 or more", of=np.array([0, 1, 2, 1 << 32], np.uint64))
    refused(host, "null cols with entries", co=None)
    refused(host, "offsets[0]", of=np.array([3, 2, 1, 0], np.uint64), co=np.array([9, 9], np.uint32))      # two faults at once
    ref = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(1, np.uint64)
    for bad, word in ((dict(of=np.array([1, 1, 2, 2], np.uint64)), "offsets[0] is not 0"), (dict(co=np.array([1, 3], np.uint32)), "is not below n")):
        kw = dict(of=offs, co=cols)
        kw.update(bad)
        assert L.hnswgpu_csr_components(0, 3, _p(kw["of"]), _p(kw["co"]), None, None, _p(ref[0]), _p(ref[1]), _p(ref[2])) == N.ERR_ARG
        theirs = N.last_error()
        refused(host, word, **bad)
        assert N.last_error() == theirs.replace("csr components", "csr dbscan")          # the same refusal in the same words
    # n == 0: no vertex, no cluster, nothing else written -- whatever the other pointers are
    for call in (host, dev):
        c = np.full(1, CLUSTERS, np.uint64)
        assert call(n=0, of=np.zeros(1, np.uint64), co=None, di=None, label=None, c=c) == N.OK and c[0] == 0
        assert o.arrays_untouched()
    for bad in (dict(offsets=[0, 1], cols=[0], min_samples=0), dict(offsets=[0, 1], cols=[0], dists=[1.0], eps=float("nan")),
                dict(offsets=[0, 1], cols=[1]), dict(offsets=[0, 2], cols=[0]), dict(offsets=[0, 1], cols=[0], dists=[1.0, 2.0])):
        with pytest.raises(native.HnswError) as err:           # the Python function hands the refusals on
            native.csr_dbscan(**bad)
        assert err.value.code == N.ERR_ARG
    got = native.csr_dbscan([0], [])
    assert got.n_clusters == 0 and len(got.labels) == 0 and got.labels.dtype == np.int32 and got.core.dtype == bool


def test_index_without_a_point_has_no_cluster_and_needs_no_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    res = e.dbscan(0.5, 3)                                      # no handle yet
    assert res.n_clusters == 0 and len(res.labels) == len(res.core) == len(res.counts) == len(res.anchors) == 0
    e.parallel_insert(np.zeros((0, 8), np.float32))            # (a handle exists from the first insertion on)
    assert e.handle
    o = _Outs(1)
    assert L.hnswdbs_exact(e.handle, 0.5, 3, None, None, None, None, _p(o.c)) == N.OK and o.c[0] == 0
    o.c[0] = CLUSTERS
    assert L.hnswdbs_exact_device(e.handle, 0.5, 3, None, None, None, None, _p(o.c), None) == N.OK and o.c[0] == 0
    assert o.arrays_untouched()
    assert L.hnswdbs_exact(e.handle, 0.5, 0, None, None, None, None, _p(o.c)) == N.ERR_ARG           # still refused
    assert e.dbscan(0.5, 3).n_clusters == 0


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    offs, cols = np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32)
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_dbscan.py checks the answers)
        assert h.dbscan(float("inf"), 1).labels.tolist() == [0] * 50
        assert native.csr_dbscan(offs, cols, add_self=True).labels.tolist() == [0, 0, 0]
        return
    with pytest.raises(native.HnswError) as e:
        h.dbscan(0.5, 3)
    assert e.value.code == N.ERR_DEVICE
    with pytest.raises(native.HnswError) as e:
        native.csr_dbscan(offs, cols)
    assert e.value.code == N.ERR_DEVICE
    o = _Outs(50)
    rc = L.hnswdbs_exact_device(h.handle, 0.5, 3, _p(o.label), _p(o.core), _p(o.count), _p(o.anchor), _p(o.c), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
    rc = L.hnswdbs_csr_device(0, 3, _p(offs), _p(cols), None, 0.5, 1, 0, _p(o.label), _p(o.core), _p(o.count), _p(o.anchor), _p(o.c), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
