"""Connected components on the device (Hnsw.knn_graph_components -> hnswgpu_graph_components / _device, csr_components ->
hnswgpu_csr_components / _device, csrc/graph_components.hip).

The expected answers never come from the code under test.  For the CSR entries the model is `components`, a plain union-find, on the
same edge list.  For the index entries D is what the existing public calls return for every point (exact_knn_graph_flat /
knn_graph_flat with point_ids None), positions come from `position_table`, and `cut_and_join` (tests/test_graph_components_abi.py)
cuts D, joins it through `symmetrise` and labels it.  Every comparison is exact: the labels, the sizes, the count, and the slots
behind the count that must stay as they were."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import uniform
from test_graph_components_abi import components, csr_edges, cut_and_join
from test_gpu_symmetric_graph import Index, _uniform_index, hub_data, positive

pytestmark = pytest.mark.gpu
MODES = ("union", "mutual")
MODE_CODE = {"union": 0, "mutual": 1}
EFS = (None, 32)
LABEL, SIZE, COUNT = 0xA5A5A5A5, 0x5A5A5A5A, 0x7777


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _f32(x):
    return None if x is None else np.array([x], np.float32)


# ----------------------------------------------------------------------------------------------------- the CSR entries
def to_csr(n, edges):
    """edge (r, c) listed in row r, the rows' entries in the order given"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.argsort(e[:, 0], kind="stable")
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=offsets[1:])
    return offsets, np.ascontiguousarray(e[order, 1].astype(np.uint32)), order


def csr_host(native, n, offsets, cols, dists=None, cut=None):
    """the host entry itself on out arrays at their sentinels: (rc, labels, sizes, c)"""
    lab, sizes, c = np.full(max(n, 1), LABEL, np.uint32), np.full(max(n, 1), SIZE, np.uint32), np.full(1, COUNT, np.uint64)
    cutp = _f32(cut)
    rc = native.lib().hnswgpu_csr_components(0, n, _p(offsets), _p(cols), _p(dists), _p(cutp), _p(lab), _p(sizes), _p(c))
    return rc, lab, sizes, int(c[0])


def csr_device(native, n, offsets, cols, dists=None, cut=None, stream=None):
    """the device entry on tensors at their sentinels: (rc, labels, sizes, c)"""
    import torch
    d_offs = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
    d_cols = torch.from_numpy(cols.view(np.int32).copy() if len(cols) else np.zeros(1, np.int32)).cuda()
    d_dists = torch.from_numpy(np.ascontiguousarray(dists, np.float32)).cuda() if dists is not None and len(dists) else None
    if dists is not None and d_dists is None:
        d_dists = torch.zeros(1, dtype=torch.float32, device="cuda")
    lab = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    sizes = torch.full((max(n, 1),), -2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c = np.full(1, COUNT, np.uint64)
    cutp = _f32(cut)
    rc = native.lib().hnswgpu_csr_components_device(0, n, _ptr(d_offs), _ptr(d_cols), _ptr(d_dists), _p(cutp), _ptr(lab), _ptr(sizes), _p(c),
                                                    C.c_void_p(stream.cuda_stream) if stream is not None else None)
    return rc, lab.cpu().numpy().view(np.uint32), sizes.cpu().numpy().view(np.uint32), int(c[0])


def check_csr(native, n, offsets, cols, dists=None, cut=None, what=""):
    """host form (twice: the same bytes) and device form against the model; nothing written behind the count"""
    want_lab, want_sizes = components(n, csr_edges(offsets, cols, dists, cut))
    c = len(want_sizes)
    first = None
    for form in ("host", "host again", "device"):
        rc, lab, sizes, got_c = (csr_device if form == "device" else csr_host)(native, n, offsets, cols, dists, cut)
        assert rc == 0, (what, form, native._native.last_error())
        assert got_c == c, (what, form, got_c, c)
        assert np.array_equal(lab[:n], want_lab), (what, form, "labels", np.flatnonzero(lab[:n] != want_lab)[:4])
        assert np.array_equal(sizes[:c], want_sizes), (what, form, "sizes")
        assert (sizes[c:] == (SIZE if form != "device" else 0xFFFFFFFE)).all(), (what, form, "behind the count")
        if form == "host":
            first = lab.tobytes() + sizes.tobytes()
        elif form == "host again":
            assert lab.tobytes() + sizes.tobytes() == first, (what, "two calls differ")
    res = native.csr_components(offsets, cols, dists, cut)
    assert res.n_components == c and np.array_equal(res.labels, want_lab) and np.array_equal(res.sizes, want_sizes), (what, "python")
    return want_lab, want_sizes


def test_tiny_graphs(native):
    none = np.zeros(0, np.uint32)
    check_csr(native, 1, np.array([0, 0], np.uint64), none, what="one vertex")
    check_csr(native, 1, np.array([0, 1], np.uint64), np.array([0], np.uint32), what="one vertex, a self-loop")
    lab, sizes = check_csr(native, 2, np.array([0, 0, 0], np.uint64), none, what="two isolated")
    assert lab.tolist() == [0, 1] and sizes.tolist() == [1, 1]
    for offs, col in (([0, 1, 1], 1), ([0, 0, 1], 0)):          # the one edge named from either end
        lab, sizes = check_csr(native, 2, np.array(offs, np.uint64), np.array([col], np.uint32), what="two joined")
        assert lab.tolist() == [0, 0] and sizes.tolist() == [2]


def _numberings(n, seed):
    return {"in order": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "permuted": np.random.default_rng(seed).permutation(n)}


@pytest.mark.parametrize("length", [63, 64, 65, 257, 5000])
def test_a_path_named_from_one_end_only(native, length):
    """a deep chain, work that crosses wavefronts and workgroups, weak connectivity: every edge is listed in ONE row"""
    for name, v in _numberings(length, length).items():
        offsets, cols, _ = to_csr(length, np.stack([v[:-1], v[1:]], 1))
        lab, sizes = check_csr(native, length, offsets, cols, what=f"path {length} {name}")
        assert sizes.tolist() == [length] and not lab.any()


def test_a_star_is_a_hub_row(native):
    """70 000 leaves: the centre's row holds them all -- at position 0, at position n - 1, and named by the leaves instead"""
    n = 70001
    for centre in (0, n - 1):
        leaves = np.setdiff1d(np.arange(n), [centre])
        for name, e in (("hub row", np.stack([np.full(n - 1, centre), leaves], 1)), ("named by the leaves", np.stack([leaves, np.full(n - 1, centre)], 1))):
            offsets, cols, _ = to_csr(n, e)
            assert int(np.diff(offsets.astype(np.int64)).max()) == (n - 1 if name == "hub row" else 1)
            lab, sizes = check_csr(native, n, offsets, cols, what=f"star, centre {centre}, {name}")
            assert sizes.tolist() == [n]


def test_disjoint_triangles_interleaved(native):
    t = np.arange(3000)
    e = np.concatenate([np.stack([t, t + 3000], 1), np.stack([t + 3000, t + 6000], 1), np.stack([t + 6000, t], 1)])
    offsets, cols, _ = to_csr(9000, e)
    lab, sizes = check_csr(native, 9000, offsets, cols, what="triangles")
    assert sizes.tolist() == [3] * 3000 and np.array_equal(lab, np.tile(t, 3).astype(np.uint32))


def test_two_paths_joined_at_their_far_ends(native):
    a, b = np.arange(2000), np.arange(2000, 4000)
    e = np.concatenate([np.stack([a[:-1], a[1:]], 1), np.stack([b[1:], b[:-1]], 1), [[1999, 3999]]])
    offsets, cols, _ = to_csr(4000, e)
    lab, sizes = check_csr(native, 4000, offsets, cols, what="two paths")
    assert sizes.tolist() == [4000]
    offsets, cols, _ = to_csr(4000, e[:-1])                      # and without the joining edge
    lab, sizes = check_csr(native, 4000, offsets, cols, what="two paths apart")
    assert sizes.tolist() == [2000, 2000]


def test_a_grid_under_a_random_numbering(native):
    v = np.random.default_rng(64).permutation(64 * 64).reshape(64, 64)
    e = np.concatenate([np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], 1), np.stack([v[1:, :].ravel(), v[:-1, :].ravel()], 1)])
    offsets, cols, _ = to_csr(4096, e)
    lab, sizes = check_csr(native, 4096, offsets, cols, what="grid")
    assert sizes.tolist() == [4096]
    e = e[(e[:, 0] // 7 + e[:, 1]) % 3 != 0]                     # and with a third of the edges gone
    offsets, cols, _ = to_csr(4096, e)
    check_csr(native, 4096, offsets, cols, what="grid with holes")


@pytest.mark.parametrize("n,out", [(20000, 1), (3000, 2)])
def test_random_graphs(native, n, out):
    rng = np.random.default_rng(n)
    e = np.stack([np.repeat(np.arange(n), out), rng.integers(0, n, n * out)], 1)
    offsets, cols, _ = to_csr(n, e)
    lab, sizes = check_csr(native, n, offsets, cols, what=f"random {n} x {out}")
    assert 1 < len(sizes) < n or out == 2


def test_self_loops_repeats_and_empty_rows(native):
    n = 300
    rng = np.random.default_rng(5)
    e = np.stack([rng.integers(0, n // 3, 200) * 3, rng.integers(0, n, 200)], 1)          # rows 1, 2 mod 3 are empty
    e = np.concatenate([e, e[:50], e[:50], np.stack([np.arange(0, n, 3)] * 2, 1), [[n - 1, n - 1]] * 3])
    offsets, cols, _ = to_csr(n, e)
    assert (np.diff(offsets.astype(np.int64)) == 0).sum() >= n // 2
    base = components(n, [tuple(x) for x in np.unique(e[e[:, 0] != e[:, 1]], axis=0).tolist()])
    lab, sizes = check_csr(native, n, offsets, cols, what="loops, repeats, empty rows")
    assert np.array_equal(lab, base[0]) and np.array_equal(sizes, base[1])                # they change nothing


def test_the_cut_is_an_ordered_comparison_on_the_stored_bits(native):
    n = 2000
    rng = np.random.default_rng(9)
    e = np.stack([rng.integers(0, n, 3000), rng.integers(0, n, 3000)], 1)
    offsets, cols, order = to_csr(n, e)
    d = rng.random(3000, dtype=np.float32)
    d[::7], d[1::7], d[2::7], d[3::7] = np.nan, -0.0, np.inf, 0.0
    d = d[order]
    assert np.isnan(d).sum() > 400 and (np.signbit(d) & (d == 0)).sum() > 400
    seen = []
    for cut in (0.0, -0.0, 0.5, float("inf"), None):
        lab, sizes = check_csr(native, n, offsets, cols, d, cut, what=f"cut {cut}")
        seen.append(len(sizes))
    assert seen[0] == seen[1] > seen[2] > seen[3] > seen[4]      # -0 = +0; each wider cut joins more; NaN counts only without a cut
    lab, sizes = check_csr(native, n, offsets, cols, d, float("-inf"), what="cut -inf")
    assert len(sizes) == n
    check_csr(native, n, offsets, cols, None, None, what="no dists, no cut")


def test_an_invalid_graph_is_an_argument_error_never_a_fault(native):
    NN = native._native
    offs, cols = np.array([0, 2, 3, 3, 5], np.uint64), np.array([1, 2, 3, 0, 1], np.uint32)
    bad = {"offsets[0]": (np.array([1, 2, 3, 3, 5], np.uint64), cols),
           "descend": (np.array([0, 3, 2, 3, 5], np.uint64), cols),
           "descend ": (np.array([0, 2, 3, 6, 5], np.uint64), np.array([1, 2, 3, 0, 1, 1], np.uint32)),
           "not below n": (offs, np.array([1, 2, 4, 0, 1], np.uint32)),
           "not below n ": (offs, np.array([1, 2, 3, 0, 0xFFFFFFFF], np.uint32)),
           "2^32": (np.array([0, 0, 0, 0, 1 << 32], np.uint64), cols),
           "2^32 ": (np.array([0, 2, 3, 3, (1 << 64) - 1], np.uint64), cols)}
    for form in (csr_host, csr_device):
        for word, (o, c) in bad.items():
            rc, lab, sizes, count = form(native, 4, o, c)
            assert rc == NN.ERR_ARG and word.strip() in NN.last_error(), (form.__name__, word, rc, NN.last_error())
            assert count == COUNT and len(set(lab.tolist())) == 1 and len(set(sizes.tolist())) == 1 and lab[0] != 0, (word, "written")
        rc, lab, sizes, count = form(native, 4, offs, cols)       # the well-formed one, after all that
        assert rc == NN.OK and count == 1 and lab[:4].tolist() == [0] * 4 and sizes[0] == 4


def test_two_host_threads_call_at_once(native):
    jobs = {}
    for name, (n, out) in {"a": (20000, 1), "b": (3000, 2)}.items():
        rng = np.random.default_rng(n + 1)
        offsets, cols, _ = to_csr(n, np.stack([np.repeat(np.arange(n), out), rng.integers(0, n, n * out)], 1))
        jobs[name] = (offsets, cols, components(n, csr_edges(offsets, cols)))
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [native.csr_components(jobs[name][0], jobs[name][1]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name, (_, _, (lab, sizes)) in jobs.items():
        for got in out[name]:
            assert np.array_equal(got.labels, lab) and np.array_equal(got.sizes, sizes), name


# ----------------------------------------------------------------------------------------------------- the index entries
_WANT = {}


def want_of(ix, k, ef, mode, cut=None):
    """the model's (labels, sizes), computed once per case and shared"""
    key = (id(ix), k, ef, mode, None if cut is None else float(np.float32(cut)))
    if key not in _WANT:
        res, pos = ix.D(k, ef)
        _WANT[key] = (ix, cut_and_join(ix.n, res.counts, pos, res.dists, mode, cut))   # (ix is kept: an id is unique among LIVE objects only)
    return _WANT[key][1]


def check_index(ix, k, ef, mode, cut=None, what=""):
    lab, sizes = want_of(ix, k, ef, mode, cut)
    got = ix.h.knn_graph_components(k, ef, mode, cut)
    what = f"{what} n {ix.n} k {k} ef {ef} {mode} cut {cut}"
    assert got.n_components == len(sizes), (what, got.n_components, len(sizes))
    assert got.labels.dtype == np.uint32 and np.array_equal(got.labels, lab), (what, "labels", np.flatnonzero(got.labels != lab)[:4])
    assert got.sizes.dtype == np.uint32 and np.array_equal(got.sizes, sizes), (what, "sizes")
    return got


def check_all(ix, k, what="", efs=EFS, cut=None):
    for ef in efs:
        for mode in MODES:
            check_index(ix, k, ef, mode, cut, what)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_indexes(native, oracle, tmp_path, n):
    ix = Index(native, oracle, tmp_path, uniform(n, 8, 10 + n))
    for k in (1, 3):
        check_all(ix, k, "small")
    got = ix.h.knn_graph_components(3)
    assert got.n_components == 1 and got.sizes.tolist() == [n]    # k >= n - 1: the complete graph
    # the host entry itself: the sizes behind the count stay as they were
    lab, sizes, c = np.full(n, LABEL, np.uint32), np.full(n + 2, SIZE, np.uint32), np.full(1, COUNT, np.uint64)
    assert native.lib().hnswgpu_graph_components(ix.h.handle, 1, 0, 1, None, _p(lab), _p(sizes), _p(c)) == 0
    want = want_of(ix, 1, None, "mutual")
    assert c[0] == len(want[1]) and np.array_equal(lab, want[0]) and np.array_equal(sizes[:c[0]], want[1]) and (sizes[int(c[0]):] == SIZE).all()
    assert native.lib().hnswgpu_graph_components(ix.h.handle, 1, 0, 1, None, _p(lab), None, _p(c)) == 0             # out_sizes may be NULL
    assert np.array_equal(lab, want[0])


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_block_edges(native, oracle, tmp_path_factory, n):
    """k = 1 gives many components; one wavefront less one, one, one more; a block and a bit"""
    ix = _uniform_index(native, oracle, tmp_path_factory, n)
    for k in (1, 3):
        check_all(ix, k, "edges")
    assert len(want_of(ix, 1, None, "union")[1]) > 1


@pytest.mark.parametrize("k", [5, 16])
def test_many_blocks(native, oracle, tmp_path_factory, k):
    check_all(_uniform_index(native, oracle, tmp_path_factory, 3000), k, "3000")


def test_a_cut_at_the_median_stored_distance(native, oracle, tmp_path_factory):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    res, _ = ix.D(5, None)
    cut = float(np.median(res.dists[np.arange(5)[None, :] < res.counts[:, None]]))
    check_all(ix, 5, "median", cut=cut)
    with_cut, without = want_of(ix, 5, None, "union", cut), want_of(ix, 5, None, "union")
    assert len(with_cut[1]) > len(without[1])                   # (the cut does cut: on the model)
    for extreme in (float("inf"), 0.0):
        check_index(ix, 5, None, "union", extreme, "extreme")
    assert len(want_of(ix, 5, None, "union", 0.0)[1]) == ix.n


def test_separated_clusters_stay_apart(native, oracle, tmp_path):
    """40 tight clusters of 50 points (the data of the hub test without its hub; the centres are 0.4 apart at least, a cluster is
    0.006 wide): the 5 nearest of a point are in its cluster, so the exact D never leaves a cluster -- asserted on D.  The graph
    search at ef = 32 may miss a point's own cluster on this M = 8 graph and answer from another: its D is held to the model only,
    and to the clusters where it happens to stay inside them."""
    ix = Index(native, oracle, tmp_path, hub_data()[:2000])
    cluster = np.arange(2000) // 50                             # (ids are 0 .. n - 1: position = id)
    for ef in EFS:
        res, pos = ix.D(5, ef)
        inside = bool((cluster[pos] == cluster[:, None])[np.arange(5)[None, :] < res.counts[:, None]].all())
        assert inside or ef is not None                        # the precondition, on D
        for mode in MODES:
            got = check_index(ix, 5, ef, mode, None, "clusters")
            if not inside:
                continue
            assert got.n_components >= 40
            firsts = {}
            for lab, cl in zip(got.labels.tolist(), cluster.tolist()):
                assert firsts.setdefault(lab, cl) == cl, "a component spans two clusters"


@pytest.mark.parametrize("shared", [False, True])
def test_exact_copies_and_repeated_ids(native, oracle, tmp_path, shared):
    base = uniform(400, 8, 31)
    perm = np.random.default_rng(32).permutation(1200)
    X = np.ascontiguousarray(np.tile(base, (3, 1))[perm])
    ids = np.ascontiguousarray((np.arange(1200, dtype=np.uint64) % 400 if shared else np.arange(1200, dtype=np.uint64) * 2 + 1)[perm])
    ix = Index(native, oracle, tmp_path, X, ids)
    for k in (1, 5):
        check_all(ix, k, f"copies shared {shared}")
    got = check_index(ix, 2, None, "mutual", 0.0, "copies at distance 0")          # under a cut of 0 only the copies are joined
    assert got.n_components == 400 and got.sizes.tolist() == [3] * 400


def test_mutual_singletons_are_the_empty_mutual_rows(native, oracle, tmp_path_factory):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    for ef in EFS:
        got = check_index(ix, 5, ef, "mutual")
        rows = ix.h.symmetric_knn_graph_flat(5, ef, "mutual")
        alone = np.flatnonzero(got.sizes[got.labels] == 1)
        assert len(alone) > 0 and np.array_equal(alone, np.flatnonzero(rows.counts == 0))


def test_labels_equal_the_components_of_the_symmetrised_graph(native, oracle, tmp_path_factory):
    """hnswgpu_symmetric_graph_device's outputs, as they stand on the device, into hnswgpu_csr_components_device; under a cut too
    (DistL2 stores the same bits in both directions, so cutting the symmetrised UNION graph is cutting D)"""
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    res, _ = ix.D(5, None)
    median = float(np.median(res.dists[np.arange(5)[None, :] < res.counts[:, None]]))
    for ef in EFS:
        for mode in MODES:
            cap = 2 * ix.n * 5
            offs = torch.zeros(ix.n + 1, dtype=torch.int64, device="cuda")
            pos = torch.zeros(cap, dtype=torch.int32, device="cuda")
            dists = torch.zeros(cap, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rc = L.hnswgpu_symmetric_graph_device(ix.h.handle, 5, 0 if ef is None else ef, MODE_CODE[mode], cap, _ptr(offs), _ptr(pos), None, _ptr(dists),
                                                  None, None, None)
            assert rc == NN.OK, NN.last_error()
            for cut in (None, median):
                lab = torch.full((ix.n,), -1, dtype=torch.int32, device="cuda")
                sizes = torch.full((ix.n,), -2, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                c = np.zeros(1, np.uint64)
                cutp = _f32(cut)
                rc = L.hnswgpu_csr_components_device(0, ix.n, _ptr(offs), _ptr(pos), _ptr(dists), _p(cutp), _ptr(lab), _ptr(sizes), _p(c), None)
                assert rc == NN.OK, NN.last_error()
                got = ix.h.knn_graph_components(5, ef, mode, cut)
                assert got.n_components == int(c[0]) and np.array_equal(got.labels, lab.cpu().numpy().view(np.uint32)), (ef, mode, cut)
                assert np.array_equal(got.sizes, sizes.cpu().numpy().view(np.uint32)[:int(c[0])])
                want = want_of(ix, 5, ef, mode, cut)
                assert np.array_equal(got.labels, want[0]) and np.array_equal(got.sizes, want[1])


def test_a_cut_between_the_two_directions_of_a_pair(native, oracle, tmp_path):
    """DistJeffreys: d(i->j) and d(j->i) differ in their bits for some mutual pair of D; the cut at the smaller of the two keeps one
    direction and drops the other -- the pair is joined under UNION and not MUTUAL any more"""
    ix = Index(native, oracle, tmp_path, positive(300, 8, 0), metric="DistJeffreys")
    res, pos = ix.D(5, None)
    slot = {(i, int(pos[i, s])): res.dists[i, s] for i in range(ix.n) for s in range(int(res.counts[i]))}
    differing = sorted((i, j) for (i, j), d in slot.items() if (j, i) in slot and slot[(j, i)].view(np.uint32) != d.view(np.uint32))
    assert len(differing) >= 2, "the data must hold a pair whose two directions differ in their bits"     # on D
    i, j = differing[0]
    cut = float(min(slot[(i, j)], slot[(j, i)]))
    assert (slot[(i, j)] <= np.float32(cut)) != (slot[(j, i)] <= np.float32(cut))
    for mode in MODES:
        check_index(ix, 5, None, mode, cut, "Jeffreys")
        check_index(ix, 5, None, mode, None, "Jeffreys")
    check_index(ix, 5, 32, "mutual", cut, "Jeffreys")
    assert not np.array_equal(want_of(ix, 5, None, "union", cut)[0], want_of(ix, 5, None, "mutual", cut)[0])


def test_device_entry_on_a_stream(native, oracle, tmp_path_factory, tmp_path):
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    stream = torch.cuda.Stream()
    res, _ = ix.D(5, None)
    median = float(np.median(res.dists[np.arange(5)[None, :] < res.counts[:, None]]))
    for ef in EFS:
        for mode in MODES:
            for cut in (None, median):
                lab, sizes = want_of(ix, 5, ef, mode, cut)
                c = len(sizes)
                d_lab = torch.full((ix.n,), -1, dtype=torch.int32, device="cuda")
                d_sizes = torch.full((ix.n,), -2, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                count, cutp = np.full(1, COUNT, np.uint64), _f32(cut)
                rc = L.hnswgpu_graph_components_device(ix.h.handle, 5, 0 if ef is None else ef, MODE_CODE[mode], _p(cutp), _ptr(d_lab), _ptr(d_sizes),
                                                       _p(count), C.c_void_p(stream.cuda_stream))
                assert rc == NN.OK, NN.last_error()
                assert count[0] == c and np.array_equal(d_lab.cpu().numpy().view(np.uint32), lab), (ef, mode, cut)
                got = d_sizes.cpu().numpy()
                assert np.array_equal(got[:c].view(np.uint32), sizes) and (got[c:] == -2).all()
    count = np.full(1, COUNT, np.uint64)
    rc = L.hnswgpu_graph_components_device(ix.h.handle, 5, 0, 0, None, _ptr(d_lab), None, _p(count), None)           # out_sizes may be NULL
    assert rc == NN.OK and count[0] == len(want_of(ix, 5, None, "union")[1])
    cold = Index(native, oracle, tmp_path, uniform(65, 8, 65), upload=False)               # never uploaded
    d_lab = torch.full((65,), -1, dtype=torch.int32, device="cuda")
    count = np.full(1, COUNT, np.uint64)
    rc = L.hnswgpu_graph_components_device(cold.h.handle, 3, 0, 0, None, _ptr(d_lab), None, _p(count), None)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error()
    assert count[0] == COUNT and (d_lab == -1).all()


def test_the_same_call_gives_the_same_bytes(native, oracle, tmp_path_factory, knob):
    """twice in a row; and with D arriving in many chunks (HNSWGPU_GRAPH_CHUNK = 97: 31 chunks, the last partial)"""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)

    def both(ef, mode):
        got = ix.h.knn_graph_components(16, ef, mode)
        return got.labels.tobytes() + got.sizes.tobytes()
    for mode in MODES:
        first = {ef: both(ef, mode) for ef in EFS}
        for ef in EFS:
            assert both(ef, mode) == first[ef]
        knob("HNSWGPU_GRAPH_CHUNK", 97)
        try:
            for ef in EFS:
                assert both(ef, mode) == first[ef], (mode, ef, "chunks of 97")
        finally:
            knob("HNSWGPU_GRAPH_CHUNK", None)
        lab, sizes = want_of(ix, 16, None, mode)
        assert first[None] == lab.tobytes() + sizes.tobytes()
