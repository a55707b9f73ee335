"""No kernel may read scratch memory that its own call has not written.

Every device entry works in scratch whose contents on entry nobody defines: the pooled search workspaces, the exact unit's pooled
block, the call-scoped allocations of the graph units, the builder backend's buffers.  HNSWGPU_POISON_SCRATCH=<byte> (test hook,
host code only: csrc/hip_host.hpp) fills every such block with that byte where it passes from nobody's to a call's.  This file
computes nothing new: every case runs a comparison the suite already has -- the oracle, the f64 reference, the models -- with the
knob unset and then at one of three bytes, and asserts besides

  * that the answer's bytes equal those of the same call with the knob unset, and
  * that the "[hnswgpu poison]" line of HNSWGPU_TRACE_LAUNCH reports more than 0 bytes filled with that byte: the hook ran.

0xFF is the u32 "none", KEY_NONE, -1 and a NaN; 0x5A is 1 515 870 810, below 2^31, and a large finite float; 0x01 is a small non-zero
count and a denormal-sized float.  The shapes are the suite's own, the smallest at which each path still runs; indexes, references
and the knob-unset answers are made once per case and shared by the three bytes.  The cases run one call at a time: the fill waits
for the device."""
import re
import time

import numpy as np
import pytest

import test_gpu_build_windows as BW
import test_gpu_dendrogram as DN
import test_gpu_exact_knn as EK
import test_gpu_exact_knn_filter_set as EFS
import test_gpu_exact_range as ER
import test_gpu_filter_set as FS
import test_gpu_graph_components as GC
import test_gpu_hdbscan as HD
import test_gpu_knn_graph as KG
import test_gpu_range_search as RS
import test_gpu_spanning_forest as SF
import test_gpu_symmetric_graph as SG
from conftest import uniform
from test_dendrogram_abi import dendrogram, random_forest
from test_gpu_build_windows import oracle_build  # noqa: F401  (the module's fixture: the windowed oracle build, made once)
from test_gpu_counters import _device_search, _pair, assert_lean_sound, assert_same_counters, check
from test_gpu_f16_storage import _r16, _to
from test_gpu_f64_reference import _assert_exact, _exhaustive_index
from test_gpu_parity import _tie_heavy, assert_same
from test_gpu_relaunch import _forced_call, _spread
from test_graph_components_abi import components, csr_edges
from test_hdbscan_abi import hdbscan_model
from test_knn_graph_abi import apply_drop_self, resolve
from test_range_search_abi import fixture, fixture_expected
from test_spanning_forest_abi import spanning_forest

pytestmark = pytest.mark.gpu

BYTES = [0xFF, 0x5A, 0x01]
_POISON = re.compile(r"^\[hnswgpu poison\] blocks (\d+) bytes (\d+) byte 0x([0-9a-f]{2})$", re.M)


class _Tee:
    """capfd for the helpers that read the launch lines themselves: what they read stays readable here"""

    def __init__(self, capfd):
        self.capfd, self.err = capfd, ""

    def readouterr(self):
        r = self.capfd.readouterr()
        self.err += r.err
        return r


def _blob(x):
    """the bytes of an answer: arrays as they are, objects by their attributes in name order.  Of the per-query stats words (st) the
    two clock readings, words 4 and 5, are left out."""
    if x is None:
        return b"-"
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, (bool, int, float, str, np.generic)):
        return repr(x).encode()
    if isinstance(x, (tuple, list)):
        return b"|".join(_blob(v) for v in x)
    if isinstance(x, dict):
        return b"|".join(_blob(x[k]) for k in sorted(x))
    out = []
    for name in sorted(vars(x)):
        v = getattr(x, name)
        if name.startswith("_") or callable(v):
            continue
        out.append(name.encode() + b"=" + (_blob(v[:, [0, 1, 2, 3, 6, 7]]) if name in ("st", "stats") and isinstance(v, np.ndarray) else _blob(v)))
    return b"|".join(out)


_PLAIN = {}   # case -> the bytes of its answer with the knob unset, and the seconds that call took
_MADE = {}    # what the cases share: indexes, inputs, references (never modified)


def _once(key, make):
    if key not in _MADE:
        _MADE[key] = make()
    return _MADE[key]


def _tmp(factory, name):
    return _once(("tmp", name), lambda: factory.mktemp("poison_" + name))


def _poisoned(knob, capfd, byte, case, run, expect=()):
    """run(capfd) -- which compares its answer with its own reference -- with the knob unset (once per case) and at `byte`; the two
    assertions of this file; `expect`: what the traced launch lines of the poisoned run must name (the path ran)"""
    if case not in _PLAIN:
        knob("HNSWGPU_POISON_SCRATCH", None)
        t0 = time.perf_counter()
        plain = run(capfd)
        _PLAIN[case] = (_blob(plain), time.perf_counter() - t0)
    knob("HNSWGPU_POISON_SCRATCH", byte)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    tee = _Tee(capfd)
    t0 = time.perf_counter()
    try:
        got = run(tee)
    finally:
        seconds = time.perf_counter() - t0
        tee.readouterr()
        knob("HNSWGPU_POISON_SCRATCH", None)
        knob("HNSWGPU_TRACE_LAUNCH", None)
    print(f"[poison seconds] {case}: knob unset {_PLAIN[case][1]:.3f}, 0x{byte:02x} {seconds:.3f}")
    lines = _POISON.findall(tee.err)
    assert lines, (case, "no poisoned call traced", tee.err[-400:])
    for blocks, nbytes, used in lines:
        assert int(blocks) > 0 and int(nbytes) > 0 and int(used, 16) == byte, (case, blocks, nbytes, used)
    for text in expect:
        assert text in tee.err, (case, text, [ln for ln in tee.err.splitlines() if ln.startswith("[hnswgpu launch]")])
    assert _blob(got) == _PLAIN[case][0], (case, f"the answer under 0x{byte:02x} differs from the answer with the knob unset")
    return got


# ----------------------------------------------------------------------------------------------------- the hook itself
def _tiny_call(native):
    rc, lab, sizes, c = GC.csr_host(native, 2, np.array([0, 1, 1], np.uint64), np.array([1], np.uint32))
    assert rc == 0 and c == 1 and lab.tolist() == [0, 0]


def test_the_hook_parses_and_reloads(native, knob, capfd):
    """unset, not a number, or outside 0 .. 255: off -- not a line; 0 is a byte like any other"""
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    for value in (None, "", "x", "-1", "256", "12x", "1e2"):
        knob("HNSWGPU_POISON_SCRATCH", value)
        capfd.readouterr()
        _tiny_call(native)
        assert not _POISON.findall(capfd.readouterr().err), value
    for value, byte in (("0", 0), ("1", 1), ("255", 255), ("0x5A", 0x5A)):
        knob("HNSWGPU_POISON_SCRATCH", value)
        capfd.readouterr()
        _tiny_call(native)
        lines = _POISON.findall(capfd.readouterr().err)
        assert len(lines) == 1 and int(lines[0][0]) > 0 and int(lines[0][1]) > 0 and int(lines[0][2], 16) == byte, (value, lines)
    knob("HNSWGPU_TRACE_LAUNCH", None)          # without the trace the hook still fills, and says nothing
    capfd.readouterr()
    _tiny_call(native)
    assert "[hnswgpu" not in capfd.readouterr().err


# ----------------------------------------------------------------------------------------------------- search
def _exhaustive(native, oracle, factory, n, d, m):
    return _once(("exhaustive", n, d, m), lambda: _exhaustive_index(native, oracle, _tmp(factory, f"x{n}"), "DistL2", n, d, m, 3))


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("n,d,m,ef,slots", [(60, 8, 16, 64, 1), (120, 8, 16, 128, 2), (250, 16, 24, 256, 4), (500, 16, 32, 512, 16)])
def test_every_result_set_shape(native, oracle, tmp_path_factory, knob, capfd, n, d, m, ef, slots, byte):
    """ef >= n through the host entry (two pooled workspaces a call): the exact f64 k-NN of the reachable set, and k > ef"""
    X, h, reach = _exhaustive(native, oracle, tmp_path_factory, n, d, m)
    Q = uniform(200, d, 4)
    Q[:10] = X[:10]

    def run(_):
        res = h.parallel_search_flat(Q, 10, ef)
        _assert_exact("DistL2", X, Q, res, 10, reach, f"slots {slots}")
        wide = h.parallel_search_flat(Q, n + 5, 8)
        _assert_exact("DistL2", X, Q, wide, n + 5, reach, "k > ef")
        return res, wide
    _poisoned(knob, capfd, byte, ("slots", slots), run, expect=(f"slots {slots},",))


@pytest.mark.parametrize("byte", BYTES)
def test_the_literal_kernel(native, oracle, tmp_path_factory, knob, capfd, byte):
    X, h, reach = _exhaustive(native, oracle, tmp_path_factory, 500, 16, 32)
    Q = uniform(60, 16, 5)

    def run(_):
        res = h.parallel_search_flat(Q, 10, 1100)
        _assert_exact("DistL2", X, Q, res, 10, reach, "ef 1100")
        return res
    _poisoned(knob, capfd, byte, "literal", run, expect=("literal kernel, pass 0",))


def _tie_pair(native, oracle, factory):
    def make():
        o, h = _pair(native, oracle, _tmp(factory, "ties"), _tie_heavy("grid", 4000, 6, 77), 8, 40, "DistL2", "ties")
        Q = _tie_heavy("grid", 600, 6, 78)
        return o, h, Q, o.parallel_search(Q, 10, 100, want_counters="per_query")
    return _once("ties", make)


@pytest.mark.parametrize("byte", BYTES)
def test_ties_strict_and_lean(native, oracle, tmp_path_factory, knob, capfd, byte):
    """strict: the oracle's answers and counters, queries ended with the literal heaps (status 3); lean: flagged queries (status 2)"""
    o, h, Q, ref = _tie_pair(native, oracle, tmp_path_factory)

    def run(_):
        res = _device_search(native, h, Q, 10, 100)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, "ties")
        assert (res.st[:, 3] == 3).sum() > 20
        h.set_strict_ties(False)
        try:
            lean = _device_search(native, h, Q, 10, 100)
        finally:
            h.set_strict_ties(True)
        assert_lean_sound(lean, ref, True, "ties (lean)")
        return res, lean
    _poisoned(knob, capfd, byte, "ties", run)


def _relaunch_pair(native, oracle, factory):
    def make():
        X = _spread(4000, 16, 21)
        o, h = _pair(native, oracle, _tmp(factory, "relaunch"), X, 16, 100, "DistL2", "rl")
        return X, o, h, _spread(600, 16, 22)
    return _once("relaunch", make)


@pytest.mark.parametrize("byte", BYTES)
def test_the_three_relaunch_paths(native, oracle, tmp_path_factory, knob, capfd, byte):
    """one bitmap slice and a forced first table: no slice, the grown table, the bitmap kernels -- strict, then lean; w.bitmap, w.cand
    and w.oplog are asked for again in the middle of the call"""
    X, o, h, Q = _relaunch_pair(native, oracle, tmp_path_factory)

    def run(cap):
        res, _, _ = _forced_call(native, knob, cap, h, o, Q, 10, 64, "poisoned relaunch")
        knob("HNSWGPU_HASH_BITS", None)
        knob("HNSWGPU_BITMAP_SLICES", None)
        return res.ids, res.dists, res.layers, res.ranks, res.counts, res.st[:, [0, 1, 2, 3, 6, 7]]
    _poisoned(knob, capfd, byte, "relaunch", run, expect=("visited set bitmap",))


@pytest.mark.parametrize("byte", BYTES)
def test_the_pair_pass(native, oracle, tmp_path_factory, knob, capfd, byte):
    """600 queries, two per wavefront, on 120 points (the table shrunk so that the id bits suffice): the exact f64 k-NN"""
    X, h, reach = _exhaustive(native, oracle, tmp_path_factory, 120, 8, 16)
    Q = uniform(600, 8, 11)

    def run(_):
        knob("HNSWGPU_PAIR_SEARCH", "1")
        knob("HNSWGPU_PAIR_TBITS_DELTA", "-20")
        try:
            res = h.parallel_search_flat(Q, 10, 128)
        finally:
            knob("HNSWGPU_PAIR_SEARCH", None)
            knob("HNSWGPU_PAIR_TBITS_DELTA", None)
        _assert_exact("DistL2", X, Q, res, 10, reach, "pair pass")
        return res
    _poisoned(knob, capfd, byte, "pair", run, expect=("pair pass",))


@pytest.mark.parametrize("byte", BYTES)
def test_one_filter(native, oracle, tmp_path_factory, knob, capfd, byte):
    X, o, h, _ = _relaunch_pair(native, oracle, tmp_path_factory)
    allowed = np.sort(np.random.default_rng(30).choice(4000, 1200, replace=False)).astype(np.uint64)
    Q = np.concatenate([_spread(150, 16, 93), X[:50]])
    ref = _once("one filter ref", lambda: o.parallel_search_filter(Q, 10, 200, allowed, want_counters="per_query"))

    def run(_):
        res = _device_search(native, h, Q, 10, 200, allowed)
        assert np.array_equal(res.st[:, 3] == 6, ref.status == 1)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, "one filter")
        return res
    _poisoned(knob, capfd, byte, "one filter", run, expect=("literal kernel",))


def _filter_set_case(native, oracle, factory):
    def make():
        X = uniform(FS.N_MIXED, FS.D_MIXED, 301)
        origin = (7 * np.arange(FS.N_MIXED) + 3).astype(np.uint64)
        o, h = FS._pair(native, oracle, _tmp(factory, "fs"), X, 8, 40, "DistL2", origin)
        Q = uniform(70, FS.D_MIXED, 303)
        filters = [FS._subset(origin, f, 20 + i) for i, f in enumerate((0.5, 0.02, 1.0, 0.1, 0.0, 0.3, 0.05))]
        filter_of = ((np.arange(70) * 5 + 2) % 7).astype(np.uint32)
        return h, Q, filters, filter_of, FS._oracle_answers(o, Q, 10, 40, filters, filter_of)
    return _once("filter set", make)


@pytest.mark.parametrize("byte", BYTES)
def test_a_filter_set_in_two_groups(native, oracle, tmp_path_factory, knob, capfd, byte):
    """a bitmap of this index is 252 bytes; 0.00097 MiB = 1017 bytes hold four: seven filters are two groups"""
    h, Q, filters, filter_of, ref = _filter_set_case(native, oracle, tmp_path_factory)

    def run(_):
        knob("HNSWGPU_FILTER_SET_MB", "0.00097")
        try:
            got = h.parallel_search_filters_flat(Q, 10, 40, filters, filter_of)
        finally:
            knob("HNSWGPU_FILTER_SET_MB", None)
        FS._assert_equal(got, ref, "two groups")
        return got
    _poisoned(knob, capfd, byte, "filter set", run, expect=("filter set: filters 0..3", "filter set: filters 4..6"))


@pytest.mark.parametrize("byte", BYTES)
def test_simd8_arithmetic(native, oracle, tmp_path_factory, knob, capfd, byte):
    def make():
        o, h = _pair(native, oracle, _tmp(tmp_path_factory, "s8"), uniform(2500, 37, 61), 12, 60, "DistL2", "s8")
        return o, h, uniform(300, 37, 62)
    o, h, Q = _once("simd8", make)

    def run(_):
        h.set_arithmetic("simd8")
        o.set_simd_order(True)
        try:
            res, _ = check(native, h, o, Q, 10, 64, "simd8")
        finally:
            h.set_arithmetic("scalar")
            o.set_simd_order(False)
        return res
    _poisoned(knob, capfd, byte, "simd8", run)


@pytest.mark.parametrize("byte", BYTES)
def test_f16_storage(native, oracle, tmp_path_factory, knob, capfd, byte):
    def make():
        X = _r16(native, uniform(3000, 128, 502))
        o, h = _pair(native, oracle, _tmp(tmp_path_factory, "f16"), X, 16, 100, "DistL2", "f16")
        Q = uniform(300, 128, 602)
        return o, _to(h, "f16"), Q, o.parallel_search(Q, 10, 100, want_counters="per_query")
    o, h, Q, ref = _once("f16", make)

    def run(_):
        assert h.get_storage() == "f16"
        res = _device_search(native, h, Q, 10, 100)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, "f16")
        return res
    _poisoned(knob, capfd, byte, "f16", run)


@pytest.mark.parametrize("byte", BYTES)
def test_approximate_range_search_with_growing_ef(native, oracle, tmp_path_factory, knob, capfd, byte):
    """ef from 8 to 256: every round searches the pending queries again, the staged and the held answers are the call's own blocks"""
    def make():
        o, X, Q, radii = fixture()
        return RS._load(native, o, _tmp(tmp_path_factory, "range"), "DistL2"), Q, radii
    h, Q, radii = _once("range", make)
    want = fixture_expected(8, 256)
    assert len(set(want.ef.tolist())) >= 4

    def run(_):
        got = h.range_search_flat(Q, radii, 8, 256)
        RS._same(got, want, "(8, 256)")
        return got
    _poisoned(knob, capfd, byte, "range", run)


@pytest.mark.parametrize("byte", BYTES)
def test_the_approximate_graph_in_three_chunks(native, oracle, tmp_path_factory, knob, capfd, byte):
    def make():
        metric, n, d, m, _ = KG.SHAPES["l2"]
        X = uniform(n, d, 77)
        ids = np.random.default_rng(n).permutation(n).astype(np.uint64) * 2 + 10
        o = oracle.OracleHnsw(m, n, 16, 48, metric)
        o.insert_batch(X, ids)
        tmp = _tmp(tmp_path_factory, "graph")
        o.file_dump(str(tmp), "g")
        h = native.HnswIo(str(tmp), "g").load_hnsw(metric)
        h.upload(0)
        me = h.exact_search_filters_flat(X, 1, [np.array([v], np.uint64) for v in ids])
        own = list(zip(me.layers[:, 0].tolist(), me.ranks[:, 0].tolist()))
        assert me.counts.tolist() == [1] * n and len(set(own)) == n
        rows = np.argsort(ids)
        b = dict(ref=o.parallel_search(X, 11, 40))
        return h, n, apply_drop_self(KG._subset(b, rows), [own[r] for r in rows], 10)
    h, n, want = _once("graph", make)
    chunk = (n + 2) // 3 + 33
    assert 2 * chunk < n < 3 * chunk

    def run(_):
        knob("HNSWGPU_GRAPH_CHUNK", chunk)
        try:
            got = h.knn_graph_flat(10, 40)
        finally:
            knob("HNSWGPU_GRAPH_CHUNK", None)
        KG._assert_rows(got, want, "three chunks")
        return got
    _poisoned(knob, capfd, byte, "graph chunks", run)


# ----------------------------------------------------------------------------------------------------- the exact unit
def _exact_case(native, oracle):
    """test_gpu_exact_range's built case: 2500 x 33, 37 queries (two tiles and a part), radii of every kind"""
    return _once("exact", lambda: ER._built_case(native, oracle, "DistL2", 33))


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("k", [1, 10, 2505])
def test_exact_knn(native, oracle, knob, capfd, k, byte):
    h, X, Q, ids, D, radii, _ = _exact_case(native, oracle)

    def run(_):
        res = h.exact_search_flat(Q, k)
        EK._assert_answers(oracle, "DistL2", res, Q, X, ids, k, what=f"k {k}")
        return res
    _poisoned(knob, capfd, byte, ("exact", k), run)


@pytest.mark.parametrize("byte", BYTES)
def test_exact_knn_under_one_filter(native, oracle, knob, capfd, byte):
    h, X, Q, ids, D, radii, _ = _exact_case(native, oracle)
    rows = np.sort(np.random.default_rng(7).choice(len(X), 750, replace=False))
    allowed = np.sort(np.concatenate([ids[rows], np.array([2, 3, 10 ** 15], np.uint64)]))

    def run(_):
        res = h.exact_search_flat(Q, 10, allowed)
        EK._assert_answers(oracle, "DistL2", res, Q, X, ids, 10, rows, what="one filter")
        return res
    _poisoned(knob, capfd, byte, "exact filter", run)


@pytest.mark.parametrize("byte", BYTES)
def test_exact_knn_under_a_mixed_filter_set(native, oracle, tmp_path_factory, knob, capfd, byte):
    def make():
        ix = EFS._Index(native, _tmp(tmp_path_factory, "efs"), "DistL2", 2530, 33, 77)
        ix.rows, ix.filters = EFS._seven(ix, 8)
        Q = uniform(37, 33, 2033)
        return ix, Q, oracle.dist_matrix("DistL2", Q, ix.X)
    ix, Q, D = _once("exact filter set", make)
    mixed = ((np.arange(37) * 3 + 1) % 7).astype(np.uint32)

    def run(_):
        res = ix.h.exact_search_filters_flat(Q, 10, ix.filters, mixed)
        EFS._assert_set(oracle, ix, res, Q, ix.rows, mixed, 10, "mixed", D)
        return res
    _poisoned(knob, capfd, byte, "exact filter set", run)


@pytest.mark.parametrize("byte", BYTES)
def test_exact_range_search_one_hit_per_pass(native, oracle, knob, capfd, byte):
    """HNSWGPU_RANGE_HITS_PER_PASS = 1: every query with an answer gets a fill pass of its own over the same keys, temporary
    storage and staging area"""
    h, X, Q, ids, D, radii, _ = _exact_case(native, oracle)

    def run(_):
        knob("HNSWGPU_RANGE_HITS_PER_PASS", 1)
        try:
            res = h.exact_range_search_flat(Q, radii)
        finally:
            knob("HNSWGPU_RANGE_HITS_PER_PASS", None)
        ER._assert_range(res, D, ids, radii, what="one hit per pass")
        return res
    _poisoned(knob, capfd, byte, "exact range", run)


@pytest.mark.parametrize("byte", BYTES)
def test_the_exact_graph(native, oracle, tmp_path_factory, knob, capfd, byte):
    """n = 700: three slabs and 44 tiles, the last of 12 queries, every point queried"""
    def make():
        case = KG._case("DistL2", 25)
        h = case.load(native, _tmp(tmp_path_factory, "exact_graph"))
        order = KG.dump_order(case.levels)[0]
        pos = np.empty(KG.N, np.int64)
        pos[order] = np.arange(KG.N)
        D = oracle.dist_matrix("DistL2", case.X, case.X)
        rows = resolve(case.ids, None)[0]
        return h, KG._exact_expected(D, case.ids, pos, case.pids, rows, 10)
    h, want = _once("exact graph", make)

    def run(_):
        res = h.exact_knn_graph_flat(10)
        KG._assert_rows(res, want, "exact graph")
        return res
    _poisoned(knob, capfd, byte, "exact graph", run)


# ----------------------------------------------------------------------------------------------------- the graph units
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("n", [257, 3000])
def test_the_symmetric_graph(native, oracle, tmp_path_factory, knob, capfd, n, byte):
    ix = SG._uniform_index(native, oracle, tmp_path_factory, n)

    def run(_):
        out = []
        for ef in SG.EFS:
            for mode in SG.MODES:
                want = ix.want(5, ef, mode)      # (the model on the public graph calls: made by the first, knob-unset run)
                got = ix.h.symmetric_knn_graph_flat(5, ef, mode)
                SG._same(got, want, f"n {n} ef {ef} {mode}")
                out.append(got)
        return out
    _poisoned(knob, capfd, byte, ("symmetric", n), run)


@pytest.mark.parametrize("byte", BYTES)
def test_components_of_a_random_csr(native, knob, capfd, byte):
    def make():
        n = 3000
        e = np.stack([np.repeat(np.arange(n), 2), np.random.default_rng(n).integers(0, n, n * 2)], 1)
        offsets, cols, _ = GC.to_csr(n, e)
        return n, offsets, cols, components(n, csr_edges(offsets, cols, None, None))
    n, offsets, cols, (want_lab, want_sizes) = _once("csr components", make)

    def run(_):
        rc, lab, sizes, c = GC.csr_host(native, n, offsets, cols)
        assert rc == 0 and c == len(want_sizes), (rc, c)
        assert np.array_equal(lab[:n], want_lab) and np.array_equal(sizes[:c], want_sizes) and (sizes[c:] == GC.SIZE).all()
        dev = GC.csr_device(native, n, offsets, cols)
        assert dev[0] == 0 and dev[3] == c and np.array_equal(dev[1][:n], want_lab) and np.array_equal(dev[2][:c], want_sizes)
        return lab, sizes, c, dev[1], dev[2]
    _poisoned(knob, capfd, byte, "csr components", run)


@pytest.mark.parametrize("byte", BYTES)
def test_components_of_the_index_with_a_cut(native, oracle, tmp_path_factory, knob, capfd, byte):
    ix = SG._uniform_index(native, oracle, tmp_path_factory, 3000)

    def run(_):
        res, _ = ix.D(5, None)
        cut = float(np.median(res.dists[np.arange(5)[None, :] < res.counts[:, None]]))
        out = [GC.check_index(ix, 5, ef, mode, cut, "cut") for ef in GC.EFS for mode in GC.MODES]
        return [(g.labels, g.sizes, g.n_components) for g in out]
    _poisoned(knob, capfd, byte, "index components", run)


def _forest_rows(native, n, offsets, cols, d, want):
    wa, wb, ww = want
    m = len(wa)
    out = []
    for call in (SF.csr_host, SF.csr_device):
        rc, a, b, w, got_m = call(native, n, offsets, cols, d)
        assert rc == 0 and got_m == m, (rc, got_m, m, native._native.last_error())
        assert np.array_equal(a[:m], wa) and np.array_equal(b[:m], wb) and np.array_equal(w[:m], SF._bits(ww))
        assert (a[m:] == SF.A).all() and (b[m:] == SF.B).all() and (w[m:] == SF.W).all()
        out += [a, b, w]
    return out


@pytest.mark.parametrize("byte", BYTES)
def test_the_spanning_forest_of_a_csr_with_hostile_weights(native, knob, capfd, byte):
    """NaN (two payloads), -0, +0, +inf, negatives on 2000 vertices; then without weights"""
    def make():
        n = 2000
        rng = np.random.default_rng(9)
        e = np.stack([rng.integers(0, n, 3000), rng.integers(0, n, 3000)], 1)
        offsets, cols, order = GC.to_csr(n, e)
        d = rng.random(3000, dtype=np.float32) - np.float32(0.25)
        d[::7], d[1::7], d[2::7], d[3::7] = np.nan, -0.0, np.inf, 0.0
        d.view(np.uint32)[::14] = 0xFFC00001
        d = d[order]
        return (n, offsets, cols, d, spanning_forest(n, SF.csr_triples(offsets, cols, d)), spanning_forest(n, SF.csr_triples(offsets, cols, None)))
    n, offsets, cols, d, want, want_plain = _once("csr forest", make)

    def run(_):
        return _forest_rows(native, n, offsets, cols, d, want) + _forest_rows(native, n, offsets, cols, None, want_plain)
    _poisoned(knob, capfd, byte, "csr forest", run)


@pytest.mark.parametrize("byte", BYTES)
def test_the_spanning_forests_of_tiny_graphs(native, knob, capfd, byte):
    def run(_):
        SF.test_tiny_graphs(native)
        rc, a, b, w, m = SF.csr_host(native, 2, np.array([0, 1, 1], np.uint64), np.array([1], np.uint32), np.array([2.5], np.float32))
        assert rc == 0 and m == 1
        return a, b, w
    _poisoned(knob, capfd, byte, "tiny forests", run)


@pytest.mark.parametrize("byte", BYTES)
def test_the_spanning_forest_of_the_index_with_core_distances(native, oracle, tmp_path_factory, knob, capfd, byte):
    ix = SG._uniform_index(native, oracle, tmp_path_factory, 3000)

    def run(_):
        out = [SF.check_index(ix, 5, ef, mode, 3, "core") for ef in SF.EFS for mode in SF.MODES]
        return [(g.a, g.b, g.weights, g.n_edges) for g in out]
    _poisoned(knob, capfd, byte, "index forest", run)


def _dendrogram_rows(native, n, edges, want):
    a, b = np.ascontiguousarray(edges[:, 0], np.uint32), np.ascontiguousarray(edges[:, 1], np.uint32)
    m = len(a)
    out = []
    for call in (DN.forest_host, DN.forest_device):
        rc, left, right, size = call(native, n, a, b)
        assert rc == 0, native._native.last_error()
        for got, exp, sentinel in ((left, want[0], DN.LEFT), (right, want[1], DN.RIGHT), (size, want[2], DN.SIZE)):
            assert np.array_equal(got[:m], exp) and (got[m:] == sentinel).all()
        out += [left, right, size]
    return out


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_the_dendrogram_around_a_block_boundary(native, knob, capfd, m, byte):
    """a chain of m edges in order and a random forest of exactly m: `size` stands where `top` stood, the compress kernel's marks
    where `wsum` stands next"""
    def make():
        chain = DN.path(m + 1)
        forest = np.asarray(random_forest(m + 40, np.random.default_rng(m), keep=1.0)[:m], np.int64).reshape(-1, 2)
        return chain, dendrogram(m + 1, chain), forest, dendrogram(m + 40, forest)
    chain, want_chain, forest, want_forest = _once(("dendrogram", m), make)

    def run(_):
        return _dendrogram_rows(native, m + 1, chain, want_chain) + _dendrogram_rows(native, m + 40, forest, want_forest)
    _poisoned(knob, capfd, byte, ("dendrogram", m), run)


@pytest.mark.parametrize("byte", BYTES)
def test_the_dendrogram_of_a_random_tree(native, knob, capfd, byte):
    def make():
        n = 20000
        e = np.asarray(random_forest(n, np.random.default_rng(n), keep=1.0), np.int64).reshape(-1, 2)
        assert len(e) == n - 1
        return n, e, dendrogram(n, e)
    n, e, want = _once("random tree", make)
    _poisoned(knob, capfd, byte, "random tree", lambda _: _dendrogram_rows(native, n, e, want))


def _hdbscan_rows(native, n, a, b, w, mcs, wants, exact, what):
    out = []
    for method in HD.METHODS:       # leaf: the clusters that win are exactly the leaves, every other `wins` word stays as zeroed
        for call in (HD.forest_host, HD.forest_device):
            rc, o = call(native, n, a, b, w, mcs, method)
            assert rc == 0, (what, method, native._native.last_error())
            HD.compare(o, wants[method], (what, mcs, method), exact)
            out.append(HD._bytes(o))
    return out


def _hdbscan_case(name):
    if name == "comb":
        n, e, w = HD.comb(200, 3)
        mcs, exact = 3, True
    elif name == "bit-reversed":
        n, mcs, exact = 4096, 2, True
        order = np.argsort(np.array([DN._bit_reversed(i, 12) for i in range(n - 1)]), kind="stable")
        level = np.array([len(format(i, "b")) - len(format(i, "b").rstrip("1")) for i in range(n - 1)])
        e, w = DN.path(n)[order], np.exp2(level[order]).astype(np.float32)
    else:
        n, mcs, exact = 257, 5, False
        e = DN.path(n)[np.random.default_rng(2571).permutation(n - 1)]
        w = np.sort(np.random.default_rng(2570).random(n - 1, dtype=np.float32) + np.float32(0.05))
    e = np.asarray(e, np.int64).reshape(-1, 2)
    a, b = np.ascontiguousarray(e[:, 0], np.uint32), np.ascontiguousarray(e[:, 1], np.uint32)
    w = np.ascontiguousarray(w, np.float32)
    wants = {method: hdbscan_model(n, a, b, w, mcs, method) for method in HD.METHODS}
    assert all(v is not None for v in wants.values())
    return n, a, b, w, mcs, wants, exact


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("name", ["comb", "bit-reversed", "float path"])
def test_hdbscan_of_a_forest(native, knob, capfd, name, byte):
    """comb(200, 3): the arrival counters climb 199 steps; the bit-reversed path of 4096 at mcs = 2: K at its bound, every per-cluster
    slot in use; the 257-vertex path with float weights.  Six per-cluster arrays are zeroed by one memset: both methods"""
    n, a, b, w, mcs, wants, exact = _once(("hdbscan", name), lambda: _hdbscan_case(name))
    _poisoned(knob, capfd, byte, ("hdbscan", name), lambda _: _hdbscan_rows(native, n, a, b, w, mcs, wants, exact, name))


@pytest.mark.parametrize("byte", BYTES)
def test_hdbscan_of_the_index(native, oracle, tmp_path_factory, knob, capfd, byte):
    ix = SG._uniform_index(native, oracle, tmp_path_factory, 3000)

    def run(_):
        out = HD.check_index(ix, 5, None, "union", 3, 10, "3000")
        return [(g.labels, g.probabilities, g.point_cluster, g.point_w, g.cluster_parent, g.cluster_birth_w, g.cluster_size, g.stability,
                 g.selected, g.n_clusters, g.n_labels, g.forest.a, g.forest.b, g.forest.weights, g.dendrogram.left, g.dendrogram.right,
                 g.dendrogram.sizes) for g, _ in (out[m] for m in HD.METHODS)]
    _poisoned(knob, capfd, byte, "index hdbscan", run)


# ----------------------------------------------------------------------------------------------------- GPU-assisted build
@pytest.mark.parametrize("byte", BYTES)
def test_the_gpu_assisted_build(native, oracle, oracle_build, knob, capfd, byte):  # noqa: F811
    """one host thread, windows of 256 points on the default grid: the dump equals the windowed oracle's byte for byte; the backend's
    scratch is filled in front of every window and every patch"""
    def run(_):
        stats, sizes = BW._case(native, oracle_build, oracle, BW.PLAIN)
        assert sizes == [256] * 5 + [196]
        directory = oracle_build(BW.PLAIN)[0]
        return [open(directory / ("gpu" + ext), "rb").read() for ext in (".hnsw.graph", ".hnsw.data")]
    _poisoned(knob, capfd, byte, "build", run)


# ----------------------------------------------------------------------------------------------------- one handle, every layout
def _reuse_case(native, oracle, factory):
    def make():
        n, d = 1500, 16
        X = uniform(n, d, 811)
        ids = np.arange(n, dtype=np.uint64)
        o, h = FS._pair(native, oracle, _tmp(factory, "reuse"), X, 8, 40, "DistL2", ids)
        Q = uniform(37, d, 812)
        Q[:3] = X[5:8]
        D = oracle.dist_matrix("DistL2", Q, X)
        radii, _ = ER._cycled_radii(D)
        DX = oracle.dist_matrix("DistL2", X, X)
        graph = np.zeros((n, 10), np.uint64), np.zeros((n, 10), np.float32)
        for p in range(n):
            c = np.delete(np.arange(n), p)
            best = c[np.lexsort((ids[c], DX[p, c]))][:10]
            graph[0][p], graph[1][p] = ids[best], DX[p, best] + np.float32(0.0)
        allowed = np.sort(np.random.default_rng(813).choice(n, 500, replace=False)).astype(np.uint64)
        filtered = o.parallel_search_filter(Q, 10, 1100, allowed, want_counters="per_query")
        return dict(X=X, o=o, h=h, ids=ids, Q=Q, D=D, radii=radii, graph=graph, allowed=allowed, filtered=filtered)
    return _once("reuse", make)


@pytest.mark.parametrize("byte", [None] + BYTES)
def test_one_handle_through_every_layout(native, oracle, tmp_path_factory, knob, capfd, byte):
    """exact k-NN with k = 1024, with k = 1, an exact range search, the exact graph, a filtered search with ef 1100 and a plain search
    with ef 16, in this order on one handle: the exact unit's block and the pooled workspace pass from layout to layout, and every
    answer is compared with its own reference -- knob unset, where the words are what the call before left, and at every byte"""
    r = _reuse_case(native, oracle, tmp_path_factory)
    h, o, X, Q, ids = r["h"], r["o"], r["X"], r["Q"], r["ids"]
    knob("HNSWGPU_POISON_SCRATCH", byte)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    for k in (1024, 1):
        EK._assert_answers(oracle, "DistL2", h.exact_search_flat(Q, k), Q, X, ids, k, what=f"k {k}")
    ER._assert_range(h.exact_range_search_flat(Q, r["radii"]), r["D"], ids, r["radii"], what="range")
    g = h.exact_knn_graph_flat(10)
    assert g.counts.tolist() == [10] * len(X) and np.array_equal(g.ids, r["graph"][0])
    assert np.array_equal(g.dists.view(np.uint32), r["graph"][1].view(np.uint32))
    res = _device_search(native, h, Q, 10, 1100, r["allowed"])
    assert np.array_equal(res.st[:, 3] == 6, r["filtered"].status == 1)
    assert_same(res, r["filtered"])
    assert_same_counters(res.st, r["filtered"], "filtered, ef 1100")
    check(native, h, o, Q, 10, 16, "ef 16", lean=False)
    lines = _POISON.findall(capfd.readouterr().err)
    if byte is None:
        assert not lines
    else:
        assert len(lines) >= 6 and all(int(nb) > 0 and int(used, 16) == byte for _, nb, used in lines), lines
