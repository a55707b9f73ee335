"""The stream contract of every entry that takes a caller's HIP stream (include/hnsw_mi355x.h: the `_device` forms, the ticket pair,
the gather), called with work STILL PENDING on that stream: device inputs are read and device outputs written in the order of
`stream`, so work queued on it before the call needs no host wait, and when the call returns the stream has been waited for.

Every other test of these entries synchronises first, so the entry meets an idle device and inputs that are long since final; a
helper kernel on stream 0, a blocking copy in place of a kernel, a workspace's own stream used where the argument was meant, pass
there every time.  Torch's streams are non-blocking: the legacy null stream does not order itself against them, so such a slip is a
real race for a caller.  Here every entry is called twice behind a delay on its stream (run_entry):

  read after write   every device input holds a DECOY (a valid input of the same sizes that gives another answer); the stream holds
                     the delay, then device-to-device copies of the true inputs over the decoys.  A read that does not wait for
                     the stream sees the decoy and gives a well-formed wrong answer.
  write after read   the outputs hold a sentinel; the stream holds the delay, then copies of every output into snapshots.  A write
                     (or a clearing memset) that does not wait for the stream shows up in the snapshot.

Immediately before the call an event recorded behind the producer must still be pending -- a case whose input was already final has
tested nothing and FAILS; it is not retried.  After the call the stream must be idle.  The delay D is a condition, not a number:
each case first makes one ordinary, synchronised call of the same entry with the same shapes (which also builds every first-use state
of the replica), timed on the host; D = 2 x that, at least 20 ms.  D only has to outlast the span from queuing the producer to the
entry's first own wait on the stream, which is at most that call's duration.  The delay is torch.cuda._sleep (a chain of torch.mm
where that is missing), calibrated once with two events; no kernel of the product's.

No decoy is an input an entry refuses or one that could fault a kernel: same shapes, ids that exist, cols below n, the same CSR
total, finite non-negative radii.  Nothing here provokes anything; a wrong order only becomes a wrong answer.

The expected answers come from the models and the oracle the suite already has (imported, not restated), never from a call of the
entry under test: the oracle's searches, its distance matrix with the helpers of test_gpu_exact_knn / test_gpu_exact_range /
test_gpu_exact_knn_filter_set / test_gpu_knn_graph, range_rule, resolve and apply_drop_self, symmetrise, components and csr_edges,
pair_weights and spanning_forest, dendrogram and random_forest.  The warm-up's answers are compared with the model too.

What a case CANNOT see:
  * behind an entry's first own wait on the stream (its first read-back) the producer is done, so a stray read or write behind that
    point is invisible.  Entries that validate their input and read a word back first (the CSR pair, the dendrogram, the filter sets,
    the graph calls' id resolution) are covered up to that read-back only.
  * a stray operation on a stream that happens to share the delayed stream's hardware queue may be ordered behind the delay by the
    queue itself.  The test machines run with GPU_MAX_HW_QUEUES=4, which this file does not change; its streams are picked once per
    session among torch's so that, where possible, a marker on the null stream completes while they are delayed (_streams), which is
    the stray operation most likely to be written.
  * a stray host-blocking call that waits for the whole device (hipDeviceSynchronize, hipFree of live memory) in front of the first
    launch hides everything behind it: the producer is then done when the entry's kernels start.
"""
import ctypes as C
import time
import types
import warnings

import numpy as np
import pytest

import f64_reference as F
from conftest import uniform
from test_dendrogram_abi import dendrogram, random_forest
from test_gpu_counters import _launch_lines, _pair, assert_same_counters
from test_gpu_exact_knn import _assert_answers, _build
from test_gpu_exact_knn_filter_set import _assert_set
from test_gpu_exact_range import _assert_range
from test_gpu_filter_set import _assert_equal, _oracle_answers
from test_gpu_knn_graph import _assert_rows, _exact_expected
from test_gpu_parity import assert_same
from test_gpu_range_search import _same as _same_range
from test_gpu_relaunch import _forced_bits, _spread
from test_graph_components_abi import components, csr_edges, cut_and_join
from test_knn_graph_abi import apply_drop_self, resolve
from test_range_search_abi import fixture, fixture_expected, range_rule
from test_spanning_forest_abi import pair_weights, spanning_forest
from test_symmetric_graph_abi import symmetrise

pytestmark = pytest.mark.gpu

K, EF = 10, 48
MIN_DELAY_MS = 20.0
SENTINEL = 0xA5
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


# ----------------------------------------------------------------------------------------------------- the harness
def _sentinel(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = SENTINEL
    return a


def _dev(a):
    """a numpy array as a device tensor of the same bytes (torch has no arithmetic on u32 / u64: they travel as i32 / i64)"""
    import torch
    a = np.ascontiguousarray(a)
    assert a.size > 0
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


_CAL = {}


def _calibrate():
    """once per session: the delay kernel's units per millisecond, from two events around one delay"""
    import torch
    if _CAL:
        return _CAL
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        units = 1_000_000
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)                             # (loads the kernel)
        s.synchronize()
        for _ in range(5):                                      # (grow until it is measurable)
            with torch.cuda.stream(s):
                e0.record(s)
                torch.cuda._sleep(units)
                e1.record(s)
            s.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0:
                break
            units *= 8
        _CAL.update(kind="sleep", per_ms=units / ms)
    else:
        with torch.cuda.stream(s):
            a = torch.randn(4096, 4096, device="cuda")
            torch.mm(a, a)
            e0.record(s)
            for _ in range(8):
                torch.mm(a, a)
            e1.record(s)
        s.synchronize()
        _CAL.update(kind="mm", per_ms=8 / e0.elapsed_time(e1), a=a)
    return _CAL


def _delay(stream, ms):
    """queue about `ms` milliseconds of work on `stream`"""
    import torch
    cal = _calibrate()
    with torch.cuda.stream(stream):
        if cal["kind"] == "sleep":
            torch.cuda._sleep(int(ms * cal["per_ms"]))
        else:
            for _ in range(max(1, int(ms * cal["per_ms"] + 1))):
                torch.mm(cal["a"], cal["a"])


_POOL = []


def _streams(count):
    """`count` streams, the same ones for the whole session: torch streams on which a delay does NOT hold back the null stream come
    first (a marker recorded on the null stream completes while the stream is delayed), so that a stray launch on stream 0 is not
    hidden by a shared hardware queue.  Streams that share the null stream's queue are used only when there are no others."""
    import torch
    if not _POOL:
        null = torch.cuda.default_stream()
        tick = torch.zeros(64, device="cuda")
        tick.add_(1)                                            # (loads the marker's kernel)
        free, shared = [], []
        for _ in range(8):
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            _delay(s, 30.0)
            tick.add_(1)
            marker = torch.cuda.Event()
            marker.record(null)
            t0 = time.perf_counter()
            while not marker.query() and time.perf_counter() - t0 < 0.015:
                pass
            (free if marker.query() and not s.query() else shared).append(s)
            s.synchronize()
        if len(free) < 3:
            warnings.warn(f"only {len(free)} of 8 streams run beside the null stream: a stray operation on stream 0 may go unseen")
        _POOL.extend(free + shared)
        _CAL["free_streams"] = len(free)
    return _POOL[:count]


class Entry:
    """One call of an entry under test.
    ins    name -> (true, decoy): the device inputs (numpy, same shape and dtype, different contents)
    outs   name -> (shape, dtype): the device outputs
    call   (p, sp) -> status: p maps every name to its device address (an int), sp the streams' handles (ints)
    check  (got) -> None: got maps every output to its numpy array; asserts the model's answers
    where  name -> index of the stream its producer / snapshot is queued on (0 when absent)"""

    def __init__(self, name, ins, outs, call, check, n_streams=1, where=None):
        self.name, self.ins, self.outs, self.call, self.check, self.n_streams, self.where = name, ins, outs, call, check, n_streams, where or {}
        for k, (t, d) in ins.items():
            assert t.shape == d.shape and t.dtype == d.dtype and not np.array_equal(t, d), (name, k, "a decoy must differ from the input")


LOG = []
WARM_UP_ON_NULL_STREAM = False   # a switch for mutation runs by hand (RESULTS.md): see run_entry


def _report():
    """the last case's warm-up time and delay, for the reader of a run with -s"""
    name, warm_ms, delay_ms = LOG[-1]
    print(f"[stream order] {name}: warm-up {warm_ms:.2f} ms, D {delay_ms:.2f} ms, delay by {_CAL['kind']}, {_CAL.get('free_streams')} of 8 streams beside the null stream")


def run_entry(native, e):
    """the warm-up, then the two cases of the module's docstring"""
    import torch
    NN = native._native
    streams = _streams(e.n_streams)
    sp = [s.cuda_stream for s in streams]
    used = sorted({e.where.get(k, 0) for k in list(e.ins) + list(e.outs)})   # (an empty shard's stream is nothing the entry waits for)
    true_in = {k: _dev(t) for k, (t, _) in e.ins.items()}

    def fresh_outs():
        return {k: _dev(_sentinel(shape, dtype)) for k, (shape, dtype) in e.outs.items()}

    def ptrs(ins, outs):
        p = {k: t.data_ptr() for k, t in ins.items()}
        p.update({k: t.data_ptr() for k, t in outs.items()})
        return p

    def read(outs):
        torch.cuda.synchronize()
        return {k: _host(t, e.outs[k][1]).reshape(e.outs[k][0]) for k, t in outs.items()}

    def behind_a_delay(ms, copies):
        """per stream: the delay, the copies (dst, src) that belong to it, an event behind them; returns the events"""
        events = []
        for i, s in enumerate(streams):
            _delay(s, ms)
            with torch.cuda.stream(s):
                for name, dst, src in copies:
                    if e.where.get(name, 0) == i:
                        dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
            events.append(ev)
        return events

    # the warm-up: an ordinary call on an idle device, timed on the host.  (WARM_UP_ON_NULL_STREAM: on stream 0 instead -- for a run
    # against a library with a launch moved to stream 0 on purpose, whose idle-stream call would otherwise race with itself)
    outs = fresh_outs()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = e.call(ptrs(true_in, outs), [None] * len(sp) if WARM_UP_ON_NULL_STREAM else sp)
    warm_ms = (time.perf_counter() - t0) * 1e3
    assert rc == NN.OK, (e.name, "warm-up", NN.last_error())
    e.check(read(outs))
    delay_ms = max(2.0 * warm_ms, MIN_DELAY_MS)
    LOG.append((e.name, warm_ms, delay_ms))
    _report()

    if e.ins:                                                   # read after write
        bufs = {k: _dev(d) for k, (_, d) in e.ins.items()}
        outs = fresh_outs()
        torch.cuda.synchronize()
        events = behind_a_delay(delay_ms, [(k, bufs[k], true_in[k]) for k in bufs])
        assert not any(ev.query() for ev in events), (e.name, "read after write: the producer was done before the call: nothing tested")
        rc = e.call(ptrs(bufs, outs), sp)
        idle = [streams[i].query() for i in used]
        assert rc == NN.OK, (e.name, "read after write", NN.last_error())
        assert all(idle), (e.name, "read after write: the call returned with work pending on its stream")
        try:
            e.check(read(outs))
        except AssertionError as err:
            raise AssertionError(f"{e.name}: READ AFTER WRITE -- an input was read before the work queued on the stream had produced it: {err}") from err

    # write after read
    outs = fresh_outs()
    snaps = {k: torch.zeros_like(t) for k, t in outs.items()}
    torch.cuda.synchronize()
    events = behind_a_delay(delay_ms, [(k, snaps[k], outs[k]) for k in outs])
    assert not any(ev.query() for ev in events), (e.name, "write after read: the snapshots were done before the call: nothing tested")
    rc = e.call(ptrs(true_in, outs), sp)
    idle = [streams[i].query() for i in used]
    assert rc == NN.OK, (e.name, "write after read", NN.last_error())
    assert all(idle), (e.name, "write after read: the call returned with work pending on its stream")
    got = read(outs)
    for k, t in snaps.items():
        snap = _host(t, np.uint8)
        assert (snap == SENTINEL).all(), (f"{e.name}: WRITE AFTER READ -- output `{k}` was written before the work queued on the stream had read it: "
                                          f"{int((snap != SENTINEL).sum())} of {snap.size} snapshot bytes changed, first at byte {int(np.flatnonzero(snap != SENTINEL)[0])}")
    e.check(got)


# ----------------------------------------------------------------------------------------------------- the harness, on itself
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize("stray", [None, "read", "write"])
def test_the_harness_sees_a_stray_operation_on_stream_0(native, stray):
    """An "entry" made of plain HIP copies, out = in: on its stream it passes; with its input read through stream 0 the read-after-write
    case must fail, with its output cleared through stream 0 the write-after-read case must -- what the three changed libraries of
    RESULTS.md show for the product, kept in the suite for the harness.  Plain copies of valid buffers: nothing can fault.  Where no
    stream runs beside the null stream (see _streams) a stray operation on stream 0 cannot be seen, and only the clean form is held."""
    import torch
    hip = _hip()
    true, decoy = np.arange(4096, dtype=np.uint32), np.arange(4096, dtype=np.uint32)[::-1].copy()
    tmp = torch.zeros(4096, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    D2D = 3

    def call(p, sp):
        src = p["in"]
        if stray == "read":                                     # the input read early, off the caller's stream
            assert hip.hipMemcpyAsync(tmp.data_ptr(), src, true.nbytes, D2D, None) == 0 and hip.hipStreamSynchronize(None) == 0
            src = tmp.data_ptr()
        if stray == "write":                                    # the output's first word cleared early, off the caller's stream
            assert hip.hipMemsetAsync(p["out"], 0, 8, None) == 0 and hip.hipStreamSynchronize(None) == 0
        rc = hip.hipMemcpyAsync(p["out"], src, true.nbytes, D2D, sp[0])
        return rc or hip.hipStreamSynchronize(sp[0])

    def check(got):
        assert np.array_equal(got["out"], true)
    entry = Entry(f"a copy, stray {stray}", {"in": (true, decoy)}, {"out": (true.shape, true.dtype)}, call, check)
    _streams(1)
    if stray is None:
        run_entry(native, entry)
    elif _CAL["free_streams"] == 0:
        warnings.warn("no stream runs beside the null stream: the harness cannot see a stray operation on stream 0 here")
    else:
        with pytest.raises(AssertionError, match="READ AFTER WRITE" if stray == "read" else "WRITE AFTER READ"):
            run_entry(native, entry)


# ----------------------------------------------------------------------------------------------------- the fixtures
class _Ix:
    pass


@pytest.fixture(scope="module")
def ix(native, oracle, tmp_path_factory):
    """the fixture of tests/test_range_search_abi.py (3000 uniform points of dimension 8 under ids 0 .. n - 1, DistL2, M = 8, built by
    the oracle; 300 queries: 18 tiles of 16 and a part, four wavefronts and a part; radii from the distance quantiles), loaded by the
    product and uploaded.  Ids are 0 .. n - 1: row, DataId and position (the ascending-id order) are one number.  Every point's p_id
    comes from the host-side graph walk, its dump position from the DataMap: no device call."""
    o, X, Q, radii = fixture()
    tmp = tmp_path_factory.mktemp("stream_order")
    o.file_dump(str(tmp), "s")
    x = _Ix()
    x.o, x.X, x.Q, x.radii, x.n, x.nq, x.d, x.metric = o, X, Q, radii, len(X), len(Q), X.shape[1], "DistL2"
    x.h = native.HnswIo(str(tmp), "s").load_hnsw("DistL2")
    x.h.upload(0)
    _pids(x)
    x.ids_dump = np.asarray(native.DataMap.from_hnswdump(str(tmp), "s").get_dataid_iter(), np.uint64)
    x.pos = np.empty(x.n, np.int64)
    x.pos[x.ids_dump.astype(np.int64)] = np.arange(x.n)          # dump position of row (= id) r
    rng = np.random.default_rng(5)
    x.allowed = np.sort(rng.choice(x.n, 900, replace=False)).astype(np.uint64)
    x.allowed_decoy = np.sort(rng.choice(x.n, 900, replace=False)).astype(np.uint64)
    # three filters of a set (half, a tenth, a hundredth of the ids), every query naming its own; the decoy: the same offsets over other
    # ids, filter_of rotated (still below n_filters)
    x.filters = [np.sort(rng.choice(x.n, m, replace=False)).astype(np.uint64) for m in (1500, 300, 30)]
    x.filters_decoy = [np.sort(rng.choice(x.n, m, replace=False)).astype(np.uint64) for m in (1500, 300, 30)]
    x.filter_offsets = np.concatenate([[0], np.cumsum([len(f) for f in x.filters])]).astype(np.uint64)
    x.filter_of = (np.arange(x.nq) % 3).astype(np.uint32)
    x.filter_of_decoy = ((np.arange(x.nq) + 1) % 3).astype(np.uint32)
    x.points = rng.choice(x.n, 300, replace=True).astype(np.uint64)          # (with repetitions: every occurrence has its own row)
    x.points_decoy = rng.choice(x.n, 300, replace=True).astype(np.uint64)
    x.radii_decoy = np.roll(radii, 3)                            # permuted: finite, non-negative, another radius for every query
    assert np.isfinite(radii).all() and (radii >= 0).all() and (x.radii_decoy != radii).mean() > 0.5
    x._Dnn, x._graph = None, {}
    return x


def _pids(x):
    """layer[r], rank[r] and pids[r] of row r of an index whose ids are 0 .. n - 1, from the neighbour lists read on the host"""
    origin = F.GraphWalk(x.h).origin                             # p_id -> DataId
    assert sorted(origin.values()) == list(range(x.n))
    x.layer, x.rank = np.zeros(x.n, np.uint8), np.zeros(x.n, np.int32)
    for (l, r), i in origin.items():
        x.layer[i], x.rank[i] = l, r
    x.ids = np.arange(x.n, dtype=np.uint64)
    x.pids = list(zip(x.layer.tolist(), x.rank.tolist()))


def _Dnn(x, oracle):
    if x._Dnn is None:
        x._Dnn = oracle.dist_matrix(x.metric, x.X, x.X)
    return x._Dnn


def _res(got, rows, k):
    """the outputs of a k-NN entry as the object the suite's comparisons take"""
    return types.SimpleNamespace(ids=got["ids"].reshape(rows, k), dists=got["dists"].reshape(rows, k), layers=got["layers"].reshape(rows, k),
                                 ranks=got["ranks"].reshape(rows, k), counts=got["counts"])


def _knn_outs(rows, k, stats=False, tag=""):
    o = {tag + "ids": ((rows, k), np.uint64), tag + "dists": ((rows, k), np.float32), tag + "layers": ((rows, k), np.uint8),
         tag + "ranks": ((rows, k), np.int32), tag + "counts": ((rows,), np.uint32)}
    if stats:
        o[tag + "stats"] = ((rows, 8), np.uint32)
    return o


def _flat_filters(filters):
    return np.concatenate(filters)


# ----------------------------------------------------------------------------------------------------- 1. the search, four launch sequences
def _search_entry(native, h, Q, ref, k, ef, name):
    L = native.lib()
    nq, d = Q.shape

    def call(p, sp):
        return L.hnswgpu_search_batch_device(h.handle, p["q"], nq, d, k, ef, p["ids"], p["dists"], p["layers"], p["ranks"], p["counts"], p["stats"], sp[0])

    def check(got):
        assert_same(_res(got, nq, k), ref)
        assert_same_counters(got["stats"], ref, name)            # words 0, 1, 2 and word 7's descent share, as tests/test_gpu_counters.py
        assert set(np.unique(got["stats"][:, 3]).tolist()) <= {0, 3}, (name, "status", np.unique(got["stats"][:, 3]))
    return Entry(name, {"q": (Q, np.ascontiguousarray(Q[::-1]))}, _knn_outs(nq, k, stats=True), call, check)


def test_search_default_sequence(native, ix):
    ref = ix.o.parallel_search(ix.Q, K, EF, want_counters="per_query")
    run_entry(native, _search_entry(native, ix.h, ix.Q, ref, K, EF, "search_batch_device"))


def test_search_pair_first_pass(native, ix, knob, capfd):
    """HNSWGPU_PAIR_SEARCH forced on: two queries per wavefront read the queries first (601 queries: the pass needs 512, and the last
    wavefront's second half idles)"""
    Q = uniform(601, ix.d, 7)
    ref = ix.o.parallel_search(Q, K, EF, want_counters="per_query")
    knob("HNSWGPU_PAIR_SEARCH", "1")
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    run_entry(native, _search_entry(native, ix.h, Q, ref, K, EF, "search_batch_device, pair pass"))
    lines = _launch_lines(capfd)
    _report()
    assert sum("pair pass" in ln for ln in lines) == 3, lines    # the warm-up and the two cases


def test_search_literal_heap_kernel(native, ix, knob, capfd):
    """ef = 1100 > 1024: the literal-heap kernel answers"""
    ref = ix.o.parallel_search(ix.Q, K, 1100, want_counters="per_query")
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    run_entry(native, _search_entry(native, ix.h, ix.Q, ref, K, 1100, "search_batch_device, ef 1100"))
    lines = _launch_lines(capfd)
    _report()
    assert sum("literal kernel" in ln for ln in lines) >= 3, lines


def test_search_forced_relaunch(native, oracle, tmp_path, knob, capfd):
    """the index and the hooks of tests/test_gpu_relaunch.py: one bitmap slice and a first table of 2^b cells, b from the oracle's
    counters -- three launches, and the queries are read again by each of them"""
    o, h = _pair(native, oracle, str(tmp_path), _spread(4000, 16, 21), 16, 100, "DistL2", "rl")
    Q = np.ascontiguousarray(_spread(600, 16, 22)[:300])
    ref = o.parallel_search(Q, K, 64, want_counters="per_query")
    knob("HNSWGPU_HASH_BITS", _forced_bits(ref))
    knob("HNSWGPU_BITMAP_SLICES", 1)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    run_entry(native, _search_entry(native, h, Q, ref, K, 64, "search_batch_device, forced relaunch"))
    lines = [ln for ln in _launch_lines(capfd) if "visited set" in ln]
    _report()
    assert len(lines) == 9 and sum("visited set bitmap" in ln for ln in lines) == 3, lines   # three launches per call, the third on the bitmap


# ----------------------------------------------------------------------------------------------------- 2, 3. filtered searches
def test_search_filtered(native, ix):
    L = native.lib()
    ref = ix.o.parallel_search_filter(ix.Q, K, EF, ix.allowed, want_counters="per_query")
    panics = C.c_uint32(77)

    def call(p, sp):
        return L.hnswgpu_search_batch_filtered_device(ix.h.handle, p["q"], ix.nq, ix.d, K, EF, p["allowed"], len(ix.allowed), p["ids"], p["dists"],
                                                      p["layers"], p["ranks"], p["counts"], p["stats"], sp[0], C.byref(panics))

    def check(got):
        assert_same(_res(got, ix.nq, K), ref)
        assert_same_counters(got["stats"], ref, "filtered")
        assert panics.value == 0 and not (got["stats"][:, 3] == 6).any()
    run_entry(native, Entry("search_batch_filtered_device", {"q": (ix.Q, np.ascontiguousarray(ix.Q[::-1])), "allowed": (ix.allowed, ix.allowed_decoy)},
                            _knn_outs(ix.nq, K, stats=True), call, check))


def _set_ins(ix):
    """the inputs of a filter-set call but the offsets: the decoy set has the same offsets, so they are no decoy and stay put"""
    return {"q": (ix.Q, np.ascontiguousarray(ix.Q[::-1])), "f_ids": (_flat_filters(ix.filters), _flat_filters(ix.filters_decoy)),
            "f_of": (ix.filter_of, ix.filter_of_decoy)}


def test_search_filter_set(native, ix):
    L = native.lib()
    ref = _oracle_answers(ix.o, ix.Q, K, EF, ix.filters, ix.filter_of)
    panics = C.c_uint32(77)
    ins, off = _set_ins(ix), _dev_const(ix.filter_offsets)

    def call(p, sp):
        return L.hnswgpu_search_batch_filter_set_device(ix.h.handle, p["q"], ix.nq, ix.d, K, EF, p["f_ids"], off.data_ptr(), len(ix.filters), p["f_of"],
                                                        p["ids"], p["dists"], p["layers"], p["ranks"], p["counts"], p["stats"], sp[0], C.byref(panics))

    def check(got):
        a = _res(got, ix.nq, K)
        a.status = (got["stats"][:, 3] == 6).astype(np.uint8)
        _assert_equal(a, ref, "filter set")
        assert panics.value == int(ref.status.sum()) == 0
    run_entry(native, Entry("search_batch_filter_set_device", ins, _knn_outs(ix.nq, K, stats=True), call, check))


def _dev_const(a):
    import torch
    t = _dev(a)
    torch.cuda.synchronize()
    return t


# ----------------------------------------------------------------------------------------------------- 4. two tickets in flight
def test_ticket_pair_two_in_flight(native, ix):
    """two tickets on two streams, each behind its own delayed producer, with its own outputs; ended in reverse order"""
    L = native.lib()
    ref = ix.o.parallel_search(ix.Q, K, EF)
    half = {"a.": (0, 150), "b.": (150, 300)}

    def call(p, sp):
        tickets = []
        for i, (tag, (lo, hi)) in enumerate(half.items()):
            t = C.c_void_p()
            rc = L.hnswgpu_search_batch_device_begin(ix.h.handle, p[tag + "q"], hi - lo, ix.d, K, EF, p[tag + "ids"], p[tag + "dists"], p[tag + "layers"],
                                                     p[tag + "ranks"], p[tag + "counts"], p[tag + "stats"], sp[i], C.byref(t))
            assert rc == 0 and t.value, native._native.last_error()
            tickets.append(t)
        rcs = [L.hnswgpu_search_batch_end(t) for t in reversed(tickets)]
        return max(rcs)

    def check(got):
        for tag, (lo, hi) in half.items():
            part = types.SimpleNamespace(ids=ref.ids[lo:hi], dists=ref.dists[lo:hi], layers=ref.layers[lo:hi], ranks=ref.ranks[lo:hi], counts=ref.counts[lo:hi])
            assert_same(_res({k[len(tag):]: v for k, v in got.items() if k.startswith(tag)}, hi - lo, K), part)
            assert set(np.unique(got[tag + "stats"][:, 3]).tolist()) <= {0, 3}
    ins, outs, where = {}, {}, {}
    for i, (tag, (lo, hi)) in enumerate(half.items()):
        ins[tag + "q"] = (np.ascontiguousarray(ix.Q[lo:hi]), np.ascontiguousarray(ix.Q[lo:hi][::-1]))
        outs.update(_knn_outs(hi - lo, K, stats=True, tag=tag))
        where.update({name: i for name in list(outs) + [tag + "q"] if name.startswith(tag)})
    run_entry(native, Entry("search_batch_device_begin / _end", ins, outs, call, check, n_streams=2, where=where))


# ----------------------------------------------------------------------------------------------------- 5, 6. shards and their gather
SHARDS = (160, 0, 140)                                          # three shards on device 0, the middle one empty


def _shard_ptrs(p, names):
    return (C.c_void_p * 3)(*[p.get(name) for name in names])


def test_sharded_device(native, ix):
    L = native.lib()
    ref = ix.o.parallel_search(ix.Q, K, EF)
    bounds = np.cumsum((0,) + SHARDS)
    live = [s for s in range(3) if SHARDS[s]]

    def call(p, sp):
        arr = lambda what: _shard_ptrs(p, [f"{s}.{what}" for s in range(3)])   # noqa: E731  (NULL for the empty shard)
        return L.hnswgpu_search_batch_sharded_device(ix.h.handle, (C.c_int * 3)(0, 0, 0), 3, arr("q"), (C.c_uint64 * 3)(*SHARDS), ix.d, K, EF, arr("ids"),
                                                     arr("dists"), arr("layers"), arr("ranks"), arr("counts"), (C.c_void_p * 3)(*sp))

    def check(got):
        for s in live:
            lo, hi = bounds[s], bounds[s + 1]
            part = types.SimpleNamespace(ids=ref.ids[lo:hi], dists=ref.dists[lo:hi], layers=ref.layers[lo:hi], ranks=ref.ranks[lo:hi], counts=ref.counts[lo:hi])
            assert_same(_res({k[2:]: v for k, v in got.items() if k.startswith(f"{s}.")}, hi - lo, K), part)
    ins, outs, where = {}, {}, {}
    for s in live:
        rows = ix.Q[bounds[s]:bounds[s + 1]]
        ins[f"{s}.q"] = (np.ascontiguousarray(rows), np.ascontiguousarray(rows[::-1]))
        outs.update(_knn_outs(SHARDS[s], K, tag=f"{s}."))
        where.update({name: s for name in list(outs) + [f"{s}.q"] if name.startswith(f"{s}.")})
    run_entry(native, Entry("search_batch_sharded_device", ins, outs, call, check, n_streams=3, where=where))


def test_gather_sharded_answers(native, ix):
    """the per-shard answers are produced behind a delay on root_stream; the answer is their concatenation in shard order"""
    L = native.lib()
    rng = np.random.default_rng(9)
    kinds = {"ids": np.uint64, "dists": np.float32, "layers": np.uint8, "ranks": np.int32, "counts": np.uint32}
    live = [s for s in range(3) if SHARDS[s]]

    def answers():
        out = {}
        for s in live:
            for what, dtype in kinds.items():
                shape = (SHARDS[s],) if what == "counts" else (SHARDS[s], K)
                out[f"{s}.{what}"] = rng.random(shape, dtype=np.float32) if dtype is np.float32 else rng.integers(0, 200, shape).astype(dtype)
        return out
    true, decoy = answers(), answers()
    total = sum(SHARDS)

    def call(p, sp):
        arr = lambda what: _shard_ptrs(p, [f"{s}.{what}" for s in range(3)])   # noqa: E731
        return L.hnswgpu_gather_sharded_answers((C.c_int * 3)(0, 0, 0), 3, (C.c_uint64 * 3)(*SHARDS), K, arr("ids"), arr("dists"), arr("layers"), arr("ranks"),
                                                arr("counts"), 0, p["root.ids"], p["root.dists"], p["root.layers"], p["root.ranks"], p["root.counts"], sp[0])

    def check(got):
        for what in kinds:
            want = np.concatenate([true[f"{s}.{what}"] for s in live])
            assert got["root." + what].tobytes() == want.tobytes(), what
    run_entry(native, Entry("gather_sharded_answers", {k: (true[k], decoy[k]) for k in true}, _knn_outs(total, K, tag="root."), call, check))


# ----------------------------------------------------------------------------------------------------- 7, 8. exact k-NN
@pytest.fixture(scope="module")
def cosine(native):
    """the same points under DistCosine, built by the product's host builder (ids 0 .. n - 1): the prep kernel sums the query norms"""
    x = _Ix()
    x.X, x.n, x.metric = fixture()[1], 3000, "DistCosine"
    x.h = _build(native, x.X, "DistCosine")
    _pids(x)
    return x


@pytest.mark.parametrize("metric", ["DistL2", "DistCosine"])
@pytest.mark.parametrize("filtered", [False, True])
def test_exact_search(native, oracle, ix, cosine, metric, filtered):
    L = native.lib()
    x = ix if metric == "DistL2" else cosine
    Q, nq, d = ix.Q, ix.nq, ix.d
    allowed = ix.allowed if filtered else None

    def call(p, sp):
        return L.hnswgpu_exact_search_batch_device(x.h.handle, p["q"], nq, d, K, p.get("allowed"), len(allowed) if filtered else 0, p["ids"], p["dists"],
                                                   p["layers"], p["ranks"], p["counts"], sp[0])

    def check(got):
        res = _res(got, nq, K)
        _assert_answers(oracle, metric, res, Q, x.X, x.ids, K, rows=allowed.astype(np.int64) if filtered else None, what=f"{metric} filtered {filtered}")
        at = res.ids.astype(np.int64)                            # (the ids are the oracle's by now; ids are rows)
        assert np.array_equal(res.layers, x.layer[at]) and np.array_equal(res.ranks, x.rank[at]), "p_ids"
    ins = {"q": (Q, np.ascontiguousarray(Q[::-1]))}
    if filtered:
        ins["allowed"] = (ix.allowed, ix.allowed_decoy)
    run_entry(native, Entry(f"exact_search_batch_device, {metric}{', filter' if filtered else ''}", ins, _knn_outs(nq, K), call, check))


@pytest.mark.parametrize("groups", [1, 2])
def test_exact_search_filter_set(native, oracle, ix, knob, groups):
    """groups = 2: a bitmap of this index is 94 words = 376 bytes and HNSWGPU_FILTER_SET_MB = 0.00075 MiB = 786 bytes hold two (the
    construction of tests/test_gpu_exact_knn_filter_set.py, at this index's size): the three filters are two groups, and the group
    list kernels read filter_of again"""
    L = native.lib()
    if groups == 2:
        knob("HNSWGPU_FILTER_SET_MB", "0.00075")
    rows_of = [f.astype(np.int64) for f in ix.filters]
    ins, off = _set_ins(ix), _dev_const(ix.filter_offsets)

    def call(p, sp):
        return L.hnswgpu_exact_search_batch_filter_set_device(ix.h.handle, p["q"], ix.nq, ix.d, K, p["f_ids"], off.data_ptr(), len(ix.filters), p["f_of"],
                                                              p["ids"], p["dists"], p["layers"], p["ranks"], p["counts"], sp[0])

    def check(got):
        _assert_set(oracle, ix, _res(got, ix.nq, K), ix.Q, rows_of, ix.filter_of, K, f"exact filter set, groups {groups}")
    run_entry(native, Entry(f"exact_search_batch_filter_set_device, {groups} group(s)", ins, _knn_outs(ix.nq, K), call, check))


# ----------------------------------------------------------------------------------------------------- 9, 10. range searches
def _csr_outs(nq, cap, with_ef):
    o = {"offsets": ((nq + 1,), np.uint64), "ids": ((cap,), np.uint64), "dists": ((cap,), np.float32), "layers": ((cap,), np.uint8),
         "ranks": ((cap,), np.int32)}
    if with_ef:
        o.update(ef=((nq,), np.uint32), flags=((nq,), np.uint8))
    return o


def _untouched_behind(got, total):
    for what in ("ids", "dists", "layers", "ranks"):
        assert (got[what][total:].view(np.uint8) == SENTINEL).all(), (what, "written behind the total")


def test_exact_range_search(native, oracle, ix):
    """queries, radii and the filter all arrive late; cap = every eligible point for every query, so that no mix of true and decoy
    inputs can ask for more"""
    L = native.lib()
    D = oracle.dist_matrix(ix.metric, ix.Q, ix.X)
    cap = ix.nq * len(ix.allowed)

    def call(p, sp):
        return L.hnswgpu_exact_range_search_batch_device(ix.h.handle, p["q"], ix.nq, ix.d, p["radii"], p["allowed"], len(ix.allowed), cap, p["offsets"],
                                                         p["ids"], p["dists"], p["layers"], p["ranks"], sp[0])

    def check(got):
        total = int(got["offsets"][-1])
        assert total <= cap
        res = native.RangeResult(got["offsets"], got["ids"][:total], got["dists"][:total], got["layers"][:total], got["ranks"][:total])
        _assert_range(res, D, ix.ids, ix.radii, rows=ix.allowed.astype(np.int64), pids=ix.pids, what="exact range")
        _untouched_behind(got, total)
    ins = {"q": (ix.Q, np.ascontiguousarray(ix.Q[::-1])), "radii": (ix.radii, ix.radii_decoy), "allowed": (ix.allowed, ix.allowed_decoy)}
    run_entry(native, Entry("exact_range_search_batch_device", ins, _csr_outs(ix.nq, cap, False), call, check))


@pytest.mark.parametrize("filtered", [False, True])
def test_range_search(native, ix, filtered):
    """ef_first = 8, ef_max = 256: five rounds, a word read back per round; d_out_offsets[0] is cleared by a memset of its own"""
    L = native.lib()
    ef_first, ef_max = 8, 256
    if filtered:
        want = range_rule(lambda Q, k, ef: ix.o.parallel_search_filter(Q, k, ef, ix.allowed), ix.Q, ix.radii, ef_first, ef_max)
    else:
        want = fixture_expected(ef_first, ef_max)
    cap = ix.nq * ef_max

    def call(p, sp):
        return L.hnswgpu_range_search_batch_device(ix.h.handle, p["q"], ix.nq, ix.d, p["radii"], ef_first, ef_max, p.get("allowed"),
                                                   len(ix.allowed) if filtered else 0, cap, p["offsets"], p["ids"], p["dists"], p["layers"], p["ranks"],
                                                   p["ef"], p["flags"], sp[0])

    def check(got):
        total = int(got["offsets"][-1])
        assert total == int(want.offsets[-1]) <= cap
        res = native.RangeResult(got["offsets"], got["ids"][:total], got["dists"][:total], got["layers"][:total], got["ranks"][:total], got["ef"], got["flags"])
        _same_range(res, want, f"range search, filtered {filtered}")
        _untouched_behind(got, total)
    ins = {"q": (ix.Q, np.ascontiguousarray(ix.Q[::-1])), "radii": (ix.radii, ix.radii_decoy)}
    if filtered:
        ins["allowed"] = (ix.allowed, ix.allowed_decoy)
    run_entry(native, Entry(f"range_search_batch_device{', filter' if filtered else ''}", ins, _csr_outs(ix.nq, cap, True), call, check))


# ----------------------------------------------------------------------------------------------------- 11, 12. queries by stored point
def _rows_of_points(ix, point_ids):
    flat, unknown = resolve(ix.ids_dump, point_ids)
    assert unknown == 0                                         # true or decoy: every id names a point
    return ix.ids_dump[flat].astype(np.int64)                   # dump position -> id = row


def test_graph_search(native, ix):
    L = native.lib()
    np_ = len(ix.points)
    rows = _rows_of_points(ix, ix.points)
    _rows_of_points(ix, ix.points_decoy)
    wide = ix.o.parallel_search(np.ascontiguousarray(ix.X[rows]), K + 1, 32)
    want = apply_drop_self(wide, [ix.pids[r] for r in rows], K)

    def call(p, sp):
        return L.hnswgpu_graph_search_batch_device(ix.h.handle, p["points"], np_, K, 32, p["ids"], p["dists"], p["layers"], p["ranks"], p["counts"], sp[0])

    def check(got):
        _assert_rows(_res(got, np_, K), want, "graph search")
    run_entry(native, Entry("graph_search_batch_device", {"points": (ix.points, ix.points_decoy)}, _knn_outs(np_, K), call, check))


def test_exact_graph(native, oracle, ix):
    L = native.lib()
    np_ = len(ix.points)
    rows = _rows_of_points(ix, ix.points)
    _rows_of_points(ix, ix.points_decoy)
    want = _exact_expected(_Dnn(ix, oracle), ix.ids, ix.pos, ix.pids, rows, K, ix.allowed.astype(np.int64))

    def call(p, sp):
        return L.hnswgpu_exact_graph_batch_device(ix.h.handle, p["points"], np_, K, p["allowed"], len(ix.allowed), p["ids"], p["dists"], p["layers"],
                                                  p["ranks"], p["counts"], sp[0])

    def check(got):
        _assert_rows(_res(got, np_, K), want, "exact graph")
    run_entry(native, Entry("exact_graph_batch_device", {"points": (ix.points, ix.points_decoy), "allowed": (ix.allowed, ix.allowed_decoy)},
                            _knn_outs(np_, K), call, check))


# ----------------------------------------------------------------------------------------------------- 13, 14, 15. CSR graphs and forests
N_CSR, TOTAL_CSR = 5000, 20000


def _random_csr(seed):
    """n = 5000 rows of ragged lengths that add up to 20000 entries, every col below n, weights in [0, 1): two seeds give two graphs
    with different offsets and the same offsets[n], so every grid an entry sizes from the total stays right"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(rng.multinomial(TOTAL_CSR, np.full(N_CSR, 1.0 / N_CSR)))]).astype(np.uint64)
    return offsets, rng.integers(0, N_CSR, TOTAL_CSR).astype(np.uint32), rng.random(TOTAL_CSR, dtype=np.float32)


def _csr_ins():
    (o1, c1, d1), (o2, c2, d2) = _random_csr(1), _random_csr(2)
    assert int(o1[-1]) == int(o2[-1]) == TOTAL_CSR and not np.array_equal(o1, o2)
    return (o1, c1, d1), {"offsets": (o1, o2), "cols": (c1, c2), "dists": (d1, d2)}


def _csr_forest_want(offsets, cols, dists):
    rows = np.repeat(np.arange(N_CSR, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    return spanning_forest(N_CSR, zip(rows.tolist(), cols.tolist(), dists.tolist()))


def test_csr_components(native):
    L = native.lib()
    (offsets, cols, dists), ins = _csr_ins()
    cut = np.array([0.5], np.float32)
    want_lab, want_sizes = components(N_CSR, csr_edges(offsets, cols, dists, 0.5))
    decoy_lab, _ = components(N_CSR, csr_edges(ins["offsets"][1], ins["cols"][1], ins["dists"][1], 0.5))
    assert not np.array_equal(want_lab, decoy_lab) and 1 < len(want_sizes) < N_CSR
    c = np.zeros(1, np.uint64)

    def call(p, sp):
        c[0] = 0x7777
        return L.hnswgpu_csr_components_device(0, N_CSR, p["offsets"], p["cols"], p["dists"], cut.ctypes.data, p["label"], p["sizes"], c.ctypes.data, sp[0])

    def check(got):
        n_c = len(want_sizes)
        assert int(c[0]) == n_c
        assert np.array_equal(got["label"], want_lab) and np.array_equal(got["sizes"][:n_c], want_sizes)
        assert (got["sizes"][n_c:].view(np.uint8) == SENTINEL).all()
    run_entry(native, Entry("csr_components_device", ins, {"label": ((N_CSR,), np.uint32), "sizes": ((N_CSR,), np.uint32)}, call, check))


def _forest_outs():
    return {"a": ((N_CSR - 1,), np.uint32), "b": ((N_CSR - 1,), np.uint32), "w": ((N_CSR - 1,), np.float32)}


def _check_forest(got, want, m, what=""):
    a, b, w = want
    assert m == len(a), (what, m, len(a))
    assert np.array_equal(got["a"][:m], a) and np.array_equal(got["b"][:m], b), (what, "ends")
    assert np.array_equal(got["w"][:m].view(np.uint32), w.view(np.uint32)), (what, "weights")
    for x in ("a", "b", "w"):
        assert (got[x][m:].view(np.uint8) == SENTINEL).all(), (what, x, "written behind the edges")


def test_csr_spanning_forest(native):
    L = native.lib()
    (offsets, cols, dists), ins = _csr_ins()
    want = _csr_forest_want(offsets, cols, dists)
    m = np.zeros(1, np.uint64)

    def call(p, sp):
        m[0] = 0x7777
        return L.hnswgpu_csr_spanning_forest_device(0, N_CSR, p["offsets"], p["cols"], p["dists"], p["a"], p["b"], p["w"], m.ctypes.data, sp[0])
    run_entry(native, Entry("csr_spanning_forest_device", ins, _forest_outs(), call, lambda got: _check_forest(got, want, int(m[0]), "csr forest")))


def _dendrogram_outs(slots):
    return {"left": ((slots,), np.uint32), "right": ((slots,), np.uint32), "size": ((slots,), np.uint32)}


def _check_dendrogram(got, want, m, what=""):
    for x, w in zip(("left", "right", "size"), want):
        assert len(w) == m and np.array_equal(got[x][:m], w), (what, x)
        assert (got[x][m:].view(np.uint8) == SENTINEL).all(), (what, x, "written behind the merges")


def test_forest_dendrogram(native):
    """two random forests over the same 5000 vertices, cut to the same number of edges (a prefix of a forest is a forest)"""
    L = native.lib()
    f1, f2 = random_forest(N_CSR, np.random.default_rng(11)), random_forest(N_CSR, np.random.default_rng(12))
    m = min(len(f1), len(f2))
    f1, f2 = f1[:m], f2[:m]
    a1, b1, a2, b2 = (np.ascontiguousarray(x.astype(np.uint32)) for x in (f1[:, 0], f1[:, 1], f2[:, 0], f2[:, 1]))
    want = dendrogram(N_CSR, f1)
    assert want is not None and dendrogram(N_CSR, f2) is not None

    def call(p, sp):
        return L.hnswgpu_forest_dendrogram_device(0, N_CSR, m, p["a"], p["b"], p["left"], p["right"], p["size"], sp[0])
    run_entry(native, Entry("forest_dendrogram_device", {"a": (a1, a2), "b": (b1, b2)}, _dendrogram_outs(m + 3), call,
                            lambda got: _check_dendrogram(got, want, m, "dendrogram")))


def test_pipeline_forest_then_dendrogram_on_one_stream(native):
    """as a caller would: a delayed producer of a CSR graph, hnswgpu_csr_spanning_forest_device, its device outputs straight into
    hnswgpu_forest_dendrogram_device -- no host wait of the test's own between the two calls"""
    L = native.lib()
    (offsets, cols, dists), ins = _csr_ins()
    want_forest = _csr_forest_want(offsets, cols, dists)
    want = dendrogram(N_CSR, zip(want_forest[0].tolist(), want_forest[1].tolist()))
    m = np.zeros(1, np.uint64)

    def call(p, sp):
        m[0] = 0x7777
        rc = L.hnswgpu_csr_spanning_forest_device(0, N_CSR, p["offsets"], p["cols"], p["dists"], p["a"], p["b"], p["w"], m.ctypes.data, sp[0])
        if rc != 0:
            return rc
        return L.hnswgpu_forest_dendrogram_device(0, N_CSR, int(m[0]), p["a"], p["b"], p["left"], p["right"], p["size"], sp[0])

    def check(got):
        _check_forest(got, want_forest, int(m[0]), "pipeline forest")
        _check_dendrogram(got, want, int(m[0]), "pipeline dendrogram")
    outs = _forest_outs()
    outs.update(_dendrogram_outs(N_CSR - 1))
    run_entry(native, Entry("csr_spanning_forest_device -> forest_dendrogram_device", ins, outs, call, check))


# ----------------------------------------------------------------------------------------------------- 16. the four index entries
GRAPH_K = 5
GRAPH_MODES = [(0, "union"), (32, "mutual")]                    # ef = 0: the exact graph; ef = 32: the graph search
MODE_CODE = {"union": 0, "mutual": 1}


def _graph(ix, oracle, ef):
    """the directed graph D of every point from the models: (counts, neighbour positions, dists) -- positions are ids here"""
    if ef not in ix._graph:
        rows = np.arange(ix.n)
        if ef == 0:
            ids, dists, _, _, counts = _exact_expected(_Dnn(ix, oracle), ix.ids, ix.pos, ix.pids, rows, GRAPH_K)
        else:
            wide = ix.o.parallel_search(ix.X, GRAPH_K + 1, ef)
            ids, dists, _, _, counts, _ = apply_drop_self(wide, ix.pids, GRAPH_K)
        ix._graph[ef] = (counts, ids.astype(np.int64), dists)
    return ix._graph[ef]


@pytest.mark.parametrize("ef,mode", GRAPH_MODES)
def test_symmetric_graph(native, oracle, ix, ef, mode):
    L = native.lib()
    offsets, cols, bits, _, _ = symmetrise(ix.n, *_graph(ix, oracle, ef), mode)
    total = int(offsets[-1])
    cap = total + 5
    at = cols.astype(np.int64)

    def call(p, sp):
        return L.hnswgpu_symmetric_graph_device(ix.h.handle, GRAPH_K, ef, MODE_CODE[mode], cap, p["offsets"], p["pos"], p["ids"], p["dists"], p["layers"],
                                                p["ranks"], sp[0])

    def check(got):
        assert np.array_equal(got["offsets"], offsets)
        assert np.array_equal(got["pos"][:total], cols) and np.array_equal(got["ids"][:total], ix.ids[at])
        assert np.array_equal(got["dists"][:total].view(np.uint32), bits)
        assert np.array_equal(got["layers"][:total], ix.layer[at]) and np.array_equal(got["ranks"][:total], ix.rank[at])
        _untouched_behind(got, total)
        assert (got["pos"][total:].view(np.uint8) == SENTINEL).all()
    outs = _csr_outs(ix.n, cap, False)
    outs["pos"] = ((cap,), np.uint32)
    run_entry(native, Entry(f"symmetric_graph_device, ef {ef} {mode}", {}, outs, call, check))


@pytest.mark.parametrize("ef,mode", GRAPH_MODES)
def test_graph_components(native, oracle, ix, ef, mode):
    L = native.lib()
    counts, pos, dists = _graph(ix, oracle, ef)
    cut = np.array([np.median(dists[:, 0])], np.float32)         # half of the nearest-neighbour edges survive: many components
    want_lab, want_sizes = cut_and_join(ix.n, counts, pos, dists, mode, cut[0])
    assert 1 < len(want_sizes) < ix.n
    c = np.zeros(1, np.uint64)

    def call(p, sp):
        c[0] = 0x7777
        return L.hnswgpu_graph_components_device(ix.h.handle, GRAPH_K, ef, MODE_CODE[mode], cut.ctypes.data, p["label"], p["sizes"], c.ctypes.data, sp[0])

    def check(got):
        n_c = len(want_sizes)
        assert int(c[0]) == n_c and np.array_equal(got["label"], want_lab) and np.array_equal(got["sizes"][:n_c], want_sizes)
        assert (got["sizes"][n_c:].view(np.uint8) == SENTINEL).all()
    run_entry(native, Entry(f"graph_components_device, ef {ef} {mode}", {}, {"label": ((ix.n,), np.uint32), "sizes": ((ix.n,), np.uint32)}, call, check))


def _index_forest_want(ix, oracle, ef, mode):
    counts, pos, dists = _graph(ix, oracle, ef)
    return spanning_forest(ix.n, pair_weights(ix.n, counts, pos, dists, mode))


@pytest.mark.parametrize("ef,mode", GRAPH_MODES)
def test_graph_spanning_forest(native, oracle, ix, ef, mode):
    L = native.lib()
    want = _index_forest_want(ix, oracle, ef, mode)
    m = np.zeros(1, np.uint64)

    def call(p, sp):
        m[0] = 0x7777
        return L.hnswgpu_graph_spanning_forest_device(ix.h.handle, GRAPH_K, ef, MODE_CODE[mode], 0, p["a"], p["b"], p["w"], m.ctypes.data, sp[0])
    outs = {k: ((ix.n - 1,), t) for k, (_, t) in _forest_outs().items()}
    run_entry(native, Entry(f"graph_spanning_forest_device, ef {ef} {mode}", {}, outs, call, lambda got: _check_forest(got, want, int(m[0]), "index forest")))


@pytest.mark.parametrize("ef,mode", GRAPH_MODES)
def test_graph_dendrogram(native, oracle, ix, ef, mode):
    L = native.lib()
    want_forest = _index_forest_want(ix, oracle, ef, mode)
    want = dendrogram(ix.n, zip(want_forest[0].tolist(), want_forest[1].tolist()))
    m = np.zeros(1, np.uint64)

    def call(p, sp):
        m[0] = 0x7777
        return L.hnswgpu_graph_dendrogram_device(ix.h.handle, GRAPH_K, ef, MODE_CODE[mode], 0, p["a"], p["b"], p["w"], p["left"], p["right"], p["size"],
                                                 m.ctypes.data, sp[0])

    def check(got):
        _check_forest(got, want_forest, int(m[0]), "index dendrogram, forest")
        _check_dendrogram(got, want, int(m[0]), "index dendrogram")
    outs = {k: ((ix.n - 1,), t) for k, (_, t) in _forest_outs().items()}
    outs.update(_dendrogram_outs(ix.n - 1))
    run_entry(native, Entry(f"graph_dendrogram_device, ef {ef} {mode}", {}, outs, call, check))
