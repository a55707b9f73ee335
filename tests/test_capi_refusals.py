"""What the batched C entries answer BEFORE a device is touched, pinned to the letter: the exact return code, the complete
hnswgpu_last_error() text and the exact bytes of every output array, for the eight host / _device pairs behind the filter-set search,
the exact k-NN (plain and under a filter set), the exact range search, the two stored-point graph calls, the approximate range search
and the symmetrised graph, plus hnswgpu_search_batch_filtered(_device); and for the eight pairs behind the components, the spanning
forest, the dendrogram and HDBSCAN (hnswhdb_*), each of an index and of a graph or forest the caller hands in.  The other ABI tests look
for a word of the message; this table is what keeps the one body a pair has in capi.cpp, the argument checks the bodies share and the
order they fire in from drifting.

Every case returns before the HIP runtime is asked anything, so the answers are the same with and without a GPU.  CPU only.  (That is
also why a _device form has no row with a bad array of its own: it does not read the array, its kernels do, and the rows of the host
form's "host_only_" checks are one-sided for that reason.  The GPU tests of each unit hold the device side of those.)"""
import ctypes as C

import numpy as np
import pytest

NOT_RESIDENT = "index is not resident on a device: call hnswgpu_upload first"
F16_TAIL = " reads f32 rows only: the index is set to HNSWGPU_STORAGE_F16 (hnswgpu_set_storage(idx, HNSWGPU_STORAGE_F32) first)"
GATHER = "the graph search (its gather kernel copies stored rows)"
SORTED = "the id vector of a filter must be sorted ascending"
DIM = "query dimension differs from the index dimension"
OFFSETS = "null out_offsets: the offsets are written by every call"
CAP = "cap > 0 with null out_ids or out_dists (the count-only call is cap == 0)"
SIMD8_TAIL = " answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8"
NO_FILTERS = "a filter set without filters: n_filters is 0 (an unfiltered batch is "

IN_DTYPES = {"queries": np.float32, "radii": np.float32, "allowed_ids": np.uint64, "filter_ids": np.uint64, "filter_offsets": np.uint64,
             "filter_of": np.uint32, "point_ids": np.uint64, "max_dist": np.float32, "offsets": np.uint64, "cols": np.uint32, "dists": np.float32,
             "a": np.uint32, "b": np.uint32, "w": np.float32}
OUTS = ("out_ids", "out_dists", "out_layer", "out_rank", "out_counts", "out_status", "out_offsets", "out_ef", "out_flags", "out_pos", "n_panics",
        "out_label", "out_sizes", "out_n_components", "out_a", "out_b", "out_w", "out_n_edges", "out_left", "out_right", "out_size", "out_labels",
        "out_prob", "out_point_cluster", "out_point_w", "out_cluster_parent", "out_cluster_birth_w", "out_cluster_size", "out_stability",
        "out_selected", "out_n_clusters", "out_n_labels")
SENTINEL, OUT_BYTES = 0x5A, 512
# a well-formed call on the 50 x 8 index: 3 queries (or points), knbn 4, two filters {1, 5, 9} and {2, 3}
DEFAULTS = dict(queries=np.linspace(0, 1, 24), nq=3, d=8, k=4, ef=16, radii=[0.5, 0.5, 0.5], allowed_ids=None, n_allowed=0,
                filter_ids=[1, 5, 9, 2, 3], filter_offsets=[0, 3, 5], n_filters=2, filter_of=[0, 1, 0], point_ids=[0, 1, 2], np=3,
                ef_first=4, ef_max=16, cap=16, mode=0, stats=None, stream=None,
                # ... and for the entries that take a graph or a forest of their own: the path 0 - 1 - 2 - 3, in CSR and as an edge list
                device=0, n=4, m=3, offsets=[0, 1, 3, 5, 6], cols=[1, 0, 2, 1, 3, 2], dists=[.25, .25, .5, .5, .75, .75], max_dist=None,
                a=[0, 1, 2], b=[1, 2, 3], w=[.25, .5, .75], core_k=0, min_cluster_size=2, method=0)

CASES = []


def case(base, forms, label, rc, msg, state="plain", zero=None, **kw):
    """one row per form of the pair: "h" the host-buffer entry, "d" its _device form.  zero: {output: leading bytes that are 0
    afterwards}; every other byte of every output keeps its sentinel.  msg None: the call succeeds (the message is not its to set)."""
    for form in forms:
        name = base + ("_device" if form == "d" else "")
        CASES.append(pytest.param(name, state, kw, rc, msg, zero or {}, id="%s-%s-%s" % (name[8:], state, label)))


# ------------------------------------------------------------------------- hnswgpu_search_batch_filtered(_device)
B = "hnswgpu_search_batch_filtered"
case(B, "h", "null_handle", "ERR_ARG", "null argument", idx=None)
case(B, "d", "null_handle", "ERR_ARG", "null argument", idx=None, zero={"n_panics": 4})
case(B, "hd", "null_filter", "ERR_ARG", "null filter", n_allowed=2)
case(B, "h", "unsorted", "ERR_ARG", SORTED, allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted+null_handle", "ERR_ARG", SORTED, idx=None, allowed_ids=[5, 3], n_allowed=2)
case(B, "hd", "null_filter+null_handle", "ERR_ARG", "null filter", idx=None, n_allowed=2)
case(B, "h", "answers_nothing", "OK", None, state="empty", zero={"out_counts": 12, "out_status": 3})
case(B, "h", "no_query", "OK", None, state="empty", nq=0)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, zero={"n_panics": 4})
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="empty", zero={"n_panics": 4})

# ------------------------------------------------- the two filter-set pairs: what can be checked without reading the set
for B, sib, exact in (("hnswgpu_search_batch_filter_set", "hnswgpu_search_batch", False),
                      ("hnswgpu_exact_search_batch_filter_set", "hnswgpu_exact_search_batch", True)):
    for form, zp in (("h", {}), ("d", {} if exact else {"n_panics": 4})):   # the search's device form zeroes *n_panics first
        case(B, form, "null_handle", "ERR_ARG", "null argument", idx=None, zero=zp)
        for buf in ("queries", "out_ids", "out_dists", "out_counts"):
            case(B, form, "null_" + buf, "ERR_ARG", "null buffer", zero=zp, **{buf: None})
        case(B, form, "null_filter_of", "ERR_ARG", "null filter_of: every query names its filter", filter_of=None, zero=zp)
        case(B, form, "null_filter_offsets", "ERR_ARG", "null filter_offsets", filter_offsets=None, zero=zp)
        case(B, form, "too_many_filters", "ERR_ARG", "too many filters: filter_of is 32 bits wide", n_filters=1 << 32, zero=zp)
        case(B, form, "null_handle+null_queries", "ERR_ARG", "null argument", idx=None, queries=None, zero=zp)
        case(B, form, "null_queries+no_filters", "ERR_ARG", "null buffer", queries=None, n_filters=0, zero=zp)
        case(B, form, "no_filters+null_filter_of", "ERR_ARG", "null filter_of: every query names its filter", n_filters=0, filter_of=None, zero=zp)
        case(B, form, "no_filters+too_many_k", "ERR_ARG", NO_FILTERS + sib + ("_device)" if form == "d" else ")"), n_filters=0, k=4097, zero=zp)
        case(B, form, "no_query", "OK", None, nq=0, zero=zp)
        case(B, form, "no_query_no_buffers", "OK", None, nq=0, n_filters=0, queries=None, filter_ids=None, filter_offsets=None, filter_of=None,
             out_ids=None, out_dists=None, out_counts=None, zero=zp)
    case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, zero={} if exact else {"n_panics": 4})
    case(B, "d", "never_uploaded_unread_set", "ERR_DEVICE", NOT_RESIDENT, filter_offsets=[1, 3, 2], filter_of=[7, 7, 7],
         zero={} if exact else {"n_panics": 4})
    # ... and what only the host entry can: the set itself
    case(B, "h", "offsets_start", "ERR_ARG", "filter_offsets must start at 0", filter_offsets=[1, 3, 5])
    case(B, "h", "offsets_descend", "ERR_ARG", "filter_offsets must ascend: filter_offsets[2] is below its predecessor", filter_offsets=[0, 3, 2])
    case(B, "h", "null_filter_ids", "ERR_ARG", "null filter_ids", filter_ids=None)
    case(B, "h", "unsorted_filter", "ERR_ARG", "the id vector of filter 1 is not sorted ascending", filter_ids=[1, 5, 9, 3, 2])
    case(B, "h", "filter_of_range", "ERR_ARG", "filter_of[1] = 2 names no filter (n_filters = 2)", filter_of=[0, 2, 0])
    case(B, "h", "offsets_start+filter_of_range", "ERR_ARG", "filter_offsets must start at 0", filter_offsets=[1, 3, 5], filter_of=[0, 2, 0])
    case(B, "h", "unsorted_filter+filter_of_range", "ERR_ARG", "the id vector of filter 1 is not sorted ascending", filter_ids=[1, 5, 9, 3, 2],
         filter_of=[9, 0, 0])
    case(B, "h", "empty_filters_need_no_ids", "OK", None, state="empty", filter_ids=None, filter_offsets=[0, 0, 0],
         zero={"out_counts": 12, "out_ids": 96, "out_dists": 48, "out_layer": 12, "out_rank": 48} if exact else {"out_counts": 12, "out_status": 3})
    case(B, "h", "no_query", "OK", None, state="empty", nq=0)
case("hnswgpu_search_batch_filter_set", "h", "no_filters", "ERR_ARG",
     "a filter set without filters: n_filters is 0 (an unfiltered batch is hnswgpu_search_batch)", n_filters=0)
case("hnswgpu_search_batch_filter_set", "d", "no_filters", "ERR_ARG",
     "a filter set without filters: n_filters is 0 (an unfiltered batch is hnswgpu_search_batch_device)", n_filters=0, zero={"n_panics": 4})
case("hnswgpu_search_batch_filter_set", "h", "answers_nothing", "OK", None, state="empty", zero={"out_counts": 12, "out_status": 3})
case("hnswgpu_search_batch_filter_set", "h", "answers_nothing_no_status", "OK", None, state="empty", out_status=None, zero={"out_counts": 12})

B = "hnswgpu_exact_search_batch_filter_set"
case(B, "h", "no_filters", "ERR_ARG", "a filter set without filters: n_filters is 0 (an unfiltered batch is hnswgpu_exact_search_batch)", n_filters=0)
case(B, "d", "no_filters", "ERR_ARG", "a filter set without filters: n_filters is 0 (an unfiltered batch is hnswgpu_exact_search_batch_device)",
     n_filters=0)
case(B, "hd", "k_0", "ERR_ARG", "knbn must be > 0", k=0)
case(B, "hd", "k_4097", "ERR_ARG", "exact search: knbn above 4096", k=4097)
case(B, "hd", "wrong_d", "ERR_ARG", DIM, d=7)
case(B, "hd", "simd8", "ERR_ARG", "exact search" + SIMD8_TAIL, state="simd8")
case(B, "hd", "f16", "ERR_ARG", "exact search" + F16_TAIL, state="f16")
case(B, "hd", "k_0+wrong_d", "ERR_ARG", "knbn must be > 0", k=0, d=7)
case(B, "hd", "wrong_d+simd8", "ERR_ARG", DIM, state="simd8", d=7)
case(B, "hd", "k_0+no_query", "ERR_ARG", "knbn must be > 0", k=0, nq=0)
case(B, "h", "unsorted_filter+k_0", "ERR_ARG", "the id vector of filter 1 is not sorted ascending", filter_ids=[1, 5, 9, 3, 2], k=0)
case(B, "h", "k_0", "ERR_ARG", "knbn must be > 0", state="empty", k=0)
case(B, "h", "answers_nothing", "OK", None, state="empty", d=7,
     zero={"out_counts": 12, "out_ids": 96, "out_dists": 48, "out_layer": 12, "out_rank": 48})
case(B, "h", "answers_nothing_no_layer_rank", "OK", None, state="empty", out_layer=None, out_rank=None,
     zero={"out_counts": 12, "out_ids": 96, "out_dists": 48})

# ------------------------------------------------------------------------------- hnswgpu_exact_search_batch(_device)
B = "hnswgpu_exact_search_batch"
case(B, "hd", "null_handle", "ERR_ARG", "null argument", idx=None)
for buf in ("queries", "out_ids", "out_dists", "out_counts"):
    case(B, "hd", "null_" + buf, "ERR_ARG", "null buffer", **{buf: None})
case(B, "hd", "k_0", "ERR_ARG", "knbn must be > 0", k=0)
case(B, "hd", "k_4097", "ERR_ARG", "exact search: knbn above 4096", k=4097)
case(B, "hd", "wrong_d", "ERR_ARG", DIM, d=7)
case(B, "hd", "null_filter", "ERR_ARG", "null filter", n_allowed=2)
case(B, "hd", "simd8", "ERR_ARG", "exact search" + SIMD8_TAIL, state="simd8")
case(B, "hd", "f16", "ERR_ARG", "exact search" + F16_TAIL, state="f16")
case(B, "hd", "k_0+wrong_d", "ERR_ARG", "knbn must be > 0", k=0, d=7)
case(B, "hd", "null_buffer+k_0", "ERR_ARG", "null buffer", out_dists=None, k=0)
case(B, "hd", "wrong_d+null_filter", "ERR_ARG", DIM, d=7, n_allowed=2)
case(B, "hd", "null_filter+simd8", "ERR_ARG", "null filter", state="simd8", n_allowed=2)
case(B, "h", "unsorted", "ERR_ARG", SORTED, allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted+simd8", "ERR_ARG", "exact search" + SIMD8_TAIL, state="simd8", allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted", "ERR_ARG", SORTED, state="empty", allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "answers_nothing", "OK", None, state="empty", d=7,
     zero={"out_counts": 12, "out_ids": 96, "out_dists": 48, "out_layer": 12, "out_rank": 48})
case(B, "h", "answers_nothing_no_layer_rank", "OK", None, state="empty", out_layer=None, out_rank=None,
     zero={"out_counts": 12, "out_ids": 96, "out_dists": 48})
case(B, "h", "no_query", "OK", None, state="empty", nq=0)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT)
case(B, "d", "never_uploaded_no_query", "ERR_DEVICE", NOT_RESIDENT, nq=0)
case(B, "d", "never_uploaded_unread_filter", "ERR_DEVICE", NOT_RESIDENT, allowed_ids=[5, 3], n_allowed=2)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="empty")

# ------------------------------------------------------------------------- hnswgpu_exact_range_search_batch(_device)
B = "hnswgpu_exact_range_search_batch"
case(B, "hd", "null_handle", "ERR_ARG", "null argument", idx=None)
case(B, "hd", "null_out_offsets", "ERR_ARG", OFFSETS, out_offsets=None)
case(B, "hd", "null_queries", "ERR_ARG", "null queries", queries=None)
case(B, "hd", "null_radii", "ERR_ARG", "null radii: every query names its radius", radii=None)
case(B, "hd", "cap_null_out_ids", "ERR_ARG", CAP, out_ids=None)
case(B, "hd", "cap_null_out_dists", "ERR_ARG", CAP, out_dists=None)
case(B, "hd", "wrong_d", "ERR_ARG", DIM, d=7)
case(B, "hd", "null_filter", "ERR_ARG", "null filter", n_allowed=2)
case(B, "hd", "simd8", "ERR_ARG", "exact range search" + SIMD8_TAIL, state="simd8")
case(B, "hd", "f16", "ERR_ARG", "exact range search" + F16_TAIL, state="f16")
case(B, "hd", "null_out_offsets+wrong_d", "ERR_ARG", OFFSETS, out_offsets=None, d=7)
case(B, "hd", "wrong_d+simd8", "ERR_ARG", DIM, state="simd8", d=7)
case(B, "hd", "cap+null_filter", "ERR_ARG", CAP, out_ids=None, n_allowed=2)
case(B, "h", "unsorted", "ERR_ARG", SORTED, allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted+simd8", "ERR_ARG", "exact range search" + SIMD8_TAIL, state="simd8", allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "answers_nothing", "OK", None, state="empty", zero={"out_offsets": 32})
case(B, "h", "count_only_answers_nothing", "OK", None, state="empty", cap=0, out_ids=None, out_dists=None, zero={"out_offsets": 32})
case(B, "h", "no_query", "OK", None, nq=0, zero={"out_offsets": 8})
case(B, "h", "no_query", "OK", None, state="empty", nq=0, queries=None, radii=None, zero={"out_offsets": 8})
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT)
case(B, "d", "never_uploaded_no_query", "ERR_DEVICE", NOT_RESIDENT, nq=0)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="empty")

# --------------------------------------------------- hnswgpu_graph_search_batch(_device), hnswgpu_exact_graph_batch(_device)
for B, exact in (("hnswgpu_graph_search_batch", False), ("hnswgpu_exact_graph_batch", True)):
    case(B, "hd", "null_handle", "ERR_ARG", "null argument", idx=None)
    for buf in ("out_ids", "out_dists", "out_counts"):
        case(B, "hd", "null_" + buf, "ERR_ARG", "null buffer", **{buf: None})
    case(B, "hd", "every_point_np", "ERR_ARG", "point_ids is NULL (every point): np must be nb_point = 50, not 3", point_ids=None)
    case(B, "hd", "every_point_np", "ERR_ARG", "point_ids is NULL (every point): np must be nb_point = 0, not 3", state="empty", point_ids=None)
    case(B, "hd", "k_0", "ERR_ARG", "knbn must be > 0", k=0)
    case(B, "hd", "null_buffer+k_0", "ERR_ARG", "null buffer", out_counts=None, k=0)
    case(B, "hd", "every_point_np+k_0", "ERR_ARG", "point_ids is NULL (every point): np must be nb_point = 50, not 3", point_ids=None, k=0)
    case(B, "hd", "k_0+f16", "ERR_ARG", "knbn must be > 0", state="f16", k=0)
    case(B, "hd", "no_point", "OK", None, np=0)
    case(B, "hd", "every_point_of_none", "OK", None, state="empty", point_ids=None, np=0, out_ids=None, out_dists=None, out_counts=None)
    case(B, "h", "names_no_point", "ERR_ARG", "3 of the 3 point_ids name no point of the index", state="empty")
    case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT)
    case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="empty")
B = "hnswgpu_graph_search_batch"
case(B, "hd", "f16", "ERR_ARG", GATHER + F16_TAIL, state="f16")
case(B, "hd", "f16_no_point", "ERR_ARG", GATHER + F16_TAIL, state="f16", np=0)
case(B, "d", "never_uploaded_k_4097", "ERR_DEVICE", NOT_RESIDENT, k=4097)     # the limits of the exact call are not this one's
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="simd8")
B = "hnswgpu_exact_graph_batch"
case(B, "hd", "k_4097", "ERR_ARG", "exact graph: knbn above 4096", k=4097)
case(B, "hd", "null_filter", "ERR_ARG", "null filter", n_allowed=2)
case(B, "hd", "simd8", "ERR_ARG", "exact graph" + SIMD8_TAIL, state="simd8")
case(B, "hd", "f16", "ERR_ARG", "exact graph" + F16_TAIL, state="f16")
case(B, "hd", "k_4097+null_filter", "ERR_ARG", "exact graph: knbn above 4096", k=4097, n_allowed=2)
case(B, "hd", "every_point_np+simd8", "ERR_ARG", "point_ids is NULL (every point): np must be nb_point = 50, not 3", state="simd8", point_ids=None)
case(B, "hd", "null_filter+simd8", "ERR_ARG", "null filter", state="simd8", n_allowed=2)
case(B, "h", "unsorted", "ERR_ARG", SORTED, allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted+no_point", "ERR_ARG", SORTED, allowed_ids=[5, 3], n_allowed=2, np=0)
case(B, "h", "unsorted+simd8", "ERR_ARG", "exact graph" + SIMD8_TAIL, state="simd8", allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted+names_no_point", "ERR_ARG", SORTED, state="empty", allowed_ids=[5, 3], n_allowed=2)
case(B, "d", "never_uploaded_unread_filter", "ERR_DEVICE", NOT_RESIDENT, allowed_ids=[5, 3], n_allowed=2)

# ------------------------------------------------------------------------------- hnswgpu_range_search_batch(_device)
B = "hnswgpu_range_search_batch"
FILTER_EF = "range search with a filter: ef_first must be >= 2 (the reference panics at ef == 1, src/hnsw.rs:973)"
case(B, "hd", "null_handle", "ERR_ARG", "null argument", idx=None)
case(B, "hd", "null_out_offsets", "ERR_ARG", OFFSETS, out_offsets=None)
case(B, "hd", "null_queries", "ERR_ARG", "null queries", queries=None)
case(B, "hd", "null_radii", "ERR_ARG", "null radii: every query names its radius", radii=None)
case(B, "hd", "ef_first_0", "ERR_ARG", "ef_first must be >= 1", ef_first=0)
case(B, "hd", "ef_first_above_ef_max", "ERR_ARG", "ef_first is above ef_max", ef_first=32)
case(B, "hd", "ef_max_4097", "ERR_ARG", "range search: ef_max above 4096", ef_max=4097)
case(B, "hd", "null_filter", "ERR_ARG", "null filter", n_allowed=2)
case(B, "hd", "filtered_ef_first_1", "ERR_ARG", FILTER_EF, ef_first=1, allowed_ids=[3, 5], n_allowed=2)
case(B, "hd", "empty_filter_ef_first_1", "ERR_ARG", FILTER_EF, ef_first=1, allowed_ids=[3, 5], n_allowed=0)
case(B, "hd", "cap_null_out_ids", "ERR_ARG", CAP, out_ids=None)
case(B, "hd", "cap_null_out_dists", "ERR_ARG", CAP, out_dists=None)
case(B, "hd", "wrong_d", "ERR_ARG", DIM, d=7)
case(B, "hd", "ef_first_0+wrong_d", "ERR_ARG", "ef_first must be >= 1", ef_first=0, d=7)
case(B, "hd", "ef_first_above+ef_max_4097", "ERR_ARG", "ef_first is above ef_max", ef_first=5000, ef_max=4097)
case(B, "hd", "ef_max_4097+null_filter", "ERR_ARG", "range search: ef_max above 4096", ef_max=4097, n_allowed=2)
case(B, "hd", "filtered_ef_first_1+cap", "ERR_ARG", FILTER_EF, ef_first=1, allowed_ids=[3, 5], n_allowed=2, out_ids=None)
for state in ("simd8", "f16"):                                                 # (either arithmetic and storage is served: neither is refused)
    case(B, "hd", "wrong_d", "ERR_ARG", DIM, state=state, d=7)
    case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state=state)
case(B, "h", "unsorted", "ERR_ARG", SORTED, allowed_ids=[5, 3], n_allowed=2)
case(B, "h", "unsorted+wrong_d", "ERR_ARG", DIM, allowed_ids=[5, 3], n_allowed=2, d=7)
case(B, "h", "answers_nothing", "OK", None, state="empty", zero={"out_offsets": 32, "out_ef": 12, "out_flags": 3})
case(B, "h", "answers_nothing_no_ef_flags", "OK", None, state="empty", out_ef=None, out_flags=None, zero={"out_offsets": 32})
case(B, "h", "no_query", "OK", None, nq=0, zero={"out_offsets": 8})
case(B, "h", "no_query", "OK", None, state="empty", nq=0, zero={"out_offsets": 8})
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT)

# ---------------------------------------------------------------------------------- hnswgpu_symmetric_graph(_device)
B = "hnswgpu_symmetric_graph"
SYM_CAP = "cap > 0 with null out_pos or out_dists (the count-only call is cap == 0)"
case(B, "hd", "null_handle", "ERR_ARG", "null argument", idx=None)
for ef in (0, 32):
    case(B, "hd", "null_out_offsets_ef%d" % ef, "ERR_ARG", OFFSETS, out_offsets=None, ef=ef)
    case(B, "hd", "k_0_ef%d" % ef, "ERR_ARG", "knbn must be > 0", k=0, ef=ef)
    case(B, "hd", "mode_2_ef%d" % ef, "ERR_ARG", "unknown mode 2: HNSWGPU_SYM_UNION or HNSWGPU_SYM_MUTUAL", mode=2, ef=ef)
    case(B, "hd", "cap_null_out_pos_ef%d" % ef, "ERR_ARG", SYM_CAP, out_pos=None, ef=ef)
    case(B, "hd", "cap_null_out_dists_ef%d" % ef, "ERR_ARG", SYM_CAP, out_dists=None, ef=ef)
    case(B, "hd", "slots_ef%d" % ef, "ERR_ARG", "symmetric graph: nb_point x knbn = 50 x 21474837 = 1073741850 slots, above 2^30 = 1073741824",
         k=21474837, ef=ef)
    case(B, "hd", "slots_past_u64_ef%d" % ef, "ERR_ARG", "symmetric graph: nb_point x knbn = 50 x 4611686018427387904 slots, above 2^30 = 1073741824",
         k=1 << 62, ef=ef)
    case(B, "hd", "k_0+mode_2_ef%d" % ef, "ERR_ARG", "knbn must be > 0", k=0, mode=2, ef=ef)
    case(B, "hd", "mode_2+simd8_ef%d" % ef, "ERR_ARG", "unknown mode 4294967295: HNSWGPU_SYM_UNION or HNSWGPU_SYM_MUTUAL", state="simd8",
         mode=0xFFFFFFFF, ef=ef)
case(B, "hd", "k_4097", "ERR_ARG", "exact graph: knbn above 4096", k=4097, ef=0)
case(B, "hd", "simd8", "ERR_ARG", "exact graph" + SIMD8_TAIL, state="simd8", ef=0)
case(B, "hd", "f16", "ERR_ARG", "exact graph" + F16_TAIL, state="f16", ef=0)
case(B, "hd", "f16_ef32", "ERR_ARG", GATHER + F16_TAIL, state="f16", ef=32)
case(B, "hd", "k_4097+simd8", "ERR_ARG", "exact graph: knbn above 4096", state="simd8", k=4097, ef=0)
case(B, "h", "no_edge", "OK", None, state="empty", zero={"out_offsets": 8})
case(B, "h", "no_edge_ef32_count_only", "OK", None, state="empty", ef=32, cap=0, out_pos=None, out_dists=None, zero={"out_offsets": 8})
case(B, "h", "k_0", "ERR_ARG", "knbn must be > 0", state="empty", k=0)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, ef=0)
case(B, "d", "never_uploaded_ef32_k_4097", "ERR_DEVICE", NOT_RESIDENT, ef=32, k=4097)
case(B, "d", "never_uploaded_ef32", "ERR_DEVICE", NOT_RESIDENT, state="simd8", ef=32)

# ------------------------------------------------------- what the five index entries below share: the directed graph D they read
MODE_2 = "unknown mode 2: HNSWGPU_SYM_UNION or HNSWGPU_SYM_MUTUAL"


def directed_graph_rows(B, what, ok, **first):
    """the refusals of directed_graph_shape and directed_graph_source, in their order, behind a pair's own checks of its answer's slots
    (first: one fault those checks find, which fires before every one here).  ok: what an index with no point answers."""
    fk, = first
    fmsg = {"out_n_components": "null out_n_components: the number of components is written by every call",
            "out_n_edges": "null out_n_edges: the number of edges is written by every call"}[fk]
    case(B, "hd", "null_handle", "ERR_ARG", "null argument", idx=None)
    case(B, "hd", "null_handle+k_0", "ERR_ARG", "null argument", idx=None, k=0)
    for ef in (0, 32):
        case(B, "hd", "null_%s_ef%d" % (fk, ef), "ERR_ARG", fmsg, ef=ef, **first)
        case(B, "hd", "k_0_ef%d" % ef, "ERR_ARG", "knbn must be > 0", k=0, ef=ef)
        case(B, "hd", "mode_2_ef%d" % ef, "ERR_ARG", MODE_2, mode=2, ef=ef)
        case(B, "hd", "slots_ef%d" % ef, "ERR_ARG", what + ": nb_point x knbn = 50 x 21474837 = 1073741850 slots, above 2^30 = 1073741824",
             k=21474837, ef=ef)
        case(B, "hd", "slots_past_u64_ef%d" % ef, "ERR_ARG", what + ": nb_point x knbn = 50 x 4611686018427387904 slots, above 2^30 = 1073741824",
             k=1 << 62, ef=ef)
        case(B, "hd", "null_%s+mode_2_ef%d" % (fk, ef), "ERR_ARG", fmsg, mode=2, ef=ef, **first)
        case(B, "hd", "k_0+mode_2_ef%d" % ef, "ERR_ARG", "knbn must be > 0", k=0, mode=2, ef=ef)
        case(B, "hd", "mode_2+slots_ef%d" % ef, "ERR_ARG", MODE_2, mode=2, k=21474837, ef=ef)
        case(B, "hd", "mode_2+simd8_ef%d" % ef, "ERR_ARG", "unknown mode 4294967295: HNSWGPU_SYM_UNION or HNSWGPU_SYM_MUTUAL", state="simd8",
             mode=0xFFFFFFFF, ef=ef)
        case(B, "hd", "slots+f16_ef%d" % ef, "ERR_ARG", what + ": nb_point x knbn = 50 x 21474837 = 1073741850 slots, above 2^30 = 1073741824",
             state="f16", k=21474837, ef=ef)
    case(B, "hd", "k_4097", "ERR_ARG", "exact graph: knbn above 4096", k=4097, ef=0)
    case(B, "hd", "simd8", "ERR_ARG", "exact graph" + SIMD8_TAIL, state="simd8", ef=0)
    case(B, "hd", "f16", "ERR_ARG", "exact graph" + F16_TAIL, state="f16", ef=0)
    case(B, "hd", "f16_ef32", "ERR_ARG", GATHER + F16_TAIL, state="f16", ef=32)
    case(B, "hd", "k_4097+simd8", "ERR_ARG", "exact graph: knbn above 4096", state="simd8", k=4097, ef=0)
    case(B, "hd", "k_4097+f16_ef32", "ERR_ARG", GATHER + F16_TAIL, state="f16", k=4097, ef=32)
    case(B, "hd", "no_vertex", "OK", None, state="empty", zero=ok)
    case(B, "hd", "no_vertex_ef0", "OK", None, state="empty", ef=0, zero=ok)
    case(B, "hd", "k_0", "ERR_ARG", "knbn must be > 0", state="empty", k=0)
    case(B, "hd", "mode_2", "ERR_ARG", MODE_2, state="one", mode=2)
    case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, ef=0)
    case(B, "d", "never_uploaded_ef32_k_4097", "ERR_DEVICE", NOT_RESIDENT, ef=32, k=4097)     # the limits of the exact call are not the search's
    case(B, "d", "never_uploaded_ef32", "ERR_DEVICE", NOT_RESIDENT, state="simd8", ef=32)


def csr_rows(B, what, **first):
    """the refusals of a CSR pair behind its own checks of the answer's slots: what both forms see of the graph, then what only the host
    form can read (first: one fault of the answer's slots, which fires before every one here)"""
    fk, = first
    fmsg = {"out_n_components": "null out_n_components: the number of components is written by every call",
            "out_n_edges": "null out_n_edges: the number of edges is written by every call"}[fk]
    above = what + ": n = 2147483648 vertices, above 2^31 - 1"
    case(B, "hd", "null_" + fk, "ERR_ARG", fmsg, **first)
    case(B, "hd", "n_above", "ERR_ARG", above, n=1 << 31)
    case(B, "hd", "null_offsets", "ERR_ARG", "null offsets", offsets=None)
    case(B, "hd", "null_offsets_one_vertex", "ERR_ARG", "null offsets", n=1, offsets=None)
    case(B, "hd", "null_%s+n_above" % fk, "ERR_ARG", fmsg, n=1 << 31, **first)
    case(B, "hd", "n_above+null_offsets", "ERR_ARG", above, n=1 << 31, offsets=None)
    # ... the graph itself: the host form reads it, the device form's kernels do (no row: they run on a device)
    case(B, "h", "host_only_offsets_start", "ERR_ARG", what + ": offsets[0] is not 0", offsets=[1, 1, 3, 5, 6])
    case(B, "h", "host_only_offsets_descend", "ERR_ARG", what + ": the offsets descend at row 1", offsets=[0, 3, 1, 5, 6])
    case(B, "h", "host_only_too_many_entries", "ERR_ARG", what + ": offsets[n] = 4294967296 is 2^32 or more", offsets=[0, 1, 3, 5, 1 << 32])
    case(B, "h", "host_only_null_cols", "ERR_ARG", what + ": null cols with entries", cols=None)
    case(B, "h", "host_only_col_range", "ERR_ARG", what + ": col 4 at entry 4 is not below n", cols=[1, 0, 2, 1, 4, 2])
    case(B, "h", "host_only_offsets_start+col_range", "ERR_ARG", what + ": offsets[0] is not 0", offsets=[1, 1, 3, 5, 6], cols=[1, 0, 2, 1, 4, 2])
    case(B, "h", "host_only_offsets_descend+too_many_entries", "ERR_ARG", what + ": the offsets descend at row 1", offsets=[0, 3, 1, 5, 1 << 32])
    case(B, "h", "host_only_too_many_entries+null_cols", "ERR_ARG", what + ": offsets[n] = 4294967296 is 2^32 or more",
         offsets=[0, 1, 3, 5, 1 << 32], cols=None)
    case(B, "h", "host_only_null_offsets+col_range", "ERR_ARG", "null offsets", offsets=None, cols=[1, 0, 2, 1, 4, 2])
    case(B, "h", "host_only_null_%s+offsets_start" % fk, "ERR_ARG", fmsg, offsets=[1, 1, 3, 5, 6], **first)


# ------------------------------------------------------ hnswgpu_graph_components(_device), hnswgpu_csr_components(_device)
N_COMP = "null out_n_components: the number of components is written by every call"
NAN_CUT = "max_dist is NaN: no distance compares to it (NULL is the call without a cut)"
B = "hnswgpu_graph_components"
directed_graph_rows(B, "graph components", {"out_n_components": 8}, out_n_components=None)
case(B, "hd", "null_out_label", "ERR_ARG", "null out_label", out_label=None)
case(B, "hd", "nan_max_dist", "ERR_ARG", NAN_CUT, max_dist=[np.nan])
case(B, "hd", "null_out_n_components+null_out_label", "ERR_ARG", N_COMP, out_n_components=None, out_label=None)
case(B, "hd", "null_out_label+nan_max_dist", "ERR_ARG", "null out_label", out_label=None, max_dist=[np.nan])
case(B, "hd", "nan_max_dist+k_0", "ERR_ARG", NAN_CUT, max_dist=[np.nan], k=0)
case(B, "hd", "nan_max_dist+f16", "ERR_ARG", NAN_CUT, state="f16", max_dist=[np.nan])
case(B, "hd", "no_vertex_no_label", "OK", None, state="empty", out_label=None, out_sizes=None, max_dist=[0.5], zero={"out_n_components": 8})
case(B, "hd", "nan_max_dist", "ERR_ARG", NAN_CUT, state="empty", max_dist=[np.nan])
case(B, "hd", "null_out_label", "ERR_ARG", "null out_label", state="one", out_label=None)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="one")
case(B, "d", "never_uploaded_cut_no_sizes", "ERR_DEVICE", NOT_RESIDENT, max_dist=[0.5], out_sizes=None)

B = "hnswgpu_csr_components"
CUT_DISTS = "max_dist without dists: a cut needs the entries' distances"
csr_rows(B, "csr components", out_n_components=None)
case(B, "hd", "null_out_label", "ERR_ARG", "null out_label", out_label=None)
case(B, "hd", "nan_max_dist", "ERR_ARG", NAN_CUT, max_dist=[np.nan])
case(B, "hd", "cut_without_dists", "ERR_ARG", CUT_DISTS, max_dist=[0.5], dists=None)
case(B, "hd", "null_out_label+nan_max_dist", "ERR_ARG", "null out_label", out_label=None, max_dist=[np.nan])
case(B, "hd", "nan_max_dist+n_above", "ERR_ARG", NAN_CUT, max_dist=[np.nan], n=1 << 31)
case(B, "hd", "null_offsets+cut_without_dists", "ERR_ARG", "null offsets", offsets=None, max_dist=[0.5], dists=None)
case(B, "hd", "no_vertex", "OK", None, n=0, zero={"out_n_components": 8})
case(B, "hd", "no_vertex_no_array", "OK", None, n=0, offsets=None, cols=None, dists=None, out_label=None, out_sizes=None, zero={"out_n_components": 8})
case(B, "hd", "no_vertex+cut_without_dists", "ERR_ARG", CUT_DISTS, n=0, max_dist=[0.5], dists=None)
case(B, "hd", "no_vertex+nan_max_dist", "ERR_ARG", NAN_CUT, n=0, max_dist=[np.nan])
case(B, "h", "host_only_cut_without_dists+offsets_start", "ERR_ARG", CUT_DISTS, max_dist=[0.5], dists=None, offsets=[1, 1, 3, 5, 6])

# ------------------------------------------- hnswgpu_graph_spanning_forest(_device), hnswgpu_csr_spanning_forest(_device)
N_EDGES = "null out_n_edges: the number of edges is written by every call"
ABW = "null out_a, out_b or out_w"
CORE_K = "core_k = 5 is above knbn = 4: a row of D has knbn slots"


def forest_rows(B, **more):
    """what hnswgpu_graph_spanning_forest checks around the directed graph's own: hnswgpu_graph_dendrogram repeats it in its words"""
    for buf in ("out_a", "out_b", "out_w"):
        case(B, "hd", "null_" + buf, "ERR_ARG", ABW, **{buf: None})
    case(B, "hd", "core_k_above_k", "ERR_ARG", CORE_K, core_k=5)
    case(B, "hd", "null_out_n_edges+null_out_a", "ERR_ARG", N_EDGES, out_n_edges=None, out_a=None)
    case(B, "hd", "null_out_b+k_0", "ERR_ARG", ABW, out_b=None, k=0)
    case(B, "hd", "mode_2+core_k_above_k", "ERR_ARG", MODE_2, mode=2, core_k=5)
    case(B, "hd", "core_k_above_k+slots", "ERR_ARG", "core_k = 21474838 is above knbn = 21474837: a row of D has knbn slots", k=21474837,
         core_k=21474838)
    case(B, "hd", "core_k_above_k+f16", "ERR_ARG", CORE_K, state="f16", core_k=5)
    case(B, "hd", "core_k_above_k+simd8_ef0", "ERR_ARG", CORE_K, state="simd8", core_k=5, ef=0)
    for state in ("empty", "one"):                                             # no vertex, or one: no edge, and no array needed
        case(B, "hd", "no_edge", "OK", None, state=state, zero={"out_n_edges": 8})
        case(B, "hd", "no_edge_no_array", "OK", None, state=state, out_a=None, out_b=None, out_w=None, zero={"out_n_edges": 8}, **more)
        case(B, "hd", "core_k_above_k", "ERR_ARG", CORE_K, state=state, core_k=5)
        case(B, "hd", "null_out_n_edges", "ERR_ARG", N_EDGES, state=state, out_n_edges=None)
    case(B, "d", "never_uploaded_core_k_is_k", "ERR_DEVICE", NOT_RESIDENT, core_k=4, ef=0)


B = "hnswgpu_graph_spanning_forest"
directed_graph_rows(B, "graph spanning forest", {"out_n_edges": 8}, out_n_edges=None)
forest_rows(B)

B = "hnswgpu_csr_spanning_forest"
csr_rows(B, "csr spanning forest", out_n_edges=None)
for buf in ("out_a", "out_b", "out_w"):
    case(B, "hd", "null_" + buf, "ERR_ARG", ABW, **{buf: None})
case(B, "hd", "null_out_n_edges+null_out_a", "ERR_ARG", N_EDGES, out_n_edges=None, out_a=None)
case(B, "hd", "null_out_w+n_above", "ERR_ARG", ABW, out_w=None, n=1 << 31)
case(B, "hd", "null_out_w+null_offsets", "ERR_ARG", ABW, out_w=None, offsets=None)
for n in (0, 1):                                                               # no vertex, or one: no edge, and no array is read
    case(B, "hd", "no_edge_n%d" % n, "OK", None, n=n, zero={"out_n_edges": 8})
    case(B, "hd", "no_edge_no_out_array_n%d" % n, "OK", None, n=n, out_a=None, out_b=None, out_w=None, cols=None, dists=None,
         zero={"out_n_edges": 8})
    case(B, "hd", "no_edge_unread_graph_n%d" % n, "OK", None, n=n, offsets=[7, 3], cols=[9, 9, 9, 9, 9, 9], zero={"out_n_edges": 8})
case(B, "hd", "no_vertex_no_offsets", "OK", None, n=0, offsets=None, zero={"out_n_edges": 8})

# ---------------------------------------------- hnswgpu_forest_dendrogram(_device), hnswgpu_graph_dendrogram(_device)
B = "hnswgpu_forest_dendrogram"
LRS = "null out_left, out_right or out_size"
FD_N = "forest dendrogram: n = 2147483648 vertices, above 2^31 - 1"
END = "forest dendrogram: edge %d has an end that is not below n"
LOOP = "forest dendrogram: edge %d joins a vertex to itself"


def forest_input_rows(B, none_zeroed):
    """the shape of a forest given as an edge list, and the ends that only the host form can read: hnswgpu_forest_dendrogram and, in the
    same words, hnswhdb_forest (none_zeroed: what n == 0 zeroes)"""
    case(B, "hd", "n_above", "ERR_ARG", FD_N, n=1 << 31)
    case(B, "hd", "m_above", "ERR_ARG", "forest dendrogram: m = 4 edges among n = 4 vertices: a forest has at most n - 1", m=4)
    case(B, "hd", "m_above_no_vertex", "ERR_ARG", "forest dendrogram: m = 1 edges among n = 0 vertices: a forest has at most n - 1", n=0, m=1)
    case(B, "hd", "m_above_one_vertex", "ERR_ARG", "forest dendrogram: m = 1 edges among n = 1 vertices: a forest has at most n - 1", n=1, m=1)
    case(B, "hd", "n_above+m_above", "ERR_ARG", FD_N, n=1 << 31, m=1 << 31)
    case(B, "hd", "m_above+null_a", "ERR_ARG", "forest dendrogram: m = 4 edges among n = 4 vertices: a forest has at most n - 1", m=4, a=None)
    case(B, "hd", "n_above+null_b", "ERR_ARG", FD_N, n=1 << 31, b=None)
    case(B, "hd", "no_vertex", "OK", None, n=0, m=0, zero=none_zeroed)
    case(B, "hd", "no_vertex_no_input", "OK", None, n=0, m=0, a=None, b=None, zero=none_zeroed)
    # ... the ends: the host form reads them, the device form's kernel does (no row: it runs on a device)
    case(B, "h", "host_only_end_a", "ERR_ARG", END % 2, a=[0, 1, 4])
    case(B, "h", "host_only_end_b", "ERR_ARG", END % 0, b=[0xFFFFFFFF, 2, 3])
    case(B, "h", "host_only_self_loop", "ERR_ARG", LOOP % 1, b=[1, 1, 3])
    case(B, "h", "host_only_end+self_loop_before", "ERR_ARG", LOOP % 0, a=[1, 1, 4])
    case(B, "h", "host_only_end+self_loop_behind", "ERR_ARG", END % 1, a=[0, 9, 3])
    case(B, "h", "host_only_end+self_loop_same_edge", "ERR_ARG", END % 0, a=[7, 1, 2], b=[7, 2, 3])
    case(B, "h", "host_only_m_above+end", "ERR_ARG", "forest dendrogram: m = 4 edges among n = 4 vertices: a forest has at most n - 1", m=4,
         a=[0, 1, 4, 0], b=[1, 2, 3, 2])


forest_input_rows(B, {})
case(B, "hd", "null_a", "ERR_ARG", "null a or b", a=None)
case(B, "hd", "null_b", "ERR_ARG", "null a or b", b=None)
for buf in ("out_left", "out_right", "out_size"):
    case(B, "hd", "null_" + buf, "ERR_ARG", LRS, **{buf: None})
case(B, "hd", "null_b+null_out_size", "ERR_ARG", "null a or b", b=None, out_size=None)
case(B, "h", "host_only_null_out_left+end", "ERR_ARG", LRS, out_left=None, a=[0, 1, 4])
for n in (0, 1, 4):                                                            # no merge: no array is read or written
    case(B, "hd", "no_merge_n%d" % n, "OK", None, n=n, m=0)
    case(B, "hd", "no_merge_no_array_n%d" % n, "OK", None, n=n, m=0, a=None, b=None, out_left=None, out_right=None, out_size=None)
case(B, "h", "host_only_no_merge_unread_ends", "OK", None, m=0, a=[9, 9, 9], b=[9, 9, 9])

B = "hnswgpu_graph_dendrogram"
directed_graph_rows(B, "graph spanning forest", {"out_n_edges": 8}, out_n_edges=None)
forest_rows(B, out_left=None, out_right=None, out_size=None)
for buf in ("out_left", "out_right", "out_size"):
    case(B, "hd", "null_" + buf, "ERR_ARG", LRS, **{buf: None})
case(B, "hd", "null_out_a+null_out_left", "ERR_ARG", ABW, out_a=None, out_left=None)
case(B, "hd", "core_k_above_k+null_out_right", "ERR_ARG", CORE_K, core_k=5, out_right=None)
case(B, "hd", "f16+null_out_size", "ERR_ARG", GATHER + F16_TAIL, state="f16", out_size=None)
case(B, "hd", "simd8_ef0+null_out_left", "ERR_ARG", "exact graph" + SIMD8_TAIL, state="simd8", ef=0, out_left=None)

# ------------------------------------------------------------------ hnswhdb_forest(_device), hnswhdb_graph(_device)
COUNTS = "null out_n_clusters or out_n_labels: the two counts are written by every call"
MCS = "min_cluster_size = %d: it must be in 2 .. 2^31 - 1"
METHOD_2 = "unknown method 2: HNSWGPU_SELECT_EOM or HNSWGPU_SELECT_LEAF"
DESCEND = "forest hdbscan: the weights descend at edge %d: the edges' order is the merge order, ascending by weight"
HDB_ARRAYS = ("out_prob", "out_point_cluster", "out_point_w", "out_cluster_parent", "out_cluster_birth_w", "out_cluster_size", "out_stability",
              "out_selected")


def clustering_rows(B, forms, **kw):
    """what all four HDBSCAN entries check of the clustering's own arguments, in their order (kw: what makes the call reach them)"""
    case(B, forms, "null_out_n_clusters", "ERR_ARG", COUNTS, out_n_clusters=None, **kw)
    case(B, forms, "null_out_n_labels", "ERR_ARG", COUNTS, out_n_labels=None, **kw)
    for mcs in (0, 1, 1 << 31):
        case(B, forms, "min_cluster_size_%d" % mcs, "ERR_ARG", MCS % mcs, min_cluster_size=mcs, **kw)
    case(B, forms, "method_2", "ERR_ARG", METHOD_2, method=2, **kw)
    case(B, forms, "null_out_labels", "ERR_ARG", "null out_labels", out_labels=None, **kw)
    case(B, forms, "null_out_n_labels+min_cluster_size_1", "ERR_ARG", COUNTS, out_n_labels=None, min_cluster_size=1, **kw)
    case(B, forms, "min_cluster_size_1+method_2", "ERR_ARG", MCS % 1, min_cluster_size=1, method=2, **kw)
    case(B, forms, "method_2+null_out_labels", "ERR_ARG", "unknown method 4294967295: HNSWGPU_SELECT_EOM or HNSWGPU_SELECT_LEAF",
         method=0xFFFFFFFF, out_labels=None, **kw)


B = "hnswhdb_forest"
forest_input_rows(B, {"out_n_clusters": 8, "out_n_labels": 8})
clustering_rows(B, "hd")
for buf in ("a", "b", "w"):
    case(B, "hd", "null_" + buf, "ERR_ARG", "null a, b or w", **{buf: None})
case(B, "hd", "null_w+null_out_n_clusters", "ERR_ARG", "null a, b or w", w=None, out_n_clusters=None)
case(B, "hd", "m_above+min_cluster_size_1", "ERR_ARG", "forest dendrogram: m = 4 edges among n = 4 vertices: a forest has at most n - 1", m=4,
     min_cluster_size=1)
case(B, "hd", "no_vertex_no_array", "OK", None, n=0, m=0, a=None, b=None, w=None, out_labels=None, zero={"out_n_clusters": 8, "out_n_labels": 8},
     **{buf: None for buf in HDB_ARRAYS})
case(B, "hd", "no_vertex+min_cluster_size_1", "ERR_ARG", MCS % 1, n=0, m=0, min_cluster_size=1)
case(B, "hd", "no_vertex+method_2", "ERR_ARG", METHOD_2, n=0, m=0, method=2)
case(B, "hd", "null_out_labels_one_vertex", "ERR_ARG", "null out_labels", n=1, m=0, out_labels=None)
# ... the weights: the host form reads them behind the ends, the device form's kernel does (no row: it runs on a device)
case(B, "h", "host_only_weights_descend", "ERR_ARG", DESCEND % 2, w=[.25, .75, .5])
case(B, "h", "host_only_weights_descend_from_nan", "ERR_ARG", DESCEND % 1, w=[np.nan, .5, .75])
case(B, "h", "host_only_weights_descend_below_zero", "ERR_ARG", DESCEND % 1, w=[0.0, -1.0, .75])
case(B, "h", "host_only_end+weights_descend", "ERR_ARG", END % 2, a=[0, 1, 4], w=[.75, .5, .25])
case(B, "h", "host_only_self_loop+weights_descend", "ERR_ARG", LOOP % 2, b=[1, 2, 2], w=[.75, .5, .25])
case(B, "h", "host_only_method_2+weights_descend", "ERR_ARG", METHOD_2, method=2, w=[.75, .5, .25])
case(B, "h", "host_only_null_out_labels+end", "ERR_ARG", "null out_labels", out_labels=None, a=[0, 1, 4])

B = "hnswhdb_graph"
directed_graph_rows(B, "graph spanning forest", {"out_n_edges": 8, "out_n_clusters": 8, "out_n_labels": 8}, out_n_edges=None)
clustering_rows(B, "hd")
clustering_rows(B, "hd", state="one")
case(B, "hd", "core_k_above_k", "ERR_ARG", CORE_K, core_k=5)
case(B, "hd", "null_out_n_edges+null_out_n_clusters", "ERR_ARG", N_EDGES, out_n_edges=None, out_n_clusters=None)
case(B, "hd", "mode_2+core_k_above_k", "ERR_ARG", MODE_2, mode=2, core_k=5)
case(B, "hd", "core_k_above_k+f16", "ERR_ARG", CORE_K, state="f16", core_k=5)
case(B, "hd", "core_k_above_k+min_cluster_size_1", "ERR_ARG", CORE_K, core_k=5, min_cluster_size=1)
case(B, "hd", "f16+min_cluster_size_1", "ERR_ARG", GATHER + F16_TAIL, state="f16", min_cluster_size=1)
case(B, "hd", "simd8_ef0+null_out_n_labels", "ERR_ARG", "exact graph" + SIMD8_TAIL, state="simd8", ef=0, out_n_labels=None)
case(B, "hd", "k_0+method_2", "ERR_ARG", "knbn must be > 0", k=0, method=2)
case(B, "hd", "no_vertex_no_array", "OK", None, state="empty", out_a=None, out_b=None, out_w=None, out_left=None, out_right=None, out_size=None,
     out_labels=None, zero={"out_n_edges": 8, "out_n_clusters": 8, "out_n_labels": 8}, **{buf: None for buf in HDB_ARRAYS})
case(B, "hd", "min_cluster_size_1", "ERR_ARG", MCS % 1, state="empty", min_cluster_size=1)
case(B, "hd", "null_out_n_clusters", "ERR_ARG", COUNTS, state="empty", out_n_clusters=None)
case(B, "d", "never_uploaded", "ERR_DEVICE", NOT_RESIDENT, state="one")
case(B, "d", "never_uploaded_optional_arrays", "ERR_DEVICE", NOT_RESIDENT, out_a=None, out_b=None, out_w=None, out_left=None, out_right=None,
     out_size=None, **{buf: None for buf in HDB_ARRAYS})
case(B, "d", "never_uploaded_leaf_core_k_is_k", "ERR_DEVICE", NOT_RESIDENT, core_k=4, ef=0, method=1)


def prototype(name):
    import hnsw_rs_amd._native as N
    return (N.HDBSCAN_HEADER if name.startswith("hnswhdb_") else N.HEADER).prototypes[name]


@pytest.fixture(scope="module")
def handles(native):
    """50 points x 8 dimensions, never uploaded, in every setting the checks look at -- and an index without a point, and one with one"""
    X = native.round_to_f16(np.random.default_rng(1).random((50, 8), dtype=np.float32))
    made = {}
    for state in ("plain", "simd8", "f16"):
        h = native.Hnsw(8, 50, 16, 32, "DistL2")
        h.set_build_options(nthreads=1)
        h.parallel_insert(X)
        if state == "simd8":
            h.set_arithmetic("simd8")
        if state == "f16":
            h.set_storage("f16")
        made[state] = h
    made["empty"] = native.Hnsw(8, 10, 16, 32, "DistL2")
    made["empty"].parallel_insert(np.zeros((0, 8), np.float32))     # (a handle exists from the first insertion on)
    assert made["empty"].handle
    made["one"] = native.Hnsw(8, 10, 16, 32, "DistL2")
    made["one"].set_build_options(nthreads=1)
    made["one"].parallel_insert(X[:1])
    return made


def test_the_table_names_every_entry_of_the_seventeen_pairs():
    import hnsw_rs_amd._native as N
    names = {p.values[0] for p in CASES}
    assert len(names) == 34 and all(n in N.SYMBOLS or n in N.HDBSCAN_SYMBOLS for n in names)
    assert sum(n in N.HDBSCAN_SYMBOLS for n in names) == 4
    assert all(n + "_device" in names for n in names if not n.endswith("_device"))
    for n in names:  # per entry: two faults at once (their order) ...
        labels = [p.id for p in CASES if p.values[0] == n]
        assert any("+" in s for s in labels), n
        if prototype(n)[2][0] == "idx":  # ... of those that take a handle: a null one, and a _device form's answer before any upload
            assert any("null_handle" in s for s in labels), n
            assert not n.endswith("_device") or any(p.values[0] == n and p.values[4] == NOT_RESIDENT for p in CASES), n
        elif not n.endswith("_device"):  # ... of those that take a graph or a forest: what only the host form can read, and the order it is read in
            assert any("host_only" in s and "+" in s for s in labels) and not any("host_only" in p.id for p in CASES if p.values[0] == n + "_device"), n
    assert sum(prototype(n)[2][0] == "idx" for n in names) == 26


@pytest.mark.parametrize("name, state, kw, rc, msg, zero", CASES)
def test_refusal(native, handles, name, state, kw, rc, msg, zero):
    import hnsw_rs_amd._native as N
    unknown = set(kw) - set(DEFAULTS) - set(OUTS) - {"idx"}
    assert not unknown and set(zero) <= set(OUTS), (unknown, zero)
    outs = {o: np.full(OUT_BYTES, SENTINEL, np.uint8) for o in OUTS}
    keep, args = [], []
    for arg in prototype(name)[2]:
        key = arg[2:] if arg.startswith("d_") else arg
        if key == "idx":
            args.append(None if "idx" in kw else handles[state].handle)
            continue
        v = kw[key] if key in kw else (outs[key] if key in outs else DEFAULTS[key])
        if key in IN_DTYPES and v is not None:
            v = np.ascontiguousarray(v, dtype=IN_DTYPES[key])
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data_as(C.c_void_p)
        args.append(v)
    got = getattr(N.lib(), name)(*args)
    assert got == getattr(N, rc), (got, N.last_error())
    if msg is not None:
        assert N.last_error() == msg
    for o, a in outs.items():
        z = zero.get(o, 0)
        assert not a[:z].any() and (a[z:] == SENTINEL).all(), (o, z, a[:z + 8].tolist())
