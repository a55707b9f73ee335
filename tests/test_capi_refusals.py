"""What the batched C entries answer BEFORE a device is touched, pinned to the letter: the exact return code, the complete
hnswgpu_last_error() text and the exact bytes of every output array, for the eight host / _device pairs behind the filter-set search,
the exact k-NN (plain and under a filter set), the exact range search, the two stored-point graph calls, the approximate range search
and the symmetrised graph, plus hnswgpu_search_batch_filtered(_device).  The other ABI tests look for a word of the message; this
table is what keeps the shared argument checks of capi.cpp (and the order they fire in) from drifting between the pairs.

Every case returns before the HIP runtime is asked anything, so the answers are the same with and without a GPU.  CPU only."""
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
             "filter_of": np.uint32, "point_ids": np.uint64}
OUTS = ("out_ids", "out_dists", "out_layer", "out_rank", "out_counts", "out_status", "out_offsets", "out_ef", "out_flags", "out_pos", "n_panics")
SENTINEL, OUT_BYTES = 0x5A, 512
# a well-formed call on the 50 x 8 index: 3 queries (or points), knbn 4, two filters {1, 5, 9} and {2, 3}
DEFAULTS = dict(queries=np.linspace(0, 1, 24), nq=3, d=8, k=4, ef=16, radii=[0.5, 0.5, 0.5], allowed_ids=None, n_allowed=0,
                filter_ids=[1, 5, 9, 2, 3], filter_offsets=[0, 3, 5], n_filters=2, filter_of=[0, 1, 0], point_ids=[0, 1, 2], np=3,
                ef_first=4, ef_max=16, cap=16, mode=0, stats=None, stream=None)

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


@pytest.fixture(scope="module")
def handles(native):
    """50 points x 8 dimensions, never uploaded, in every setting the checks look at -- and an index without a point"""
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
    return made


def test_the_table_names_every_entry_of_the_nine_pairs():
    import hnsw_rs_amd._native as N
    names = {p.values[0] for p in CASES}
    assert len(names) == 18 and all(n in N.SYMBOLS for n in names)
    for n in names:  # per entry: a null handle, and two faults at once (their order)
        labels = [p.id for p in CASES if p.values[0] == n]
        assert any("null_handle" in s for s in labels) and any("+" in s for s in labels), n
    assert all(n + "_device" in names for n in names if not n.endswith("_device"))
    assert all(any(p.values[0] == n and p.values[4] == NOT_RESIDENT for p in CASES) for n in names if n.endswith("_device"))


@pytest.mark.parametrize("name, state, kw, rc, msg, zero", CASES)
def test_refusal(native, handles, name, state, kw, rc, msg, zero):
    import hnsw_rs_amd._native as N
    unknown = set(kw) - set(DEFAULTS) - set(OUTS) - {"idx"}
    assert not unknown and set(zero) <= set(OUTS), (unknown, zero)
    outs = {o: np.full(OUT_BYTES, SENTINEL, np.uint8) for o in OUTS}
    keep, args = [], []
    for arg in N.HEADER.prototypes[name][2]:
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
