// knn_graph.hip -- queries by stored point (gfx950 only): the device side of hnswgpu_graph_search_batch / hnswgpu_exact_graph_batch
// and their _device forms (the entries are in capi.cpp) -- the k-NN graph of the indexed points, the point itself left out by
// identity -- and graph_order, the DataId ranks of a replica for the units that build on that graph.  DESIGN.md "Queries by stored
// point".  capi.cpp holds every argument check that needs no device; host: every buffer is plain host memory, else device memory;
// both calls wait for `stream`.  Exact: exact_device of exact_knn.hip with the points' flat ids in place of queries (its prep_rows
// kernel tiles the rows themselves, its slab kernel's SELF variant skips each query's own rank).  Approximate: graph_gather_kernel,
// the batched search with knbn = k + 1, graph_compact_kernel.
//   graph_resolve_kernel   DataIds into flat ids: a binary search over origin_id[order[.]], the first point of a repeated id
//   graph_gather_kernel    the first d elements of the named rows into a dense query matrix (approximate graph)
//   graph_compact_kernel   the search's (k + 1)-wide answers into the caller's k-wide rows, the point's own entry dropped
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "capi_index.hpp"
#include "exact_internal.hpp"
#include "graph_internal.hpp"
#include "hnswio.hpp"
#include "search_kernels.hpp"

namespace hnswgpu {
namespace {

constexpr uint64_t GRAPH_SCRATCH = 256ull << 20;  // bytes of gathered queries and staged answers per chunk of points at most

// one thread per named point.  ids == nullptr: every point, row i being position i of the ascending (DataId, dump order) order.
// An id that no point carries is counted in *n_unknown (its slot gets flat id 0 and is never used: the call fails).
__global__ __launch_bounds__(256) void graph_resolve_kernel(const uint64_t* __restrict__ origin_id, const uint32_t* __restrict__ order, uint32_t n,
                                                           const uint64_t* __restrict__ ids, uint32_t np, uint32_t* __restrict__ flat,
                                                           uint32_t* __restrict__ n_unknown) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= np) return;
    if (ids == nullptr) { flat[i] = order[i]; return; }  // (the caller has checked np == n)
    const uint64_t id = ids[i];
    uint32_t lo = 0, hi = n;  // the first position whose id is >= id
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (origin_id[order[mid]] < id) lo = mid + 1u; else hi = mid;
    }
    uint32_t f = 0;
    if (lo < n && origin_id[order[lo]] == id) f = order[lo];
    else atomicAdd(n_unknown, 1u);
    flat[i] = f;
}

// one thread per element of the query matrix: q[i][j] = element j < d of the row of point flat[i].  The row's padding -- zeros, or
// a DistCosine norm in its last 8 bytes -- stays behind.
__global__ __launch_bounds__(256) void graph_gather_kernel(DeviceIndexView ix, const uint32_t* __restrict__ flat, uint64_t total, float* __restrict__ q) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const uint64_t i = e / ix.d;
    const uint32_t j = (uint32_t)(e - i * ix.d);
    q[e] = ix.vec[(size_t)flat[i] * ix.row_stride + j];
}

// one wavefront per row: the search's answer for the stored vector of point flat[row] with knbn = k + 1 (src) into the k-wide
// row of dst.  The entry whose p_id is the point's own is removed; when there is none and the answer is full, its last entry.
// The slots behind what remains are zeroed.
__global__ __launch_bounds__(64) void graph_compact_kernel(DeviceIndexView ix, const uint32_t* __restrict__ flat, GraphRows src, GraphRows dst, uint32_t k) {
    const uint32_t lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    const uint32_t k1 = k + 1u;
    const uint32_t cnt = src.counts[row] < k1 ? src.counts[row] : k1;
    const uint32_t own = flat[row];
    const size_t s0 = (size_t)row * k1, d0 = (size_t)row * k;
    uint32_t pos = 0xFFFFFFFFu;  // where the point's own entry is (a p_id names one point: at most one entry)
    for (uint32_t j = lane; j < cnt; j += 64u)
        if (ix.layer_offset[src.layer[s0 + j] < NB_LAYER_MAX ? src.layer[s0 + j] : NB_LAYER_MAX] + (uint32_t)src.rank[s0 + j] == own) pos = j;
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)pos, o, 64);
        pos = other < pos ? other : pos;
    }
    const uint32_t left = pos != 0xFFFFFFFFu ? cnt - 1u : (cnt < k ? cnt : k);
    for (uint32_t j = lane; j < k; j += 64u) {
        const bool have = j < left;
        const size_t s = s0 + (j < pos ? j : j + 1u);
        dst.ids[d0 + j] = have ? src.ids[s] : 0ull;
        dst.dists[d0 + j] = have ? src.dists[s] : 0.f;
        if (dst.layer) dst.layer[d0 + j] = have ? src.layer[s] : (uint8_t)0;
        if (dst.rank) dst.rank[d0 + j] = have ? src.rank[s] : 0;
    }
    if (lane == 0u) dst.counts[row] = left;
}

// the points that `a` names as flat ids in device memory (m_flat; word 0 of m_ctrl counts the unknown ids); point_ids is host memory
// for `host`.  Returns ERR_ARG, nothing searched and no output written, when an id names no point.
int graph_resolve(const DeviceIndexView& v, const ExactState& st, const GraphCallArgs& a, bool host, DevMem& m_flat, hipStream_t stream, std::string& err) {
    DevMem m_ids, m_ctrl;
    HIP_TRY(m_flat.alloc(a.np * sizeof(uint32_t)));
    HIP_TRY(m_ctrl.alloc(256));
    const uint64_t* d_ids = a.point_ids;
    if (host && a.point_ids != nullptr) {
        HIP_TRY(m_ids.alloc(a.np * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(m_ids.p, a.point_ids, a.np * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        d_ids = static_cast<const uint64_t*>(m_ids.p);
    }
    uint32_t unknown = 0;
    HIP_TRY(hipMemsetAsync(m_ctrl.p, 0, 4, stream));
    hipLaunchKernelGGL(graph_resolve_kernel, grid_of(a.np), dim3(256), 0, stream, v.origin_id, st.order(), v.n, d_ids, (uint32_t)a.np,
                       static_cast<uint32_t*>(m_flat.p), static_cast<uint32_t*>(m_ctrl.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&unknown, m_ctrl.p, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (unknown != 0) {
        err = std::to_string(unknown) + " of the " + std::to_string(a.np) + " point_ids name no point of the index";
        return ERR_ARG;
    }
    return OK;
}

}  // namespace

// Approximate graph: chunk by chunk of at most HNSWGPU_GRAPH_CHUNK points (unset: what GRAPH_SCRATCH holds), the points' vectors
// gathered on the device, searched by the batched search itself with knbn = k + 1, and compacted into the caller's rows.
int graph_search(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, bool host, void* stream_v, std::string& err) {
    const uint64_t np = a.np, k = a.k, ef = a.ef;
    if (np == 0) return OK;
    const DeviceIndexView& v = dev.view();
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "graph search", err);
    if (!st) return ERR_DEVICE;
    const GraphRows out{a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts};  // np rows of k slots
    DevMem m_flat, m_q;
    AnswerStage wide, stage;  // the search's (k + 1)-wide answers; a host call's k-wide ones
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)
    int rc = graph_resolve(v, *st, a, host, m_flat, stream, err);
    if (rc != OK) return rc;
    const uint32_t* d_flat = static_cast<const uint32_t*>(m_flat.p);

    const uint64_t d = v.d, k1 = k + 1;
    const uint64_t per_point = d * 4 + k1 * 17 + 4 + (host ? k * 17 + 4 : 0);
    const int64_t knob = knobs().graph_chunk;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({np, GRAPH_SCRATCH / per_point, knob > 0 ? (uint64_t)knob : np}));
    HIP_TRY(m_q.alloc(chunk * d * 4));
    float* d_q = static_cast<float*>(m_q.p);
    if ((rc = wide.alloc("graph search", chunk, k1, err)) != OK) return rc;
    if (host && (rc = stage.alloc("graph search", chunk, k, err)) != OK) return rc;

    for (uint64_t c0 = 0; c0 < np; c0 += chunk) {
        const uint64_t cq = std::min(chunk, np - c0);
        hipLaunchKernelGGL(graph_gather_kernel, grid_of(cq * d), dim3(256), 0, stream, v, d_flat + c0, cq * d, d_q);
        HIP_TRY(hipGetLastError());
        rc = dev.search_device(d_q, cq, d, k1, ef, wide.rows.ids, wide.rows.dists, wide.rows.layer, wide.rows.rank, wide.rows.counts, nullptr, stream, nullptr, 0,
                               nullptr, err);
        if (rc != OK) return rc;
        hipLaunchKernelGGL(graph_compact_kernel, dim3((uint32_t)cq), dim3(64), 0, stream, v, d_flat + c0, wide.rows, host ? stage.rows : rows_at(out, c0, k),
                           (uint32_t)k);
        HIP_TRY(hipGetLastError());
        if (host && (rc = copy_rows_out(rows_at(out, c0, k), stage.rows, cq * k, cq, stream, err)) != OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// Exact graph: the exact k-NN's own chunk loop over tiles built from the rows themselves, the slab kernel's SELF variant
int exact_graph(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, bool host, void* stream_v, std::string& err) {
    const uint64_t np = a.np, k = a.k;
    if (np == 0) return OK;
    const DeviceIndexView& v = dev.view();
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "exact graph", err);
    if (!st) return ERR_DEVICE;
    const GraphRows out{a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts};  // np rows of k slots
    DevMem m_flat;
    FilterUpload filter;
    AnswerStage stage;
    int rc = graph_resolve(v, *st, a, host, m_flat, stream, err);  // (waits for the stream)
    if (rc != OK) return rc;
    ExactCall c{nullptr, static_cast<const uint32_t*>(m_flat.p), np, v.d, k, a.allowed, a.n_allowed, nullptr, out};
    if (!host) return exact_device(dev, origin_id, c, stream, err);
    if ((rc = filter.put(a.allowed, a.n_allowed, err)) != OK) return rc;
    c.d_allowed = filter.d_allowed;
    // chunks of points: the staged answers stay within 64 MB whatever np is
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(np, (64ull << 20) / (k * 17 + 4)));
    if ((rc = stage.alloc("exact graph", chunk, k, err)) != OK) return rc;
    c.out = stage.rows;
    for (uint64_t c0 = 0; c0 < np; c0 += chunk, c.d_self += chunk) {
        c.nq = std::min(chunk, np - c0);
        if ((rc = exact_device(dev, origin_id, c, stream, err)) != OK) return rc;
        if ((rc = copy_rows_out(rows_at(out, c0, k), stage.rows, c.nq * k, c.nq, stream, err)) != OK) return rc;
    }
    return OK;
}

// The DataId ranks of the replica's state, for symmetric_graph.hip and the units behind it (graph_internal.hpp): made on first use,
// like every call here does
int graph_order(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, GraphOrder& out, std::string& err) {
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "symmetric graph", err);
    if (!st) return ERR_DEVICE;
    out.keep = st;
    out.d_rank = st->rank();
    out.d_order = st->order();
    return OK;
}

}  // namespace hnswgpu
