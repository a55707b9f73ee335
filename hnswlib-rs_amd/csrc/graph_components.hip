// graph_components.hip -- connected components on the device (gfx950 only): the device side of hnswgpu_graph_components(_device)
// and hnswgpu_csr_components(_device) of include/hnsw_mi355x.h (the entries and every check that needs no device are in capi.cpp).
// DESIGN.md "Connected components".
//
// A lock-free union-find over u32 parents (ECL-CC: Jaiganesh & Burtscher, HPDC 2018), one thread per ENTRY of the graph:
//   cc_check_offsets_kernel  (CSR) one thread per row: offsets[0] == 0, no descent, offsets[n] < 2^32 -- flags and the total in one word
//   cc_check_cols_kernel     (CSR) a fixed grid strides over the offsets[n] cols: every col < n.  The word is read back BEFORE any
//                            kernel below runs: no kernel follows a col that was not checked.
//   cc_init_kernel           parent[v] = v
//   cc_hook_csr_kernel       one thread per entry e: its row by a binary search in the offsets, the cut, unite(row, col)
//   cc_hook_slots_kernel     (index, UNION) one thread per slot of D: the neighbour's position through the rank array as in
//                            sym_expand_kernel, the cut, unite(i, j).  No sort: every surviving slot is an edge.
//   cc_hook_records_kernel   (index, MUTUAL) one thread per sorted edge record of symmetric_graph.hip: a forward record (i, j) whose
//                            successor is the reverse record (i, j) is a pair named both ways; the two records carry d(i->j) and
//                            d(j->i), the cut looks at both, unite(i, j)
//   cc_compress_kernel       one thread per vertex: parent[v] = its root; mark[v] = (v is a root)
//   (rocPRIM)                an exclusive scan of the marks: a root's dense number in ascending root order, and the count c
//   cc_label_kernel          one thread per vertex: label[v] = number of parent[v]; sizes[label] += 1 (integer atomics, one per
//                            wavefront where the wavefront agrees on the label)
// The invariant behind every loop: parent[v] <= v at all times, and a write to parent[v] only ever lowers it (a compare-and-swap of a
// root v to a smaller root, an atomic min with an ancestor).  So the links have no cycle, a walk up strictly descends, and a root is
// the smallest vertex of its tree.  Once the hooks are done the trees are the components whatever the timing was: the answer is a
// function of the graph alone.  No wavefront waits on another; no kernel walks a row.
#include <hip/hip_runtime.h>

#include <string>

#include "capi_index.hpp"
#include "csr_intake.hpp"
#include "graph_internal.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"
#include "union_find.hpp"

namespace hnswgpu {
namespace {

// d <= cut as an ordered comparison: false for a NaN, -0 equals +0
__device__ __forceinline__ bool survives(float d, uint32_t has_cut, float cut) { return has_cut == 0u || d <= cut; }

__global__ __launch_bounds__(256) void cc_init_kernel(uint32_t* __restrict__ parent, uint32_t n) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) parent[v] = v;
}

// one thread per entry e of a checked CSR: offsets[0] = 0 <= e < total = offsets[n], the offsets ascend, every col < n
__global__ __launch_bounds__(256) void cc_hook_csr_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ cols,
                                                         const float* __restrict__ dists, uint32_t n, uint32_t total, uint32_t has_cut, float cut,
                                                         uint32_t* parent) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    if (has_cut != 0u && !(dists[e] <= cut)) return;
    uint32_t lo = 0u, hi = n;  // offsets[lo] <= e < offsets[hi]; ends: hi - lo halves
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= (uint64_t)e) lo = mid; else hi = mid;
    }
    const uint32_t c = cols[e];
    if (c != lo) cc_unite(parent, lo, c);
}

// one thread per slot t = i k + s of D
__global__ __launch_bounds__(256) void cc_hook_slots_kernel(DeviceIndexView ix, const uint32_t* __restrict__ rank_of, const uint8_t* __restrict__ layer,
                                                           const int32_t* __restrict__ rank, const float* __restrict__ dists,
                                                           const uint32_t* __restrict__ counts, uint32_t k, uint32_t slots, uint32_t has_cut, float cut,
                                                           uint32_t* parent) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= slots) return;
    const uint32_t i = t / k, s = t - i * k;
    if (s >= counts[i] || !survives(dists[t], has_cut, cut)) return;
    const uint32_t l = layer[t] < NB_LAYER_MAX ? layer[t] : NB_LAYER_MAX;
    const uint32_t flat = ix.layer_offset[l] + (uint32_t)rank[t];
    if (flat >= ix.n) return;  // (a p_id of the index, whatever the slot holds)
    const uint32_t j = rank_of[flat];
    if (j < ix.n && j != i) cc_unite(parent, i, j);
}

// one thread per sorted record: the forward record of a pair that has its reverse record too
__global__ __launch_bounds__(256) void cc_hook_records_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t records,
                                                             uint32_t n, uint32_t has_cut, float cut, uint32_t* parent) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t + 1u >= records) return;
    const uint64_t key = keys[t];
    const uint32_t row = (uint32_t)(key >> 33), col = (uint32_t)(key >> 1);
    if (row >= n || col >= n || (key & FLAG_REV) != 0ull || keys[t + 1u] != (key | FLAG_REV)) return;
    if (!survives(__uint_as_float(vals[t]), has_cut, cut) || !survives(__uint_as_float(vals[t + 1u]), has_cut, cut)) return;
    if (row != col) cc_unite(parent, row, col);
}

#include "union_find_compress.inc"

// one thread per vertex; parent[v] is v's root, number_of[r] the dense number of root r
__global__ __launch_bounds__(256) void cc_label_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ number_of, uint32_t n,
                                                      uint32_t* __restrict__ label, uint32_t* __restrict__ sizes) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < n;
    uint32_t lab = 0u;
    if (live) {
        lab = number_of[parent[v]];
        label[v] = lab;
    }
    if (sizes == nullptr) return;
    // lane 0 of a wavefront holds its smallest v: it is live whenever any lane is
    const uint32_t first = __builtin_amdgcn_readfirstlane(lab);
    const uint64_t all = __ballot(live), same = __ballot(live && lab == first);
    if (same == all) {
        if ((threadIdx.x & 63u) == 0u && live) atomicAdd(sizes + first, (uint32_t)__popcll(all));
    } else if (live) {
        atomicAdd(sizes + lab, 1u);
    }
}

// what every form keeps for the length of a call: parent, mark and the scan of the marks (4 n, 4 n + 4, 4 n + 4 bytes)
struct Forest {
    DevMem mem;
    uint32_t* parent = nullptr;
    uint32_t* mark = nullptr;
    uint32_t* number_of = nullptr;
};
int forest_init(Forest& f, uint64_t n, hipStream_t stream, std::string& err) {
    ScratchLayout lay;
    lay.arrays(n + 1, f.parent, f.mark, f.number_of);
    const int rc = alloc_layout("components", f.mem, lay, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(cc_init_kernel, grid_of(n), dim3(256), 0, stream, f.parent, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return OK;
}

// the hooks are on the stream: roots, their numbers, the labels and the sizes.  host: out_label / out_sizes are host memory.
int forest_answer(Forest& f, uint64_t n, bool host, uint32_t* out_label, uint32_t* out_sizes, uint64_t* out_n, hipStream_t stream, std::string& err) {
    DevMem m_temp, m_out;
    HIP_TRY(hipMemsetAsync(f.mark + n, 0, 4, stream));
    hipLaunchKernelGGL(cc_compress_kernel, grid_of(n), dim3(256), 0, stream, f.parent, (uint32_t)n, f.mark);
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(m_temp, f.mark, f.number_of, n + 1, stream, err);
    if (rc != OK) return rc;
    uint32_t c = 0;
    HIP_TRY(hipMemcpyAsync(&c, f.number_of + n, 4, hipMemcpyDeviceToHost, stream));  // the read-back of the device entries
    HIP_TRY(hipStreamSynchronize(stream));
    if (c == 0 || c > n) {
        err = "components: " + std::to_string(c) + " roots among " + std::to_string(n) + " vertices";
        return ERR_FORMAT;
    }
    uint32_t* d_label = out_label;
    uint32_t* d_sizes = out_sizes;
    if (host) {
        ScratchLayout lay;
        lay.array(d_label, n);
        lay.bytes(d_sizes, (uint64_t)c * 4);  // (the block ends with the c words)
        rc = alloc_layout("components", m_out, lay, err);
        if (rc != OK) return rc;
        if (!out_sizes) d_sizes = nullptr;
    }
    if (d_sizes) HIP_TRY(hipMemsetAsync(d_sizes, 0, (uint64_t)c * 4, stream));
    hipLaunchKernelGGL(cc_label_kernel, grid_of(n), dim3(256), 0, stream, f.parent, f.number_of, (uint32_t)n, d_label, d_sizes);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(out_label, d_label, n * 4, hipMemcpyDeviceToHost, stream));
        if (out_sizes) HIP_TRY(hipMemcpyAsync(out_sizes, d_sizes, (uint64_t)c * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    *out_n = c;
    return OK;
}

}  // namespace

// Both index entries (capi.cpp refers to it weakly, capi_index.hpp): n >= 1.  Waits for `stream` before it returns.
int graph_components(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ComponentsArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const DeviceIndexView& v = dev.view();
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t n = v.n, k = a.k, slots = n * k;  // (n k <= 2^30: checked by the entries)
    StagedGraph d;
    SortedRecords rec;
    Forest f;
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)
    GraphOrder ord;
    int rc = graph_order(dev, origin_id, ord, err);
    if (rc != OK) return rc;
    const uint32_t has_cut = a.has_cut ? 1u : 0u;
    if (a.mode == HNSWGPU_SYM_UNION) {
        rc = stage_directed_graph(dev, origin_id, k, a.ef, stream_v, d, err);
        if (rc != OK) return rc;
        rc = forest_init(f, n, stream, err);
        if (rc != OK) return rc;
        hipLaunchKernelGGL(cc_hook_slots_kernel, grid_of(slots), dim3(256), 0, stream, v, ord.d_rank, d.layer, d.rank, d.dists, d.counts, (uint32_t)k,
                           (uint32_t)slots, has_cut, a.max_dist, f.parent);
    } else {
        rc = sorted_edge_records(dev, origin_id, ord, k, a.ef, stream_v, rec, err);
        if (rc != OK) return rc;
        rec.keys_a.release();  // (the sort's other half: not needed here)
        rec.vals_a.release();
        rc = forest_init(f, n, stream, err);
        if (rc != OK) return rc;
        hipLaunchKernelGGL(cc_hook_records_kernel, grid_of(rec.records), dim3(256), 0, stream, static_cast<const uint64_t*>(rec.keys_b.p),
                           static_cast<const uint32_t*>(rec.vals_b.p), (uint32_t)rec.records, (uint32_t)n, has_cut, a.max_dist, f.parent);
    }
    HIP_TRY(hipGetLastError());
    return forest_answer(f, n, host, a.out_label, a.out_sizes, a.out_n, stream, err);
}

// Both CSR entries: 1 <= n < 2^31.  host: every array is host memory and has passed the same checks on the host (capi.cpp).
int csr_components(const CsrComponentsArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = use_device_ordinal("csr components", a.device, err);
    if (rc != OK) return rc;
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    const uint64_t n = a.n;
    CsrOnDevice csr;
    Forest f;
    Drain drain{stream};
    rc = csr_intake("csr components", n, a.offsets, a.cols, a.dists, host, a.has_cut, stream, csr, err);
    if (rc != OK) return rc;
    const uint64_t total = csr.total;
    rc = forest_init(f, n, stream, err);
    if (rc != OK) return rc;
    if (total != 0) {
        hipLaunchKernelGGL(cc_hook_csr_kernel, grid_of(total), dim3(256), 0, stream, csr.offsets, csr.cols, csr.dists, (uint32_t)n, (uint32_t)total,
                           a.has_cut ? 1u : 0u, a.max_dist, f.parent);
        HIP_TRY(hipGetLastError());
    }
    return forest_answer(f, n, host, a.out_label, a.out_sizes, a.out_n, stream, err);
}

}  // namespace hnswgpu
