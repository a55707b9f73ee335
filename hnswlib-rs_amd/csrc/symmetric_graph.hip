// symmetric_graph.hip -- the k-NN graph of the indexed points made undirected, in CSR (gfx950 only): the device side of
// hnswgpu_symmetric_graph / hnswgpu_symmetric_graph_device of include/hnsw_mi355x.h (the entries and every check that needs no
// device are in capi.cpp).  DESIGN.md "Symmetrised k-NN graph".
//
// The directed graph D is one call of the graph path itself (exact_graph or graph_search of knn_graph.hip, every point, device
// buffers): n rows of k slots, counts[i] of them used.  Then
//   sym_expand_kernel   one thread per slot of D: the neighbour's p_id into its position j (flat id, then the rank array of the
//                       exact path), the forward record (i, j, FWD) and the reverse record (j, i, REV), both carrying the slot's
//                       distance bits.  A record is a 64-bit key {row, col, flag} and a 32-bit value; a slot behind counts[i]
//                       writes two records of row n, which sort behind every row.
//   (rocPRIM)           a radix sort of the records by key: by row, then col, FWD before REV
//   sym_mark_kernel     one thread per record: the head of a run of equal (row, col) -- a run has one or two records -- is an entry
//                       of the answer under UNION, and under MUTUAL iff the run has both records.  The head is the FWD record when
//                       the run has one, so the head's value is the entry's distance.
//   (rocPRIM)           an exclusive scan of the marks: every entry's slot in the answer (records are in row order), and the total
//   sym_offsets_kernel  one thread per row: a binary search for the row's first record; the scan's value there is the row's offset
//   sym_fill_kernel     one thread per record: an entry writes {order bits of its distance, col} and its raw distance bits at its slot
//   (rocPRIM)           a segmented radix sort, one segment per row, the raw bits as the value: the order within a row
//   sym_decode_kernel   one thread per entry: position, DataId, distance bits as stored, p_id
// No atomics and no write whose place depends on timing: the answer is a function of D alone.  No kernel walks a row: a row of
// n - 1 entries costs what n - 1 entries of short rows cost.
// The first half -- D staged (stage_directed_graph), expanded and sorted (sorted_edge_records) -- is shared with
// graph_components.hip through graph_internal.hpp: the components of the UNION graph hook D's slots, those of the MUTUAL graph the
// sorted records.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "graph_internal.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"

namespace hnswgpu {
namespace {

// (a record's key, rec_key and FLAG_REV, is in graph_internal.hpp: graph_components.hip reads the sorted records too)
// one thread per slot t = i k + s of D; records 2 t and 2 t + 1
__global__ __launch_bounds__(256) void sym_expand_kernel(DeviceIndexView ix, const uint32_t* __restrict__ rank_of, const uint8_t* __restrict__ layer,
                                                        const int32_t* __restrict__ rank, const float* __restrict__ dists,
                                                        const uint32_t* __restrict__ counts, uint32_t k, uint32_t slots, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= slots) return;
    const uint32_t i = t / k, s = t - i * k;
    uint64_t fwd = rec_key(ix.n, 0u, 0ull), rev = fwd;  // (behind every row)
    uint32_t bits = 0u;
    if (s < counts[i]) {
        const uint32_t l = layer[t] < NB_LAYER_MAX ? layer[t] : NB_LAYER_MAX;
        const uint32_t flat = ix.layer_offset[l] + (uint32_t)rank[t];
        if (flat < ix.n) {  // (a p_id of the index, whatever the slot holds)
            const uint32_t j = rank_of[flat];
            fwd = rec_key(i, j, 0ull);
            rev = rec_key(j, i, FLAG_REV);
            bits = __float_as_uint(dists[t]);
        }
    }
    keys[2u * (size_t)t] = fwd;
    keys[2u * (size_t)t + 1u] = rev;
    vals[2u * (size_t)t] = bits;
    vals[2u * (size_t)t + 1u] = bits;
}

// one thread per sorted record: mark[t] = 1 iff the record is an entry of the answer
__global__ __launch_bounds__(256) void sym_mark_kernel(const uint64_t* __restrict__ keys, uint32_t records, uint32_t n, uint32_t mutual,
                                                      uint32_t* __restrict__ mark) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= records) return;
    const uint64_t key = keys[t];
    bool entry = (uint32_t)(key >> 33) < n && (t == 0u || (keys[t - 1u] >> 1) != (key >> 1));  // a real row, the head of its run
    if (entry && mutual != 0u) entry = (key & FLAG_REV) == 0ull && t + 1u < records && keys[t + 1u] == (key | FLAG_REV);
    mark[t] = entry ? 1u : 0u;
}

// one thread per row r of 0 .. n: offsets[r] = the entries of the rows before r = the scan at the first record of a row >= r
__global__ __launch_bounds__(256) void sym_offsets_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ slot_of, uint32_t records,
                                                         uint32_t n, uint64_t* __restrict__ offsets) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > n) return;
    const uint64_t first = rec_key(r, 0u, 0ull);
    uint32_t lo = 0, hi = records;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] < first) lo = mid + 1u; else hi = mid;
    }
    offsets[r] = slot_of[lo];  // (slot_of has records + 1 entries: the last is the total)
}

// one thread per sorted record: an entry's sort key within its row and its raw distance bits, at its slot of the answer
__global__ __launch_bounds__(256) void sym_fill_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ mark, const uint32_t* __restrict__ slot_of, uint32_t records,
                                                      uint64_t* __restrict__ row_keys, uint32_t* __restrict__ row_bits) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= records || mark[t] == 0u) return;
    const uint32_t col = (uint32_t)(keys[t] >> 1), bits = vals[t], to = slot_of[t];
    row_keys[to] = ((uint64_t)dist_order_bits(__uint_as_float(bits)) << 32) | col;
    row_bits[to] = bits;
}

struct SymSlots {
    uint32_t* pos;
    uint64_t* ids;   // may be nullptr
    uint32_t* bits;
    uint8_t* layer;  // may be nullptr
    int32_t* rank;   // may be nullptr
};
// one thread per entry of the answer, in its final place
__global__ __launch_bounds__(256) void sym_decode_kernel(DeviceIndexView ix, const uint32_t* __restrict__ order, const uint64_t* __restrict__ row_keys,
                                                        const uint32_t* __restrict__ row_bits, uint32_t total, SymSlots out) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const uint32_t col = (uint32_t)row_keys[e];
    const uint32_t flat = order[col < ix.n ? col : 0u];  // (a position, whatever the slot holds)
    uint32_t l = 0;
    while (l + 1 < NB_LAYER_MAX && flat >= ix.layer_offset[l + 1]) ++l;
    out.pos[e] = col;
    if (out.ids) out.ids[e] = ix.origin_id[flat];
    out.bits[e] = row_bits[e];  // the stored bits: a -0 or a NaN's payload comes back as D holds it
    if (out.layer) out.layer[e] = (uint8_t)l;
    if (out.rank) out.rank[e] = (int32_t)(flat - ix.layer_offset[l]);
}

// the CSR offsets as the segment bounds of the sort
struct SegBound {
    __host__ __device__ unsigned int operator()(uint64_t v) const { return (unsigned int)v; }
};
typedef rocprim::transform_iterator<const uint64_t*, SegBound, unsigned int> seg_iter_t;

}  // namespace

// D staged for every point: the graph path's own call into one allocation (graph_internal.hpp)
int stage_directed_graph(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, uint64_t k, uint64_t ef, void* stream_v, StagedGraph& out,
                         std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const uint64_t n = dev.view().n, slots = n * k;
    uint64_t* d_ids = nullptr;
    ScratchLayout lay;
    lay.arrays(slots, d_ids, out.dists, out.rank);
    lay.array(out.counts, n);
    lay.array(out.layer, slots);
    const int rc = alloc_layout("graph", out.mem, lay, err);
    if (rc != OK) return rc;
    const GraphCallArgs every_point{nullptr, n, k, ef, nullptr, 0, d_ids, out.dists, out.layer, out.rank, out.counts};
    return ef == 0 ? exact_graph(dev, origin_id, every_point, false, stream, err) : graph_search(dev, origin_id, every_point, false, stream, err);
}

// D's edge records, sorted (graph_internal.hpp)
int sorted_edge_records(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphOrder& ord, uint64_t k, uint64_t ef, void* stream_v,
                        SortedRecords& out, std::string& err) {
    StagedGraph d;
    return sorted_edge_records_keeping(dev, origin_id, ord, k, ef, stream_v, out, d, err);  // (D is in the records: released here)
}

// the same, D left in `d`
int sorted_edge_records_keeping(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphOrder& ord, uint64_t k, uint64_t ef, void* stream_v,
                                SortedRecords& out, StagedGraph& d, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const DeviceIndexView& v = dev.view();
    const uint64_t n = v.n;
    const uint64_t slots = n * k, records = 2 * slots;  // (n k <= 2^30: checked by the entries)
    out.records = records;
    DevMem m_temp;
    Drain drain{stream};
    // D, staged: the graph path's own answer for every point, row i the point at position i
    int rc = stage_directed_graph(dev, origin_id, k, ef, stream_v, d, err);
    if (rc != OK) return rc;

    // the records, and their sort.  keys_a has room for one word more per half: it holds the marks and their scan afterwards.
    HIP_TRY(out.keys_a.alloc(records * 8 + 256));
    HIP_TRY(out.keys_b.alloc(records * 8));
    HIP_TRY(out.vals_a.alloc(records * 4));
    HIP_TRY(out.vals_b.alloc(records * 4));
    uint64_t* keys_a = static_cast<uint64_t*>(out.keys_a.p);
    uint64_t* keys_b = static_cast<uint64_t*>(out.keys_b.p);
    uint32_t* vals_a = static_cast<uint32_t*>(out.vals_a.p);
    uint32_t* vals_b = static_cast<uint32_t*>(out.vals_b.p);
    hipLaunchKernelGGL(sym_expand_kernel, grid_of(slots), dim3(256), 0, stream, v, ord.d_rank, d.layer, d.rank, d.dists, d.counts, (uint32_t)k, (uint32_t)slots,
                       keys_a, vals_a);
    HIP_TRY(hipGetLastError());
    unsigned end_bit = 34;  // the flag, the col, and the bits of a row number 0 .. n
    while (end_bit < 64 && (n >> (end_bit - 33)) != 0) ++end_bit;
    rc = radix_sort_pairs(m_temp, keys_a, keys_b, vals_a, vals_b, (uint32_t)records, end_bit, stream, err);
    if (rc != OK) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;  // (the sort's temporary storage is released here)
}

// Both entries (capi.cpp refers to it weakly, capi_index.hpp).  host: the out arrays are plain host memory, else device memory.
// Waits for `stream` before it returns.  dev_p == nullptr (device entry on an empty index): the one offset is zeroed.
int symmetric_graph(DeviceIndex* dev_p, const std::vector<uint64_t>& origin_id, const SymGraphArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (dev_p == nullptr) {  // no point: no row
        HIP_TRY(hipMemsetAsync(a.out_offsets, 0, 8, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return OK;
    }
    DeviceIndex& dev = *dev_p;
    const DeviceIndexView& v = dev.view();
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t n = v.n, k = a.k;
    const uint64_t records = 2 * n * k;  // (n k <= 2^30: checked by the entries)
    SortedRecords rec;
    DevMem m_temp, m_offs, m_row;
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)
    GraphOrder ord;
    int rc = graph_order(dev, origin_id, ord, err);
    if (rc != OK) return rc;
    rc = sorted_edge_records(dev, origin_id, ord, k, a.ef, stream_v, rec, err);
    if (rc != OK) return rc;
    uint64_t* keys_a = static_cast<uint64_t*>(rec.keys_a.p);
    uint64_t* keys_b = static_cast<uint64_t*>(rec.keys_b.p);
    uint32_t* vals_a = static_cast<uint32_t*>(rec.vals_a.p);
    uint32_t* vals_b = static_cast<uint32_t*>(rec.vals_b.p);

    // marks, their scan, the offsets, the total
    uint32_t* mark = reinterpret_cast<uint32_t*>(keys_a);
    uint32_t* slot_of = mark + records + 1;
    HIP_TRY(hipMemsetAsync(mark + records, 0, 4, stream));
    hipLaunchKernelGGL(sym_mark_kernel, grid_of(records), dim3(256), 0, stream, keys_b, (uint32_t)records, (uint32_t)n, a.mode == HNSWGPU_SYM_MUTUAL ? 1u : 0u,
                       mark);
    HIP_TRY(hipGetLastError());
    rc = exclusive_scan_u32(m_temp, mark, slot_of, records + 1, stream, err);
    if (rc != OK) return rc;
    uint64_t* d_offs = a.out_offsets;
    if (host) {
        HIP_TRY(m_offs.alloc((n + 1) * 8));
        d_offs = static_cast<uint64_t*>(m_offs.p);
    }
    hipLaunchKernelGGL(sym_offsets_kernel, grid_of(n + 1), dim3(256), 0, stream, keys_b, slot_of, (uint32_t)records, (uint32_t)n, d_offs);
    HIP_TRY(hipGetLastError());
    uint32_t total32 = 0;
    HIP_TRY(hipMemcpyAsync(&total32, slot_of + records, 4, hipMemcpyDeviceToHost, stream));  // the one read-back of the device entry
    if (host) HIP_TRY(hipMemcpyAsync(a.out_offsets, d_offs, (n + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    m_temp.release();
    const uint64_t total = total32;
    if (total > a.cap) {
        err = "the answers need " + std::to_string(total) + " slots, cap is " + std::to_string(a.cap);
        return HNSWGPU_ERR_CAPACITY;
    }
    if (total == 0) return OK;

    // the entries at their rows, every row sorted, decoded
    uint64_t *row_keys_in, *row_keys;
    uint32_t* row_bits;
    ScratchLayout lay;
    lay.arrays(total, row_keys_in, row_keys, row_bits);
    rc = alloc_layout("symmetric graph", m_row, lay, err);
    if (rc != OK) return rc;
    uint32_t* row_bits_in = vals_a;  // (free since the sort; total <= records)
    hipLaunchKernelGGL(sym_fill_kernel, grid_of(records), dim3(256), 0, stream, keys_b, vals_b, mark, slot_of, (uint32_t)records, row_keys_in, row_bits_in);
    HIP_TRY(hipGetLastError());
    const seg_iter_t seg(d_offs, SegBound{});
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, temp_bytes, row_keys_in, row_keys, row_bits_in, row_bits, (unsigned)total, (unsigned)n, seg, seg + 1, 0u,
                                                64u, stream));
    HIP_TRY(m_temp.alloc(std::max<size_t>(temp_bytes, 256)));
    HIP_TRY(rocprim::segmented_radix_sort_pairs(m_temp.p, temp_bytes, row_keys_in, row_keys, row_bits_in, row_bits, (unsigned)total, (unsigned)n, seg, seg + 1, 0u,
                                                64u, stream));
    SymSlots out{a.out_pos, a.out_ids, reinterpret_cast<uint32_t*>(a.out_dists), a.out_layer, a.out_rank};
    if (host) {
        // staged where the sorted records and the marks were (the fill has read them; the stream orders the kernels): 8 + 4 bytes
        // per record behind keys_b / vals_b, 8 behind keys_a, and total <= records
        out.ids = a.out_ids ? keys_b : nullptr;
        out.bits = vals_b;
        out.pos = reinterpret_cast<uint32_t*>(keys_a);
        out.rank = a.out_rank ? reinterpret_cast<int32_t*>(keys_a) + total : nullptr;
        out.layer = a.out_layer ? reinterpret_cast<uint8_t*>(row_keys_in) : nullptr;  // (the segmented sort's input: read before the decoding)
    }
    hipLaunchKernelGGL(sym_decode_kernel, grid_of(total), dim3(256), 0, stream, v, ord.d_order, row_keys, row_bits, (uint32_t)total, out);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(a.out_pos, out.pos, total * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(a.out_dists, out.bits, total * 4, hipMemcpyDeviceToHost, stream));
        if (a.out_ids) HIP_TRY(hipMemcpyAsync(a.out_ids, out.ids, total * 8, hipMemcpyDeviceToHost, stream));
        if (a.out_rank) HIP_TRY(hipMemcpyAsync(a.out_rank, out.rank, total * 4, hipMemcpyDeviceToHost, stream));
        if (a.out_layer) HIP_TRY(hipMemcpyAsync(a.out_layer, out.layer, total, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

}  // namespace hnswgpu
