// spanning_forest.hip -- the minimum spanning forest of a graph on the device (gfx950 only): the device side of
// hnswgpu_graph_spanning_forest(_device) and hnswgpu_csr_spanning_forest(_device) of include/hnsw_mi355x.h (the entries and every
// check that needs no device are in capi.cpp).  DESIGN.md "Minimum spanning forest".
//
// Boruvka over the union-find of union_find.hpp, integer atomics only.  The edges {lo < hi, weight bits} are brought into the strict
// total order (order bits of the weight, lo, hi) ONCE; from then on an edge's index is its rank and every comparison is a u32 min:
//   msf_core_kernel     (index, core_k >= 1) one thread per vertex: the stored distance of slot min(core_k, counts[v]) - 1 of row v of D
//                       (core_of_rows of graph_internal.hpp: cluster_predict.hip's core distances too)
//   msf_mark_kernel     (index) one thread per sorted edge record of symmetric_graph.hip: the head of a run of equal (row, col) with
//                       row < col is a pair {lo, hi}; its FWD record carries d(lo->hi), its REV record d(hi->lo).  UNION keeps every
//                       pair, MUTUAL the pairs with both records.
//   (rocPRIM)           an exclusive scan of the marks: the pair's place in the edge list, which is in (lo, hi) order like the records
//   msf_pairs_kernel    (index) one thread per record: a marked one writes lo, hi and the weight -- min (UNION) or max (MUTUAL) of the
//                       directions, then the max with core(lo), core(hi)
//   msf_entries_kernel  (CSR) one thread per entry e: its row by a binary search in the offsets, the key (lo, hi) and the weight bits
//   (rocPRIM)           (CSR) a radix sort of the entries by (lo, hi); msf_unpack_kernel takes the keys apart again.  Self-loops stay
//                       in the list: no round ever picks one.
//   msf_keys_kernel     one thread per edge: the order bits of its weight, and its own number
//   (rocPRIM)           a STABLE radix sort by the order bits: the list is in (order bits, lo, hi) order, the value is where the edge was
//   msf_gather_kernel   one thread per rank: the ends of the edge of that rank; flag = 0
//   msf_init_kernel     parent[v] = v, best[v] = NONE
//   a round, at most ceil(log2 n) + 1 times:
//     msf_pick_kernel     one thread per rank e: the roots of its ends (parent[] is compressed: one load each); if they differ,
//                         best[root] = min(best[root], e) for both (an atomic min, behind a load that lets a loser skip it)
//     msf_hook_kernel     one thread per vertex: a root with a best edge flags it, unites its ends, clears best and counts itself
//     cc_compress_kernel  parent[v] = its root
//     the count is read back: 0 ends the loop
//   (rocPRIM)           an exclusive scan of the flags: a forest edge's place in the answer, and n - c
//   msf_answer_kernel   one thread per rank: a flagged edge writes lo, hi and the stored bits of its weight
// Why the rounds are right: under a strict total order the lightest edge leaving a component is in THE minimum spanning forest, and
// the edges picked in one round have no cycle (on a cycle of picks the heaviest edge was picked by neither of its sides).  So every
// flagged edge is a forest edge, every unite joins two trees, and cc_unite's invariant holds as in graph_components.hip.  Repeated
// pairs need no removal: the lighter copy, or the lower-ranked of equal copies, wins the min, and the other copy joins nothing later.
// Why they end: every component that still has an outgoing edge hooks, so their number at least halves per round; after
// ceil(log2 n) rounds at most one is left, and the next round counts 0.  The bound is hard: a round past it is an internal error.
// No wavefront waits on another; the answer is a function of the edge list alone.
#include <hip/hip_runtime.h>

#include <algorithm>
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

constexpr uint32_t NONE = 0xFFFFFFFFu;  // no best edge (an edge's rank is below it: at most 2^32 - 1 edges)

// one thread per vertex: core[v] = the bits of slot min(core_k, counts[v]) - 1 of row v, +0 for an empty row
__global__ __launch_bounds__(256) void msf_core_kernel(const float* __restrict__ dists, const uint32_t* __restrict__ counts, uint32_t k, uint32_t core_k,
                                                      uint32_t n, uint32_t* __restrict__ core) {
    const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    uint32_t c = counts[v];
    if (c > k) c = k;  // (a slot of the row, whatever the count holds)
    if (c > core_k) c = core_k;
    core[v] = c == 0u ? 0u : __float_as_uint(dists[v * k + (c - 1u)]);
}

// Record t as a pair of the undirected graph: true iff it is the head of a run of equal (row, col) with row < col < n that `mutual`
// keeps.  has_fwd / has_rev: the run's FWD record (lo -> hi, at t) and its REV record (hi -> lo, at t or t + 1).
__device__ __forceinline__ bool pair_at(const uint64_t* __restrict__ keys, uint32_t records, uint32_t n, uint32_t mutual, uint32_t t, uint32_t& lo,
                                        uint32_t& hi, bool& has_fwd, bool& has_rev) {
    const uint64_t key = keys[t];
    lo = (uint32_t)(key >> 33);
    hi = (uint32_t)(key >> 1);
    if (lo >= hi || hi >= n) return false;
    if (t != 0u && (keys[t - 1u] >> 1) == (key >> 1)) return false;  // not the head of its run
    has_fwd = (key & FLAG_REV) == 0ull;
    has_rev = !has_fwd || (t + 1u < records && keys[t + 1u] == (key | FLAG_REV));
    return mutual == 0u || (has_fwd && has_rev);
}

// one thread per sorted record
__global__ __launch_bounds__(256) void msf_mark_kernel(const uint64_t* __restrict__ keys, uint32_t records, uint32_t n, uint32_t mutual,
                                                      uint32_t* __restrict__ mark) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= records) return;
    uint32_t lo, hi;
    bool f, r;
    mark[t] = pair_at(keys, records, n, mutual, t, lo, hi, f, r) ? 1u : 0u;
}

// one thread per sorted record: a marked one is edge slot_of[t].  core == nullptr: no core distances.
__global__ __launch_bounds__(256) void msf_pairs_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ slot_of, uint32_t records, uint32_t n, uint32_t mutual,
                                                       const uint32_t* __restrict__ core, uint32_t* __restrict__ e_lo, uint32_t* __restrict__ e_hi,
                                                       uint32_t* __restrict__ e_bits) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= records) return;
    uint32_t lo, hi;
    bool has_fwd, has_rev;
    if (!pair_at(keys, records, n, mutual, t, lo, hi, has_fwd, has_rev)) return;
    uint32_t w = vals[t];  // the one direction there is, or lo -> hi
    if (has_fwd && has_rev) {
        const uint32_t back = vals[t + 1u], ow = dist_order_bits(__uint_as_float(w)), ob = dist_order_bits(__uint_as_float(back));
        if (mutual != 0u ? ob > ow : ob < ow) w = back;  // (a tie keeps lo -> hi)
    }
    if (core != nullptr) {  // max(pair, core(lo), core(hi)); a tie keeps the earlier of the three
        const uint32_t cl = core[lo], ch = core[hi];
        if (dist_order_bits(__uint_as_float(cl)) > dist_order_bits(__uint_as_float(w))) w = cl;
        if (dist_order_bits(__uint_as_float(ch)) > dist_order_bits(__uint_as_float(w))) w = ch;
    }
    const uint32_t to = slot_of[t];
    e_lo[to] = lo;
    e_hi[to] = hi;
    e_bits[to] = w;
}

// one thread per entry e of a checked CSR: offsets[0] = 0 <= e < total = offsets[n], the offsets ascend, every col < n
__global__ __launch_bounds__(256) void msf_entries_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ cols,
                                                         const float* __restrict__ dists, uint32_t n, uint32_t total, uint64_t* __restrict__ keys,
                                                         uint32_t* __restrict__ bits) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    uint32_t lo = 0u, hi = n;  // offsets[lo] <= e < offsets[hi]; ends: hi - lo halves
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= (uint64_t)e) lo = mid; else hi = mid;
    }
    const uint32_t r = lo, c = cols[e];
    keys[e] = ((uint64_t)(r < c ? r : c) << 32) | (r < c ? c : r);
    bits[e] = dists != nullptr ? __float_as_uint(dists[e]) : 0u;
}

// one thread per sorted entry
__global__ __launch_bounds__(256) void msf_unpack_kernel(const uint64_t* __restrict__ keys, uint32_t m, uint32_t* __restrict__ e_lo,
                                                        uint32_t* __restrict__ e_hi) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= m) return;
    e_lo[e] = (uint32_t)(keys[e] >> 32);
    e_hi[e] = (uint32_t)keys[e];
}

// one thread per edge of the (lo, hi)-ordered list
__global__ __launch_bounds__(256) void msf_keys_kernel(const uint32_t* __restrict__ e_bits, uint32_t m, uint32_t* __restrict__ okey, uint32_t* __restrict__ self) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= m) return;
    okey[e] = dist_order_bits(__uint_as_float(e_bits[e]));
    self[e] = e;
}

// one thread per rank: from[e] < m is where the edge of rank e stands in the (lo, hi)-ordered list
__global__ __launch_bounds__(256) void msf_gather_kernel(const uint32_t* __restrict__ from, const uint32_t* __restrict__ e_lo,
                                                        const uint32_t* __restrict__ e_hi, uint32_t m, uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                                        uint32_t* __restrict__ flag) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e > m) return;
    flag[e] = 0u;  // (m + 1 flags: the scan's total is behind the last)
    if (e == m) return;
    const uint32_t f = from[e];
    a[e] = e_lo[f];
    b[e] = e_hi[f];
}

__global__ __launch_bounds__(256) void msf_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ best, uint32_t n) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    parent[v] = v;
    best[v] = NONE;
}

// one thread per rank e; a[e], b[e] < n.  parent[] is compressed and nothing hooks here: parent[v] is v's root.
__global__ __launch_bounds__(256) void msf_pick_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t m,
                                                      const uint32_t* __restrict__ parent, uint32_t* best) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= m) return;
    const uint32_t ra = parent[a[e]], rb = parent[b[e]];
    if (ra == rb) return;
    // best[] only falls during this kernel, so a value at or below e, however old, says that e cannot win: most threads skip the
    // atomic (ranks ascend with the thread number), which otherwise meet at the few roots of a late round
    if (__hip_atomic_load(best + ra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > e) atomicMin(best + ra, e);
    if (__hip_atomic_load(best + rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > e) atomicMin(best + rb, e);
}

// one thread per vertex: best[v] is NONE or a rank below m (set for roots only)
__global__ __launch_bounds__(256) void msf_hook_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n, uint32_t* parent,
                                                      uint32_t* __restrict__ best, uint32_t* __restrict__ flag, uint32_t* __restrict__ hooked) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    uint32_t e = NONE;
    if (v < n) e = best[v];
    if (e != NONE) {
        best[v] = NONE;
        flag[e] = 1u;  // (two roots that picked the same edge write the same 1)
        cc_unite(parent, a[e], b[e]);
    }
    const uint64_t did = __ballot(e != NONE);
    if (did != 0ull && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)did) - 1u) atomicAdd(hooked, (uint32_t)__popcll(did));
}

#include "union_find_compress.inc"

// one thread per rank: a flagged edge is edge slot_of[e] of the answer
__global__ __launch_bounds__(256) void msf_answer_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ from,
                                                        const uint32_t* __restrict__ e_bits, const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ slot_of, uint32_t m, uint32_t cap, uint32_t* __restrict__ out_a,
                                                        uint32_t* __restrict__ out_b, uint32_t* __restrict__ out_w) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= m || flag[e] == 0u) return;
    const uint32_t to = slot_of[e];
    if (to >= cap) return;  // (a forest of n vertices has at most n - 1 edges; the host checks the total)
    out_a[to] = a[e];
    out_b[to] = b[e];
    out_w[to] = e_bits[from[e]];  // the stored bits: a -0 or a NaN's payload comes back as the graph holds it
}

// ceil(log2 n) + 1: the rounds a forest of n >= 2 vertices can take, the one that counts 0 included
uint32_t round_bound(uint64_t n) {
    uint32_t bits = 0;
    while (bits < 63 && (1ull << bits) < n) ++bits;
    return bits + 1;
}

// The edge list in (lo, hi) order, m >= 0 edges in device memory, every end below n; n >= 2.  Ranks the edges, runs the rounds and
// writes the answer.  host: the out arrays are host memory.  Waits for the stream.
int forest_of_edges(uint64_t n, uint64_t m, const uint32_t* e_lo, const uint32_t* e_hi, const uint32_t* e_bits, bool host, uint32_t* out_a,
                    uint32_t* out_b, float* out_w, uint64_t* out_n, hipStream_t stream, std::string& err) {
    if (m == 0) {  // no edge: every vertex its own tree
        HIP_TRY(hipStreamSynchronize(stream));
        *out_n = 0;
        return OK;
    }
    const uint32_t bound = round_bound(n);
    DevMem mem, m_temp, m_out;
    Drain drain{stream};
    // m + 1 words each (flag and its scan stand where the two okeys stood), then n words each, then a word per round
    uint32_t *okey_in, *okey_out, *self, *from, *a, *b, *parent, *best, *mark, *hooked;
    ScratchLayout lay;
    lay.arrays(m + 1, okey_in, okey_out, self, from, a, b);
    lay.arrays(n, parent, best, mark);
    lay.array(hooked, bound);
    int rc = alloc_layout("spanning forest", mem, lay, err);
    if (rc != OK) return rc;
    uint32_t* flag = okey_in;      // (free once the sort is done)
    uint32_t* slot_of = okey_out;  // (its keys are never read)

    // rank
    hipLaunchKernelGGL(msf_keys_kernel, grid_of(m), dim3(256), 0, stream, e_bits, (uint32_t)m, okey_in, self);
    HIP_TRY(hipGetLastError());
    rc = radix_sort_pairs(m_temp, okey_in, okey_out, self, from, (size_t)m, 32u, stream, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(msf_gather_kernel, grid_of(m + 1), dim3(256), 0, stream, from, e_lo, e_hi, (uint32_t)m, a, b, flag);
    HIP_TRY(hipGetLastError());

    // rounds
    hipLaunchKernelGGL(msf_init_kernel, grid_of(n), dim3(256), 0, stream, parent, best, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(hooked, 0, (uint64_t)bound * 4, stream));
    bool done = false;
    for (uint32_t round = 0; round < bound && !done; ++round) {
        hipLaunchKernelGGL(msf_pick_kernel, grid_of(m), dim3(256), 0, stream, a, b, (uint32_t)m, parent, best);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(msf_hook_kernel, grid_of(n), dim3(256), 0, stream, a, b, (uint32_t)n, parent, best, flag, hooked + round);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(cc_compress_kernel, grid_of(n), dim3(256), 0, stream, parent, (uint32_t)n, mark);
        HIP_TRY(hipGetLastError());
        uint32_t count = 0;
        HIP_TRY(hipMemcpyAsync(&count, hooked + round, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        done = count == 0;
    }
    if (!done) {
        err = "spanning forest: components still hook after " + std::to_string(bound) + " rounds over " + std::to_string(n) + " vertices";
        return ERR_FORMAT;
    }

    // the flagged edges, in rank order
    m_temp.release();
    rc = exclusive_scan_u32(m_temp, flag, slot_of, m + 1, stream, err);
    if (rc != OK) return rc;
    uint32_t edges = 0;
    HIP_TRY(hipMemcpyAsync(&edges, slot_of + m, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (edges >= n) {
        err = "spanning forest: " + std::to_string(edges) + " edges among " + std::to_string(n) + " vertices";
        return ERR_FORMAT;
    }
    if (edges == 0) {
        *out_n = 0;
        return OK;
    }
    uint32_t* d_a = out_a;
    uint32_t* d_b = out_b;
    uint32_t* d_w = reinterpret_cast<uint32_t*>(out_w);
    if (host) {
        ScratchLayout staged;
        staged.arrays(edges, d_a, d_b, d_w);
        rc = alloc_layout("spanning forest", m_out, staged, err);
        if (rc != OK) return rc;
    }
    hipLaunchKernelGGL(msf_answer_kernel, grid_of(m), dim3(256), 0, stream, a, b, from, e_bits, flag, slot_of, (uint32_t)m, edges, d_a, d_b, d_w);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(out_a, d_a, (uint64_t)edges * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(out_b, d_b, (uint64_t)edges * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(out_w, d_w, (uint64_t)edges * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    *out_n = edges;
    return OK;
}

}  // namespace

// graph_internal.hpp: this unit's core distances, and cluster_predict.hip's
int core_of_rows(const float* dists, const uint32_t* counts, uint64_t k, uint64_t core_k, uint64_t n, uint32_t* core, void* stream, std::string& err) {
    hipLaunchKernelGGL(msf_core_kernel, grid_of(n), dim3(256), 0, static_cast<hipStream_t>(stream), dists, counts, (uint32_t)k, (uint32_t)core_k, (uint32_t)n,
                       core);
    HIP_TRY(hipGetLastError());
    return OK;
}

// Both index entries (capi.cpp refers to it weakly, capi_index.hpp): n >= 2, core_k <= k.  Waits for `stream` before it returns.
int graph_spanning_forest(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ForestArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const DeviceIndexView& v = dev.view();
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t n = v.n, k = a.k;  // (n k <= 2^30: checked by the entries)
    const uint32_t mutual = a.mode == HNSWGPU_SYM_MUTUAL ? 1u : 0u;
    SortedRecords rec;
    DevMem m_core, m_temp, m_edges;
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)
    GraphOrder ord;
    int rc = graph_order(dev, origin_id, ord, err);
    if (rc != OK) return rc;
    uint32_t* core = nullptr;
    if (a.core_k != 0) {  // the core distances come from D itself: it is kept until they are read
        StagedGraph d;
        rc = sorted_edge_records_keeping(dev, origin_id, ord, k, a.ef, stream_v, rec, d, err);
        if (rc != OK) return rc;
        HIP_TRY(m_core.alloc(round_up(n * 4, 256)));
        core = static_cast<uint32_t*>(m_core.p);
        rc = core_of_rows(d.dists, d.counts, k, a.core_k, n, core, stream_v, err);
        if (rc != OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream));  // (D is released at the brace)
    } else {
        rc = sorted_edge_records(dev, origin_id, ord, k, a.ef, stream_v, rec, err);
        if (rc != OK) return rc;
    }
    const uint64_t records = rec.records;
    const uint64_t* keys = static_cast<const uint64_t*>(rec.keys_b.p);
    const uint32_t* vals = static_cast<const uint32_t*>(rec.vals_b.p);
    rec.vals_a.release();  // (the sort's other half of the values: not needed here)
    // marks and their scan, where the sort's other half of the keys stood (records * 8 + 256 bytes: two arrays of records + 1 words)
    uint32_t* mark = static_cast<uint32_t*>(rec.keys_a.p);
    uint32_t* slot_of = mark + records + 1;
    HIP_TRY(hipMemsetAsync(mark + records, 0, 4, stream));
    hipLaunchKernelGGL(msf_mark_kernel, grid_of(records), dim3(256), 0, stream, keys, (uint32_t)records, (uint32_t)n, mutual, mark);
    HIP_TRY(hipGetLastError());
    rc = exclusive_scan_u32(m_temp, mark, slot_of, records + 1, stream, err);
    if (rc != OK) return rc;
    uint32_t m32 = 0;
    HIP_TRY(hipMemcpyAsync(&m32, slot_of + records, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    m_temp.release();
    const uint64_t m = m32;
    if (m > records / 2) {
        err = "spanning forest: " + std::to_string(m) + " pairs out of " + std::to_string(records) + " records";
        return ERR_FORMAT;
    }
    uint32_t *e_lo, *e_hi, *e_bits;
    ScratchLayout lay;
    lay.arrays(std::max<uint64_t>(m, 1), e_lo, e_hi, e_bits);
    rc = alloc_layout("spanning forest", m_edges, lay, err);
    if (rc != OK) return rc;
    if (m != 0) {
        hipLaunchKernelGGL(msf_pairs_kernel, grid_of(records), dim3(256), 0, stream, keys, vals, slot_of, (uint32_t)records, (uint32_t)n, mutual, core, e_lo,
                           e_hi, e_bits);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    rec.keys_a.release();  // the records are in the edge list
    rec.keys_b.release();
    rec.vals_b.release();
    m_core.release();
    return forest_of_edges(n, m, e_lo, e_hi, e_bits, host, a.out_a, a.out_b, a.out_w, a.out_n, stream, err);
}

// Both CSR entries: 2 <= n < 2^31.  host: every array is host memory and has passed the same checks on the host (capi.cpp).
int csr_spanning_forest(const CsrForestArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = use_device_ordinal("csr spanning forest", a.device, err);
    if (rc != OK) return rc;
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    const uint64_t n = a.n;
    CsrOnDevice csr;
    DevMem m_keys, m_temp, m_edges;
    Drain drain{stream};
    rc = csr_intake("csr spanning forest", n, a.offsets, a.cols, a.dists, host, a.dists != nullptr, stream, csr, err);
    if (rc != OK) return rc;
    const uint64_t m = csr.total;
    if (m == 0) return forest_of_edges(n, 0, nullptr, nullptr, nullptr, host, a.out_a, a.out_b, a.out_w, a.out_n, stream, err);
    // the entries as (lo, hi) keys with their bits, sorted by key
    uint64_t *keys_in, *keys_out;
    uint32_t *bits_in, *e_lo, *e_hi, *e_bits;
    ScratchLayout keyed, edges;
    keyed.arrays(m, keys_in, keys_out, bits_in);
    edges.arrays(m, e_lo, e_hi, e_bits);
    rc = alloc_layout("csr spanning forest", m_keys, keyed, err);
    if (rc != OK) return rc;
    rc = alloc_layout("csr spanning forest", m_edges, edges, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(msf_entries_kernel, grid_of(m), dim3(256), 0, stream, csr.offsets, csr.cols, csr.dists, (uint32_t)n, (uint32_t)m, keys_in, bits_in);
    HIP_TRY(hipGetLastError());
    unsigned end_bit = 33;  // hi below n in the low word, lo below n above it
    while (end_bit < 64 && (n >> (end_bit - 32)) != 0) ++end_bit;
    rc = radix_sort_pairs(m_temp, keys_in, keys_out, bits_in, e_bits, (size_t)m, end_bit, stream, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(msf_unpack_kernel, grid_of(m), dim3(256), 0, stream, keys_out, (uint32_t)m, e_lo, e_hi);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    m_keys.release();
    m_temp.release();
    csr.mem.release();
    return forest_of_edges(n, m, e_lo, e_hi, e_bits, host, a.out_a, a.out_b, a.out_w, a.out_n, stream, err);
}

}  // namespace hnswgpu
