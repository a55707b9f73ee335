// dbscan_parts.hpp -- what the two exact DBSCAN units share around their two passes over the pairs: dbscan.hip (every pair through the
// f32 chain, twice) and dbscan_screen.hip (a two-sided matrix-core screen, the chain on the band).  The state of a call and its
// layout, its initialisation, the core flags and the core bitmap between the passes, and the finish: roots, the clusters' numbers,
// labels and anchors.  Private: not installed, not part of the ABI; a unit includes it once, behind exact_tile.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "exact_internal.hpp"
#include "rocprim_host.hpp"
#include "union_find.hpp"

namespace hnswgpu {
namespace {

constexpr unsigned long long BEST_NONE = ~0ull;        // behind every key: no core point in the set
enum { PASS_COUNT = 0, PASS_LINK = 1 };

typedef __attribute__((address_space(4))) const unsigned long long* umask_ptr_t;

// parent[v] = v, best[v] = none, count[v] = 0
__global__ __launch_bounds__(256) void dbs_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ count, unsigned long long* __restrict__ best,
                                                       uint32_t n) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    parent[v] = v;
    count[v] = 0u;
    best[v] = BEST_NONE;
}

// One thread per row f of the index (rank != nullptr; position rank[f]) or per vertex f (rank == nullptr; position f): count += add_self,
// the core flag by position and, cmask != nullptr, the core bitmap by f -- a wavefront's 64 rows are one aligned word
__global__ __launch_bounds__(256) void dbs_core_kernel(const uint32_t* __restrict__ rank, uint32_t* __restrict__ count, uint32_t n, uint32_t add_self,
                                                       uint64_t min_samples, uint8_t* __restrict__ core, unsigned long long* __restrict__ cmask) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    bool c = false;
    if (f < n) {
        const uint32_t v = rank != nullptr ? rank[f] : f;
        const uint32_t k = count[v] + add_self;  // (a row's entries, offsets[n] < 2^32 at most, or n rows: the sum with add_self may wrap only at 2^32 - 1 entries in one row)
        c = (uint64_t)k >= min_samples;
        count[v] = k;
        core[v] = c ? 1 : 0;
    }
    const unsigned long long m = __ballot(c);
    if (cmask != nullptr && (threadIdx.x & 63u) == 0u && f < n) cmask[f >> 6] = m;
}

#include "union_find_compress.inc"

// mark[v] (v is a root) &= core[v]: the roots of the clusters
__global__ __launch_bounds__(256) void dbs_flag_kernel(const uint8_t* __restrict__ core, uint32_t n, uint32_t* __restrict__ mark) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n && core[v] == 0) mark[v] = 0u;
}

// one thread per vertex; parent[v] is v's root, number_of[r] the cluster of root r
__global__ __launch_bounds__(256) void dbs_answer_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ number_of,
                                                         const uint8_t* __restrict__ core, const uint32_t* __restrict__ count,
                                                         const unsigned long long* __restrict__ best, uint32_t n, int32_t* __restrict__ out_label,
                                                         uint8_t* __restrict__ out_core, uint32_t* __restrict__ out_count, uint32_t* __restrict__ out_anchor) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const bool c = core[v] != 0;
    uint32_t anchor = v;
    if (!c) {
        const unsigned long long b = best[v];
        anchor = b == BEST_NONE ? 0xFFFFFFFFu : (uint32_t)b;
    }
    int32_t label = -1;
    if (anchor < n) label = (int32_t)number_of[parent[anchor]];
    out_label[v] = label;
    if (out_core) out_core[v] = c ? 1 : 0;
    if (out_count) out_count[v] = count[v];
    if (out_anchor) out_anchor[v] = anchor < n ? anchor : 0xFFFFFFFFu;
}

// What every form keeps for the length of a call, in the block of the form's own layout: 25 n bytes and the scan's temporary storage
// (the host form: the staged labels and anchors besides; core and count are copied out as they stand)
struct DbscanState {
    uint32_t *parent = nullptr, *count = nullptr, *mark = nullptr, *number_of = nullptr;
    unsigned long long* best = nullptr;
    uint8_t* core = nullptr;
    void* temp = nullptr;
    size_t temp_bytes = 0;
    int32_t* stage_label = nullptr;
    uint32_t* stage_anchor = nullptr;
};
int dbscan_state_layout(DbscanState& s, ScratchLayout& lay, uint64_t n, bool host, const DbscanOut& out, hipStream_t stream, std::string& err) {
    HIP_TRY(rocprim::exclusive_scan(nullptr, s.temp_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u, (size_t)(n + 1),
                                    rocprim::plus<uint32_t>(), stream));
    lay.arrays(n, s.parent, s.count);
    lay.array(s.best, n);
    lay.array(s.core, n);
    lay.arrays(n + 1, s.mark, s.number_of);
    lay.bytes(s.temp, round_up(std::max<size_t>(s.temp_bytes, 256), 256));
    if (host) {
        lay.array(s.stage_label, n);
        if (out.anchor) lay.array(s.stage_anchor, n);
    }
    return OK;
}
int dbscan_state_init(const DbscanState& s, uint64_t n, hipStream_t stream, std::string& err) {
    hipLaunchKernelGGL(dbs_init_kernel, grid_of(n), dim3(256), 0, stream, s.parent, s.count, s.best, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return OK;
}

// The finish of every form; the unions and the keys are on the stream.  Roots, the clusters' numbers, c read back, the answer into
// the caller's arrays (host: through the staging).  Waits for the stream.
int dbscan_finish(const DbscanState& s, uint64_t n, bool host, const DbscanOut& out, hipStream_t stream, std::string& err) {
    HIP_TRY(hipMemsetAsync(s.mark + n, 0, 4, stream));
    hipLaunchKernelGGL(cc_compress_kernel, grid_of(n), dim3(256), 0, stream, s.parent, (uint32_t)n, s.mark);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dbs_flag_kernel, grid_of(n), dim3(256), 0, stream, s.core, (uint32_t)n, s.mark);
    HIP_TRY(hipGetLastError());
    size_t need = s.temp_bytes;
    HIP_TRY(rocprim::exclusive_scan(s.temp, need, static_cast<const uint32_t*>(s.mark), s.number_of, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), stream));
    uint32_t c = 0;
    HIP_TRY(hipMemcpyAsync(&c, s.number_of + n, 4, hipMemcpyDeviceToHost, stream));  // the one read-back
    HIP_TRY(hipStreamSynchronize(stream));
    if (c > n) {
        err = "dbscan: " + std::to_string(c) + " clusters among " + std::to_string(n) + " vertices";
        return ERR_FORMAT;
    }
    hipLaunchKernelGGL(dbs_answer_kernel, grid_of(n), dim3(256), 0, stream, s.parent, s.number_of, s.core, s.count, s.best, (uint32_t)n,
                       host ? s.stage_label : out.label, host ? nullptr : out.core, host ? nullptr : out.count, host ? s.stage_anchor : out.anchor);
    HIP_TRY(hipGetLastError());
    if (host) {
        const int rc = copy_out({{out.label, s.stage_label, n * 4}, {out.core, s.core, n}, {out.count, s.count, n * 4}, {out.anchor, s.stage_anchor, n * 4}},
                                true, stream, err);
        if (rc != OK) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(stream));
    }
    *out.out_n = c;
    return OK;
}

}  // namespace
}  // namespace hnswgpu
