// dbscan.hip -- DBSCAN(eps, min_samples) on the device (gfx950 only): the device side of hnswdbs_exact(_device) and
// hnswdbs_csr(_device) of include/hnsw_mi355x_dbscan.h, which holds the contract (the entries and every check that needs no device
// are in capi.cpp).  DESIGN.md "DBSCAN".  No list of neighbours is built: a count per point, a union per close pair of core points,
// one nearest core point per point that is not core.
//   (exact_prep_rows)    the stored rows tiled as queries in POSITION order, chunk by chunk; each slot carries its position
//   dbscan_slab_kernel   <METRIC, PASS> the frame of exact_range_slab_kernel (exact_tile.hpp, exact_row_chain.inc): one wavefront per
//                        (tile of TQ queries, slab of rows), ONE ROW PER LANE.  COUNT: a ballot and a popcount per (query, 64 rows),
//                        at the end one integer atomic add per query into count[its position].  LINK: the 64 rows of a step are 64
//                        consecutive flat ids from a multiple of 64 on, their core mask is one aligned scalar load; a step where no
//                        core row lies in the slab is skipped before the chain.  A core query unites with every core row it hits
//                        (union_find.hpp), skipping rows whose parent is the query's root as last seen; a query that is not core
//                        lowers best[its position] to the smallest key {distance bits, position} of the core rows it hits.
//   dbs_csr_count_kernel / dbs_csr_link_kernel   (CSR) the same two steps, one thread per entry, its row by a binary search
//   dbs_core_kernel      core[v] = count[v] + add_self >= min_samples, by position; (exact) the core bitmap by FLAT ID
//   cc_compress_kernel, dbs_flag_kernel, (rocPRIM), dbs_answer_kernel   the finish of both forms: every parent its root; the flag
//                        "core and its own root"; its exclusive scan -- a root's cluster number, the last word is c --; labels,
//                        anchors and the optional outputs into the caller's arrays
// Only core points are ever united, and union_find.hpp hangs the larger root under the smaller: a tree's root is the smallest core
// position of its cluster, so the scan numbers the clusters as the contract does.  Integer atomics only: the answer is a function
// of the input alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "csr_intake.hpp"
#include "exact_internal.hpp"
#include "exact_tile.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"
#include "union_find.hpp"

namespace hnswgpu {
namespace {

constexpr uint64_t DBSCAN_TILE_BUDGET = 64ull << 20;  // bytes of tiled queries per chunk of tiles (the range search's)
constexpr unsigned long long BEST_NONE = ~0ull;        // behind every key: no core point in the set
enum { PASS_COUNT = 0, PASS_LINK = 1 };

typedef __attribute__((address_space(4))) const unsigned long long* umask_ptr_t;

struct DbscanSlabArgs : SlabArgs {
    float eps;
    const uint32_t* qpos;             // [tiles * TQ] the position of the slot's query (behind the last: 0xFFFFFFFF)
    uint32_t* count;                  // [n] by position.  COUNT: added to.
    const uint8_t* core;              // [n] by position (LINK)
    const unsigned long long* cmask;  // [ceil(n / 64)] one bit per FLAT id (LINK)
    uint32_t* parent;                 // [n] by position (LINK)
    unsigned long long* best;         // [n] by position (LINK)
};

// (exact_range_slab_kernel's cap of four waves per SIMD was measured for this loop shape)
#ifndef HNSW_DBSCAN_MAX_WAVES
#define HNSW_DBSCAN_MAX_WAVES 4
#endif
// per query of the tile its position, whether it is core and its root as last seen are wave-uniform
template <int METRIC, int PASS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(
    METRIC == DIST_JEFFREYS || METRIC == DIST_JENSENSHANNON ? 2 : (HNSW_DBSCAN_MAX_WAVES < 4 ? HNSW_DBSCAN_MAX_WAVES : 4), HNSW_DBSCAN_MAX_WAVES)))
void dbscan_slab_kernel(DeviceIndexView ix, DbscanSlabArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    const uint32_t lane = threadIdx.x;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const SlabTile T = slab_tile<METRIC>(ix, a, slab, tile);
    const uint32_t nvalid = T.nvalid, nchunk = a.nchunk;
    const float eps = a.eps;
    uint32_t cnt[TQ];   // COUNT: the hits so far
    uint32_t qp[TQ];    // LINK: the query's position
    uint32_t root[TQ];  // LINK: a root the query had (trees only merge: whatever hangs under it is in the query's tree)
    uint32_t qcore = 0u;  // LINK: bit t = query t is core
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        cnt[t] = 0u;
        if constexpr (PASS == PASS_LINK) {
            const uint32_t qs = tile * (uint32_t)TQ + ((uint32_t)t < nvalid ? (uint32_t)t : 0u);  // (the slots behind the last query never link)
            qp[t] = ((uword_ptr_t)a.qpos)[qs];
            root[t] = qp[t];
        }
    }
    if constexpr (PASS == PASS_LINK) {
        bool c = false;
        if (lane < nvalid) c = a.core[a.qpos[tile * (uint32_t)TQ + lane]] != 0;
        qcore = (uint32_t)__ballot(c);
    }

    for (uint32_t r0 = T.lo; r0 < T.hi; r0 += 64u) {
        uint32_t r;
        bool in;
        const bool ok = slab_row(T, r0, lane, nullptr, r, in);
        unsigned long long cm = ~0ull;
        if constexpr (PASS == PASS_LINK) {
            cm = ((umask_ptr_t)a.cmask)[r0 >> 6];  // (T.lo and the step are multiples of 64)
            if ((__ballot(ok) & cm) == 0ull) continue;  // (wave-uniform) no core row among these 64: nothing to unite with, no anchor
        }
#include "exact_row_chain.inc"
        const uint32_t rk = PASS == PASS_LINK ? a.rank[r] : 0u;
        const bool mine = ok && ((cm >> lane) & 1ull) != 0ull;
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            if ((uint32_t)t < nvalid) {
                const float v = tile_dist<METRIC>(a, tile * (uint32_t)TQ + (uint32_t)t, acc[t], s2);
                const bool hit = mine && v <= eps;  // (a NaN on either side: no hit)
                const unsigned long long m = __ballot(hit);
                if (m != 0ull) {
                    if constexpr (PASS == PASS_COUNT) {
                        cnt[t] += popc64(m);
                    } else if ((qcore >> t) & 1u) {
                        bool did = false;
                        if (hit && parent_of(a.parent, rk) != root[t]) {
                            cc_unite(a.parent, qp[t], rk);
                            did = true;
                        }
                        if (__ballot(did) != 0ull) {  // the query's root may have changed: one lane looks
                            uint32_t now = 0u;
                            if (lane == 0u) now = cc_find(a.parent, qp[t]);
                            root[t] = (uint32_t)__builtin_amdgcn_readfirstlane((int)now);
                        }
                    } else if (hit) {
                        atomicMin(a.best + qp[t], (unsigned long long)make_key(v, rk));
                    }
                }
            }
        }
    }
    if constexpr (PASS == PASS_COUNT) {
        if (lane < nvalid) {
            uint32_t c = 0;
#pragma unroll
            for (int t = 0; t < TQ; ++t)
                if (lane == (uint32_t)t) c = cnt[t];
            if (c != 0u) atomicAdd(a.count + a.qpos[tile * (uint32_t)TQ + lane], c);
        }
    }
}

hipError_t launch_dbscan_slab(int metric, bool link, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const DbscanSlabArgs& a) {
    return launch_for_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (link) hipLaunchKernelGGL((dbscan_slab_kernel<M, PASS_LINK>), grid, dim3(64), 0, stream, ix, a);
        else hipLaunchKernelGGL((dbscan_slab_kernel<M, PASS_COUNT>), grid, dim3(64), 0, stream, ix, a);
    });
}

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

// e's row in a checked CSR: offsets[row] <= e < offsets[row + 1].  Ends: hi - lo halves.
__device__ __forceinline__ uint32_t row_of_entry(const uint64_t* __restrict__ offsets, uint32_t n, uint32_t e) {
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= (uint64_t)e) lo = mid; else hi = mid;
    }
    return lo;
}
// entry e is in its row's set: dists == nullptr, or dists[e] <= eps as an ordered comparison
__device__ __forceinline__ bool entry_in(const float* __restrict__ dists, uint32_t e, float eps) {
    return dists == nullptr || dists[e] <= eps;
}

// one thread per entry e of a checked CSR
__global__ __launch_bounds__(256) void dbs_csr_count_kernel(const uint64_t* __restrict__ offsets, const float* __restrict__ dists, uint32_t n, uint32_t total,
                                                            float eps, uint32_t* count) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total || !entry_in(dists, e, eps)) return;
    atomicAdd(count + row_of_entry(offsets, n, e), 1u);
}

// one thread per entry e = (i, j): both core: unite; i not core and j core: j is a candidate of i
__global__ __launch_bounds__(256) void dbs_csr_link_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ cols,
                                                           const float* __restrict__ dists, uint32_t n, uint32_t total, float eps,
                                                           const uint8_t* __restrict__ core, uint32_t* parent, unsigned long long* best) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total || !entry_in(dists, e, eps)) return;
    const uint32_t j = cols[e];
    if (core[j] == 0) return;
    const uint32_t i = row_of_entry(offsets, n, e);
    if (core[i] != 0) {
        if (i != j) cc_unite(parent, i, j);
    } else {
        const float w = dists != nullptr ? dists[e] : 0.f;
        atomicMin(best + i, ((unsigned long long)dist_order_bits(w) << 32) | j);
    }
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

// What both forms keep for the length of a call, in the block of the form's own layout: 25 n bytes and the scan's temporary storage
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

// The finish of both forms; the unions and the keys are on the stream.  Roots, the clusters' numbers, c read back, the answer into
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

// Both index entries (capi.cpp refers to it weakly, capi_index.hpp): n >= 1.  Waits for `stream` before it returns.
int exact_dbscan(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& c, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const DeviceIndexView& v = dev.view();
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "dbscan", err);
    if (!st) return ERR_DEVICE;
    const uint64_t n = v.n, d = v.d;

    // the stored rows as queries, in position order: chunks of whole tiles under the budget, slabs cut for a chunk's tiles
    const uint64_t nchunk = (d + 3) / 4;
    const uint64_t per_tile = round_up(nchunk * TQ * 16, 256) + round_up(TQ * 8, 256) + round_up(TQ * 4, 256);
    const uint64_t chunk_tiles = std::min<uint64_t>({(n + TQ - 1) / TQ, std::max<uint64_t>(1, DBSCAN_TILE_BUDGET / per_tile), 65535});
    SlabPlan plan(n, d, std::min<uint64_t>(n, chunk_tiles * TQ));
    plan.cut();

    DbscanState s;
    unsigned long long* d_cmask;
    float* d_qt;
    double* d_qnorm;
    uint32_t* d_qpos;
    ScratchLayout lay;
    int rc = dbscan_state_layout(s, lay, n, host, c.out, stream, err);
    if (rc != OK) return rc;
    lay.array(d_cmask, (n + 63) / 64);
    plan.tiles(lay, chunk_tiles, d_qt, d_qnorm);
    lay.bytes(d_qpos, chunk_tiles * round_up(TQ * 4, 256));
    lay.skip(256);
    ScratchLease lease(st.get());
    rc = alloc_layout("dbscan", lease, lay, err);
    if (rc != OK) return rc;

    Drain drain{stream};  // whatever happens, nothing of this call is still running when the scratch block goes back to the pool

    rc = dbscan_state_init(s, n, stream, err);
    if (rc != OK) return rc;
    DbscanSlabArgs a{};
    static_cast<SlabArgs&>(a) = slab_args(*st, dev, plan, d_qt, d_qnorm, nullptr);
    a.eps = c.eps;
    a.qpos = d_qpos;
    a.count = s.count;
    a.core = s.core;
    a.cmask = d_cmask;
    a.parent = s.parent;
    a.best = s.best;
    // one pass: every chunk of positions [q0, q0 + cq) tiled (the slots' contiguous 4-byte positions: TQ * 4 = 64 bytes a tile, so
    // slot i of the chunk is word i) and run against every slab
    auto pass = [&](bool link) -> int {
        for (uint64_t q0 = 0; q0 < n; q0 += chunk_tiles * TQ) {
            const uint64_t cq = std::min<uint64_t>(chunk_tiles * TQ, n - q0);
            const uint32_t tiles = (uint32_t)((cq + TQ - 1) / TQ);
            HIP_TRY(exact_prep_rows(stream, v, st->order() + q0, st->rank(), cq, plan, tiles * (uint32_t)TQ, d_qt, d_qnorm, d_qpos));
            a.nq = (uint32_t)cq;
            HIP_TRY(launch_dbscan_slab(dev.dist(), link, dim3((uint32_t)plan.slabs, tiles), stream, v, a));
        }
        return OK;
    };
    rc = pass(false);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(dbs_core_kernel, grid_of(n), dim3(256), 0, stream, st->rank(), s.count, (uint32_t)n, 0u, c.min_samples, s.core, d_cmask);
    HIP_TRY(hipGetLastError());
    rc = pass(true);
    if (rc != OK) return rc;
    return dbscan_finish(s, n, host, c.out, stream, err);
}

// Both CSR entries: 1 <= n < 2^31.  host: every array is host memory and has passed the same checks on the host (capi.cpp).
int csr_dbscan(const CsrDbscanArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = use_device_ordinal("csr dbscan", a.device, err);
    if (rc != OK) return rc;
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    const uint64_t n = a.n;
    const DbscanArgs& c = a.call;
    CsrOnDevice csr;
    DevMem mem;
    DbscanState s;
    Drain drain{stream};
    rc = csr_intake("csr dbscan", n, a.offsets, a.cols, a.dists, host, a.dists != nullptr, stream, csr, err);
    if (rc != OK) return rc;
    const uint64_t total = csr.total;
    ScratchLayout lay;
    rc = dbscan_state_layout(s, lay, n, host, c.out, stream, err);
    if (rc != OK) return rc;
    rc = alloc_layout("csr dbscan", mem, lay, err);
    if (rc != OK) return rc;
    rc = dbscan_state_init(s, n, stream, err);
    if (rc != OK) return rc;
    if (total != 0) {
        hipLaunchKernelGGL(dbs_csr_count_kernel, grid_of(total), dim3(256), 0, stream, csr.offsets, csr.dists, (uint32_t)n, (uint32_t)total, c.eps, s.count);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(dbs_core_kernel, grid_of(n), dim3(256), 0, stream, static_cast<const uint32_t*>(nullptr), s.count, (uint32_t)n, a.add_self,
                       c.min_samples, s.core, static_cast<unsigned long long*>(nullptr));
    HIP_TRY(hipGetLastError());
    if (total != 0) {
        hipLaunchKernelGGL(dbs_csr_link_kernel, grid_of(total), dim3(256), 0, stream, csr.offsets, csr.cols, csr.dists, (uint32_t)n, (uint32_t)total, c.eps,
                           s.core, s.parent, s.best);
        HIP_TRY(hipGetLastError());
    }
    return dbscan_finish(s, n, host, c.out, stream, err);
}

}  // namespace hnswgpu
