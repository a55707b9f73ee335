// exact_range_screen_parts.hpp -- what the two screens of the exact range search share: exact_range_screen.hip (the tile's queries
// resident in LDS, rows up to 1120 elements) and exact_range_screen_long.hip (queries and rows both streamed, rows up to 4096
// elements).  The arguments of a screen kernel and its test (screen_within), the rerank and the scatter kernels, the capacities, and
// the driver: the loop over blocks of queries and chunks of tiles, the staging of host buffers, the routes, the fallback.  A unit
// names its screen kernel through a KIND:
//   static bool shape(int device, uint64_t dpad, RangeScreenShape* s)   the workgroup for rows of dpad elements; false: not screened
//   static float coeff(int metric, uint64_t d)                          the coefficient of the bound's error term
//   static hipError_t launch(bool launch, int metric, const RangeScreenShape& s, dim3 grid, hipStream_t, view, args)
//                                                                       the launch of one chunk -- and, launch == false, once per
//                                                                       call in front of the first: more LDS than the default limit
//                                                                       of a launch is said to the runtime per kernel
// Private: not installed, not part of the ABI; a unit includes it once.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_index.hpp"
#include "exact_internal.hpp"
#include "exact_range_parts.hpp"
#include "exact_screen_parts.hpp"
#include "exact_tile.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

// The default capacities (HNSWGPU_RANGE_SCREEN_CAP sets both).  With the staging of a host call -- 17 bytes an answer -- they keep
// a call's block within SCRATCH_BUDGET: 32 MB of candidates, 128 MB of keys, 136 MB of staged answers, 16 MB of padded queries.
constexpr uint64_t RS_CAND_CAP = 2ull << 20;     // candidates of one chunk: (query slot, flat row, key), 16 bytes each
constexpr uint64_t RS_KEY_CAP = 8ull << 20;      // answers of one call: two key buffers of 8 bytes each
constexpr uint64_t RS_QPAD_BYTES = 16ull << 20;  // padded queries of one chunk
constexpr uint32_t RS_RERANK_WG = 2048;          // workgroups of the rerank and of the scatter: they stride over the candidates

struct RangeScreenArgs {
    const float* qpad;      // [tiles * qt][dpad] the chunk's queries, zero padded (also behind the last query)
    const float* qn;        // [tiles * qt] their squared norms, plain f32
    const float* xn;        // [n] the rows' squared norms, plain f32
    const float* radius;    // [nq] the chunk's radii
    const uint32_t* allow;  // one bit per flat id, or nullptr: no filter
    uint32_t* cq;           // [cand_cap] a candidate's query slot in the chunk ...
    uint32_t* crow;         // ... and its flat row
    unsigned long long* ctr;  // the candidates of the chunk so far: goes on counting past cand_cap
    uint32_t cand_cap;
    uint32_t nq;            // queries of this chunk
    uint32_t dpad, nkc;     // elements of a padded query = KC * nkc
    uint32_t qt;            // queries of a tile = SQ * wavefronts of a workgroup
    uint32_t slab_rows;     // a multiple of 32 NT
    float cu;               // screen_coeff
    uint32_t zero_tail;     // DistCosine rows that carry their norm in their last 8 bytes: those two elements are no data
};

// The workgroup of a screen kernel at one row length (KIND::shape)
struct RangeScreenShape {
    uint32_t waves;         // wavefronts of a workgroup
    uint32_t nt;            // accumulator tiles of a wavefront
    uint64_t qt;            // queries of a tile = SQ * waves
    uint64_t rows;          // rows of a staged block = 32 nt: a slab is a multiple
    uint64_t lds;           // bytes
};

// screen_lb<METRIC>(s, nq, nx, cu) <= radius.  cut: the radius -- or, DistL2, sqrt_cut(radius) (exact_screen_parts.hpp), and the test is made in front of
// screen_lb's square root on the very value it would take the root of (DESIGN.md 15.14 has the equivalence).
template <int METRIC>
__device__ __forceinline__ bool screen_within(float s, float nq, float nx, float cu, float cut) {
    if constexpr (METRIC == DIST_L2) {
        const bool ok = nq >= NORM_LO && nq <= NORM_HI && nx >= NORM_LO && nx <= NORM_HI && fabsf(s) <= 3.0e38f;
        const float w = nq + nx;
        const float t = w - 2.f * s;
        const float x = fmaxf(t - cu * w, 0.f);
        return (ok ? x : 0.f) <= cut;
    } else {
        return screen_lb<METRIC>(s, nq, nx, cu) <= cut;
    }
}

struct RangeRerankArgs {
    SlabArgs sa;            // tile_dist: qnorm (the crate's arithmetic, [slots]) and nrm2; rank
    const float* qpad;      // [slots][dpad]
    const float* radius;    // [nq] the chunk's radii
    const uint32_t* cq;     // the screen's candidates
    const uint32_t* crow;
    const unsigned long long* ctr;
    uint32_t cand_cap, dpad;
    uint64_t* ckey;         // [cand_cap] per candidate its key, or KEY_NONE
    uint32_t* count;        // [slots] the hits of every query of the chunk (zeroed)
    uint32_t* overflow;     // sticky: a chunk's candidates outgrew the buffer
};

// One candidate per lane: its distance in the text of exact_row_chain.inc, one (query, row) chain instead of TQ.  A chunk whose
// candidates outgrew the buffer says so and does nothing more: the call is answered by the existing path.
template <int METRIC>
__global__ __launch_bounds__(256) void range_rerank_kernel(DeviceIndexView ix, RangeRerankArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    const unsigned long long found = *a.ctr;
    if (found > (unsigned long long)a.cand_cap) {
        if (blockIdx.x == 0u && threadIdx.x == 0u) *a.overflow = 1u;
        return;
    }
    const uint32_t nchunk = a.sa.nchunk;
    const bool norm_in_tail = METRIC == DIST_COSINE && a.sa.nrm2 == nullptr && nchunk * 4u == ix.row_stride;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < (uint32_t)found; p += gridDim.x * 256u) {
        const uint32_t qs = a.cq[p], flat = a.crow[p];
        const float4* const qrow = reinterpret_cast<const float4*>(a.qpad + (size_t)qs * a.dpad);
        const float* rowf = ix.vec + (size_t)flat * ix.row_stride;
        const float4* row = reinterpret_cast<const float4*>(rowf);
        double s2 = 0.;
        if constexpr (METRIC == DIST_COSINE)
            s2 = a.sa.nrm2 != nullptr ? a.sa.nrm2[flat] : *reinterpret_cast<const double*>(rowf + ix.row_stride - 2u);
        ACC acc = 0;
        for (uint32_t c = 0; c < nchunk; ++c) {
            float4 x = row[c];
            if (norm_in_tail && c + 1u == nchunk) { x.z = 0.f; x.w = 0.f; }
            chain4<METRIC, ACC>(acc, qrow[c], x);
        }
        const float v = tile_dist<METRIC>(a.sa, qs, acc, s2);
        const bool hit = v <= a.radius[qs];  // (a NaN on either side: no hit)
        a.ckey[p] = hit ? make_key(v, a.sa.rank[flat]) : KEY_NONE;
        if (hit) atomicAdd(a.count + qs, 1u);
    }
}

// The hits of a chunk into the call's keys: query q's at offs[q] + a cursor of its own (the chunk's counters, which the scan left at
// zero).  Keys are unique and every query's segment is sorted afterwards: the order of arrival reaches no output.
__global__ __launch_bounds__(256) void range_scatter_kernel(const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cq, const unsigned long long* __restrict__ ctr,
                                                           uint32_t cand_cap, const uint64_t* __restrict__ offs, uint32_t* __restrict__ cursor,
                                                           uint64_t* __restrict__ keys, uint64_t key_cap) {
    const unsigned long long found = *ctr;
    if (found > (unsigned long long)cand_cap) return;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < (uint32_t)found; p += gridDim.x * 256u) {
        const uint64_t key = ckey[p];
        if (key == KEY_NONE) continue;
        const uint32_t q = cq[p];
        const uint64_t at = offs[q] + atomicAdd(cursor + q, 1u);
        if (at < key_cap) keys[at] = key;  // (past the buffer: dropped; the total tells)
    }
}

enum Route { ROUTE_DONE, ROUTE_UNSCREENED, ROUTE_OUTGROWN };

// Both entries.  Per block of queries (host buffers: at most 64 MB of them; device: the batch) and per chunk of tiles: prep, screen,
// rerank, scan, scatter; the offsets and the overflow word come back once per block.  Then, when the total fits cap and the key
// buffer, per block: sort and decode -- into the caller's arrays (device) or into a staging area that is copied out (host).  Waits
// for `stream` before it returns.  *route: ROUTE_DONE, or why the caller has to run the existing path instead (nothing of the
// caller's but out_offsets has been written then).  d_allowed: c.allowed on the device.
template <typename KIND>
int range_screened_passes(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& c, bool host, const uint64_t* d_allowed,
                          hipStream_t stream, Route* route, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t nq = c.nq, d = c.d, n = v.n;
    const GraphRows out{c.out_ids, c.out_dists, c.out_layer, c.out_rank, nullptr};  // cap slots; no counts
    *route = ROUTE_UNSCREENED;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t dpad = round_up(d, KC);
    RangeScreenShape sh{};
    if (!(nq != 0 && metric_has_screen(dev.dist()) && n >= SCREEN_MIN_ROWS && KIND::shape(dev.device(), dpad, &sh))) return OK;
    const uint64_t qt = sh.qt, rbn = sh.rows;

    const Knobs& kn = knobs();
    const uint64_t key_budget = kn.range_screen_cap > 0 ? (uint64_t)kn.range_screen_cap : RS_KEY_CAP;
    const uint64_t block_q = host ? std::max<uint64_t>(1, std::min<uint64_t>(nq, (64ull << 20) / (d * 4 + 12))) : nq;
    uint64_t chunk_tiles = std::min<uint64_t>({(block_q + qt - 1) / qt, std::max<uint64_t>(1, RS_QPAD_BYTES / (qt * dpad * 4)), 65535});
    if (kn.range_screen_tiles > 0) chunk_tiles = std::min<uint64_t>(chunk_tiles, (uint64_t)kn.range_screen_tiles);
    const uint64_t slots = chunk_tiles * qt;
    // a chunk's candidates: the capacity -- never more than the chunk has pairs
    const uint64_t cand_cap = std::min<uint64_t>(kn.range_screen_cap > 0 ? (uint64_t)kn.range_screen_cap : RS_CAND_CAP, std::min(slots, nq) * n);
    // the call's keys: the budget -- never more than there are pairs or than the caller has room for (a count-only call: none)
    const uint64_t all_pairs = nq > 0xFFFFFFFFull / n ? 0xFFFFFFFFull : nq * n;
    const uint64_t key_cap = std::min<uint64_t>({key_budget, all_pairs, c.cap});
    size_t temp_bytes = 0;
    if (key_cap != 0) HIP_TRY(sort_segments(nullptr, temp_bytes, nullptr, nullptr, (uint32_t)key_cap, (uint32_t)block_q, nullptr, 0, stream));

    uint32_t *d_allow = nullptr, *d_cq, *d_crow, *d_count, *d_flag;
    float *d_qpad, *d_qn;
    double* d_qnorm;
    unsigned long long* d_ctr;
    uint64_t *d_ckey, *d_keys_a, *d_keys_b;
    void* d_temp;
    GraphRows staged{};
    ScratchLayout lay;
    if (d_allowed != nullptr) lay.array(d_allow, (n + 31) / 32);
    lay.array(d_qpad, slots * dpad);
    lay.array(d_qn, slots);
    lay.array(d_qnorm, slots);
    lay.arrays(cand_cap, d_cq, d_crow);
    lay.array(d_ckey, cand_cap);
    lay.array(d_count, slots);
    lay.bytes(d_ctr, 256);
    lay.bytes(d_flag, 256);
    lay.arrays(key_cap, d_keys_a, d_keys_b);
    if (host) lay.arrays(key_cap, staged.ids, staged.dists, staged.rank, staged.layer);
    if (lay.size() > SCRATCH_BUDGET) return OK;  // (a bitmap of a very large index, a hook: not screened)
    lay.bytes(d_temp, round_up(temp_bytes, 256));
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "exact range search", err);
    if (!st) return ERR_DEVICE;
    const float* d_xn = nullptr;
    int rc = row_norms(*st, v, stream, &d_xn, err);
    if (rc != OK) return rc;
    ScratchLease lease(st.get());
    rc = alloc_layout("exact range search", lease, lay, err);
    if (rc != OK) return rc;

    DevMem m_q, m_rad, m_off;
    if (host) {
        HIP_TRY(m_q.alloc(block_q * d * 4));
        HIP_TRY(m_rad.alloc(block_q * 4));
        HIP_TRY(m_off.alloc((block_q + 1) * 8));
    }
    // the offsets on the host: the caller's array, or a copy of it
    std::vector<uint64_t> off_copy;
    if (!host) off_copy.resize(nq + 1);
    uint64_t* const h_off = host ? c.out_offsets : off_copy.data();
    h_off[0] = 0;

    // whatever happens, nothing of this call is still running when the scratch block goes back to the pool
    Drain drain{stream};

    if (d_allow != nullptr) HIP_TRY(launch_allow_bitmap(stream, v.origin_id, v.n, d_allowed, c.n_allowed, d_allow));
    HIP_TRY(hipMemsetAsync(d_flag, 0, 4, stream));
    HIP_TRY(KIND::launch(false, dev.dist(), sh, dim3(), stream, v, RangeScreenArgs{}));
    const bool zero_tail = dev.dist() == DIST_COSINE && dev.side_norms() == nullptr;
    const uint32_t work_wg = (uint32_t)std::min<uint64_t>(RS_RERANK_WG, (cand_cap + 255) / 256);
    const bool one_block = block_q >= nq;
    const float* dq = c.queries;
    const float* dr = c.radii;
    uint64_t* doff = c.out_offsets;
    for (uint64_t b0 = 0; b0 < nq; b0 += block_q) {
        const uint64_t bq = std::min(block_q, nq - b0);
        if (host) {
            HIP_TRY(hipMemcpyAsync(m_q.p, c.queries + b0 * d, bq * d * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(m_rad.p, c.radii + b0, bq * 4, hipMemcpyHostToDevice, stream));
            dq = static_cast<const float*>(m_q.p);
            dr = static_cast<const float*>(m_rad.p);
            doff = static_cast<uint64_t*>(m_off.p);
        }
        for (uint64_t q0 = 0; q0 < bq; q0 += slots) {
            const uint64_t cq = std::min(slots, bq - q0), tiles = (cq + qt - 1) / qt;
            const uint32_t n_slots = (uint32_t)(tiles * qt);
            // slabs of rows: enough workgroups to fill the device, whole blocks of rows
            uint64_t slabs = std::max<uint64_t>(1, std::min<uint64_t>((SCREEN_WG_TARGET + tiles - 1) / tiles, n / SCREEN_SLAB_ROWS));
            const uint64_t slab_rows = round_up((n + slabs - 1) / slabs, rbn);
            slabs = (n + slab_rows - 1) / slab_rows;
            HIP_TRY(hipMemsetAsync(d_ctr, 0, 8, stream));
            HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)n_slots * 4, stream));
            hipLaunchKernelGGL(exact_screen_prep_kernel, grid_of(n_slots), dim3(256), 0, stream, dq + q0 * d, (uint32_t)cq, (uint32_t)d, (uint32_t)dpad, n_slots,
                               d_qpad, d_qn, d_qnorm);
            HIP_TRY(hipGetLastError());
            const RangeScreenArgs a{d_qpad, d_qn, d_xn, dr + q0, d_allow, d_cq, d_crow, d_ctr, (uint32_t)cand_cap, (uint32_t)cq, (uint32_t)dpad,
                                    (uint32_t)(dpad / KC), (uint32_t)qt, (uint32_t)slab_rows, KIND::coeff(dev.dist(), d), zero_tail ? 1u : 0u};
            HIP_TRY(KIND::launch(true, dev.dist(), sh, dim3((uint32_t)slabs, (uint32_t)tiles), stream, v, a));
            const RangeRerankArgs r{SlabArgs{nullptr, d_qnorm, st->rank(), nullptr, dev.side_norms(), (uint32_t)cq, (uint32_t)((d + 3) / 4), (uint32_t)slab_rows, (uint32_t)slabs},
                                    d_qpad, dr + q0, d_cq, d_crow, d_ctr, (uint32_t)cand_cap, (uint32_t)dpad, d_ckey, d_count, d_flag};
            HIP_TRY(for_screened_metric(dev.dist(), [&](auto m) {
                hipLaunchKernelGGL((range_rerank_kernel<decltype(m)::value>), dim3(work_wg), dim3(256), 0, stream, v, r);
            }));
            hipLaunchKernelGGL(exact_range_scan_kernel, dim3(1), dim3(1024), 0, stream, d_count, (uint32_t)cq, 1u, doff + q0, q0 == 0, h_off[b0]);
            HIP_TRY(hipGetLastError());
            if (key_cap != 0) {
                hipLaunchKernelGGL(range_scatter_kernel, dim3(work_wg), dim3(256), 0, stream, d_ckey, d_cq, d_ctr, (uint32_t)cand_cap, doff + q0, d_count, d_keys_a,
                                   key_cap);
                HIP_TRY(hipGetLastError());
            }
        }
        uint32_t outgrown = 0;
        HIP_TRY(hipMemcpyAsync(h_off + b0 + 1, doff + 1, bq * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&outgrown, d_flag, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (outgrown != 0) { *route = ROUTE_OUTGROWN; return OK; }
    }
    const uint64_t total = h_off[nq];
    *route = ROUTE_DONE;
    if (total > c.cap) {
        err = "the answers need " + std::to_string(total) + " slots, cap is " + std::to_string(c.cap);
        return HNSWGPU_ERR_CAPACITY;
    }
    if (total == 0 || out.ids == nullptr) return OK;
    if (total > key_cap) { *route = ROUTE_OUTGROWN; return OK; }

    // ---- sort and decode
    if (!out.layer) staged.layer = nullptr;  // (what the caller does not ask for is not decoded)
    if (!out.rank) staged.rank = nullptr;
    for (uint64_t b0 = 0; b0 < nq; b0 += block_q) {
        const uint64_t bq = std::min(block_q, nq - b0), hits = h_off[b0 + bq] - h_off[b0];
        if (hits == 0) continue;
        if (!one_block) HIP_TRY(hipMemcpyAsync(doff, h_off + b0, (bq + 1) * 8, hipMemcpyHostToDevice, stream));
        size_t need = 0;
        HIP_TRY(sort_segments(nullptr, need, d_keys_a + h_off[b0], d_keys_b, (uint32_t)hits, (uint32_t)bq, doff, h_off[b0], stream));
        if (need > temp_bytes) { err = "internal error: the sort's temporary storage"; return ERR_DEVICE; }
        HIP_TRY(sort_segments(d_temp, need, d_keys_a + h_off[b0], d_keys_b, (uint32_t)hits, (uint32_t)bq, doff, h_off[b0], stream));
        const GraphRows mine = rows_at(out, h_off[b0], 1);  // the block's slots of the caller's arrays
        const GraphRows& to = host ? staged : mine;
        hipLaunchKernelGGL(exact_range_decode_kernel, dim3((uint32_t)((hits + 255) / 256)), dim3(256), 0, stream, v, d_keys_b, (uint32_t)hits, st->order(), to.ids,
                           to.dists, to.layer, to.rank);
        HIP_TRY(hipGetLastError());
        if (host) {
            rc = copy_rows_out(mine, staged, hits, 0, stream, err);
            if (rc != OK) return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// A whole call behind KIND's screen.  stats (host memory, may be nullptr): {screened, answered by the existing path because a buffer
// was outgrown, not screened}.
template <typename KIND>
int range_screened_call(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, uint64_t* out_stats, bool host, void* stream,
                        std::string& err) {
    uint64_t own[3];
    uint64_t* const stats = out_stats ? out_stats : own;
    stats[0] = stats[1] = stats[2] = 0;
    Route route = ROUTE_UNSCREENED;
    {   // (the screened path's block is back in the pool before the existing path takes its own)
        DeviceGuard on(dev.device());
        HIP_TRY(on.status());
        FilterUpload filter;
        if (host) {
            const int rc = filter.put(a.allowed, a.n_allowed, err);
            if (rc != OK) return rc;
        }
        const int rc = range_screened_passes<KIND>(dev, origin_id, a, host, host ? filter.d_allowed : a.allowed, static_cast<hipStream_t>(stream), &route, err);
        if (route == ROUTE_DONE) stats[0] = a.nq;
        if (rc != OK || route == ROUTE_DONE) return rc;
    }
    stats[route == ROUTE_OUTGROWN ? 1 : 2] = a.nq;
    return exact_range(dev, origin_id, a, host, stream, err);
}

}  // namespace
}  // namespace hnswgpu
