// exact_range_screen.hip -- exact range search behind a matrix-core screen (gfx950 only): the device side of
// hnswxr_exact_range_search_batch(_device) of include/hnsw_mi355x_exact_range_screen.h (the entries and the argument checks are in
// capi.cpp).  The answers are those of exact_range.hip byte for byte; DESIGN.md section 15.14 holds the pipeline and the argument,
// section 15.13 the bound.  DistL2, DistDot and DistCosine.
//
//   exact_screen_prep_kernel   (exact_screen_parts.hpp) the queries of a chunk zero padded, their norms in both arithmetics
//   range_screen_kernel        one workgroup of W <= 4 wavefronts per (tile of 32 W queries, slab of rows): the data movement of
//                              exact_screen_kernel -- the tile's queries resident in LDS, the rows streamed through LDS 32 elements
//                              at a time, double buffered, one barrier per block -- with NT = 2 or 4 accumulator tiles a wavefront
//                              (32 queries x 32 NT rows: one read of the queries serves NT MFMAs).  Epilogue per accumulator
//                              register: is the pair's LOWER BOUND (screen_lb) at or below the query's radius?  A ballot; one
//                              atomic per ballot with bits reserves the slots, the lanes store (query slot, flat row).  No lists, no
//                              keys, no merge.
//   range_rerank_kernel        one candidate per lane through the exact chain (chain4, tile_dist: the bits of exact_range.hip); a
//                              hit leaves its key and counts for its query, a miss leaves KEY_NONE
//   exact_range_scan_kernel    (exact_range_parts.hpp) the counts of a chunk into the CSR offsets, carried from chunk to chunk
//   range_scatter_kernel       the hits' keys to offsets[q] + a cursor per query, in the call's key buffer
//   sort_segments, exact_range_decode_kernel   (exact_range_parts.hpp) once the total is known: every query's keys ascending, then
//                              ids, distances and p_ids
//
// A call whose candidates outgrow a chunk's buffer or whose answers outgrow the key buffer is answered by exact_range, whole.
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

// Accumulator tiles of a wavefront where the LDS holds the larger row blocks without costing a wavefront: 4 (32 queries x 128 rows)
// or 2 (32 x 64, the k-NN screen's).  RESULTS.md "Exact range search" has both figures.
#ifndef HNSW_RANGE_SCREEN_NT
#define HNSW_RANGE_SCREEN_NT 4
#endif

uint64_t range_screen_lds_bytes(uint64_t waves, uint64_t dpad, uint64_t nt) { return screen_lds_bytes(waves, dpad) + 2ull * (nt - 2) * 32 * RPITCH * 4; }

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

template <int METRIC, int NT>
__global__ __launch_bounds__(64 * MAX_WAVES) void range_screen_kernel(DeviceIndexView ix, RangeScreenArgs a) {
    constexpr uint32_t RBN = 32u * NT;  // rows of a staged block: NT tiles of 32
    constexpr uint32_t F4 = RBN * 8u;   // its float4s
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nthr = blockDim.x;
    const uint32_t half = lane >> 5, l32 = lane & 31u;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t qt = a.qt, dpad = a.dpad, nkc = a.nkc, qpitch = dpad + 4u;
    float* const qs = reinterpret_cast<float*>(lds_raw);  // [qt][qpitch]
    float* const rbuf = qs + (size_t)qt * qpitch;         // [2][RBN][RPITCH]
    float* const qnl = rbuf + 2u * RBN * RPITCH;          // [qt] the queries' norms
    float* const cutl = qnl + qt;                         // [qt] what a bound is compared with (screen_within)

    const uint32_t nvalid = a.nq - tile * qt < qt ? a.nq - tile * qt : qt;
    // the tile's queries: resident from here on
    {
        const float4* const src = reinterpret_cast<const float4*>(a.qpad + (size_t)tile * qt * dpad);
        const uint32_t c4n = dpad >> 2;
        for (uint32_t i = tid; i < qt * c4n; i += nthr) {
            const uint32_t q = i / c4n, c = i - q * c4n;
            *reinterpret_cast<float4*>(qs + (size_t)q * qpitch + 4u * c) = src[i];
        }
        for (uint32_t q = tid; q < qt; q += nthr) {
            const float rad = q < nvalid ? a.radius[tile * qt + q] : -1.f;
            qnl[q] = a.qn[tile * qt + q];
            cutl[q] = METRIC == DIST_L2 ? sqrt_cut(rad) : rad;
        }
    }
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t steps = ((hi - lo + RBN - 1u) / RBN) * nkc;  // (block of rows, chunk of elements), chunk fastest
    const uint32_t row_stride = ix.row_stride;

    // this thread's part of a staged block: float4 number i = tid + j * nthr of RBN x 8.  Rows behind the slab re-read its last row;
    // they are no candidates (epilogue).
    float4 pre[F4 / 64u];
    auto fetch = [&](uint32_t s) {
        const uint32_t blk = s / nkc, c = s - blk * nkc;
#pragma unroll
        for (uint32_t j = 0; j < F4 / 64u; ++j) {
            const uint32_t i = tid + j * nthr;
            if (i < F4) {
                const uint32_t r = lo + blk * RBN + (i >> 3), e = c * KC + 4u * (i & 7u);
                float4 v = *reinterpret_cast<const float4*>(ix.vec + (size_t)(r < hi ? r : hi - 1u) * row_stride + e);
                if (a.zero_tail != 0u && e + 4u == row_stride) { v.z = 0.f; v.w = 0.f; }
                pre[j] = v;
            }
        }
    };
    auto stage = [&](uint32_t s) {
        float* const dst = rbuf + (s & 1u) * (RBN * RPITCH);
#pragma unroll
        for (uint32_t j = 0; j < F4 / 64u; ++j) {
            const uint32_t i = tid + j * nthr;
            if (i < F4) *reinterpret_cast<float4*>(dst + (i >> 3) * RPITCH + 4u * (i & 7u)) = pre[j];
        }
    };

    v16f acc[NT];
#pragma unroll
    for (int tb = 0; tb < NT; ++tb)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[tb][v] = 0.f;
    bool mine = wave * SQ < nvalid;  // (wave-uniform) this wavefront has a query at all -- and the chunk's buffer still has room
    const float* const qrow = qs + (size_t)(wave * SQ + l32) * qpitch + 4u * half;

    fetch(0u);
    stage(0u);
    __syncthreads();
    for (uint32_t s = 0; s < steps; ++s) {
        if (s + 1u < steps) fetch(s + 1u);
        const uint32_t blk = s / nkc, c = s - blk * nkc;
        if (mine) {
            // 32 elements: four groups of 8.  A lane reads 4 consecutive elements of its query and of its NT rows (the lower 32 lanes
            // the group's first four, the upper 32 its last four); MFMA m of the group multiplies element m of both halves.
            const float* const b0 = rbuf + (s & 1u) * (RBN * RPITCH) + l32 * RPITCH + 4u * half;
            const float* const qa = qrow + c * KC;
#pragma unroll
            for (uint32_t g = 0; g < KC / 8u; ++g) {
                const float4 q4 = *reinterpret_cast<const float4*>(qa + 8u * g);
                float4 x[NT];
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) x[tb] = *reinterpret_cast<const float4*>(b0 + (uint32_t)tb * 32u * RPITCH + 8u * g);
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, x[tb].x, acc[tb], 0, 0, 0);
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, x[tb].y, acc[tb], 0, 0, 0);
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, x[tb].z, acc[tb], 0, 0, 0);
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, x[tb].w, acc[tb], 0, 0, 0);
            }
            if (c + 1u == nkc) {
                // Register v of an accumulator tile: row = this lane's (l32) of the tile, query 8 (v / 4) + 4 half + v % 4 of the
                // wavefront's 32.  Every lane is active here: lane 0 reserves the slots of a ballot's candidates.
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) {
                    const uint32_t r = lo + blk * RBN + 32u * (uint32_t)tb + l32;
                    const bool in = r < hi;
                    const uint32_t rc = in ? r : hi - 1u;
                    const float nx = a.xn[rc];
                    bool elig = in;
                    if (a.allow != nullptr) elig = in && ((a.allow[rc >> 5] >> (rc & 31u)) & 1u) != 0u;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const uint32_t ql = wave * SQ + 8u * ((uint32_t)v >> 2) + ((uint32_t)v & 3u) + 4u * half;
                        const bool cand = elig && ql < nvalid && screen_within<METRIC>(acc[tb][v], qnl[ql], nx, a.cu, cutl[ql]);
                        const unsigned long long m = __ballot(cand);
                        if (m != 0ull) {
                            unsigned long long base = 0ull;
                            if (lane == 0u) base = atomicAdd(a.ctr, (unsigned long long)popc64(m));
                            base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                            const unsigned long long p = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                            if (cand && p < (unsigned long long)a.cand_cap) {  // (past the buffer: dropped; the counter tells)
                                a.cq[p] = tile * qt + ql;
                                a.crow[p] = r;
                            }
                            // the buffer was full before this ballot: the call is the existing path's, and this wavefront only
                            // keeps the workgroup's barriers from here on (the counter is past the capacity and stays there)
                            if (base >= (unsigned long long)a.cand_cap) mine = false;
                        }
                    }
                }
#pragma unroll
                for (int tb = 0; tb < NT; ++tb)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[tb][v] = 0.f;
            }
        }
        if (s + 1u < steps) stage(s + 1u);
        __syncthreads();
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

// (kernel: &range_screen_kernel<M, NT>) the launch of one chunk -- and, launch == false, once per call in front of the first: more
// LDS than the default limit of a launch is said to the runtime per kernel
hipError_t range_screen(bool launch, int metric, uint32_t nt, dim3 grid, uint32_t waves, uint32_t lds, hipStream_t stream, const DeviceIndexView& ix,
                        const RangeScreenArgs& a) {
    hipError_t said = hipSuccess;
    const hipError_t e = for_screened_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (!launch) said = nt == 4u ? hipFuncSetAttribute(reinterpret_cast<const void*>(&range_screen_kernel<M, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                     : hipFuncSetAttribute(reinterpret_cast<const void*>(&range_screen_kernel<M, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        else if (nt == 4u) hipLaunchKernelGGL((range_screen_kernel<M, 4>), grid, dim3(64u * waves), lds, stream, ix, a);
        else hipLaunchKernelGGL((range_screen_kernel<M, 2>), grid, dim3(64u * waves), lds, stream, ix, a);
    });
    return said != hipSuccess ? said : e;
}

enum Route { ROUTE_DONE, ROUTE_UNSCREENED, ROUTE_OUTGROWN };

// Both entries.  Per block of queries (host buffers: at most 64 MB of them; device: the batch) and per chunk of tiles: prep, screen,
// rerank, scan, scatter; the offsets and the overflow word come back once per block.  Then, when the total fits cap and the key
// buffer, per block: sort and decode -- into the caller's arrays (device) or into a staging area that is copied out (host).  Waits
// for `stream` before it returns.  *route: ROUTE_DONE, or why the caller has to run the existing path instead (nothing of the
// caller's but out_offsets has been written then).  d_allowed: c.allowed on the device.
int range_screened_passes(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& c, bool host, const uint64_t* d_allowed,
                          hipStream_t stream, Route* route, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t nq = c.nq, d = c.d, n = v.n;
    const GraphRows out{c.out_ids, c.out_dists, c.out_layer, c.out_rank, nullptr};  // cap slots; no counts
    *route = ROUTE_UNSCREENED;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t dpad = round_up(d, KC);
    const uint64_t waves = nq != 0 && metric_has_screen(dev.dist()) && n >= SCREEN_MIN_ROWS ? screen_waves(dev.device(), dpad) : 0;
    if (waves == 0) return OK;
    int lds_limit = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev.device()));
    const uint64_t nt = HNSW_RANGE_SCREEN_NT == 4 && range_screen_lds_bytes(waves, dpad, 4) <= (uint64_t)lds_limit ? 4 : 2;
    const uint64_t qt = waves * SQ, rbn = 32 * nt;

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
    const uint32_t lds = (uint32_t)range_screen_lds_bytes(waves, dpad, nt);
    HIP_TRY(range_screen(false, dev.dist(), (uint32_t)nt, dim3(), (uint32_t)waves, lds, stream, v, RangeScreenArgs{}));
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
                                    (uint32_t)(dpad / KC), (uint32_t)qt, (uint32_t)slab_rows, screen_coeff(dev.dist(), d), zero_tail ? 1u : 0u};
            HIP_TRY(range_screen(true, dev.dist(), (uint32_t)nt, dim3((uint32_t)slabs, (uint32_t)tiles), (uint32_t)waves, lds, stream, v, a));
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

}  // namespace

// The device side of hnswxr_exact_range_search_batch(_device); capi.cpp holds the entries and every argument check.  stats (host
// memory, may be nullptr): {screened, answered by the existing path because a buffer was outgrown, not screened}.
int exact_range_screened(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, uint64_t* out_stats, bool host, void* stream,
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
        const int rc = range_screened_passes(dev, origin_id, a, host, host ? filter.d_allowed : a.allowed, static_cast<hipStream_t>(stream), &route, err);
        if (route == ROUTE_DONE) stats[0] = a.nq;
        if (rc != OK || route == ROUTE_DONE) return rc;
    }
    stats[route == ROUTE_OUTGROWN ? 1 : 2] = a.nq;
    return exact_range(dev, origin_id, a, host, stream, err);
}

}  // namespace hnswgpu
