// dbscan_screen_parts.hpp -- what the two screens of exact DBSCAN share: dbscan_screen.hip (the tile's queries resident in LDS, rows
// up to 1120 elements) and dbscan_screen_long.hip (queries and rows both streamed, rows up to 4096 elements).  The arguments of a
// screen kernel, the two-sided test (screen_band), the preparation of a chunk's points, the cut, the rerank, the capacities, and the
// driver: the two passes over chunks of positions, the routes, the
// fallback, the bounds matrix.  A unit names its screen kernel through a KIND:
//   static bool shape(int device, uint64_t dpad, DbscanScreenShape* s)   the workgroup for rows of dpad elements; false: not screened
//   static float coeff(int metric, uint64_t d)                           the coefficient of both bounds' error term
//   static const char* too_long()                                        the tail of the matrix entry's refusal
//   template <int PASS> static hipError_t launch(bool launch, int metric, const DbscanScreenShape& s, dim3 grid, hipStream_t, view, args)
//                                                                        the launch of one chunk -- and, launch == false, once per
//                                                                        call in front of the first: more LDS than the default limit
//                                                                        of a launch is said to the runtime per kernel
// Private: not installed, not part of the ABI; a unit includes it once.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_index.hpp"
// (the CSR validation kernels that come with the union-find have no caller in these units)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "union_find.hpp"
#pragma clang diagnostic pop
#include "dbscan_parts.hpp"
#include "exact_internal.hpp"
#include "exact_screen_parts.hpp"
#include "exact_tile.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

constexpr uint64_t DS_CAND_CAP = 2ull << 20;     // candidates of one chunk and pass: (query slot, flat row), 8 bytes each
constexpr uint64_t DS_QPAD_BYTES = 16ull << 20;  // padded queries of one chunk
constexpr uint32_t DS_RERANK_WG = 2048;          // workgroups of the rerank: they stride over the candidates
constexpr uint64_t DS_MATRIX_PAIRS = 1ull << 24; // the bounds matrix entries: nq * n at most
enum { PASS_BOUNDS = 2 };                        // beside PASS_COUNT and PASS_LINK: the store epilogue of the bounds matrix entries

struct DbscanScreenArgs {
    const float* qpad;      // [tiles * qt][dpad] the chunk's queries, zero padded (also behind the last query)
    const float* qn;        // [tiles * qt] their squared norms, plain f32
    const float* xn;        // [n] the rows' squared norms, plain f32
    const uint32_t* qpos;   // [tiles * qt] the position of the slot's query (COUNT, LINK)
    const float* cut;       // one word: what a bound is compared with -- eps, or, DistL2, sqrt_cut(eps)
    const uint32_t* rank;   // [n] position of flat id f (LINK)
    uint32_t* count;        // [n] by position (COUNT: added to)
    const uint8_t* core;    // [n] by position (LINK)
    const unsigned long long* cmask;  // [ceil(n / 64)] one bit per FLAT id (LINK)
    uint32_t* parent;       // [n] by position (LINK)
    uint32_t* cq;           // [cand_cap] a candidate's query slot in the chunk ...
    uint32_t* crow;         // ... and its flat row
    unsigned long long* ctr;  // the candidates of the chunk and pass so far: goes on counting past cand_cap
    float* out_lb;          // BOUNDS: [nq][n]
    float* out_ub;
    uint32_t cand_cap;
    uint32_t nq;            // queries of this chunk
    uint32_t dpad, nkc;     // elements of a padded query = KC * nkc
    uint32_t qt;            // queries of a tile = SQ * wavefronts of a workgroup
    uint32_t slab_rows;     // a multiple of 32 NT and of 64
    float cu;               // screen_coeff
    uint32_t zero_tail;     // DistCosine rows that carry their norm in their last 8 bytes: those two elements are no data
};

// The workgroup of a screen kernel at one row length (KIND::shape)
struct DbscanScreenShape {
    uint32_t waves;         // wavefronts of a workgroup
    uint32_t nt;            // accumulator tiles of a wavefront
    uint64_t qt;            // queries of a tile = SQ * waves
    uint64_t rows;          // rows of a staged block = 32 nt (64 or 128): a slab is a multiple
    uint64_t lds;           // bytes
};

// The operands of the two compares of a pair and whether the pair lies in the proved range.  lo: screen_lb -- DistL2: the value
// screen_lb takes the root of, by its operations in its order (+0 outside the range, as screen_lb has it) --; hi: screen_ub, DistL2:
// likewise in front of the root.  hi means nothing where ok is false.
template <int METRIC>
__device__ __forceinline__ void screen_band(float s, float nq, float nx, float cu, bool& ok, float& lo, float& hi) {
    ok = screen_proved(s, nq, nx);
    if constexpr (METRIC == DIST_L2) {
        const float w = nq + nx;
        const float t = w - 2.f * s;
        const float e = cu * w;
        lo = ok ? fmaxf(t - e, 0.f) : 0.f;
        hi = fmaxf(t + e, 0.f);
    } else {
        lo = screen_lb<METRIC>(s, nq, nx, cu);
        hi = screen_ub<METRIC>(s, nq, nx, cu);
    }
}

// the chunk's stored rows as queries, by position: slot qs holds the point of flat id order[qs] -- its first d elements zero padded,
// the plain f32 norm of exact_screen_xnorm_kernel, the f64 norm of prep_slot (exact_knn.hip), its position q0 + qs (behind the last:
// zeros and 0xFFFFFFFF)
__global__ void dbscan_screen_prep_kernel(DeviceIndexView ix, const uint32_t* __restrict__ order, uint32_t q0, uint32_t nq, uint32_t dpad, uint32_t n_slots,
                                          float* __restrict__ qpad, float* __restrict__ qn, double* __restrict__ qnorm, uint32_t* __restrict__ qpos) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= n_slots) return;
    const uint32_t live = qs < nq ? ix.d : 0u;
    const float* const src = ix.vec + (size_t)(qs < nq ? order[qs] : 0u) * ix.row_stride;
    float nf = 0.f;
    double s1 = 0.;
    for (uint32_t i = 0; i < dpad; ++i) {
        const float e = i < live ? src[i] : 0.f;
        const float sq = e * e;
        nf = nf + sq;
        s1 = s1 + (double)sq;
        qpad[(size_t)qs * dpad + i] = e;
    }
    qn[qs] = nf;
    qnorm[qs] = s1;
    qpos[qs] = qs < nq ? q0 + qs : 0xFFFFFFFFu;
}

// once per call: the value both bounds are compared with
__global__ void dbscan_cut_kernel(float eps, bool l2, float* __restrict__ cut) { *cut = l2 ? sqrt_cut(eps) : eps; }

struct DbscanRerankArgs {
    SlabArgs sa;            // tile_dist: qnorm (the crate's arithmetic, [slots]) and nrm2; rank
    const float* qpad;      // [slots][dpad]
    const uint32_t* qpos;   // [slots]
    const uint32_t* cq;     // the screen's candidates
    const uint32_t* crow;
    const unsigned long long* ctr;
    uint32_t cand_cap, dpad;
    float eps;
    uint32_t* count;        // COUNT
    const uint8_t* core;    // LINK
    uint32_t* parent;
    unsigned long long* best;
};

// One candidate per lane: its distance in the text of exact_row_chain.inc, one (query, row) chain instead of TQ, then the test of
// dbscan_slab_kernel and what it does with a hit.  A pass whose candidates outgrew the buffer does nothing: the host reads the counter.
template <int METRIC, int PASS>
__global__ __launch_bounds__(256) void dbscan_rerank_kernel(DeviceIndexView ix, DbscanRerankArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    const unsigned long long found = *a.ctr;
    if (found > (unsigned long long)a.cand_cap) return;
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
        if (!(v <= a.eps)) continue;  // (a NaN: no hit)
        const uint32_t pq = a.qpos[qs];
        if constexpr (PASS == PASS_COUNT) {
            atomicAdd(a.count + pq, 1u);
        } else {
            const uint32_t rk = a.sa.rank[flat];  // (the screen passes core rows only)
            if (a.core[pq] != 0) cc_unite(a.parent, pq, rk);
            else atomicMin(a.best + pq, (unsigned long long)make_key(v, rk));
        }
    }
}

// slabs of rows for `tiles` tiles of queries: enough workgroups to fill the device, whole blocks of rows, every slab from a multiple
// of 64 flat rows on (a block is 64 or 128 rows)
void dbscan_screen_slabs(const DbscanScreenShape& sh, uint64_t n, uint64_t tiles, uint64_t& slabs, uint64_t& slab_rows) {
    slabs = std::max<uint64_t>(1, std::min<uint64_t>((SCREEN_WG_TARGET + tiles - 1) / tiles, n / SCREEN_SLAB_ROWS));
    slab_rows = round_up((n + slabs - 1) / slabs, sh.rows);
    slabs = (n + slab_rows - 1) / slab_rows;
}

enum Route { ROUTE_DONE, ROUTE_UNSCREENED, ROUTE_OUTGROWN };

// Both entries.  The state of dbscan.hip; per pass and per chunk of positions: prep, screen, rerank; the chunks' counters come back once
// per pass.  Between the passes dbs_core_kernel, behind them dbscan_finish.  Waits for `stream` before it returns.  *route: ROUTE_DONE,
// or why the caller has to run the existing path instead (nothing of the caller's has been written then).  *pairs: the candidates of
// both passes, what went through the exact chain.
template <typename KIND>
int dbscan_screened_passes(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& c, bool host, hipStream_t stream, Route* route,
                           uint64_t* pairs, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t n = v.n, d = v.d;
    *route = ROUTE_UNSCREENED;
    const uint64_t dpad = round_up(d, KC);
    DbscanScreenShape sh{};
    if (!metric_has_screen(dev.dist()) || n < SCREEN_MIN_ROWS || !KIND::shape(dev.device(), dpad, &sh)) return OK;
    const uint64_t qt = sh.qt;

    const Knobs& kn = knobs();
    const uint64_t chunk_tiles = std::min<uint64_t>({(n + qt - 1) / qt, std::max<uint64_t>(1, DS_QPAD_BYTES / (qt * dpad * 4)), 65535});
    const uint64_t slots = chunk_tiles * qt, chunks = (n + slots - 1) / slots;
    // a chunk's candidates: the capacity -- never more than the chunk has pairs
    const uint64_t cand_cap = std::min<uint64_t>(kn.dbscan_screen_cap > 0 ? (uint64_t)kn.dbscan_screen_cap : DS_CAND_CAP, std::min(slots, n) * n);

    DbscanState s;
    unsigned long long *d_cmask, *d_ctr;
    uint32_t *d_cq, *d_crow, *d_qpos;
    float *d_qpad, *d_qn, *d_cut;
    double* d_qnorm;
    ScratchLayout lay;
    int rc = dbscan_state_layout(s, lay, n, host, c.out, stream, err);
    if (rc != OK) return rc;
    lay.array(d_cmask, (n + 63) / 64);
    lay.array(d_qpad, slots * dpad);
    lay.array(d_qn, slots);
    lay.array(d_qnorm, slots);
    lay.array(d_qpos, slots);
    lay.arrays(cand_cap, d_cq, d_crow);
    lay.array(d_ctr, 2 * chunks);  // one counter per (pass, chunk)
    lay.bytes(d_cut, 256);
    if (lay.size() > SCRATCH_BUDGET) return OK;  // (a very large index: not screened)
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "dbscan", err);
    if (!st) return ERR_DEVICE;
    const float* d_xn = nullptr;
    rc = row_norms(*st, v, stream, &d_xn, err);
    if (rc != OK) return rc;
    ScratchLease lease(st.get());
    rc = alloc_layout("dbscan", lease, lay, err);
    if (rc != OK) return rc;

    Drain drain{stream};  // whatever happens, nothing of this call is still running when the scratch block goes back to the pool

    rc = dbscan_state_init(s, n, stream, err);
    if (rc != OK) return rc;
    HIP_TRY(hipMemsetAsync(d_ctr, 0, 2 * chunks * 8, stream));
    hipLaunchKernelGGL(dbscan_cut_kernel, dim3(1), dim3(1), 0, stream, c.eps, dev.dist() == DIST_L2, d_cut);
    HIP_TRY(hipGetLastError());
    HIP_TRY(KIND::template launch<PASS_COUNT>(false, dev.dist(), sh, dim3(), stream, v, DbscanScreenArgs{}));
    HIP_TRY(KIND::template launch<PASS_LINK>(false, dev.dist(), sh, dim3(), stream, v, DbscanScreenArgs{}));
    const bool zero_tail = dev.dist() == DIST_COSINE && dev.side_norms() == nullptr;
    const uint32_t work_wg = (uint32_t)std::min<uint64_t>(DS_RERANK_WG, (cand_cap + 255) / 256);
    std::vector<unsigned long long> h_ctr(chunks);
    *pairs = 0;

    // one pass: every chunk of positions [q0, q0 + cq) prepared, screened against every slab, its candidates through the chain; then the
    // counters of the pass.  True in *outgrown: a chunk had more candidates than the buffer holds.
    auto pass = [&](bool link, bool* outgrown) -> int {
        unsigned long long* const ctr0 = d_ctr + (link ? chunks : 0);
        for (uint64_t k = 0; k < chunks; ++k) {
            const uint64_t q0 = k * slots, cq = std::min(slots, n - q0), tiles = (cq + qt - 1) / qt;
            const uint32_t n_slots = (uint32_t)(tiles * qt);
            uint64_t slabs, slab_rows;
            dbscan_screen_slabs(sh, n, tiles, slabs, slab_rows);
            hipLaunchKernelGGL(dbscan_screen_prep_kernel, grid_of(n_slots), dim3(256), 0, stream, v, st->order() + q0, (uint32_t)q0, (uint32_t)cq, (uint32_t)dpad,
                               n_slots, d_qpad, d_qn, d_qnorm, d_qpos);
            HIP_TRY(hipGetLastError());
            const DbscanScreenArgs a{d_qpad, d_qn, d_xn, d_qpos, d_cut, st->rank(), s.count, s.core, d_cmask, s.parent, d_cq, d_crow, ctr0 + k, nullptr, nullptr,
                                     (uint32_t)cand_cap, (uint32_t)cq, (uint32_t)dpad, (uint32_t)(dpad / KC), (uint32_t)qt, (uint32_t)slab_rows,
                                     KIND::coeff(dev.dist(), d), zero_tail ? 1u : 0u};
            const dim3 grid((uint32_t)slabs, (uint32_t)tiles);
            HIP_TRY(link ? KIND::template launch<PASS_LINK>(true, dev.dist(), sh, grid, stream, v, a)
                         : KIND::template launch<PASS_COUNT>(true, dev.dist(), sh, grid, stream, v, a));
            const DbscanRerankArgs r{SlabArgs{nullptr, d_qnorm, st->rank(), nullptr, dev.side_norms(), (uint32_t)cq, (uint32_t)((d + 3) / 4), (uint32_t)slab_rows, (uint32_t)slabs},
                                     d_qpad, d_qpos, d_cq, d_crow, ctr0 + k, (uint32_t)cand_cap, (uint32_t)dpad, c.eps, s.count, s.core, s.parent, s.best};
            HIP_TRY(for_screened_metric(dev.dist(), [&](auto m) {
                constexpr int M = decltype(m)::value;
                if (link) hipLaunchKernelGGL((dbscan_rerank_kernel<M, PASS_LINK>), dim3(work_wg), dim3(256), 0, stream, v, r);
                else hipLaunchKernelGGL((dbscan_rerank_kernel<M, PASS_COUNT>), dim3(work_wg), dim3(256), 0, stream, v, r);
            }));
        }
        HIP_TRY(hipMemcpyAsync(h_ctr.data(), ctr0, chunks * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *outgrown = false;
        for (uint64_t k = 0; k < chunks; ++k) {
            *pairs += std::min<uint64_t>(h_ctr[k], cand_cap);
            if (h_ctr[k] > cand_cap) *outgrown = true;
        }
        return OK;
    };
    bool outgrown = false;
    rc = pass(false, &outgrown);
    if (rc != OK) return rc;
    if (outgrown) { *route = ROUTE_OUTGROWN; return OK; }
    hipLaunchKernelGGL(dbs_core_kernel, grid_of(n), dim3(256), 0, stream, st->rank(), s.count, (uint32_t)n, 0u, c.min_samples, s.core, d_cmask);
    HIP_TRY(hipGetLastError());
    rc = pass(true, &outgrown);
    if (rc != OK) return rc;
    if (outgrown) { *route = ROUTE_OUTGROWN; return OK; }
    *route = ROUTE_DONE;
    return dbscan_finish(s, n, host, c.out, stream, err);
}

// A whole call behind KIND's screen.  stats (host memory, may be nullptr): {points answered through the screen, answered by the
// existing path because a buffer was outgrown, not screened, pairs that went through the exact chain}.
template <typename KIND>
int dbscan_screened_call(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& a, uint64_t* out_stats, bool host, void* stream,
                         std::string& err) {
    uint64_t own[4];
    uint64_t* const stats = out_stats ? out_stats : own;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    const uint64_t n = dev.view().n;
    Route route = ROUTE_UNSCREENED;
    {   // (the screened path's block is back in the pool before the existing path takes its own)
        DeviceGuard on(dev.device());
        HIP_TRY(on.status());
        const int rc = dbscan_screened_passes<KIND>(dev, origin_id, a, host, static_cast<hipStream_t>(stream), &route, stats + 3, err);
        if (route == ROUTE_DONE) stats[0] = n;
        if (rc != OK || route == ROUTE_DONE) return rc;
    }
    stats[route == ROUTE_OUTGROWN ? 1 : 2] = n;
    return exact_dbscan(dev, origin_id, a, host, stream, err);
}

// The device side of a bounds matrix entry (host buffers): KIND's screen kernel with a store epilogue
template <typename KIND>
int dbscan_bounds_matrix_call(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanBoundsArgs& a, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t n = v.n;
    if (!metric_has_screen(dev.dist())) { err = "dbscan bounds matrix: this distance has no screen (DistL2, DistDot, DistCosine have)"; return ERR_ARG; }
    if (a.nq * n > DS_MATRIX_PAIRS) { err = "dbscan bounds matrix: nq * n above 2^24 pairs"; return ERR_ARG; }
    if (a.nq == 0 || n == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t dpad = round_up(a.d, KC);
    DbscanScreenShape sh{};
    if (!KIND::shape(dev.device(), dpad, &sh)) { err = std::string("dbscan bounds matrix: rows too long ") + KIND::too_long(); return ERR_ARG; }
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "dbscan bounds matrix", err);
    if (!st) return ERR_DEVICE;
    const float* d_xn = nullptr;
    int rc = row_norms(*st, v, nullptr, &d_xn, err);
    if (rc != OK) return rc;
    const uint64_t tiles = (a.nq + sh.qt - 1) / sh.qt, slots = tiles * sh.qt;
    uint64_t slabs, slab_rows;
    dbscan_screen_slabs(sh, n, tiles, slabs, slab_rows);
    float *d_src, *d_qpad, *d_qn, *d_lb, *d_ub;
    double* d_qnorm;
    ScratchLayout lay;
    lay.array(d_src, a.nq * a.d);
    lay.array(d_qpad, slots * dpad);
    lay.array(d_qn, slots);
    lay.array(d_qnorm, slots);
    lay.arrays(a.nq * n, d_lb, d_ub);
    DevMem mem;
    rc = alloc_layout("dbscan bounds matrix", mem, lay, err);
    if (rc != OK) return rc;
    Drain drain{nullptr};
    HIP_TRY(hipMemcpyAsync(d_src, a.queries, a.nq * a.d * 4, hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(exact_screen_prep_kernel, grid_of(slots), dim3(256), 0, nullptr, d_src, (uint32_t)a.nq, (uint32_t)a.d, (uint32_t)dpad, (uint32_t)slots,
                       d_qpad, d_qn, d_qnorm);
    HIP_TRY(hipGetLastError());
    DbscanScreenArgs s{};
    s.qpad = d_qpad, s.qn = d_qn, s.xn = d_xn, s.out_lb = d_lb, s.out_ub = d_ub;
    s.nq = (uint32_t)a.nq, s.dpad = (uint32_t)dpad, s.nkc = (uint32_t)(dpad / KC), s.qt = (uint32_t)sh.qt, s.slab_rows = (uint32_t)slab_rows;
    s.cu = KIND::coeff(dev.dist(), a.d);
    s.zero_tail = dev.dist() == DIST_COSINE && dev.side_norms() == nullptr ? 1u : 0u;
    HIP_TRY(KIND::template launch<PASS_BOUNDS>(false, dev.dist(), sh, dim3(), nullptr, v, s));
    HIP_TRY(KIND::template launch<PASS_BOUNDS>(true, dev.dist(), sh, dim3((uint32_t)slabs, (uint32_t)tiles), nullptr, v, s));
    return copy_out({{a.out_lb, d_lb, a.nq * n * 4}, {a.out_ub, d_ub, a.nq * n * 4}}, true, nullptr, err);
}

}  // namespace
}  // namespace hnswgpu
