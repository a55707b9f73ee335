// exact_screen_knn.hpp -- what the two screens of the exact k-NN share: exact_screen.hip (the tile's queries resident in LDS, rows up
// to 1120 elements) and exact_screen_long.hip (queries and rows both streamed, rows up to 4096 elements).  The arguments of a screen
// kernel, the insertion into a (query, slab) list, the rerank kernel with its certificate, the cut of a call, and the driver: the loop
// over chunks of tiles, the fallback, the staging of host buffers, the matrix of bounds.  A unit names its screen kernel through a
// KIND:
//   static uint64_t waves(int device, uint64_t dpad, bool self)   wavefronts of a workgroup for rows of dpad elements; 0: not screened
//   static uint64_t lds_bytes(uint64_t waves, uint64_t dpad, bool self)
//   static constexpr uint64_t ROWS                        rows of a staged block: a slab is a multiple
//   static float coeff(int metric, uint64_t d)            the coefficient of the bound's error term
//   static const char* too_long()                         the tail of the matrix entry's refusal
//   template <bool MATRIX> static hipError_t launch(int metric, dim3 grid, uint32_t waves, uint32_t lds, hipStream_t, view, args)
// self / args.self != nullptr: the kernel's SELF variant, whose queries are stored points read from the replica's own rows and never
// their own candidates -- the k-NN graph of the stored points (screened_graph_call).
// Private: not installed, not part of the ABI; a unit includes it once, behind exact_screen_parts.hpp and exact_list.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <vector>

#include "capi_index.hpp"
#include "exact_internal.hpp"
#include "exact_list.hpp"
#include "exact_screen_parts.hpp"
#include "exact_tile.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

// How many keys a (query, slab) list holds beyond k.  A query is certified when fewer than this many rows outside its answer have a
// lower bound at or below its k-th distance.  The value rests on an ESTIMATE of how dense the candidates are near the k-th distance
// (well below one row for 10^6 uniform points at d = 128) that nobody has measured on real data; k = 10 gives lists
// of 64 keys, one step of list_insert.
constexpr uint32_t SCREEN_MARGIN = 54;
constexpr uint32_t SCREEN_MAX_C = 4096;       // longer lists: the call runs the existing path
constexpr uint64_t SCREEN_MATRIX_PAIRS = 1ull << 24;  // hnswxs_screen_matrix: nq * n at most

struct ScreenArgs {
    const float* qpad;      // [tiles * qt][dpad] the chunk's queries, zero padded (also behind the last query)
    const float* qn;        // [tiles * qt] their squared norms, plain f32
    const float* xn;        // [n] the rows' squared norms, plain f32
    const uint32_t* rank;   // [n] position of flat id f in ascending (DataId, flat id) order
    const uint32_t* allow;  // one bit per flat id, or nullptr: no filter
    uint64_t* lists;        // [tiles][n_slabs][qt][cap] ascending keys
    uint32_t* lens;         // [tiles][n_slabs][qt]
    float* out_lb;          // MATRIX: [nq][n], the bound of every pair
    uint32_t nq;            // queries of this chunk
    uint32_t dpad, nkc;     // elements of a padded query = KC * nkc
    uint32_t qt;            // queries of a tile = SQ * wavefronts of a workgroup
    uint32_t slab_rows;     // a multiple of RB
    uint32_t n_slabs;       // <= MAX_SLABS
    uint32_t cap;           // C
    float cu;               // screen_coeff
    uint32_t zero_tail;     // DistCosine rows that carry their norm in their last 8 bytes: those two elements are no data
    const uint32_t* self;   // SELF: [nq] the chunk's queries are the stored points of these flat ids; qpad and qn are not read
};

// SELF (the k-NN graph of the stored points, hnsw_mi355x_exact_graph_screen.h): query slot q of a chunk is the point of flat id
// self[q], and a slot behind the chunk's last query names no point
constexpr uint32_t NO_SELF = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t self_slot(const uint32_t* __restrict__ self, uint32_t q, uint32_t nq) { return q < nq ? self[q] : NO_SELF; }
// Four elements of a stored point brought as a query: elements e .. e + 3 of the row of flat id f, the first d of the row and zeros
// behind them -- what exact_screen_prep_kernel writes for the point's vector, without the copy.  The row's own padding (zeros, or a
// DistCosine norm in its last 8 bytes) lies behind element d - 1 and never gets here.  e < round_up(d, 32) <= row_stride.
__device__ __forceinline__ v4f self_query4(const DeviceIndexView& ix, uint32_t f, uint32_t e) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (f != NO_SELF && e < ix.d) {
        v = *reinterpret_cast<const v4f*>(ix.vec + (size_t)f * ix.row_stride + e);
        if (e + 1u >= ix.d) v.y = 0.f;
        if (e + 2u >= ix.d) v.z = 0.f;
        if (e + 3u >= ix.d) v.w = 0.f;
    }
    return v;
}

// the keys of the lanes in `mask` into the list of query ql of this wavefront's workgroup (wave-uniform but for `key`)
__device__ __forceinline__ void screen_insert(uint64_t* list, uint64_t* thr, uint32_t* len, uint32_t ql, uint32_t cap, uint64_t key, uint64_t mask) {
    ListState s{len[ql], thr[ql]};
    s = list_insert<false>(list, cap, s, key, mask);
    if ((threadIdx.x & 63u) == 0u) {
        len[ql] = s.len;
        thr[ql] = s.thr;
    }
    wave_lds_fence();
}

struct RerankArgs {
    SlabArgs sa;            // tile_dist: qnorm (the crate's arithmetic, [slots]) and nrm2
    const float* qpad;      // [slots][dpad]
    const uint64_t* lists;  // the screen's
    const uint32_t* lens;
    const uint32_t* order;  // [n] the inverse of rank
    uint32_t dpad, qt, n_slabs, cap, k, sort_n;  // sort_n: the power of two >= cap
    uint32_t q0;            // the chunk's first query in the call
    GraphRows out;          // the chunk's rows of the caller's arrays
    uint32_t* fb_list;      // the call's queries that are not certified ...
    uint32_t* fb_count;     // ... and how many
    const uint32_t* self;   // SELF: [cq] ScreenArgs::self; qpad is not read
};

// One wavefront per query.  Merge: lane s walks the list of slab s, the smallest head is the next candidate -- min(total, C) of them,
// 64 at a time one per lane, each through the exact chain at once.  Certified: total < C (no list was full and the merge dropped
// nothing: every eligible row is a candidate), or the bound in the C-th merged key is greater, as an f32, than the exact k-th distance
// (every row that a list or the merge dropped has a key behind that one, so a distance above the cut; a NaN k-th distance is behind
// every bound: not certified).
// SELF: the query's elements are read from the index row of its flat id, whose tail is no data exactly as a candidate row's is not
// (the screen has kept the point itself out of its lists: it is no candidate here).
template <int METRIC, bool SELF>
__global__ __launch_bounds__(64) void exact_rerank_kernel(DeviceIndexView ix, RerankArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint64_t* const ek = reinterpret_cast<uint64_t*>(lds_raw);  // [sort_n] the exact keys
    const uint32_t lane = threadIdx.x;
    const uint32_t qs = blockIdx.x;
    const uint32_t tile = qs / a.qt, t = qs % a.qt;
    const uint32_t k = a.k, cap = a.cap;
    const size_t slot = ((size_t)tile * a.n_slabs + (lane < a.n_slabs ? lane : 0u)) * a.qt + t;
    const uint64_t* list = a.lists + slot * cap;
    const uint32_t len = lane < a.n_slabs ? a.lens[slot] : 0u;
    uint32_t total = len;
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    const uint32_t cnt = total < cap ? total : cap;
    const float4* const qrow = reinterpret_cast<const float4*>(SELF ? ix.vec + (size_t)a.self[qs] * ix.row_stride : a.qpad + (size_t)qs * a.dpad);
    const uint32_t nchunk = a.sa.nchunk;
    const bool norm_in_tail = METRIC == DIST_COSINE && a.sa.nrm2 == nullptr && nchunk * 4u == ix.row_stride;
    for (uint32_t i = lane; i < a.sort_n; i += 64u) ek[i] = KEY_NONE;
    uint32_t h = 0;
    uint64_t cur = len > 0u ? list[0] : KEY_NONE;
    uint64_t got = KEY_NONE, last = KEY_NONE;
    for (uint32_t j = 0; j < cnt; ++j) {
        uint64_t m = cur;
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(m >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)m, o, 64);
            m = other < m ? other : m;
        }
        if (cur == m) {  // keys are unique: one lane
            ++h;
            cur = h < len ? list[h] : KEY_NONE;
        }
        if (lane == (j & 63u)) got = m;
        last = m;
        if ((j & 63u) == 63u || j + 1u == cnt) {
            const uint32_t jj = (j & ~63u) + lane;
            if (jj <= j) {  // this lane's candidate through the chain of exact_row_chain.inc
                const uint32_t rk = (uint32_t)got, flat = a.order[rk];
                const float* rowf = ix.vec + (size_t)flat * ix.row_stride;
                const float4* row = reinterpret_cast<const float4*>(rowf);
                double s2 = 0.;
                if constexpr (METRIC == DIST_COSINE)
                    s2 = a.sa.nrm2 != nullptr ? a.sa.nrm2[flat] : *reinterpret_cast<const double*>(rowf + ix.row_stride - 2u);
                ACC acc = 0;
                for (uint32_t c = 0; c < nchunk; ++c) {
                    float4 x = row[c], q4 = qrow[c];
                    if (norm_in_tail && c + 1u == nchunk) {
                        x.z = 0.f, x.w = 0.f;
                        if constexpr (SELF) q4.z = 0.f, q4.w = 0.f;
                    }
                    chain4<METRIC, ACC>(acc, q4, x);
                }
                ek[jj] = make_key(tile_dist<METRIC>(a.sa, qs, acc, s2), rk);
            }
        }
    }
    __syncthreads();
    // bitonic sort of sort_n keys, ascending (the keys are unique; KEY_NONE fills the tail)
    for (uint32_t size = 2u; size <= a.sort_n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
            for (uint32_t i = lane; i < (a.sort_n >> 1); i += 64u) {
                const uint32_t x = ((i & ~(stride - 1u)) << 1) | (i & (stride - 1u)), y = x | stride;
                const uint64_t kx = ek[x], ky = ek[y];
                const bool up = (x & size) == 0u;
                if ((kx > ky) == up) { ek[x] = ky; ek[y] = kx; }
            }
            __syncthreads();
        }
    }
    const uint32_t q = a.q0 + qs;  // the query's row in the chunk's out arrays is qs
    bool certified = total < cap;
    if (!certified && k <= cnt) certified = (uint32_t)(last >> 32) > (uint32_t)(ek[k - 1u] >> 32);
    if (!certified) {
        if (lane == 0u) a.fb_list[atomicAdd(a.fb_count, 1u)] = q;
        return;
    }
    const uint32_t n_ans = cnt < k ? cnt : k;
    for (uint32_t j = lane; j < k; j += 64u) {
        const size_t o = (size_t)qs * k + j;
        if (j < n_ans) {
            const uint64_t key = ek[j];
            write_answer(ix, a.order, key, (uint32_t)key, o, a.out.ids, a.out.dists, a.out.layer, a.out.rank);
        } else {  // slots behind the answers: zero, as the search entries leave them
            a.out.ids[o] = 0ull;
            a.out.dists[o] = 0.f;
            if (a.out.layer) a.out.layer[o] = 0;
            if (a.out.rank) a.out.rank[o] = 0;
        }
    }
    if (lane == 0u) a.out.counts[qs] = n_ans;
}

// SELF, DistCosine: one thread per query of the chunk: the stored point's squared norm in the crate's arithmetic -- f32 squares widened
// to f64 and summed left to right over the first d elements, what exact_screen_prep_kernel's qnorm is for the point's vector (the
// zeros of its padded copy add nothing).  The plain f32 norm needs no pass: it is the replica's xn[flat].
__global__ void exact_screen_self_norm_kernel(DeviceIndexView ix, const uint32_t* __restrict__ self, uint32_t nq, double* __restrict__ qnorm) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= nq) return;
    const float* row = ix.vec + (size_t)self[qs] * ix.row_stride;
    double s1 = 0.;
    for (uint32_t i = 0; i < ix.d; ++i) {
        const float sq = row[i] * row[i];
        s1 = s1 + (double)sq;
    }
    qnorm[qs] = s1;
}

// The cut of a screened call: tiles of qt queries, slabs of rows (whole staged blocks of `rows`)
struct ScreenPlan {
    uint64_t dpad, nkc, waves, qt, tiles_total, slabs, slab_rows, cap, rows;
    bool cut(uint64_t n, uint64_t nq, uint64_t most) {
        tiles_total = (nq + qt - 1) / qt;
        slabs = std::min<uint64_t>({MAX_SLABS, (SCREEN_WG_TARGET + tiles_total - 1) / tiles_total, most});
        if (slabs == 0) return false;
        slab_rows = std::max<uint64_t>(SCREEN_SLAB_ROWS, round_up((n + slabs - 1) / slabs, rows));
        slabs = (n + slab_rows - 1) / slab_rows;
        return true;
    }
};

// every pointer is device memory; waits for `stream` before it returns.  stats: {certified, fallen back, not screened}
// c.d_self != nullptr (the k-NN graph): query q is the stored point of flat id d_self[q], never its own answer; d_queries is not read,
// c.d is the index's, and the scratch holds no copy of a query -- the screen and the rerank read the replica's rows (SELF).
template <class KIND>
int screened_device(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactCall& c, uint64_t* stats, hipStream_t stream, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t nq = c.nq, d = c.d, k = c.k, n = v.n;
    const uint32_t* const d_self = c.d_self;
    const bool self = d_self != nullptr;
    stats[0] = stats[1] = stats[2] = 0;
    if (nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    ScreenPlan plan{};
    plan.dpad = round_up(d, KC), plan.nkc = plan.dpad / KC, plan.cap = k + SCREEN_MARGIN, plan.rows = KIND::ROWS;
    plan.waves = metric_has_screen(dev.dist()) && plan.cap <= SCREEN_MAX_C && n >= SCREEN_MIN_ROWS ? KIND::waves(dev.device(), plan.dpad, self) : 0;
    plan.qt = plan.waves * SQ;
    const uint64_t words = (n + 31) / 32, cap = plan.cap;
    const bool filtered = c.d_allowed != nullptr;
    // in front of the tiles: the bitmap, the fallback list, its count
    const uint64_t fixed_bytes = round_up(filtered ? words * 4 : 0, 256) + round_up(nq * 4, 256) + 256;
    bool screened = plan.waves != 0 && fixed_bytes < SCRATCH_BUDGET / 2;
    // a query slot's own bytes: the padded copy and its plain norm (SELF: neither), the norm in the crate's arithmetic
    const uint64_t q_bytes = (self ? 0 : plan.dpad * 4 + 4) + 8;
    // slabs: never more lists than the budget holds for one tile
    if (screened) screened = plan.cut(n, nq, (SCRATCH_BUDGET - fixed_bytes) / (plan.qt * (q_bytes + cap * 8 + 4) + 2048));
    if (!screened) {  // the existing path, wholesale
        stats[2] = nq;
        return exact_device(dev, origin_id, c, stream, err);
    }
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "exact search", err);
    if (!st) return ERR_DEVICE;
    const float* d_xn = nullptr;
    int rc = row_norms(*st, v, stream, &d_xn, err);
    if (rc != OK) return rc;

    const uint64_t qt = plan.qt, slabs = plan.slabs, dpad = plan.dpad;
    // queries per chunk: whole tiles, what the budget holds, a grid the launch accepts (every array of a chunk is dense over its slots)
    const uint64_t per_tile = qt * q_bytes + slabs * qt * (cap * 8 + 4);
    const uint64_t chunk_tiles = std::min<uint64_t>({plan.tiles_total, (SCRATCH_BUDGET - fixed_bytes - 5 * 256) / per_tile, 65535});
    if (chunk_tiles == 0) { err = "exact screen: scratch plan"; return ERR_FORMAT; }
    uint32_t *d_allow, *d_fb, *d_fb_count, *d_lens;
    float *d_qpad, *d_qn;
    double* d_qnorm;
    uint64_t* d_lists;
    ScratchLayout lay;
    lay.array(d_allow, filtered ? words : 0);
    lay.array(d_fb, nq);
    lay.bytes(d_fb_count, 256);
    lay.array(d_qpad, self ? 0 : chunk_tiles * qt * dpad);
    lay.array(d_qn, self ? 0 : chunk_tiles * qt);
    lay.array(d_qnorm, chunk_tiles * qt);
    lay.array(d_lists, chunk_tiles * slabs * qt * cap);
    lay.array(d_lens, chunk_tiles * slabs * qt);
    if (lay.size() > SCRATCH_BUDGET) { err = "exact screen: scratch layout"; return ERR_FORMAT; }
    ScratchLease lease(st.get());
    rc = alloc_layout("exact screen", lease, lay, err);
    if (rc != OK) return rc;
    // whatever happens, nothing of this call is still running when the scratch block goes back to the pool
    Drain drain{stream};

    if (filtered) HIP_TRY(launch_allow_bitmap(stream, v.origin_id, v.n, c.d_allowed, c.n_allowed, d_allow));
    HIP_TRY(hipMemsetAsync(d_fb_count, 0, 4, stream));
    const uint32_t lds = (uint32_t)KIND::lds_bytes(plan.waves, dpad, self);
    uint32_t sort_n = 2;
    while (sort_n < cap) sort_n <<= 1;
    const bool zero_tail = dev.dist() == DIST_COSINE && dev.side_norms() == nullptr;
    for (uint64_t t0 = 0; t0 < plan.tiles_total; t0 += chunk_tiles) {
        const uint64_t tiles = std::min(chunk_tiles, plan.tiles_total - t0);
        const uint64_t q0 = t0 * qt, cq = std::min<uint64_t>(tiles * qt, nq - q0);
        const uint32_t n_slots = (uint32_t)(tiles * qt);
        const uint32_t* const chunk_self = self ? d_self + q0 : nullptr;
        if (!self) {
            hipLaunchKernelGGL(exact_screen_prep_kernel, grid_of(n_slots), dim3(256), 0, stream, c.d_queries + q0 * d, (uint32_t)cq, (uint32_t)d, (uint32_t)dpad,
                               n_slots, d_qpad, d_qn, d_qnorm);
        } else if (dev.dist() == DIST_COSINE) {  // (the one metric whose last step reads the query's norm: tile_dist)
            hipLaunchKernelGGL(exact_screen_self_norm_kernel, grid_of(cq), dim3(256), 0, stream, v, chunk_self, (uint32_t)cq, d_qnorm);
        }
        HIP_TRY(hipGetLastError());
        ScreenArgs a{d_qpad, d_qn, d_xn, st->rank(), filtered ? d_allow : nullptr, d_lists, d_lens, nullptr, (uint32_t)cq, (uint32_t)dpad, (uint32_t)plan.nkc,
                     (uint32_t)qt, (uint32_t)plan.slab_rows, (uint32_t)slabs, (uint32_t)cap, KIND::coeff(dev.dist(), d), zero_tail ? 1u : 0u, chunk_self};
        HIP_TRY(KIND::template launch<false>(dev.dist(), dim3((uint32_t)slabs, (uint32_t)tiles), (uint32_t)plan.waves, lds, stream, v, a));
        RerankArgs r{SlabArgs{nullptr, d_qnorm, st->rank(), nullptr, dev.side_norms(), (uint32_t)cq, (uint32_t)((d + 3) / 4), (uint32_t)plan.slab_rows, (uint32_t)slabs},
                     d_qpad, d_lists, d_lens, st->order(), (uint32_t)dpad, (uint32_t)qt, (uint32_t)slabs, (uint32_t)cap, (uint32_t)k, sort_n, (uint32_t)q0,
                     rows_at(c.out, q0, k), d_fb, d_fb_count, chunk_self};
        HIP_TRY(for_screened_metric(dev.dist(), [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (self) hipLaunchKernelGGL((exact_rerank_kernel<M, true>), dim3((uint32_t)cq), dim3(64), sort_n * 8u, stream, v, r);
            else hipLaunchKernelGGL((exact_rerank_kernel<M, false>), dim3((uint32_t)cq), dim3(64), sort_n * 8u, stream, v, r);
        }));
    }
    uint32_t fallen = 0;
    HIP_TRY(hipMemcpyAsync(&fallen, d_fb_count, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    stats[0] = nq - fallen, stats[1] = fallen;
    if (fallen == 0) return OK;
    ExactCall f = c;  // the listed queries (SELF: the listed points of d_self) through the existing path, into their own rows
    f.nq = fallen;
    f.d_qlist = d_fb;
    return exact_device(dev, origin_id, f, stream, err);
}

// The device side of a screened k-NN entry pair; capi.cpp holds the entries and every argument check.
template <class KIND>
int screened_call(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactScreenArgs& a, bool host, void* stream, std::string& err) {
    uint64_t stats[3] = {0, 0, 0};
    uint64_t* const out_stats = a.out_stats ? a.out_stats : stats;
    ExactCall c;
    c.d_queries = a.queries;
    c.nq = a.nq, c.d = a.d, c.k = a.k;
    c.d_allowed = a.allowed, c.n_allowed = a.n_allowed;
    c.out = GraphRows{a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts};
    if (!host) return screened_device<KIND>(dev, origin_id, c, out_stats, static_cast<hipStream_t>(stream), err);
    // host buffers: queries and answers are staged in chunks of at most 64 MB, each one call of the device path on the null stream
    out_stats[0] = out_stats[1] = out_stats[2] = 0;
    if (a.nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    FilterUpload filter;
    int rc = filter.put(a.allowed, a.n_allowed, err);
    if (rc != OK) return rc;
    const uint64_t per_q = a.d * 4 + a.k * 17 + 4;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(a.nq, (64ull << 20) / per_q));
    DevMem m_q;
    AnswerStage stage;
    HIP_TRY(m_q.alloc(chunk * a.d * 4));
    if ((rc = stage.alloc("exact search", chunk, a.k, err)) != OK) return rc;
    c.d_queries = static_cast<const float*>(m_q.p);
    c.d_allowed = filter.d_allowed;
    c.out = stage.rows;
    for (uint64_t q0 = 0; q0 < a.nq; q0 += chunk) {
        c.nq = std::min(chunk, a.nq - q0);
        uint64_t part[3];
        HIP_TRY(hipMemcpy(m_q.p, a.queries + q0 * a.d, c.nq * a.d * 4, hipMemcpyHostToDevice));
        if ((rc = screened_device<KIND>(dev, origin_id, c, part, nullptr, err)) != OK) return rc;
        if ((rc = copy_rows_out(rows_at(GraphRows{a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts}, q0, a.k), stage.rows, c.nq * a.k, c.nq, nullptr, err)) != OK)
            return rc;
        for (int i = 0; i < 3; ++i) out_stats[i] += part[i];
    }
    return OK;
}

// The device side of a screen matrix entry (host buffers): the screen kernel with a store epilogue
template <class KIND>
int screen_matrix_call(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ScreenMatrixArgs& a, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t n = v.n, dpad = round_up(a.d, KC);
    if (!metric_has_screen(dev.dist())) { err = "exact screen matrix: this distance has no screen (DistL2, DistDot, DistCosine have)"; return ERR_ARG; }
    if (a.nq * n > SCREEN_MATRIX_PAIRS) { err = "exact screen matrix: nq * n above 2^24 pairs"; return ERR_ARG; }
    if (a.nq == 0 || n == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint32_t waves = (uint32_t)KIND::waves(dev.device(), dpad, a.self);
    if (waves == 0) { err = std::string("exact screen matrix: rows too long ") + KIND::too_long(); return ERR_ARG; }
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "exact screen matrix", err);
    if (!st) return ERR_DEVICE;
    const float* d_xn = nullptr;
    int rc = row_norms(*st, v, nullptr, &d_xn, err);
    if (rc != OK) return rc;
    DevMem m_flat, mem;  // a.self: the named points as flat ids -- the only query operand there is
    if (a.self && (rc = graph_resolve(v, *st, GraphCallArgs{a.point_ids, a.nq, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr}, true, m_flat, nullptr, err)) != OK)
        return rc;
    ScreenPlan plan{};
    plan.dpad = dpad, plan.nkc = dpad / KC, plan.waves = waves, plan.qt = waves * SQ, plan.cap = 0, plan.rows = KIND::ROWS;
    plan.cut(n, a.nq, MAX_SLABS);
    const uint64_t slots = plan.tiles_total * plan.qt;
    float *d_src, *d_qpad, *d_qn, *d_lb;
    double* d_qnorm;
    ScratchLayout lay;
    lay.array(d_src, a.self ? 0 : a.nq * a.d);
    lay.array(d_qpad, a.self ? 0 : slots * dpad);
    lay.array(d_qn, a.self ? 0 : slots);
    lay.array(d_qnorm, a.self ? 0 : slots);
    lay.array(d_lb, a.nq * n);
    rc = alloc_layout("exact screen matrix", mem, lay, err);
    if (rc != OK) return rc;
    Drain drain{nullptr};
    if (!a.self) {
        HIP_TRY(hipMemcpyAsync(d_src, a.queries, a.nq * a.d * 4, hipMemcpyHostToDevice, nullptr));
        hipLaunchKernelGGL(exact_screen_prep_kernel, grid_of(slots), dim3(256), 0, nullptr, d_src, (uint32_t)a.nq, (uint32_t)a.d, (uint32_t)dpad, (uint32_t)slots,
                           d_qpad, d_qn, d_qnorm);
        HIP_TRY(hipGetLastError());
    }
    ScreenArgs s{d_qpad, d_qn, d_xn, st->rank(), nullptr, nullptr, nullptr, d_lb, (uint32_t)a.nq, (uint32_t)dpad, (uint32_t)plan.nkc, (uint32_t)plan.qt,
                 (uint32_t)plan.slab_rows, (uint32_t)plan.slabs, 0u, KIND::coeff(dev.dist(), a.d), dev.dist() == DIST_COSINE && dev.side_norms() == nullptr ? 1u : 0u,
                 static_cast<const uint32_t*>(m_flat.p)};
    HIP_TRY(KIND::template launch<true>(dev.dist(), dim3((uint32_t)plan.slabs, (uint32_t)plan.tiles_total), waves, (uint32_t)KIND::lds_bytes(waves, dpad, a.self), nullptr, v,
                                        s));
    return copy_out({{a.out_lb, d_lb, a.nq * n * 4}}, true, nullptr, err);
}

// The device side of the screened exact graph (hnswxg_exact_graph_batch(_device)): exact_graph of knn_graph.hip with screened_device
// in the place of exact_device.  The named points become flat ids on the device; a host call's answers are staged in chunks of at
// most 64 MB.  out_stats ([3], host memory, may be nullptr) is written when the call has succeeded, never before.
template <class KIND>
int screened_graph_call(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, uint64_t* out_stats, bool host, void* stream_v,
                        std::string& err) {
    const uint64_t np = a.np, k = a.k;
    uint64_t stats[3] = {0, 0, 0};
    if (np != 0) {
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
        if (!host) {
            if ((rc = screened_device<KIND>(dev, origin_id, c, stats, stream, err)) != OK) return rc;
        } else {
            if ((rc = filter.put(a.allowed, a.n_allowed, err)) != OK) return rc;
            c.d_allowed = filter.d_allowed;
            const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(np, (64ull << 20) / (k * 17 + 4)));
            if ((rc = stage.alloc("exact graph", chunk, k, err)) != OK) return rc;
            c.out = stage.rows;
            for (uint64_t c0 = 0; c0 < np; c0 += chunk, c.d_self += chunk) {
                c.nq = std::min(chunk, np - c0);
                uint64_t part[3];
                if ((rc = screened_device<KIND>(dev, origin_id, c, part, stream, err)) != OK) return rc;
                if ((rc = copy_rows_out(rows_at(out, c0, k), stage.rows, c.nq * k, c.nq, stream, err)) != OK) return rc;
                for (int i = 0; i < 3; ++i) stats[i] += part[i];
            }
        }
    }
    if (out_stats) out_stats[0] = stats[0], out_stats[1] = stats[1], out_stats[2] = stats[2];
    return OK;
}

}  // namespace
}  // namespace hnswgpu
