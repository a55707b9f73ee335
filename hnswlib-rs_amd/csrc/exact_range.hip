// exact_range.hip -- exact range search over every point of an uploaded index (gfx950 only): the device side of
// hnswgpu_exact_range_search_batch / _device (the entries are in capi.cpp).  Every eligible row with dist <= the query's radius, in
// the exact k-NN's key order.  DESIGN.md "Exact range search".
//   exact_range_slab_kernel    the tile and the chain of exact_knn.hip's slab kernel (exact_tile.hpp) without the lists.  Count pass:
//                              a ballot and a popcount per (query, 64 rows) into a counter per (query, slab).  Fill pass: the same
//                              loop, the hitting lanes write their keys, compacted by the ballot's prefix, at the (query, slab) base.
//   exact_range_scan_kernel    the counters, query major and slab minor, into the CSR offsets and into each slab's base
//   (rocPRIM)                  every query's segment of keys sorted ascending
//   exact_range_decode_kernel  keys into ids, distances and p_ids
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_index.hpp"
#include "exact_internal.hpp"
#include "exact_tile.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

constexpr uint64_t RANGE_HITS_PER_PASS = 8ull << 20;  // answers one fill pass holds at most (HNSWGPU_RANGE_HITS_PER_PASS), or one query's
constexpr uint64_t RANGE_TILE_BUDGET = 64ull << 20;   // bytes of tiled queries and counters per chunk of tiles

typedef __attribute__((address_space(4))) const float* ufloat_ptr_t;
typedef __attribute__((address_space(4))) const uint64_t* uquad_ptr_t;

struct ExactRangeArgs : SlabArgs {
    const float* radius;    // [nq] the chunk's radii
    uint32_t* cnt;          // [nq][n_slabs]; count pass: the hits of (query, slab), written.  Fill pass: the hits of the query in the slabs
                            // before this one, read (nullptr: one slab)
    const uint64_t* offs;   // fill pass: [nq] where each query's answer starts among the batch's answers
    uint64_t* keys;         // fill pass: the chunk's keys, slot 0 being answer key_base of the batch; nullptr: count pass
    uint64_t key_base;
    uint32_t key_cap;       // slots behind keys
};

// At most this many waves per SIMD: without the lists the loop needs 40 VGPRs and eight waves would fit, but every wavefront
// streams its tile's queries through the scalar cache (8 KB per tile at d = 128), and with more tiles resident than the cache
// holds the scalar loads the loop waits for slow down: 1M x 128 DistL2, 10 000 queries, count pass 238 ms uncapped, 189 ms at
// five, 161 ms at four (the k-NN kernel's 88 VGPRs give it five).
#ifndef HNSW_RANGE_MAX_WAVES
#define HNSW_RANGE_MAX_WAVES 4
#endif
// per query of the tile the radius and the counter (fill pass: the next slot) are wave-uniform
template <int METRIC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(
    METRIC == DIST_JEFFREYS || METRIC == DIST_JENSENSHANNON ? 2 : (HNSW_RANGE_MAX_WAVES < 4 ? HNSW_RANGE_MAX_WAVES : 4), HNSW_RANGE_MAX_WAVES)))
void exact_range_slab_kernel(DeviceIndexView ix, ExactRangeArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    const uint32_t lane = threadIdx.x;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const SlabTile T = slab_tile<METRIC>(ix, a, slab, tile);
    const uint32_t nvalid = T.nvalid, nchunk = a.nchunk;
    const bool fill = a.keys != nullptr;
    float rad[TQ];
    uint32_t pos[TQ];  // count pass: the hits so far; fill pass: the slot of the next hit
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        const uint32_t qs = tile * (uint32_t)TQ + ((uint32_t)t < nvalid ? (uint32_t)t : 0u);  // (the slots behind the last query are never counted)
        rad[t] = ((ufloat_ptr_t)a.radius)[qs];
        pos[t] = 0u;
        if (fill) {
            pos[t] = (uint32_t)(((uquad_ptr_t)a.offs)[qs] - a.key_base);
            if (a.cnt != nullptr) pos[t] += ((uword_ptr_t)a.cnt)[(size_t)qs * a.n_slabs + slab];
        }
    }

    for (uint32_t r0 = T.lo; r0 < T.hi; r0 += 64u) {
        uint32_t r;
        bool in;
        const bool ok = slab_row(T, r0, lane, a.allow, r, in);
        if (__ballot(ok) == 0ull) continue;  // (wave-uniform) nothing eligible for any query among these 64 rows
#include "exact_row_chain.inc"
        const uint32_t rk = fill ? a.rank[r] : 0u;
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            if ((uint32_t)t < nvalid) {
                const float v = tile_dist<METRIC>(a, tile * (uint32_t)TQ + (uint32_t)t, acc[t], s2);
                const bool hit = ok && v <= rad[t];  // (a NaN on either side: no hit)
                const unsigned long long m = __ballot(hit);
                if (m != 0ull) {
                    if (fill && hit) {
                        const uint32_t p = pos[t] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        if (p < a.key_cap) a.keys[p] = make_key(v, rk);
                    }
                    pos[t] += popc64(m);
                }
            }
        }
    }
    if (!fill && lane < nvalid) {
        uint32_t c = 0;
#pragma unroll
        for (int t = 0; t < TQ; ++t)
            if (lane == (uint32_t)t) c = pos[t];
        a.cnt[(size_t)(tile * (uint32_t)TQ + lane) * a.n_slabs + slab] = c;
    }
}

// one workgroup: the counters of a chunk, query major and slab minor, into offs[q + 1] = offs[0] + the hits of queries 0 .. q, and
// in place every counter into the hits of its query in the slabs before it.  offs[0]: set to `base` (set_base), else what the
// previous chunk left there.
__global__ __launch_bounds__(1024) void exact_range_scan_kernel(uint32_t* __restrict__ cnt, uint32_t nq, uint32_t n_slabs, uint64_t* __restrict__ offs,
                                                               bool set_base, uint64_t base) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nq + 1023u) / 1024u;
    const uint32_t q0 = t * per < nq ? t * per : nq, q1 = nq - q0 < per ? nq : q0 + per;
    uint64_t sum = 0;
    for (uint32_t q = q0; q < q1; ++q)
        for (uint32_t s = 0; s < n_slabs; ++s) sum += cnt[(size_t)q * n_slabs + s];
    part[t] = sum;
    __syncthreads();
    if (t == 0u) {
        uint64_t run = set_base ? base : offs[0];
        if (set_base) offs[0] = base;
        for (uint32_t i = 0; i < 1024u; ++i) { const uint64_t p = part[i]; part[i] = run; run += p; }
    }
    __syncthreads();
    uint64_t run = part[t];
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t in_query = 0;
        for (uint32_t s = 0; s < n_slabs; ++s) {
            const uint32_t c = cnt[(size_t)q * n_slabs + s];
            cnt[(size_t)q * n_slabs + s] = in_query;
            in_query += c;
        }
        run += in_query;
        offs[q + 1u] = run;
    }
}

// one thread per sorted key: the answer it stands for
__global__ __launch_bounds__(256) void exact_range_decode_kernel(DeviceIndexView ix, const uint64_t* __restrict__ keys, uint32_t count,
                                                                const uint32_t* __restrict__ order, uint64_t* __restrict__ out_ids,
                                                                float* __restrict__ out_dists, uint8_t* __restrict__ out_layer,
                                                                int32_t* __restrict__ out_rank) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const uint64_t key = keys[j];
    const uint32_t rk = (uint32_t)key < ix.n ? (uint32_t)key : 0u;  // (a rank, whatever the slot holds)
    write_answer(ix, order, key, rk, j, out_ids, out_dists, out_layer, out_rank);
}

hipError_t launch_range_slab(int metric, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const ExactRangeArgs& a) {
    return launch_for_metric(metric, [&](auto m) { hipLaunchKernelGGL((exact_range_slab_kernel<decltype(m)::value>), grid, dim3(64), 0, stream, ix, a); });
}

// an answer's position among the batch's answers -> its slot in the chunk's keys (the segment bounds of the sort)
struct RangeSlot {
    uint64_t base;
    __host__ __device__ unsigned int operator()(uint64_t v) const { return (unsigned int)(v - base); }
};
typedef rocprim::transform_iterator<const uint64_t*, RangeSlot, unsigned int> range_slot_iter_t;
hipError_t sort_segments(void* temp, size_t& temp_bytes, uint64_t* keys_in, uint64_t* keys_out, uint32_t count, uint32_t segments,
                         const uint64_t* d_offs, uint64_t base, hipStream_t stream) {
    const range_slot_iter_t begin(d_offs, RangeSlot{base});
    return rocprim::segmented_radix_sort_keys(temp, temp_bytes, keys_in, keys_out, count, segments, begin, begin + 1, 0u, 64u, stream);
}

// the fill pass's plan: the consecutive queries [qa, qb) of [qa, q_end) whose answers fit `budget` slots, at most max_q of them and
// one at least (a single query may hit every point).  offs: the CSR offsets of the batch, on the host.
uint64_t range_chunk_end(const uint64_t* offs, uint64_t qa, uint64_t q_end, uint64_t budget, uint64_t max_q) {
    uint64_t qb = qa + 1;
    while (qb < q_end && qb - qa < max_q && offs[qb + 1] - offs[qa] <= budget) ++qb;
    return qb;
}

// Both entries.  Count pass over every query (host buffers: in blocks of at most 64 MB of queries), the offsets complete on the
// caller's side; then, when the total fits cap, the fill pass chunk by chunk of the plan: keys, sort, decode -- into the caller's
// arrays (device) or into a staging area that is copied out (host).  Waits for `stream` before it returns.
// d_allowed: c.allowed on the device (not nullptr: a filter, even when it is empty).
int exact_range_passes(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& c, bool host, const uint64_t* d_allowed,
                       hipStream_t stream, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t nq = c.nq, d = c.d;
    const GraphRows out{c.out_ids, c.out_dists, c.out_layer, c.out_rank, nullptr};  // cap slots; no counts
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    if (nq == 0 || v.n == 0) {  // no query: the one offset; no point: every answer is empty
        if (host) { std::memset(c.out_offsets, 0, (nq + 1) * 8); return OK; }
        HIP_TRY(hipMemsetAsync(c.out_offsets, 0, (nq + 1) * 8, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return OK;
    }
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "exact range search", err);
    if (!st) return ERR_DEVICE;

    SlabPlan plan(v.n, d, nq);
    plan.cut();
    const uint64_t n = plan.n, slabs = plan.slabs;
    // more than one slab: fewer than 8192 tiles, the batch's counters are 1 MB at most and stay for the fill pass; one slab: a
    // query's base is its offset, the counters are a chunk's
    const bool keep = slabs > 1;
    const uint64_t per_tile = plan.qt_bytes() + plan.qnorm_bytes() + (keep ? 0 : TQ * 4);
    const uint64_t block_q = host ? std::max<uint64_t>(1, std::min<uint64_t>(nq, (64ull << 20) / (d * 4 + 12))) : nq;
    const uint64_t chunk_tiles = std::min<uint64_t>({(block_q + TQ - 1) / TQ, std::max<uint64_t>(1, RANGE_TILE_BUDGET / per_tile), 65535});
    const uint64_t cnt_bytes = round_up(keep ? nq * slabs * 4 : chunk_tiles * TQ * 4, 256);
    const int64_t knob = knobs().range_hits_per_pass;
    const uint64_t budget = knob > 0 ? (uint64_t)knob : RANGE_HITS_PER_PASS;
    const uint64_t max_fill_q = std::min<uint64_t>(block_q, chunk_tiles * TQ);
    // the keys of one fill pass: the budget, or one query's answer where that is larger -- never more than the caller has room for
    const uint64_t all_pairs = nq > 0xFFFFFFFFull / n ? 0xFFFFFFFFull : nq * n;
    const uint64_t key_cap = std::min<uint64_t>({std::max(budget, n), all_pairs, c.cap});
    if (key_cap > 0xFFFFFFF0ull) { err = "index too large for the exact range search"; return ERR_ARG; }
    size_t temp_bytes = 0;
    if (key_cap != 0)
        HIP_TRY(sort_segments(nullptr, temp_bytes, nullptr, nullptr, (uint32_t)key_cap, (uint32_t)max_fill_q, nullptr, 0, stream));

    // (d_qt, d_qnorm: every tile's part padded, tile behind tile; staged: the staging of a host call)
    uint32_t *d_allow = nullptr, *d_cnt;
    float* d_qt;
    double* d_qnorm;
    uint64_t *d_keys_a, *d_keys_b;
    void* d_temp;
    GraphRows staged{};
    ScratchLayout lay;
    if (d_allowed != nullptr) lay.array(d_allow, plan.words);
    plan.tiles(lay, chunk_tiles, d_qt, d_qnorm);
    lay.bytes(d_cnt, cnt_bytes);
    lay.arrays(key_cap, d_keys_a, d_keys_b);
    lay.bytes(d_temp, round_up(temp_bytes, 256));
    if (host) lay.arrays(key_cap, staged.ids, staged.dists, staged.rank, staged.layer);
    lay.skip(256);
    ScratchLease lease(st.get());
    const int rc_lease = alloc_layout("exact range search", lease, lay, err);
    if (rc_lease != OK) return rc_lease;

    DevMem m_q, m_rad, m_off;
    if (host) {
        HIP_TRY(m_q.alloc(block_q * d * 4));
        HIP_TRY(m_rad.alloc(block_q * 4));
        HIP_TRY(m_off.alloc((block_q + 1) * 8));
    }
    // the offsets on the host: the caller's array, or a copy of it (the plan of the fill pass is made here)
    std::vector<uint64_t> off_copy;
    if (!host) off_copy.resize(nq + 1);
    uint64_t* const h_off = host ? c.out_offsets : off_copy.data();
    h_off[0] = 0;

    Drain drain{stream};

    if (d_allow != nullptr) HIP_TRY(launch_allow_bitmap(stream, v.origin_id, v.n, d_allowed, c.n_allowed, d_allow));
    ExactRangeArgs a{};
    static_cast<SlabArgs&>(a) = slab_args(*st, dev, plan, d_qt, d_qnorm, d_allow);
    // queries [q0, q0 + cq) of a block into the tiles
    auto prep = [&](const float* dq, uint64_t cq) { return exact_prep_queries(stream, dq, cq, d, plan, (uint32_t)((cq + TQ - 1) / TQ * TQ), d_qt, d_qnorm); };
    const bool one_block = block_q >= nq;
    // where block [b0, b0 + bq) has its queries, radii and offsets on the device
    const float* dq = c.queries;
    const float* dr = c.radii;
    uint64_t* doff = c.out_offsets;
    auto stage_block = [&](uint64_t b0, uint64_t bq) -> int {
        if (!host) return OK;
        HIP_TRY(hipMemcpyAsync(m_q.p, c.queries + b0 * d, bq * d * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(m_rad.p, c.radii + b0, bq * 4, hipMemcpyHostToDevice, stream));
        dq = static_cast<const float*>(m_q.p);
        dr = static_cast<const float*>(m_rad.p);
        doff = static_cast<uint64_t*>(m_off.p);
        return OK;
    };

    // ---- the count pass
    for (uint64_t b0 = 0; b0 < nq; b0 += block_q) {
        const uint64_t bq = std::min(block_q, nq - b0);
        const int rc = stage_block(b0, bq);
        if (rc != OK) return rc;
        for (uint64_t q0 = 0; q0 < bq; q0 += chunk_tiles * TQ) {
            const uint64_t cq = std::min<uint64_t>(chunk_tiles * TQ, bq - q0);
            HIP_TRY(prep(dq + q0 * d, cq));
            a.radius = dr + q0;
            a.cnt = d_cnt + (keep ? (b0 + q0) * slabs : 0);
            a.offs = nullptr;
            a.keys = nullptr;
            a.nq = (uint32_t)cq;
            HIP_TRY(launch_range_slab(dev.dist(), dim3((uint32_t)slabs, (uint32_t)((cq + TQ - 1) / TQ)), stream, v, a));
            hipLaunchKernelGGL(exact_range_scan_kernel, dim3(1), dim3(1024), 0, stream, a.cnt, (uint32_t)cq, (uint32_t)slabs, doff + q0, q0 == 0,
                               h_off[b0]);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h_off + b0 + 1, doff + 1, bq * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    const uint64_t total = h_off[nq];
    if (total > c.cap) {
        err = "the answers need " + std::to_string(total) + " slots, cap is " + std::to_string(c.cap);
        return HNSWGPU_ERR_CAPACITY;
    }
    if (total == 0 || out.ids == nullptr) return OK;

    // ---- the fill pass
    if (!out.layer) staged.layer = nullptr;  // (what the caller does not ask for is not decoded)
    if (!out.rank) staged.rank = nullptr;
    for (uint64_t b0 = 0; b0 < nq; b0 += block_q) {
        const uint64_t bq = std::min(block_q, nq - b0);
        if (h_off[b0 + bq] == h_off[b0]) continue;  // a block of empty answers
        if (!one_block) {
            const int rc = stage_block(b0, bq);
            if (rc != OK) return rc;
            HIP_TRY(hipMemcpyAsync(doff, h_off + b0, (bq + 1) * 8, hipMemcpyHostToDevice, stream));
        }
        for (uint64_t qa = b0, qb; qa < b0 + bq; qa = qb) {
            qb = range_chunk_end(h_off, qa, b0 + bq, budget, max_fill_q);
            const uint64_t hits = h_off[qb] - h_off[qa], cq = qb - qa;
            if (hits == 0) continue;
            if (hits > key_cap) { err = "internal error: a fill pass of " + std::to_string(hits) + " answers"; return ERR_DEVICE; }
            HIP_TRY(prep(dq + (qa - b0) * d, cq));
            a.radius = dr + (qa - b0);
            a.cnt = keep ? d_cnt + qa * slabs : nullptr;
            a.offs = doff + (qa - b0);
            a.keys = d_keys_a;
            a.key_base = h_off[qa];
            a.key_cap = (uint32_t)hits;
            a.nq = (uint32_t)cq;
            HIP_TRY(launch_range_slab(dev.dist(), dim3((uint32_t)slabs, (uint32_t)((cq + TQ - 1) / TQ)), stream, v, a));
            size_t need = 0;
            HIP_TRY(sort_segments(nullptr, need, d_keys_a, d_keys_b, (uint32_t)hits, (uint32_t)cq, a.offs, a.key_base, stream));
            if (need > temp_bytes) { err = "internal error: the sort's temporary storage"; return ERR_DEVICE; }
            HIP_TRY(sort_segments(d_temp, need, d_keys_a, d_keys_b, (uint32_t)hits, (uint32_t)cq, a.offs, a.key_base, stream));
            const GraphRows mine = rows_at(out, h_off[qa], 1);  // the pass's slots of the caller's arrays
            const GraphRows& to = host ? staged : mine;
            hipLaunchKernelGGL(exact_range_decode_kernel, dim3((uint32_t)((hits + 255) / 256)), dim3(256), 0, stream, v, d_keys_b, (uint32_t)hits,
                               st->order(), to.ids, to.dists, to.layer, to.rank);
            HIP_TRY(hipGetLastError());
            if (host) {
                const int rc = copy_rows_out(mine, staged, hits, 0, stream, err);
                if (rc != OK) return rc;
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

}  // namespace

// The device side of hnswgpu_exact_range_search_batch(_device); capi.cpp holds the entries and every argument check (capi_index.hpp).
int exact_range(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, bool host, void* stream, std::string& err) {
    if (!host) return exact_range_passes(dev, origin_id, a, false, a.allowed, static_cast<hipStream_t>(stream), err);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    FilterUpload filter;
    const int rc = filter.put(a.allowed, a.n_allowed, err);
    if (rc != OK) return rc;
    return exact_range_passes(dev, origin_id, a, true, filter.d_allowed, nullptr, err);
}

}  // namespace hnswgpu
