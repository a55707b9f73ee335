// exact_knn.hip -- exhaustive exact k-NN over every point of an uploaded index, filter included (gfx950 only):
// hnswgpu_exact_search_batch / hnswgpu_exact_search_batch_device of include/hnsw_mi355x.h, and the device side of
// hnswgpu_exact_search_batch_filter_set / _device (a set of filters, each query naming its own; the entries are in capi.cpp).
// DESIGN.md "Exact k-NN".
//
//   exact_knn_prep_kernel   the queries of a chunk, zero padded and regrouped by tiles of TQ queries (element-chunk major),
//                           DistCosine: + every query's squared norm in the crate's arithmetic
//   exact_knn_slab_kernel   one wavefront per (tile of TQ queries, slab of rows): ONE ROW PER LANE, the row's float4 is read once
//                           and used for the TQ queries of the tile, whose elements are wave-uniform (scalar loads: they are the
//                           SGPR operand of the per-element instruction).  Every (query, row) pair is one left-to-right chain in
//                           one lane, made of the search's own per-element terms (search_kernels.inc) -- bit for bit the f32 the
//                           search computes.  Selection: per (query, slab) a sorted list of the min(k, n) smallest 64-bit keys
//                           {distance bits, DataId rank} with a running threshold (the list's last key once it is full): after the
//                           warm-up a row costs one 64-bit compare per query.
//   exact_knn_merge_kernel  one wavefront per query: the slabs' lists merged (lane s holds the head of slab s), the answers written
//
// Filter set: the slab kernel's SET variant keeps a 16-bit eligibility mask per lane (bit t: the row's bit in the bitmap of the
// filter that query t of the tile names), so a tile may mix filters; the prep and merge kernels reach a query through an optional
// list (a group's queries tiled densely, wherever they sit in the batch).
//
// Keys are unique (the rank is a permutation), so every step is deterministic and a tie group is cut at position k by DataId --
// and a query's answer does not depend on which tile, group or chunk it is served in.
//
// Range search (the device side of hnswgpu_exact_range_search_batch / _device; the entries are in capi.cpp): every eligible row
// with dist <= the query's radius, in the same key order.  DESIGN.md "Exact range search".
//   exact_range_slab_kernel    the slab kernel's tile and chain without the lists.  Count pass: a ballot and a popcount per
//                              (query, 64 rows) into a counter per (query, slab).  Fill pass: the same loop, the hitting lanes
//                              write their keys, compacted by the ballot's prefix, at the (query, slab) base.
//   exact_range_scan_kernel    the counters, query major and slab minor, into the CSR offsets and into each slab's base
//   (rocPRIM)                  every query's segment of keys sorted ascending
//   exact_range_decode_kernel  keys into ids, distances and p_ids
//
// Queries by stored point (the device side of hnswgpu_graph_search_batch / hnswgpu_exact_graph_batch and their _device forms; the
// entries are in capi.cpp): the k-NN graph of the indexed points, the point itself left out by identity.  DESIGN.md "Queries by
// stored point".  Exact: exact_knn_prep_rows_kernel tiles the rows themselves and the slab kernel's SELF variant skips each
// query's own rank.  Approximate: graph_gather_kernel, the batched search with knbn = k + 1, graph_compact_kernel.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>
#include <exception>
#include <numeric>
#include <vector>

#include "capi_index.hpp"
#include "graph_internal.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "search_kernels.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "search_kernels.inc"  // the per-element terms and the last step of Distance::eval, shared with the search

namespace hnswgpu {
namespace {

constexpr int TQ = 16;                          // queries per wavefront (one accumulator each per lane)
constexpr uint64_t KEY_NONE = ~0ull;            // behind every key: the threshold of a list that is not full yet
constexpr uint32_t MIN_SLAB_ROWS = 256;
constexpr uint32_t MAX_SLABS = 64;              // the merge keeps one slab per lane
constexpr uint64_t SCRATCH_BUDGET = 320ull << 20;  // bytes of scratch per call at most, whatever nq and n are

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const v4f* qtile_ptr_t;  // wave-uniform addresses: scalar loads
typedef __attribute__((address_space(4))) const uint32_t* uword_ptr_t;

struct ExactKnnArgs {
    const float* qt;        // [tiles][nchunk][TQ] float4: element chunk c of the tile's TQ queries side by side, zero padded
    const double* qnorm;    // [tiles * TQ] DistCosine: the queries' squared norms
    const uint32_t* rank;   // [n] position of flat id f in ascending (DataId, flat id) order
    const uint32_t* order;  // [n] its inverse
    const uint32_t* allow;  // one bit per flat id, or nullptr: no filter
    const double* nrm2;     // DistCosine: side array of the points' squared norms, or nullptr: in the rows
    uint64_t* lists;        // [tiles][n_slabs][TQ][cap] ascending keys
    uint32_t* lens;         // [tiles][n_slabs][TQ]
    uint32_t nq;            // queries of this chunk
    uint32_t nchunk;        // float4 chunks of a row that hold data: ceil(d / 4)
    uint32_t cap;           // min(k, n)
    uint32_t slab_rows;     // a multiple of 64
    uint32_t n_slabs;       // <= MAX_SLABS
    uint32_t k;
    uint64_t* out_ids;      // the chunk's rows of the caller's arrays
    float* out_dists;
    uint8_t* out_layer;
    int32_t* out_rank;
    uint32_t* out_counts;
    // (behind everything the kernels of the one-filter call read: their code does not move)
    const uint32_t* qlist;  // tile slot -> row of the caller's arrays, or nullptr: the slot's own number
    const uint32_t* tword;  // [tiles * TQ] filter set: first word of the slot's bitmap in `allow` (prep kernel)
    const uint32_t* self_rank;  // [tiles * TQ] k-NN graph: the slot's query is the stored point of this DataId rank (prep kernel), never its own answer
};

// (dist_order_bits, the order of a key's upper half, is in graph_internal.hpp: symmetric_graph.hip builds the same keys)
// A key: order bits above, the DataId rank below.  Every NaN has the same order bits and comes back as the canonical quiet NaN.
__device__ __forceinline__ uint64_t make_key(float v, uint32_t rank) { return ((uint64_t)dist_order_bits(v) << 32) | rank; }
__device__ __forceinline__ float dist_of_key(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    if (u == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {
    return ((uint64_t)readlane_u((uint32_t)(v >> 32), lane) << 32) | readlane_u((uint32_t)v, lane);
}
__device__ __forceinline__ uint64_t first_lane_u64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// the lists are private to one wavefront; what one lane stored another lane loads later
__device__ __forceinline__ void list_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// four more elements of one (query, row) chain, left to right (round_chain's terms, one lane per row instead of a lane group)
template <int METRIC, typename ACC>
__device__ __forceinline__ void chain4(ACC& acc, const float4 q, const float4 x) {
    if constexpr (METRIC == DIST_JENSENSHANNON) {
        float ta, tb;
        jensenshannon_terms(q.x, x.x, ta, tb); acc = acc + ta; acc = acc + tb;
        jensenshannon_terms(q.y, x.y, ta, tb); acc = acc + ta; acc = acc + tb;
        jensenshannon_terms(q.z, x.z, ta, tb); acc = acc + ta; acc = acc + tb;
        jensenshannon_terms(q.w, x.w, ta, tb); acc = acc + ta; acc = acc + tb;
    } else if constexpr (METRIC == DIST_HELLINGER) {
        acc = acc + hellinger_term(q.x, x.x); acc = acc + hellinger_term(q.y, x.y);
        acc = acc + hellinger_term(q.z, x.z); acc = acc + hellinger_term(q.w, x.w);
    } else if constexpr (METRIC == DIST_JEFFREYS) {
        acc = acc + jeffreys_term(q.x, x.x); acc = acc + jeffreys_term(q.y, x.y);
        acc = acc + jeffreys_term(q.z, x.z); acc = acc + jeffreys_term(q.w, x.w);
    } else {
        const v2f lo = term2<METRIC>(v2f{q.x, q.y}, v2f{x.x, x.y});
        const v2f hi = term2<METRIC>(v2f{q.z, q.w}, v2f{x.z, x.w});
        acc = acc + (ACC)lo.x; acc = acc + (ACC)lo.y; acc = acc + (ACC)hi.x; acc = acc + (ACC)hi.y;
    }
}

struct ListState {
    uint32_t len;
    uint64_t thr;  // KEY_NONE until the list is full, then its last key
};
// the keys of the lanes in `mask` go into the sorted list (all lanes take part; everything but `key` is wave-uniform)
__device__ __attribute__((noinline)) ListState list_insert(uint64_t* list, uint32_t cap, ListState s, uint64_t key, uint64_t mask) {
    const uint32_t lane = threadIdx.x;
    // (arguments arrive in vector registers: say that they are wave-uniform, the loops below are scalar control flow then)
    mask = first_lane_u64(mask);
    cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)cap);
    s.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.len);
    s.thr = first_lane_u64(s.thr);
    while (mask != 0ull) {
        const int b = ctz64(mask);
        mask &= mask - 1ull;
        const uint64_t kb = readlane_u64(key, b);
        if (!(kb < s.thr)) continue;  // an earlier key of this mask moved the threshold
        // the entries above kb move up one slot, chunk by chunk from the tail (a chunk is loaded whole before it is stored); the
        // one that falls off a full list is dropped.  Sorted: the entries below kb are a prefix, the walk ends in their chunk.
        uint32_t pos = 0;
        for (uint32_t c = (s.len + 63u) >> 6; c-- > 0u;) {
            const uint32_t i = (c << 6) + lane;
            const bool have = i < s.len;
            const uint64_t v = have ? list[i] : KEY_NONE;
            const bool below = have && v < kb;
            const unsigned long long bm = __ballot(below);
            if (have && !below && i + 1u < cap) list[i + 1u] = v;
            if (bm != 0ull) { pos = (c << 6) + popc64(bm); break; }
        }
        if (lane == 0u) list[pos] = kb;
        if (s.len < cap) ++s.len;
        list_fence();
        if (s.len == cap) s.thr = first_lane_u64(list[cap - 1u]);
    }
    return s;
}

// SET: `allow` holds one bitmap of ceil(n / 32) words per filter of the group and every query of the tile names its own
// (a.tword); else one bitmap (or none) for all.
// SELF (k-NN graph): every query of the tile is a stored point, named by its DataId rank (a.self_rank), and that one row -- the
// point itself, not its copies and not the other points of its DataId -- is never inserted into the query's lists.
template <int METRIC, bool SET, bool SELF>
// (the two distances that go through ln_f32 get twice the registers: their inner loop spilled at four waves per SIMD)
__global__ __launch_bounds__(64, METRIC == DIST_JEFFREYS || METRIC == DIST_JENSENSHANNON ? 2 : 4) void exact_knn_slab_kernel(DeviceIndexView ix, ExactKnnArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    const uint32_t lane = threadIdx.x;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t nvalid = a.nq - tile * (uint32_t)TQ < (uint32_t)TQ ? a.nq - tile * (uint32_t)TQ : (uint32_t)TQ;
    const uint32_t nchunk = a.nchunk, cap = a.cap;
    const size_t slot = ((size_t)tile * a.n_slabs + slab) * (size_t)TQ;
    uint64_t* const lists = a.lists + slot * cap;
    const qtile_ptr_t qc = (qtile_ptr_t)(reinterpret_cast<const v4f*>(a.qt) + (size_t)tile * nchunk * (size_t)TQ);
    // DistCosine rows that carry their norm in their last 8 bytes: when the last data chunk is the row's last chunk, its .z/.w
    // are those bytes, not the zero padding the sum expects (norm_fits_row: they lie behind element d - 1)
    const bool norm_in_tail = METRIC == DIST_COSINE && a.nrm2 == nullptr && nchunk * 4u == ix.row_stride;
    ListState st[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) st[t] = ListState{0u, KEY_NONE};
    // filter set: where the bitmap of each query's filter starts (wave-uniform: scalar registers); the slots behind the last
    // query of a part-filled tile never insert
    uint32_t tword[TQ];
    bool one_filter = true;  // every query of the tile names the same filter: one word per step serves all
    if constexpr (SET) {
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            tword[t] = ((uword_ptr_t)a.tword)[tile * (uint32_t)TQ + (uint32_t)t];
            one_filter = one_filter && ((uint32_t)t >= nvalid || tword[t] == tword[0]);
        }
    }
    const uint32_t valid_bits = (1u << nvalid) - 1u;
    // the tile's own ranks are wave-uniform: one scalar load of 64 bytes, 16 scalar registers for the kernel's life (the compare
    // below then has a scalar operand and costs no vector register)
    uint32_t self[TQ];
    if constexpr (SELF) {
#pragma unroll
        for (int t = 0; t < TQ; ++t) self[t] = ((uword_ptr_t)a.self_rank)[tile * (uint32_t)TQ + (uint32_t)t];
    }

    for (uint32_t r0 = lo; r0 < hi; r0 += 64u) {
        const bool in = r0 + lane < hi;
        const uint32_t r = in ? r0 + lane : hi - 1u;  // lanes past the slab re-read its last row
        bool ok = in;
        uint32_t elig = 0u;  // SET: bit t = this row is eligible for query t
        if constexpr (SET) {
            const uint32_t* const w = a.allow + (r >> 5);
            const uint32_t sh = r & 31u;
            if (one_filter) {
                elig = ((w[tword[0]] >> sh) & 1u) != 0u ? valid_bits : 0u;
            } else {
                uint32_t word[TQ];  // one word per query, all loads issued before any is used
#pragma unroll
                for (int t = 0; t < TQ; ++t) word[t] = w[tword[t]];
#pragma unroll
                for (int t = 0; t < TQ; ++t) elig |= ((word[t] >> sh) & 1u) << t;
                elig &= valid_bits;
            }
            if (!in) elig = 0u;
            ok = elig != 0u;
        } else {
            if (a.allow != nullptr) ok = in && ((a.allow[r >> 5] >> (r & 31u)) & 1u) != 0u;
        }
        if (__ballot(ok) == 0ull) continue;  // (wave-uniform) nothing eligible for any query among these 64 rows
        const float* rowf = ix.vec + (size_t)r * ix.row_stride;
        const float4* row = reinterpret_cast<const float4*>(rowf);
        double s2 = 0.;
        if constexpr (METRIC == DIST_COSINE)
            s2 = a.nrm2 != nullptr ? a.nrm2[r] : *reinterpret_cast<const double*>(rowf + ix.row_stride - 2u);
        ACC acc[TQ];
#pragma unroll
        for (int t = 0; t < TQ; ++t) acc[t] = 0;
        float4 x = row[0];
        for (uint32_t c = 0; c < nchunk; ++c) {
            const float4 xn = row[c + 1u < nchunk ? c + 1u : c];  // (written as a prefetch; as compiled the load sits at the head of the loop and is waited for at once)
            if (norm_in_tail && c + 1u == nchunk) { x.z = 0.f; x.w = 0.f; }
#pragma unroll
            for (int t = 0; t < TQ; ++t) {
                const v4f q = qc[(size_t)c * TQ + t];
                chain4<METRIC, ACC>(acc[t], make_float4(q.x, q.y, q.z, q.w), x);
            }
            x = xn;
        }
        const uint32_t rk = a.rank[r];
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            if ((uint32_t)t < nvalid) {
                float v;
                if constexpr (METRIC == DIST_COSINE) {
                    const double s1 = ((nrm_ptr_t)a.qnorm)[tile * (uint32_t)TQ + (uint32_t)t];
                    v = 0.f;
                    if (s1 > 0. && s2 > 0.) {
                        const double du = 1. - acc[t] / __builtin_sqrt(s1 * s2);
                        v = (float)fmax(du, 0.);
                    }
                } else {
                    v = dist_finish<METRIC>(acc[t]);
                }
                const uint64_t key = make_key(v, rk);
                bool mine = SET ? ((elig >> t) & 1u) != 0u : ok;
                if constexpr (SELF) mine = mine && rk != self[t];
                const unsigned long long m = __ballot(mine && key < st[t].thr);
                if (m != 0ull) st[t] = list_insert(lists + (size_t)t * cap, cap, st[t], key, m);
            }
        }
    }
    if (lane < nvalid) {
        uint32_t len = 0;
#pragma unroll
        for (int t = 0; t < TQ; ++t)
            if (lane == (uint32_t)t) len = st[t].len;
        a.lens[slot + lane] = len;
    }
}

// one wavefront per query: lane s walks the list of slab s; the smallest head is the next answer
__global__ __launch_bounds__(64) void exact_knn_merge_kernel(DeviceIndexView ix, ExactKnnArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t qs = blockIdx.x;  // the query's slot in the chunk's tiles; q: its row in the caller's arrays
    const uint32_t q = a.qlist != nullptr ? a.qlist[qs] : qs;
    const uint32_t tile = qs / (uint32_t)TQ, t = qs % (uint32_t)TQ;
    const uint32_t k = a.k;
    const size_t slot = ((size_t)tile * a.n_slabs + (lane < a.n_slabs ? lane : 0u)) * (size_t)TQ + t;
    const uint64_t* list = a.lists + slot * a.cap;
    const uint32_t len = lane < a.n_slabs ? a.lens[slot] : 0u;
    uint32_t total = len;
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    const uint32_t cnt = total < k ? total : k;
    uint32_t h = 0;
    uint64_t cur = len > 0u ? list[0] : KEY_NONE;
    uint64_t mine = KEY_NONE;
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
        if (lane == (j & 63u)) mine = m;
        if ((j & 63u) == 63u || j + 1u == cnt) {  // 64 answers at a time, one per lane
            const uint32_t jj = (j & ~63u) + lane;
            if (jj <= j) {
                const uint32_t flat = a.order[(uint32_t)mine];
                uint32_t l = 0;
                while (l + 1 < NB_LAYER_MAX && flat >= ix.layer_offset[l + 1]) ++l;
                const size_t o = (size_t)q * k + jj;
                a.out_ids[o] = ix.origin_id[flat];
                a.out_dists[o] = dist_of_key(mine);
                if (a.out_layer) a.out_layer[o] = (uint8_t)l;
                if (a.out_rank) a.out_rank[o] = (int32_t)(flat - ix.layer_offset[l]);
            }
        }
    }
    for (uint32_t j = cnt + lane; j < k; j += 64u) {  // slots behind the answers: zero, as the search entries leave them
        const size_t o = (size_t)q * k + j;
        a.out_ids[o] = 0ull;
        a.out_dists[o] = 0.f;
        if (a.out_layer) a.out_layer[o] = 0;
        if (a.out_rank) a.out_rank[o] = 0;
    }
    if (lane == 0u) a.out_counts[q] = cnt;
}

// one thread per query slot of the chunk's tiles: the row into its tile (slots behind the last query: zeros).  Slot qs holds row
// qlist[qs] of src (qlist == nullptr: row qs).  Filter set (tword != nullptr): the first word of the bitmap that row's filter has
// in the group's bitmaps, slot_of[row] * words -- the caller bounds the bitmaps of a group to 2^32 words.
__global__ void exact_knn_prep_kernel(const float* __restrict__ src, uint32_t nq, uint32_t d, uint32_t nchunk, uint32_t n_slots,
                                      float* __restrict__ qt, double* __restrict__ qnorm, const uint32_t* __restrict__ qlist,
                                      const uint32_t* __restrict__ slot_of, uint32_t words, uint32_t* __restrict__ tword) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= n_slots) return;
    const uint32_t tile = qs / (uint32_t)TQ, t = qs % (uint32_t)TQ;
    const uint32_t q = qs < nq && qlist != nullptr ? qlist[qs] : qs;
    if (tword != nullptr) tword[qs] = qs < nq ? slot_of[q] * words : 0u;
    double s1 = 0.;  // DistCosine: f32 squares widened to f64, summed left to right (finish_staged_query)
    for (uint32_t c = 0; c < nchunk; ++c) {
        float e[4];
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t i = 4u * c + j;
            e[j] = qs < nq && i < d ? src[(size_t)q * d + i] : 0.f;
            s1 = s1 + (double)(e[j] * e[j]);
        }
        reinterpret_cast<float4*>(qt)[((size_t)tile * nchunk + c) * (size_t)TQ + t] = make_float4(e[0], e[1], e[2], e[3]);
    }
    qnorm[qs] = s1;
}

// k-NN graph: the same tiles from the index's own rows -- slot qs holds the stored point flat[qs], its first d elements (what lies
// behind them in the padded row, a DistCosine norm included, never reaches the tile), the squared norm summed as above, so the
// bits are those of the point's vector brought as a query -- and the slot's own DataId rank (slots behind the last: no rank)
__global__ void exact_knn_prep_rows_kernel(DeviceIndexView ix, const uint32_t* __restrict__ flat, const uint32_t* __restrict__ rank, uint32_t nq,
                                           uint32_t nchunk, uint32_t n_slots, float* __restrict__ qt, double* __restrict__ qnorm,
                                           uint32_t* __restrict__ self_rank) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= n_slots) return;
    const uint32_t tile = qs / (uint32_t)TQ, t = qs % (uint32_t)TQ;
    const uint32_t f = qs < nq ? flat[qs] : 0u;
    const float* src = ix.vec + (size_t)f * ix.row_stride;
    double s1 = 0.;
    for (uint32_t c = 0; c < nchunk; ++c) {
        float e[4];
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t i = 4u * c + j;
            e[j] = qs < nq && i < ix.d ? src[i] : 0.f;
            s1 = s1 + (double)(e[j] * e[j]);
        }
        reinterpret_cast<float4*>(qt)[((size_t)tile * nchunk + c) * (size_t)TQ + t] = make_float4(e[0], e[1], e[2], e[3]);
    }
    qnorm[qs] = s1;
    self_rank[qs] = qs < nq ? rank[f] : 0xFFFFFFFFu;
}

template <bool SET, bool SELF>
hipError_t launch_slab_of(int metric, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const ExactKnnArgs& a) {
    switch (metric) {
        case DIST_L2: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_L2, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_COSINE: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_COSINE, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_DOT: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_DOT, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_L1: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_L1, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_HELLINGER: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_HELLINGER, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_JEFFREYS: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_JEFFREYS, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_JENSENSHANNON: hipLaunchKernelGGL((exact_knn_slab_kernel<DIST_JENSENSHANNON, SET, SELF>), grid, dim3(64), 0, stream, ix, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_slab(int metric, bool set, bool self, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const ExactKnnArgs& a) {
    if (self) return launch_slab_of<false, true>(metric, grid, stream, ix, a);  // (the graph calls take one filter or none)
    return set ? launch_slab_of<true, false>(metric, grid, stream, ix, a) : launch_slab_of<false, false>(metric, grid, stream, ix, a);
}

// What a replica keeps for this unit (DeviceIndex::extension): the DataId ranks, and scratch blocks that calls take turns with
struct ExactState {
    int device = -1;
    void* d_rank = nullptr;
    void* d_order = nullptr;
    std::mutex mu;
    std::vector<std::pair<void*, uint64_t>> pool;  // free scratch blocks {address, bytes}
    ~ExactState() {
        DeviceGuard on(device);
        if (d_rank) (void)hipFree(d_rank);
        if (d_order) (void)hipFree(d_order);
        for (auto& b : pool) (void)hipFree(b.first);
    }
};
struct ScratchLease {
    ExactState* st;
    void* p = nullptr;
    uint64_t bytes = 0;
    explicit ScratchLease(ExactState* s) : st(s) {}
    hipError_t take(uint64_t need) {
        {
            std::lock_guard<std::mutex> g(st->mu);
            if (!st->pool.empty()) { p = st->pool.back().first; bytes = st->pool.back().second; st->pool.pop_back(); }
        }
        // (HNSWGPU_POISON_SCRATCH: the block a call takes, reused or new, is nobody's over its whole size)
        if (bytes >= need) return poison_scratch(p, bytes);
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = need;
        return poison_scratch(p, bytes);
    }
    ~ScratchLease() {
        if (!p) return;
        std::lock_guard<std::mutex> g(st->mu);
        st->pool.emplace_back(p, bytes);
    }
};
// a call's block from the pool, sized by the arrays that `lay` names and divided among them
int take_layout(const char* what, ScratchLease& lease, ScratchLayout& lay, std::string& err) {
    HIP_TRY(lease.take(lay.size()));
    if (lay.place(lease.p, lease.bytes)) return OK;
    err = std::string(what) + ": scratch layout";
    return ERR_FORMAT;
}

// rank[f] = position of flat id f in ascending (origin id, flat id) order, and the inverse: once per replica, on the host
std::shared_ptr<void> make_state(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, std::string& err) {
    const uint32_t n = dev.view().n;
    if (origin_id.size() != n) { err = "internal error: the host view and the replica differ"; return nullptr; }
    std::vector<uint32_t> order(n), rank(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return origin_id[x] < origin_id[y]; });
    for (uint32_t i = 0; i < n; ++i) rank[order[i]] = i;
    std::shared_ptr<ExactState> st(new ExactState());
    st->device = dev.device();
    auto put = [&](void** p, const std::vector<uint32_t>& h) {
        hipError_t e = hipMalloc(p, (size_t)n * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(*p, h.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) err = std::string("exact search: uploading the id ranks: ") + hipGetErrorString(e);
        return e == hipSuccess;
    };
    if (!put(&st->d_rank, rank) || !put(&st->d_order, order)) return nullptr;
    return st;
}

// A filter set behind a call (device pointers), and the knob that bounds the bitmaps one launch holds
struct SetCall {
    const FilterSet* fs;
    uint64_t bitmap_budget;  // HNSWGPU_FILTER_SET_MB in bytes
};
constexpr uint64_t MAX_FILTER_SET_WAVES = 1ull << 31;  // allow_bitmap_set_kernel: four wavefronts per workgroup, 2^29 workgroups

// the device path: every pointer is device memory; waits for `stream` before it returns.
// set == nullptr: no filter, or one for the batch (d_allowed).  Else query q is answered under filter fs->filter_of[q]: the
// bitmaps are built group by group -- as many consecutive filters as the bound and this unit's scratch budget hold -- and per group
// its queries are listed (launch_filter_group), tiled densely and searched; one group (the usual case): all queries in batch order.
// d_self != nullptr (k-NN graph; no set): query q is the stored point of flat id d_self[q], d_queries is not read, and the point
// itself is no candidate of its own row.
int exact_device(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const float* d_queries, uint64_t nq, uint64_t d,
                 uint64_t k, const uint64_t* d_allowed, uint64_t n_allowed, bool filtered, const SetCall* set, uint64_t* d_out_ids,
                 float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, hipStream_t stream, std::string& err,
                 const uint32_t* d_self = nullptr) {
    const DeviceIndexView& v = dev.view();
    if (nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    std::string serr;
    std::shared_ptr<void> ext = dev.extension([&]() { return make_state(dev, origin_id, serr); });
    if (!ext) { err = serr.empty() ? "exact search: no device state" : serr; return ERR_DEVICE; }
    ExactState* st = static_cast<ExactState*>(ext.get());

    const uint64_t n = v.n;
    const uint64_t cap = std::min<uint64_t>(k, n);
    const uint64_t nchunk = (d + 3) / 4;
    const uint64_t tiles_total = (nq + TQ - 1) / TQ;
    // slabs: enough (tile, slab) wavefronts to fill the device, never more lists than the budget holds for one tile
    uint64_t slabs = std::min<uint64_t>(MAX_SLABS, (8192 + tiles_total - 1) / tiles_total);
    const uint64_t words = (n + 31) / 32, slot_bytes = words * 4;
    // in front of the tiles: the bitmap -- or, for a filter set, the bitmaps of a group (at most half of the budget), two words of
    // counters and, when there is more than one group, the list of a group's queries and every query's slot
    uint64_t per_group = 1, groups = 1, ctrl_bytes = 0, qlist_bytes = 0;
    if (set) {
        if (set->bitmap_budget < slot_bytes) {
            err = "HNSWGPU_FILTER_SET_MB is smaller than one filter's bitmap (" + std::to_string(slot_bytes) + " bytes for this index)";
            return ERR_ARG;
        }
        per_group = std::min<uint64_t>({set->bitmap_budget / slot_bytes, (SCRATCH_BUDGET / 2) / slot_bytes, set->fs->n_filters,
                                        MAX_FILTER_SET_WAVES / ((n + 63) / 64) - 1});
        if (per_group == 0) { err = "index too large for the exact search's scratch budget"; return ERR_ARG; }
        groups = (set->fs->n_filters + per_group - 1) / per_group;
        ctrl_bytes = 256;
        if (groups > 1) qlist_bytes = round_up(nq * 4, 256);
    }
    const uint64_t allow_bytes = round_up(per_group * slot_bytes, 256) + ctrl_bytes + 2 * qlist_bytes;
    const uint64_t fixed_bytes = allow_bytes + round_up(TQ * (nchunk * 16 + 8), 256) + 4096;  // the bitmap(s) and one tile's queries
    if (fixed_bytes >= SCRATCH_BUDGET) { err = "index, batch or dimension too large for the exact search's scratch budget"; return ERR_ARG; }
    const uint64_t list_budget = SCRATCH_BUDGET - fixed_bytes;
    slabs = std::min(slabs, list_budget / ((uint64_t)TQ * (cap * 8 + 4)));
    if (slabs == 0) { err = "knbn too large for the exact search's scratch budget"; return ERR_ARG; }
    const uint64_t slab_rows = std::max<uint64_t>(MIN_SLAB_ROWS, round_up((n + slabs - 1) / slabs, 64));
    slabs = (n + slab_rows - 1) / slab_rows;
    // queries per chunk: whole tiles, what the budget holds, a grid the launch accepts
    const uint64_t tword_bytes = set ? round_up(TQ * 4, 256) : 0;
    const uint64_t self_bytes = d_self ? round_up(TQ * 4, 256) : 0;
    const uint64_t per_tile = round_up(nchunk * TQ * 16, 256) + round_up(TQ * 8, 256) + round_up(slabs * TQ * cap * 8, 256) + round_up(slabs * TQ * 4, 256) +
                              tword_bytes + self_bytes;
    const uint64_t chunk_tiles = std::min<uint64_t>({tiles_total, (SCRATCH_BUDGET - allow_bytes) / per_tile, 65535});
    if (chunk_tiles == 0) { err = "knbn too large for the exact search's scratch budget"; return ERR_ARG; }

    // (a per-tile array: every tile's part padded, tile behind tile)
    uint32_t *d_allow, *d_ctrl, *d_qlist, *d_slot_of, *d_lens, *d_tword = nullptr, *d_self_rank = nullptr;
    float* d_qt;
    double* d_qnorm;
    uint64_t* d_lists;
    ScratchLayout lay;
    lay.array(d_allow, per_group * words);
    lay.bytes(d_ctrl, ctrl_bytes);  // [0] entries of filter_of that name no filter, [1] queries of the group
    lay.bytes(d_qlist, qlist_bytes);
    lay.bytes(d_slot_of, qlist_bytes);
    lay.bytes(d_qt, chunk_tiles * round_up(nchunk * TQ * 16, 256));
    lay.bytes(d_qnorm, chunk_tiles * round_up(TQ * 8, 256));
    lay.bytes(d_lists, chunk_tiles * round_up(slabs * TQ * cap * 8, 256));
    lay.bytes(d_lens, chunk_tiles * round_up(slabs * TQ * 4, 256));
    if (set) lay.bytes(d_tword, chunk_tiles * tword_bytes);
    if (d_self) lay.bytes(d_self_rank, chunk_tiles * self_bytes);
    if (lay.size() != allow_bytes + chunk_tiles * per_tile) {  // (what the budget above counted: before anything is taken)
        err = "exact search: scratch layout";
        return ERR_FORMAT;
    }
    ScratchLease lease(st);
    const int rc_lease = take_layout("exact search", lease, lay, err);
    if (rc_lease != OK) return rc_lease;

    // whatever happens, nothing of this call is still running when the scratch block goes back to the pool
    Drain drain{stream};

    // `count` queries in chunks of whole tiles: slot i of the tiles is query qlist[i] (nullptr: query i) of the batch, searched
    // under the bitmap slot_of[that query] of the group (filter set only)
    auto run = [&](const uint32_t* qlist, uint64_t count, const uint32_t* slot_of) -> int {
        const uint64_t tiles_all = (count + TQ - 1) / TQ;
        for (uint64_t t0 = 0; t0 < tiles_all; t0 += chunk_tiles) {
            const uint64_t tiles = std::min(chunk_tiles, tiles_all - t0);
            const uint64_t q0 = t0 * TQ, cq = std::min<uint64_t>(tiles * TQ, count - q0);
            const uint64_t row0 = qlist ? 0 : q0;  // a list names rows of the whole batch; without one the chunk's rows start at q0
            ExactKnnArgs a{};
            a.qt = d_qt;
            a.qnorm = d_qnorm;
            a.rank = static_cast<const uint32_t*>(st->d_rank);
            a.order = static_cast<const uint32_t*>(st->d_order);
            a.allow = filtered || set ? d_allow : nullptr;
            a.nrm2 = dev.side_norms();
            a.lists = d_lists;
            a.lens = d_lens;
            a.nq = (uint32_t)cq;
            a.nchunk = (uint32_t)nchunk;
            a.cap = (uint32_t)cap;
            a.slab_rows = (uint32_t)slab_rows;
            a.n_slabs = (uint32_t)slabs;
            a.k = (uint32_t)k;
            a.out_ids = d_out_ids + row0 * k;
            a.out_dists = d_out_dists + row0 * k;
            a.out_layer = d_out_layer ? d_out_layer + row0 * k : nullptr;
            a.out_rank = d_out_rank ? d_out_rank + row0 * k : nullptr;
            a.out_counts = d_out_counts + row0;
            a.qlist = qlist ? qlist + q0 : nullptr;
            a.tword = d_tword;
            a.self_rank = d_self_rank;
            const uint32_t n_slots = (uint32_t)(tiles * TQ);
            if (d_self)
                hipLaunchKernelGGL(exact_knn_prep_rows_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, v, d_self + row0, a.rank, (uint32_t)cq,
                                   (uint32_t)nchunk, n_slots, d_qt, d_qnorm, d_self_rank);
            else
                hipLaunchKernelGGL(exact_knn_prep_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, d_queries + row0 * d, (uint32_t)cq,
                                   (uint32_t)d, (uint32_t)nchunk, n_slots, d_qt, d_qnorm, a.qlist, slot_of ? slot_of + row0 : nullptr, (uint32_t)words, d_tword);
            HIP_TRY(hipGetLastError());
            HIP_TRY(launch_slab(dev.dist(), set != nullptr, d_self != nullptr, dim3((uint32_t)slabs, (uint32_t)tiles), stream, v, a));
            hipLaunchKernelGGL(exact_knn_merge_kernel, dim3((uint32_t)cq), dim3(64), 0, stream, v, a);
            HIP_TRY(hipGetLastError());
        }
        return OK;
    };

    if (!set) {
        if (filtered) HIP_TRY(launch_allow_bitmap(stream, v.origin_id, v.n, d_allowed, n_allowed, d_allow));
        const int rc = run(nullptr, nq, nullptr);
        if (rc != OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        return OK;
    }
    // The slab kernel indexes the bitmaps with filter_of's values: the entries that name no filter are counted, and the count is
    // read back (while the first group's bitmaps are being built) before anything is searched or written.
    const FilterSet& fs = *set->fs;
    uint32_t h_ctrl[2] = {0u, 0u};
    HIP_TRY(hipMemsetAsync(d_ctrl, 0, 8, stream));
    HIP_TRY(launch_filter_of_check(stream, fs.filter_of, (uint32_t)nq, fs.n_filters, d_ctrl));
    HIP_TRY(launch_allow_bitmap_set(stream, v.origin_id, v.n, fs.ids, fs.offsets, 0, (uint32_t)per_group, d_allow));
    HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h_ctrl[0] != 0) {
        err = std::to_string(h_ctrl[0]) + " entries of filter_of name no filter of the set (>= n_filters = " + std::to_string(fs.n_filters) + ")";
        return ERR_ARG;
    }
    if (groups == 1) {
        const int rc = run(nullptr, nq, fs.filter_of);
        if (rc != OK) return rc;
    } else {
        for (uint64_t f0 = 0; f0 < fs.n_filters; f0 += per_group) {
            const uint32_t n_slots = (uint32_t)std::min<uint64_t>(per_group, fs.n_filters - f0);
            // (the stream is in order: the previous group's search is behind its bitmaps, its list and its slots)
            if (f0 != 0) HIP_TRY(launch_allow_bitmap_set(stream, v.origin_id, v.n, fs.ids, fs.offsets, (uint32_t)f0, n_slots, d_allow));
            HIP_TRY(hipMemsetAsync(d_ctrl + 1, 0, 4, stream));
            HIP_TRY(launch_filter_group(stream, fs.filter_of, (uint32_t)nq, (uint32_t)f0, n_slots, d_qlist, d_slot_of, d_ctrl + 1));
            HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            const uint32_t members = h_ctrl[1];
            if (members == 0) continue;  // a group without queries launches nothing
            const int rc = run(d_qlist, members, d_slot_of);
            if (rc != OK) return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

uint64_t filter_set_budget() {
    const int64_t knob = knobs().filter_set_bytes;
    return knob >= 0 ? (uint64_t)knob : 256ull << 20;
}

// ---------------------------------------------------------------------------------------------------------------- range search
constexpr uint64_t RANGE_HITS_PER_PASS = 8ull << 20;  // answers one fill pass holds at most (HNSWGPU_RANGE_HITS_PER_PASS), or one query's
constexpr uint64_t RANGE_TILE_BUDGET = 64ull << 20;   // bytes of tiled queries and counters per chunk of tiles

typedef __attribute__((address_space(4))) const float* ufloat_ptr_t;
typedef __attribute__((address_space(4))) const uint64_t* uquad_ptr_t;

struct ExactRangeArgs {
    const float* qt;        // as ExactKnnArgs
    const double* qnorm;
    const float* radius;    // [nq] the chunk's radii
    const uint32_t* rank;
    const uint32_t* allow;
    const double* nrm2;
    uint32_t* cnt;          // [nq][n_slabs]; count pass: the hits of (query, slab), written.  Fill pass: the hits of the query in the slabs
                            // before this one, read (nullptr: one slab)
    const uint64_t* offs;   // fill pass: [nq] where each query's answer starts among the batch's answers
    uint64_t* keys;         // fill pass: the chunk's keys, slot 0 being answer key_base of the batch; nullptr: count pass
    uint64_t key_base;
    uint32_t key_cap;       // slots behind keys
    uint32_t nq;
    uint32_t nchunk;
    uint32_t slab_rows;
    uint32_t n_slabs;
};

// At most this many waves per SIMD: without the lists the loop needs 40 VGPRs and eight waves would fit, but every wavefront
// streams its tile's queries through the scalar cache (8 KB per tile at d = 128), and with more tiles resident than the cache
// holds the scalar loads the loop waits for slow down: 1M x 128 DistL2, 10 000 queries, count pass 238 ms uncapped, 189 ms at
// five, 161 ms at four (the k-NN kernel's 88 VGPRs give it five).
#ifndef HNSW_RANGE_MAX_WAVES
#define HNSW_RANGE_MAX_WAVES 4
#endif
// exact_knn_slab_kernel's loop; per query of the tile the radius and the counter (fill pass: the next slot) are wave-uniform
template <int METRIC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(
    METRIC == DIST_JEFFREYS || METRIC == DIST_JENSENSHANNON ? 2 : (HNSW_RANGE_MAX_WAVES < 4 ? HNSW_RANGE_MAX_WAVES : 4), HNSW_RANGE_MAX_WAVES)))
void exact_range_slab_kernel(DeviceIndexView ix, ExactRangeArgs a) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    const uint32_t lane = threadIdx.x;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t nvalid = a.nq - tile * (uint32_t)TQ < (uint32_t)TQ ? a.nq - tile * (uint32_t)TQ : (uint32_t)TQ;
    const uint32_t nchunk = a.nchunk;
    const qtile_ptr_t qc = (qtile_ptr_t)(reinterpret_cast<const v4f*>(a.qt) + (size_t)tile * nchunk * (size_t)TQ);
    const bool norm_in_tail = METRIC == DIST_COSINE && a.nrm2 == nullptr && nchunk * 4u == ix.row_stride;
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

    for (uint32_t r0 = lo; r0 < hi; r0 += 64u) {
        const bool in = r0 + lane < hi;
        const uint32_t r = in ? r0 + lane : hi - 1u;  // lanes past the slab re-read its last row
        bool ok = in;
        if (a.allow != nullptr) ok = in && ((a.allow[r >> 5] >> (r & 31u)) & 1u) != 0u;
        if (__ballot(ok) == 0ull) continue;  // (wave-uniform) nothing eligible among these 64 rows
        const float* rowf = ix.vec + (size_t)r * ix.row_stride;
        const float4* row = reinterpret_cast<const float4*>(rowf);
        double s2 = 0.;
        if constexpr (METRIC == DIST_COSINE)
            s2 = a.nrm2 != nullptr ? a.nrm2[r] : *reinterpret_cast<const double*>(rowf + ix.row_stride - 2u);
        ACC acc[TQ];
#pragma unroll
        for (int t = 0; t < TQ; ++t) acc[t] = 0;
        float4 x = row[0];
        for (uint32_t c = 0; c < nchunk; ++c) {
            const float4 xn = row[c + 1u < nchunk ? c + 1u : c];
            if (norm_in_tail && c + 1u == nchunk) { x.z = 0.f; x.w = 0.f; }
#pragma unroll
            for (int t = 0; t < TQ; ++t) {
                const v4f q = qc[(size_t)c * TQ + t];
                chain4<METRIC, ACC>(acc[t], make_float4(q.x, q.y, q.z, q.w), x);
            }
            x = xn;
        }
        const uint32_t rk = fill ? a.rank[r] : 0u;
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            if ((uint32_t)t < nvalid) {
                float v;
                if constexpr (METRIC == DIST_COSINE) {
                    const double s1 = ((nrm_ptr_t)a.qnorm)[tile * (uint32_t)TQ + (uint32_t)t];
                    v = 0.f;
                    if (s1 > 0. && s2 > 0.) {
                        const double du = 1. - acc[t] / __builtin_sqrt(s1 * s2);
                        v = (float)fmax(du, 0.);
                    }
                } else {
                    v = dist_finish<METRIC>(acc[t]);
                }
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

// one thread per sorted key: the answer it stands for (exact_knn_merge_kernel's decoding; a -0 distance comes back as +0)
__global__ __launch_bounds__(256) void exact_range_decode_kernel(DeviceIndexView ix, const uint64_t* __restrict__ keys, uint32_t count,
                                                                const uint32_t* __restrict__ order, uint64_t* __restrict__ out_ids,
                                                                float* __restrict__ out_dists, uint8_t* __restrict__ out_layer,
                                                                int32_t* __restrict__ out_rank) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const uint64_t key = keys[j];
    const uint32_t rk = (uint32_t)key < ix.n ? (uint32_t)key : 0u;  // (a rank, whatever the slot holds)
    const uint32_t flat = order[rk];
    uint32_t l = 0;
    while (l + 1 < NB_LAYER_MAX && flat >= ix.layer_offset[l + 1]) ++l;
    out_ids[j] = ix.origin_id[flat];
    out_dists[j] = dist_of_key(key);
    if (out_layer) out_layer[j] = (uint8_t)l;
    if (out_rank) out_rank[j] = (int32_t)(flat - ix.layer_offset[l]);
}

hipError_t launch_range_slab(int metric, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const ExactRangeArgs& a) {
    switch (metric) {
        case DIST_L2: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_L2>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_COSINE: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_COSINE>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_DOT: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_DOT>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_L1: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_L1>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_HELLINGER: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_HELLINGER>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_JEFFREYS: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_JEFFREYS>), grid, dim3(64), 0, stream, ix, a); break;
        case DIST_JENSENSHANNON: hipLaunchKernelGGL((exact_range_slab_kernel<DIST_JENSENSHANNON>), grid, dim3(64), 0, stream, ix, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
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

// A call's buffers: plain host memory (host) or device memory; `allowed` is device memory either way
struct RangeCall {
    bool host;
    const float* queries;
    const float* radii;
    const uint64_t* d_allowed;
    uint64_t n_allowed;
    bool filtered;
    uint64_t cap;
    uint64_t* offsets;
    uint64_t* ids;
    float* dists;
    uint8_t* layer;
    int32_t* rank;
};

// Both entries.  Count pass over every query (host buffers: in blocks of at most 64 MB of queries), the offsets complete on the
// caller's side; then, when the total fits cap, the fill pass chunk by chunk of the plan: keys, sort, decode -- into the caller's
// arrays (device) or into a staging area that is copied out (host).  Waits for `stream` before it returns.
int exact_range_passes(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const RangeCall& io, uint64_t nq, uint64_t d, hipStream_t stream,
                       std::string& err) {
    const DeviceIndexView& v = dev.view();
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    if (nq == 0) {
        if (io.host) { io.offsets[0] = 0; return OK; }
        HIP_TRY(hipMemsetAsync(io.offsets, 0, 8, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return OK;
    }
    if (v.n == 0) {  // no point: every answer is empty
        if (io.host) { std::memset(io.offsets, 0, (nq + 1) * 8); return OK; }
        HIP_TRY(hipMemsetAsync(io.offsets, 0, (nq + 1) * 8, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return OK;
    }
    std::string serr;
    std::shared_ptr<void> ext = dev.extension([&]() { return make_state(dev, origin_id, serr); });
    if (!ext) { err = serr.empty() ? "exact range search: no device state" : serr; return ERR_DEVICE; }
    ExactState* st = static_cast<ExactState*>(ext.get());

    const uint64_t n = v.n;
    const uint64_t nchunk = (d + 3) / 4;
    const uint64_t tiles_total = (nq + TQ - 1) / TQ;
    uint64_t slabs = std::min<uint64_t>(MAX_SLABS, (8192 + tiles_total - 1) / tiles_total);
    const uint64_t slab_rows = std::max<uint64_t>(MIN_SLAB_ROWS, round_up((n + slabs - 1) / slabs, 64));
    slabs = (n + slab_rows - 1) / slab_rows;
    // more than one slab: fewer than 8192 tiles, the batch's counters are 1 MB at most and stay for the fill pass; one slab: a
    // query's base is its offset, the counters are a chunk's
    const bool keep = slabs > 1;
    const uint64_t words = (n + 31) / 32;
    const uint64_t tile_bytes = round_up(nchunk * TQ * 16, 256) + round_up(TQ * 8, 256);
    const uint64_t per_tile = tile_bytes + (keep ? 0 : TQ * 4);
    const uint64_t block_q = io.host ? std::max<uint64_t>(1, std::min<uint64_t>(nq, (64ull << 20) / (d * 4 + 12))) : nq;
    const uint64_t chunk_tiles = std::min<uint64_t>({(block_q + TQ - 1) / TQ, std::max<uint64_t>(1, RANGE_TILE_BUDGET / per_tile), 65535});
    const uint64_t cnt_bytes = round_up(keep ? nq * slabs * 4 : chunk_tiles * TQ * 4, 256);
    const int64_t knob = knobs().range_hits_per_pass;
    const uint64_t budget = knob > 0 ? (uint64_t)knob : RANGE_HITS_PER_PASS;
    const uint64_t max_fill_q = std::min<uint64_t>(block_q, chunk_tiles * TQ);
    // the keys of one fill pass: the budget, or one query's answer where that is larger -- never more than the caller has room for
    const uint64_t all_pairs = nq > 0xFFFFFFFFull / n ? 0xFFFFFFFFull : nq * n;
    const uint64_t key_cap = std::min<uint64_t>({std::max(budget, n), all_pairs, io.cap});
    if (key_cap > 0xFFFFFFF0ull) { err = "index too large for the exact range search"; return ERR_ARG; }
    size_t temp_bytes = 0;
    if (key_cap != 0)
        HIP_TRY(sort_segments(nullptr, temp_bytes, nullptr, nullptr, (uint32_t)key_cap, (uint32_t)max_fill_q, nullptr, 0, stream));

    // (d_qt, d_qnorm: every tile's part padded, tile behind tile; the s_ arrays: the staging of a host call)
    uint32_t *d_allow = nullptr, *d_cnt;
    float *d_qt, *s_dists = nullptr;
    double* d_qnorm;
    uint64_t *d_keys_a, *d_keys_b, *s_ids = nullptr;
    void* d_temp;
    int32_t* s_rank = nullptr;
    uint8_t* s_layer = nullptr;
    ScratchLayout lay;
    if (io.filtered) lay.array(d_allow, words);
    lay.bytes(d_qt, chunk_tiles * round_up(nchunk * TQ * 16, 256));
    lay.bytes(d_qnorm, chunk_tiles * round_up(TQ * 8, 256));
    lay.bytes(d_cnt, cnt_bytes);
    lay.arrays(key_cap, d_keys_a, d_keys_b);
    lay.bytes(d_temp, round_up(temp_bytes, 256));
    if (io.host) lay.arrays(key_cap, s_ids, s_dists, s_rank, s_layer);
    lay.skip(256);
    ScratchLease lease(st);
    const int rc_lease = take_layout("exact range search", lease, lay, err);
    if (rc_lease != OK) return rc_lease;

    DevMem m_q, m_rad, m_off;
    if (io.host) {
        HIP_TRY(m_q.alloc(block_q * d * 4));
        HIP_TRY(m_rad.alloc(block_q * 4));
        HIP_TRY(m_off.alloc((block_q + 1) * 8));
    }
    // the offsets on the host: the caller's array, or a copy of it (the plan of the fill pass is made here)
    std::vector<uint64_t> off_copy;
    if (!io.host) off_copy.resize(nq + 1);
    uint64_t* const h_off = io.host ? io.offsets : off_copy.data();
    h_off[0] = 0;

    Drain drain{stream};

    if (io.filtered) HIP_TRY(launch_allow_bitmap(stream, v.origin_id, v.n, io.d_allowed, io.n_allowed, d_allow));
    ExactRangeArgs a{};
    a.qt = d_qt;
    a.qnorm = d_qnorm;
    a.rank = static_cast<const uint32_t*>(st->d_rank);
    a.allow = d_allow;
    a.nrm2 = dev.side_norms();
    a.nchunk = (uint32_t)nchunk;
    a.slab_rows = (uint32_t)slab_rows;
    a.n_slabs = (uint32_t)slabs;
    // queries [q0, q0 + cq) of a block into the tiles
    auto prep = [&](const float* dq, uint64_t cq) -> int {
        const uint32_t n_slots = (uint32_t)((cq + TQ - 1) / TQ * TQ);
        hipLaunchKernelGGL(exact_knn_prep_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, dq, (uint32_t)cq, (uint32_t)d, (uint32_t)nchunk,
                           n_slots, d_qt, d_qnorm, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
        return OK;
    };
    const bool one_block = block_q >= nq;
    // where block [b0, b0 + bq) has its queries, radii and offsets on the device
    const float* dq = io.queries;
    const float* dr = io.radii;
    uint64_t* doff = io.offsets;
    auto stage_block = [&](uint64_t b0, uint64_t bq) -> int {
        if (!io.host) return OK;
        HIP_TRY(hipMemcpyAsync(m_q.p, io.queries + b0 * d, bq * d * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(m_rad.p, io.radii + b0, bq * 4, hipMemcpyHostToDevice, stream));
        dq = static_cast<const float*>(m_q.p);
        dr = static_cast<const float*>(m_rad.p);
        doff = static_cast<uint64_t*>(m_off.p);
        return OK;
    };

    // ---- the count pass
    for (uint64_t b0 = 0; b0 < nq; b0 += block_q) {
        const uint64_t bq = std::min(block_q, nq - b0);
        int rc = stage_block(b0, bq);
        if (rc != OK) return rc;
        for (uint64_t q0 = 0; q0 < bq; q0 += chunk_tiles * TQ) {
            const uint64_t cq = std::min<uint64_t>(chunk_tiles * TQ, bq - q0);
            if ((rc = prep(dq + q0 * d, cq)) != OK) return rc;
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
    if (total > io.cap) {
        err = "the answers need " + std::to_string(total) + " slots, cap is " + std::to_string(io.cap);
        return HNSWGPU_ERR_CAPACITY;
    }
    if (total == 0 || io.ids == nullptr) return OK;

    // ---- the fill pass
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
            const int rc = prep(dq + (qa - b0) * d, cq);
            if (rc != OK) return rc;
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
            const uint64_t o = h_off[qa];
            hipLaunchKernelGGL(exact_range_decode_kernel, dim3((uint32_t)((hits + 255) / 256)), dim3(256), 0, stream, v, d_keys_b, (uint32_t)hits,
                               static_cast<const uint32_t*>(st->d_order), io.host ? s_ids : io.ids + o, io.host ? s_dists : io.dists + o,
                               io.host ? (io.layer ? s_layer : nullptr) : (io.layer ? io.layer + o : nullptr),
                               io.host ? (io.rank ? s_rank : nullptr) : (io.rank ? io.rank + o : nullptr));
            HIP_TRY(hipGetLastError());
            if (io.host) {
                HIP_TRY(hipMemcpyAsync(io.ids + o, s_ids, hits * 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipMemcpyAsync(io.dists + o, s_dists, hits * 4, hipMemcpyDeviceToHost, stream));
                if (io.rank) HIP_TRY(hipMemcpyAsync(io.rank + o, s_rank, hits * 4, hipMemcpyDeviceToHost, stream));
                if (io.layer) HIP_TRY(hipMemcpyAsync(io.layer + o, s_layer, hits, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));  // the staging area is the next pass's
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// ------------------------------------------------------------------------------------------------------------------ k-NN graph
// Queries by stored point (the device side of hnswgpu_graph_search_batch / hnswgpu_exact_graph_batch and their _device forms; the
// entries are in capi.cpp).  DESIGN.md "Queries by stored point".
//   graph_resolve_kernel   DataIds into flat ids: a binary search over origin_id[order[.]], the first point of a repeated id
//   graph_gather_kernel    the first d elements of the named rows into a dense query matrix (approximate graph)
//   graph_compact_kernel   the search's (k + 1)-wide answers into the caller's k-wide rows, the point's own entry dropped
constexpr uint64_t GRAPH_SCRATCH = 256ull << 20;  // bytes of gathered queries and staged answers per chunk of points at most

// one thread per named point.  ids == nullptr: every point, row i being position i of the ascending (DataId, dump order) order.
// An id that no point carries is counted in *n_unknown (its slot gets flat id 0 and is never used: the call fails).
__global__ __launch_bounds__(256) void graph_resolve_kernel(const uint64_t* __restrict__ origin_id, const uint32_t* __restrict__ order, uint32_t n,
                                                           const uint64_t* __restrict__ ids, uint32_t np, uint32_t* __restrict__ flat,
                                                           uint32_t* __restrict__ n_unknown) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= np) return;
    if (ids == nullptr) { flat[i] = order[i]; return; }  // (the caller has checked np == n)
    const uint64_t id = ids[i];
    uint32_t lo = 0, hi = n;  // the first position whose id is >= id
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (origin_id[order[mid]] < id) lo = mid + 1u; else hi = mid;
    }
    uint32_t f = 0;
    if (lo < n && origin_id[order[lo]] == id) f = order[lo];
    else atomicAdd(n_unknown, 1u);
    flat[i] = f;
}

// one thread per element of the query matrix: q[i][j] = element j < d of the row of point flat[i].  The row's padding -- zeros, or
// a DistCosine norm in its last 8 bytes -- stays behind.
__global__ __launch_bounds__(256) void graph_gather_kernel(DeviceIndexView ix, const uint32_t* __restrict__ flat, uint64_t total, float* __restrict__ q) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const uint64_t i = e / ix.d;
    const uint32_t j = (uint32_t)(e - i * ix.d);
    q[e] = ix.vec[(size_t)flat[i] * ix.row_stride + j];
}

struct GraphRows {  // answers, row major
    uint64_t* ids;
    float* dists;
    uint8_t* layer;   // the caller's may be nullptr; the staged ones never are
    int32_t* rank;
    uint32_t* counts;
};
// one wavefront per row: the search's answer for the stored vector of point flat[row] with knbn = k + 1 (src) into the k-wide
// row of dst.  The entry whose p_id is the point's own is removed; when there is none and the answer is full, its last entry.
// The slots behind what remains are zeroed.
__global__ __launch_bounds__(64) void graph_compact_kernel(DeviceIndexView ix, const uint32_t* __restrict__ flat, GraphRows src, GraphRows dst, uint32_t k) {
    const uint32_t lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    const uint32_t k1 = k + 1u;
    const uint32_t cnt = src.counts[row] < k1 ? src.counts[row] : k1;
    const uint32_t own = flat[row];
    const size_t s0 = (size_t)row * k1, d0 = (size_t)row * k;
    uint32_t pos = 0xFFFFFFFFu;  // where the point's own entry is (a p_id names one point: at most one entry)
    for (uint32_t j = lane; j < cnt; j += 64u)
        if (ix.layer_offset[src.layer[s0 + j] < NB_LAYER_MAX ? src.layer[s0 + j] : NB_LAYER_MAX] + (uint32_t)src.rank[s0 + j] == own) pos = j;
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)pos, o, 64);
        pos = other < pos ? other : pos;
    }
    const uint32_t left = pos != 0xFFFFFFFFu ? cnt - 1u : (cnt < k ? cnt : k);
    for (uint32_t j = lane; j < k; j += 64u) {
        const bool have = j < left;
        const size_t s = s0 + (j < pos ? j : j + 1u);
        dst.ids[d0 + j] = have ? src.ids[s] : 0ull;
        dst.dists[d0 + j] = have ? src.dists[s] : 0.f;
        if (dst.layer) dst.layer[d0 + j] = have ? src.layer[s] : (uint8_t)0;
        if (dst.rank) dst.rank[d0 + j] = have ? src.rank[s] : 0;
    }
    if (lane == 0u) dst.counts[row] = left;
}

// A graph call's buffers: plain host memory (host) or device memory, point_ids and allowed too
struct GraphCall {
    bool host;
    const uint64_t* point_ids;  // nullptr: every point
    uint64_t np, k;
    GraphRows out;              // np rows of k slots
};

// the named points as flat ids in device memory (m_flat; word 0 of m_ctrl counts the unknown ids).  Returns ERR_ARG, nothing
// searched and no output written, when an id names no point.
int graph_resolve(const DeviceIndexView& v, const ExactState* st, const GraphCall& io, DevMem& m_flat, hipStream_t stream, std::string& err) {
    DevMem m_ids, m_ctrl;
    HIP_TRY(m_flat.alloc(io.np * sizeof(uint32_t)));
    HIP_TRY(m_ctrl.alloc(256));
    const uint64_t* d_ids = io.point_ids;
    if (io.host && io.point_ids != nullptr) {
        HIP_TRY(m_ids.alloc(io.np * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(m_ids.p, io.point_ids, io.np * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        d_ids = static_cast<const uint64_t*>(m_ids.p);
    }
    uint32_t unknown = 0;
    HIP_TRY(hipMemsetAsync(m_ctrl.p, 0, 4, stream));
    hipLaunchKernelGGL(graph_resolve_kernel, dim3((uint32_t)((io.np + 255) / 256)), dim3(256), 0, stream, v.origin_id, static_cast<const uint32_t*>(st->d_order),
                       v.n, d_ids, (uint32_t)io.np, static_cast<uint32_t*>(m_flat.p), static_cast<uint32_t*>(m_ctrl.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&unknown, m_ctrl.p, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (unknown != 0) {
        err = std::to_string(unknown) + " of the " + std::to_string(io.np) + " point_ids name no point of the index";
        return ERR_ARG;
    }
    return OK;
}

// rows [c0, c0 + ..) of k-wide answers
GraphRows rows_at(const GraphRows& r, uint64_t c0, uint64_t k) {
    return GraphRows{r.ids + c0 * k, r.dists + c0 * k, r.layer ? r.layer + c0 * k : nullptr, r.rank ? r.rank + c0 * k : nullptr, r.counts + c0};
}
// The one device staging of this unit for a chunk of k-NN answers, k slots a row: ids, dists, rank, counts and layer in one block,
// each 256-aligned -- and the way of a chunk's first cq rows out to host rows
struct AnswerStage {
    DevMem mem;
    GraphRows rows{};
    hipError_t alloc(uint64_t chunk, uint64_t k) {
        ScratchLayout lay;
        lay.arrays(chunk * k, rows.ids, rows.dists, rows.rank);
        lay.array(rows.counts, chunk);
        lay.array(rows.layer, chunk * k);
        const hipError_t e = mem.alloc(lay.size());
        if (e != hipSuccess) { mem.p = nullptr; return e; }
        return lay.place(mem.p, lay.size()) ? hipSuccess : hipErrorInvalidValue;
    }
    hipError_t copy_out(const GraphRows& dst, uint64_t cq, uint64_t k, hipStream_t stream) const {  // (dst.layer, dst.rank may be nullptr)
        hipError_t e = hipMemcpyAsync(dst.ids, rows.ids, cq * k * 8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst.dists, rows.dists, cq * k * 4, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && dst.rank) e = hipMemcpyAsync(dst.rank, rows.rank, cq * k * 4, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && dst.layer) e = hipMemcpyAsync(dst.layer, rows.layer, cq * k, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst.counts, rows.counts, cq * 4, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);  // the staging area is the next chunk's
        return e;
    }
};

// Host buffers of an exact k-NN call: queries and answers are staged in chunks of at most 64 MB, each chunk one call of the device
// path on the null stream.  d_set == nullptr: no filter, or one for the batch (d_allowed, on the device).  Else d_set's ids and offsets
// are on the device, and every chunk brings its own rows of filter_of (host memory) along.
int exact_host_chunks(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                      const uint64_t* d_allowed, uint64_t n_allowed, bool filtered, const FilterSet* d_set, const uint32_t* filter_of,
                      const GraphRows& out, std::string& err) {
    const uint64_t per_q = d * 4 + k * 17 + 4 + (d_set ? 4 : 0);
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(nq, (64ull << 20) / per_q));
    DevMem m_q, m_of;
    AnswerStage stage;
    HIP_TRY(m_q.alloc(chunk * d * 4));
    if (d_set) HIP_TRY(m_of.alloc(chunk * sizeof(uint32_t)));
    HIP_TRY(stage.alloc(chunk, k));
    const FilterSet chunk_set{d_set ? d_set->ids : nullptr, d_set ? d_set->offsets : nullptr, d_set ? d_set->n_filters : 0, static_cast<const uint32_t*>(m_of.p)};
    const SetCall call{&chunk_set, filter_set_budget()};
    for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint64_t cq = std::min(chunk, nq - q0);
        HIP_TRY(hipMemcpy(m_q.p, queries + q0 * d, cq * d * 4, hipMemcpyHostToDevice));
        if (d_set) HIP_TRY(hipMemcpy(m_of.p, filter_of + q0, cq * sizeof(uint32_t), hipMemcpyHostToDevice));
        const int rc = exact_device(dev, origin_id, static_cast<const float*>(m_q.p), cq, d, k, d_allowed, n_allowed, filtered, d_set ? &call : nullptr,
                                    stage.rows.ids, stage.rows.dists, stage.rows.layer, stage.rows.rank, stage.rows.counts, nullptr, err);
        if (rc != OK) return rc;
        HIP_TRY(stage.copy_out(rows_at(out, q0, k), cq, k, nullptr));
    }
    return OK;
}
// the host side of hnswgpu_exact_search_batch: the filter, when there is one, goes to the device once
int exact_host(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
               const uint64_t* allowed, uint64_t n_allowed, const GraphRows& out, std::string& err) {
    if (nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    DevMem m_allowed;  // (a filter that is empty still is a filter: a non-null pointer that is never dereferenced)
    if (allowed != nullptr) {
        HIP_TRY(m_allowed.alloc(std::max<uint64_t>(1, n_allowed) * sizeof(uint64_t)));
        if (n_allowed != 0) HIP_TRY(hipMemcpy(m_allowed.p, allowed, n_allowed * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    return exact_host_chunks(dev, origin_id, queries, nq, d, k, static_cast<const uint64_t*>(m_allowed.p), n_allowed, allowed != nullptr, nullptr, nullptr,
                             out, err);
}

}  // namespace

// The device side of hnswgpu_exact_search_batch_filter_set(_device); capi.cpp holds the entries and every argument check
// (capi_index.hpp).
int exact_filter_set(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactSetArgs& a, bool host, void* stream, std::string& err) {
    const GraphRows out{a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts};
    if (!host) {
        const SetCall set{&a.set, filter_set_budget()};
        return exact_device(dev, origin_id, a.queries, a.nq, a.d, a.k, nullptr, 0, false, &set, out.ids, out.dists, out.layer, out.rank, out.counts,
                            static_cast<hipStream_t>(stream), err);
    }
    // host buffers: the set goes to the device once; queries and answers go chunk by chunk (exact_host_chunks)
    if (a.nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const FilterSet& set = a.set;
    const uint64_t n_ids = set.offsets[set.n_filters];
    DevMem m_ids, m_off;
    HIP_TRY(m_ids.alloc(std::max<uint64_t>(1, n_ids) * sizeof(uint64_t)));  // (filters that are all empty: never read)
    HIP_TRY(m_off.alloc((set.n_filters + 1) * sizeof(uint64_t)));
    if (n_ids != 0) HIP_TRY(hipMemcpy(m_ids.p, set.ids, n_ids * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m_off.p, set.offsets, (set.n_filters + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    const FilterSet d_set{static_cast<const uint64_t*>(m_ids.p), static_cast<const uint64_t*>(m_off.p), set.n_filters, nullptr};
    return exact_host_chunks(dev, origin_id, a.queries, a.nq, a.d, a.k, nullptr, 0, false, &d_set, set.filter_of, out, err);
}

// The device side of hnswgpu_exact_range_search_batch(_device); capi.cpp holds the entries and every argument check (capi_index.hpp).
int exact_range(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, bool host, void* stream, std::string& err) {
    // (a filter that is empty still is a filter: a non-null pointer that is never dereferenced)
    RangeCall io{host, a.queries, a.radii, a.allowed, a.n_allowed, a.allowed != nullptr, a.cap, a.out_offsets, a.out_ids, a.out_dists, a.out_layer,
                 a.out_rank};
    if (!host) return exact_range_passes(dev, origin_id, io, a.nq, a.d, static_cast<hipStream_t>(stream), err);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    DevMem m_allowed;  // host buffers: the filter, when there is one, goes to the device once
    if (a.allowed != nullptr) {
        HIP_TRY(m_allowed.alloc(std::max<uint64_t>(1, a.n_allowed) * sizeof(uint64_t)));
        if (a.n_allowed != 0) HIP_TRY(hipMemcpy(m_allowed.p, a.allowed, a.n_allowed * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    io.d_allowed = static_cast<const uint64_t*>(m_allowed.p);
    return exact_range_passes(dev, origin_id, io, a.nq, a.d, nullptr, err);
}

// The device side of hnswgpu_graph_search_batch(_device) and hnswgpu_exact_graph_batch(_device); capi.cpp holds the entries and
// every argument check that needs no device (capi_index.hpp).  host: every buffer is plain host memory, else device memory.  Both wait
// for `stream` before they return.

// Approximate graph: chunk by chunk of at most HNSWGPU_GRAPH_CHUNK points (unset: what GRAPH_SCRATCH holds), the points' vectors
// gathered on the device, searched by the batched search itself with knbn = k + 1, and compacted into the caller's rows.
int graph_search(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, bool host, void* stream_v, std::string& err) {
    const uint64_t np = a.np, k = a.k, ef = a.ef;
    if (np == 0) return OK;
    const DeviceIndexView& v = dev.view();
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    std::string serr;
    std::shared_ptr<void> ext = dev.extension([&]() { return make_state(dev, origin_id, serr); });
    if (!ext) { err = serr.empty() ? "graph search: no device state" : serr; return ERR_DEVICE; }
    const ExactState* st = static_cast<const ExactState*>(ext.get());
    const GraphCall io{host, a.point_ids, np, k, {a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts}};
    DevMem m_flat, m_q;
    AnswerStage wide, stage;  // the search's (k + 1)-wide answers; a host call's k-wide ones
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)
    int rc = graph_resolve(v, st, io, m_flat, stream, err);
    if (rc != OK) return rc;
    const uint32_t* d_flat = static_cast<const uint32_t*>(m_flat.p);

    const uint64_t d = v.d, k1 = k + 1;
    const uint64_t per_point = d * 4 + k1 * 17 + 4 + (host ? k * 17 + 4 : 0);
    const int64_t knob = knobs().graph_chunk;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({np, GRAPH_SCRATCH / per_point, knob > 0 ? (uint64_t)knob : np}));
    HIP_TRY(m_q.alloc(chunk * d * 4));
    float* d_q = static_cast<float*>(m_q.p);
    HIP_TRY(wide.alloc(chunk, k1));
    if (host) HIP_TRY(stage.alloc(chunk, k));

    for (uint64_t c0 = 0; c0 < np; c0 += chunk) {
        const uint64_t cq = std::min(chunk, np - c0);
        hipLaunchKernelGGL(graph_gather_kernel, dim3((uint32_t)((cq * d + 255) / 256)), dim3(256), 0, stream, v, d_flat + c0, cq * d, d_q);
        HIP_TRY(hipGetLastError());
        rc = dev.search_device(d_q, cq, d, k1, ef, wide.rows.ids, wide.rows.dists, wide.rows.layer, wide.rows.rank, wide.rows.counts, nullptr, stream, nullptr, 0,
                               nullptr, err);
        if (rc != OK) return rc;
        hipLaunchKernelGGL(graph_compact_kernel, dim3((uint32_t)cq), dim3(64), 0, stream, v, d_flat + c0, wide.rows,
                           host ? stage.rows : rows_at(io.out, c0, k), (uint32_t)k);
        HIP_TRY(hipGetLastError());
        if (host) HIP_TRY(stage.copy_out(rows_at(io.out, c0, k), cq, k, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// Exact graph: the exact k-NN's own chunk loop over tiles built from the rows themselves, the slab kernel's SELF variant
int exact_graph(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, bool host, void* stream_v, std::string& err) {
    const uint64_t np = a.np, k = a.k, n_allowed = a.n_allowed;
    const uint64_t* allowed = a.allowed;
    if (np == 0) return OK;
    const DeviceIndexView& v = dev.view();
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    std::string serr;
    std::shared_ptr<void> ext = dev.extension([&]() { return make_state(dev, origin_id, serr); });
    if (!ext) { err = serr.empty() ? "exact graph: no device state" : serr; return ERR_DEVICE; }
    const ExactState* st = static_cast<const ExactState*>(ext.get());
    const GraphCall io{host, a.point_ids, np, k, {a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts}};
    DevMem m_flat, m_allowed;
    AnswerStage stage;
    int rc = graph_resolve(v, st, io, m_flat, stream, err);  // (waits for the stream)
    if (rc != OK) return rc;
    const uint32_t* d_flat = static_cast<const uint32_t*>(m_flat.p);
    const bool filtered = allowed != nullptr;
    if (!host)
        return exact_device(dev, origin_id, nullptr, np, v.d, k, allowed, n_allowed, filtered, nullptr, io.out.ids, io.out.dists, io.out.layer, io.out.rank,
                            io.out.counts, stream, err, d_flat);
    // (a filter that is empty still is a filter: a non-null pointer that is never dereferenced)
    const uint64_t* d_allowed = filtered ? reinterpret_cast<const uint64_t*>(m_flat.p) : nullptr;
    if (filtered && n_allowed != 0) {
        HIP_TRY(m_allowed.alloc(n_allowed * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(m_allowed.p, allowed, n_allowed * sizeof(uint64_t), hipMemcpyHostToDevice));
        d_allowed = static_cast<const uint64_t*>(m_allowed.p);
    }
    // chunks of points: the staged answers stay within 64 MB whatever np is
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(np, (64ull << 20) / (k * 17 + 4)));
    HIP_TRY(stage.alloc(chunk, k));
    for (uint64_t c0 = 0; c0 < np; c0 += chunk) {
        const uint64_t cq = std::min(chunk, np - c0);
        rc = exact_device(dev, origin_id, nullptr, cq, v.d, k, d_allowed, n_allowed, filtered, nullptr, stage.rows.ids, stage.rows.dists, stage.rows.layer,
                          stage.rows.rank, stage.rows.counts, stream, err, d_flat + c0);
        if (rc != OK) return rc;
        HIP_TRY(stage.copy_out(rows_at(io.out, c0, k), cq, k, stream));
    }
    return OK;
}

// The DataId ranks of the replica's state, for symmetric_graph.hip (graph_internal.hpp): made on first use, like every call here does
int graph_order(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, GraphOrder& out, std::string& err) {
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    std::string serr;
    std::shared_ptr<void> ext = dev.extension([&]() { return make_state(dev, origin_id, serr); });
    if (!ext) { err = serr.empty() ? "symmetric graph: no device state" : serr; return ERR_DEVICE; }
    const ExactState* st = static_cast<const ExactState*>(ext.get());
    out.keep = ext;
    out.d_rank = static_cast<const uint32_t*>(st->d_rank);
    out.d_order = static_cast<const uint32_t*>(st->d_order);
    return OK;
}

// The exact k-NN of new vectors without a filter, for cluster_predict.hip (graph_internal.hpp): exact_device as
// hnswgpu_exact_search_batch_device calls it
int exact_queries_device(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                         uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, void* stream,
                         std::string& err) {
    return exact_device(dev, origin_id, d_queries, nq, d, k, nullptr, 0, false, nullptr, d_out_ids, d_out_dists, d_out_layer, d_out_rank, d_out_counts,
                        static_cast<hipStream_t>(stream), err);
}

}  // namespace hnswgpu
#pragma clang diagnostic pop

using namespace hnswgpu;

extern "C" {

int hnswgpu_exact_search_batch_device(const hnswgpu_index* cidx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                      const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids, float* d_out_dists,
                                      uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, void* stream) {
    try {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return capi_fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = capi_check_exact_call(idx, d_queries, nq, d, k, d_allowed_ids, n_allowed, d_out_ids, d_out_dists, d_out_counts);
    if (rc != HNSWGPU_OK) return rc;
    DeviceIndex* dev = nullptr;
    rc = capi_resident_replica(idx, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return capi_finish(exact_device(*dev, idx->flat->origin_id, d_queries, nq, d, k, d_allowed_ids, n_allowed, d_allowed_ids != nullptr, nullptr, d_out_ids,
                                    d_out_dists, d_out_layer, d_out_rank, d_out_counts, static_cast<hipStream_t>(stream), err),
                       err);
    HNSWGPU_CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_exact_search_batch(const hnswgpu_index* cidx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                               const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dists,
                               uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts) {
    try {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return capi_fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = capi_check_exact_call(idx, queries, nq, d, k, allowed_ids, n_allowed, out_ids, out_dists, out_counts);
    if (rc != HNSWGPU_OK) return rc;
    rc = capi_check_sorted_filter(allowed_ids, n_allowed);
    if (rc != HNSWGPU_OK) return rc;
    if (capi_index_empty(idx)) {  // no point: every answer is empty
        capi_zero_knn_answers(nq, k, out_ids, out_dists, out_layer, out_rank, out_counts);
        return HNSWGPU_OK;
    }
    DeviceIndex* dev = nullptr;
    rc = capi_primary_f32_replica(idx, sl, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return capi_finish(exact_host(*dev, idx->flat->origin_id, queries, nq, d, k, allowed_ids, n_allowed,
                                  GraphRows{out_ids, out_dists, out_layer, out_rank, out_counts}, err),
                       err);
    HNSWGPU_CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

}  // extern "C"
