// exact_knn.hip -- exhaustive exact k-NN over every point of an uploaded index, filter included (gfx950 only):
// hnswgpu_exact_search_batch / hnswgpu_exact_search_batch_device of include/hnsw_mi355x.h, and the device side of
// hnswgpu_exact_search_batch_filter_set / _device (a set of filters, each query naming its own; the entries are in capi.cpp).
// DESIGN.md "Exact k-NN".  exact_device, the call itself, also serves knn_graph.hip and cluster_predict.hip, and the replica's state
// (the DataId ranks, the scratch pool) is made here for every unit that uses it (exact_internal.hpp).
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <numeric>
#include <vector>

#include "capi_index.hpp"
#include "exact_internal.hpp"
#include "exact_tile.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

constexpr uint64_t SCRATCH_BUDGET = 320ull << 20;  // bytes of scratch per call at most, whatever nq and n are

struct ExactKnnArgs : SlabArgs {
    const uint32_t* order;  // [n] the inverse of rank
    uint64_t* lists;        // [tiles][n_slabs][TQ][cap] ascending keys
    uint32_t* lens;         // [tiles][n_slabs][TQ]
    uint32_t cap;           // min(k, n)
    uint32_t k;
    GraphRows out;          // the chunk's rows of the caller's arrays
    const uint32_t* qlist;  // tile slot -> row of the caller's arrays, or nullptr: the slot's own number
    const uint32_t* tword;  // [tiles * TQ] filter set: first word of the slot's bitmap in `allow` (prep kernel)
    const uint32_t* self_rank;  // [tiles * TQ] k-NN graph: the slot's query is the stored point of this DataId rank (prep kernel), never its own answer
};

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {
    return ((uint64_t)readlane_u((uint32_t)(v >> 32), lane) << 32) | readlane_u((uint32_t)v, lane);
}
__device__ __forceinline__ uint64_t first_lane_u64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// the lists are private to one wavefront; what one lane stored another lane loads later
__device__ __forceinline__ void list_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

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
    const SlabTile T = slab_tile<METRIC>(ix, a, slab, tile);
    const uint32_t nvalid = T.nvalid, nchunk = a.nchunk, cap = a.cap;
    const size_t slot = ((size_t)tile * a.n_slabs + slab) * (size_t)TQ;
    uint64_t* const lists = a.lists + slot * cap;
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

    for (uint32_t r0 = T.lo; r0 < T.hi; r0 += 64u) {
        uint32_t r;
        bool in;
        bool ok = slab_row(T, r0, lane, SET ? nullptr : a.allow, r, in);
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
        }
        if (__ballot(ok) == 0ull) continue;  // (wave-uniform) nothing eligible for any query among these 64 rows
#include "exact_row_chain.inc"
        const uint32_t rk = a.rank[r];
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            if ((uint32_t)t < nvalid) {
                const float v = tile_dist<METRIC>(a, tile * (uint32_t)TQ + (uint32_t)t, acc[t], s2);
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
            if (jj <= j) write_answer(ix, a.order, mine, (uint32_t)mine, (size_t)q * k + jj, a.out.ids, a.out.dists, a.out.layer, a.out.rank);
        }
    }
    for (uint32_t j = cnt + lane; j < k; j += 64u) {  // slots behind the answers: zero, as the search entries leave them
        const size_t o = (size_t)q * k + j;
        a.out.ids[o] = 0ull;
        a.out.dists[o] = 0.f;
        if (a.out.layer) a.out.layer[o] = 0;
        if (a.out.rank) a.out.rank[o] = 0;
    }
    if (lane == 0u) a.out.counts[q] = cnt;
}

// the first `live` elements of src, then zeros, as slot qs of the tiles qt; returns the squared norm in the crate's arithmetic
// (DistCosine): f32 squares widened to f64, summed left to right (finish_staged_query)
__device__ __forceinline__ double prep_slot(const float* __restrict__ src, uint32_t live, uint32_t nchunk, uint32_t qs, float* __restrict__ qt) {
    const uint32_t tile = qs / (uint32_t)TQ, t = qs % (uint32_t)TQ;
    double s1 = 0.;
    for (uint32_t c = 0; c < nchunk; ++c) {
        float e[4];
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t i = 4u * c + j;
            e[j] = i < live ? src[i] : 0.f;
            s1 = s1 + (double)(e[j] * e[j]);
        }
        reinterpret_cast<float4*>(qt)[((size_t)tile * nchunk + c) * (size_t)TQ + t] = make_float4(e[0], e[1], e[2], e[3]);
    }
    return s1;
}

// one thread per query slot of the chunk's tiles: the row into its tile (slots behind the last query: zeros).  Slot qs holds row
// qlist[qs] of src (qlist == nullptr: row qs).  Filter set (tword != nullptr): the first word of the bitmap that row's filter has
// in the group's bitmaps, slot_of[row] * words -- the caller bounds the bitmaps of a group to 2^32 words.
__global__ void exact_knn_prep_kernel(const float* __restrict__ src, uint32_t nq, uint32_t d, uint32_t nchunk, uint32_t n_slots,
                                      float* __restrict__ qt, double* __restrict__ qnorm, const uint32_t* __restrict__ qlist,
                                      const uint32_t* __restrict__ slot_of, uint32_t words, uint32_t* __restrict__ tword) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= n_slots) return;
    const uint32_t q = qs < nq && qlist != nullptr ? qlist[qs] : qs;
    if (tword != nullptr) tword[qs] = qs < nq ? slot_of[q] * words : 0u;
    qnorm[qs] = prep_slot(src + (size_t)q * d, qs < nq ? d : 0u, nchunk, qs, qt);
}

// k-NN graph: the same tiles from the index's own rows -- slot qs holds the stored point flat[qs], its first d elements (what lies
// behind them in the padded row, a DistCosine norm included, never reaches the tile), the squared norm summed as above, so the
// bits are those of the point's vector brought as a query -- and the slot's own DataId rank (slots behind the last: no rank)
__global__ void exact_knn_prep_rows_kernel(DeviceIndexView ix, const uint32_t* __restrict__ flat, const uint32_t* __restrict__ rank, uint32_t nq,
                                           uint32_t nchunk, uint32_t n_slots, float* __restrict__ qt, double* __restrict__ qnorm,
                                           uint32_t* __restrict__ self_rank) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= n_slots) return;
    const uint32_t f = qs < nq ? flat[qs] : 0u;
    qnorm[qs] = prep_slot(ix.vec + (size_t)f * ix.row_stride, qs < nq ? ix.d : 0u, nchunk, qs, qt);
    self_rank[qs] = qs < nq ? rank[f] : 0xFFFFFFFFu;
}

hipError_t launch_slab(int metric, bool set, bool self, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const ExactKnnArgs& a) {
    return launch_for_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (self) hipLaunchKernelGGL((exact_knn_slab_kernel<M, false, true>), grid, dim3(64), 0, stream, ix, a);  // (the graph calls take one filter or none)
        else if (set) hipLaunchKernelGGL((exact_knn_slab_kernel<M, true, false>), grid, dim3(64), 0, stream, ix, a);
        else hipLaunchKernelGGL((exact_knn_slab_kernel<M, false, false>), grid, dim3(64), 0, stream, ix, a);
    });
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

constexpr uint64_t MAX_FILTER_SET_WAVES = 1ull << 31;  // allow_bitmap_set_kernel: four wavefronts per workgroup, 2^29 workgroups
// the knob that bounds the bitmaps one launch holds: HNSWGPU_FILTER_SET_MB in bytes
uint64_t filter_set_budget() {
    const int64_t knob = knobs().filter_set_bytes;
    return knob >= 0 ? (uint64_t)knob : 256ull << 20;
}

}  // namespace

std::shared_ptr<ExactState> replica_state(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const char* what, std::string& err) {
    std::string serr;
    std::shared_ptr<void> ext = dev.extension([&]() { return make_state(dev, origin_id, serr); });
    if (!ext) err = serr.empty() ? std::string(what) + ": no device state" : serr;
    return std::static_pointer_cast<ExactState>(ext);
}

hipError_t exact_prep_queries(hipStream_t stream, const float* d_src, uint64_t cq, uint64_t d, const SlabPlan& plan, uint32_t n_slots, float* d_qt,
                              double* d_qnorm, const uint32_t* qlist, const uint32_t* slot_of, uint32_t* tword) {
    hipLaunchKernelGGL(exact_knn_prep_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, d_src, (uint32_t)cq, (uint32_t)d, (uint32_t)plan.nchunk,
                       n_slots, d_qt, d_qnorm, qlist, slot_of, (uint32_t)plan.words, tword);
    return hipGetLastError();
}

hipError_t exact_prep_rows(hipStream_t stream, const DeviceIndexView& ix, const uint32_t* d_flat, const uint32_t* d_rank, uint64_t cq, const SlabPlan& plan,
                           uint32_t n_slots, float* d_qt, double* d_qnorm, uint32_t* d_self_rank) {
    hipLaunchKernelGGL(exact_knn_prep_rows_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, stream, ix, d_flat, d_rank, (uint32_t)cq, (uint32_t)plan.nchunk,
                       n_slots, d_qt, d_qnorm, d_self_rank);
    return hipGetLastError();
}

// the device path: every pointer is device memory; waits for `stream` before it returns.
// No set: no filter, or one for the batch (c.d_allowed).  Else query q is answered under filter set->filter_of[q]: the
// bitmaps are built group by group -- as many consecutive filters as the bound and this unit's scratch budget hold -- and per group
// its queries are listed (launch_filter_group), tiled densely and searched; one group (the usual case): all queries in batch order.
// c.d_self != nullptr (k-NN graph; no set): query q is the stored point of flat id d_self[q], d_queries is not read, and the point
// itself is no candidate of its own row.
int exact_device(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactCall& c, hipStream_t stream, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t nq = c.nq, d = c.d, k = c.k;
    const FilterSet* const set = c.set;
    const uint32_t* const d_self = c.d_self;
    const bool filtered = c.d_allowed != nullptr;
    if (nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "exact search", err);
    if (!st) return ERR_DEVICE;

    SlabPlan plan(v.n, d, nq);
    const uint64_t n = plan.n, nchunk = plan.nchunk, words = plan.words, slot_bytes = words * 4;
    const uint64_t cap = std::min<uint64_t>(k, n);
    // in front of the tiles: the bitmap -- or, for a filter set, the bitmaps of a group (at most half of the budget), two words of
    // counters and, when there is more than one group, the list of a group's queries and every query's slot
    uint64_t per_group = 1, groups = 1, ctrl_bytes = 0, qlist_bytes = 0;
    if (set) {
        const uint64_t bitmap_budget = filter_set_budget();
        if (bitmap_budget < slot_bytes) {
            err = "HNSWGPU_FILTER_SET_MB is smaller than one filter's bitmap (" + std::to_string(slot_bytes) + " bytes for this index)";
            return ERR_ARG;
        }
        per_group = std::min<uint64_t>({bitmap_budget / slot_bytes, (SCRATCH_BUDGET / 2) / slot_bytes, set->n_filters,
                                        MAX_FILTER_SET_WAVES / ((n + 63) / 64) - 1});
        if (per_group == 0) { err = "index too large for the exact search's scratch budget"; return ERR_ARG; }
        groups = (set->n_filters + per_group - 1) / per_group;
        ctrl_bytes = 256;
        if (groups > 1) qlist_bytes = round_up(nq * 4, 256);
    }
    const uint64_t allow_bytes = round_up(per_group * slot_bytes, 256) + ctrl_bytes + 2 * qlist_bytes;
    const uint64_t fixed_bytes = allow_bytes + round_up(TQ * (nchunk * 16 + 8), 256) + 4096;  // the bitmap(s) and one tile's queries
    if (fixed_bytes >= SCRATCH_BUDGET) { err = "index, batch or dimension too large for the exact search's scratch budget"; return ERR_ARG; }
    // slabs: never more lists than the budget holds for one tile
    if (!plan.cut((SCRATCH_BUDGET - fixed_bytes) / ((uint64_t)TQ * (cap * 8 + 4)))) { err = "knbn too large for the exact search's scratch budget"; return ERR_ARG; }
    const uint64_t slabs = plan.slabs;
    // queries per chunk: whole tiles, what the budget holds, a grid the launch accepts
    const uint64_t tword_bytes = set ? round_up(TQ * 4, 256) : 0;
    const uint64_t self_bytes = d_self ? round_up(TQ * 4, 256) : 0;
    const uint64_t per_tile = plan.qt_bytes() + plan.qnorm_bytes() + round_up(slabs * TQ * cap * 8, 256) + round_up(slabs * TQ * 4, 256) + tword_bytes + self_bytes;
    const uint64_t chunk_tiles = std::min<uint64_t>({plan.tiles_total, (SCRATCH_BUDGET - allow_bytes) / per_tile, 65535});
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
    plan.tiles(lay, chunk_tiles, d_qt, d_qnorm);
    lay.bytes(d_lists, chunk_tiles * round_up(slabs * TQ * cap * 8, 256));
    lay.bytes(d_lens, chunk_tiles * round_up(slabs * TQ * 4, 256));
    if (set) lay.bytes(d_tword, chunk_tiles * tword_bytes);
    if (d_self) lay.bytes(d_self_rank, chunk_tiles * self_bytes);
    // (what the budget above counted: before anything is taken)
    if (lay.size() != allow_bytes + chunk_tiles * per_tile) { err = "exact search: scratch layout"; return ERR_FORMAT; }
    ScratchLease lease(st.get());
    const int rc_lease = alloc_layout("exact search", lease, lay, err);
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
            ExactKnnArgs a{slab_args(*st, dev, plan, d_qt, d_qnorm, filtered || set ? d_allow : nullptr), st->order(), d_lists, d_lens, (uint32_t)cap,
                           (uint32_t)k, rows_at(c.out, row0, k), qlist ? qlist + q0 : nullptr, d_tword, d_self_rank};
            a.nq = (uint32_t)cq;
            const uint32_t n_slots = (uint32_t)(tiles * TQ);
            if (d_self) {
                HIP_TRY(exact_prep_rows(stream, v, d_self + row0, a.rank, cq, plan, n_slots, d_qt, d_qnorm, d_self_rank));
            } else {
                HIP_TRY(exact_prep_queries(stream, c.d_queries + row0 * d, cq, d, plan, n_slots, d_qt, d_qnorm, a.qlist, slot_of ? slot_of + row0 : nullptr, d_tword));
            }
            HIP_TRY(launch_slab(dev.dist(), set != nullptr, d_self != nullptr, dim3((uint32_t)slabs, (uint32_t)tiles), stream, v, a));
            hipLaunchKernelGGL(exact_knn_merge_kernel, dim3((uint32_t)cq), dim3(64), 0, stream, v, a);
            HIP_TRY(hipGetLastError());
        }
        return OK;
    };

    if (!set) {
        if (filtered) HIP_TRY(launch_allow_bitmap(stream, v.origin_id, v.n, c.d_allowed, c.n_allowed, d_allow));
        const int rc = run(nullptr, nq, nullptr);
        if (rc != OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        return OK;
    }
    // The slab kernel indexes the bitmaps with filter_of's values: the entries that name no filter are counted, and the count is
    // read back (while the first group's bitmaps are being built) before anything is searched or written.
    const FilterSet& fs = *set;
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

namespace {

// Host buffers of an exact k-NN call (c.d_queries and c.out are host memory here): queries and answers are staged in chunks of at
// most 64 MB, each chunk one call of the device path on the null stream.  c.set == nullptr: no filter, or one for the batch
// (`allowed`, host memory).  Else the set's ids and offsets are on the device, and every chunk brings its own rows of filter_of
// (host memory) along.
int exact_host_chunks(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactCall& c, const uint64_t* allowed, const uint32_t* filter_of,
                      std::string& err) {
    const uint64_t nq = c.nq, d = c.d, k = c.k;
    if (nq == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    FilterUpload filter;  // the one filter of the batch (`allowed`, host memory), when there is one, goes to the device once
    int rc = filter.put(allowed, c.n_allowed, err);
    if (rc != OK) return rc;
    const uint64_t per_q = d * 4 + k * 17 + 4 + (c.set ? 4 : 0);
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(nq, (64ull << 20) / per_q));
    DevMem m_q, m_of;
    AnswerStage stage;
    HIP_TRY(m_q.alloc(chunk * d * 4));
    if (c.set) HIP_TRY(m_of.alloc(chunk * sizeof(uint32_t)));
    if ((rc = stage.alloc("exact search", chunk, k, err)) != OK) return rc;
    const FilterSet chunk_set{c.set ? c.set->ids : nullptr, c.set ? c.set->offsets : nullptr, c.set ? c.set->n_filters : 0, static_cast<const uint32_t*>(m_of.p)};
    ExactCall part = c;
    part.d_queries = static_cast<const float*>(m_q.p);
    part.d_allowed = filter.d_allowed;
    part.set = c.set ? &chunk_set : nullptr;
    part.out = stage.rows;
    for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
        part.nq = std::min(chunk, nq - q0);
        HIP_TRY(hipMemcpy(m_q.p, c.d_queries + q0 * d, part.nq * d * 4, hipMemcpyHostToDevice));
        if (c.set) HIP_TRY(hipMemcpy(m_of.p, filter_of + q0, part.nq * sizeof(uint32_t), hipMemcpyHostToDevice));
        if ((rc = exact_device(dev, origin_id, part, nullptr, err)) != OK) return rc;
        if ((rc = copy_rows_out(rows_at(c.out, q0, k), stage.rows, part.nq * k, part.nq, nullptr, err)) != OK) return rc;
    }
    return OK;
}

}  // namespace

// The device side of hnswgpu_exact_search_batch_filter_set(_device); capi.cpp holds the entries and every argument check
// (capi_index.hpp).
int exact_filter_set(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactSetArgs& a, bool host, void* stream, std::string& err) {
    ExactCall c;
    c.d_queries = a.queries;
    c.nq = a.nq, c.d = a.d, c.k = a.k;
    c.set = &a.set;
    c.out = GraphRows{a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts};
    if (!host) return exact_device(dev, origin_id, c, static_cast<hipStream_t>(stream), err);
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
    c.set = &d_set;
    return exact_host_chunks(dev, origin_id, c, nullptr, set.filter_of, err);
}

}  // namespace hnswgpu

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
    const ExactCall c{d_queries, nullptr, nq, d, k, d_allowed_ids, n_allowed, nullptr, {d_out_ids, d_out_dists, d_out_layer, d_out_rank, d_out_counts}};
    return capi_finish(exact_device(*dev, idx->flat->origin_id, c, static_cast<hipStream_t>(stream), err), err);
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
    const ExactCall c{queries, nullptr, nq, d, k, nullptr, n_allowed, nullptr, {out_ids, out_dists, out_layer, out_rank, out_counts}};
    return capi_finish(exact_host_chunks(*dev, idx->flat->origin_id, c, allowed_ids, nullptr, err), err);
    HNSWGPU_CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

}  // extern "C"
