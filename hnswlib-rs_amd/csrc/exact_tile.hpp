// exact_tile.hpp -- the device pieces that the slab kernels of exact_knn.hip and exact_range.hip share: a tile of TQ queries against a
// slab of rows, ONE ROW PER LANE.  The 64-bit key {distance bits, DataId rank} and its way back into an answer, the four-element
// step of a (query, row) chain, the frame of a (tile, slab) wavefront, the last step of a distance, and the dispatch of a launch over
// the metric.  The chain itself is text, exact_row_chain.inc: as a function that takes acc[TQ] it costs registers.  Private: not
// installed, not part of the ABI; a kernel unit includes it once.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "exact_internal.hpp"  // TQ
#include "graph_internal.hpp"  // dist_order_bits
#include "search_kernels.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "search_kernels.inc"  // the per-element terms and the last step of Distance::eval, shared with the search
#pragma clang diagnostic pop

namespace hnswgpu {
namespace {

constexpr uint64_t KEY_NONE = ~0ull;  // behind every key: the threshold of a list that is not full yet

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const v4f* qtile_ptr_t;  // wave-uniform addresses: scalar loads
typedef __attribute__((address_space(4))) const uint32_t* uword_ptr_t;

// (dist_order_bits, the order of a key's upper half, is in graph_internal.hpp: symmetric_graph.hip builds the same keys)
// A key: order bits above, the DataId rank below.  Every NaN has the same order bits and comes back as the canonical quiet NaN.
__device__ __forceinline__ uint64_t make_key(float v, uint32_t rank) { return ((uint64_t)dist_order_bits(v) << 32) | rank; }
__device__ __forceinline__ float dist_of_key(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    if (u == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
// Key -> answer: slot o of the out arrays gets the point whose DataId rank is the key's lower half (rk: that half, in range) -- its
// DataId, the key's distance (a -0 comes back as +0) and, where asked for, its p_id
__device__ __forceinline__ void write_answer(const DeviceIndexView& ix, const uint32_t* __restrict__ order, uint64_t key, uint32_t rk, size_t o,
                                             uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank) {
    const uint32_t flat = order[rk];
    uint32_t l = 0;
    while (l + 1 < NB_LAYER_MAX && flat >= ix.layer_offset[l + 1]) ++l;
    out_ids[o] = ix.origin_id[flat];
    out_dists[o] = dist_of_key(key);
    if (out_layer) out_layer[o] = (uint8_t)l;
    if (out_rank) out_rank[o] = (int32_t)(flat - ix.layer_offset[l]);
}

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

// What every slab kernel is told (the head of its own arguments)
struct SlabArgs {
    const float* qt;        // [tiles][nchunk][TQ] float4: element chunk c of the tile's TQ queries side by side, zero padded
    const double* qnorm;    // [tiles * TQ] DistCosine: the queries' squared norms
    const uint32_t* rank;   // [n] position of flat id f in ascending (DataId, flat id) order
    const uint32_t* allow;  // one bit per flat id, or nullptr: no filter
    const double* nrm2;     // DistCosine: side array of the points' squared norms, or nullptr: in the rows
    uint32_t nq;            // queries of this chunk
    uint32_t nchunk;        // float4 chunks of a row that hold data: ceil(d / 4)
    uint32_t slab_rows;     // a multiple of 64
    uint32_t n_slabs;       // <= MAX_SLABS
};
// (everything but nq, which is a chunk's; d_allow: the one bitmap, the bitmaps of a filter set, or nullptr)
inline SlabArgs slab_args(const ExactState& st, const DeviceIndex& dev, const SlabPlan& plan, const float* d_qt, const double* d_qnorm, const uint32_t* d_allow) {
    return SlabArgs{d_qt, d_qnorm, st.rank(), d_allow, dev.side_norms(), 0u, (uint32_t)plan.nchunk, (uint32_t)plan.slab_rows, (uint32_t)plan.slabs};
}
// The frame of one (tile, slab) wavefront
struct SlabTile {
    uint32_t lo, hi;    // the slab's rows
    uint32_t nvalid;    // queries of the tile (the last tile may be part filled)
    qtile_ptr_t qc;     // the tile's queries
    bool norm_in_tail;  // DistCosine rows that carry their norm in their last 8 bytes: when the last data chunk is the row's last
                        // chunk, its .z/.w are those bytes, not the zero padding the sum expects (norm_fits_row: they lie behind
                        // element d - 1)
};
template <int METRIC>
__device__ __forceinline__ SlabTile slab_tile(const DeviceIndexView& ix, const SlabArgs& a, uint32_t slab, uint32_t tile) {
    SlabTile T;
    T.lo = slab * a.slab_rows;
    T.hi = ix.n - T.lo < a.slab_rows ? ix.n : T.lo + a.slab_rows;
    T.nvalid = a.nq - tile * (uint32_t)TQ < (uint32_t)TQ ? a.nq - tile * (uint32_t)TQ : (uint32_t)TQ;
    T.qc = (qtile_ptr_t)(reinterpret_cast<const v4f*>(a.qt) + (size_t)tile * a.nchunk * (size_t)TQ);
    T.norm_in_tail = METRIC == DIST_COSINE && a.nrm2 == nullptr && a.nchunk * 4u == ix.row_stride;
    return T;
}
// This lane's row of the 64 behind r0 (lanes past the slab re-read its last row); true: it lies in the slab and, under the one
// bitmap `allow` (nullptr: none), is eligible
__device__ __forceinline__ bool slab_row(const SlabTile& T, uint32_t r0, uint32_t lane, const uint32_t* allow, uint32_t& r, bool& in) {
    in = r0 + lane < T.hi;
    r = in ? r0 + lane : T.hi - 1u;
    bool ok = in;
    if (allow != nullptr) ok = in && ((allow[r >> 5] >> (r & 31u)) & 1u) != 0u;
    return ok;
}
// The last step: a chain's sum into the distance of (query slot qs, a row whose squared norm is s2 -- DistCosine only)
template <int METRIC, typename ACC>
__device__ __forceinline__ float tile_dist(const SlabArgs& a, uint32_t qs, ACC acc, double s2) {
    if constexpr (METRIC == DIST_COSINE) {
        const double s1 = ((nrm_ptr_t)a.qnorm)[qs];
        float v = 0.f;
        if (s1 > 0. && s2 > 0.) {
            const double du = 1. - acc / __builtin_sqrt(s1 * s2);
            v = (float)fmax(du, 0.);
        }
        return v;
    } else {
        return dist_finish<METRIC>(acc);
    }
}

// One launch per metric: f(std::integral_constant<int, METRIC>) launches the kernel's instantiation for the replica's distance
template <typename F>
hipError_t launch_for_metric(int metric, F&& f) {
    switch (metric) {
        case DIST_L2: f(std::integral_constant<int, DIST_L2>{}); break;
        case DIST_COSINE: f(std::integral_constant<int, DIST_COSINE>{}); break;
        case DIST_DOT: f(std::integral_constant<int, DIST_DOT>{}); break;
        case DIST_L1: f(std::integral_constant<int, DIST_L1>{}); break;
        case DIST_HELLINGER: f(std::integral_constant<int, DIST_HELLINGER>{}); break;
        case DIST_JEFFREYS: f(std::integral_constant<int, DIST_JEFFREYS>{}); break;
        case DIST_JENSENSHANNON: f(std::integral_constant<int, DIST_JENSENSHANNON>{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace
}  // namespace hnswgpu
