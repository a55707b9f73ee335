// dbscan_screen.hip -- exact DBSCAN behind a two-sided matrix-core screen (gfx950 only): the device side of hnswxd_exact(_device) and
// hnswxd_bounds_matrix of include/hnsw_mi355x_dbscan_screen.h (the entries and the argument checks are in capi.cpp).  The answers are
// those of dbscan.hip byte for byte; DESIGN.md section 15.15 holds the pipeline, the upper bound and the argument, section 15.13 the
// lower bound.  DistL2, DistDot and DistCosine.  DBSCAN needs "v <= eps or not" of nearly every pair and the bits of v of very few:
// the screen proves hits (ub <= eps) as well as misses (lb > eps), and only the band between the two sees the exact chain.
//
//   dbscan_screen_prep_kernel  the stored rows of a chunk of positions as queries: zero padded, their norms in both arithmetics, and
//                              per slot its position
//   dbscan_screen_kernel       <METRIC, PASS, NT> one workgroup of W <= 4 wavefronts per (tile of 32 W queries, slab of rows): the data
//                              movement of range_screen_kernel.  Epilogue per accumulator register -- one row per lane, two queries
//                              across the lane halves --: the pair is SURE (proved and ub <= eps), a MISS (lb > eps) or UNDECIDED.
//                              COUNT: a ballot of the sure pairs, a popcount into the query's counter in LDS, at the end one atomic
//                              add per (query, slab); the undecided pairs into the candidate buffer.  LINK: the rows' core bits from
//                              the bitmap word; a core query unites with its sure core rows (the skip rule of dbscan.hip); the
//                              undecided pairs with a core row, and every pair that is no miss of a query that is NOT core with a
//                              core row -- its key needs the distance's bits --, into the buffer.  BOUNDS: lb and ub stored.
//   dbscan_rerank_kernel       <METRIC, PASS> one candidate per lane through the exact chain (chain4, tile_dist: the bits of
//                              dbscan.hip), then v <= eps: a count, a union, or a key into best[]
//   dbs_init_kernel, dbs_core_kernel, dbscan_finish   (dbscan_parts.hpp) the state, the core flags between the passes, the finish
//
// A call whose candidates outgrow a chunk's buffer is answered by exact_dbscan, whole.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_index.hpp"
// (the CSR validation kernels that come with the union-find have no caller in this unit)
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
constexpr uint64_t DS_MATRIX_PAIRS = 1ull << 24; // hnswxd_bounds_matrix: nq * n at most
enum { PASS_BOUNDS = 2 };                        // beside PASS_COUNT and PASS_LINK: the store epilogue of hnswxd_bounds_matrix

// Accumulator tiles of a wavefront: the rule of exact_range_screen.hip -- 4 where the LDS holds the larger row blocks without costing
// a wavefront, else 2
#ifndef HNSW_DBSCAN_SCREEN_NT
#define HNSW_DBSCAN_SCREEN_NT 4
#endif

uint64_t dbscan_screen_lds_bytes(uint64_t waves, uint64_t dpad, uint64_t nt) { return screen_lds_bytes(waves, dpad) + 2ull * (nt - 2) * 32 * RPITCH * 4; }

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

template <int METRIC, int PASS, int NT>
__global__ __launch_bounds__(64 * MAX_WAVES) void dbscan_screen_kernel(DeviceIndexView ix, DbscanScreenArgs a) {
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
    uint32_t* const qposl = reinterpret_cast<uint32_t*>(qnl + qt);  // [qt] their positions
    uint32_t* const auxl = qposl + qt;                    // [qt] COUNT: the sure hits so far; LINK: a root the query had
    uint32_t* const corel = auxl + qt;                    // [qt] LINK: the query is core

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
            qnl[q] = a.qn[tile * qt + q];
            if constexpr (PASS != PASS_BOUNDS) {
                const uint32_t pos = q < nvalid ? a.qpos[tile * qt + q] : 0u;
                qposl[q] = pos;
                auxl[q] = PASS == PASS_LINK ? pos : 0u;
                corel[q] = PASS == PASS_LINK && q < nvalid ? a.core[pos] : 0u;
            }
        }
    }
    float cut = 0.f;
    if constexpr (PASS != PASS_BOUNDS) cut = *a.cut;
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t steps = ((hi - lo + RBN - 1u) / RBN) * nkc;  // (block of rows, chunk of elements), chunk fastest
    const uint32_t row_stride = ix.row_stride;

    // this thread's part of a staged block: float4 number i = tid + j * nthr of RBN x 8.  Rows behind the slab re-read its last row;
    // they are misses (epilogue).
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
    // the lanes of `take` (wave-uniform ballot `m`, not empty) into the candidate buffer as (query slot ql of the tile, flat row r):
    // lane 0 reserves the slots.  False: the buffer was full before this ballot -- the call is the existing path's.
    auto append = [&](bool take, unsigned long long m, uint32_t ql, uint32_t r) -> bool {
        unsigned long long base = 0ull;
        if (lane == 0u) base = atomicAdd(a.ctr, (unsigned long long)popc64(m));
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        const unsigned long long p = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (take && p < (unsigned long long)a.cand_cap) {  // (past the buffer: dropped; the counter tells)
            a.cq[p] = tile * qt + ql;
            a.crow[p] = r;
        }
        return base < (unsigned long long)a.cand_cap;
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
                // wavefront's 32: a ballot's lower word is one query's 32 rows, its upper word another's.  Every lane is active here.
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) {
                    const uint32_t r0 = lo + blk * RBN + 32u * (uint32_t)tb;  // (a multiple of 32: lo and RBN are multiples of 64)
                    const uint32_t r = r0 + l32;
                    const bool in = r < hi;
                    const uint32_t rc = in ? r : hi - 1u;
                    const float nx = a.xn[rc];
                    [[maybe_unused]] uint32_t rk = 0u;
                    [[maybe_unused]] bool rowcore = false;
                    if constexpr (PASS == PASS_LINK) {
                        // the tile's 32 core bits: half of the aligned word of 64 flat ids (rows past n: no bit)
                        uint32_t cw = 0u;
                        if (r0 < hi) cw = (uint32_t)(((umask_ptr_t)a.cmask)[r0 >> 6] >> (r0 & 32u));
                        if (cw == 0u) continue;  // (wave-uniform) no core row among these 32: nothing to unite with, no anchor
                        rowcore = in && ((cw >> l32) & 1u) != 0u;
                        rk = a.rank[rc];
                    }
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const uint32_t ql = wave * SQ + 8u * ((uint32_t)v >> 2) + ((uint32_t)v & 3u) + 4u * half;
                        bool ok;
                        float blo, bhi;
                        screen_band<METRIC>(acc[tb][v], qnl[ql], nx, a.cu, ok, blo, bhi);
                        const bool live = in && ql < nvalid;
                        if constexpr (PASS == PASS_BOUNDS) {
                            if (live) {
                                const size_t o = (size_t)(tile * qt + ql) * ix.n + r;
                                a.out_lb[o] = METRIC == DIST_L2 ? __builtin_sqrtf(blo) : blo;
                                a.out_ub[o] = !ok ? __builtin_inff() : METRIC == DIST_L2 ? __builtin_sqrtf(bhi) : bhi;
                            }
                        } else {
                            const bool notmiss = live && blo <= cut;      // else a miss: lb > eps (rows past the slab, slots past the chunk)
                            const bool sure = notmiss && ok && bhi <= cut;  // proved and ub <= eps; what is neither is undecided
                            bool cand;
                            if constexpr (PASS == PASS_COUNT) {
                                const unsigned long long m = __ballot(sure);
                                const uint32_t mw = half != 0u ? (uint32_t)(m >> 32) : (uint32_t)m;
                                if (l32 == 0u && mw != 0u) auxl[ql] += __popc(mw);  // (the wavefront owns its queries: no atomic)
                                cand = notmiss && !sure;
                            } else {
                                if (__ballot(notmiss && rowcore) == 0ull) continue;  // (wave-uniform)
                                const bool qcore = corel[ql] != 0u;
                                // the skip rule of dbscan.hip: trees only merge, so a row whose parent is a root the query had is in
                                // the query's tree already
                                bool did = false;
                                if (sure && rowcore && qcore && parent_of(a.parent, rk) != auxl[ql]) {
                                    cc_unite(a.parent, qposl[ql], rk);
                                    did = true;
                                }
                                const unsigned long long md = __ballot(did);
                                if (md != 0ull) {  // a query's root may have changed: one lane of its half looks
                                    const uint32_t mw = half != 0u ? (uint32_t)(md >> 32) : (uint32_t)md;
                                    if (l32 == 0u && mw != 0u) auxl[ql] = cc_find(a.parent, qposl[ql]);
                                    wave_lds_fence();
                                }
                                cand = notmiss && rowcore && (!qcore || !sure);  // not core: the key needs the bits, sure or not
                            }
                            const unsigned long long mc = __ballot(cand);
                            // the buffer was full before this ballot: the call is the existing path's, and this wavefront only keeps
                            // the workgroup's barriers from here on (the counter is past the capacity and stays there)
                            if (mc != 0ull && !append(cand, mc, ql, r)) mine = false;
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
    if constexpr (PASS == PASS_COUNT) {
        // one integer add per (query, slab); the barrier behind the last block has made the counters visible
        if (lane < SQ && wave * SQ + lane < nvalid) {
            const uint32_t cnt = auxl[wave * SQ + lane];
            if (cnt != 0u) atomicAdd(a.count + qposl[wave * SQ + lane], cnt);
        }
    }
}

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

// (kernel: &dbscan_screen_kernel<M, PASS, NT>) one launch -- and, launch == false, once per call in front of the first: more LDS than
// the default limit of a launch is said to the runtime per kernel
template <int PASS>
hipError_t dbscan_screen(bool launch, int metric, uint32_t nt, dim3 grid, uint32_t waves, uint32_t lds, hipStream_t stream, const DeviceIndexView& ix,
                         const DbscanScreenArgs& a) {
    hipError_t said = hipSuccess;
    const hipError_t e = for_screened_metric(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (!launch) said = nt == 4u ? hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_screen_kernel<M, PASS, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                     : hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_screen_kernel<M, PASS, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        else if (nt == 4u) hipLaunchKernelGGL((dbscan_screen_kernel<M, PASS, 4>), grid, dim3(64u * waves), lds, stream, ix, a);
        else hipLaunchKernelGGL((dbscan_screen_kernel<M, PASS, 2>), grid, dim3(64u * waves), lds, stream, ix, a);
    });
    return said != hipSuccess ? said : e;
}

// the shape of a screen launch on this device for rows of d elements; waves == 0: no screen
struct ScreenShape {
    uint64_t dpad = 0, waves = 0, nt = 0, qt = 0, rbn = 0;
    uint32_t lds = 0;
    int pick(int device, uint64_t d) {
        dpad = round_up(d, KC);
        waves = screen_waves(device, dpad);
        if (waves == 0) return 0;
        int limit = 0;
        if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return waves = 0;
        nt = HNSW_DBSCAN_SCREEN_NT == 4 && dbscan_screen_lds_bytes(waves, dpad, 4) <= (uint64_t)limit ? 4 : 2;
        qt = waves * SQ, rbn = 32 * nt;
        lds = (uint32_t)dbscan_screen_lds_bytes(waves, dpad, nt);
        return (int)waves;
    }
    // slabs of rows for `tiles` tiles of queries: enough workgroups to fill the device, whole blocks of rows, every slab from a
    // multiple of 64 flat rows on (rbn is 64 or 128)
    void cut(uint64_t n, uint64_t tiles, uint64_t& slabs, uint64_t& slab_rows) const {
        slabs = std::max<uint64_t>(1, std::min<uint64_t>((SCREEN_WG_TARGET + tiles - 1) / tiles, n / SCREEN_SLAB_ROWS));
        slab_rows = round_up((n + slabs - 1) / slabs, rbn);
        slabs = (n + slab_rows - 1) / slab_rows;
    }
};

enum Route { ROUTE_DONE, ROUTE_UNSCREENED, ROUTE_OUTGROWN };

// Both entries.  The state of dbscan.hip; per pass and per chunk of positions: prep, screen, rerank; the chunks' counters come back once
// per pass.  Between the passes dbs_core_kernel, behind them dbscan_finish.  Waits for `stream` before it returns.  *route: ROUTE_DONE,
// or why the caller has to run the existing path instead (nothing of the caller's has been written then).  *pairs: the candidates of
// both passes, what went through the exact chain.
int dbscan_screened_passes(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& c, bool host, hipStream_t stream, Route* route,
                           uint64_t* pairs, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t n = v.n, d = v.d;
    *route = ROUTE_UNSCREENED;
    ScreenShape sh;
    if (!metric_has_screen(dev.dist()) || n < SCREEN_MIN_ROWS || sh.pick(dev.device(), d) == 0) return OK;
    const uint64_t dpad = sh.dpad, qt = sh.qt;

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
    HIP_TRY(dbscan_screen<PASS_COUNT>(false, dev.dist(), (uint32_t)sh.nt, dim3(), (uint32_t)sh.waves, sh.lds, stream, v, DbscanScreenArgs{}));
    HIP_TRY(dbscan_screen<PASS_LINK>(false, dev.dist(), (uint32_t)sh.nt, dim3(), (uint32_t)sh.waves, sh.lds, stream, v, DbscanScreenArgs{}));
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
            sh.cut(n, tiles, slabs, slab_rows);
            hipLaunchKernelGGL(dbscan_screen_prep_kernel, grid_of(n_slots), dim3(256), 0, stream, v, st->order() + q0, (uint32_t)q0, (uint32_t)cq, (uint32_t)dpad,
                               n_slots, d_qpad, d_qn, d_qnorm, d_qpos);
            HIP_TRY(hipGetLastError());
            const DbscanScreenArgs a{d_qpad, d_qn, d_xn, d_qpos, d_cut, st->rank(), s.count, s.core, d_cmask, s.parent, d_cq, d_crow, ctr0 + k, nullptr, nullptr,
                                     (uint32_t)cand_cap, (uint32_t)cq, (uint32_t)dpad, (uint32_t)(dpad / KC), (uint32_t)qt, (uint32_t)slab_rows,
                                     screen_coeff(dev.dist(), d), zero_tail ? 1u : 0u};
            const dim3 grid((uint32_t)slabs, (uint32_t)tiles);
            HIP_TRY(link ? dbscan_screen<PASS_LINK>(true, dev.dist(), (uint32_t)sh.nt, grid, (uint32_t)sh.waves, sh.lds, stream, v, a)
                         : dbscan_screen<PASS_COUNT>(true, dev.dist(), (uint32_t)sh.nt, grid, (uint32_t)sh.waves, sh.lds, stream, v, a));
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

}  // namespace

// The device side of hnswxd_exact(_device); capi.cpp holds the entries and every argument check: n >= 1.  stats (host memory, may be
// nullptr): {points answered through the screen, answered by the existing path because a buffer was outgrown, not screened, pairs
// that went through the exact chain}.
int exact_dbscan_screened(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& a, uint64_t* out_stats, bool host, void* stream,
                          std::string& err) {
    uint64_t own[4];
    uint64_t* const stats = out_stats ? out_stats : own;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    const uint64_t n = dev.view().n;
    Route route = ROUTE_UNSCREENED;
    {   // (the screened path's block is back in the pool before the existing path takes its own)
        DeviceGuard on(dev.device());
        HIP_TRY(on.status());
        const int rc = dbscan_screened_passes(dev, origin_id, a, host, static_cast<hipStream_t>(stream), &route, stats + 3, err);
        if (route == ROUTE_DONE) stats[0] = n;
        if (rc != OK || route == ROUTE_DONE) return rc;
    }
    stats[route == ROUTE_OUTGROWN ? 1 : 2] = n;
    return exact_dbscan(dev, origin_id, a, host, stream, err);
}

// The device side of hnswxd_bounds_matrix (host buffers): the screen kernel with a store epilogue
int dbscan_bounds_matrix(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanBoundsArgs& a, std::string& err) {
    const DeviceIndexView& v = dev.view();
    const uint64_t n = v.n;
    if (!metric_has_screen(dev.dist())) { err = "dbscan bounds matrix: this distance has no screen (DistL2, DistDot, DistCosine have)"; return ERR_ARG; }
    if (a.nq * n > DS_MATRIX_PAIRS) { err = "dbscan bounds matrix: nq * n above 2^24 pairs"; return ERR_ARG; }
    if (a.nq == 0 || n == 0) return OK;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    ScreenShape sh;
    if (sh.pick(dev.device(), a.d) == 0) { err = "dbscan bounds matrix: rows too long for a query tile in LDS"; return ERR_ARG; }
    const std::shared_ptr<ExactState> st = replica_state(dev, origin_id, "dbscan bounds matrix", err);
    if (!st) return ERR_DEVICE;
    const float* d_xn = nullptr;
    int rc = row_norms(*st, v, nullptr, &d_xn, err);
    if (rc != OK) return rc;
    const uint64_t tiles = (a.nq + sh.qt - 1) / sh.qt, slots = tiles * sh.qt;
    uint64_t slabs, slab_rows;
    sh.cut(n, tiles, slabs, slab_rows);
    float *d_src, *d_qpad, *d_qn, *d_lb, *d_ub;
    double* d_qnorm;
    ScratchLayout lay;
    lay.array(d_src, a.nq * a.d);
    lay.array(d_qpad, slots * sh.dpad);
    lay.array(d_qn, slots);
    lay.array(d_qnorm, slots);
    lay.arrays(a.nq * n, d_lb, d_ub);
    DevMem mem;
    rc = alloc_layout("dbscan bounds matrix", mem, lay, err);
    if (rc != OK) return rc;
    Drain drain{nullptr};
    HIP_TRY(hipMemcpyAsync(d_src, a.queries, a.nq * a.d * 4, hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(exact_screen_prep_kernel, grid_of(slots), dim3(256), 0, nullptr, d_src, (uint32_t)a.nq, (uint32_t)a.d, (uint32_t)sh.dpad, (uint32_t)slots,
                       d_qpad, d_qn, d_qnorm);
    HIP_TRY(hipGetLastError());
    DbscanScreenArgs s{};
    s.qpad = d_qpad, s.qn = d_qn, s.xn = d_xn, s.out_lb = d_lb, s.out_ub = d_ub;
    s.nq = (uint32_t)a.nq, s.dpad = (uint32_t)sh.dpad, s.nkc = (uint32_t)(sh.dpad / KC), s.qt = (uint32_t)sh.qt, s.slab_rows = (uint32_t)slab_rows;
    s.cu = screen_coeff(dev.dist(), a.d);
    s.zero_tail = dev.dist() == DIST_COSINE && dev.side_norms() == nullptr ? 1u : 0u;
    HIP_TRY(dbscan_screen<PASS_BOUNDS>(false, dev.dist(), (uint32_t)sh.nt, dim3(), (uint32_t)sh.waves, sh.lds, nullptr, v, s));
    HIP_TRY(dbscan_screen<PASS_BOUNDS>(true, dev.dist(), (uint32_t)sh.nt, dim3((uint32_t)slabs, (uint32_t)tiles), (uint32_t)sh.waves, sh.lds, nullptr, v, s));
    return copy_out({{a.out_lb, d_lb, a.nq * n * 4}, {a.out_ub, d_ub, a.nq * n * 4}}, true, nullptr, err);
}

}  // namespace hnswgpu
