// dbscan_screen.hip -- exact DBSCAN behind a two-sided matrix-core screen (gfx950 only): the device side of hnswxd_exact(_device) and
// hnswxd_bounds_matrix of include/hnsw_mi355x_dbscan_screen.h (the entries and the argument checks are in capi.cpp).  The answers are
// those of dbscan.hip byte for byte; DESIGN.md section 15.15 holds the pipeline, the upper bound and the argument, section 15.13 the
// lower bound.  DistL2, DistDot and DistCosine.  DBSCAN needs "v <= eps or not" of nearly every pair and the bits of v of very few:
// the screen proves hits (ub <= eps) as well as misses (lb > eps), and only the band between the two sees the exact chain.
//
// dbscan_screen_parts.hpp holds what this unit shares with dbscan_screen_long.hip: the arguments, screen_band, the prep, cut and
// rerank kernels and the driver; this unit names its kernel to it through ResidentDbscanScreen.
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

#include "dbscan_screen_parts.hpp"

namespace hnswgpu {
namespace {

// Accumulator tiles of a wavefront: the rule of exact_range_screen.hip -- 4 where the LDS holds the larger row blocks without costing
// a wavefront, else 2
#ifndef HNSW_DBSCAN_SCREEN_NT
#define HNSW_DBSCAN_SCREEN_NT 4
#endif

uint64_t dbscan_screen_lds_bytes(uint64_t waves, uint64_t dpad, uint64_t nt) { return screen_lds_bytes(waves, dpad) + 2ull * (nt - 2) * 32 * RPITCH * 4; }

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

// This unit's screen for the driver of dbscan_screen_parts.hpp: the tile's queries resident in LDS, as many wavefronts (4 at most) as
// its LDS holds queries for
struct ResidentDbscanScreen {
    static bool shape(int device, uint64_t dpad, DbscanScreenShape* s) {
        const uint64_t waves = screen_waves(device, dpad);
        int limit = 0;
        if (waves == 0 || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return false;
        const uint64_t nt = HNSW_DBSCAN_SCREEN_NT == 4 && dbscan_screen_lds_bytes(waves, dpad, 4) <= (uint64_t)limit ? 4 : 2;
        *s = DbscanScreenShape{(uint32_t)waves, (uint32_t)nt, waves * SQ, 32 * nt, dbscan_screen_lds_bytes(waves, dpad, nt)};
        return true;
    }
    static float coeff(int metric, uint64_t d) { return screen_coeff(metric, d); }
    static const char* too_long() { return "for a query tile in LDS"; }
    // (kernel: &dbscan_screen_kernel<M, PASS, NT>)
    template <int PASS>
    static hipError_t launch(bool launch, int metric, const DbscanScreenShape& s, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const DbscanScreenArgs& a) {
        const uint32_t lds = (uint32_t)s.lds;
        hipError_t said = hipSuccess;
        const hipError_t e = for_screened_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (!launch) said = s.nt == 4u ? hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_screen_kernel<M, PASS, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                           : hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_screen_kernel<M, PASS, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            else if (s.nt == 4u) hipLaunchKernelGGL((dbscan_screen_kernel<M, PASS, 4>), grid, dim3(64u * s.waves), lds, stream, ix, a);
            else hipLaunchKernelGGL((dbscan_screen_kernel<M, PASS, 2>), grid, dim3(64u * s.waves), lds, stream, ix, a);
        });
        return said != hipSuccess ? said : e;
    }
};

}  // namespace

// The device side of hnswxd_exact(_device); capi.cpp holds the entries and every argument check: n >= 1.  stats (host memory, may be
// nullptr): {points answered through the screen, answered by the existing path because a buffer was outgrown, not screened, pairs
// that went through the exact chain}.
int exact_dbscan_screened(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& a, uint64_t* out_stats, bool host, void* stream,
                          std::string& err) {
    return dbscan_screened_call<ResidentDbscanScreen>(dev, origin_id, a, out_stats, host, stream, err);
}

// The device side of hnswxd_bounds_matrix (host buffers): the screen kernel with a store epilogue
int dbscan_bounds_matrix(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanBoundsArgs& a, std::string& err) {
    return dbscan_bounds_matrix_call<ResidentDbscanScreen>(dev, origin_id, a, err);
}

}  // namespace hnswgpu
