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
// Everything but range_screen_kernel -- the other kernels, the capacities and the driver -- is in exact_range_screen_parts.hpp, which
// exact_range_screen_long.hip (rows of up to 4096 elements) shares.
#include <hip/hip_runtime.h>

#include "exact_range_screen_parts.hpp"

namespace hnswgpu {
namespace {

// Accumulator tiles of a wavefront where the LDS holds the larger row blocks without costing a wavefront: 4 (32 queries x 128 rows)
// or 2 (32 x 64, the k-NN screen's).  RESULTS.md "Exact range search" has both figures.
#ifndef HNSW_RANGE_SCREEN_NT
#define HNSW_RANGE_SCREEN_NT 4
#endif

uint64_t range_screen_lds_bytes(uint64_t waves, uint64_t dpad, uint64_t nt) { return screen_lds_bytes(waves, dpad) + 2ull * (nt - 2) * 32 * RPITCH * 4; }

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


// This unit's screen for the driver of exact_range_screen_parts.hpp: a tile's queries resident, as many wavefronts as the LDS holds
// queries for.  (kernel: &range_screen_kernel<M, NT>)
struct ResidentRangeScreen {
    static bool shape(int device, uint64_t dpad, RangeScreenShape* s) {
        const uint64_t waves = screen_waves(device, dpad);
        int lds_limit = 0;
        if (waves == 0 || hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return false;
        const uint64_t nt = HNSW_RANGE_SCREEN_NT == 4 && range_screen_lds_bytes(waves, dpad, 4) <= (uint64_t)lds_limit ? 4 : 2;
        *s = RangeScreenShape{(uint32_t)waves, (uint32_t)nt, waves * SQ, 32 * nt, range_screen_lds_bytes(waves, dpad, nt)};
        return true;
    }
    static float coeff(int metric, uint64_t d) { return screen_coeff(metric, d); }
    static hipError_t launch(bool launch, int metric, const RangeScreenShape& s, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const RangeScreenArgs& a) {
        const uint32_t lds = (uint32_t)s.lds;
        hipError_t said = hipSuccess;
        const hipError_t e = for_screened_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (!launch) said = s.nt == 4u ? hipFuncSetAttribute(reinterpret_cast<const void*>(&range_screen_kernel<M, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                           : hipFuncSetAttribute(reinterpret_cast<const void*>(&range_screen_kernel<M, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            else if (s.nt == 4u) hipLaunchKernelGGL((range_screen_kernel<M, 4>), grid, dim3(64u * s.waves), lds, stream, ix, a);
            else hipLaunchKernelGGL((range_screen_kernel<M, 2>), grid, dim3(64u * s.waves), lds, stream, ix, a);
        });
        return said != hipSuccess ? said : e;
    }
};

}  // namespace

// The device side of hnswxr_exact_range_search_batch(_device); capi.cpp holds the entries and every argument check.  stats (host
// memory, may be nullptr): {screened, answered by the existing path because a buffer was outgrown, not screened}.
int exact_range_screened(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, uint64_t* out_stats, bool host, void* stream,
                         std::string& err) {
    return range_screened_call<ResidentRangeScreen>(dev, origin_id, a, out_stats, host, stream, err);
}

}  // namespace hnswgpu
