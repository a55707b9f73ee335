// exact_range_screen_long.hip -- the exact range search's screen for long rows (gfx950 only): the device side of
// hnswxrl_exact_range_search_batch(_device) of include/hnsw_mi355x_exact_range_long.h (the entries and the argument checks are in
// capi.cpp).  The contract, the rerank, the scatter, the sort, the capacities and the fallback are exact_range_screen.hip's
// (exact_range_screen_parts.hpp); the screen kernel is another one, and DESIGN.md section 15.18 holds its layout and why the argument
// of section 15.14 carries over with the coefficient of section 15.16.
//
//   range_screen_long_kernel   one workgroup of four wavefronts per (tile of 128 queries, slab of rows).  NEITHER operand is resident:
//                              per step one chunk of 32 elements of the tile's 128 queries and of a block of 32 NT rows goes global ->
//                              registers -> LDS (pitch 36 floats for both, queries in front), double buffered, the next step's loads
//                              issued before this step's MFMAs and stored behind them, one barrier per step.  LDS does not depend on d.
//                              A wavefront owns 32 queries -- the A operand -- and NT accumulator tiles of 32 x 32, zeroed per row block
//                              and alive across its dpad / 32 steps.  The 16 queries that a lane's accumulator registers belong to never
//                              change, so their norms and cuts leave LDS once, behind the prologue, and stay in registers: the epilogue
//                              of a row block reads nothing but the block's row norms and the filter's words.  Epilogue per accumulator
//                              register: screen_within against the query's cut, a ballot, one 64-bit atomic per ballot with bits, the
//                              lanes store (query slot, flat row).  No lists, no thresholds, no keys.
//
// Rows of up to 256 elements go to exact_range_screen.hip's driver as they are: four wavefronts with resident queries read a query
// once per slab, not once per row block.
#include <hip/hip_runtime.h>

#include "exact_range_screen_parts.hpp"

namespace hnswgpu {
namespace {

// Accumulator tiles of a wavefront: 4 (32 queries x 128 rows, 74 752 bytes of LDS) or 2 (32 x 64, 56 320 bytes).  Two workgroups
// fit a CU either way; DESIGN.md 15.18 and RESULTS.md "Exact range search, long rows" have the registers and the times of both.
#ifndef HNSW_RANGE_LONG_NT
#define HNSW_RANGE_LONG_NT 4
#endif
constexpr uint32_t RL_QT = SQ * MAX_WAVES;   // queries of a tile
constexpr uint32_t RL_THREADS = 64u * MAX_WAVES;
constexpr uint32_t RL_PRE_Q = RL_QT * 8u / RL_THREADS;  // float4s of the queries' chunk per thread; of the rows': NT
static_assert(RL_THREADS == 256u && RL_PRE_Q == 4u, "a thread stages row (tid >> 3) + 32 j of the queries and of the rows");

constexpr uint64_t range_long_lds_bytes(uint64_t nt) { return 2ull * (RL_QT + 32 * nt) * RPITCH * 4 + RL_QT * 8; }

template <int METRIC, int NT>
__global__ __launch_bounds__(RL_THREADS, 2) void range_screen_long_kernel(DeviceIndexView ix, RangeScreenArgs a) {
    constexpr uint32_t RBN = 32u * NT;              // rows of a staged block
    constexpr uint32_t BUF = (RL_QT + RBN) * RPITCH;  // floats of one staged step: the tile's queries in front, the block's rows behind
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t half = lane >> 5, l32 = lane & 31u;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t dpad = a.dpad, nkc = a.nkc;
    float* const buf = reinterpret_cast<float*>(lds_raw);  // [2][RL_QT + RBN][RPITCH]
    float* const qnl = buf + 2u * BUF;                     // [RL_QT] the queries' norms
    float* const cutl = qnl + RL_QT;                       // [RL_QT] what a bound is compared with (screen_within)

    const uint32_t nvalid = a.nq - tile * RL_QT < RL_QT ? a.nq - tile * RL_QT : RL_QT;
    // once per (workgroup, query): the norm and the cut.  A slot behind the chunk's last query: radius -1, no candidate
    if (tid < RL_QT) {
        const float rad = tid < nvalid ? a.radius[tile * RL_QT + tid] : -1.f;
        qnl[tid] = a.qn[tile * RL_QT + tid];
        cutl[tid] = METRIC == DIST_L2 ? sqrt_cut(rad) : rad;
    }
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t steps = ((hi - lo + RBN - 1u) / RBN) * nkc;  // (block of rows, chunk of elements), chunk fastest
    const uint32_t row_stride = ix.row_stride;

    // This thread's part of a step: elements 4 (tid & 7) and the three behind of the queries (tid >> 3) + 32 j (every slot of the tile
    // is there, zero padded) and of the block's rows (tid >> 3) + 32 j.  Rows behind the slab re-read its last row; they are no
    // candidates (epilogue).
    const uint32_t srow = tid >> 3, e4 = 4u * (tid & 7u);
    const float* const qsrc = a.qpad + (size_t)(tile * RL_QT + srow) * dpad + e4;
    v4f preq[RL_PRE_Q], prex[NT];
    auto fetch = [&](uint32_t blk, uint32_t c) {
#pragma unroll
        for (int j = 0; j < (int)RL_PRE_Q; ++j) preq[j] = *reinterpret_cast<const v4f*>(qsrc + (size_t)(32u * (uint32_t)j) * dpad + c * KC);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const uint32_t r = lo + blk * RBN + srow + 32u * (uint32_t)j, e = c * KC + e4;
            v4f v = *reinterpret_cast<const v4f*>(ix.vec + (size_t)(r < hi ? r : hi - 1u) * row_stride + e);
            if (a.zero_tail != 0u && e + 4u == row_stride) { v.z = 0.f; v.w = 0.f; }
            prex[j] = v;
        }
    };
    auto stage = [&](uint32_t s) {
        float* const dst = buf + (s & 1u) * BUF + srow * RPITCH + e4;
#pragma unroll
        for (int j = 0; j < (int)RL_PRE_Q; ++j) *reinterpret_cast<v4f*>(dst + 32u * (uint32_t)j * RPITCH) = preq[j];
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<v4f*>(dst + (RL_QT + 32u * (uint32_t)j) * RPITCH) = prex[j];
    };

    v16f acc[NT];
#pragma unroll
    for (int tb = 0; tb < NT; ++tb)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[tb][v] = 0.f;
    bool mine = wave * SQ < nvalid;  // (wave-uniform) this wavefront has a query at all -- and the chunk's buffer still has room

    fetch(0u, 0u);
    stage(0u);
    __syncthreads();  // (also: the prologue's norms and cuts)
    // Register v of an accumulator tile: row = this lane's (l32) of the tile, query 8 (v / 4) + 4 half + v % 4 of the wavefront's 32
    // -- the same 16 queries for every tile and every row block of the slab.  Their norms and cuts, from LDS once.
    float qn_r[16], cut_r[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const uint32_t ql = wave * SQ + 8u * ((uint32_t)v >> 2) + ((uint32_t)v & 3u) + 4u * half;
        qn_r[v] = qnl[ql];
        cut_r[v] = cutl[ql];
    }
    uint32_t blk = 0, c = 0;  // of step s
    for (uint32_t s = 0; s < steps; ++s) {
        const bool last_chunk = c + 1u == nkc;
        const uint32_t nblk = last_chunk ? blk + 1u : blk, nc = last_chunk ? 0u : c + 1u;  // of step s + 1
        if (s + 1u < steps) fetch(nblk, nc);
        if (mine) {
            // 32 elements: four groups of 8.  A lane reads 4 consecutive elements of its query and of its NT rows (the lower 32 lanes
            // the group's first four, the upper 32 its last four); MFMA m of the group multiplies element m of both halves.
            const float* const qa = buf + (s & 1u) * BUF + (wave * SQ + l32) * RPITCH + 4u * half;
            const float* const b0 = buf + (s & 1u) * BUF + (RL_QT + l32) * RPITCH + 4u * half;
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
            if (last_chunk) {
                // Every lane is active here: lane 0 reserves the slots of a ballot's candidates.
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
                        const bool cand = elig && ql < nvalid && screen_within<METRIC>(acc[tb][v], qn_r[v], nx, a.cu, cut_r[v]);
                        const unsigned long long m = __ballot(cand);
                        if (m != 0ull) {
                            unsigned long long base = 0ull;
                            if (lane == 0u) base = atomicAdd(a.ctr, (unsigned long long)popc64(m));
                            base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                            const unsigned long long p = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                            if (cand && p < (unsigned long long)a.cand_cap) {  // (past the buffer: dropped; the counter tells)
                                a.cq[p] = tile * RL_QT + ql;
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
        blk = nblk, c = nc;
    }
}

// This unit's screen for the driver of exact_range_screen_parts.hpp: queries and rows both streamed, four wavefronts at every length
struct StreamedRangeScreen {
    static bool shape(int device, uint64_t dpad, RangeScreenShape* s) {
        int limit = 0;
        if (dpad > LONG_MAX_DPAD || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return false;
        const uint64_t nt = HNSW_RANGE_LONG_NT == 4 && range_long_lds_bytes(4) <= (uint64_t)limit ? 4 : 2;
        if (range_long_lds_bytes(nt) > (uint64_t)limit) return false;
        *s = RangeScreenShape{MAX_WAVES, (uint32_t)nt, RL_QT, 32 * nt, range_long_lds_bytes(nt)};
        return true;
    }
    static float coeff(int metric, uint64_t d) { return screen_coeff_long(metric, d); }
    // (kernel: &range_screen_long_kernel<M, NT>)
    static hipError_t launch(bool launch, int metric, const RangeScreenShape& s, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const RangeScreenArgs& a) {
        const uint32_t lds = (uint32_t)s.lds;
        hipError_t said = hipSuccess;
        const hipError_t e = for_screened_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (!launch) said = s.nt == 4u ? hipFuncSetAttribute(reinterpret_cast<const void*>(&range_screen_long_kernel<M, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                           : hipFuncSetAttribute(reinterpret_cast<const void*>(&range_screen_long_kernel<M, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            else if (s.nt == 4u) hipLaunchKernelGGL((range_screen_long_kernel<M, 4>), grid, dim3(RL_THREADS), lds, stream, ix, a);
            else hipLaunchKernelGGL((range_screen_long_kernel<M, 2>), grid, dim3(RL_THREADS), lds, stream, ix, a);
        });
        return said != hipSuccess ? said : e;
    }
};

}  // namespace

// The device side of hnswxrl_exact_range_search_batch(_device): by the rows' padded length the resident screen's call as it is, or
// the streamed screen (rows it does not take, above 4096 elements, are not screened: the existing path, stats word 2)
int exact_range_screened_long(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, uint64_t* out_stats, bool host, void* stream,
                              std::string& err) {
    if (round_up(a.d, KC) < LONG_MIN_DPAD) return exact_range_screened(dev, origin_id, a, out_stats, host, stream, err);
    return range_screened_call<StreamedRangeScreen>(dev, origin_id, a, out_stats, host, stream, err);
}

}  // namespace hnswgpu
