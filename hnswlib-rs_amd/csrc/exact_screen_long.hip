// exact_screen_long.hip -- the exact k-NN screen for long rows (gfx950 only): the device side of hnswxl_exact_search_batch(_device) and
// hnswxl_screen_matrix of include/hnsw_mi355x_exact_long.h (the entries and the argument checks are in capi.cpp).  The contract, the
// rerank, the certificate and the fallback are exact_screen.hip's (exact_screen_knn.hpp); the screen kernel is another one, and DESIGN.md
// section 15.16 holds its layout and the bound for rows of more than 1120 elements.
//
//   exact_screen_long_kernel   one workgroup of four wavefronts per (tile of 128 queries, slab of rows).  NEITHER operand is resident:
//                              per step one chunk of 32 elements of the tile's 128 queries and of a block of 32 NT rows goes global ->
//                              registers -> LDS (pitch 36 floats for both), double buffered, the next step's loads issued before this
//                              step's MFMAs and stored behind them, one barrier per step.  LDS does not depend on d.  A wavefront owns
//                              32 queries and multiplies them with all 32 NT rows of the block: per 8-element group one 16-byte read
//                              of its query and NT of its rows, 4 NT v_mfma_f32_32x32x2_f32 into NT accumulator tiles of 32 x 32, which
//                              live across the dpad / 32 steps of a row block.  Epilogue once per row block: exact_screen_kernel's.
//
// Rows of up to 256 elements go to exact_screen.hip's driver as they are: four wavefronts with resident queries read a query once per
// slab, not once per row block.  The same routing serves the screened exact graph (hnswxg_*, include/hnsw_mi355x_exact_graph_screen.h),
// whose device side is here: both screens' SELF variants, DESIGN.md section 15.17.
#include <hip/hip_runtime.h>

#include "exact_screen_knn.hpp"

namespace hnswgpu {
namespace {

#ifndef HNSW_LONG_NT
#define HNSW_LONG_NT 2  // accumulator tiles of a wavefront (DESIGN.md 15.16 has the variants that were timed: 4 is slower)
#endif
#ifndef HNSW_LONG_WAVES_PER_SIMD
#define HNSW_LONG_WAVES_PER_SIMD 2  // what the registers are held to: 256 VGPRs, two workgroups per CU (at NT = 4 that spills)
#endif
constexpr uint32_t LONG_NT = HNSW_LONG_NT;
constexpr uint32_t LONG_QT = SQ * MAX_WAVES;         // queries of a tile
constexpr uint32_t LONG_ROWS = 32u * LONG_NT;        // rows of a staged block
constexpr uint32_t LONG_STAGED = LONG_QT + LONG_ROWS;  // staged rows of a step: the tile's queries in front, the block's rows behind
constexpr uint32_t LONG_THREADS = 64u * MAX_WAVES;
constexpr uint32_t LONG_PRE_Q = LONG_QT * 8u / LONG_THREADS;    // float4s of the queries' chunk per thread; of the rows': LONG_NT
static_assert(LONG_THREADS == 256u && LONG_QT * 8u % LONG_THREADS == 0u, "a thread stages row (tid >> 3) + 32 j of the queries and of the rows");

uint64_t long_lds_bytes(bool self) { return 2ull * LONG_STAGED * RPITCH * 4 + LONG_QT * (self ? 20 : 16); }

// SELF (the k-NN graph of the stored points): exact_screen_kernel's, with the query fetch of every step reading 32 elements of the
// tile's points from their own index rows (a thread keeps the flat ids of its four query rows in registers)
template <int METRIC, bool MATRIX, bool SELF>
__global__ __launch_bounds__(LONG_THREADS, HNSW_LONG_WAVES_PER_SIMD) void exact_screen_long_kernel(DeviceIndexView ix, ScreenArgs a) {
    constexpr uint32_t BUF = LONG_STAGED * RPITCH;  // floats of one staged step
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t half = lane >> 5, l32 = lane & 31u;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t dpad = a.dpad, nkc = a.nkc;
    float* const buf = reinterpret_cast<float*>(lds_raw);                    // [2][LONG_STAGED][RPITCH]
    uint64_t* const thr = reinterpret_cast<uint64_t*>(buf + 2u * BUF);       // [LONG_QT]
    uint32_t* const len = reinterpret_cast<uint32_t*>(thr + LONG_QT);        // [LONG_QT]
    float* const qnl = reinterpret_cast<float*>(len + LONG_QT);              // [LONG_QT]
    [[maybe_unused]] uint32_t* const own = reinterpret_cast<uint32_t*>(qnl + LONG_QT);  // SELF: [LONG_QT] the queries' own DataId ranks

    const uint32_t nvalid = a.nq - tile * LONG_QT < LONG_QT ? a.nq - tile * LONG_QT : LONG_QT;
    if (tid < LONG_QT) {
        thr[tid] = KEY_NONE;
        len[tid] = 0u;
        if constexpr (SELF) {
            const uint32_t f = self_slot(a.self, tile * LONG_QT + tid, a.nq);
            qnl[tid] = f != NO_SELF ? a.xn[f] : 0.f;
            own[tid] = f != NO_SELF ? a.rank[f] : NO_SELF;
        } else {
            qnl[tid] = a.qn[tile * LONG_QT + tid];
        }
    }
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t nblk = (hi - lo + LONG_ROWS - 1u) / LONG_ROWS;
    const uint32_t steps = nblk * nkc;  // (block of rows, chunk of elements), chunk fastest
    const uint32_t row_stride = ix.row_stride;

    // This thread's part of a step: elements 4 (tid & 7) and the three behind of the queries (tid >> 3) + 32 j (every slot of the tile
    // is there, zero padded) and of the block's rows (tid >> 3) + 32 j.  Rows behind the slab re-read its last row; they are no
    // candidates (epilogue).
    const uint32_t srow = tid >> 3, e4 = 4u * (tid & 7u);
    const float* const qsrc = a.qpad + (size_t)(tile * LONG_QT + srow) * dpad + e4;
    v4f preq[LONG_PRE_Q], prex[LONG_NT];
    [[maybe_unused]] uint32_t qf[LONG_PRE_Q];  // SELF: the flat ids of this thread's query rows (a slot behind the last query: none, zeros)
    if constexpr (SELF) {
#pragma unroll
        for (int j = 0; j < (int)LONG_PRE_Q; ++j) qf[j] = self_slot(a.self, tile * LONG_QT + srow + 32u * (uint32_t)j, a.nq);
    }
    auto fetch = [&](uint32_t blk, uint32_t c) {
#pragma unroll
        for (int j = 0; j < (int)LONG_PRE_Q; ++j) {
            if constexpr (SELF) preq[j] = self_query4(ix, qf[j], c * KC + e4);
            else preq[j] = *reinterpret_cast<const v4f*>(qsrc + (size_t)(32u * (uint32_t)j) * dpad + c * KC);
        }
#pragma unroll
        for (int j = 0; j < (int)LONG_NT; ++j) {
            const uint32_t r = lo + blk * LONG_ROWS + srow + 32u * (uint32_t)j, e = c * KC + e4;
            v4f v = *reinterpret_cast<const v4f*>(ix.vec + (size_t)(r < hi ? r : hi - 1u) * row_stride + e);
            if (a.zero_tail != 0u && e + 4u == row_stride) { v.z = 0.f; v.w = 0.f; }
            prex[j] = v;
        }
    };
    auto stage = [&](uint32_t s) {
        float* const dst = buf + (s & 1u) * BUF + srow * RPITCH + e4;
#pragma unroll
        for (int j = 0; j < (int)LONG_PRE_Q; ++j) *reinterpret_cast<v4f*>(dst + 32u * (uint32_t)j * RPITCH) = preq[j];
#pragma unroll
        for (int j = 0; j < (int)LONG_NT; ++j) *reinterpret_cast<v4f*>(dst + (LONG_QT + 32u * (uint32_t)j) * RPITCH) = prex[j];
    };

    v16f acc[LONG_NT];
#pragma unroll
    for (uint32_t tb = 0; tb < LONG_NT; ++tb)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[tb][v] = 0.f;
    const bool mine = wave * SQ < nvalid;  // (wave-uniform) this wavefront has a query at all
    const size_t slot = ((size_t)tile * a.n_slabs + slab) * LONG_QT;
    const uint32_t cap = a.cap;

    fetch(0u, 0u);
    stage(0u);
    __syncthreads();
    uint32_t blk = 0, c = 0;  // of step s
    for (uint32_t s = 0; s < steps; ++s) {
        const bool last_chunk = c + 1u == nkc;
        const uint32_t nblk_ = last_chunk ? blk + 1u : blk, nc = last_chunk ? 0u : c + 1u;  // of step s + 1
        if (s + 1u < steps) fetch(nblk_, nc);
        if (mine) {
            // 32 elements: four groups of 8.  A lane reads 4 consecutive elements of its query and of its NT rows (the lower 32 lanes
            // the group's first four, the upper 32 its last four); MFMA m of the group multiplies element m of both halves.
            const float* const qa = buf + (s & 1u) * BUF + (wave * SQ + l32) * RPITCH + 4u * half;
            const float* const b0 = buf + (s & 1u) * BUF + (LONG_QT + l32) * RPITCH + 4u * half;
#pragma unroll
            for (uint32_t g = 0; g < KC / 8u; ++g) {
                const float4 q4 = *reinterpret_cast<const float4*>(qa + 8u * g);
                float4 x[LONG_NT];
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb) x[tb] = *reinterpret_cast<const float4*>(b0 + tb * 32u * RPITCH + 8u * g);
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, x[tb].x, acc[tb], 0, 0, 0);
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, x[tb].y, acc[tb], 0, 0, 0);
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, x[tb].z, acc[tb], 0, 0, 0);
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, x[tb].w, acc[tb], 0, 0, 0);
            }
            if (last_chunk) {
                // Register v of an accumulator tile: row = this lane's (l32) of the tile, query 8 (v / 4) + 4 half + v % 4 of the
                // wavefront's 32.  A ballot's lower word is one query's 32 rows, its upper word another's.
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb) {
                    const uint32_t r = lo + blk * LONG_ROWS + 32u * tb + l32;
                    const bool in = r < hi;
                    const uint32_t rc = in ? r : hi - 1u;
                    const float nx = a.xn[rc];
                    [[maybe_unused]] const uint32_t rk = a.rank[rc];
                    [[maybe_unused]] bool elig = in;
                    if constexpr (!MATRIX)
                        if (a.allow != nullptr) elig = in && ((a.allow[rc >> 5] >> (rc & 31u)) & 1u) != 0u;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const uint32_t q_lo = wave * SQ + 8u * ((uint32_t)v >> 2) + ((uint32_t)v & 3u);  // the lower lanes' query
                        const uint32_t ql = q_lo + 4u * half;
                        const float lb = screen_lb<METRIC>(acc[tb][v], qnl[ql], nx, a.cu);
                        if constexpr (MATRIX) {
                            if (in && ql < nvalid) a.out_lb[(size_t)(tile * LONG_QT + ql) * ix.n + r] = lb;
                        } else {
                            const uint64_t key = make_key(lb, rk);
                            bool cand = elig && ql < nvalid;
                            if constexpr (SELF) cand = cand && rk != own[ql];
                            const unsigned long long m = __ballot(cand && key < thr[ql]);
                            if ((m & 0xFFFFFFFFull) != 0ull)
                                screen_insert(a.lists + (slot + q_lo) * cap, thr, len, q_lo, cap, key, m & 0xFFFFFFFFull);
                            if ((m >> 32) != 0ull)
                                screen_insert(a.lists + (slot + q_lo + 4u) * cap, thr, len, q_lo + 4u, cap, key, m & ~0xFFFFFFFFull);
                        }
                    }
                }
#pragma unroll
                for (uint32_t tb = 0; tb < LONG_NT; ++tb)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[tb][v] = 0.f;
            }
        }
        if (s + 1u < steps) stage(s + 1u);
        __syncthreads();
        blk = nblk_, c = nc;
    }
    if constexpr (!MATRIX)
        for (uint32_t q = tid; q < nvalid; q += LONG_THREADS) a.lens[slot + q] = len[q];
}

// This unit's screen for the driver of exact_screen_knn.hpp: queries and rows both streamed
struct StreamedScreen {
    static constexpr uint64_t ROWS = LONG_ROWS;
    static uint64_t waves(int device, uint64_t dpad, bool self) {
        int limit = 0;
        if (dpad > LONG_MAX_DPAD || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return 0;
        return long_lds_bytes(self) <= (uint64_t)limit ? MAX_WAVES : 0;
    }
    static uint64_t lds_bytes(uint64_t, uint64_t, bool self) { return long_lds_bytes(self); }
    static float coeff(int metric, uint64_t d) { return screen_coeff_long(metric, d); }
    static const char* too_long() { return "for the streamed screen (d above 4096)"; }
    template <bool MATRIX>
    static hipError_t launch(int metric, dim3 grid, uint32_t, uint32_t lds, hipStream_t stream, const DeviceIndexView& ix, const ScreenArgs& a) {
        return for_screened_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            // (more LDS than the default limit of a launch: said once per kernel; a refusal shows in the launch itself)
            if (a.self != nullptr) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&exact_screen_long_kernel<M, MATRIX, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL((exact_screen_long_kernel<M, MATRIX, true>), grid, dim3(LONG_THREADS), lds, stream, ix, a);
            } else {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&exact_screen_long_kernel<M, MATRIX, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL((exact_screen_long_kernel<M, MATRIX, false>), grid, dim3(LONG_THREADS), lds, stream, ix, a);
            }
        });
    }
};

}  // namespace

// The device side of hnswxl_exact_search_batch(_device): by the rows' padded length the resident screen's driver as it is, or the
// streamed screen (rows it does not take, above 4096 elements, are not screened: the existing path, stats word 2)
int exact_screened_long(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactScreenArgs& a, bool host, void* stream, std::string& err) {
    if (round_up(a.d, KC) < LONG_MIN_DPAD) return exact_screened(dev, origin_id, a, host, stream, err);
    return screened_call<StreamedScreen>(dev, origin_id, a, host, stream, err);
}

// The device side of hnswxl_screen_matrix (host buffers): the streamed screen kernel with a store epilogue, whatever d is
int exact_screen_long_matrix(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ScreenMatrixArgs& a, std::string& err) {
    return screen_matrix_call<StreamedScreen>(dev, origin_id, a, err);
}

// The device side of hnswxg_exact_graph_batch(_device) (hnsw_mi355x_exact_graph_screen.h): the k-NN graph of the stored points behind
// the SELF variant of the screen that the rows' padded length picks, as above (above 4096 elements: not screened, stats word 2)
int exact_graph_screened(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, uint64_t* out_stats, bool host, void* stream,
                         std::string& err) {
    if (round_up((uint64_t)dev.view().d, KC) < LONG_MIN_DPAD) return exact_graph_screened_resident(dev, origin_id, a, out_stats, host, stream, err);
    return screened_graph_call<StreamedScreen>(dev, origin_id, a, out_stats, host, stream, err);
}

// The device side of hnswxg_screen_matrix (host buffers; a.self): the bounds of the kernel that the graph call runs at this length
int exact_graph_screen_matrix(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ScreenMatrixArgs& a, std::string& err) {
    if (round_up(a.d, KC) < LONG_MIN_DPAD) return exact_screen_matrix(dev, origin_id, a, err);
    return screen_matrix_call<StreamedScreen>(dev, origin_id, a, err);
}

}  // namespace hnswgpu
