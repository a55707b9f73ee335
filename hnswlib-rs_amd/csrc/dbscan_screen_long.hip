// dbscan_screen_long.hip -- exact DBSCAN's two-sided screen for long rows (gfx950 only): the device side of hnswxdl_exact(_device) and
// hnswxdl_bounds_matrix of include/hnsw_mi355x_dbscan_long.h (the entries and the argument checks are in capi.cpp).  The contract, the
// passes, the prep, cut and rerank kernels, the capacities and the fallback are dbscan_screen.hip's (dbscan_screen_parts.hpp); the
// screen kernel is another one.  DESIGN.md section 15.19 holds its layout and the upper bound beyond 1120 elements, section 15.16 the
// lower bound there, section 15.15 the pipeline and why the answers are those of dbscan.hip byte for byte.
//
//   dbscan_screen_long_kernel  <METRIC, PASS, NT> one workgroup of four wavefronts per (tile of 128 query slots, slab of rows).  NEITHER
//                              operand is resident: per step one chunk of 32 elements of the tile's 128 padded points and of a block
//                              of 32 NT rows goes global -> registers -> LDS (pitch 36 floats for both, queries in front), double
//                              buffered, the next step's loads issued before this step's MFMAs and stored behind them, one barrier per
//                              step.  LDS does not depend on d.  A wavefront owns 32 queries -- the A operand -- and NT accumulator
//                              tiles of 32 x 32, zeroed per row block and alive across its dpad / 32 steps.  Per query of the tile, in
//                              LDS: the norm, the position, COUNT a counter, LINK the core flag and a root the query had.  The 16
//                              queries that a lane's accumulator registers belong to never change, so their norms leave LDS once and
//                              stay in registers; the cut is one word of the call, in a scalar.  Epilogue per accumulator register:
//                              the text of dbscan_screen_kernel's -- SURE, MISS or UNDECIDED by screen_band and two compares; COUNT a
//                              ballot and a popcount, LINK cc_unite under the skip rule, the band into the candidate buffer; BOUNDS
//                              lb and ub stored.
//
// Rows of up to 256 elements go to dbscan_screen.hip's call as they are: four wavefronts with resident queries read a query once per
// slab, not once per row block.
#include <hip/hip_runtime.h>

#include "dbscan_screen_parts.hpp"

namespace hnswgpu {
namespace {

// Accumulator tiles of a wavefront: 4 (32 queries x 128 rows, 75 776 bytes of LDS) or 2 (32 x 64, 57 344 bytes).  Two workgroups fit
// a CU either way; DESIGN.md 15.19 has the registers of both for every pass.
#ifndef HNSW_DBSCAN_LONG_NT
#define HNSW_DBSCAN_LONG_NT 4
#endif
constexpr uint32_t DL_QT = SQ * MAX_WAVES;   // query slots of a tile
constexpr uint32_t DL_THREADS = 64u * MAX_WAVES;
constexpr uint32_t DL_PRE_Q = DL_QT * 8u / DL_THREADS;  // float4s of the queries' chunk per thread; of the rows': NT
static_assert(DL_THREADS == 256u && DL_PRE_Q == 4u, "a thread stages row (tid >> 3) + 32 j of the queries and of the rows");

constexpr uint64_t dbscan_long_lds_bytes(uint64_t nt) { return 2ull * (DL_QT + 32 * nt) * RPITCH * 4 + DL_QT * 16; }

template <int METRIC, int PASS, int NT>
__global__ __launch_bounds__(DL_THREADS, 2) void dbscan_screen_long_kernel(DeviceIndexView ix, DbscanScreenArgs a) {
    constexpr uint32_t RBN = 32u * NT;              // rows of a staged block
    constexpr uint32_t BUF = (DL_QT + RBN) * RPITCH;  // floats of one staged step: the tile's queries in front, the block's rows behind
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t half = lane >> 5, l32 = lane & 31u;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t dpad = a.dpad, nkc = a.nkc;
    float* const buf = reinterpret_cast<float*>(lds_raw);  // [2][DL_QT + RBN][RPITCH]
    float* const qnl = buf + 2u * BUF;                     // [DL_QT] the queries' norms
    uint32_t* const qposl = reinterpret_cast<uint32_t*>(qnl + DL_QT);  // [DL_QT] their positions
    uint32_t* const auxl = qposl + DL_QT;                  // [DL_QT] COUNT: the sure hits so far; LINK: a root the query had
    uint32_t* const corel = auxl + DL_QT;                  // [DL_QT] LINK: the query is core

    const uint32_t nvalid = a.nq - tile * DL_QT < DL_QT ? a.nq - tile * DL_QT : DL_QT;
    // once per (workgroup, query slot): the norm and the pass's state.  A slot behind the chunk's last query is never live (epilogue)
    if (tid < DL_QT) {
        qnl[tid] = a.qn[tile * DL_QT + tid];
        if constexpr (PASS != PASS_BOUNDS) {
            const uint32_t pos = tid < nvalid ? a.qpos[tile * DL_QT + tid] : 0u;
            qposl[tid] = pos;
            auxl[tid] = PASS == PASS_LINK ? pos : 0u;
            corel[tid] = PASS == PASS_LINK && tid < nvalid ? a.core[pos] : 0u;
        }
    }
    float cut = 0.f;
    if constexpr (PASS != PASS_BOUNDS) cut = *a.cut;
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t steps = ((hi - lo + RBN - 1u) / RBN) * nkc;  // (block of rows, chunk of elements), chunk fastest
    const uint32_t row_stride = ix.row_stride;

    // This thread's part of a step: elements 4 (tid & 7) and the three behind of the queries (tid >> 3) + 32 j (every slot of the tile
    // is there, zero padded) and of the block's rows (tid >> 3) + 32 j.  Rows behind the slab re-read its last row; they are misses
    // (epilogue).
    const uint32_t srow = tid >> 3, e4 = 4u * (tid & 7u);
    const float* const qsrc = a.qpad + (size_t)(tile * DL_QT + srow) * dpad + e4;
    v4f preq[DL_PRE_Q], prex[NT];
    auto fetch = [&](uint32_t blk, uint32_t c) {
#pragma unroll
        for (int j = 0; j < (int)DL_PRE_Q; ++j) preq[j] = *reinterpret_cast<const v4f*>(qsrc + (size_t)(32u * (uint32_t)j) * dpad + c * KC);
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
        for (int j = 0; j < (int)DL_PRE_Q; ++j) *reinterpret_cast<v4f*>(dst + 32u * (uint32_t)j * RPITCH) = preq[j];
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<v4f*>(dst + (DL_QT + 32u * (uint32_t)j) * RPITCH) = prex[j];
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
            a.cq[p] = tile * DL_QT + ql;
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

    fetch(0u, 0u);
    stage(0u);
    __syncthreads();  // (also: the prologue's norms and state)
    // Register v of an accumulator tile: row = this lane's (l32) of the tile, query 8 (v / 4) + 4 half + v % 4 of the wavefront's 32
    // -- the same 16 queries for every tile and every row block of the slab: a ballot's lower word is one query's 32 rows, its upper
    // word another's.  Their norms, from LDS once.
    float qn_r[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) qn_r[v] = qnl[wave * SQ + 8u * ((uint32_t)v >> 2) + ((uint32_t)v & 3u) + 4u * half];
    uint32_t blk = 0, c = 0;  // of step s
    for (uint32_t s = 0; s < steps; ++s) {
        const bool last_chunk = c + 1u == nkc;
        const uint32_t nblk = last_chunk ? blk + 1u : blk, nc = last_chunk ? 0u : c + 1u;  // of step s + 1
        if (s + 1u < steps) fetch(nblk, nc);
        if (mine) {
            // 32 elements: four groups of 8.  A lane reads 4 consecutive elements of its query and of its NT rows (the lower 32 lanes
            // the group's first four, the upper 32 its last four); MFMA m of the group multiplies element m of both halves.
            const float* const qa = buf + (s & 1u) * BUF + (wave * SQ + l32) * RPITCH + 4u * half;
            const float* const b0 = buf + (s & 1u) * BUF + (DL_QT + l32) * RPITCH + 4u * half;
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
                // Every lane is active here.
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
                        screen_band<METRIC>(acc[tb][v], qn_r[v], nx, a.cu, ok, blo, bhi);
                        const bool live = in && ql < nvalid;
                        if constexpr (PASS == PASS_BOUNDS) {
                            if (live) {
                                const size_t o = (size_t)(tile * DL_QT + ql) * ix.n + r;
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
        blk = nblk, c = nc;
    }
    if constexpr (PASS == PASS_COUNT) {
        // one integer add per (query, slab); the barrier behind the last block has made the counters visible
        if (lane < SQ && wave * SQ + lane < nvalid) {
            const uint32_t cnt = auxl[wave * SQ + lane];
            if (cnt != 0u) atomicAdd(a.count + qposl[wave * SQ + lane], cnt);
        }
    }
}

// This unit's screen for the driver of dbscan_screen_parts.hpp: queries and rows both streamed, four wavefronts at every length
struct StreamedDbscanScreen {
    static bool shape(int device, uint64_t dpad, DbscanScreenShape* s) {
        int limit = 0;
        if (dpad > LONG_MAX_DPAD || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return false;
        const uint64_t nt = HNSW_DBSCAN_LONG_NT == 4 && dbscan_long_lds_bytes(4) <= (uint64_t)limit ? 4 : 2;
        if (dbscan_long_lds_bytes(nt) > (uint64_t)limit) return false;
        *s = DbscanScreenShape{MAX_WAVES, (uint32_t)nt, DL_QT, 32 * nt, dbscan_long_lds_bytes(nt)};
        return true;
    }
    // both bounds: DESIGN.md 15.19 carries the upper side's second-order terms to d = 4096 and needs no more than the lower side's
    static float coeff(int metric, uint64_t d) { return screen_coeff_long(metric, d); }
    static const char* too_long() { return "for the streamed screen (d above 4096)"; }
    // (kernel: &dbscan_screen_long_kernel<M, PASS, NT>)
    template <int PASS>
    static hipError_t launch(bool launch, int metric, const DbscanScreenShape& s, dim3 grid, hipStream_t stream, const DeviceIndexView& ix, const DbscanScreenArgs& a) {
        const uint32_t lds = (uint32_t)s.lds;
        hipError_t said = hipSuccess;
        const hipError_t e = for_screened_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (!launch) said = s.nt == 4u ? hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_screen_long_kernel<M, PASS, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                           : hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_screen_long_kernel<M, PASS, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            else if (s.nt == 4u) hipLaunchKernelGGL((dbscan_screen_long_kernel<M, PASS, 4>), grid, dim3(DL_THREADS), lds, stream, ix, a);
            else hipLaunchKernelGGL((dbscan_screen_long_kernel<M, PASS, 2>), grid, dim3(DL_THREADS), lds, stream, ix, a);
        });
        return said != hipSuccess ? said : e;
    }
};

}  // namespace

// The device side of hnswxdl_exact(_device): by the rows' padded length the resident screen's call as it is, or the streamed screen
// (rows it does not take, above 4096 elements, are not screened: the existing path, stats word 2)
int exact_dbscan_screened_long(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& a, uint64_t* out_stats, bool host, void* stream,
                               std::string& err) {
    if (round_up((uint64_t)dev.view().d, KC) < LONG_MIN_DPAD) return exact_dbscan_screened(dev, origin_id, a, out_stats, host, stream, err);
    return dbscan_screened_call<StreamedDbscanScreen>(dev, origin_id, a, out_stats, host, stream, err);
}

// The device side of hnswxdl_bounds_matrix (host buffers): the streamed screen kernel with a store epilogue, whatever d is
int dbscan_bounds_matrix_long(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanBoundsArgs& a, std::string& err) {
    return dbscan_bounds_matrix_call<StreamedDbscanScreen>(dev, origin_id, a, err);
}

}  // namespace hnswgpu
