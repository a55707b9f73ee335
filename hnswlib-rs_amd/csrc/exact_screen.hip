// exact_screen.hip -- exhaustive exact k-NN behind a matrix-core screen (gfx950 only): the device side of
// hnswxs_exact_search_batch(_device) and hnswxs_screen_matrix of include/hnsw_mi355x_exact_screen.h (the entries and
// the argument checks are in capi.cpp).  The answers are those of exact_knn.hip byte for byte; DESIGN.md section 15.13 holds the layout,
// the bound and its derivation.  DistL2, DistDot and DistCosine, whose distance is a function of the inner product q.x and of the two
// squared norms.
//
//   exact_screen_prep_kernel   the queries of a chunk zero padded to whole 32-element chunks, every query's squared norm twice: in plain
//                              f32 (the screen's) and in the crate's arithmetic (the rerank's DistCosine finish)
//   exact_screen_xnorm_kernel  the rows' squared norms in plain f32: once per replica
//   exact_screen_kernel        one workgroup of W <= 4 wavefronts per (tile of 32 W queries, slab of rows).  The tile's queries stay in
//                              LDS for the kernel's life; the rows stream through LDS 64 rows x 32 elements at a time, double
//                              buffered.  A wavefront owns 32 queries: per staged chunk 32 v_mfma_f32_32x32x2_f32 into two 32 x 32
//                              accumulator tiles (queries are the A operand, rows the B operand: an accumulator register holds one row
//                              per lane, for two queries -- the lower and the upper 32 lanes).  Epilogue per 64 rows: every value
//                              becomes a LOWER BOUND of the f32 distance that the exact chain gives for the pair (screen_lb), a ballot
//                              over the rows of a query finds the bounds below the query's threshold, and those go into the query's
//                              sorted list of the C = k + SCREEN_MARGIN smallest keys {order bits of the bound, DataId rank}
//                              (exact_list.hpp): one writing wavefront per (query, slab), as in exact_knn.hip.
//   exact_rerank_kernel        one wavefront per query: the slabs' lists merged to the C smallest keys; each candidate's distance in
//                              the exact chain (chain4, tile_dist: the bits of exact_knn.hip), one candidate per lane; the exact keys
//                              sorted in LDS; the certificate; the answer written, or the query appended to the fallback list.
//
// The screen and the rerank have a SELF variant each, for hnswxg_exact_graph_batch(_device) and hnswxg_screen_matrix of
// include/hnsw_mi355x_exact_graph_screen.h: the queries are stored points, gathered from the replica's own rows (no prep kernel, no
// padded copy), and never their own candidates.
// The queries on the fallback list are answered by exact_device (exact_knn.hip) into their own rows; the host reads back one count.
// The rerank kernel and the driver are in exact_screen_knn.hpp, shared with exact_screen_long.hip; this unit holds the screen kernel.
#include <hip/hip_runtime.h>

#include "exact_screen_knn.hpp"

namespace hnswgpu {
namespace {

// SELF (the k-NN graph of the stored points): the tile's queries are stored points.  The prologue gathers each from its own index row
// into its LDS slot -- there is no padded copy in scratch --, its plain f32 norm is the replica's xn, and its DataId rank lies in LDS
// beside its threshold: the one row that is the point itself is never inserted (by identity: its copies and the other points of its
// DataId are candidates like any row).
template <int METRIC, bool MATRIX, bool SELF>
__global__ __launch_bounds__(64 * MAX_WAVES) void exact_screen_kernel(DeviceIndexView ix, ScreenArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nthr = blockDim.x;
    const uint32_t half = lane >> 5, l32 = lane & 31u;
    const uint32_t slab = blockIdx.x, tile = blockIdx.y;
    const uint32_t qt = a.qt, dpad = a.dpad, nkc = a.nkc, qpitch = dpad + 4u;
    float* const qs = reinterpret_cast<float*>(lds_raw);              // [qt][qpitch]
    float* const rbuf = qs + (size_t)qt * qpitch;                     // [2][RB][RPITCH]
    uint64_t* const thr = reinterpret_cast<uint64_t*>(rbuf + 2u * RB * RPITCH);  // [qt]
    uint32_t* const len = reinterpret_cast<uint32_t*>(thr + qt);      // [qt]
    float* const qnl = reinterpret_cast<float*>(len + qt);            // [qt]
    [[maybe_unused]] uint32_t* const own = reinterpret_cast<uint32_t*>(qnl + qt);  // SELF: [qt] the queries' own DataId ranks

    const uint32_t nvalid = a.nq - tile * qt < qt ? a.nq - tile * qt : qt;
    // the tile's queries: resident from here on
    {
        const float4* const src = reinterpret_cast<const float4*>(a.qpad + (size_t)tile * qt * dpad);
        const uint32_t c4n = dpad >> 2;
        for (uint32_t i = tid; i < qt * c4n; i += nthr) {
            const uint32_t q = i / c4n, c = i - q * c4n;
            if constexpr (SELF) *reinterpret_cast<v4f*>(qs + (size_t)q * qpitch + 4u * c) = self_query4(ix, self_slot(a.self, tile * qt + q, a.nq), 4u * c);
            else *reinterpret_cast<float4*>(qs + (size_t)q * qpitch + 4u * c) = src[i];
        }
        for (uint32_t q = tid; q < qt; q += nthr) {
            thr[q] = KEY_NONE;
            len[q] = 0u;
            if constexpr (SELF) {
                const uint32_t f = self_slot(a.self, tile * qt + q, a.nq);
                qnl[q] = f != NO_SELF ? a.xn[f] : 0.f;
                own[q] = f != NO_SELF ? a.rank[f] : NO_SELF;
            } else {
                qnl[q] = a.qn[tile * qt + q];
            }
        }
    }
    const uint32_t lo = slab * a.slab_rows;
    const uint32_t hi = ix.n - lo < a.slab_rows ? ix.n : lo + a.slab_rows;
    const uint32_t steps = ((hi - lo + RB - 1u) / RB) * nkc;  // (block of rows, chunk of elements), chunk fastest
    const uint32_t row_stride = ix.row_stride;

    // this thread's part of a staged block: float4 number i = tid + j * nthr of RB x 8 (a block is 512 of them).  Rows behind the slab
    // re-read its last row; they are no candidates (epilogue).
    float4 pre[8];
    auto fetch = [&](uint32_t s) {
        const uint32_t blk = s / nkc, c = s - blk * nkc;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t i = tid + j * nthr;
            if (i < RB * 8u) {
                const uint32_t r = lo + blk * RB + (i >> 3), e = c * KC + 4u * (i & 7u);
                float4 v = *reinterpret_cast<const float4*>(ix.vec + (size_t)(r < hi ? r : hi - 1u) * row_stride + e);
                if (a.zero_tail != 0u && e + 4u == row_stride) { v.z = 0.f; v.w = 0.f; }
                pre[j] = v;
            }
        }
    };
    auto stage = [&](uint32_t s) {
        float* const dst = rbuf + (s & 1u) * (RB * RPITCH);
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t i = tid + j * nthr;
            if (i < RB * 8u) *reinterpret_cast<float4*>(dst + (i >> 3) * RPITCH + 4u * (i & 7u)) = pre[j];
        }
    };

    v16f acc0, acc1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
    const bool mine = wave * SQ < nvalid;  // (wave-uniform) this wavefront has a query at all
    const float* const qrow = qs + (size_t)(wave * SQ + l32) * qpitch + 4u * half;
    const size_t slot = ((size_t)tile * a.n_slabs + slab) * qt;
    const uint32_t cap = a.cap;

    fetch(0u);
    stage(0u);
    __syncthreads();
    for (uint32_t s = 0; s < steps; ++s) {
        if (s + 1u < steps) fetch(s + 1u);
        const uint32_t blk = s / nkc, c = s - blk * nkc;
        if (mine) {
            // 32 elements: four groups of 8.  A lane reads 4 consecutive elements of its query and of its two rows (the lower 32
            // lanes the group's first four, the upper 32 its last four); MFMA m of the group multiplies element m of both halves.
            const float* const b0 = rbuf + (s & 1u) * (RB * RPITCH) + l32 * RPITCH + 4u * half;
            const float* const b1 = b0 + 32u * RPITCH;
            const float* const qa = qrow + c * KC;
#pragma unroll
            for (uint32_t g = 0; g < KC / 8u; ++g) {
                const float4 q4 = *reinterpret_cast<const float4*>(qa + 8u * g);
                const float4 x0 = *reinterpret_cast<const float4*>(b0 + 8u * g);
                const float4 x1 = *reinterpret_cast<const float4*>(b1 + 8u * g);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, x0.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, x1.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, x0.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, x1.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, x0.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, x1.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, x0.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, x1.w, acc1, 0, 0, 0);
            }
            if (c + 1u == nkc) {
                // Register v of an accumulator tile: row = this lane's (l32) of the tile, query 8 (v / 4) + 4 half + v % 4 of the
                // wavefront's 32.  A ballot's lower word is one query's 32 rows, its upper word another's.
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) {
                    const uint32_t r = lo + blk * RB + 32u * (uint32_t)tb + l32;
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
                        const float lb = screen_lb<METRIC>(tb == 0 ? acc0[v] : acc1[v], qnl[ql], nx, a.cu);
                        if constexpr (MATRIX) {
                            if (in && ql < nvalid) a.out_lb[(size_t)(tile * qt + ql) * ix.n + r] = lb;
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
                for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
            }
        }
        if (s + 1u < steps) stage(s + 1u);
        __syncthreads();
    }
    if constexpr (!MATRIX)
        for (uint32_t q = tid; q < nvalid; q += nthr) a.lens[slot + q] = len[q];
}

// This unit's screen for the driver of exact_screen_knn.hpp: the tile's queries resident in LDS
struct ResidentScreen {
    static constexpr uint64_t ROWS = RB;
    static uint64_t waves(int device, uint64_t dpad, bool self) { return screen_waves(device, dpad, self); }
    static uint64_t lds_bytes(uint64_t waves, uint64_t dpad, bool self) { return screen_lds_bytes(waves, dpad, self); }
    static float coeff(int metric, uint64_t d) { return screen_coeff(metric, d); }
    static const char* too_long() { return "for a query tile in LDS"; }
    template <bool MATRIX>
    static hipError_t launch(int metric, dim3 grid, uint32_t waves, uint32_t lds, hipStream_t stream, const DeviceIndexView& ix, const ScreenArgs& a) {
        return for_screened_metric(metric, [&](auto m) {
            constexpr int M = decltype(m)::value;
            // (more LDS than the default limit of a launch: said once per kernel; a refusal shows in the launch itself)
            if (a.self != nullptr) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&exact_screen_kernel<M, MATRIX, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL((exact_screen_kernel<M, MATRIX, true>), grid, dim3(64u * waves), lds, stream, ix, a);
            } else {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&exact_screen_kernel<M, MATRIX, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL((exact_screen_kernel<M, MATRIX, false>), grid, dim3(64u * waves), lds, stream, ix, a);
            }
        });
    }
};

}  // namespace

// The device side of hnswxg_exact_graph_batch(_device) for rows of up to 256 elements (exact_screen_long.hip routes): the resident
// screen's SELF variant, four wavefronts
int exact_graph_screened_resident(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, uint64_t* out_stats, bool host, void* stream,
                                  std::string& err) {
    return screened_graph_call<ResidentScreen>(dev, origin_id, a, out_stats, host, stream, err);
}

// The device side of hnswxs_exact_search_batch(_device); capi.cpp holds the entries and every argument check.
int exact_screened(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactScreenArgs& a, bool host, void* stream, std::string& err) {
    return screened_call<ResidentScreen>(dev, origin_id, a, host, stream, err);
}

// The device side of hnswxs_screen_matrix (host buffers): the screen kernel with a store epilogue
int exact_screen_matrix(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ScreenMatrixArgs& a, std::string& err) {
    return screen_matrix_call<ResidentScreen>(dev, origin_id, a, err);
}

}  // namespace hnswgpu

