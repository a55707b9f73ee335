// search_kernels.inc -- device code of the search path (included once per metric translation unit).
// See search_device.hip for the overview; everything here is gfx950-only HIP.
#pragma clang fp contract(off)
#include <type_traits>
#include "ln_f32.hpp"

// tuning knobs (overridable with make TUNE=-D...)
#ifndef HNSW_LB_WAVES
#define HNSW_LB_WAVES 5   // __launch_bounds__ waves per SIMD of the lean kernel (<= 64 S result slots, S < 16)
#endif
#ifndef HNSW_MERGE_LISTS
#define HNSW_MERGE_LISTS 1  // accept rule for a whole neighbour list at once (merge_list) when at least this many qualify; 0: never
#endif
#ifndef HNSW_LB_WAVES_STRICT
#define HNSW_LB_WAVES_STRICT 4  // strict kernel: the literal-heap rerun needs ~120 VGPRs; spilling it slows both paths
#endif
#ifndef HNSW_LB_DESCEND
#define HNSW_LB_DESCEND 6  // waves per SIMD of the descent kernel
#endif
#ifndef HNSW_DPP_ASM
#define HNSW_DPP_ASM 1  // the DPP adds of the distance chain written out as inline assembly: no s_nop pairs in front of them (dpp_add)
#endif
#ifndef HNSW_PIPE_ROWS
#define HNSW_PIPE_ROWS 1  // strict search kernel with 4 result slots per lane: the next round's row loads in front of this round's chain (group_dist PIPE)
#endif
#ifndef HNSW_DEEP_G2
#define HNSW_DEEP_G2 1  // strict search kernel, lists of more than 16 fresh ids: sixteen row loads per lane in flight (group_dist DEEP)
#endif
#ifndef HNSW_COLD
#define HNSW_COLD __attribute__((noinline))  // the cold literal-heap paths of a strict search: real calls (own register allocation)
#endif
#ifndef HNSW_PHASE_TIMING
#define HNSW_PHASE_TIMING 0  // 1: per-query cycle counts of the expansion phases go to stats (profiling builds); 2: of the literal pops
#endif
#if HNSW_PHASE_TIMING
#define PH_T(var) const unsigned long long var = clock64()
#define PH_ACC(idx, t0, t1) ph[idx] += (uint32_t)((t1) - (t0))
#else
#define PH_T(var)
#define PH_ACC(idx, t0, t1)
#endif

namespace hnswgpu {
namespace {

__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ uint32_t readlane_u(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ uint32_t popc64(unsigned long long m) { return (uint32_t)__popcll(m); }
__device__ __forceinline__ int ctz64(unsigned long long m) { return __ffsll((long long)m) - 1; }
__device__ __forceinline__ unsigned long long lanemask_lt(int lane) { return (1ull << lane) - 1ull; }

// ---------------------------------------------------------------------------------------
// Distance<f32>::eval (anndists 0.1, scalar build): the last step after the left-to-right sum `a`.  Rows and
// queries are zero padded and x + 0 == x, so running over the padding leaves every sum bit-identical to the
// reference's d-term sum.
// ---------------------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ float dist_finish(float a) {
    if constexpr (METRIC == DIST_L2) return __builtin_sqrtf(a);          // sqrt(sum (a-b)^2): a true metric, not squared
    else if constexpr (METRIC == DIST_DOT) return fmaxf(1.f - a, 0.f);   // 1 - sum a*b, clamped at 0
    else if constexpr (METRIC == DIST_HELLINGER) return __builtin_sqrtf(fmaxf(1.f - a, 0.f));  // sqrt(max(1 - sum sqrt(a) sqrt(b), 0))
    else if constexpr (METRIC == DIST_JENSENSHANNON) return __builtin_sqrtf(0.5f * a);          // sqrt(0.5 * sum ...)
    else return a;                                                       // DistL1: sum |a-b|; DistJeffreys: the sum itself
}
// per-element terms of the distances between probability vectors (anndists 0.1; va = the query, vb = the row)
__device__ __forceinline__ float hellinger_term(float q, float x) { return __builtin_sqrtf(q) * __builtin_sqrtf(x); }
__device__ __forceinline__ float jeffreys_term(float q, float x) {
    const float M_MIN = 1.0e-30f;
    return (q - x) * ln_f32(fmaxf(q, M_MIN) / fmaxf(x, M_MIN));
}
// DistJensenShannon adds up to two terms per element, in this order; a skipped term is an added +0 (exact: the running
// sum is never -0)
__device__ __forceinline__ void jensenshannon_terms(float q, float x, float& ta, float& tb) {
    const float mean_ab = 0.5f * (q + x);
    ta = q > 0.f ? q * ln_f32(q / mean_ab) : 0.f;
    tb = x > 0.f ? x * ln_f32(x / mean_ab) : 0.f;
}

// Single-wavefront workgroups: LDS instructions of one wave execute in program order, so a
// ds_write followed by a ds_read of another lane's data needs no s_barrier and no drained counter --
// only a fence that keeps the compiler from reordering the two.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// per-point squared norms (DistCosine's third sum), wave-uniform base pointer => scalar loads of the base
typedef __attribute__((address_space(4))) const double* nrm_ptr_t;

// ---------------------------------------------------------------------------------------
// batch_dist: distances from the query (staged in LDS by stage_query) to `nf` <= 64 rows whose flat ids sit in
// ids_lds[0..nf).  Returns the distance to row r in LANE r (INFINITY in the other lanes).
//
// G lanes per row, straight from global memory.  Lane g of a row's group loads the float4 chunks g, g + G,
// g + 2G, ... (G x 16 B contiguous per row and load instruction: whole 64- or 32-byte sectors) and forms the
// per-element terms of ITS chunks -- these are independent, exact, and two per instruction (packed f32).  The
// reference's left-to-right sum is the one dependent chain; it runs in the group's first lane, which reads the
// other lanes' terms through the DPP operand of v_add_f32 (row_shl:j, no extra instruction).  Per row of d
// elements that is d adds plus d/G subtract+multiply instruction slots instead of 3d, and the rows of a batch
// share them: 16 rows at G = 4, 32 rows at G = 2.  The query sits in LDS (every lane needs different chunks).
//
// DistCosine sums f32 products in f64 (three sums).  The two norms do not depend on the pair: the query's is
// summed once per query (stage_query), every point's once at upload (row_sq_norms_kernel) -- the crate's own
// arithmetic: f32 square widened to f64, summed left to right -- so only sum a_i*b_i is left per row: f32
// products by all lanes of a group, the f64 add chain in its first lane (v_mov_dpp + v_cvt_f64_f32 + v_add_f64).
// ---------------------------------------------------------------------------------------
// DistCosine: the query's own sum of squares (the crate's arithmetic: f32 squares widened to f64, summed left to right) goes
// behind the staged row; the other metrics need nothing more.  Ends with the tile visible to every lane.
template <int METRIC>
__device__ __forceinline__ void finish_staged_query(float4* tile, uint32_t row_stride, int lane, uint32_t d) {
    __syncthreads();
    if constexpr (METRIC == KM_COSINE_SIMD8) {
        // the query's sum of squares in the crate's SIMD order (f32: 8 vertical accumulators over the full blocks of 8,
        // horizontal sum, then the d % 8 tail elements)
        const float* qf = reinterpret_cast<const float*>(tile);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        uint32_t i = 0;
        for (; i + 8u <= d; i += 8u)
            for (int j = 0; j < 8; ++j) acc[j] = acc[j] + qf[i + j] * qf[i + j];
        float s1 = 0.f;
        for (int j = 0; j < 8; ++j) s1 = s1 + acc[j];
        for (; i < d; ++i) s1 = s1 + qf[i] * qf[i];
        if (lane == 0) *reinterpret_cast<float*>(tile + (row_stride >> 2)) = s1;
        __syncthreads();
    }
    if constexpr (METRIC == DIST_COSINE || METRIC == KM_COSINE_F16) {  // (half rows: the query side is f32 all the same)
        double s1 = 0.;
        for (uint32_t c = 0; c < (row_stride >> 2); ++c) {
            const float4 v = tile[c];
            s1 = s1 + (double)(v.x * v.x); s1 = s1 + (double)(v.y * v.y); s1 = s1 + (double)(v.z * v.z); s1 = s1 + (double)(v.w * v.w);
        }
        if (lane == 0) *reinterpret_cast<double*>(tile + (row_stride >> 2)) = s1;
        __syncthreads();
    }
}
// copies the (zero padded) query row into LDS (once per query); DistCosine: + the query's own sum of squares behind it
// (stored_row: the query is a row of the index itself -- construction -- whose last 8 bytes may hold its norm, see group_dist)
template <int METRIC>
__device__ __forceinline__ void stage_query(float4* tile, const float* __restrict__ qglobal, uint32_t row_stride, int lane,
                                            uint32_t d, bool stored_row_with_norm = false) {
    const float4* src = reinterpret_cast<const float4*>(qglobal);
    for (uint32_t i = (uint32_t)lane; i < (row_stride >> 2); i += 64) {
        float4 v = src[i];
        if (METRIC == DIST_COSINE && stored_row_with_norm && i + 1u == (row_stride >> 2)) { v.z = 0.f; v.w = 0.f; }
        tile[i] = v;
    }
    finish_staged_query<METRIC>(tile, row_stride, lane, d);
}

typedef float v2f __attribute__((ext_vector_type(2)));
template <int J>
__device__ __forceinline__ float dpp_row_shl(float v) {  // value of lane + J (same row of 16 lanes)
    if constexpr (J == 0) return v;
    else return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x100 + J, 0xf, 0xf, true));
}
template <int METRIC>
__device__ __forceinline__ v2f term2(const v2f s, const v2f r) {
    if constexpr (METRIC == DIST_L2) {
        const v2f t = s - r;
        return t * t;
    } else if constexpr (METRIC == DIST_L1) {
        const v2f t = s - r;
        return v2f{fabsf(t.x), fabsf(t.y)};
    } else {
        return s * r;  // DistDot, and the dot-product sum of DistCosine (f32 products, like the crate)
    }
}
// The DPP adds of a chunk, written out by hand: acc += lo.x, lo.y, hi.x, hi.y of lane + 1, then of lane + 2, lane + 3.  Left to
// itself the compiler puts `s_nop 1` in front of every v_add_f32_dpp: its hazard recogniser holds "VALU writes a VGPR, a DPP
// instruction reads it: 2 wait states" against ALL operands of the next instruction, the running sum included -- but only the
// operand that goes through the lane-permute network is fetched early, and that one (a term) was written at least two
// instructions before (the chunk's four own-lane adds come first): 96 of the 128 adds of a d = 128 row each dragged an idle
// issue slot and two idle cycles along.  (One asm statement per chunk: between two of them the compiler would put a nop
// again.  HNSW_DPP_ASM = 0: the compiler's form; the bit-exactness tests of the arithmetic run on whichever is built.)
#define HNSW_DPP_ADD(term, j) "v_add_f32_dpp %0, " term ", %0 row_shl:" #j " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define HNSW_DPP_ADD4(j) HNSW_DPP_ADD("%1", j) HNSW_DPP_ADD("%2", j) HNSW_DPP_ADD("%3", j) HNSW_DPP_ADD("%4", j)
template <int G>
__device__ __forceinline__ void dpp_tail(float& acc, float a, float b, float c, float d) {
    static_assert(G == 2 || G == 4, "lanes per row");
    if constexpr (G == 4) asm(HNSW_DPP_ADD4(1) HNSW_DPP_ADD4(2) HNSW_DPP_ADD4(3) : "+v"(acc) : "v"(a), "v"(b), "v"(c), "v"(d));
    else asm(HNSW_DPP_ADD4(1) : "+v"(acc) : "v"(a), "v"(b), "v"(c), "v"(d));
}
// ACC = float (L2 / L1 / Dot) or double (Cosine: every f32 term is widened before it is added)
template <int G, int J, typename ACC>
__device__ __forceinline__ void chain_add(ACC& acc, const v2f lo, const v2f hi) {
    if constexpr (std::is_same<ACC, float>::value && HNSW_DPP_ASM != 0) {
        acc = acc + lo.x;
        acc = acc + lo.y;
        acc = acc + hi.x;
        acc = acc + hi.y;
        dpp_tail<G>(acc, lo.x, lo.y, hi.x, hi.y);
    } else {
        acc = acc + (ACC)dpp_row_shl<J>(lo.x);
        acc = acc + (ACC)dpp_row_shl<J>(lo.y);
        acc = acc + (ACC)dpp_row_shl<J>(hi.x);
        acc = acc + (ACC)dpp_row_shl<J>(hi.y);
        if constexpr (J + 1 < G) chain_add<G, J + 1, ACC>(acc, lo, hi);
    }
}
// DistJensenShannon: two terms per element (a's, then b's)
template <int G, int J>
__device__ __forceinline__ void chain_add2(float& acc, const float4 ta, const float4 tb) {
    acc = acc + dpp_row_shl<J>(ta.x); acc = acc + dpp_row_shl<J>(tb.x);
    acc = acc + dpp_row_shl<J>(ta.y); acc = acc + dpp_row_shl<J>(tb.y);
    acc = acc + dpp_row_shl<J>(ta.z); acc = acc + dpp_row_shl<J>(tb.z);
    acc = acc + dpp_row_shl<J>(ta.w); acc = acc + dpp_row_shl<J>(tb.w);
    if constexpr (J + 1 < G) chain_add2<G, J + 1>(acc, ta, tb);
}
// norm_tail (wave-uniform): this round ends with the row's last chunk and that chunk's .z/.w are not data but the row's
// f64 squared norm (DistCosine rows with two free floats of padding, see group_dist): the lane holding it (g == G - 1) hands
// the two words to the group's first lane and replaces them by the zero padding the sum expects.
// between(): work that does not depend on the rows, run after this round's loads are issued and before they are used
struct NoOverlap { __device__ __forceinline__ void operator()() const {} };
// ROW: the element type of the stored rows -- float, or _Float16 on a half-storage replica (KM_*_F16).  A chunk is four elements
// either way (16 or 8 bytes); the lane <-> chunk map, the rounds and everything behind round_load are the same.
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
template <typename ROW> struct row_chunk { typedef float4 type; };
template <> struct row_chunk<_Float16> { typedef half4_t type; };
template <int G, int NU>
__device__ __forceinline__ void round_load(float4 (&x)[NU], const float4* __restrict__ row) {
#pragma unroll
    for (int u = 0; u < NU; ++u) x[u] = row[u * G];
}
// half rows: 8 bytes per chunk and lane, widened into the same float4 (binary16 -> binary32 is exact, subnormals included:
// v_cvt_f32_f16 under the default mode, which keeps f16 denormals) -- the chain then sees the values an f32 replica holds
template <int G, int NU>
__device__ __forceinline__ void round_load(float4 (&x)[NU], const half4_t* __restrict__ row) {
    half4_t h[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) h[u] = row[u * G];
#pragma unroll
    for (int u = 0; u < NU; ++u) x[u] = make_float4((float)h[u].x, (float)h[u].y, (float)h[u].z, (float)h[u].w);
}
template <int METRIC, int G, int NU, typename ACC>
__device__ __forceinline__ void round_chain(ACC& acc, float4 (&x)[NU], const float4* qp, bool norm_tail, bool last_lane, double& s2) {
    if constexpr (METRIC == DIST_COSINE) {
        if (norm_tail) {
            const uint32_t lo = __builtin_bit_cast(uint32_t, dpp_row_shl<G - 1>(x[NU - 1].z));
            const uint32_t hi = __builtin_bit_cast(uint32_t, dpp_row_shl<G - 1>(x[NU - 1].w));
            s2 = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
            if (last_lane) { x[NU - 1].z = 0.f; x[NU - 1].w = 0.f; }
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const float4 qv = qp[u * G];
        if constexpr (METRIC == DIST_JENSENSHANNON) {
            float4 ta, tb;
            jensenshannon_terms(qv.x, x[u].x, ta.x, tb.x);
            jensenshannon_terms(qv.y, x[u].y, ta.y, tb.y);
            jensenshannon_terms(qv.z, x[u].z, ta.z, tb.z);
            jensenshannon_terms(qv.w, x[u].w, ta.w, tb.w);
            chain_add2<G, 0>(acc, ta, tb);
        } else if constexpr (METRIC == DIST_HELLINGER || METRIC == DIST_JEFFREYS) {
            v2f lo, hi;
            if constexpr (METRIC == DIST_HELLINGER) {
                lo = v2f{hellinger_term(qv.x, x[u].x), hellinger_term(qv.y, x[u].y)};
                hi = v2f{hellinger_term(qv.z, x[u].z), hellinger_term(qv.w, x[u].w)};
            } else {
                lo = v2f{jeffreys_term(qv.x, x[u].x), jeffreys_term(qv.y, x[u].y)};
                hi = v2f{jeffreys_term(qv.z, x[u].z), jeffreys_term(qv.w, x[u].w)};
            }
            chain_add<G, 0, ACC>(acc, lo, hi);
        } else {
            const v2f lo = term2<METRIC>(v2f{qv.x, qv.y}, v2f{x[u].x, x[u].y});
            const v2f hi = term2<METRIC>(v2f{qv.z, qv.w}, v2f{x[u].z, x[u].w});
            chain_add<G, 0, ACC>(acc, lo, hi);
        }
    }
}
template <int METRIC, int G, int NU, typename ACC, typename ROW = float, typename BETWEEN>
__device__ __forceinline__ void group_round(ACC& acc, const typename row_chunk<ROW>::type* __restrict__ row, const float4* qp, bool norm_tail,
                                            bool last_lane, double& s2, BETWEEN&& between, bool run_between) {
    float4 x[NU];
    round_load<G, NU>(x, row);
    if (run_between) between();
    round_chain<METRIC, G, NU, ACC>(acc, x, qp, norm_tail, last_lane, s2);
}
// rows s0 .. s0 + 64/G of the batch; returns `result` with the lanes of these rows replaced
// DEEP: two lanes per row with SIXTEEN loads per lane in flight where the row has them (a d = 128 row whole): the second round of
// eight no longer starts behind the first round's chain, one HBM round trip later (64 VGPRs of loads: for kernels with room)
// PIPE: long rows (more than one round of eight loads per lane: d > 32 G) with the NEXT round's loads issued before this round's
// chain -- two sets of eight registers quadruples that take turns, no copies -- so that a wavefront always has row bytes in
// flight; without it a d = 784 row is seven rounds of "round trip, then chain" one after the other, and the kernel sits at 0.65 of
// the HBM peak with its vector ALU half idle (profiles/r06_mnist784_hbm_rocprofv3_summary.txt).  32 more VGPRs: for the kernels
// that has them (strict, 4 result slots per lane -- ef 129 .. 256, what BASELINE's d = 784 config is searched with --, built for
// three waves per SIMD; the 16-slot kernel is at its 256 registers already).
// row_dist: the distance from the query at `qlds` (per lane: a wavefront may hold two queries, hnsw_search_pair_kernel) to row `id`,
// computed by the G lanes of the row's group; the value is valid in the group's first lane (g == 0)
// RS: the row stride as a compile-time fact (0: the run-time argument) -- the rounds below are then decided by the compiler
template <int METRIC, int G, bool DEEP = false, bool PIPE = false, typename ROW = float, int RS = 0, typename BETWEEN>
__device__ __forceinline__ float row_dist(const float* __restrict__ vec, uint32_t row_stride_arg, nrm_ptr_t nrm2, const float4* qlds,
                                          uint32_t id, uint32_t g, BETWEEN&& between, bool run_between) {
    typedef typename std::conditional<METRIC == DIST_COSINE, double, float>::type ACC;
    typedef typename row_chunk<ROW>::type chunk_t;
    const uint32_t row_stride = RS != 0 ? (uint32_t)RS : row_stride_arg;
    const uint32_t nchunk = row_stride >> 2;  // four-element chunks per row: a multiple of 8
    // (half rows: `vec` names binary16 elements, row_stride of them per row -- the row's address halves, nothing else moves)
    const chunk_t* row = reinterpret_cast<const chunk_t*>(reinterpret_cast<const ROW*>(vec) + (size_t)id * row_stride) + g;
    const float4* qp = qlds + g;
    // DistCosine: the point's squared norm comes from nrm2[] -- or, when that is null, from the last 8 bytes of the row
    // itself (rows whose zero padding has room for it: no second fetch, the bytes arrive with the row's last sector)
    double s2 = 0.;
    bool in_row = false;
    if constexpr (METRIC == DIST_COSINE) {
        in_row = std::is_same<ROW, float>::value && nrm2 == nullptr;  // (half rows never carry their norm)
        if (!in_row) s2 = nrm2[id];
    }
    const bool last_lane = g == (uint32_t)(G - 1);
    ACC acc = 0;
    // rounds of NU loads per lane, all in flight before the first is consumed; a row is a whole number of
    // 8-chunk (128-byte) units, so the tail of a row is a round of 4 and/or 2 loads
    // (`between` runs behind the loads of the row's first round)
    uint32_t base = 0;
    if constexpr (DEEP && G == 2) {
        for (; base + 16u * (uint32_t)G <= nchunk; base += 16u * (uint32_t)G)
            group_round<METRIC, G, 16, ACC, ROW>(acc, row + base, qp + base, in_row && base + 16u * (uint32_t)G == nchunk, last_lane, s2, between,
                                            run_between && base == 0u);
    }
    if constexpr (PIPE) {
        constexpr uint32_t STEP = 8u * (uint32_t)G;
        if (base + STEP <= nchunk) {
            float4 x[8], y[8];
            round_load<G, 8>(x, row + base);
            if (run_between && base == 0u) between();
            for (;;) {
                bool more = base + 2u * STEP <= nchunk;  // (wave-uniform)
                if (more) round_load<G, 8>(y, row + base + STEP);
                round_chain<METRIC, G, 8, ACC>(acc, x, qp + base, in_row && base + STEP == nchunk, last_lane, s2);
                base += STEP;
                if (!more) break;
                more = base + 2u * STEP <= nchunk;
                if (more) round_load<G, 8>(x, row + base + STEP);
                round_chain<METRIC, G, 8, ACC>(acc, y, qp + base, in_row && base + STEP == nchunk, last_lane, s2);
                base += STEP;
                if (!more) break;
            }
        }
    } else {
        for (; base + 8u * (uint32_t)G <= nchunk; base += 8u * (uint32_t)G)
            group_round<METRIC, G, 8, ACC, ROW>(acc, row + base, qp + base, in_row && base + 8u * (uint32_t)G == nchunk, last_lane, s2, between,
                                           run_between && base == 0u);
    }
    if (base + 4u * (uint32_t)G <= nchunk) {
        group_round<METRIC, G, 4, ACC, ROW>(acc, row + base, qp + base, in_row && base + 4u * (uint32_t)G == nchunk, last_lane, s2, between,
                                       run_between && base == 0u);
        base += 4u * (uint32_t)G;
    }
    if constexpr (G == 4) {
        if (base + 2u * (uint32_t)G <= nchunk) {
            group_round<METRIC, G, 2, ACC, ROW>(acc, row + base, qp + base, in_row && base + 2u * (uint32_t)G == nchunk, last_lane, s2, between,
                                           run_between && base == 0u);
            base += 2u * (uint32_t)G;
        }
    }
    float v;
    if constexpr (METRIC == DIST_COSINE) {
        const double s1 = *reinterpret_cast<const double*>(qlds + nchunk);
        v = 0.f;
        if (s1 > 0. && s2 > 0.) {
            const double du = 1. - acc / __builtin_sqrt(s1 * s2);
            v = (float)fmax(du, 0.);
        }
    } else {
        v = dist_finish<METRIC>(acc);
    }
    return v;
}
template <int METRIC, int G, bool DEEP = false, bool PIPE = false, typename ROW = float, int RS = 0, typename BETWEEN>
__device__ __forceinline__ float group_dist(const float* __restrict__ vec, uint32_t row_stride, nrm_ptr_t nrm2, const float4* qlds,
                                            const uint32_t* ids_lds, uint32_t s0, uint32_t nf, int lane, float result, BETWEEN&& between,
                                            bool run_between) {
    constexpr uint32_t ROWS = 64u / (uint32_t)G;
    const uint32_t g = (uint32_t)lane & (uint32_t)(G - 1);
    const uint32_t r = s0 + (uint32_t)lane / (uint32_t)G;
    // lanes past the last row re-read row s0 (same cache lines as the lanes that own it: free)
    const uint32_t id = ids_lds[r < nf ? r : s0];
    float v = row_dist<METRIC, G, DEEP, PIPE, ROW, RS>(vec, row_stride, nrm2, qlds, id, g, between, run_between);
    v = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((((uint32_t)lane - s0) * (uint32_t)G) & 63u) << 2, __builtin_bit_cast(int, v)));
    if ((uint32_t)lane >= s0 && (uint32_t)lane < s0 + ROWS && (uint32_t)lane < nf) result = v;
    return result;
}

// ---------------------------------------------------------------------------------------
// The same distances in (an unpinned restatement of: the crate is not available here, see HNSWGPU_ARITH_SIMD8 in the header) the
// summation order of the crate's `simdeez_f` / `stdsimd` builds (Cargo.toml:104-111; every number
// the reference publishes comes from them, README.md:46-56): 8 vertical f32 accumulators over the full blocks of 8 elements,
// their horizontal sum left to right, then the d % 8 tail elements one by one; DistCosine with three such f32 sums.  Opt-in
// (hnswgpu_set_arithmetic), never the default: the answers then equal the oracle's dist_simd8, not the scalar build's.
// Four lanes per row with the SAME loads as the scalar routine (lane g: float4 chunks g, g + 4, ...: 64 contiguous bytes per row
// and instruction -- an eight-byte-per-lane layout that keeps every accumulator lane-local was measured first and lost 10 % to
// the doubled number of load instructions): the four chunks of one round are the blocks 2u (lanes 0, 1) and 2u + 1 (lanes 2, 3),
// lane 0 / 2 holding slots 0-3, lane 1 / 3 slots 4-7.  Lanes 0 and 1 keep the 8 accumulators: they add their own terms (block
// 2u), then the terms of lanes 2 and 3 (block 2u + 1) through the DPP operand -- per accumulator d / 8 adds in block order, as
// the crate's vertical loop does -- and lane 0 finishes with the horizontal sum and the tail: 16 dependent adds whatever d is.
// ---------------------------------------------------------------------------------------
template <int KM>
__device__ __forceinline__ constexpr int simd8_base() {
    return KM == KM_L2_SIMD8 ? DIST_L2 : KM == KM_COSINE_SIMD8 ? DIST_COSINE : KM == KM_DOT_SIMD8 ? DIST_DOT : DIST_L1;
}
template <int BASE>
__device__ __forceinline__ float4 simd8_term(const float4 q, const float4 x) {
    const v2f lo = term2<BASE>(v2f{q.x, q.y}, v2f{x.x, x.y}), hi = term2<BASE>(v2f{q.z, q.w}, v2f{x.z, x.w});
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 dpp4_shl2(const float4 t) { return make_float4(dpp_row_shl<2>(t.x), dpp_row_shl<2>(t.y), dpp_row_shl<2>(t.z), dpp_row_shl<2>(t.w)); }
__device__ __forceinline__ float4 sel4(bool c, const float4 a) { return c ? a : make_float4(0.f, 0.f, 0.f, 0.f); }
// acc += the terms of blocks b0 = 2 u and b0 + 1 (in lanes 0 / 1 of the row's group), in that order; blocks >= nblk go to `tail`
// instead (the tail block; behind it the zero padding, whose terms are exact zeros wherever they are added)
__device__ __forceinline__ void simd8_accumulate(float4& acc, float4& tail, const float4 t, uint32_t b0, uint32_t nblk, bool all_full) {
    const float4 t1 = dpp4_shl2(t);
    if (all_full) {
        acc = add4(add4(acc, t), t1);
    } else {
        const bool f0 = b0 < nblk, f1 = b0 + 1u < nblk;  // wave-uniform
        acc = add4(add4(acc, sel4(f0, t)), sel4(f1, t1));
        tail = add4(add4(tail, sel4(!f0, t)), sel4(!f1, t1));
    }
}
// horizontal sum of the 8 accumulators (slots 0-3 in the group's lane 0, 4-7 in lane 1), then the 8 slots of the tail
__device__ __forceinline__ float simd8_finish_sum(const float4 acc, const float4 tail) {
    float s = 0.f + acc.x;
    s = s + acc.y; s = s + acc.z; s = s + acc.w;
    s = s + dpp_row_shl<1>(acc.x); s = s + dpp_row_shl<1>(acc.y); s = s + dpp_row_shl<1>(acc.z); s = s + dpp_row_shl<1>(acc.w);
    s = s + tail.x; s = s + tail.y; s = s + tail.z; s = s + tail.w;
    s = s + dpp_row_shl<1>(tail.x); s = s + dpp_row_shl<1>(tail.y); s = s + dpp_row_shl<1>(tail.z); s = s + dpp_row_shl<1>(tail.w);
    return s;
}
// one round: NU chunks per lane = block pairs u0 .. u0 + NU - 1, all loads in flight before the first is used
template <int BASE, int NU, typename BETWEEN>
__device__ __forceinline__ void simd8_round(float4& acc, float4& acc2, float4& tail, float4& tail2, const float4* __restrict__ row,
                                            const float4* qp, uint32_t u0, uint32_t nblk, bool zero_norm_words, BETWEEN&& between,
                                            bool run_between) {
    float4 x[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) x[u] = row[u * 4];
    if (run_between) between();
    if (zero_norm_words) { x[NU - 1].z = 0.f; x[NU - 1].w = 0.f; }  // DistCosine rows: not data but the stored f64 norm (group_dist)
    const bool all_full = 2u * (u0 + (uint32_t)NU) <= nblk;  // the usual round: full blocks only
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const uint32_t b0 = 2u * (u0 + (uint32_t)u);
        simd8_accumulate(acc, tail, simd8_term<BASE>(qp[u * 4], x[u]), b0, nblk, all_full);
        if constexpr (BASE == DIST_COSINE)
            simd8_accumulate(acc2, tail2, make_float4(x[u].x * x[u].x, x[u].y * x[u].y, x[u].z * x[u].z, x[u].w * x[u].w), b0, nblk, all_full);
    }
}
// rows s0 .. s0 + 16 of the batch; returns `result` with the lanes of these rows replaced
template <int KM, typename BETWEEN>
__device__ __forceinline__ float group_dist_simd8(const float* __restrict__ vec, uint32_t row_stride, uint32_t d, bool norm_in_row,
                                                  const float4* qlds, const uint32_t* ids_lds, uint32_t s0, uint32_t nf, int lane,
                                                  float result, BETWEEN&& between, bool run_between) {
    constexpr int BASE = simd8_base<KM>();
    const uint32_t g = (uint32_t)lane & 3u;
    const uint32_t r = s0 + ((uint32_t)lane >> 2);
    const uint32_t id = ids_lds[r < nf ? r : s0];
    const float4* row = reinterpret_cast<const float4*>(vec + (size_t)id * row_stride) + g;
    const float4* qp = qlds + g;
    const uint32_t nblk = d >> 3;             // full blocks of 8 (the tail block, if any, is block nblk)
    const uint32_t npair = row_stride >> 4;   // block pairs per padded row = chunks per lane: a multiple of 2
    const bool last_lane_norm = BASE == DIST_COSINE && norm_in_row && g == 3u;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), acc2 = acc, tail = acc, tail2 = acc;
    uint32_t u0 = 0;
    for (; u0 + 8u <= npair; u0 += 8u)
        simd8_round<BASE, 8>(acc, acc2, tail, tail2, row + 4u * u0, qp + 4u * u0, u0, nblk, last_lane_norm && u0 + 8u == npair, between, run_between && u0 == 0u);
    if (u0 + 4u <= npair) {
        simd8_round<BASE, 4>(acc, acc2, tail, tail2, row + 4u * u0, qp + 4u * u0, u0, nblk, last_lane_norm && u0 + 4u == npair, between, run_between && u0 == 0u);
        u0 += 4u;
    }
    if (u0 + 2u <= npair)
        simd8_round<BASE, 2>(acc, acc2, tail, tail2, row + 4u * u0, qp + 4u * u0, u0, nblk, last_lane_norm && u0 + 2u == npair, between, run_between && u0 == 0u);
    const float s = simd8_finish_sum(acc, tail);
    float v;
    if constexpr (BASE == DIST_COSINE) {
        const float s1 = *reinterpret_cast<const float*>(qlds + (row_stride >> 2));  // the query's, summed the same way (finish_staged_query)
        const float s2 = simd8_finish_sum(acc2, tail2);
        v = s1 > 0.f && s2 > 0.f ? fmaxf(1.f - s / __builtin_sqrtf(s1 * s2), 0.f) : 0.f;
    } else {
        v = dist_finish<BASE>(s);
    }
    v = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((((uint32_t)lane - s0) * 4u) & 63u) << 2, __builtin_bit_cast(int, v)));
    if ((uint32_t)lane >= s0 && (uint32_t)lane < s0 + 16u && (uint32_t)lane < nf) result = v;
    return result;
}

// between(): runs ONCE, while the first row loads of the batch are in flight (the search puts the insertion of the batch's ids
// into the visited table there: work that does not need the rows, behind an HBM round trip that has to be waited for anyway)
template <int METRIC, bool DEEP = false, bool PIPE = false, int RS = 0, typename BETWEEN>
__device__ __forceinline__ float batch_dist(const float* __restrict__ vec, uint32_t row_stride, uint32_t d, nrm_ptr_t nrm2,
                                            const float4* qlds, const uint32_t* ids_lds, uint32_t nf, int lane, BETWEEN&& between) {
    float result = INFINITY;
    uint32_t s0 = 0;
    if constexpr (METRIC >= KM_F16_FIRST) {  // half rows: the base metric's routine on binary16 rows (DistCosine's norms always beside them)
        (void)d;
        while (s0 < nf) {
            if (nf - s0 <= 16u) {
                result = group_dist<f16_base_metric(METRIC), 4, false, PIPE, _Float16, RS>(vec, row_stride, nrm2, qlds, ids_lds, s0, nf, lane, result, between, s0 == 0u);
                s0 += 16u;
            } else {
                result = group_dist<f16_base_metric(METRIC), 2, DEEP, PIPE, _Float16, RS>(vec, row_stride, nrm2, qlds, ids_lds, s0, nf, lane, result, between, s0 == 0u);
                s0 += 32u;
            }
        }
    } else if constexpr (METRIC >= KM_SIMD8_FIRST) {  // the crate's simdeez_f summation order: its own routine, 16 rows per round
        while (s0 < nf) {
            result = group_dist_simd8<METRIC>(vec, row_stride, d, nrm2 == nullptr, qlds, ids_lds, s0, nf, lane, result, between, s0 == 0u);
            s0 += 16u;
        }
    } else {
        (void)d;
        while (s0 < nf) {
            if (nf - s0 <= 16u) {
                result = group_dist<METRIC, 4, false, PIPE, float, RS>(vec, row_stride, nrm2, qlds, ids_lds, s0, nf, lane, result, between, s0 == 0u);
                s0 += 16u;
            } else {
                result = group_dist<METRIC, 2, DEEP, PIPE, float, RS>(vec, row_stride, nrm2, qlds, ids_lds, s0, nf, lane, result, between, s0 == 0u);
                s0 += 32u;
            }
        }
    }
    return result;
}
template <int METRIC>
__device__ __forceinline__ float batch_dist(const float* __restrict__ vec, uint32_t row_stride, uint32_t d, nrm_ptr_t nrm2,
                                            const float4* qlds, const uint32_t* ids_lds, uint32_t nf, int lane) {
    return batch_dist<METRIC>(vec, row_stride, d, nrm2, qlds, ids_lds, nf, lane, NoOverlap());
}

// ---------------------------------------------------------------------------------------
// Visited set (reference: hashbrown::HashMap<PointId, Arc<Point>>, src/hnsw.rs:955-956, :1016-1017),
// one per wavefront.  All three are EXACT (no false positives) and return true when `id` was not yet
// visited, marking it.
//   CELL16 : 8-cell buckets in LDS with 16-bit cells.  The id is passed through a bijection of
//            [0, 2^idbits); its top bits select the home bucket, and the cell stores
//            {valid, bucket displacement, remaining restbits} -- enough to identify the id, at
//            half the LDS of a table of full ids (LDS per wave is what bounds occupancy here).
//   CELL32 : same with full 32-bit ids (large indexes where restbits would not fit).
//   GLOBAL_BITMAP : one bit per point in a per-workgroup HBM slice; cannot overflow; last resort.
// A lane that cannot place its id within the displacement budget reports overflow; the query is
// then re-run from scratch with a larger representation (never a silent miss).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix_id(uint32_t id, uint32_t idbits) {
    const uint32_t mask = idbits >= 32 ? 0xFFFFFFFFu : ((1u << idbits) - 1u);
    const uint32_t sh = (idbits + 1u) >> 1;
    uint32_t h = (id * 0x9E3779B1u) & mask;
    h ^= h >> sh;
    h = (h * 0x85EBCA6Bu) & mask;
    h ^= h >> sh;
    return h;
}
// inverse of mix_id (each step is a bijection of [0, 2^idbits): odd multipliers have inverses mod 2^k,
// and x ^= x >> s is an involution once 2s >= idbits)
__device__ __forceinline__ uint32_t unmix_id(uint32_t h, uint32_t idbits) {
    const uint32_t mask = idbits >= 32 ? 0xFFFFFFFFu : ((1u << idbits) - 1u);
    const uint32_t sh = (idbits + 1u) >> 1;
    h ^= h >> sh;
    h = (h * 0xA5CB9243u) & mask;  // 0x85EBCA6B^-1 mod 2^32
    h ^= h >> sh;
    h = (h * 0x0E8B2F51u) & mask;  // 0x9E3779B1^-1 mod 2^32
    return h;
}
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
// The table is an array of BUCKETS of 8 sixteen-bit cells = one aligned 16-byte block, fetched with ONE ds_read_b128; cell c
// of a bucket is half c & 1 of word c >> 1.  cell = {valid, bdisp (2..6 bits), the id's remaining restbits bits}.  An id lives
// in its home bucket or, when that was full at its insertion, in one of the next ones (bdisp says how far).  Cells FILL FROM
// THE BOTTOM (an insertion always takes the first empty cell, by compare-and-swap on its word) and are never emptied, so
// "number of valid cells" locates the first empty one and a bucket that is not full holds every id whose home it is.
// does one of the 8 cells equal `tag`?  (packed 16-bit minimum of the four xor-ed words: a zero half <=> a match)
__device__ __forceinline__ bool bucket_has(const uint4 v, uint32_t tag) {
    const uint32_t tt = tag * 0x10001u;
    const uint32_t m = pk_min_u16(pk_min_u16(v.x ^ tt, v.y ^ tt), pk_min_u16(v.z ^ tt, v.w ^ tt));
    return (m & 0xFFFFu) == 0u || (m >> 16) == 0u;
}
__device__ __forceinline__ uint32_t bucket_fill(const uint4 v) {  // valid cells (= index of the first empty one)
    return (uint32_t)__popc(v.x & 0x80008000u) + (uint32_t)__popc(v.y & 0x80008000u) + (uint32_t)__popc(v.z & 0x80008000u) +
           (uint32_t)__popc(v.w & 0x80008000u);
}
struct Probe16 {   // what the test of an id leaves behind for its insertion
    uint4 v;           // the home bucket as it was read
    uint32_t bucket;
    uint32_t tag0;     // {valid, bdisp = 0, rest}
    uint32_t cnt;      // valid cells of v (when the id was not found in it)
};
// the displacement field takes the bits the id leaves free (at least 2, as the host guarantees; at most 6)
__device__ __forceinline__ uint32_t cell16_maxbd(uint32_t restbits) { return 1u << (15u - restbits < 6u ? 15u - restbits : 6u); }
// Test alone: 1 = visited already; 0 = not in its home bucket, which has room => not in the table at all (fresh);
// 2 = home bucket full and the id is not in it: it may live further on (visit_cell16 finds out).
__device__ __forceinline__ int cell16_test(const uint32_t* words, uint32_t restbits, uint32_t idbits, uint32_t id, Probe16& p) {
    const uint32_t h = mix_id(id, idbits);
    p.bucket = h >> restbits;  // home bucket
    p.tag0 = 0x8000u | (h & ((1u << restbits) - 1u));
    p.v = reinterpret_cast<const uint4*>(words)[p.bucket];
    p.cnt = 0u;
    if (bucket_has(p.v, p.tag0)) return 1;
    p.cnt = bucket_fill(p.v);
    return p.cnt == 8u ? 2 : 0;
}
// Insertion of an id KNOWN to be absent (cell16_test returned 0; other lanes may have filled cells since): 1 = done,
// 2 = no room within the displacement budget.
__device__ __forceinline__ int cell16_insert(uint32_t* words, uint32_t tbits, uint32_t restbits, Probe16& p) {
    const uint32_t bmask = (1u << (tbits - 3u)) - 1u;
    const uint32_t maxbd = cell16_maxbd(restbits);
    uint32_t bucket = p.bucket, bd = 0;
    uint4 v = p.v;
    {   // the usual case first, straight line: the bucket is as the test saw it (its fill count with it) and the word is still the same
        const uint32_t k = p.cnt >> 1;
        const uint32_t w32 = k == 0u ? v.x : k == 1u ? v.y : k == 2u ? v.z : v.w;
        const uint32_t old = atomicCAS(&words[bucket * 4u + k], w32, w32 | (p.tag0 << ((p.cnt & 1u) * 16u)));
        if (old == w32) return 1;
        if (k == 0u) v.x = old; else if (k == 1u) v.y = old; else if (k == 2u) v.z = old; else v.w = old;
    }
    for (;;) {
        const uint32_t cnt = bucket_fill(v);
        if (cnt == 8u) {  // filled up meanwhile: next bucket
            if (++bd == maxbd) return 2;
            bucket = (bucket + 1u) & bmask;
            v = reinterpret_cast<const uint4*>(words)[bucket];
            continue;
        }
        const uint32_t k = cnt >> 1;
        const uint32_t w32 = k == 0u ? v.x : k == 1u ? v.y : k == 2u ? v.z : v.w;
        const uint32_t tag = p.tag0 | (bd << restbits);
        const uint32_t old = atomicCAS(&words[bucket * 4u + k], w32, w32 | (tag << ((cnt & 1u) * 16u)));
        if (old == w32) return 1;
        // this word changed under us (another lane of the batch): carry on with what it holds now
        if (k == 0u) v.x = old; else if (k == 1u) v.y = old; else if (k == 2u) v.z = old; else v.w = old;
    }
}
// test + insertion in one go: returns 0 = already visited, 1 = newly marked, 2 = no room.
__device__ __forceinline__ int visit_cell16(uint32_t* words, uint32_t tbits, uint32_t idbits, uint32_t restbits, uint32_t id) {
    const uint32_t h = mix_id(id, idbits);
    const uint32_t bmask = (1u << (tbits - 3u)) - 1u;
    uint32_t bucket = h >> restbits;  // home bucket
    const uint32_t tag0 = 0x8000u | (h & ((1u << restbits) - 1u));
    const uint4* blocks = reinterpret_cast<const uint4*>(words);
    const uint32_t maxbd = cell16_maxbd(restbits);
    for (uint32_t bd = 0; bd < maxbd; ++bd, bucket = (bucket + 1u) & bmask) {
        const uint32_t tag = tag0 | (bd << restbits);
        uint4 v = blocks[bucket];
        for (;;) {
            if (bucket_has(v, tag)) return 0;
            const uint32_t cnt = bucket_fill(v);
            if (cnt == 8u) break;  // the bucket is full (and stays full: nothing is ever removed): next bucket
            const uint32_t k = cnt >> 1;
            const uint32_t w32 = k == 0u ? v.x : k == 1u ? v.y : k == 2u ? v.z : v.w;
            if (atomicCAS(&words[bucket * 4u + k], w32, w32 | (tag << ((cnt & 1u) * 16u))) == w32) return 1;
            v = blocks[bucket];  // this word changed under us (another lane of the batch): look at the bucket again
        }
    }
    return 2;
}
__device__ __forceinline__ int visit_cell32(uint32_t* tab, uint32_t tbits, uint32_t id) {
    const uint32_t mask = (1u << tbits) - 1u;
    uint32_t h = (id * 0x9E3779B1u) >> (32u - tbits);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint32_t old = atomicCAS(&tab[h], EMPTY_SLOT, id);
        if (old == EMPTY_SLOT) return 1;
        if (old == id) return 0;
        h = (h + 1u) & mask;
    }
    return 2;
}
__device__ __forceinline__ int visit_bitmap(uint32_t* bm, uint32_t id) {
    const uint32_t bit = 1u << (id & 31u);
    const uint32_t old = atomicOr(&bm[id >> 5], bit);
    return (old & bit) == 0u ? 1 : 0;
}

// ---------------------------------------------------------------------------------------
// Result set R (reference: return_points, a max-heap capped at ef, plus candidate_points).
// Kept as ONE array sorted ascending by distance, entry j in VGPR slot j/64 of lane j%64, with an
// EXPANDED flag: the candidates of the reference are exactly the not-yet-expanded members of R
// (an entry evicted from R can only terminate the loop when popped: SURVEY.md section 3.1).
// Insertion keeps arrival order among equal distances and reports whether an equal distance was
// already present (a tie: the reference's answer then depends on its heaps' internal order).
// ---------------------------------------------------------------------------------------
template <int S>
__device__ __forceinline__ bool r_insert(float (&rd)[S], uint32_t (&ri)[S], uint32_t& len, uint32_t ef, float xd,
                                         uint32_t xi, int lane) {
    uint32_t pos = 0;
    bool tie = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
        pos += popc64(__ballot(j < len && rd[s] <= xd));
        tie = tie || (__ballot(j < len && rd[s] == xd) != 0ull);
    }
#pragma unroll
    for (int s = S - 1; s >= 0; --s) {
        // entry j-1 -> j: DPP wave_shr:1 inside a slot, lane 63 of the previous slot into lane 0
        int od = __float_as_int(rd[s]), oi = (int)ri[s];
        if (s > 0) {
            od = __builtin_amdgcn_readlane(__float_as_int(rd[s - 1]), 63);
            oi = __builtin_amdgcn_readlane((int)ri[s - 1], 63);
        }
        const float pd = __int_as_float(__builtin_amdgcn_update_dpp(od, __float_as_int(rd[s]), 0x138, 0xf, 0xf, false));
        const uint32_t pi = (uint32_t)__builtin_amdgcn_update_dpp(oi, (int)ri[s], 0x138, 0xf, 0xf, false);
        const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
        if (j > pos) { rd[s] = pd; ri[s] = pi; }
        else if (j == pos) { rd[s] = xd; ri[s] = xi; }
    }
    len = len + 1 > ef ? ef : len + 1;  // the entry pushed past ef-1 is the evicted worst (src/hnsw.rs:1051-1053)
    return tie;
}
template <int S>
__device__ __forceinline__ float r_worst(const float (&rd)[S], uint32_t len) {
    float w = 0.f;
    const uint32_t j = len - 1;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if ((j >> 6) == (uint32_t)s) w = readlane_f(rd[s], (int)(j & 63));
    return w;
}
template <int S>
__device__ __forceinline__ float r_dist_at(const float (&rd)[S], uint32_t j) {
    float w = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if ((j >> 6) == (uint32_t)s) w = readlane_f(rd[s], (int)(j & 63u));
    return w;
}
// nearest not-yet-expanded member of R: returns its index, or -1
// lanes l of slot s whose entry 64 s + l exists (a scalar mask: a vote over `j < len && ...` costs three vector instructions more)
__device__ __forceinline__ unsigned long long slot_lanes(uint32_t len, int s) {
    const uint32_t lo = (uint32_t)s * 64u;
    return len >= lo + 64u ? ~0ull : (len > lo ? (1ull << (len - lo)) - 1ull : 0ull);
}
template <int S>
__device__ __forceinline__ int r_next(const uint32_t (&ri)[S], uint32_t len, int lane) {
    int j0 = -1;
    (void)lane;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const unsigned long long m = __ballot((ri[s] & EXPANDED) == 0u) & slot_lanes(len, s);
        if (j0 < 0 && m != 0ull) j0 = s * 64 + ctz64(m);
    }
    return j0;
}
template <int S>
__device__ __forceinline__ uint32_t r_id_flag_at(const uint32_t (&ri)[S], uint32_t j) {
    uint32_t v = 0;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if ((j >> 6) == (uint32_t)s) v = readlane_u(ri[s], (int)(j & 63u));
    return v;
}
template <int S>
__device__ __forceinline__ uint32_t r_id_at(const uint32_t (&ri)[S], int j) {
    uint32_t v = 0;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if ((j >> 6) == s) v = readlane_u(ri[s], j & 63);
    return v & ~EXPANDED;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}

// ---------------------------------------------------------------------------------------
// Literal emulation of Rust's std::collections::BinaryHeap (used when equal distances make the
// reference's answer depend on heap order; see the exact-replay section further down).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ hent_t hmake(float key, uint32_t id) { return ((hent_t)__float_as_uint(key) << 32) | id; }
__device__ __forceinline__ float hkey(hent_t e) { return __uint_as_float((uint32_t)(e >> 32)); }
__device__ __forceinline__ uint32_t hid(hent_t e) { return (uint32_t)e; }
// A heap array: entries [0, lds_cap) live in LDS (the top levels, touched by every operation), the rest in
// the workgroup's global scratch slice (L1-bypassing relaxed agent-scope accesses, served by the L2).
struct HeapMem {
    hent_t* lds;
    hent_t* glb;
    uint32_t lds_cap;
};
__device__ __forceinline__ hent_t hload(const HeapMem& H, uint32_t i) {
    if (i < H.lds_cap) return H.lds[i];
    return __hip_atomic_load(H.glb + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void hstore(const HeapMem& H, uint32_t i, hent_t v) {
    if (i < H.lds_cap) H.lds[i] = v;
    else __hip_atomic_store(H.glb + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// orders the stores of one heap operation before the loads of the next (single wave: LDS is in order,
// global stores are waited for)
__device__ __forceinline__ void hfence() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
// when every entry touched lives in LDS the hardware already keeps the order; only the compiler is fenced
__device__ __forceinline__ void hfence_for(const HeapMem& H, uint32_t max_index) {
    if (max_index < H.lds_cap) wave_lds_fence();
    else hfence();
}
__device__ __forceinline__ hent_t readlane_h(hent_t v, int lane) {
    const uint32_t lo = readlane_u((uint32_t)v, lane), hi = readlane_u((uint32_t)(v >> 32), lane);
    return ((hent_t)hi << 32) | lo;
}

__device__ __forceinline__ hent_t bperm_h(hent_t v, uint32_t src_lane) {  // every lane reads v of lane src_lane
    const int addr = (int)(src_lane << 2);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(v >> 32));
    return ((hent_t)hi << 32) | lo;
}

// BinaryHeap::push: data.push(item); sift_up(0, old_len): while pos > 0 { if elt <= data[parent] break; move parent down }
// PROBE: look at the parent alone first -- the usual push of a search does not pass it (one uniform read, no ancestor chain).
// The replay of a log pushes candidates, which are by construction nearer than most of the heap and climb: there the probe is
// a round trip in front of the one that loads the ancestors anyway (PROBE = false: straight to the chain).
template <bool PROBE = true>
__device__ __forceinline__ void heap_push(const HeapMem& H, uint32_t& len, hent_t item, int lane) {
    const uint32_t pos = len;
    len += 1;
    if constexpr (PROBE) {
        // common case first: the new entry does not even pass its parent (one uniform read)
        if (pos == 0u || hkey(item) <= hkey(hload(H, (pos - 1u) >> 1))) {
            if (lane == 0) hstore(H, pos, item);
            hfence_for(H, pos);
            return;
        }
    }
    // ancestor j of pos is ((pos+1) >> j) - 1
    const uint32_t p1 = lane < 32 ? (pos + 1u) >> lane : 0u;
    const bool anc = lane >= 1 && p1 >= 1u;
    const hent_t e = anc ? hload(H, p1 - 1u) : 0ull;
    const unsigned long long am = __ballot(anc);
    const unsigned long long stop = __ballot(anc && hkey(item) <= hkey(e));
    const int depth = (int)popc64(am);                       // ancestors are lanes 1..depth
    const int moved = stop != 0ull ? ctz64(stop) - 1 : depth;  // how many ancestors move down one step
    if (lane >= 1 && lane <= moved) hstore(H, ((pos + 1u) >> (lane - 1)) - 1u, e);
    if (lane == 0) hstore(H, ((pos + 1u) >> moved) - 1u, item);
    hfence_for(H, pos);
}

// BinaryHeap::push of SEVERAL items in a row -- the entries {-de, idc} of the lanes in `mask`, lowest lane first -- with ONE
// round trip to the heap's memory.  The new positions len .. len + m - 1 are consecutive, so the union of their root paths is
// small (at j levels above the new leaves it spans at most ((m - 1) >> j) + 2 nodes): for m <= 16 every node of it gets a lane
// of its own -- 16 lanes for the new leaves, then 9, 5, 3 and 2 per further level -- is loaded once, the m sift-ups run one
// after the other on those registers (uniform control flow: readlane, compare, one predicated move per level climbed), and what changed
// is stored back.  A sift-up by itself costs an LDS (or, below the heap's LDS part, an L2) round trip per push plus ~60
// instructions; here a push costs ~12 instructions per level it climbs.  Needs m <= 16 <= len (the new leaves are then nobody's
// ancestors), len + m < 2^19 (lanes for 20 levels) and all new leaves on ONE level of the tree (no power of two among the new
// 1-based positions: else the root is the j-th ancestor of one part and the (j+1)-th of the other and would sit in two lanes --
// found by the round's soak, one filtered query in 1 024; the lane algorithm is emulated and fuzzed against std's push in
// tests/test_heap_batch_push.py); the caller falls back to heap_push otherwise.
__device__ __forceinline__ uint32_t push_batch_lane0(uint32_t j) { return j == 0u ? 0u : j == 1u ? 16u : j == 2u ? 25u : j == 3u ? 30u : 33u + 2u * (j - 4u); }
__device__ __forceinline__ void heap_push_batch16(const HeapMem& H, uint32_t& len, unsigned long long mask, float de, uint32_t idc, int lane) {
    const uint32_t m = popc64(mask);
    const uint32_t p0 = len + 1u, pl = len + m;  // 1-based indices of the first and the last new position
    const uint32_t l = (uint32_t)lane;
    const uint32_t j = l < 16u ? 0u : l < 25u ? 1u : l < 30u ? 2u : l < 33u ? 3u : 4u + ((l - 33u) >> 1);
    const uint32_t node = (p0 >> j) + (l - push_batch_lane0(j));  // 1-based
    const bool valid = node >= 1u && node <= (pl >> j);
    hent_t v = valid && j >= 1u ? hload(H, node - 1u) : 0ull;
    uint32_t vlo = (uint32_t)v, vhi = (uint32_t)(v >> 32);
    unsigned long long touched = 0ull;
    uint32_t i = 0;
    for (unsigned long long mm = mask; mm != 0ull; mm &= mm - 1ull, ++i) {
        const int src = ctz64(mm);
        const uint32_t ikey = __float_as_uint(-readlane_f(de, src)), iid = readlane_u(idc, src);
        uint32_t cur = p0 + i, jc = 0u, lane_cur = i;
        for (;;) {
            const uint32_t par = cur >> 1;
            if (par == 0u) break;
            const uint32_t lane_par = push_batch_lane0(jc + 1u) + (par - (p0 >> (jc + 1u)));
            const uint32_t pkey = readlane_u(vhi, (int)lane_par);
            if (__uint_as_float(ikey) <= __uint_as_float(pkey)) break;  // sift_up: stops on <=
            const uint32_t pid = readlane_u(vlo, (int)lane_par);
            if (l == lane_cur) { vhi = pkey; vlo = pid; }
            touched |= 1ull << lane_cur;
            cur = par;
            jc += 1u;
            lane_cur = lane_par;
        }
        if (l == lane_cur) { vhi = ikey; vlo = iid; }
        touched |= 1ull << lane_cur;
    }
    if (((touched >> l) & 1ull) != 0ull) hstore(H, node - 1u, ((hent_t)vhi << 32) | vlo);
    len += m;
    hfence_for(H, len);
}
// any number of items: runs of <= 16 through heap_push_batch16, small or huge heaps one push at a time
__device__ __forceinline__ void heap_push_batch(const HeapMem& H, uint32_t& len, unsigned long long mask, float de, uint32_t idc, int lane) {
    while (mask != 0ull) {
        unsigned long long run = 0ull;
        for (int t = 0; t < 16 && mask != 0ull; ++t) {
            run |= mask & (~mask + 1ull);
            mask &= mask - 1ull;
        }
        // (a run that crosses a power of two -- its leaves then sit on two levels -- would meet the root twice, as the 8th ancestor
        // of one part and the 9th of the other: two lanes for one node; once per doubling of the heap, pushed one at a time)
        const uint32_t m = popc64(run);
        const bool one_level = __clz((int)(len + 1u)) == __clz((int)(len + m));
        if (len >= 64u && len + 16u < (1u << 19) && m >= 2u && one_level) {
            heap_push_batch16(H, len, run, de, idc, lane);
        } else {
            for (; run != 0ull; run &= run - 1ull) {
                const int src = ctz64(run);
                heap_push(H, len, hmake(-readlane_f(de, src), readlane_u(idc, src)), lane);
            }
        }
    }
}

// Greater-child path from the root of H[0..end): at a node with two children take the right one when
// data[left] <= data[right], with only a left child take it.  Returns the number m of path nodes below the
// root; lane j (1..m) receives the j-th node's index and entry, lane 0 index 0.
__device__ __forceinline__ int heap_chase(const HeapMem& H, uint32_t end, int lane, uint32_t& my_pos, hent_t& my_ent) {
    int m = 0;
    uint32_t p = 0;
    my_pos = 0;
    my_ent = 0ull;
    for (;;) {
        // lane L <= 62 holds the descendant of p at relative depth t = floor(log2(L+1)), offset L+1-2^t
        const uint32_t L1 = (uint32_t)lane + 1u;
        const uint32_t t = 31u - (uint32_t)__clz((int)L1);
        const unsigned long long idx64 = (((unsigned long long)p + 1ull) << t) - 1ull + (unsigned long long)(L1 - (1u << t));
        const bool valid = lane < 63 && idx64 < (unsigned long long)end;
        const uint32_t idx = (uint32_t)idx64;
        const hent_t e = valid ? hload(H, idx) : 0ull;
        const unsigned long long vm = __ballot(valid);
        int cur = 0;
        bool bottom = false;
        for (int step = 0; step < 5; ++step) {
            const int l = 2 * cur + 1, r = l + 1;
            if (((vm >> l) & 1ull) == 0ull) { bottom = true; break; }
            int nxt = l;
            if ((vm >> r) & 1ull) {
                const float kl = hkey(readlane_h(e, l)), kr = hkey(readlane_h(e, r));
                nxt = (kl <= kr) ? r : l;
            }
            m += 1;
            const hent_t en = readlane_h(e, nxt);
            const uint32_t ip = readlane_u(idx, nxt);
            if (lane == m) { my_pos = ip; my_ent = en; }
            cur = nxt;
        }
        if (bottom) break;
        p = readlane_u(idx, cur);
    }
    return m;
}

// BinaryHeap::pop: swap-remove the root with the last element, sift_down_to_bottom(0), then sift_up.
__device__ __forceinline__ hent_t heap_pop(const HeapMem& H, uint32_t& len, int lane) {
    const hent_t last = hload(H, len - 1u);
    len -= 1;
    if (len == 0u) return last;
    const hent_t root = hload(H, 0u);
    uint32_t my_pos;
    hent_t my_ent;
    const int m = heap_chase(H, len, lane, my_pos, my_ent);
    // the element re-inserted at the bottom climbs back while it is > the entry above it
    const unsigned long long le = __ballot(lane >= 1 && lane <= m && hkey(last) <= hkey(my_ent));
    const int jstar = le != 0ull ? 63 - __clzll((long long)le) : 0;
    const uint32_t prev_pos = (uint32_t)__shfl_up((int)my_pos, 1);
    if (lane >= 1 && lane <= jstar) hstore(H, prev_pos, my_ent);
    if (lane == jstar) hstore(H, my_pos, last);
    hfence_for(H, len);
    return root;
}

// BinaryHeap::push with the parents of the next positions prefetched: `pcache` holds, in lane j, the entry at index
// pbase + j where pbase = parent(len at prefetch time) -- one coalesced load issued before the distances of a
// batch are computed, so that the usual push (the new entry does not pass its parent) costs no memory round trip
// and leaves its store un-waited.  The caller drains the stores (hfence) before anything else reads the heap.
__device__ __forceinline__ hent_t heap_parent_cache(const HeapMem& H, uint32_t len, int lane, uint32_t& pbase) {
    pbase = len > 0u ? (len - 1u) >> 1 : 0u;
    return pbase + (uint32_t)lane < len ? hload(H, pbase + (uint32_t)lane) : 0ull;
}
__device__ __forceinline__ void heap_push_cached(const HeapMem& H, uint32_t& len, hent_t item, int lane, hent_t& pcache, uint32_t pbase) {
    const uint32_t pos = len;
    bool stays = pos == 0u;
    if (!stays) stays = hkey(item) <= hkey(readlane_h(pcache, (int)(((pos - 1u) >> 1) - pbase)));
    if (stays) {
        len += 1;
        if (lane == 0) hstore(H, pos, item);
        if (pos - pbase < 64u && (uint32_t)lane == pos - pbase) pcache = item;  // it may be the parent of a later push
        return;
    }
    hfence();  // the sift up reads ancestors: earlier un-waited stores first
    heap_push(H, len, item, lane);
    hfence();
    pcache = pbase + (uint32_t)lane < len ? hload(H, pbase + (uint32_t)lane) : 0ull;
}

// BinaryHeap::pop for heaps of < 32768 entries (3 rounds of 5 levels), without the serial readlane walk of
// heap_chase: in every round the 63 lanes hold the subtree below the node reached so far, each lane compares its
// two children (ds_bpermute), and the greater-child walk is five scalar bit tests.  Nothing is compacted: a path
// node that moves up simply stores its entry at its parent's index.
__device__ __forceinline__ hent_t heap_pop3(const HeapMem& H, uint32_t& len, int lane) {
    const hent_t last = hload(H, len - 1u);
    len -= 1;
    if (len == 0u) return last;
    const uint32_t end = len;
    // lane L holds the node with 1-based index L + 1 of the 63-node subtree rooted (lane 0) at the round's start
    const uint32_t L1 = (uint32_t)lane + 1u;
    const uint32_t t = 31u - (uint32_t)__clz((int)L1);
    const uint32_t off = L1 - (1u << t);
    uint32_t idx[3] = {0u, 0u, 0u};
    hent_t ent[3] = {0ull, 0ull, 0ull};
    unsigned long long pathm[3] = {0ull, 0ull, 0ull}, lem[3] = {0ull, 0ull, 0ull};
    hent_t root = 0ull;
    uint32_t p = 0;
    bool more = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (more) {
            const unsigned long long idx64 = (((unsigned long long)p + 1ull) << t) - 1ull + (unsigned long long)off;
            const bool valid = lane < 63 && idx64 < (unsigned long long)end;
            idx[r] = (uint32_t)idx64;
            ent[r] = valid ? hload(H, idx[r]) : 0ull;
            if (r == 0) root = readlane_h(ent[0], 0);
            const unsigned long long vm = __ballot(valid);
            const uint32_t cl = 2u * (uint32_t)lane + 1u;
            const float kl = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((cl & 63u) << 2), (int)(uint32_t)(ent[r] >> 32)));
            const float kr = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)(((cl + 1u) & 63u) << 2), (int)(uint32_t)(ent[r] >> 32)));
            const bool hl = lane <= 30 && ((vm >> cl) & 1ull) != 0ull;
            const bool pr = lane <= 30 && ((vm >> (cl + 1u)) & 1ull) != 0ull && kl <= kr;
            const unsigned long long hm = __ballot(hl), pm = __ballot(pr);
            uint32_t cur = 0;
            unsigned long long bits = 0ull;
            more = false;
            for (int step = 0; step < 5; ++step) {
                if (((hm >> cur) & 1ull) == 0ull) break;
                cur = 2u * cur + 1u + (uint32_t)((pm >> cur) & 1ull);
                bits |= 1ull << cur;
                if (step == 4) more = true;  // five levels walked and not at the bottom yet
            }
            pathm[r] = bits;
            lem[r] = __ballot(((bits >> lane) & 1ull) != 0ull && hkey(last) <= hkey(ent[r]));
            if (more) p = readlane_u(idx[r], (int)cur);
        }
    }
    // sift_up of `last` from the bottom of the path: it stops below the deepest path node it is <= to
    int rstar = -1;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (lem[r] != 0ull) rstar = r;
    if (rstar < 0) {
        if (lane == 0) hstore(H, 0u, last);
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (r <= rstar) {
                const int lstar = r == rstar ? 63 - __clzll((long long)lem[r]) : 63;
                if (((pathm[r] >> lane) & 1ull) != 0ull && lane <= lstar) hstore(H, (idx[r] - 1u) >> 1, ent[r]);
                if (r == rstar && lane == lstar) hstore(H, idx[r], last);
            }
        }
    }
    hfence_for(H, len);
    return root;
}

// ---- The same two operations for a heap that lies in LDS as a whole (every index touched is below the heap's lds_cap: the
// caller checks len, pushes to come included, against it).  The replay of a heap-operation log runs on these when the literal
// candidate heap fits: plain ds reads and writes -- no per-lane choice between LDS and the global slice, no wait for global
// stores --, one store per push, and a pop that walks only the rounds its length needs.
// BinaryHeap::push without the parent probe: lane j >= 1 reads ancestor j of the new position, the ancestors the item passes
// (it stops on <=) move down one step and the item takes the place of the last of them: ONE predicated store.
__device__ __forceinline__ void heap_push_lds(hent_t* h, uint32_t& len, hent_t item, int lane) {
    const uint32_t pos1 = len + 1u;  // 1-based index of the new position; its ancestor j is pos1 >> j
    len += 1;
    // (lane predicates are folded into the arithmetic: a mask held in scalar registers is a pair of them for the whole replay)
    const uint32_t p1 = pos1 >> (lane < 31 ? lane : 31);  // pos1 < 2^31: lanes >= 31 hold 0 = no ancestor; lane 0 holds pos1 itself
    const hent_t e = h[(p1 > 1u ? p1 : 1u) - 1u];        // (lane 0 and the lanes past the root read some entry: not looked at)
    // the first lane >= 1 that is past the root or holds an ancestor the item does not pass (lane 31 is past the root: stop != 0)
    const unsigned long long stop = __ballot(p1 == 0u || hkey(item) <= hkey(e)) & ~1ull;
    const uint32_t moved = (uint32_t)ctz64(stop) - 1u;  // ancestors 1..moved move down one step
    // lane j in 1..moved: ancestor j goes to the place of ancestor j - 1; lane moved + 1: the item goes to the place of ancestor `moved`
    const uint32_t jm1 = (uint32_t)lane - 1u;
    if (jm1 <= moved) h[(pos1 >> (jm1 & 31u)) - 1u] = jm1 == moved ? item : e;
    wave_lds_fence();
}

// BinaryHeap::pop (swap-remove the root with the last element, sift_down_to_bottom(0), sift_up) in rounds of five levels, as
// heap_pop3 -- the 63 lanes hold the subtree below the node reached so far, every lane compares its two children, the
// greater-child walk (right child on <=) is five scalar bit tests -- but as a loop that runs while the walk has not met the
// bottom: one round below 64 entries, two below 2 048, three below 65 536.  Nothing is kept from round to round: on a root path
// of a heap the keys never rise, so the path nodes that `last` is <= to -- those move up one step, `last` comes to lie on the
// deepest of them (sift_up stops there) -- are the path's top part, and each round stores its own moves; a round that holds a
// path node `last` is greater than is the last one.  (Keys are never NaN: the reference's order panics on one.)
// ROOT = false: the popped root is neither read out nor returned (a replayed pop throws it away).
template <bool ROOT>
__device__ __forceinline__ hent_t heap_pop_lds(hent_t* h, uint32_t& len, int lane) {
    const hent_t last = h[len - 1u];
    len -= 1;
    if (len == 0u) return last;
    const uint32_t end = len;
    // lane L holds the node with 1-based index L + 1 of the 63-node subtree rooted (lane 0) at the round's start
    const uint32_t L1 = (uint32_t)lane + 1u;
    const uint32_t t = 31u - (uint32_t)__clz((int)L1);
    // (lane predicates folded into the arithmetic, as in heap_push_lds: lane 63 holds no node -- its index lies past every heap --,
    // and the lanes of the round's last level, 31..62, have their children in the next round -- theirs lie past every heap)
    const uint32_t off = lane < 63 ? L1 - (1u << t) - 1u : 0x40000000u;
    const uint32_t coff = lane <= 30 ? 1u : 0x40000000u;
    const uint32_t cl = ((2u * (uint32_t)lane + 1u) & 63u) << 2;  // ds_bpermute address of the lane of the left child
    hent_t root = 0ull;
    uint32_t p1 = 1u;  // 1-based index of the round's root
    for (;;) {
        const uint32_t idx = (p1 << t) + off;  // (< 2^22 for heaps below 65 536 entries)
        const hent_t ent = h[idx < end ? idx : 0u];
        if constexpr (ROOT) {
            if (p1 == 1u) root = readlane_h(ent, 0);
        }
        const int khi = (int)(uint32_t)(ent >> 32);
        const float kl = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)cl, khi));
        const float kr = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)cl + 4, khi));
        // lanes 0..30 have their children in the round: left child at 2 idx + 1, right child at 2 idx + 2
        const uint32_t lc = 2u * idx + coff;
        const unsigned long long hm = __ballot(lc < end);
        const unsigned long long pm = __ballot(lc + 1u < end && kl <= kr);
        uint32_t cur = 0;
        unsigned long long bits = 0ull;
        bool more = false;
        for (int step = 0; step < 5; ++step) {
            if (((hm >> cur) & 1ull) == 0ull) break;
            cur = 2u * cur + 1u + (uint32_t)((pm >> cur) & 1ull);
            bits |= 1ull << cur;
            if (step == 4) more = true;  // five levels walked and not at the bottom yet
        }
        const bool on_path = ((bits >> lane) & 1ull) != 0ull;
        const unsigned long long up = __ballot(on_path && hkey(last) <= hkey(ent));
        if (on_path && ((up >> lane) & 1ull) != 0ull) h[(idx - 1u) >> 1] = ent;
        if (up == bits && more) {  // every path node of the round moved up: the next round starts at the deepest one
            p1 = readlane_u(idx, (int)cur) + 1u;
            wave_lds_fence();
            continue;
        }
        // `last` lies on the deepest path node it is <= to; none in this round: on the round's root (the deepest so far)
        const int lstar = up != 0ull ? 63 - __clzll((long long)up) : 0;
        if (lane == lstar) h[idx] = last;
        break;
    }
    wave_lds_fence();
    return root;
}

// sift_down_range(0, end) of into_sorted_vec: descend along the greater child, stop as soon as elt >= child
__device__ __forceinline__ void heap_sift_down_range(const HeapMem& H, uint32_t end, int lane) {
    const hent_t elt = hload(H, 0u);
    uint32_t my_pos;
    hent_t my_ent;
    const int m = heap_chase(H, end, lane, my_pos, my_ent);
    const unsigned long long ge = __ballot(lane >= 1 && lane <= m && hkey(elt) >= hkey(my_ent));
    const int nshift = ge != 0ull ? ctz64(ge) - 1 : m;
    const uint32_t prev_pos = (uint32_t)__shfl_up((int)my_pos, 1);
    if (lane >= 1 && lane <= nshift) hstore(H, prev_pos, my_ent);
    if (lane == nshift) hstore(H, my_pos, elt);
    hfence();
}

// return_points when ef + 1 <= 64 * NS: the whole heap sits in VGPRs (entry i in slot i/64 of lane i%64) and
// the sift loops run on readlane / predicated moves -- no memory latency on the hottest heap.
template <int NS>
struct RegHeap {
    hent_t s[NS];
    static constexpr uint32_t CAP = 64u * (uint32_t)NS;
    __device__ __forceinline__ hent_t get(uint32_t i) const {
        if constexpr (NS == 1) {
            return readlane_h(s[0], (int)i);
        } else {
            hent_t v = 0ull;
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if ((i >> 6) == (uint32_t)k) v = readlane_h(s[k], (int)(i & 63u));
            return v;
        }
    }
    __device__ __forceinline__ void set(uint32_t i, hent_t v, int lane) {
        if constexpr (NS == 1) {
            if (lane == (int)i) s[0] = v;
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if ((i >> 6) == (uint32_t)k && lane == (int)(i & 63u)) s[k] = v;
        }
    }
    __device__ __forceinline__ void push(uint32_t& len, hent_t item, int lane) {
        uint32_t pos = len;
        len += 1;
        while (pos > 0u) {
            const uint32_t parent = (pos - 1u) >> 1;
            const hent_t pe = get(parent);
            if (hkey(item) <= hkey(pe)) break;
            set(pos, pe, lane);
            pos = parent;
        }
        set(pos, item, lane);
    }
    // Greater-child path from the root of data[0..end) (sift_down_to_bottom / sift_down_range walk it): at a node
    // with two children the right one is taken when data[left] <= data[right], with only a left child that one.
    // Every node compares its two children at once (lane-parallel, ds_bpermute), the walk itself is scalar bit
    // tests.  pathm[k] = nodes of slot k on the path that have a child on it, chosen[k] = that child's entry
    // (valid in the lanes of pathm[k]), bottom = the last node of the path.
    static constexpr int KC = NS == 1 ? 1 : NS / 2;  // slots whose nodes can have children below CAP
    __device__ __forceinline__ void chase(uint32_t end, int lane, hent_t (&chosen)[KC], unsigned long long (&pathm)[KC],
                                          uint32_t& bottom) const {
        unsigned long long hasl[KC], prefr[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
            const uint32_t cl = 2u * i + 1u, cr = cl + 1u;
            hent_t L, R;
            if constexpr (NS == 1) {
                L = bperm_h(s[0], cl & 63u);
                R = bperm_h(s[0], cr & 63u);
            } else {  // children of slot k live in slots 2k (lower lanes) and 2k + 1
                const hent_t La = bperm_h(s[2 * k], cl & 63u), Lb = bperm_h(s[2 * k + 1], cl & 63u);
                const hent_t Ra = bperm_h(s[2 * k], cr & 63u), Rb = bperm_h(s[2 * k + 1], cr & 63u);
                L = lane < 32 ? La : Lb;
                R = lane < 31 ? Ra : Rb;
                if (2 * k + 2 < NS) {  // the right child of the slot's last node opens slot 2k + 2
                    const hent_t Rc = readlane_h(s[2 * k + 2 < NS ? 2 * k + 2 : 0], 0);
                    if (lane == 63) R = Rc;
                }
            }
            const bool hl = cl < end;
            const bool pr = cr < end && hkey(L) <= hkey(R);
            chosen[k] = pr ? R : L;
            hasl[k] = __ballot(hl);
            prefr[k] = __ballot(pr);
            pathm[k] = 0ull;
        }
        uint32_t pos = 0;
        for (;;) {
            const uint32_t k = pos >> 6, b = pos & 63u;
            if (k >= (uint32_t)KC) break;
            unsigned long long hm = 0ull, pm = 0ull;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (k == (uint32_t)kk) { hm = hasl[kk]; pm = prefr[kk]; }
            if (((hm >> b) & 1ull) == 0ull) break;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (k == (uint32_t)kk) pathm[kk] |= 1ull << b;
            pos = 2u * pos + 1u + (uint32_t)((pm >> b) & 1ull);
        }
        bottom = pos;
    }
    // the tail of BinaryHeap::pop once the last element has been taken off: `last` replaces the root of
    // data[0..end), sift_down_to_bottom(0), sift_up; returns the old root.  With path p_0 (root) .. p_m and
    // entries v_0 .. v_m: J = the deepest j >= 1 with last <= v_j (0 if none); p_k takes v_{k+1} for k < J, p_J
    // takes `last`, the nodes below keep their entries (moved up by the sift down, back down by the sift up).
    __device__ __forceinline__ hent_t pop_with_last(hent_t last, uint32_t end, int lane) {
        const hent_t root = get(0u);
        hent_t chosen[KC];
        unsigned long long pathm[KC];
        uint32_t bottom;
        chase(end, lane, chosen, pathm, bottom);
        int J = -1;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
            bool onpath = i == bottom;
            if (k < KC) onpath = onpath || ((pathm[k < KC ? k : 0] >> lane) & 1ull) != 0ull;
            const unsigned long long m = __ballot(onpath && i != 0u && hkey(last) <= hkey(s[k]));
            if (m != 0ull) J = 64 * k + 63 - __clzll((long long)m);
        }
        if (J >= 0) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
                if (((pathm[k] >> lane) & 1ull) != 0ull && i < (uint32_t)J) s[k] = chosen[k];
            }
        }
        set(J >= 0 ? (uint32_t)J : 0u, last, lane);
        return root;
    }
    __device__ __forceinline__ hent_t pop(uint32_t& len, int lane) {
        const hent_t last = get(len - 1u);
        len -= 1;
        if (len == 0u) return last;
        return pop_with_last(last, len, lane);
    }
    // push(item) immediately followed by pop() on a heap that already holds CAP entries (the reference's
    // "push, then pop when len > ef" with ef == CAP): the would-be entry CAP is never materialised.  The
    // new item climbs from the virtual leaf CAP; whatever ends up in that leaf is the `last` of the pop.
    __device__ __forceinline__ void push_then_pop_full(hent_t item, int lane) {
        uint32_t cnt = 0;  // ancestors the item climbs past: a_j = ((CAP + 1) >> j) - 1
        for (uint32_t j = 1; ((CAP + 1u) >> j) >= 1u; ++j) {
            if (hkey(item) <= hkey(get(((CAP + 1u) >> j) - 1u))) break;
            cnt = j;
        }
        hent_t last = item;
        if (cnt > 0u) {
            last = get(((CAP + 1u) >> 1) - 1u);
            for (uint32_t j = 1; j < cnt; ++j) set(((CAP + 1u) >> j) - 1u, get(((CAP + 1u) >> (j + 1u)) - 1u), lane);
            set(((CAP + 1u) >> cnt) - 1u, item, lane);
        }
        (void)pop_with_last(last, CAP, lane);
    }
    // sift_down_range(0, end) of into_sorted_vec: same path, the root's entry stops above the first p_j it is >= to
    __device__ __forceinline__ void sift_down_range(uint32_t end, int lane) {
        const hent_t elt = get(0u);
        hent_t chosen[KC];
        unsigned long long pathm[KC];
        uint32_t bottom;
        chase(end, lane, chosen, pathm, bottom);
        int F = -1;
#pragma unroll
        for (int k = NS - 1; k >= 0; --k) {
            const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
            bool onpath = i == bottom;
            if (k < KC) onpath = onpath || ((pathm[k < KC ? k : 0] >> lane) & 1ull) != 0ull;
            const unsigned long long m = __ballot(onpath && i != 0u && hkey(elt) >= hkey(s[k]));
            if (m != 0ull) F = 64 * k + (int)ctz64(m);
        }
        const uint32_t dest = F >= 0 ? ((uint32_t)F - 1u) >> 1 : bottom;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
            if (((pathm[k] >> lane) & 1ull) != 0ull && i < dest) s[k] = chosen[k];
        }
        set(dest, elt, lane);
    }
};


// Greedy descent through the upper layers: ONE scan of the pivot's list per layer, the pivot moves only to a
// strictly nearer neighbour and the first index wins ties (src/hnsw.rs:1506-1529).  Returns the entry point of
// the lowest layer and its distance to the query.
template <int METRIC>
__device__ __forceinline__ void greedy_descent(const DeviceIndexView& ix, nrm_ptr_t nrm2, float4* tile, uint32_t* ids_lds, int lane,
                                               uint32_t& pivot, float& dcur, uint32_t& n_dist, uint32_t& n_expand, uint32_t& n_ids) {
    pivot = ix.entry;
    if (lane == 0) ids_lds[0] = pivot;
    __syncthreads();
    dcur = readlane_f(batch_dist<METRIC>(ix.vec, ix.row_stride, ix.d, nrm2, tile, ids_lds, 1u, lane), 0);
    n_dist += 1;
    for (int layer = (int)ix.entry_level; layer >= 1; --layer) {
        uint32_t b = 0, e = 0;
        if ((uint32_t)layer <= ix.n_up_layers) {
            const uint32_t* ptr = ix.up_ptr + (size_t)(layer - 1) * ((size_t)ix.n + 1);
            b = ptr[pivot];
            e = ptr[pivot + 1];
        }
        n_expand += 1;
        n_ids += e - b;
        float best = INFINITY;
        uint32_t best_id = pivot;
        for (uint32_t base = b; base < e; base += 64) {
            const uint32_t j = base + (uint32_t)lane;
            const bool valid = j < e;
            const uint32_t id = valid ? ix.up_ids[j] : 0u;
            const uint32_t nf = e - base < 64u ? e - base : 64u;
            wave_lds_fence();
            if (valid) ids_lds[lane] = id;
            wave_lds_fence();
            const float dl = batch_dist<METRIC>(ix.vec, ix.row_stride, ix.d, nrm2, tile, ids_lds, nf, lane);  // INF in lanes >= nf
            n_dist += nf;
            const float m = readlane_f(wave_min(dl), 0);
            const unsigned long long eq = __ballot(valid && dl == m);
            if (eq != 0ull && m < best) {  // strict '<': the first index wins ties (:1519)
                best = m;
                best_id = readlane_u(id, ctz64(eq));
            }
        }
        if (best < dcur) {  // pivot replaced once per layer, only if strictly better (:1519-1528)
            dcur = best;
            pivot = best_id;
        }
    }
}

// The first kernel of every search call, one wavefront per query:
//   * the caller's row (d floats, any alignment; device memory or pinned host memory read across PCIe: the host-buffer entry
//     points stage nothing on the device) is zero padded to the row stride -- into the LDS tile and into qpad[], where the
//     search kernel stages it from;
//   * the greedy descent through the upper layers (src/hnsw.rs:1506-1529) runs HERE, with the exact arithmetic of the search
//     (the same batch_dist): the entry point of the lowest layer, its distance and the work counters go to pre[q], and the
//     search kernels start from them.  The descent is ~4 % of a query's instructions; out of the search kernel it runs at six
//     waves per SIMD instead of four next to a visited table, and its result doubles as the scheduling key: how long a search
//     runs is predicted by the distance from the query to its layer-0 entry point (rank correlation ~0.75 with the number of
//     expansions), and a batch whose long searches start first ends ~15 % earlier than one in input order.  (Rounds 2-3 ran a
//     separate ESTIMATE of this distance with tree-reduced sums and descended again, exactly, inside the search kernel.)
//   * workgroup 0 also zeroes the call's counters (what a memset node between the kernels used to do).
template <int METRIC>
__global__ __launch_bounds__(64, HNSW_LB_DESCEND) void hnsw_descend_kernel(DeviceIndexView ix, DescendArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float4* tile = reinterpret_cast<float4*>(lds_raw);
    uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes);
    const int lane = (int)threadIdx.x;
    if (blockIdx.x == 0 && a.ctrl != nullptr && (uint32_t)lane < a.ctrl_words) a.ctrl[lane] = 0u;
    const uint32_t row_stride = ix.row_stride, d = ix.d;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {  // every descent costs about the same: static split
        const float* __restrict__ src = a.src + (size_t)q * d;
        float* tf = reinterpret_cast<float*>(tile);
        for (uint32_t c = (uint32_t)lane; c < row_stride; c += 64) tf[c] = c < d ? src[c] : 0.f;
        __syncthreads();
        float4* dst = reinterpret_cast<float4*>(a.qpad + (size_t)q * row_stride);
        for (uint32_t i = (uint32_t)lane; i < (row_stride >> 2); i += 64) dst[i] = tile[i];
        finish_staged_query<METRIC>(tile, row_stride, lane, d);
        uint32_t pivot, n_dist = 0, n_expand = 0, n_ids = 0;
        float dcur;
        greedy_descent<METRIC>(ix, (nrm_ptr_t)a.nrm2, tile, ids_lds, lane, pivot, dcur, n_dist, n_expand, n_ids);
        if (lane == 0) a.pre[q] = PreDescent{pivot, __float_as_uint(dcur), n_dist, n_expand};  // (n_ids == n_dist - 1)
        __syncthreads();  // the tile is rewritten by the next query
    }
}

// The same kernel with TWO queries per wavefront (lanes 0-31 / 32-63), for indexes whose lists above the search layer hold at most
// 16 ids (max_nb_connection <= 16: every BASELINE config but none is assumed -- the host checks the lists it uploaded).  The descent
// is bound by VALU issue like the search (profiles/r06_sift1m_rocprofv3_summary.txt: 1 488 VALU instructions per query, 4 cycles
// each, ten queries per SIMD = 28 of the kernel's 33 us), and what it issues is the reference's left-to-right sum: 128 dependent
// adds per list however few rows the list has.  With two lanes per row the 16 + 16 rows of two queries' lists share one chain
// (group_dist<2> with a per-lane query tile: rows 0-15 against the first query, 16-31 against the second), which halves the
// instructions per query.  Same arithmetic, same rule (one scan per layer, strictly nearer, first index wins): both queries walk the
// same number of layers, so the loop is wave-uniform.  A half with no list at a layer, and the slots behind a short list, re-read the
// half's pivot row (in L2 since the previous layer) and are masked out of the minimum.
template <int METRIC>
__global__ __launch_bounds__(64, HNSW_LB_DESCEND) void hnsw_descend_pair_kernel(DeviceIndexView ix, DescendArgs a) {
    if constexpr (METRIC < KM_SIMD8_FIRST) {
        extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
        const int lane = (int)threadIdx.x;
        const uint32_t half = (uint32_t)lane >> 5, hl = (uint32_t)lane & 31u;
        float4* tile = reinterpret_cast<float4*>(lds_raw + (size_t)half * a.tile_bytes);  // this half's query
        uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + 2u * (size_t)a.tile_bytes);
        if (blockIdx.x == 0 && a.ctrl != nullptr && (uint32_t)lane < a.ctrl_words) a.ctrl[lane] = 0u;
        const uint32_t row_stride = ix.row_stride, d = ix.d, nchunk = row_stride >> 2;
        const nrm_ptr_t nrm2 = (nrm_ptr_t)a.nrm2;
        const uint32_t npair = (a.nq + 1u) >> 1;
        for (uint32_t p = blockIdx.x; p < npair; p += gridDim.x) {
            const uint32_t q = 2u * p + half < a.nq ? 2u * p + half : 2u * p;  // an odd count: the last wave runs its one query twice
            const bool mine = 2u * p + half < a.nq;
            // (the entry point's list at the top layer does not depend on the query: its bounds and ids are requested first and
            // arrive with the query's row)
            uint32_t pivot = ix.entry;
            uint32_t pb = 0, pe = 0;
            const int top = (int)ix.entry_level;
            if (top >= 1 && (uint32_t)top <= ix.n_up_layers) {
                const uint32_t* ptr = ix.up_ptr + (size_t)(top - 1) * ((size_t)ix.n + 1);
                pb = ptr[pivot];
                pe = ptr[pivot + 1];
            }
            const uint32_t id_next = hl < pe - pb ? ix.up_ids[pb + hl] : pivot;
            const float* __restrict__ src = a.src + (size_t)q * d;
            float* tf = reinterpret_cast<float*>(tile);
            for (uint32_t c = hl; c < row_stride; c += 32) tf[c] = c < d ? src[c] : 0.f;
            __syncthreads();
            float4* dst = reinterpret_cast<float4*>(a.qpad + (size_t)q * row_stride);
            for (uint32_t i = hl; i < nchunk; i += 32) dst[i] = tile[i];
            if constexpr (METRIC == DIST_COSINE) {  // finish_staged_query, per half
                double s1 = 0.;
                for (uint32_t c = 0; c < nchunk; ++c) {
                    const float4 v = tile[c];
                    s1 = s1 + (double)(v.x * v.x); s1 = s1 + (double)(v.y * v.y); s1 = s1 + (double)(v.z * v.z); s1 = s1 + (double)(v.w * v.w);
                }
                if (hl == 0u) *reinterpret_cast<double*>(tile + nchunk) = s1;
            }
            // row slot r = lane / 2 of group_dist<2>: slots 0-15 belong to the first query, 16-31 to the second; the distance to
            // slot r comes back in lane r
            const uint32_t rhalf = ((uint32_t)lane >> 4) & 1u, rj = (uint32_t)lane & 15u;  // (of lanes 0-31: the slot this lane reports)
            // Two round trips per layer instead of three, and one chain less per query:
            //   * the bounds [pb, pe) of the pivot's list are known when a layer starts -- while the rows of layer L are in flight
            //     the lanes that hold its candidates (and one lane for the pivot itself) fetch THEIR bounds at layer L - 1, and
            //     whichever of them the rule picks hands its pair over by readlane;
            //   * the slots behind a short list hold the pivot's row anyway, so with <= 15 ids in the entry point's top list (the
            //     usual case: the top layer holds a handful of points) slot 15 of the first batch IS the distance to the entry
            //     point (:1506-1510) -- no batch of its own.
            float dcur = INFINITY;
            bool have_dcur = false;  // (wave-uniform: both halves start at the entry point)
            if (top < 1 || readlane_u(pe - pb, 0) > 15u) {
                if ((uint32_t)lane < 32u) ids_lds[lane] = pivot;
                __syncthreads();
                const float res0 = group_dist<METRIC, 2>(ix.vec, row_stride, nrm2, tile, ids_lds, 0u, 32u, lane, INFINITY, NoOverlap(), false);
                // (both lanes are read BEFORE the choice: inside an arm of `half != 0 ? .. : ..` the compiler knows this lane's own
                // value -- INFINITY in lanes >= 32 -- and folds the other lane's into it)
                const float e_a = readlane_f(res0, 0), e_b = readlane_f(res0, 16);
                dcur = half != 0u ? e_b : e_a;
                have_dcur = true;
            }
            __syncthreads();
            uint32_t n_dist = 1, n_expand = 0;
            for (int layer = top; layer >= 1; --layer) {
                const uint32_t len = pe - pb;  // <= 16
                n_expand += 1;
                n_dist += len;
                const uint32_t id = layer == top ? id_next : (hl < len ? ix.up_ids[pb + hl] : pivot);  // (hl == 16: the pivot, for the bounds below)
                wave_lds_fence();
                if (hl < 16u) ids_lds[16u * half + hl] = id;
                wave_lds_fence();
                uint32_t cb = 0, ce = 0;  // lanes hl <= 16: the list bounds of `id` one layer down
                if (layer >= 2 && (uint32_t)(layer - 1) <= ix.n_up_layers && hl <= 16u) {
                    const uint32_t* nptr = ix.up_ptr + (size_t)(layer - 2) * ((size_t)ix.n + 1);
                    cb = nptr[id];
                    ce = nptr[id + 1];
                }
                const float res = group_dist<METRIC, 2>(ix.vec, row_stride, nrm2, tile, ids_lds, 0u, 32u, lane, INFINITY, NoOverlap(), false);
                if (!have_dcur) {  // slot 15 / 31: the entry point's own row
                    const float e_a = readlane_f(res, 15), e_b = readlane_f(res, 31);
                    dcur = half != 0u ? e_b : e_a;
                    have_dcur = true;
                }
                // lanes 0-31 report slot `lane`: the minimum of each 16-slot half over its list, then the first slot that has it
                const uint32_t len_a = readlane_u(len, 0), len_b = readlane_u(len, 32);
                const bool rvalid = (uint32_t)lane < 32u && rj < (rhalf != 0u ? len_b : len_a);
                const float dl = rvalid ? res : INFINITY;
                float m = dl;
                m = fminf(m, __shfl_xor(m, 1));
                m = fminf(m, __shfl_xor(m, 2));
                m = fminf(m, __shfl_xor(m, 4));
                m = fminf(m, __shfl_xor(m, 8));
                const unsigned long long eq = __ballot(rvalid && dl == m);
                const uint32_t eq_a = (uint32_t)eq & 0xFFFFu, eq_b = ((uint32_t)eq >> 16) & 0xFFFFu;
                const uint32_t rid = ids_lds[(uint32_t)lane & 31u];
                // the rule, once per half on wave-uniform values: the pivot is replaced once per layer, only by a strictly nearer
                // neighbour, the first index among equals (:1519-1528)
                const float m_a = readlane_f(m, 0), m_b = readlane_f(m, 16);
                const float dc_a = readlane_f(dcur, 0), dc_b = readlane_f(dcur, 32);
                const bool mv_a = eq_a != 0u && m_a < dc_a, mv_b = eq_b != 0u && m_b < dc_b;
                const int sl_a = mv_a ? (int)ctz64(eq_a) : 16, sl_b = mv_b ? (int)ctz64(eq_b) : 16;  // whose bounds: a candidate's, or the pivot's (slot 16)
                const uint32_t id_a = readlane_u(rid, sl_a & 15), id_b = readlane_u(rid, 16 + (sl_b & 15));
                const uint32_t nb_a = readlane_u(cb, sl_a), ne_a = readlane_u(ce, sl_a);
                const uint32_t nb_b = readlane_u(cb, 32 + sl_b), ne_b = readlane_u(ce, 32 + sl_b);
                if (half != 0u ? mv_b : mv_a) {
                    dcur = half != 0u ? m_b : m_a;
                    pivot = half != 0u ? id_b : id_a;
                }
                pb = half != 0u ? nb_b : nb_a;
                pe = half != 0u ? ne_b : ne_a;
            }
            if (hl == 0u && mine) a.pre[q] = PreDescent{pivot, __float_as_uint(dcur), n_dist, n_expand};  // (n_ids == n_dist - 1)
            __syncthreads();  // the tiles are rewritten by the next pair
        }
    }
}

#if HNSW_PART == 2
// order[] = 0 .. n-1 sorted by the descent's distance descending (distances are >= 0: their bit patterns order like the
// values; equal or near-equal keys in any order -- this only schedules work).  One workgroup, counting sort over the top 13
// bits of the pattern (8 exponent + 5 mantissa bits: 3 % bins, no pass for the range).  Up to 16 keys per thread live in
// registers -- every load in flight at once -- and the LDS atomic that counts a key also hands back its rank inside the bin,
// so the scatter needs no second round of atomics; larger batches loop.
__global__ __launch_bounds__(1024) void order_desc_kernel(const PreDescent* __restrict__ pre, uint32_t n, uint32_t* __restrict__ order) {
    constexpr uint32_t BINS = 8192, KPT = 16;
    __shared__ uint32_t hist[BINS];
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x;
    auto bin_of = [](uint32_t bits) -> uint32_t { return (BINS - 1u) - ((bits & 0x7FFFFFFFu) >> 18); };  // bin 0 = largest keys
    for (uint32_t i = tid; i < BINS; i += 1024) hist[i] = 0u;
    __syncthreads();
    const bool in_regs = n <= KPT * 1024u;
    uint32_t kb[KPT], kr[KPT];
    if (in_regs) {
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) {
            const uint32_t i = tid + 1024u * j;
            kb[j] = i < n ? pre[i].dcur_bits : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) {
            kb[j] = bin_of(kb[j]);
            kr[j] = tid + 1024u * j < n ? atomicAdd(&hist[kb[j]], 1u) : 0u;
        }
    } else {
        for (uint32_t i = tid; i < n; i += 1024) atomicAdd(&hist[bin_of(pre[i].dcur_bits)], 1u);
    }
    __syncthreads();
    // exclusive prefix over the bins: 8 per thread, wave scans, then the 16 wave totals
    uint32_t c[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = hist[8 * tid + j]; mine += c[j]; }
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if ((int)(tid & 63u) >= off) incl += t;
    }
    if ((tid & 63u) == 63u) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for (uint32_t w = 0; w < (tid >> 6); ++w) run += wsum[w];
#pragma unroll
    for (int j = 0; j < 8; ++j) { hist[8 * tid + j] = run; run += c[j]; }
    __syncthreads();
    if (in_regs) {
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) {
            const uint32_t i = tid + 1024u * j;
            if (i < n) order[hist[kb[j]] + kr[j]] = i;
        }
    } else {
        for (uint32_t i = tid; i < n; i += 1024) order[atomicAdd(&hist[bin_of(pre[i].dcur_bits)], 1u)] = i;
    }
}
#endif

// ---------------------------------------------------------------------------------------
// The search kernel: one wavefront (= one 64-thread workgroup) per query, persistent grid pulling
// query indices from a global counter.
//
// Ties.  The reference keeps two BinaryHeaps; with EQUAL f32 distances some of its decisions depend on the heaps'
// internal order (Ord compares distances only, src/hnsw.rs:283-297).  The sorted array below takes the reference's
// decisions for as long as they are decided by VALUES alone, and a strict launch watches for the three places where
// they are not:
//   (A) candidate_points.pop() (:971) with two equal nearest candidates -- the next unexpanded entry has an equal,
//       still unexpanded successor;
//   (B) the same pop when an unexpanded entry that was evicted from return_points while an equal entry stayed behind
//       (a "ghost": still in the reference's candidate heap, at distance == the current farthest) is among the
//       nearest candidates -- including at the end, when the array has no candidate left but the reference would
//       still pop and expand the ghost (its distance is not > the farthest, :981);
//   (C) at the end: two equal distances inside the first k answers (or across their end), or an answer among the
//       first k that survived an eviction between equal farthest entries (:1051-1053 pops one of them, which one is
//       the heap's choice) -- into_sorted_vec (:1544) and that pop decide ids, not values.
// An evicted entry e is otherwise irrelevant: dist(e) >= the farthest at its eviction >= the farthest now, so it can
// only end the loop when popped, exactly when the array runs out of candidates.
// Every strict query logs its heap operations (one 8-byte store per accepted neighbour and per expansion).  The literal
// candidate heap is LAZY: it exists only as that log until a pop meets (A)/(B); then the heap is brought up to date from
// the part of the log it has not seen yet, THIS pop is taken from it, and the search carries on with the sorted array
// (return_points steers the search through its largest value and its length only; the array's EXPANDED flags and the ghost
// count are kept in step with what the heap popped).  The heap operations between the last such pop and the end of the
// search are never performed.  At (C) the literal return_points is rebuilt from the log and sorted the reference's way.
// Equal distances that never reach one of the three places cost nothing.
//
// status per query: 0 ok; 1 visited-set overflow (re-run bigger); 2 ok, but one of (A)-(C) was met and not resolved
// (lean launches, or a strict query whose log / candidate scratch overflowed: the host re-runs it with
// hnsw_search_exact_kernel); 3 ok, resolved with the literal heaps.
// ---------------------------------------------------------------------------------------
constexpr hent_t LOG_EXPAND = 0xFFFFFFFFFFFFFFFFull;  // log marker: candidate_points.pop() (key bits = NaN: never a distance)


// the explicit kernel arguments of hnsw_search_kernel as they lie in the kernarg segment: the out-of-line parts of the kernel
// read what they need from there (scalar loads at the point of use) instead of having it handed down through registers
typedef __attribute__((address_space(4))) const struct SearchKernargs* kernargs_t;
// (the kernarg-segment intrinsic is only meaningful inside the kernel itself -- in a called function it yields null -- so the
// kernel hands its own pointer down; it arrives in vector registers and is made wave-uniform again for scalar loads)
__device__ __forceinline__ kernargs_t uniform_kernargs(const void* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned long long u = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    return (kernargs_t)u;
}
struct SearchKernargs {  // the explicit kernel arguments of hnsw_search_kernel, as they lie in the kernarg segment
    DeviceIndexView ix;
    SearchArgs a;
};
static_assert(offsetof(SearchKernargs, a) == ((sizeof(DeviceIndexView) + alignof(SearchArgs) - 1) / alignof(SearchArgs)) * alignof(SearchArgs),
              "kernarg layout: the second argument follows the first at its own alignment");

// ---- the cold parts of a strict search, as real (non-inlined) device functions: their registers are then allocated on
// their own, and the expansion loop of the strict kernel keeps the register budget of the lean one.
struct LiteralPop {
    hent_t ce;          // the popped entry {-dist, id}
    uint32_t lenC;      // length of the literal candidate heap afterwards
    int rc;             // 0: popped; 1: the heap is empty; 2: candidate scratch exhausted
#if HNSW_PHASE_TIMING == 2
    uint32_t n_ops, t_pops;  // profiling build 2: heap operations performed, clock64 ticks inside the replayed pops
#endif
};
// Brings the literal candidate_points up to date from the entries [from, to) of the heap-operation log (a LOG_EXPAND marker
// = one pop, anything else = push of {-dist, id}; entry 0 of every log is the entry point, :958-963), then pops once (:971).
template <int TABLE>
__device__ HNSW_COLD LiteralPop literal_candidate_pop(const void* kargs, uint32_t from, uint32_t to, uint32_t lenC) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const kernargs_t ka = uniform_kernargs(kargs);
    const int lane = (int)threadIdx.x;
    from = (uint32_t)__builtin_amdgcn_readfirstlane((int)from);
    to = (uint32_t)__builtin_amdgcn_readfirstlane((int)to);
    lenC = (uint32_t)__builtin_amdgcn_readfirstlane((int)lenC);
    // LDS behind the visited table: merge_list's scatter buffer, then the top of this heap
    const uint32_t cells = 1u << ka->a.tbits;
    const uint32_t table_bytes = (TABLE == TABLE_LDS_CELL16 ? cells >> 1 : cells) * 4u;
    hent_t* heap_lds = reinterpret_cast<hent_t*>(lds_raw + ka->a.tile_bytes + IDS_BYTES + table_bytes) + ka->a.merge_entries;
    const uint32_t cand_cap = ka->a.cand_cap;
    const hent_t* oplog = ka->a.oplog + (size_t)blockIdx.x * ka->a.oplog_cap;
    const HeapMem Cq{heap_lds, ka->a.cand_scratch + (size_t)blockIdx.x * cand_cap, ka->a.cand_lds};
    LiteralPop out{0ull, lenC, 2};
#if HNSW_PHASE_TIMING == 2
    out.n_ops = to - from + 1u;
    out.t_pops = 0;
#endif
    // a chunk of the log (<= 64 entries) whose pushes leave the heap within its LDS part is replayed with the LDS-only
    // operations (the heap only grows by pushes: no index of the chunk then reaches the global slice); so is the final pop
    const auto lds_fits = [&](uint32_t len) { return len <= Cq.lds_cap && len <= cand_cap; };
    hfence();  // the log's stores have landed (entry 0 is the entry point's push, :958-963)
    bool ok = true;
    for (uint32_t base = from; base < to && ok; base += 64) {
        const uint32_t li = base + (uint32_t)lane;
        const hent_t mine = li < to ? __hip_atomic_load(oplog + li, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        const uint32_t cntb = to - base < 64u ? to - base : 64u;
        // the chunk's entries classified once, all lanes at a time: a bit per marker (= pop), and every push's {-key, id} ready
        // in its lane -- the serial part below tests a bit and reads a lane
        const unsigned long long markers = ~__ballot(mine != LOG_EXPAND);  // (lanes past the chunk's end hold 0: no marker)
        const uint32_t pushes = cntb - popc64(markers);
        const hent_t item = hmake(-hkey(mine), hid(mine));
        if (lds_fits(lenC + pushes)) {
            for (uint32_t t = 0; t < cntb; ++t) {
                if (((markers >> t) & 1ull) != 0ull) {
#if HNSW_PHASE_TIMING == 2
                    const unsigned long long tp0 = clock64();
#endif
                    (void)heap_pop_lds<false>(Cq.lds, lenC, lane);
#if HNSW_PHASE_TIMING == 2
                    out.t_pops += (uint32_t)(clock64() - tp0);
#endif
                } else {
                    heap_push_lds(Cq.lds, lenC, readlane_h(item, (int)t), lane);
                }
            }
        } else {
            for (uint32_t t = 0; t < cntb; ++t) {
                if (((markers >> t) & 1ull) != 0ull) {
#if HNSW_PHASE_TIMING == 2
                    const unsigned long long tp0 = clock64();
#endif
                    (void)heap_pop3(Cq, lenC, lane);
#if HNSW_PHASE_TIMING == 2
                    out.t_pops += (uint32_t)(clock64() - tp0);
#endif
                } else {
                    if (lenC >= cand_cap) { ok = false; break; }
                    heap_push<false>(Cq, lenC, readlane_h(item, (int)t), lane);
                }
            }
        }
    }

    if (ok) {
        if (lenC == 0u) {
            out.rc = 1;
        } else {
            out.ce = lds_fits(lenC) ? heap_pop_lds<true>(Cq.lds, lenC, lane) : heap_pop3(Cq, lenC, lane);
            out.rc = 0;
        }
    }
    out.lenC = lenC;
    return out;
}

// (C): return_points rebuilt literally from the whole log (pushes in order, "pop when len > ef", :1038, :1051-1053), then
// into_sorted_vec (:1544).  Entry j of the answer comes back in slot j / 64 of lane j % 64.
template <int S>
struct SortedR {
    hent_t s[S];
    uint32_t len;
};
template <int S>
__device__ HNSW_COLD SortedR<S> literal_return_points(const void* kargs, uint32_t log_len) {
    const kernargs_t ka = uniform_kernargs(kargs);
    const int lane = (int)threadIdx.x;
    log_len = (uint32_t)__builtin_amdgcn_readfirstlane((int)log_len);
    const uint32_t ef = ka->a.ef;
    const hent_t* oplog = ka->a.oplog + (size_t)blockIdx.x * ka->a.oplog_cap;
    hfence();
    RegHeap<S> RR;
#pragma unroll
    for (int s = 0; s < S; ++s) RR.s[s] = 0ull;
    uint32_t lenR = 0;                                                     // (entry 0 of the log: the entry point, :964-967)
    for (uint32_t base = 0; base < log_len; base += 64) {
        const uint32_t li = base + (uint32_t)lane;
        const hent_t mine = li < log_len ? __hip_atomic_load(oplog + li, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        const uint32_t cntb = log_len - base < 64u ? log_len - base : 64u;
        for (uint32_t t = 0; t < cntb; ++t) {
            const hent_t e = readlane_h(mine, (int)t);
            if (e == LOG_EXPAND) continue;
            if (lenR == RegHeap<S>::CAP) {                                 // :1038, :1051-1053
                RR.push_then_pop_full(e, lane);
            } else {
                RR.push(lenR, e, lane);
                if (lenR > ef) (void)RR.pop(lenR, lane);
            }
        }
    }
    uint32_t end = lenR;                                                   // into_sorted_vec (:1544)
    while (end > 1u) {
        end -= 1;
        const hent_t r0 = RR.get(0u), re = RR.get(end);
        RR.set(0u, re, lane);
        RR.set(end, r0, lane);
        RR.sift_down_range(end, lane);
    }
    SortedR<S> out;
#pragma unroll
    for (int s = 0; s < S; ++s) out.s[s] = RR.s[s];
    out.len = lenR < ef ? lenR : ef;
    return out;
}


// ---- The end of a query, out of line.  What it needs from the kernel arguments -- the five output arrays, the per-query stats,
// origin ids, the 17 layer offsets, the retry / flag lists and their counters -- it reads from the kernarg segment itself
// (scalar loads where they are used), so none of that stays live in scalar registers across the expansion loop of the caller:
// with everything inlined the loop ran with ~90 spilled SGPRs and reloaded them lane by lane (v_readlane) at every use.
template <int S>
struct QueryEnd {
    float rd[S];
    uint32_t ri[S];
    uint32_t q, len, status, out_status, n_dist, n_expand, n_ids, t_start, flags;  // flags: 1 equal distances met, 2 literal pop, 4 HBM bitmap used
    uint32_t feedback;  // bit 0: the query moved to the HBM bitmap, bit 1: it visited more than half of what its table holds, bit 2: table launches
#if HNSW_PHASE_TIMING
    uint32_t ph[4], ph_miss;
#endif
};
// answer slots (SearchArgs: id_stride, dist_stride, count_stride)
__device__ __forceinline__ void put_id(uint64_t* base, uint32_t stride, size_t o, uint64_t v) {
    *reinterpret_cast<uint64_t*>(reinterpret_cast<unsigned char*>(base) + o * stride) = v;
}
__device__ __forceinline__ void put_dist(float* base, uint32_t stride, size_t o, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(base) + o * stride) = v;
}
// id and distance of one answer; 16-byte records (the FFI's Neighbour_api {usize id; f32 d; 4 bytes of padding}, distances 8 bytes
// behind the ids): ONE 16-byte store per lane -- the answers of a query are then 16 k contiguous bytes, a few full-width writes
// across PCIe when they go to host memory instead of 2 k partial ones
__device__ __forceinline__ void put_answer(uint64_t* ids, uint32_t id_stride, float* dists, uint32_t dist_stride, size_t o, uint64_t id, float d) {
    if (id_stride == 16u && dist_stride == 16u && reinterpret_cast<unsigned char*>(dists) == reinterpret_cast<unsigned char*>(ids) + 8) {
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(ids) + o * 16u) = make_uint4((uint32_t)id, (uint32_t)(id >> 32), __float_as_uint(d), 0u);
    } else {
        put_id(ids, id_stride, o, id);
        put_dist(dists, dist_stride, o, d);
    }
}
__device__ __forceinline__ void put_count(uint32_t* base, uint32_t stride, size_t q, uint32_t v) {
    *reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(base) + q * stride) = v;
}
template <int S>
__device__ __attribute__((noinline)) void finish_query(const void* kargs, QueryEnd<S> e) {
    const kernargs_t ka = uniform_kernargs(kargs);
    const int lane = (int)threadIdx.x;
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.q), len = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.len);
    uint32_t status = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.status);
    uint32_t out_status = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.out_status);
    const uint32_t feedback = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.feedback);
    const uint32_t k = ka->a.k;
    uint32_t* const counters = ka->a.overflow_count;
    if (out_status == 3u && status != 1u && lane == 0) atomicAdd(counters + 4, 1u);  // ctrl[5]: answered with the literal heaps (not: given up after a replay, searched again)
    if (status == 2u) {  // flagged: (A)-(C) met and not resolved in this launch
        uint32_t* const tie_list = ka->a.tie_list;
        if (tie_list != nullptr && lane == 0) tie_list[atomicAdd(counters + 3, 1u)] = q;
    }
    if (status != 0u) out_status = status;
    // ---- into_sorted_vec + truncate to min(knbn, ef, len) (:1544-1547, :1567-1578)
    if (status != 1u) {
        const uint32_t cnt = len < k ? len : k;
        uint64_t* const out_ids = ka->a.out_ids;
        float* const out_dists = ka->a.out_dists;
        uint8_t* const out_layer = ka->a.out_layer;
        int32_t* const out_rank = ka->a.out_rank;
        const uint64_t* const origin_id = ka->ix.origin_id;
        const uint32_t id_stride = ka->a.id_stride, dist_stride = ka->a.dist_stride;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
            if (j < k) {
                const size_t o = (size_t)q * k + j;
                if (j < cnt) {
                    const uint32_t flat = e.ri[s] & ~EXPANDED;
                    uint32_t l = 0;
                    while (l + 1 < NB_LAYER_MAX && flat >= ka->ix.layer_offset[l + 1]) ++l;
                    put_answer(out_ids, id_stride, out_dists, dist_stride, o, origin_id[flat], e.rd[s]);
                    if (out_layer) out_layer[o] = (uint8_t)l;
                    if (out_rank) out_rank[o] = (int32_t)(flat - ka->ix.layer_offset[l]);
                } else {
                    put_answer(out_ids, id_stride, out_dists, dist_stride, o, 0ull, 0.f);
                    if (out_layer) out_layer[o] = 0;
                    if (out_rank) out_rank[o] = 0;
                }
            }
        }
        if (lane == 0) put_count(ka->a.out_counts, ka->a.count_stride, q, cnt);
    } else if (lane == 0) {
        const uint32_t slot = atomicAdd(counters, 1u);
        ka->a.retry_out[slot] = q;
    }
    if (lane == 0 && (feedback & 4u) != 0u) {
        // feedback for the host's table sizing (ctrl[2], ctrl[3])
        if (feedback & 1u) atomicAdd(counters + 1, 1u);
        if (feedback & 2u) atomicAdd(counters + 2, 1u);
    }
    if (lane == 0) {
        uint32_t* st = ka->a.stats + (size_t)q * 8;
        st[0] = e.n_dist; st[1] = e.n_expand; st[2] = e.n_ids; st[3] = out_status;
        st[4] = e.t_start; st[5] = (uint32_t)wall_clock64(); st[6] = (e.flags & 4u) ? 1u : 0u;
        // flags (equal distances met / a literal pop) | what of st[0], st[1] ran in hnsw_descend_kernel: lists scanned << 8, n_dist << 16
        st[7] = (e.flags & 3u) | ((ka->a.pre[q].n_expand & 0xFFu) << 8) | (ka->a.pre[q].n_dist << 16);
#if HNSW_PHASE_TIMING
#if HNSW_PHASE_TIMING == 2
        st[7] = e.ph[0]; st[2] = e.ph[1]; st[6] = e.ph[3]; st[0] = 0u;       // profiling build 2: see tools/literal_profile.py (status stays)
#else
        st[7] = e.ph[0]; st[3] = e.ph[1]; st[2] = e.ph[2]; st[6] = e.ph[3];  // profiling build: overwrites status/n_ids/bitmap flag
        st[0] = e.ph_miss;                                                    // ... and n_dist
#endif
#endif
    }
}


// What the descent left for query q (hnsw_descend_kernel ran it before this launch): the entry point of the search layer, its
// distance, the descent's work counters.  Out of line like the rest of a query's start; strict launches also get entry 0 of
// the query's heap-operation log here -- the entry point, pushed on both heaps before the loop (src/hnsw.rs:958-967).
struct DescentOut {
    uint32_t pivot;
    float dcur;
    uint32_t n_dist, n_expand, n_ids;
};
__device__ __attribute__((noinline, unused)) DescentOut load_descent(const void* kargs, uint32_t q) {
    const kernargs_t ka = uniform_kernargs(kargs);
    q = (uint32_t)__builtin_amdgcn_readfirstlane((int)q);
    const PreDescent pd = ka->a.pre[q];
    DescentOut o{pd.pivot, __uint_as_float(pd.dcur_bits), pd.n_dist, pd.n_expand, pd.n_dist - 1u};
    hent_t* oplog = ka->a.oplog;
    const uint32_t cap = ka->a.oplog_cap;
    if (oplog != nullptr && cap != 0u && threadIdx.x == 0)
        __hip_atomic_store(oplog + (size_t)blockIdx.x * cap, hmake(o.dcur, o.pivot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return o;
}


// The start of a query, out of line: the next work item (`first`: the workgroup's own index, no 5000-way rush on the counter
// at launch; then the shared counter), the query row into the LDS tile, the visited set reset.  Returns the query's index, or
// EMPTY_SLOT when the work list is exhausted.
template <int METRIC, int TABLE>
__device__ __attribute__((noinline)) uint32_t begin_query(const void* kargs, bool first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const kernargs_t ka = uniform_kernargs(kargs);
    const int lane = (int)threadIdx.x;
    uint32_t wi = 0;
    if (__builtin_amdgcn_readfirstlane((int)first) != 0) {
        wi = blockIdx.x;
    } else {
        if (lane == 0) wi = atomicAdd(ka->a.work_counter, 1u);
        wi = readlane_u(wi, 0) + gridDim.x;
    }
    if (wi >= ka->a.nq) return EMPTY_SLOT;
    const uint32_t* qlist = ka->a.qlist;
    const uint32_t q = qlist ? qlist[wi] : wi;
    const uint32_t row_stride = ka->ix.row_stride;
    stage_query<METRIC>(reinterpret_cast<float4*>(lds_raw), ka->a.queries + (size_t)q * row_stride, row_stride, lane, ka->ix.d);
    if constexpr (TABLE == TABLE_GLOBAL_BITMAP) {
        const uint32_t words = ka->a.bitmap_words;
        uint32_t* bitmap = ka->a.bitmap + (size_t)blockIdx.x * words;
        for (uint32_t i = (uint32_t)lane; i < words; i += 64) bitmap[i] = 0u;
    } else {
        uint32_t* table = reinterpret_cast<uint32_t*>(lds_raw + ka->a.tile_bytes + IDS_BYTES);
        const uint32_t cells = 1u << ka->a.tbits;
        const uint32_t words = TABLE == TABLE_LDS_CELL16 ? cells >> 1 : cells;
        const uint32_t fill = TABLE == TABLE_LDS_CELL16 ? 0u : EMPTY_SLOT;
        for (uint32_t i = (uint32_t)lane; i < words; i += 64) table[i] = fill;
    }
    __syncthreads();
    return q;
}
// A query that outgrows its LDS table moves its visited set into the workgroup's HBM bitmap slice and carries on there (cells
// identify their ids exactly, so nothing is recomputed).  Out of line: it happens to a few queries in a hundred.
template <int TABLE>
__device__ __attribute__((noinline)) void migrate_table_to_bitmap(const void* kargs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const kernargs_t ka = uniform_kernargs(kargs);
    const int lane = (int)threadIdx.x;
    const uint32_t words = ka->a.bitmap_words, restbits = ka->a.restbits, idbits = ka->a.idbits;
    uint32_t* bitmap = ka->a.bitmap + (size_t)blockIdx.x * words;
    const uint32_t* table = reinterpret_cast<const uint32_t*>(lds_raw + ka->a.tile_bytes + IDS_BYTES);
    const uint32_t table_cells = 1u << ka->a.tbits;
    for (uint32_t i = (uint32_t)lane; i < words; i += 64) bitmap[i] = 0u;
    __syncthreads();
    for (uint32_t i = (uint32_t)lane; i < table_cells; i += 64) {
        uint32_t id = EMPTY_SLOT;
        if constexpr (TABLE == TABLE_LDS_CELL16) {
            const uint32_t half = (table[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
            if (half != 0u) {
                const uint32_t bdisp = (half & 0x7FFFu) >> restbits;
                const uint32_t rest = half & ((1u << restbits) - 1u);
                const uint32_t home = ((i >> 3) - bdisp) & ((table_cells >> 3) - 1u);  // home bucket
                id = unmix_id((home << restbits) | rest, idbits);
            }
        } else if constexpr (TABLE == TABLE_LDS_CELL32) {
            id = table[i];
        }
        if (id != EMPTY_SLOT) atomicOr(&bitmap[id >> 5], 1u << (id & 31u));
    }
    __syncthreads();
}

// (C): does a choice between equal entries reach the first k answers?
template <int S>
__device__ __forceinline__ bool final_order_ambiguous(const float (&rd)[S], uint32_t len, uint32_t k, float taint_w, int lane) {
    const uint32_t kk = k < len ? k : len;
    if (kk == 0u) return false;
    unsigned long long bad = 0ull;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
        const float nxt = __shfl_down(rd[s], 1);
        const float edge = s + 1 < S ? r_dist_at<S>(rd, (uint32_t)(s + 1) * 64u) : INFINITY;
        const float nd = lane == 63 ? edge : nxt;
        bad |= __ballot(j < kk && j + 1u < len && rd[s] == nd);
    }
    return bad != 0ull || r_dist_at<S>(rd, kk - 1u) == taint_w;
}

// waves per SIMD the search kernel is built for.  One half-storage instantiation gets a wave less than its f32 twin: DistL1 on half
// rows, S = 2, 32-bit cells, lean does not fit the 96 VGPRs that five waves leave -- there the compiler spilled the lane's
// lanemask_lt constant and reloaded it inside the expansion loop; built for four it takes 105 registers and no scratch
template <int METRIC, int S, int TABLE, bool STRICT>
constexpr int search_lb_waves() {
    if (STRICT) return S >= 16 ? 2 : S == 4 && HNSW_PIPE_ROWS != 0 ? 3 : HNSW_LB_WAVES_STRICT;
    if (METRIC == KM_L1_F16 && S == 2 && TABLE == TABLE_LDS_CELL32) return HNSW_LB_WAVES < 4 ? HNSW_LB_WAVES : 4;
    return S >= 16 ? 4 : HNSW_LB_WAVES;
}
// SHAPE (search_kernels.hpp): SHAPE_ANY takes the row stride and ef from the launch's arguments; SHAPE_R128_EF knows them -- rows of 128
// elements, ef == 64 S -- and the host launches it only where both hold (DeviceIndex::SearchCall::shape_launch).  One text of the
// loop either way: the two values are chosen here and handed down (batch_dist's RS, merge_list_body.inc's `ef`).
template <int METRIC, int S, int TABLE, int SHAPE, bool STRICT>
__global__ __launch_bounds__(64, (search_lb_waves<METRIC, S, TABLE, STRICT>())) void hnsw_search_kernel(DeviceIndexView ix, SearchArgs a) {
    constexpr int RS = SHAPE == SHAPE_R128_EF ? 128 : 0;
    const uint32_t ef = SHAPE == SHAPE_R128_EF ? 64u * (uint32_t)S : a.ef;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    // (the out-of-line parts of the kernel read their arguments from here)
    const void* const kargs = (const void*)__builtin_amdgcn_kernarg_segment_ptr();
    float4* tile = reinterpret_cast<float4*>(lds_raw);
    uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes);
    uint32_t* table = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes + IDS_BYTES);
    const int lane = (int)threadIdx.x;
    const uint32_t table_cells = 1u << a.tbits;
    const uint32_t table_words = TABLE == TABLE_LDS_CELL16 ? table_cells >> 1 : table_cells;
    const uint32_t table_limit = table_cells - (table_cells >> 2);  // stop inserting at 75 % load
    // this workgroup's private bitmap slice (in-launch fallback when the LDS table overflows)
    uint32_t* bitmap = blockIdx.x < a.bitmap_blocks ? a.bitmap + (size_t)blockIdx.x * a.bitmap_words : nullptr;
    // lists of more than 64 ids are scanned in batches by the 16-slot kernels only (the host sends every such index there:
    // search_device.hip); everywhere else one batch per list is a compile-time fact -- no inner loop, no runtime flags
    constexpr bool ONE_BATCH = S < 16;
    const bool single_batch = ONE_BATCH || ix.deg_stride <= 64u;
    const uint32_t nbatch = ONE_BATCH ? 1u : (ix.deg_stride + 63u) >> 6;
    const nrm_ptr_t nrm2 = (nrm_ptr_t)a.nrm2;
    bool use_bm = TABLE == TABLE_GLOBAL_BITMAP;
    const bool strict = STRICT && a.cand_scratch != nullptr && a.oplog != nullptr && TABLE != TABLE_GLOBAL_BITMAP;

    auto visit = [&](uint32_t id) __attribute__((always_inline)) -> int {
        if (TABLE == TABLE_GLOBAL_BITMAP || use_bm) return visit_bitmap(bitmap, id);
        if constexpr (TABLE == TABLE_LDS_CELL16) return visit_cell16(table, a.tbits, a.idbits, a.restbits, id);
        else return visit_cell32(table, a.tbits, id);
    };
    auto migrate_to_bitmap = [&]() __attribute__((always_inline)) {
        migrate_table_to_bitmap<TABLE>(kargs);
        use_bm = true;
    };

    // work items: the first one is the workgroup's own index, the following ones come from the shared counter (begin_query)
    bool first_item = true;
    for (;;) {
        const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)begin_query<METRIC, TABLE>(kargs, first_item));
        first_item = false;
        if (q == EMPTY_SLOT) break;
        const uint32_t t_start = (uint32_t)wall_clock64();

        // n_dist starts at 1: the reference evaluates the layer-0 entry point a second time (src/hnsw.rs:952); its distance
        // is the descent's dcur here, but the work counters follow the reference (include/hnsw_mi355x.h, d_stats)
        uint32_t n_dist = 1, n_expand = 0, n_ids = 0, status = 0, n_visited = 1;
        bool flag_tie = false;  // (A)-(C) met and not resolved here
#if HNSW_PHASE_TIMING
        uint32_t ph[4] = {0, 0, 0, 0};
        uint32_t ph_miss = 0;  // expansions whose id row had not been prefetched
#endif
        use_bm = TABLE == TABLE_GLOBAL_BITMAP;  // (begin_query has reset the visited set)

        // ---- greedy descent (src/hnsw.rs:1506-1529): done by hnsw_descend_kernel, its result is picked up here
        const DescentOut dsc = load_descent(kargs, q);
        const uint32_t pivot = (uint32_t)__builtin_amdgcn_readfirstlane((int)dsc.pivot);
        const float dcur = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dsc.dcur)));
        n_dist += (uint32_t)__builtin_amdgcn_readfirstlane((int)dsc.n_dist);
        n_expand += (uint32_t)__builtin_amdgcn_readfirstlane((int)dsc.n_expand);
        n_ids += (uint32_t)__builtin_amdgcn_readfirstlane((int)dsc.n_ids);

        // one batch of <= 64 neighbour ids: visited filter, compaction in list order, distances.
        // Returns the number of fresh ids (rank r -> lane r of de / idc); sets status on a table failure.
        float de = INFINITY;
        uint32_t idc = 0u;
        auto gather_batch = [&](uint32_t id, unsigned long long any_id) __attribute__((always_inline)) -> uint32_t {
            const bool valid = id != EMPTY_SLOT;
            n_ids += popc64(any_id);  // (= the vote over `valid`)
            if (TABLE != TABLE_GLOBAL_BITMAP && !use_bm && n_visited + 64 > table_limit) {
                if (bitmap == nullptr) { status = 1; return 0u; }  // no slice for this workgroup: host re-runs it
                migrate_to_bitmap();
            }
            // 16-bit-cell table: the TEST of every id first (one ds_read_b128 + a packed compare per lane, nothing written);
            // the fresh ids are then known, their row loads go out, and their INSERTION into the table runs behind those
            // loads (batch_dist's `between`).  The other representations mark while they test.
            bool fresh = false, to_insert = false;
            Probe16 pr{};
            if (TABLE == TABLE_LDS_CELL16 && !use_bm) {
                int t = 1;
                if (valid) t = cell16_test(table, a.restbits, a.idbits, id, pr);
                if (__ballot(t == 2) != 0ull) {  // a full home bucket: these ids are looked up (and marked) the long way, now
                    int vr = 0;
                    if (t == 2) vr = visit_cell16(table, a.tbits, a.idbits, a.restbits, id);
                    if (__ballot(vr == 2) != 0ull) {  // displacement budget exhausted inside the table (rare)
                        if (bitmap == nullptr) { status = 1; return 0u; }
                        migrate_to_bitmap();  // includes the ids this batch already placed
                        if (vr == 2) vr = visit_bitmap(bitmap, id);
                        if (t == 0) { t = 2; vr = visit_bitmap(bitmap, id); }  // tested, not yet inserted: marked in the bitmap instead
                    }
                    if (t == 2) fresh = vr == 1;
                }
                if (t == 0) { fresh = true; to_insert = true; }
            } else {
                int vr = 0;
                if (valid) vr = visit(id);
                if (__ballot(vr == 2) != 0ull) {  // (32-bit cells) no room
                    if (use_bm || bitmap == nullptr) { status = 1; return 0u; }
                    migrate_to_bitmap();
                    if (vr == 2) vr = visit_bitmap(bitmap, id);
                }
                fresh = vr == 1;
            }
            const unsigned long long fm = __ballot(fresh);
            const uint32_t nf = popc64(fm);
            if (nf == 0u) return 0u;
            n_visited += nf;
            n_dist += nf;
            // (not __syncthreads(): a workgroup-scope barrier also waits for every global load in flight -- the speculative
            // id-row prefetch of the next candidate would be waited for HERE instead of one expansion later)
            wave_lds_fence();
            if (fresh) ids_lds[popc64(fm & lanemask_lt(lane))] = id;
            wave_lds_fence();
            idc = (uint32_t)lane < nf ? ids_lds[lane] : 0u;
            PH_T(gt1);
            int irc = 1;
            de = batch_dist<METRIC, HNSW_DEEP_G2 != 0 && STRICT && S <= 2, HNSW_PIPE_ROWS != 0 && STRICT && S == 4, RS>(ix.vec, ix.row_stride, ix.d, nrm2, tile, ids_lds, nf, lane, [&]() __attribute__((always_inline)) {
                if constexpr (TABLE == TABLE_LDS_CELL16) {
                    if (to_insert) irc = cell16_insert(table, a.tbits, a.restbits, pr);
                }
            });
            PH_T(gt2);
#if HNSW_PHASE_TIMING == 1
            PH_ACC(1, gt1, gt2);  // row loads + distance chains (profiling builds: part of phase 2, also counted alone)
#endif
            if constexpr (TABLE == TABLE_LDS_CELL16) {
                if (__ballot(irc == 2) != 0ull) {  // no cell within the displacement budget (rare): the set moves to the bitmap, these ids with it
                    if (bitmap == nullptr) { status = 1; return 0u; }
                    migrate_to_bitmap();
                    if (irc == 2) (void)visit_bitmap(bitmap, id);
                }
            }
            return nf;
        };

        // ---- heap-operation log (strict launches): a LOG_EXPAND marker per pop of candidate_points, then the entries
        // that expansion accepted, in order.  Single-lane stores, never waited for unless the log is read.
        hent_t* oplog = nullptr;
        bool log_ok = false;
        uint32_t log_len = 0;
        if constexpr (STRICT) {
            if (strict) { oplog = a.oplog + (size_t)blockIdx.x * a.oplog_cap; log_ok = true; log_len = 1; }  // (entry 0: the entry point, written by the descent)
        }
        auto log_put = [&](hent_t e) __attribute__((always_inline)) {
            if constexpr (STRICT) {
                if (log_ok) {
                    if (log_len < a.oplog_cap) {
                        if (lane == 0) __hip_atomic_store(oplog + log_len, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        log_len += 1;
                    } else {
                        log_ok = false;  // too long to log: if (A)-(C) turns up, the exact kernel searches this query again
                    }
                }
            }
        };
        // The entries of one expansion -- a LOG_EXPAND marker, then the neighbours it accepted (lanes of `de` / `idc`, list
        // order) -- are not stored where they arise but at the NEXT point where the wave has just waited for memory anyway (its
        // ids have arrived): a store issued at the end of an expansion would still be in flight at the top of the next one, and
        // the wait for the prefetched id row there (vmcnt counts loads and stores alike) would wait for its acknowledgement.
        bool pend_marker = false;
        unsigned long long pend_mask = 0ull;
        auto log_flush = [&]() __attribute__((always_inline)) {
            if constexpr (STRICT) {
                if (pend_marker || pend_mask != 0ull) {
                    if (log_ok) {
                        const uint32_t n_acc = popc64(pend_mask);
                        const uint32_t need = n_acc + (pend_marker ? 1u : 0u);
                        if (log_len + need <= a.oplog_cap) {
                            if (pend_marker && lane == 0) __hip_atomic_store(oplog + log_len, LOG_EXPAND, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            const uint32_t at = log_len + (pend_marker ? 1u : 0u) +
                                                __builtin_amdgcn_mbcnt_hi((uint32_t)(pend_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pend_mask, 0u));
                            if (((pend_mask >> lane) & 1ull) != 0ull)
                                __hip_atomic_store(oplog + at, hmake(de, idc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            log_len += need;
                        } else {
                            log_ok = false;  // too long to log: if (A)-(C) turns up, the exact kernel searches this query again
                        }
                    }
                    pend_marker = false;
                    pend_mask = 0ull;
                }
            }
        };

        // ---- search_layer at the lowest non-empty layer (src/hnsw.rs:1542, :922-1064), sorted-array form:
        // return_points and candidate_points as ONE array sorted ascending by distance, an EXPANDED flag per entry
        float rd[S];
        uint32_t ri[S];
#pragma unroll
        for (int s = 0; s < S; ++s) { rd[s] = 0.f; ri[s] = 0u; }
        uint32_t len = 1;
        bool tie_any = false;    // an insertion met an equal distance already in the array
        uint32_t ghost = 0;      // unexpanded entries evicted while an equal entry stayed behind, still == the farthest
        float ghost_w = 0.f;
        float taint_w = -1.f;    // distance at which the last eviction had to choose between equal farthest entries
        uint32_t spec_for = EMPTY_SLOT, spec_ids = EMPTY_SLOT;  // prefetched id row of the likely next candidate
        // ---- accept rule for a whole neighbour list at once (return_points full: entry 64 s + l in slot s of lane l).
        // In list order, neighbour j is accepted (:1028-1037) iff it is nearer than the farthest entry at its turn,
        // i.e. iff fewer than ef of {entries of R, neighbours accepted before it} are not farther than it; its final
        // place is behind everything not farther (R first, then earlier arrivals).  So positions follow from counts,
        // and the array is rebuilt with one scatter through LDS instead of one shift per accepted neighbour.  Not
        // taken (returns false, nothing changed) when equal entries end up on both sides of the cut at ef: that
        // eviction depends on the heap order and needs section 6's bookkeeping, one neighbour at a time.
        // LDS behind the visited table: merge_list's scatter buffer (64 S + 64 entries), then the top of the literal candidate heap
        hent_t* merge_buf = reinterpret_cast<hent_t*>(table + (TABLE == TABLE_GLOBAL_BITMAP ? 0u : table_words));
        auto merge_list = [&](unsigned long long cand) __attribute__((always_inline)) -> bool {
#include "merge_list_body.inc"
            if (tie_here) tie_any = true;
            ghost = 0u;  // the last eviction lowered the farthest distance
            pend_mask |= acc;  // (the log: stored by log_flush)
            return true;
        };
        if (lane == 0) { rd[0] = dcur; ri[0] = pivot; }  // dist_to_entry_point == eval(q, pivot) (:952)
        if (lane == 0) (void)visit(pivot);
        // ---- the lazy literal candidate heap (strict launches): brought up to date from the log when a pop needs it
        uint32_t lenC = 0, log_replayed = 0;
        bool literal_used = false;  // at least one pop was taken from the literal heap
        uint32_t out_status = 0;
        for (;;) {
            PH_T(pt0);
            // c = nearest unexpanded member of R (candidate_points.pop(), :971); none left <=> every remaining
            // candidate is farther than R's worst (:981-993)
            const int cj = r_next<S>(ri, len, lane);
            bool amb = false;
            if (tie_any) {  // is this pop decided by values alone?  (A) / (B)
                if (cj >= 0) {
                    const float dcj = r_dist_at<S>(rd, (uint32_t)cj);
                    uint32_t n_equal = 0;  // unexpanded entries at the nearest candidate's distance
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
                        n_equal += popc64(__ballot(j < len && rd[s] == dcj && (ri[s] & EXPANDED) == 0u));
                    }
                    amb = n_equal >= 2u || (ghost > 0u && dcj == ghost_w);
                } else {
                    amb = ghost > 0u;
                }
            }
            if constexpr (STRICT) {
                if (strict && a.exact_first != 0u) amb = true;  // test hook: every pop comes from the literal heap
            }
            uint32_t c = 0;
            bool popped = false;
            if (__builtin_expect(amb, 0)) {
                if (STRICT && strict && log_ok) log_flush();  // the heap is brought up to date from the log: everything in it
                if (STRICT && strict && log_ok) {
#if HNSW_PHASE_TIMING == 2
                    const unsigned long long lt0 = clock64();
#endif
                    const LiteralPop lp = literal_candidate_pop<TABLE>(kargs, log_replayed, log_len, lenC);
#if HNSW_PHASE_TIMING == 2  // profiling build 2 (tools/literal_profile.py): ticks inside the literal pops, heap operations, ticks in replayed pops
                    ph[1] += (uint32_t)(clock64() - lt0);
                    ph[3] += (uint32_t)__builtin_amdgcn_readfirstlane((int)lp.n_ops);
                    ph[0] += (uint32_t)__builtin_amdgcn_readfirstlane((int)lp.t_pops);
#endif
                    // (what a real call returns sits in vector registers: made wave-uniform again, or the whole loop turns divergent)
                    lenC = (uint32_t)__builtin_amdgcn_readfirstlane((int)lp.lenC);
                    log_replayed = log_len;
                    const hent_t ce = readlane_h(lp.ce, 0);
                    const int prc = __builtin_amdgcn_readfirstlane(lp.rc);
                    if (prc == 0) {
                        literal_used = true;
                        popped = true;
                        log_put(LOG_EXPAND);
                        if (log_ok) log_replayed = log_len;             // the heap has already performed this pop
                        if (-hkey(ce) > r_worst<S>(rd, len)) break;     // :973-993
                        c = hid(ce);
                        // the array's view of the same pop: the entry is now expanded; a ghost leaves the count
                        unsigned long long found = 0ull;
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
                            const bool hit = j < len && ri[s] == c;     // (an expanded entry carries the flag: no match)
                            if (hit) ri[s] |= EXPANDED;
                            found |= __ballot(hit);
                        }
                        if (found == 0ull && ghost > 0u) ghost -= 1u;
                    } else if (prc == 1) {
                        break;                                          // candidate_points is empty (:969)
                    } else {
                        log_ok = false;                                 // candidate scratch exhausted: the exact kernel redoes this query
                        flag_tie = true;
                    }
                } else {
                    flag_tie = true;  // lean launch (or a log that overflowed): equals in arrival order, the query is flagged
                }
            }
            if (!popped) {
                if (cj < 0) break;
                c = r_id_at<S>(ri, cj);
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if ((cj >> 6) == s && lane == (cj & 63)) ri[s] |= EXPANDED;
            }
            n_expand += 1;
            const uint32_t* nrow = ix.nbr0 + (size_t)c * ix.deg_stride;
            for (uint32_t bi = 0; bi < nbatch; ++bi) {
                const uint32_t j = bi * 64u + (uint32_t)lane;
                uint32_t id;
                if (single_batch && spec_for == c) id = spec_ids;
                else id = j < ix.deg_stride ? nrow[j] : EMPTY_SLOT;
#if HNSW_PHASE_TIMING == 1
                if (!(single_batch && spec_for == c)) ph_miss += 1;
#endif
                const unsigned long long any_id = __ballot(id != EMPTY_SLOT);  // (the ids are in registers from here on)
                log_flush();                                // the previous expansion's entries: behind the wait that just ended
                if (bi == 0u && !popped) pend_marker = true;  // this expansion's marker (a literal pop logged its own at once)
                if (single_batch) {
                    // Speculate on the next candidate: its id row is fetched while this one is processed.  The load goes out
                    // only AFTER this expansion's own ids have arrived: issued before them it would sit between them and
                    // their use, and the wait for the ids would wait for the prefetch as well (one HBM round trip per
                    // expansion, the very one the prefetch is there to hide).
                    const int nj = r_next<S>(ri, len, lane);
                    if (nj >= 0) {
                        spec_for = r_id_at<S>(ri, nj);
                        spec_ids = (uint32_t)lane < ix.deg_stride ? ix.nbr0[(size_t)spec_for * ix.deg_stride + (uint32_t)lane] : EMPTY_SLOT;
                    } else {
                        spec_for = EMPTY_SLOT;
                    }
                }
                PH_T(pt1);
#if HNSW_PHASE_TIMING == 1
                PH_ACC(0, pt0, pt1);  // candidate selection + wait for its id row
#endif
                if (any_id == 0ull) break;  // lists are padded at the end only
                const uint32_t nf = gather_batch(id, any_id);
                PH_T(pt3);
                PH_ACC(2, pt1, pt3);  // visited probes + compaction + row loads + accumulate
                if (status != 0) break;
                if (nf == 0u) continue;
                // accept rule applied sequentially in list order (:1028-1053)
                float worst = r_worst<S>(rd, len);
                unsigned long long cand = nf >= 64u ? ~0ull : (1ull << nf) - 1ull;  // (lanes < nf)
                if (len >= ef) cand &= __ballot(de < worst);
                if constexpr ((S == 1 || (S <= HNSW_MERGE_SMAX && (STRICT || S <= HNSW_MERGE_LEAN_SMAX))) && HNSW_MERGE_LISTS != 0) {
                    if (len == ef && popc64(cand) >= (uint32_t)HNSW_MERGE_LISTS && merge_list(cand)) cand = 0ull;
                }
                while (cand != 0ull) {
                    const int jl = ctz64(cand);
                    const float xd = readlane_f(de, jl);
                    if (xd < worst || len < ef) {
                        const uint32_t xi = readlane_u(idc, jl);
                        pend_mask |= 1ull << jl;  // (the log: stored by log_flush)
                        const bool was_full = len == ef;
                        uint32_t last_if = 0u;  // the entry this insertion pushes out of return_points
                        if (was_full) last_if = r_id_flag_at<S>(ri, ef - 1u);
                        if (r_insert<S>(rd, ri, len, ef, xd, xi, lane)) tie_any = true;
                        const float nw = r_worst<S>(rd, len);
                        if (was_full) {
                            if (nw == worst) {  // one of >= 2 equal farthest entries left: which one is the heap's choice
                                taint_w = nw;
                                if ((last_if & EXPANDED) == 0u) { ghost += 1u; ghost_w = nw; }
                            } else {
                                ghost = 0u;     // the farthest distance fell below the ghosts'
                            }
                        }
                        worst = nw;
                    }
                    cand &= cand - 1ull;
                }
                PH_T(pt4);
#if HNSW_PHASE_TIMING == 1
                PH_ACC(3, pt3, pt4);  // result-set insertions
#endif
            }
            if (status != 0) break;
        }
        log_flush();
        if (literal_used) out_status = 3;

        if constexpr (STRICT) {
            // ---- (C): the first k answers by the reference's return_points heap, literally, when values do not decide
            if (__builtin_expect(strict && status == 0 && !flag_tie && tie_any && final_order_ambiguous<S>(rd, len, a.k, taint_w, lane), 0)) {
                if (!log_ok) {
                    flag_tie = true;
                } else {
                    const SortedR<S> sr = literal_return_points<S>(kargs, log_len);
                    len = (uint32_t)__builtin_amdgcn_readfirstlane((int)sr.len);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        rd[s] = hkey(sr.s[s]);
                        ri[s] = hid(sr.s[s]);
                    }
                    out_status = 3;
                }
            }
        } else {
            if (status == 0 && tie_any && !flag_tie && final_order_ambiguous<S>(rd, len, a.k, taint_w, lane)) flag_tie = true;
        }
        if (status == 0 && flag_tie) status = 2;
        {
            QueryEnd<S> e;
#pragma unroll
            for (int s = 0; s < S; ++s) { e.rd[s] = rd[s]; e.ri[s] = ri[s]; }
            e.q = q; e.len = len; e.status = status; e.out_status = out_status;
            e.n_dist = n_dist; e.n_expand = n_expand; e.n_ids = n_ids; e.t_start = t_start;
            e.flags = (tie_any ? 1u : 0u) | (literal_used ? 2u : 0u) | (use_bm ? 4u : 0u);
            e.feedback = (use_bm ? 1u : 0u) | (n_visited > (table_limit >> 1) ? 2u : 0u) | (TABLE != TABLE_GLOBAL_BITMAP ? 4u : 0u);
#if HNSW_PHASE_TIMING
            e.ph[0] = ph[0]; e.ph[1] = ph[1]; e.ph[2] = ph[2]; e.ph[3] = ph[3]; e.ph_miss = ph_miss;
#endif
            finish_query<S>(kargs, e);
        }
        __syncthreads();
    }
}

// =======================================================================================
// Literal search: both BinaryHeaps of the reference emulated from the first to the last operation.
//
// Used for (1) queries a strict launch could not finish itself (log or candidate scratch overflow, launches on the HBM
// bitmap) -- the host passes the flagged list -- and (2) FILTERED search (Hnsw::search_filter with a sorted id vector,
// src/hnsw.rs:1487-1580, src/filter.rs:11-15), whose loop never terminates early and whose return_points does not
// contain its candidates, so the sorted-array form does not apply.
// candidate_points on -dist, return_points on +dist: push = append + sift_up, pop = swap-remove +
// sift_down_to_bottom + sift_up, into_sorted_vec = repeated swap + sift_down_range (SURVEY.md Appendix C).  A sift only
// ever touches one root-to-leaf path, so the wave performs each heap operation cooperatively: lanes load the ancestors
// (push) or the 62 descendants of the current node within 5 levels (pop), the path is chased with readlane, and the
// shifted entries are stored in parallel.  Heaps live in an L2-resident scratch slice of the workgroup (entries =
// {key f32, id u32}) with their top levels in LDS; the visited set is the workgroup's HBM bitmap slice.
//
// Filter (x.allow != nullptr: one bit per flat id, built from the sorted id vector by allow_bitmap_kernel):
//   * the termination test does not end the loop: when the popped candidate is farther than the farthest result and
//     return_points holds >= ef entries, return_points.retain(filter) runs, and the scan of the candidate's list
//     goes ahead (:981-1001).  return_points only ever receives allowed points -- except the entry point, pushed
//     unconditionally (:964) and dropped by the clear() rule at the first allowed push (:1042-1047) -- so retain can
//     only remove a refused entry point standing alone (ef == 1); anything else is reported as an internal error;
//   * with return_points emptied that way: the next unvisited neighbour returns the empty heap (:1019-1024), and a pop
//     before that hits `return_points.peek().unwrap()` (:973): the reference PANICS; reported as status 6, count 0;
//   * an accepted neighbour always enters candidate_points, and return_points only if the filter allows it (:1035-1050);
//   * the answer is the first min(knbn, ef, len) sorted entries with the refused ones dropped (:1547-1565).
// status (stats[3]): 3 done, 4 candidate heap outgrew the launch's scratch (the host searches the query again with room for
// every point), 6 the reference panics on this query, 7 internal error (a refused point inside a return_points of more
// than one entry).
// Round 4: the kernel was latency-bound at ~500 resident queries (56 KB of LDS per workgroup for the heaps' top levels, and
// every accepted neighbour a sift-up of its own, one LDS or L2 round trip each).  Now the pushes of an expansion go into
// candidate_points together (heap_push_batch: one round trip), return_points is touched only where the filter allows a
// neighbour, the id row of the likely next candidate is prefetched, and 10 KB of LDS per workgroup let 16 of them share a
// CU: what is in flight is what hides an expansion's chain of round trips.
// =======================================================================================

template <int METRIC, int NS>
__global__ __launch_bounds__(64, 4) void hnsw_search_exact_kernel(DeviceIndexView ix, SearchArgs a, ExactArgs x) {
    RegHeap<(NS > 0 ? NS : 1)> RR;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float4* tile = reinterpret_cast<float4*>(lds_raw);
    uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes);
    const int lane = (int)threadIdx.x;
    uint32_t* bitmap = a.bitmap + (size_t)blockIdx.x * a.bitmap_words;
    const nrm_ptr_t nrm2 = (nrm_ptr_t)a.nrm2;
    // LDS: [query][ids][R heap: ef+2 entries][candidate heap: first cand_lds entries]
    hent_t* lds_heaps = reinterpret_cast<hent_t*>(lds_raw + a.tile_bytes + IDS_BYTES);
    hent_t* glb = x.heaps + (size_t)blockIdx.x * x.heap_stride;
    const uint32_t r_lds = a.ef + 2u <= x.r_lds_cap ? a.ef + 2u : x.r_lds_cap;
    const HeapMem R{lds_heaps, glb, r_lds};
    const HeapMem Cq{lds_heaps + r_lds, glb + (a.ef + 2u), x.cand_lds};
    const bool filtered = x.allow != nullptr;
    const uint32_t* allow = x.allow;  // this query's bitmap: x.allow, or, with a filter set, slot slot_of[q] behind it (chosen below)
    auto allowed = [&](uint32_t flat) __attribute__((always_inline)) -> bool { return (allow[flat >> 5] >> (flat & 31u)) & 1u; };
    // push + "pop when len > ef" of src/hnsw.rs:1038, :1051-1053 (without a push the length cannot exceed ef)
    auto r_push_capped = [&](uint32_t& len, hent_t item) __attribute__((always_inline)) {
        if constexpr (NS > 0) {
            if (len == RegHeap<(NS > 0 ? NS : 1)>::CAP) { RR.push_then_pop_full(item, lane); return; }  // (then ef == CAP)
            RR.push(len, item, lane);
            if (len > a.ef) (void)RR.pop(len, lane);
        } else {
            heap_push(R, len, item, lane);
            if (len > a.ef) (void)heap_pop(R, len, lane);
        }
    };
    // does return_points hold a point the filter refuses?
    auto r_any_refused = [&](uint32_t len) __attribute__((always_inline)) -> bool {
        unsigned long long m = 0ull;
        if constexpr (NS > 0) {
#pragma unroll
            for (int k = 0; k < (NS > 0 ? NS : 1); ++k) {
                const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
                m |= __ballot(i < len && !allowed(hid(RR.s[k])));
            }
        } else {
            for (uint32_t i0 = 0; i0 < len; i0 += 64) {
                const uint32_t i = i0 + (uint32_t)lane;
                m |= __ballot(i < len && !allowed(hid(hload(R, i < len ? i : 0u))));
            }
        }
        return m != 0ull;
    };
    auto r_get = [&](uint32_t i) __attribute__((always_inline)) -> hent_t {
        if constexpr (NS > 0) return RR.get(i);
        else return hload(R, i);
    };

    for (;;) {
        uint32_t wi = 0;
        if (lane == 0) wi = atomicAdd(a.work_counter, 1u);
        wi = readlane_u(wi, 0);
        if (wi >= a.nq) break;
        const uint32_t q = a.qlist ? a.qlist[wi] : wi;
        if (x.slot_of != nullptr) allow = x.allow + (size_t)x.slot_of[q] * x.allow_stride;  // filter set: the bitmap of this query's filter
        const uint32_t t_start = (uint32_t)wall_clock64();
        stage_query<METRIC>(tile, a.queries + (size_t)q * ix.row_stride, ix.row_stride, lane, ix.d);
        for (uint32_t i = (uint32_t)lane; i < a.bitmap_words; i += 64) bitmap[i] = 0u;
        __syncthreads();
        uint32_t n_dist = 1, n_expand = 0, n_ids = 0, status = 0;  // (1: the second evaluation of the entry point, :952)

        // ---- descent (src/hnsw.rs:1506-1529): done by hnsw_descend_kernel, like the main kernel's
        const PreDescent pd = a.pre[q];
        const uint32_t pivot = pd.pivot;
        const float dcur = __uint_as_float(pd.dcur_bits);
        n_dist += pd.n_dist; n_expand += pd.n_expand; n_ids += pd.n_dist - 1u;

        // ---- search_layer with literal heaps (src/hnsw.rs:938-1063)
        uint32_t lenR = 0, lenC = 0;
        bool returned = false;  // `return return_points` from inside the loop (:1019-1024)
        if (lane == 0) (void)visit_bitmap(bitmap, pivot);
        __syncthreads();
        heap_push(Cq, lenC, hmake(-dcur, pivot), lane);                     // :958-963
        r_push_capped(lenR, hmake(dcur, pivot));                            // :964-967 (unconditional, filter or not)
        const bool single_batch = ix.deg_stride <= 64u;
        uint32_t spec_for = EMPTY_SLOT, spec_ids = EMPTY_SLOT;  // prefetched id row of the likely next candidate (the heap's new top)
        while (lenC > 0u && status == 0 && !returned) {
            const hent_t c = lenC < 32768u ? heap_pop3(Cq, lenC, lane) : heap_pop(Cq, lenC, lane);  // :971
            if (lenR == 0u) { status = 6; break; }                          // :973 `peek().unwrap()` on an emptied heap
            float worst = hkey(r_get(0u));                                  // :973 peek
            if (-hkey(c) > worst) {                                         // :981
                if (!filtered) break;                                       // :992-993
                if (lenR >= a.ef) {                                         // :994-1000 retain(filter)
                    if (r_any_refused(lenR)) {
                        if (lenR == 1u) lenR = 0u;
                        else { status = 7; break; }
                    }
                }
            }
            n_expand += 1;
            const uint32_t* nrow = ix.nbr0 + (size_t)hid(c) * ix.deg_stride;
            const uint32_t nbatch = (ix.deg_stride + 63u) >> 6;
            for (uint32_t bi = 0; bi < nbatch; ++bi) {
                const uint32_t j = bi * 64u + (uint32_t)lane;
                uint32_t id;
                if (single_batch && spec_for == hid(c)) id = spec_ids;
                else id = j < ix.deg_stride ? nrow[j] : EMPTY_SLOT;
                const bool valid = id != EMPTY_SLOT;
                const unsigned long long vm = __ballot(valid);
                if (single_batch) {
                    // speculate on the next candidate -- the heap's top as it is now -- and fetch its id row while this one is
                    // processed (issued behind the arrival of this expansion's own ids, like the main kernel's prefetch)
                    if (lenC > 0u) {
                        spec_for = hid(hload(Cq, 0u));
                        spec_ids = (uint32_t)lane < ix.deg_stride ? ix.nbr0[(size_t)spec_for * ix.deg_stride + (uint32_t)lane] : EMPTY_SLOT;
                    } else {
                        spec_for = EMPTY_SLOT;
                    }
                }
                if (vm == 0ull) break;
                n_ids += popc64(vm);
                const bool fresh = valid && visit_bitmap(bitmap, id) == 1;  // :1016-1017
                const unsigned long long fm = __ballot(fresh);
                const uint32_t nf = popc64(fm);
                if (nf == 0u) continue;
                if (lenR == 0u) { returned = true; break; }                 // :1019-1024 (the first unvisited neighbour)
                n_dist += nf;
                wave_lds_fence();
                if (fresh) ids_lds[popc64(fm & lanemask_lt(lane))] = id;
                wave_lds_fence();
                const uint32_t idc = (uint32_t)lane < nf ? ids_lds[lane] : 0u;
                // does the filter allow this neighbour?  One bitmap word per lane, requested with the row loads
                bool alw = true;
                if (filtered) alw = (uint32_t)lane < nf && allowed(idc);
                const float de = batch_dist<METRIC>(ix.vec, ix.row_stride, ix.d, nrm2, tile, ids_lds, nf, lane);
                // The accept rule in list order (:1013-1053).  candidate_points receives every accepted neighbour and is only
                // read by the next pop, so its pushes are gathered in `acc` and performed together below; return_points (and
                // with it the threshold of the rule) changes only at a neighbour the filter allows, so the walk stops there and
                // nowhere else: between two such neighbours "accepted" is one ballot.
                const unsigned long long allow_m = __ballot(alw && (uint32_t)lane < nf);
                unsigned long long acc = 0ull;
                unsigned long long rest = nf >= 64u ? ~0ull : ((1ull << nf) - 1ull);
                while (rest != 0ull) {
                    const unsigned long long q = __ballot(((rest >> lane) & 1ull) != 0ull && (de < worst || lenR < a.ef));  // :1028
                    const unsigned long long chg = q & allow_m;
                    if (chg == 0ull) { acc |= q; break; }
                    const int jl = ctz64(chg);
                    acc |= (q & lanemask_lt(jl)) | (1ull << jl);            // :1035-1036 for all of them
                    const float xd = readlane_f(de, jl);
                    const uint32_t xi = readlane_u(idc, jl);
                    if (filtered && lenR == 1u && !allowed(hid(r_get(0u)))) lenR = 0u;  // :1042-1047 clear(): the refused entry point
                    r_push_capped(lenR, hmake(xd, xi));                     // :1038 / :1048, :1051-1053
                    worst = hkey(r_get(0u));
                    rest &= ~((2ull << jl) - 1ull);
                }
                if (acc != 0ull) {
                    if (lenC + popc64(acc) > x.cand_cap) { status = 4; break; }
                    heap_push_batch(Cq, lenC, acc, de, idc, lane);
                }
            }
        }

        // ---- into_sorted_vec (:1544) + truncate (:1547) + filter_map (:1549-1565)
        if (status == 0) {
            uint32_t end = lenR;
            while (end > 1u) {
                end -= 1;
                if constexpr (NS > 0) {
                    const hent_t r0 = RR.get(0u), re = RR.get(end);
                    RR.set(0u, re, lane);
                    RR.set(end, r0, lane);
                    RR.sift_down_range(end, lane);
                } else {
                    const hent_t r0 = hload(R, 0u), re = hload(R, end);
                    hfence();
                    if (lane == 0) {
                        hstore(R, 0u, re);
                        hstore(R, end, r0);
                    }
                    hfence();
                    heap_sift_down_range(R, end, lane);
                }
            }
            const uint32_t last = lenR < a.k ? lenR : a.k;
            uint32_t cnt = 0;  // entries written so far (filter_map drops the refused ones)
            for (uint32_t jb = 0; jb < a.k; jb += 64) {
                const uint32_t j = jb + (uint32_t)lane;
                hent_t e = 0ull;
                if (j < last) {
                    if constexpr (NS > 0) {  // entry j sits in lane j % 64 of slot j / 64
#pragma unroll
                        for (int kk = 0; kk < (NS > 0 ? NS : 1); ++kk)
                            if ((jb >> 6) == (uint32_t)kk) e = RR.s[kk];
                    } else {
                        e = hload(R, j);
                    }
                }
                const uint32_t flat = hid(e);
                const bool keep = j < last && (!filtered || allowed(flat));
                const unsigned long long km = __ballot(keep);
                if (keep) {
                    const size_t o = (size_t)q * a.k + cnt + popc64(km & lanemask_lt(lane));
                    uint32_t l = 0;
                    while (l + 1 < NB_LAYER_MAX && flat >= ix.layer_offset[l + 1]) ++l;
                    put_answer(a.out_ids, a.id_stride, a.out_dists, a.dist_stride, o, ix.origin_id[flat], hkey(e));
                    if (a.out_layer) a.out_layer[o] = (uint8_t)l;
                    if (a.out_rank) a.out_rank[o] = (int32_t)(flat - ix.layer_offset[l]);
                }
                cnt += popc64(km);
            }
            for (uint32_t j = cnt + (uint32_t)lane; j < a.k; j += 64) {
                const size_t o = (size_t)q * a.k + j;
                put_answer(a.out_ids, a.id_stride, a.out_dists, a.dist_stride, o, 0ull, 0.f);
                if (a.out_layer) a.out_layer[o] = 0;
                if (a.out_rank) a.out_rank[o] = 0;
            }
            if (lane == 0) put_count(a.out_counts, a.count_stride, q, cnt);
        } else {
            for (uint32_t j = (uint32_t)lane; j < a.k; j += 64) {
                const size_t o = (size_t)q * a.k + j;
                put_answer(a.out_ids, a.id_stride, a.out_dists, a.dist_stride, o, 0ull, 0.f);
                if (a.out_layer) a.out_layer[o] = 0;
                if (a.out_rank) a.out_rank[o] = 0;
            }
            if (lane == 0) {
                put_count(a.out_counts, a.count_stride, q, 0u);
                // ctrl[1]: internal failures, ctrl[2]: reference panics, ctrl[3]: candidate heap outgrew this launch's scratch --
                // those queries are listed and searched again with room for every point
                if (status == 4u && a.retry_out != nullptr) a.retry_out[atomicAdd(a.overflow_count + 2, 1u)] = q;
                else atomicAdd(a.overflow_count + (status == 6 ? 1 : 0), 1u);
            }
        }
        if (lane == 0) {
            uint32_t* st = a.stats + (size_t)q * 8;
            st[0] = n_dist; st[1] = n_expand; st[2] = n_ids; st[3] = status == 0 ? 3u : status;
            st[4] = t_start; st[5] = (uint32_t)wall_clock64(); st[6] = lenC; st[7] = ((pd.n_expand & 0xFFu) << 8) | (pd.n_dist << 16);
        }
        __syncthreads();
    }
}

// =======================================================================================
// Construction (SURVEY.md 8f row f1): the SEARCHES of Hnsw::insert_slice (src/hnsw.rs:1077-1215) for a window of new
// points, against a frozen snapshot of the graph in HBM.  One wavefront per point p (its vector is the query):
//   * from the entry point down to level(p) + 1: search_layer(ef = 1) per layer (:1114-1155); the hit of each layer goes
//     back to the host (it becomes an entry of p's own list at that layer, :1140-1144) and is the next layer's entry when
//     it is nearer;
//   * from min(level(p), entry level) down to 0: search_layer(ef_construction) (:1157-1197); the whole sorted candidate
//     list goes back to the host, and its nearest element -- what select_neighbours always keeps first -- is the next
//     layer's entry (:1201-1203).
// select_neighbours, the list updates and reverse_update_neighborhood_simple stay on the host (builder.cpp), which then
// patches the snapshot (scatter_lists_kernel) before the next window.  The sorted-array search_layer of the query kernel
// is used in its lean form (equal distances in arrival order: construction in the reference is racy anyway under
// parallel_insert, and the host builder it replaces is not tie-exact either).
// =======================================================================================
template <int METRIC, int S>
__global__ __launch_bounds__(64, S >= 16 ? 4 : 5) void hnsw_build_search_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float4* tile = reinterpret_cast<float4*>(lds_raw);
    uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes);
    uint32_t* table = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes + IDS_BYTES);
    const int lane = (int)threadIdx.x;
    const uint32_t table_cells = 1u << a.tbits;
    const uint32_t table_words = table_cells >> 1;
    const uint32_t table_limit = table_cells - (table_cells >> 2);
    uint32_t* bitmap = blockIdx.x < a.bitmap_blocks ? a.bitmap + (size_t)blockIdx.x * a.bitmap_words : nullptr;
    const nrm_ptr_t nrm2 = (nrm_ptr_t)a.nrm2;
    bool use_bm = false;
    uint32_t n_visited = 0;
    bool failed = false;

    auto visit = [&](uint32_t id) __attribute__((always_inline)) -> int {
        if (use_bm) return visit_bitmap(bitmap, id);
        return visit_cell16(table, a.tbits, a.idbits, a.restbits, id);
    };
    auto migrate_to_bitmap = [&]() __attribute__((always_inline)) {
        for (uint32_t i = (uint32_t)lane; i < a.bitmap_words; i += 64) bitmap[i] = 0u;
        __syncthreads();
        for (uint32_t i = (uint32_t)lane; i < table_cells; i += 64) {
            const uint32_t half = (table[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
            if (half != 0u) {
                const uint32_t bdisp = (half & 0x7FFFu) >> a.restbits;
                const uint32_t rest = half & ((1u << a.restbits) - 1u);
                const uint32_t home = ((i >> 3) - bdisp) & ((table_cells >> 3) - 1u);
                const uint32_t id = unmix_id((home << a.restbits) | rest, a.idbits);
                atomicOr(&bitmap[id >> 5], 1u << (id & 31u));
            }
        }
        __syncthreads();
        use_bm = true;
    };

    float rd[S];
    uint32_t ri[S];
    uint32_t len = 0;
    // search_layer(q, pivot, ef, layer) on the snapshot's lists of that layer; result in rd / ri / len (sorted ascending)
    auto search_layer = [&](const uint32_t* __restrict__ nbr, uint32_t stride, uint32_t ef, uint32_t pivot) __attribute__((always_inline)) {
        use_bm = false;
        n_visited = 1;
        for (uint32_t i = (uint32_t)lane; i < table_words; i += 64) table[i] = 0u;
        if (lane == 0) ids_lds[0] = pivot;
        __syncthreads();
        const float dcur = readlane_f(batch_dist<METRIC>(a.vec, a.row_stride, 0u, nrm2, tile, ids_lds, 1u, lane), 0);  // :952
#pragma unroll
        for (int s = 0; s < S; ++s) { rd[s] = 0.f; ri[s] = 0u; }
        if (lane == 0) { rd[0] = dcur; ri[0] = pivot; (void)visit(pivot); }
        len = 1;
        __syncthreads();
        const uint32_t nbatch = (stride + 63u) >> 6;
        for (;;) {
            const int cj = r_next<S>(ri, len, lane);   // candidate_points.pop() (:971); none left <=> :981-993
            if (cj < 0) break;
            const uint32_t c = r_id_at<S>(ri, cj);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if ((cj >> 6) == s && lane == (cj & 63)) ri[s] |= EXPANDED;
            const uint32_t* nrow = nbr + (size_t)c * stride;
            for (uint32_t bi = 0; bi < nbatch && !failed; ++bi) {
                const uint32_t j = bi * 64u + (uint32_t)lane;
                const uint32_t id = j < stride ? nrow[j] : EMPTY_SLOT;
                const bool valid = id != EMPTY_SLOT;
                if (__ballot(valid) == 0ull) break;
                if (!use_bm && n_visited + 64 > table_limit) {
                    if (bitmap == nullptr) { failed = true; break; }
                    migrate_to_bitmap();
                }
                int vr = 0;
                if (valid) vr = visit(id);                                  // :1016-1017
                if (__ballot(vr == 2) != 0ull) {
                    if (use_bm || bitmap == nullptr) { failed = true; break; }
                    migrate_to_bitmap();
                    if (vr == 2) vr = visit_bitmap(bitmap, id);
                }
                const bool fresh = vr == 1;
                const unsigned long long fm = __ballot(fresh);
                const uint32_t nf = popc64(fm);
                if (nf == 0u) continue;
                n_visited += nf;
                wave_lds_fence();
                if (fresh) ids_lds[popc64(fm & lanemask_lt(lane))] = id;
                wave_lds_fence();
                const uint32_t idc = (uint32_t)lane < nf ? ids_lds[lane] : 0u;
                const float de = batch_dist<METRIC>(a.vec, a.row_stride, 0u, nrm2, tile, ids_lds, nf, lane);  // :1026
                float worst = r_worst<S>(rd, len);
                unsigned long long cand = __ballot((uint32_t)lane < nf && (len < ef || de < worst));
                while (cand != 0ull) {                                      // :1028-1053 in list order
                    const int jl = ctz64(cand);
                    const float xd = readlane_f(de, jl);
                    if (xd < worst || len < ef) {
                        (void)r_insert<S>(rd, ri, len, ef, xd, readlane_u(idc, jl), lane);
                        worst = r_worst<S>(rd, len);
                    }
                    cand &= cand - 1ull;
                }
            }
            if (failed) break;
        }
    };

    for (;;) {
        uint32_t wi = 0;
        if (lane == 0) wi = atomicAdd(a.work_counter, 1u);
        wi = readlane_u(wi, 0);
        if (wi >= a.count) break;
        const uint32_t p = a.first + wi;
        const uint32_t level = a.level[p];
        stage_query<METRIC>(tile, a.vec + (size_t)p * a.row_stride, a.row_stride, lane, 0u, a.nrm2 == nullptr);
        uint32_t enter = a.entry;
        // dist_to_entry (:1110-1112)
        if (lane == 0) ids_lds[0] = enter;
        __syncthreads();
        float dist_to_entry = readlane_f(batch_dist<METRIC>(a.vec, a.row_stride, 0u, nrm2, tile, ids_lds, 1u, lane), 0);
        __syncthreads();
        for (uint32_t l = level + 1u; l <= a.entry_level; ++l)  // defaults: no hit
            if (lane == 0) a.hit_ids[(size_t)wi * NB_LAYER_MAX + l] = EMPTY_SLOT;
        for (int l = (int)a.entry_level; l > (int)level && !failed; --l) {      // :1114-1155
            if (((a.layer_mask >> l) & 1u) == 0u) continue;  // no point of exactly this level yet: search_layer returns nothing (:942-946)
            search_layer(a.lists[l], a.stride[l], 1u, enter);
            if (failed) break;
            if (len > 0u) {
                const float hd = readlane_f(rd[0], 0);
                const uint32_t hi = readlane_u(ri[0], 0) & ~EXPANDED;
                if (lane == 0) {
                    a.hit_ids[(size_t)wi * NB_LAYER_MAX + (uint32_t)l] = hi;
                    a.hit_d[(size_t)wi * NB_LAYER_MAX + (uint32_t)l] = hd;
                }
                if (hd < dist_to_entry) { enter = hi; dist_to_entry = hd; }
            }
        }
        const int top = (int)(level < a.entry_level ? level : a.entry_level);
        for (int l = top; l >= 0 && !failed; --l) {                               // :1157-1205
            const size_t slot = (size_t)a.slot0[wi] + (size_t)l;
            if (((a.layer_mask >> l) & 1u) == 0u && (uint32_t)l != level) {  // (the point itself counts at its own level, :516)
                if (lane == 0) a.out_n[slot] = 0u;
                continue;
            }
            search_layer(a.lists[l], a.stride[l], a.ef_c, enter);
            if (failed) break;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const uint32_t j = (uint32_t)s * 64u + (uint32_t)lane;
                if (j < len) {
                    a.out_ids[slot * a.ef_c + j] = ri[s] & ~EXPANDED;
                    a.out_d[slot * a.ef_c + j] = rd[s];
                }
            }
            if (lane == 0) a.out_n[slot] = len;
            if (len > 0u) enter = readlane_u(ri[0], 0) & ~EXPANDED;
        }
        if (failed) {
            if (lane == 0) atomicAdd(a.fail_count, 1u);
            failed = false;
        }
        __syncthreads();
    }
}

// =======================================================================================
// Construction: select_neighbours (src/hnsw.rs:1299-1421) for the slots of a window -- the heuristic that keeps a candidate e
// only if no neighbour selected before it is at least as near to e as e is to the new point (:1373-1375).  On the host cores
// this was 83 of the 90 thread-seconds of a 1M x 128 build (ef_c distance evaluations against up to 2 M selected rows per
// point); here one wavefront per slot walks the candidates in ascending order, stages candidate e as the "query" and gets
// dist(e, every selected row) from ONE batch_dist -- the same left-to-right arithmetic and the same argument order as the
// host's eval(e, selected), so window-1 builds still reproduce the serial graph byte for byte.
// extend_candidates (layer 0 of reloaded indexes) stays on the host: the launcher does not use this kernel then.
// LDS: [tile][ids: 64][selected ids: sel_stride][selected distances: sel_stride]
// =======================================================================================
constexpr uint32_t CAND_DISCARDED = 0x80000000u;  // flag on a candidate id (scratch): pruned, kept for keep_pruned (:1396-1411)

template <int METRIC>
__global__ __launch_bounds__(64, 6) void hnsw_build_select_kernel(SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float4* tile = reinterpret_cast<float4*>(lds_raw);
    uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + a.tile_bytes);
    uint32_t* sel_lds = ids_lds + 64;
    float* seld_lds = reinterpret_cast<float*>(sel_lds + a.sel_stride);
    const int lane = (int)threadIdx.x;
    const nrm_ptr_t nrm2 = (nrm_ptr_t)a.nrm2;
    const uint32_t nchunk = a.row_stride >> 2;
    for (;;) {
        uint32_t slot = 0;
        if (lane == 0) slot = atomicAdd(a.work_counter, 1u);
        slot = readlane_u(slot, 0);
        if (slot >= a.n_slots) break;
        const uint32_t n = a.cand_n[slot];
        const uint32_t nb = a.slot_nb[slot];
        uint32_t* cid = a.cand_ids + (size_t)slot * a.ef_c;
        const float* cd = a.cand_d + (size_t)slot * a.ef_c;
        uint32_t* oid = a.sel_ids + (size_t)slot * a.sel_stride;
        float* od = a.sel_d + (size_t)slot * a.sel_stride;
        uint32_t nsel = 0;
        if (n <= nb) {  // fewer candidates than asked for: all of them, in order (:1319-1331)
            for (uint32_t j = (uint32_t)lane; j < n; j += 64) { oid[j] = cid[j]; od[j] = cd[j]; }
            nsel = n;
        } else {
            for (uint32_t base = 0; base < n && nsel < nb; base += 64) {
                const uint32_t cnt = n - base < 64u ? n - base : 64u;
                const uint32_t my_id = (uint32_t)lane < cnt ? cid[base + (uint32_t)lane] : 0u;
                const float my_d = (uint32_t)lane < cnt ? cd[base + (uint32_t)lane] : 0.f;
                for (uint32_t t = 0; t < cnt && nsel < nb; ++t) {
                    const uint32_t e_id = readlane_u(my_id, (int)t);
                    const float e_d = readlane_f(my_d, (int)t);
                    bool keep = true;
                    if (nsel > 0u) {
                        // e as the query: its row into the tile (DistCosine: its stored norm beside it, the tail zeroed)
                        const float4* src = reinterpret_cast<const float4*>(a.vec + (size_t)e_id * a.row_stride);
                        wave_lds_fence();
                        for (uint32_t i = (uint32_t)lane; i < nchunk; i += 64) {
                            float4 v = src[i];
                            if constexpr (METRIC == DIST_COSINE) {
                                if (nrm2 == nullptr && i + 1u == nchunk) {
                                    *reinterpret_cast<double*>(tile + nchunk) = __builtin_bit_cast(double, ((unsigned long long)__float_as_uint(v.w) << 32) | __float_as_uint(v.z));
                                    v.z = 0.f;
                                    v.w = 0.f;
                                }
                            }
                            tile[i] = v;
                        }
                        if constexpr (METRIC == DIST_COSINE) {
                            if (nrm2 != nullptr && lane == 0) *reinterpret_cast<double*>(tile + nchunk) = nrm2[e_id];
                        }
                        wave_lds_fence();
                        for (uint32_t sb = 0; sb < nsel && keep; sb += 64) {
                            const uint32_t c2 = nsel - sb < 64u ? nsel - sb : 64u;
                            if ((uint32_t)lane < c2) ids_lds[lane] = sel_lds[sb + (uint32_t)lane];
                            wave_lds_fence();
                            const float dd = batch_dist<METRIC>(a.vec, a.row_stride, 0u, nrm2, tile, ids_lds, c2, lane);
                            if (__ballot((uint32_t)lane < c2 && dd <= e_d) != 0ull) keep = false;  // :1373-1375
                            wave_lds_fence();
                        }
                    }
                    if (keep) {
                        if (lane == 0) { sel_lds[nsel] = e_id; seld_lds[nsel] = e_d; }
                        nsel += 1;
                    } else if (a.keep_pruned != 0u) {
                        if (lane == 0) cid[base + t] = e_id | CAND_DISCARDED;
                    }
                }
            }
            wave_lds_fence();
            if (a.keep_pruned != 0u && nsel < nb) {  // the pruned ones fill what is left, in their order (:1396-1411)
                __threadfence_block();
                for (uint32_t j = 0; j < n && nsel < nb; ++j) {
                    const uint32_t v = __hip_atomic_load(cid + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((v & CAND_DISCARDED) != 0u) {
                        if (lane == 0) { sel_lds[nsel] = v & ~CAND_DISCARDED; seld_lds[nsel] = cd[j]; }
                        nsel += 1;
                    }
                }
                wave_lds_fence();
            }
            for (uint32_t j = (uint32_t)lane; j < nsel; j += 64) { oid[j] = sel_lds[j]; od[j] = seld_lds[j]; }
        }
        if (lane == 0) a.sel_n[slot] = nsel;
        __syncthreads();
    }
}

#ifdef HNSW_SHARED_HELPERS
// patches the snapshot: list `u` of the update batch replaces row ids[u] of its layer's array
// upd = [n_upd][1 + 1 + max_stride]: {node id, layer, ids... (EMPTY padded)}
__global__ void scatter_lists_kernel(const uint32_t* __restrict__ upd, uint32_t n_upd, uint32_t rec_words, BuildLists lists) {
    const uint32_t u = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (u >= n_upd) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t* rec = upd + (size_t)u * rec_words;
    const uint32_t node = rec[0], layer = rec[1];
    uint32_t* row = lists.lists[layer] + (size_t)node * lists.stride[layer];
    for (uint32_t j = lane; j < lists.stride[layer]; j += 64) row[j] = rec[2 + j];
}
#endif

#ifdef HNSW_SHARED_HELPERS
// allow[f] = the sorted id vector contains origin_id[f] (impl FilterT for Vec<usize>: binary_search, src/filter.rs:11-15)
__global__ void allow_bitmap_kernel(const uint64_t* __restrict__ origin_id, uint32_t n, const uint64_t* __restrict__ ids, uint64_t m,
                                    uint32_t* __restrict__ allow) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (f < n) {
        const uint64_t key = origin_id[f];
        uint64_t lo = 0, hi = m;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            const uint64_t v = ids[mid];
            if (v < key) lo = mid + 1;
            else hi = mid;
        }
        ok = lo < m && ids[lo] == key;
    }
    const unsigned long long b = __ballot(ok);  // blockDim.x is a multiple of 64: one 64-bit word pair per wave
    if ((threadIdx.x & 63u) == 0u && f < n) {
        allow[f >> 5] = (uint32_t)b;
        if (f + 32u < ((n + 31u) & ~31u)) allow[(f >> 5) + 1u] = (uint32_t)(b >> 32);
    }
}

// The bitmaps of a group of filters of a filter set in one launch: slot s = filter f0 + s, the sorted id vector
// ids[offsets[f0 + s] .. offsets[f0 + s + 1]) (CSR), its bitmap in words [s W, (s + 1) W) of `allow`, W = ceil(n / 32); bits past
// n are zero.  One wavefront per (slot, 64 flat ids): allow_bitmap_kernel's binary search inside that filter's range.  W may be
// odd, so a slot's last word abuts the next slot's first: the second word of a wave is written only where the slot has one.
__global__ void allow_bitmap_set_kernel(const uint64_t* __restrict__ origin_id, uint32_t n, const uint64_t* __restrict__ ids,
                                        const uint64_t* __restrict__ offsets, uint32_t f0, uint32_t n_slots, uint32_t* __restrict__ allow) {
    const uint32_t waves_per_slot = (n + 63u) >> 6, words = (n + 31u) >> 5;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wave >= (uint64_t)n_slots * waves_per_slot) return;  // (whole waves leave: the ballot below sees 64 lanes or none)
    const uint32_t slot = (uint32_t)(wave / waves_per_slot);
    const uint32_t f = (uint32_t)(wave % waves_per_slot) * 64u + (threadIdx.x & 63u);
    bool ok = false;
    if (f < n) {
        const uint64_t key = origin_id[f];
        const uint64_t end = offsets[(uint64_t)f0 + slot + 1u];
        uint64_t lo = offsets[(uint64_t)f0 + slot], hi = end;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            const uint64_t v = ids[mid];
            if (v < key) lo = mid + 1;
            else hi = mid;
        }
        ok = lo < end && ids[lo] == key;
    }
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63u) == 0u) {  // (f < n: the wave exists only for f < 64 waves_per_slot, and its first id is in range)
        uint32_t* out = allow + (size_t)slot * words;
        out[f >> 5] = (uint32_t)b;
        if ((f >> 5) + 1u < words) out[(f >> 5) + 1u] = (uint32_t)(b >> 32);
    }
}

// How many entries of filter_of[0..nq) name no filter of the set (>= n_filters): added to *bad.  The search kernel indexes the
// bitmaps with these values, so the call reads the count back and refuses before it launches the search.
__global__ void filter_of_check_kernel(const uint32_t* __restrict__ filter_of, uint32_t nq, uint64_t n_filters, uint32_t* __restrict__ bad) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = __ballot(q < nq && (uint64_t)filter_of[q < nq ? q : 0u] >= n_filters);
    if ((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(bad, (uint32_t)__popcll(m));
}

// The queries of one group of a filter set: every q with f0 <= filter_of[q] < f0 + n_slots is appended to qlist (count in
// *count; the order among wavefronts is the order of their atomics -- it only decides which workgroup searches which query) and
// slot_of[q] = filter_of[q] - f0.
__global__ void filter_group_kernel(const uint32_t* __restrict__ filter_of, uint32_t nq, uint32_t f0, uint32_t n_slots,
                                    uint32_t* __restrict__ qlist, uint32_t* __restrict__ slot_of, uint32_t* __restrict__ count) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t f = q < nq ? filter_of[q] : 0u;
    const bool in = q < nq && f >= f0 && f - f0 < n_slots;
    const unsigned long long m = __ballot(in);
    if (m == 0ull) return;
    uint32_t base = 0;
    if (lane == 0u) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = readlane_u(base, 0);
    if (in) {
        qlist[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = q;
        slot_of[q] = f - f0;
    }
}

#endif

// Distance<f32>::eval through the search's own routine (batch_dist: lane groups, DPP chain, G = 4 and G = 2 branches).
// Matrix mode: out[q][r] = dist(queries[q], rows[r]), one workgroup per (query, batch of `nf` consecutive rows).
// Pair mode (pairs != 0): out[q] = dist(queries[q0 + q], rows[q0 + q]), one workgroup per pair.  Arithmetic tests.
// DEEP / PIPE / RS: batch_dist's own template arguments, handed on -- the row loops the expansion loop of hnsw_search_kernel
// compiles (EVAL_* in search_kernels.hpp says which kernels); RS != 0 needs row_stride == RS (the host side checks it).
template <int METRIC, bool DEEP = false, bool PIPE = false, int RS = 0>
__global__ __launch_bounds__(64) void eval_matrix_kernel(const float* __restrict__ queries, const float* __restrict__ rows,
                                                         const double* __restrict__ nrm2, float* __restrict__ out, uint32_t n_rows,
                                                         uint32_t row_stride, uint32_t nf, uint32_t tile_bytes, uint32_t pairs, uint32_t d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float4* tile = reinterpret_cast<float4*>(lds_raw);
    uint32_t* ids_lds = reinterpret_cast<uint32_t*>(lds_raw + tile_bytes);
    const int lane = (int)threadIdx.x;
    const uint32_t q = blockIdx.y;
    const uint32_t r0 = pairs ? q : blockIdx.x * nf;
    const uint32_t cnt = pairs ? 1u : (n_rows - r0 < nf ? n_rows - r0 : nf);
    stage_query<METRIC>(tile, queries + (size_t)q * row_stride, row_stride, lane, d);
    if ((uint32_t)lane < cnt) ids_lds[lane] = r0 + (uint32_t)lane;
    __syncthreads();
    const float v = batch_dist<METRIC, DEEP, PIPE, RS>(rows, row_stride, d, (nrm_ptr_t)nrm2, tile, ids_lds, cnt, lane, NoOverlap());
    if ((uint32_t)lane < cnt) out[pairs ? (size_t)q : (size_t)q * n_rows + r0 + (uint32_t)lane] = v;
}

#ifdef HNSW_SHARED_HELPERS
// DistCosine's third sum for every point, once: f32 squares widened to f64, summed left to right over the d elements.
// out != nullptr: out[i]; else the sum goes into the last 8 bytes of the row's own padding (row_stride - d >= 2).
__global__ void row_sq_norms_kernel(float* __restrict__ vec, double* __restrict__ out, uint32_t n, uint32_t d, uint32_t row_stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* r = vec + (size_t)i * row_stride;
    double s2 = 0.;
    for (uint32_t c = 0; c < d; ++c) s2 = s2 + (double)(r[c] * r[c]);
    if (out) out[i] = s2;
    else *reinterpret_cast<double*>(r + row_stride - 2u) = s2;
}
#endif

#include "search_pair.inc"

#ifdef HNSW_SHARED_HELPERS
#include "lane_lab.inc"
#endif

}  // namespace
}  // namespace hnswgpu
