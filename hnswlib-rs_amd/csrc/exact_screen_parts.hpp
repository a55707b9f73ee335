// exact_screen_parts.hpp -- what the units behind a matrix-core screen share: exact_screen.hip (the exact k-NN),
// exact_range_screen.hip (the exact range search) and dbscan_screen.hip (exact DBSCAN).  The shape of a screen workgroup and its LDS,
// the bounds themselves (screen_coeff, screen_lb: DESIGN.md section 15.13; screen_proved, screen_ub: 15.15; sqrt_cut: 15.14), the
// preparation of a chunk's queries, and the rows' plain f32 norms, which the replica keeps.
// Private: not installed, not part of the ABI; a unit includes it once, behind exact_tile.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "exact_internal.hpp"
#include "exact_tile.hpp"

namespace hnswgpu {
namespace {

constexpr uint32_t SCREEN_MIN_ROWS = 256;     // fewer rows are not worth a tile: the call runs the existing path
constexpr uint32_t SCREEN_SLAB_ROWS = 1024;   // a slab's rows at least: every (query, slab) list costs C insertions to warm up
constexpr uint32_t SCREEN_WG_TARGET = 1024;   // workgroups a launch aims for (four per CU)
constexpr uint32_t SQ = 32;         // queries of a wavefront: the M of the MFMA
constexpr uint32_t RB = 64;         // rows of a block: two N tiles of 32
constexpr uint32_t KC = 32;         // elements of a staged chunk: one 128-byte line of every row
constexpr uint32_t RPITCH = KC + 4; // floats between two rows of a staged block: 16-byte reads of 8 consecutive rows cover every bank once
constexpr uint32_t MAX_WAVES = 4;
// The range of squared norms (f32) in which the bound is proved; outside it a pair gets the lowest bound there is
constexpr float NORM_LO = 0x1p-40f, NORM_HI = 0x1p40f;

typedef float v16f __attribute__((ext_vector_type(16)));

// The coefficient of the error term per metric (screen_lb), exact in f32: an integer below 2^13 times 2^-24
float screen_coeff(int metric, uint64_t d) {
    if (metric == DIST_L2) return (float)(4 * d + 32) * 0x1p-24f;     // of nq + nx, on the squared distance
    if (metric == DIST_DOT) return (float)(d + 32) * 0x1p-24f;         // of nq + nx, on the inner product
    return (float)(2 * d + 32) * 0x1p-24f;                           // DistCosine: absolute, on the cosine
}

// The streamed screens (exact_screen_long.hip, exact_range_screen_long.hip) by a row's padded length
constexpr uint64_t LONG_MAX_DPAD = 4096;
constexpr uint64_t LONG_MIN_DPAD = 288;              // below: the resident kernel with four wavefronts

// The coefficient of the error term for the streamed screen: screen_coeff up to 1120 elements, where it was proved with the O(du)
// factors below 1; beyond, with those factors carried for d <= 4096 and K = d + 39 >= dpad + 8.  Exact in f32: an
// integer below 2^15 times 2^-24.
[[maybe_unused]] float screen_coeff_long(int metric, uint64_t d) {
    if (d <= 1120) return screen_coeff(metric, d);
    if (metric == DIST_L2) return (float)(4 * d + 96) * 0x1p-24f;
    if (metric == DIST_DOT) return (float)(d + 64) * 0x1p-24f;
    return (float)(2 * d + 96) * 0x1p-24f;
}

// A lower bound, as an f32 that is never NaN and never below +0, of the distance exact_knn.hip computes for a pair whose inner product
// the matrix cores gave as s; nq, nx: the two squared norms in plain f32; cu: screen_coeff.  The last step is the reference's own last
// step (a correctly rounded sqrt; 1 - x and the clamp; DistCosine: in f64 and narrowed) applied to a bound of its argument: every
// step is monotone.  Outside the proved range -- a norm outside [NORM_LO, NORM_HI], NaN included, or a screen value that is not
// finite -- the answer is +0: the pair is a candidate whatever its distance.
template <int METRIC>
__device__ __forceinline__ float screen_lb(float s, float nq, float nx, float cu) {
    const bool ok = nq >= NORM_LO && nq <= NORM_HI && nx >= NORM_LO && nx <= NORM_HI && fabsf(s) <= 3.0e38f;
    float lb;
    if constexpr (METRIC == DIST_L2) {
        const float w = nq + nx;
        const float t = w - 2.f * s;
        lb = __builtin_sqrtf(fmaxf(t - cu * w, 0.f));
    } else if constexpr (METRIC == DIST_DOT) {
        const float w = nq + nx;
        lb = fmaxf(1.f - (s + cu * w), 0.f);
    } else {
        const float c = s / __builtin_sqrtf(nq * nx);
        lb = (float)fmax(1. - (double)(c + cu), 0.);
    }
    return ok ? lb : 0.f;
}

// The range in which screen_lb and screen_ub are proved: both norms in [NORM_LO, NORM_HI] (a NaN is outside), the screen value finite
__device__ __forceinline__ bool screen_proved(float s, float nq, float nx) {
    return nq >= NORM_LO && nq <= NORM_HI && nx >= NORM_LO && nx <= NORM_HI && fabsf(s) <= 3.0e38f;
}

// An upper bound, as an f32, of the same distance, from the same inputs and with the same error term as screen_lb (DESIGN.md 15.15:
// the inequalities behind screen_lb are two-sided, and the same coefficients cover the roundings on this side).  Again the
// reference's own monotone last step, on a bound of its argument from the other side.  ONLY inside screen_proved: outside it there
// is no upper bound, the value returned means nothing, and a caller has to treat the pair as undecided by screen_proved itself.
template <int METRIC>
__device__ __forceinline__ float screen_ub(float s, float nq, float nx, float cu) {
    if constexpr (METRIC == DIST_L2) {
        const float w = nq + nx;
        const float t = w - 2.f * s;
        return __builtin_sqrtf(fmaxf(t + cu * w, 0.f));
    } else if constexpr (METRIC == DIST_DOT) {
        const float w = nq + nx;
        return fmaxf(1.f - (s - cu * w), 0.f);
    } else {
        const float c = s / __builtin_sqrtf(nq * nx);
        return (float)fmax(1. - (double)(c - cu), 0.);
    }
}

// DistL2: the greatest f32 x with sqrt(x) <= r, the sqrt being screen_lb's (correctly rounded, so monotone): for every x in
// [+0, +inf], sqrt(x) <= r exactly when x <= this value.  -1 where no x has it (r below -0, r NaN).  The walk starts within a few
// units in the last place of the cut: r * r is one rounding away from r^2, and the cut lies less than two further on.  (The k-NN
// screen has no radius and no caller for it.)
[[maybe_unused]] __device__ float sqrt_cut(float r) {
    if (!(r >= 0.f)) return -1.f;
    float x = fminf(r * r, 3.4028234664e38f);
    while (x > 0.f && __builtin_sqrtf(x) > r) x = __uint_as_float(__float_as_uint(x) - 1u);
    while (x < __builtin_inff()) {
        const float y = __uint_as_float(__float_as_uint(x) + 1u);
        if (!(__builtin_sqrtf(y) <= r)) break;
        x = y;
    }
    return x;
}

// LDS of a workgroup of `waves` wavefronts: the queries (pitch dpad + 4 floats: 16-byte reads of 8 consecutive queries cover every
// bank once), two staged row blocks, and per query the threshold, the list's length and the norm -- self (the queries are stored
// points, exact_screen_knn.hpp): and the query's own DataId rank
uint64_t screen_lds_bytes(uint64_t waves, uint64_t dpad, bool self = false) {
    return waves * SQ * (dpad + 4) * 4 + 2ull * RB * RPITCH * 4 + waves * SQ * (self ? 20 : 16);
}

// one thread per query slot of the chunk's tiles: the padded row, the two norms (slots behind the last query: zeros)
__global__ void exact_screen_prep_kernel(const float* __restrict__ src, uint32_t nq, uint32_t d, uint32_t dpad, uint32_t n_slots, float* __restrict__ qpad,
                                         float* __restrict__ qn, double* __restrict__ qnorm) {
    const uint32_t qs = blockIdx.x * blockDim.x + threadIdx.x;
    if (qs >= n_slots) return;
    const uint32_t live = qs < nq ? d : 0u;
    float nf = 0.f;
    double s1 = 0.;  // f32 squares widened to f64, summed left to right: finish_staged_query
    for (uint32_t i = 0; i < dpad; ++i) {
        const float e = i < live ? src[(size_t)qs * d + i] : 0.f;
        const float sq = e * e;
        nf = nf + sq;
        s1 = s1 + (double)sq;
        qpad[(size_t)qs * dpad + i] = e;
    }
    qn[qs] = nf;
    qnorm[qs] = s1;
}

// one thread per row: the first d elements (what lies behind them, a DistCosine norm included, is no data)
__global__ void exact_screen_xnorm_kernel(DeviceIndexView ix, float* __restrict__ xn) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ix.n) return;
    const float* row = ix.vec + (size_t)r * ix.row_stride;
    float nf = 0.f;
    for (uint32_t i = 0; i < ix.d; ++i) nf = nf + row[i] * row[i];
    xn[r] = nf;
}

template <typename F>
hipError_t for_screened_metric(int metric, F&& f) {
    switch (metric) {
        case DIST_L2: f(std::integral_constant<int, DIST_L2>{}); break;
        case DIST_COSINE: f(std::integral_constant<int, DIST_COSINE>{}); break;
        case DIST_DOT: f(std::integral_constant<int, DIST_DOT>{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
bool metric_has_screen(int metric) { return metric == DIST_L2 || metric == DIST_COSINE || metric == DIST_DOT; }

// the rows' f32 norms of the replica, made by the first call that needs them (the stream is waited for)
int row_norms(ExactState& st, const DeviceIndexView& v, hipStream_t stream, const float** out, std::string& err) {
    std::lock_guard<std::mutex> g(st.mu);
    if (st.d_xnorm == nullptr) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, (size_t)v.n * sizeof(float)));
        hipLaunchKernelGGL(exact_screen_xnorm_kernel, grid_of(v.n), dim3(256), 0, stream, v, static_cast<float*>(p));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            err = std::string("exact screen: the rows' norms: ") + hipGetErrorString(e);
            return ERR_DEVICE;
        }
        st.d_xnorm = p;
    }
    *out = static_cast<const float*>(st.d_xnorm);
    return OK;
}

// wavefronts of a screen workgroup for rows of d elements on this device: as many (4 at most) as its LDS holds queries for; 0: none
// (exact_screen_long.hip keeps no queries resident and does not ask)
[[maybe_unused]] uint32_t screen_waves(int device, uint64_t dpad, bool self = false) {
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return 0;
    for (uint32_t w = MAX_WAVES; w > 0u; w >>= 1)
        if (screen_lds_bytes(w, dpad, self) <= (uint64_t)limit) return w;
    return 0;
}

}  // namespace
}  // namespace hnswgpu
