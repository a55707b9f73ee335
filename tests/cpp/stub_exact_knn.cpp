// Stand-in for exact_knn.hip on a box without HIP, beside stub_device.cpp: the two exact-search entries of the C ABI report
// "no device" behind the argument checks a caller can rely on everywhere -- so that the sanitizer build of the host side
// (tools/asan_host_suite.sh) still exports every symbol include/hnsw_mi355x.h declares.  Test infrastructure only.
#include "capi_index.hpp"
using namespace hnswgpu;
static int no_device(const hnswgpu_index* idx, const void* queries, uint64_t nq, uint64_t d, uint64_t k, const void* allowed, uint64_t n_allowed,
                     const void* out_ids, const void* out_dists, const void* out_counts) {
    if (!idx) return capi_fail(HNSWGPU_ERR_ARG, "null argument");
    if (nq != 0 && (!queries || !out_ids || !out_dists || !out_counts)) return capi_fail(HNSWGPU_ERR_ARG, "null buffer");
    if (k == 0) return capi_fail(HNSWGPU_ERR_ARG, "knbn must be > 0");
    if (k > 4096) return capi_fail(HNSWGPU_ERR_ARG, "exact search: knbn above 4096");
    if (hnswgpu_dimension(idx) != 0 && d != hnswgpu_dimension(idx)) return capi_fail(HNSWGPU_ERR_ARG, "query dimension differs from the index dimension");
    if (n_allowed != 0 && !allowed) return capi_fail(HNSWGPU_ERR_ARG, "null filter");
    {
        std::shared_lock<std::shared_mutex> sl(const_cast<hnswgpu_index*>(idx)->mu);
        if (idx->arithmetic != HNSWGPU_ARITH_SCALAR)
            return capi_fail(HNSWGPU_ERR_ARG, "exact search answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
    }
    return capi_fail(HNSWGPU_ERR_DEVICE, "no HIP device visible (a gfx950 GPU is required; there is no CPU fallback)");
}
extern "C" {
int hnswgpu_exact_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k, const uint64_t* allowed_ids,
                               uint64_t n_allowed, uint64_t* out_ids, float* out_dists, uint8_t*, int32_t*, uint32_t* out_counts) {
    for (uint64_t i = 1; allowed_ids && i < n_allowed; ++i)
        if (allowed_ids[i - 1] > allowed_ids[i]) return capi_fail(HNSWGPU_ERR_ARG, "the id vector of a filter must be sorted ascending");
    return no_device(idx, queries, nq, d, k, allowed_ids, n_allowed, out_ids, out_dists, out_counts);
}
int hnswgpu_exact_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                      const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids, float* d_out_dists, uint8_t*,
                                      int32_t*, uint32_t* d_out_counts, void*) {
    return no_device(idx, d_queries, nq, d, k, d_allowed_ids, n_allowed, d_out_ids, d_out_dists, d_out_counts);
}
}
