// exact_range_parts.hpp -- what the two exact range searches share behind their counting: exact_range.hip (two passes of the f32
// chain) and exact_range_screen.hip (a matrix-core screen and a rerank).  The scan of a chunk's counters into the CSR offsets, the
// sort of every query's segment of keys, and the way from sorted keys to answers.  Private: not installed, not part of the ABI; a
// unit includes it once, behind exact_tile.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "exact_tile.hpp"

namespace hnswgpu {
namespace {

// one workgroup: the counters of a chunk, query major and slab minor, into offs[q + 1] = offs[0] + the hits of queries 0 .. q, and
// in place every counter into the hits of its query in the slabs before it.  offs[0]: set to `base` (set_base), else what the
// previous chunk left there.
__global__ __launch_bounds__(1024) void exact_range_scan_kernel(uint32_t* __restrict__ cnt, uint32_t nq, uint32_t n_slabs, uint64_t* __restrict__ offs,
                                                               bool set_base, uint64_t base) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nq + 1023u) / 1024u;
    const uint32_t q0 = t * per < nq ? t * per : nq, q1 = nq - q0 < per ? nq : q0 + per;
    uint64_t sum = 0;
    for (uint32_t q = q0; q < q1; ++q)
        for (uint32_t s = 0; s < n_slabs; ++s) sum += cnt[(size_t)q * n_slabs + s];
    part[t] = sum;
    __syncthreads();
    if (t == 0u) {
        uint64_t run = set_base ? base : offs[0];
        if (set_base) offs[0] = base;
        for (uint32_t i = 0; i < 1024u; ++i) { const uint64_t p = part[i]; part[i] = run; run += p; }
    }
    __syncthreads();
    uint64_t run = part[t];
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t in_query = 0;
        for (uint32_t s = 0; s < n_slabs; ++s) {
            const uint32_t c = cnt[(size_t)q * n_slabs + s];
            cnt[(size_t)q * n_slabs + s] = in_query;
            in_query += c;
        }
        run += in_query;
        offs[q + 1u] = run;
    }
}

// one thread per sorted key: the answer it stands for
__global__ __launch_bounds__(256) void exact_range_decode_kernel(DeviceIndexView ix, const uint64_t* __restrict__ keys, uint32_t count,
                                                                const uint32_t* __restrict__ order, uint64_t* __restrict__ out_ids,
                                                                float* __restrict__ out_dists, uint8_t* __restrict__ out_layer,
                                                                int32_t* __restrict__ out_rank) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const uint64_t key = keys[j];
    const uint32_t rk = (uint32_t)key < ix.n ? (uint32_t)key : 0u;  // (a rank, whatever the slot holds)
    write_answer(ix, order, key, rk, j, out_ids, out_dists, out_layer, out_rank);
}

// an answer's position among the batch's answers -> its slot in the chunk's keys (the segment bounds of the sort)
struct RangeSlot {
    uint64_t base;
    __host__ __device__ unsigned int operator()(uint64_t v) const { return (unsigned int)(v - base); }
};
typedef rocprim::transform_iterator<const uint64_t*, RangeSlot, unsigned int> range_slot_iter_t;
hipError_t sort_segments(void* temp, size_t& temp_bytes, uint64_t* keys_in, uint64_t* keys_out, uint32_t count, uint32_t segments,
                         const uint64_t* d_offs, uint64_t base, hipStream_t stream) {
    const range_slot_iter_t begin(d_offs, RangeSlot{base});
    return rocprim::segmented_radix_sort_keys(temp, temp_bytes, keys_in, keys_out, count, segments, begin, begin + 1, 0u, 64u, stream);
}

}  // namespace
}  // namespace hnswgpu
