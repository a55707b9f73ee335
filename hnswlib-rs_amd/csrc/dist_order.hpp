// dist_order.hpp -- the order of a distance or an edge weight, once, for the kernels and for the host checks of capi.cpp, which
// must refuse exactly what the kernels refuse.  Plain C++ that g++ compiles too.  Private: not installed, not part of the ABI.
#pragma once
#include <cstdint>

namespace hnswgpu {

// f32 -> u32 whose unsigned order is the order of the values, every NaN behind everything (distances are >= 0: then this is the
// bit pattern with the top bit set; the other cases keep the order total whatever a distance returns)
#if defined(__HIPCC__)
__host__ __device__ __forceinline__
#else
inline
#endif
uint32_t dist_order_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    if (v != v) return 0xFFFFFFFFu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace hnswgpu
