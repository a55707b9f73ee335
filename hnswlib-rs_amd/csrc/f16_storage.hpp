// f16_storage.hpp -- binary32 -> binary16 where that loses nothing: the host side of half-precision replicas
// (hnswgpu_set_storage).  A portable bit routine: no -mf16c, no compiler half type.  It serves the representability scan
// (hnswgpu_f16_representable, set_storage, the inserts on an F16 index) and the conversion of DeviceIndex::upload alike.
#pragma once
#include <cstdint>
#include <cstring>

namespace hnswgpu {

constexpr int STORAGE_F32 = 0, STORAGE_F16 = 1;  // DeviceIndex::set_storage (HNSWGPU_STORAGE_*)

// The binary16 bits of x when (f32)(f16)x has the bits of x and x is not NaN: +-0, the f16 subnormals (multiples of 2^-24),
// the normals up to +-65504 whose last 13 mantissa bits are zero, +-inf.  false: x is not representable (*h untouched).
inline bool f16_exact_bits(float x, uint16_t* h) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t exp = (u >> 23) & 0xFFu, man = u & 0x7FFFFFu;
    if (exp == 0xFFu) {  // inf; NaN is refused (its payload would not survive a test by value)
        if (man != 0u) return false;
        *h = (uint16_t)(sign | 0x7C00u);
        return true;
    }
    if (exp == 0u) {  // zero; an f32 subnormal is below 2^-126, far under the smallest half
        if (man != 0u) return false;
        *h = sign;
        return true;
    }
    const int e = (int)exp - 127;
    if (e > 15) return false;
    if (e >= -14) {  // a normal half: 10 mantissa bits
        if ((man & 0x1FFFu) != 0u) return false;
        *h = (uint16_t)(sign | (uint32_t)(e + 15) << 10 | man >> 13);
        return true;
    }
    if (e < -24) return false;
    // a subnormal half m 2^-24, m = 1 .. 1023: the 24-bit significand shifted down by -1 - e (14 .. 23) bits, none of them set
    const uint32_t full = man | 0x800000u;
    const unsigned shift = (unsigned)(-1 - e);
    if ((full & ((1u << shift) - 1u)) != 0u) return false;
    *h = (uint16_t)(sign | full >> shift);
    return true;
}
// the number of elements of x[0..n) that are not representable; *first_bad (may be null): the index of the first one
inline uint64_t f16_count_unrepresentable(const float* x, uint64_t n, uint64_t* first_bad) {
    uint64_t bad = 0;
    uint16_t h;
    for (uint64_t i = 0; i < n; ++i)
        if (!f16_exact_bits(x[i], &h)) {
            if (bad == 0 && first_bad) *first_bad = i;
            ++bad;
        }
    return bad;
}

}  // namespace hnswgpu
