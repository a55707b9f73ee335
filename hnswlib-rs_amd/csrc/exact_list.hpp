// exact_list.hpp -- the sorted list of the smallest 64-bit keys that one wavefront keeps per (query, slab), with its running
// threshold: what the slab kernel of exact_knn.hip and the screen kernel of exact_screen.hip insert into.  Behind exact_tile.hpp
// (KEY_NONE, readlane_u, ctz64, popc64).  list_insert is a real call (noinline): only the units that insert include this.
// Private: not installed, not part of the ABI.
#pragma once
#include "exact_tile.hpp"

namespace hnswgpu {
namespace {

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {
    return ((uint64_t)readlane_u((uint32_t)(v >> 32), lane) << 32) | readlane_u((uint32_t)v, lane);
}
__device__ __forceinline__ uint64_t first_lane_u64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// the lists are private to one wavefront; what one lane stored another lane loads later
__device__ __forceinline__ void list_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

struct ListState {
    uint32_t len;
    uint64_t thr;  // KEY_NONE until the list is full, then its last key
};
// the keys of the lanes in `mask` go into the sorted list (all lanes take part; everything but `key` is wave-uniform).
// ONE_WAVE: the workgroup is this one wavefront, threadIdx.x is the lane.
template <bool ONE_WAVE>
__device__ __attribute__((noinline)) ListState list_insert(uint64_t* list, uint32_t cap, ListState s, uint64_t key, uint64_t mask) {
    const uint32_t lane = ONE_WAVE ? threadIdx.x : threadIdx.x & 63u;
    // (arguments arrive in vector registers: say that they are wave-uniform, the loops below are scalar control flow then)
    mask = first_lane_u64(mask);
    cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)cap);
    s.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.len);
    s.thr = first_lane_u64(s.thr);
    while (mask != 0ull) {
        const int b = ctz64(mask);
        mask &= mask - 1ull;
        const uint64_t kb = readlane_u64(key, b);
        if (!(kb < s.thr)) continue;  // an earlier key of this mask moved the threshold
        // the entries above kb move up one slot, chunk by chunk from the tail (a chunk is loaded whole before it is stored); the
        // one that falls off a full list is dropped.  Sorted: the entries below kb are a prefix, the walk ends in their chunk.
        uint32_t pos = 0;
        for (uint32_t c = (s.len + 63u) >> 6; c-- > 0u;) {
            const uint32_t i = (c << 6) + lane;
            const bool have = i < s.len;
            const uint64_t v = have ? list[i] : KEY_NONE;
            const bool below = have && v < kb;
            const unsigned long long bm = __ballot(below);
            if (have && !below && i + 1u < cap) list[i + 1u] = v;
            if (bm != 0ull) { pos = (c << 6) + popc64(bm); break; }
        }
        if (lane == 0u) list[pos] = kb;
        if (s.len < cap) ++s.len;
        list_fence();
        if (s.len == cap) s.thr = first_lane_u64(list[cap - 1u]);
    }
    return s;
}

}  // namespace
}  // namespace hnswgpu
