// union_find.hpp -- the lock-free union-find over u32 parents (ECL-CC: Jaiganesh & Burtscher, HPDC 2018) of graph_components.hip,
// spanning_forest.hip, dendrogram.hip and condensed_tree.hip, and the validation kernels of a CSR with their one word, which the
// first two launch through csr_intake.hpp (the other two have no caller for them).  Private, device code only.  Every name here is
// in an unnamed namespace: a unit that includes it compiles its own copy of the kernels, and host code that launches them is shared
// the same way, as a header in an unnamed namespace.  The compress kernel is union_find_compress.inc: a unit includes it, inside
// its own unnamed namespace, where its kernels stand in their order of use.
// The invariant behind every loop: parent[v] <= v at all times, and a write to parent[v] only ever lowers it (a compare-and-swap of a
// root v to a smaller root, an atomic min with an ancestor).  So the links have no cycle, a walk up strictly descends, and a root is
// the smallest vertex of its tree.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hnswgpu {
namespace {

// the validation word of the CSR form: the total in the low half, the flags above it
constexpr uint64_t BAD_FIRST = 1ull << 32, BAD_DESCENT = 1ull << 33, BAD_TOTAL = 1ull << 34, BAD_COL = 1ull << 35, BAD_NO_COLS = 1ull << 36;
constexpr uint32_t CHECK_BLOCKS = 2048;  // the grid of cc_check_cols_kernel

__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's tree as far as this thread sees it, halving the path on the way.  Ends: v takes the value of its parent, which is
// smaller, until it is its own parent -- at most v steps.
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t v) {
    uint32_t p = parent_of(parent, v);
    while (p != v) {
        const uint32_t g = parent_of(parent, p);
        if (g != p) atomicMin(parent + v, g);  // (an ancestor of v, below its parent)
        v = p;
        p = g;
    }
    return v;
}

// a and b into one tree: the larger root under the smaller.  Ends: a round that does not hook replaces the larger of (ra, rb) by its
// parent, which is smaller -- ra + rb falls every round and is never negative.
__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    uint32_t ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;  // hi was a root and hangs under lo now
        ra = old;               // somebody hooked hi first: old < hi is an ancestor of it
        rb = lo;
    }
}

// one thread per r of 0 .. n
__global__ __launch_bounds__(256) void cc_check_offsets_kernel(const uint64_t* __restrict__ offsets, uint32_t n, unsigned long long* __restrict__ word) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > n) return;
    const uint64_t here = offsets[r];
    unsigned long long bad = 0ull;
    if (r == 0u && here != 0ull) bad |= BAD_FIRST;
    if (r < n && here > offsets[r + 1u]) bad |= BAD_DESCENT;
    if (r == n) bad |= here >= (1ull << 32) ? BAD_TOTAL : here;  // (the total itself, below the flags)
    if (bad != 0ull) atomicOr(word, bad);
}

// CHECK_BLOCKS x 256 threads over the offsets[n] cols (the caller's array holds that many, whatever else the offsets say)
__global__ __launch_bounds__(256) void cc_check_cols_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ cols, uint32_t n,
                                                           unsigned long long* __restrict__ word) {
    const uint64_t total = offsets[n];
    if (total >= (1ull << 32) || total == 0ull) return;
    if (cols == nullptr) {
        if (blockIdx.x == 0u && threadIdx.x == 0u) atomicOr(word, (unsigned long long)BAD_NO_COLS);
        return;
    }
    bool bad = false;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (uint64_t)CHECK_BLOCKS * 256u) bad |= cols[e] >= n;
    if (bad) atomicOr(word, (unsigned long long)BAD_COL);
}

}  // namespace
}  // namespace hnswgpu
