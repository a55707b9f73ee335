// dendrogram.hip -- the single-linkage dendrogram of a spanning forest on the device (gfx950 only): the device side of
// hnswgpu_forest_dendrogram(_device) and hnswgpu_graph_dendrogram(_device) of include/hnsw_mi355x.h (the entries and every check
// that needs no device are in capi.cpp).  DESIGN.md "Dendrogram of a forest".
//
// The m edges in their given order are the merges; the answer names, for every edge, the two clusters it merges (a vertex v < n, or
// n + the last earlier edge inside the cluster) and the size of the result.  The sequential union-find reads an edge after all
// earlier ones; here the edge indices are halved instead, ceil(log2 m) times, over the union-find of union_find.hpp, integer
// atomics only.  Labels are cluster ids in [0, n + m); every edge carries two current labels la[e], lb[e] (its ends at first);
// w[label] is the size of that cluster (1 for a vertex).
// In memory a label x stands as the SLOT n + m - 1 - x: the cluster of edge i is slot m - 1 - i, the vertices are the slots from m
// on.  The union-find hangs the larger number under the smaller, so the root of a tree is its most recent cluster -- in a forest
// read by ascending weight the large one that many edges of a block name -- and every other tree hooks itself under it with a
// compare-and-swap on its OWN word; with the ids as they are the large cluster's word was the one all of them met at (measured:
// DESIGN.md §15.8).  dn_check_kernel writes slots, dn_size_kernel turns them back.
// Invariant: at the level with block size B the blocks are the aligned ranges of B edge indices, and the labels of an edge in the
// block that starts at s name the components of its ends under the edges 0 .. s - 1.
//   dn_check_kernel     one thread per label and per edge: w = 1 for a vertex, 0 for a cluster; la, lb = the ends (0, 0 for an edge with an
//                       end >= n or two equal ends, which the word records: the levels then run on ends that are in range)
//   a level, B = 2^ceil(log2 m) down to 2, h = B / 2, all blocks at once:
//     dn_init_kernel      parent[x] = x, top[x] = 0 for every label (top holds an edge's number + 1: 0 is "none")
//     dn_unite_kernel     one thread per edge of a lower half ((e & h) == 0): unite la[e], lb[e].  Labels of different blocks are
//                         disjoint (the invariant), so one parent array serves every block.
//     cc_compress_kernel  parent[x] = its root (its root marks go where the sums stand next: the memset behind it clears them)
//     dn_top_kernel       the same edges: top[root] = max(top[root], e + 1), one atomic per group of lanes with the same root,
//                         behind a load that lets a loser skip it
//     dn_sum_kernel       every label x: its root r has a top => wsum[r] += w[x], one atomic per group of lanes with the same root,
//                         into a block's table in LDS, which goes to memory once per root and block.  A label that no lower-half
//                         edge names is its own root without a top: it falls out.
//     dn_weight_kernel    one thread per label: a root r with a top writes w[cluster n + top[r] - 1] = wsum[r] (the same slot may
//                         be written at several levels, always with the same value)
//     dn_relabel_kernel   one thread per edge of an upper half: a label whose root has a top becomes cluster n + top - 1
//   dn_size_kernel      one thread per edge: size = w[la] + w[lb]; la == lb is a cycle, recorded in the word; la, lb as cluster ids
// Why the levels are right: the lower half of a block keeps its start s, so its labels stay valid.  The upper half starts at
// s + h: a component under 0 .. s + h - 1 is a component under 0 .. s - 1 that no lower-half edge touched -- the label stands -- or
// a union of such components, whose largest edge lies in the lower half: top is that edge.  After the level with B = 2 every edge
// is its own block.  A cycle: the first edge e that closes one has only forest edges below it, so at the level whose lower half
// joins its two sides both labels take the same root's top, and equal labels stay equal; unions from other blocks (labels are
// disjoint for a forest only) can but make them equal sooner.  A forest never has la == lb.  Every label ever written is below
// n + m, so a bad edge list is refused, never a fault.
// No wavefront waits on another, nothing is read back inside the loop, the answer is a function of the edge list alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
// (the CSR validation kernels that come with the union-find have no caller in this unit)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "union_find.hpp"
#pragma clang diagnostic pop

namespace hnswgpu {
namespace {

constexpr uint32_t BAD_END = 1u, BAD_LOOP = 2u, BAD_CYCLE = 4u;  // the one word of a call

// labels + edges can pass 2^32 - 256: a thread's number is taken in 64 bits
__device__ __forceinline__ uint64_t thread_number() { return (uint64_t)blockIdx.x * 256u + threadIdx.x; }

// max(labels, m) threads.  a / b may be la / lb themselves (the host form uploads into them): no __restrict__.
__global__ __launch_bounds__(256) void dn_check_kernel(const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t m, uint32_t labels, uint32_t* la,
                                                      uint32_t* lb, uint32_t* __restrict__ w, uint32_t* __restrict__ word) {
    const uint64_t t = thread_number();
    if (t < labels) w[t] = t >= m ? 1u : 0u;  // (slots m .. labels - 1 are the vertices)
    if (t >= m) return;
    uint32_t x = a[t], y = b[t], bad = 0u;
    if (x >= n || y >= n) bad = BAD_END;
    else if (x == y) bad = BAD_LOOP;
    if (bad != 0u) {
        x = y = 0u;
        atomicOr(word, bad);
    }
    la[t] = labels - 1u - x;
    lb[t] = labels - 1u - y;
}

__global__ __launch_bounds__(256) void dn_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ top, uint32_t labels) {
    const uint64_t x = thread_number();
    if (x >= labels) return;
    parent[x] = (uint32_t)x;
    top[x] = 0u;
}

// one thread per edge; la[e], lb[e] < labels
__global__ __launch_bounds__(256) void dn_unite_kernel(const uint32_t* __restrict__ la, const uint32_t* __restrict__ lb, uint32_t m, uint32_t h,
                                                      uint32_t* parent) {
    const uint64_t e = thread_number();
    if (e >= m || ((uint32_t)e & h) != 0u) return;
    cc_unite(parent, la[e], lb[e]);
}

#include "union_find_compress.inc"

// Where a tree is large most lanes of a wavefront meet at its root.  The two kernels below take the root of the first lane that is
// still to do, serve every lane that has the same root with ONE atomic, and repeat, WAVE_GROUPS times at the most; the lanes left
// over (a wavefront over many small trees) go one by one.  Every lane of the wavefront runs the loop: its trip count is uniform.
constexpr int WAVE_GROUPS = 4;

// top[r] = max(top[r], mine).  top[] only rises during the kernel, so a value at or above mine, however old, says that mine cannot
// win: behind the load most threads skip the atomic.
__device__ __forceinline__ void raise_top(uint32_t* top, uint32_t r, uint32_t mine) {
    if (__hip_atomic_load(top + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(top + r, mine);
}

// one thread per edge.  parent[] is compressed and nothing hooks here: parent[x] is x's root.
__global__ __launch_bounds__(256) void dn_top_kernel(const uint32_t* __restrict__ la, uint32_t m, uint32_t h, const uint32_t* __restrict__ parent,
                                                    uint32_t* top) {
    const uint64_t e = thread_number();
    const bool live = e < m && ((uint32_t)e & h) == 0u;
    const uint32_t lane = threadIdx.x & 63u, mine = (uint32_t)e + 1u;
    uint32_t r = 0u;
    if (live) r = parent[la[e]];
    uint64_t todo = __ballot(live);
    for (int t = 0; t < WAVE_GROUPS && todo != 0ull; ++t) {
        const uint32_t first = (uint32_t)__shfl((int)r, __ffsll((long long)todo) - 1);
        const uint64_t same = __ballot(live && r == first);
        // edge numbers ascend with the lane: the group's highest lane holds its largest edge
        if (lane == 63u - (uint32_t)__clzll((long long)same)) raise_top(top, r, mine);
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) raise_top(top, r, mine);
}

// A block per SUM_CHUNKS x 256 consecutive labels.  A few hundred trees of thousands of labels each, scattered over the label
// range, send thousands of atomics to each of a few hundred words, which then go one after the other (measured: §15.8).  So a
// block sums in LDS first, in an open-addressed table of SUM_SLOTS roots, and adds every root it holds once, at the end; a root
// that finds no place within two probes goes to memory at once.
constexpr uint32_t SUM_CHUNKS = 8, SUM_SLOTS = 2048, SUM_SHIFT = 21, NO_ROOT = 0xFFFFFFFFu;  // (2^(32 - SUM_SHIFT) == SUM_SLOTS)

__device__ __forceinline__ void sum_into(uint32_t* keys, uint32_t* sums, uint32_t* wsum, uint32_t r, uint32_t v) {
    uint32_t slot = (r * 2654435761u) >> SUM_SHIFT;
    for (int probe = 0; probe < 2; ++probe) {
        const uint32_t old = atomicCAS(keys + slot, NO_ROOT, r);
        if (old == NO_ROOT || old == r) {
            atomicAdd(sums + slot, v);
            return;
        }
        slot = (slot + 1u) & (SUM_SLOTS - 1u);
    }
    atomicAdd(wsum + r, v);
}

__global__ __launch_bounds__(256) void dn_sum_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ top, const uint32_t* __restrict__ w,
                                                    uint32_t labels, uint32_t* __restrict__ wsum) {
    __shared__ uint32_t keys[SUM_SLOTS], sums[SUM_SLOTS];
    for (uint32_t i = threadIdx.x; i < SUM_SLOTS; i += 256u) {
        keys[i] = NO_ROOT;
        sums[i] = 0u;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * (256u * SUM_CHUNKS);
    for (uint32_t c = 0; c < SUM_CHUNKS; ++c) {
        const uint64_t x = base + c * 256u + threadIdx.x;
        uint32_t r = 0u, mine = 0u;
        bool live = false;
        if (x < labels) {
            r = parent[x];
            live = top[r] != 0u;
            if (live) mine = w[x];
        }
        uint64_t todo = __ballot(live);
        for (int t = 0; t < WAVE_GROUPS && todo != 0ull; ++t) {
            const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t first = (uint32_t)__shfl((int)r, (int)lead);
            const bool in = live && r == first;
            uint32_t s = in ? mine : 0u;  // the group's sum, in every lane
            for (int d = 32; d >= 1; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d);
            if (lane == lead) sum_into(keys, sums, wsum, first, s);
            todo &= ~__ballot(in);
        }
        if ((todo >> lane) & 1ull) sum_into(keys, sums, wsum, r, mine);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SUM_SLOTS; i += 256u)
        if (keys[i] != NO_ROOT) atomicAdd(wsum + keys[i], sums[i]);
}

// one thread per label: 1 <= top[r] <= m, so the slot written, the one of cluster n + top[r] - 1, is below m
__global__ __launch_bounds__(256) void dn_weight_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ top,
                                                       const uint32_t* __restrict__ wsum, uint32_t m, uint32_t labels, uint32_t* __restrict__ w) {
    const uint64_t r = thread_number();
    if (r >= labels || parent[r] != (uint32_t)r) return;
    const uint32_t t = top[r];
    if (t != 0u) w[m - t] = wsum[r];
}

// one thread per edge
__global__ __launch_bounds__(256) void dn_relabel_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ top, uint32_t m, uint32_t h,
                                                        uint32_t* __restrict__ la, uint32_t* __restrict__ lb) {
    const uint64_t e = thread_number();
    if (e >= m || ((uint32_t)e & h) == 0u) return;
    const uint32_t ta = top[parent[la[e]]], tb = top[parent[lb[e]]];
    if (ta != 0u) la[e] = m - ta;
    if (tb != 0u) lb[e] = m - tb;
}

// one thread per edge: the slots become the answer's cluster ids where they stand
__global__ __launch_bounds__(256) void dn_size_kernel(uint32_t* __restrict__ la, uint32_t* __restrict__ lb, const uint32_t* __restrict__ w, uint32_t m,
                                                     uint32_t labels, uint32_t* __restrict__ size, uint32_t* __restrict__ word) {
    const uint64_t e = thread_number();
    if (e >= m) return;
    const uint32_t x = la[e], y = lb[e];
    size[e] = w[x] + w[y];
    if (x == y) atomicOr(word, BAD_CYCLE);
    la[e] = labels - 1u - x;
    lb[e] = labels - 1u - y;
}

// ceil(log2 m): the levels of m >= 1 edges
uint32_t level_count(uint64_t m) {
    uint32_t bits = 0;
    while (bits < 63 && (1ull << bits) < m) ++bits;
    return bits;
}

// The dendrogram of m >= 1 edges over n >= 2 vertices, m <= n - 1 <= 2^31 - 2; d_a, d_b are device memory (host_in: host memory,
// checked by the caller).  host_out: the out arrays are host memory.  The device of the call is current.  Waits for the stream.
int dendrogram_of_edges(uint64_t n, uint64_t m, const uint32_t* a, const uint32_t* b, bool host_in, bool host_out, uint32_t* out_left,
                        uint32_t* out_right, uint32_t* out_size, hipStream_t stream, std::string& err) {
    const uint64_t labels = n + m;  // below 2^32
    DevMem mem;
    Drain drain{stream};
    // la, lb (m words each), parent, top, wsum, w (n + m words each), the word
    uint32_t *la, *lb, *parent, *top, *wsum, *w, *d_word;
    ScratchLayout lay;
    lay.arrays(m, la, lb);
    lay.arrays(labels, parent, top, wsum, w);
    lay.array(d_word, 64);
    const int rc = alloc_layout("forest dendrogram", mem, lay, err);
    if (rc != OK) return rc;
    uint32_t* size = top;  // (free once the last level is done; m <= n + m words)
    const uint32_t n32 = (uint32_t)n, m32 = (uint32_t)m, l32 = (uint32_t)labels;

    HIP_TRY(hipMemsetAsync(d_word, 0, 4, stream));
    if (host_in) {
        HIP_TRY(hipMemcpyAsync(la, a, m * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(lb, b, m * 4, hipMemcpyHostToDevice, stream));
        a = la;
        b = lb;
    }
    hipLaunchKernelGGL(dn_check_kernel, grid_of(labels), dim3(256), 0, stream, a, b, n32, m32, l32, la, lb, w, d_word);
    HIP_TRY(hipGetLastError());
    for (uint32_t level = level_count(m); level >= 1; --level) {
        const uint32_t h = 1u << (level - 1);
        hipLaunchKernelGGL(dn_init_kernel, grid_of(labels), dim3(256), 0, stream, parent, top, l32);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(dn_unite_kernel, grid_of(m), dim3(256), 0, stream, la, lb, m32, h, parent);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(cc_compress_kernel, grid_of(labels), dim3(256), 0, stream, parent, l32, wsum);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(wsum, 0, labels * 4, stream));
        hipLaunchKernelGGL(dn_top_kernel, grid_of(m), dim3(256), 0, stream, la, m32, h, parent, top);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(dn_sum_kernel, grid_of((labels + SUM_CHUNKS - 1) / SUM_CHUNKS), dim3(256), 0, stream, parent, top, w, l32, wsum);  // (a block: SUM_CHUNKS x 256)
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(dn_weight_kernel, grid_of(labels), dim3(256), 0, stream, parent, top, wsum, m32, l32, w);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(dn_relabel_kernel, grid_of(m), dim3(256), 0, stream, parent, top, m32, h, la, lb);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(dn_size_kernel, grid_of(m), dim3(256), 0, stream, la, lb, w, m32, l32, size, d_word);
    HIP_TRY(hipGetLastError());
    uint32_t word = 0;
    HIP_TRY(hipMemcpyAsync(&word, d_word, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (word != 0u) {  // before any out slot is written
        err = std::string("forest dendrogram: ") + ((word & BAD_END)    ? "an end is not below n"
                                                    : (word & BAD_LOOP) ? "an edge joins a vertex to itself"
                                                                        : "the edges hold a cycle: an edge joins two vertices that earlier edges join");
        return ERR_ARG;
    }
    const hipMemcpyKind kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(out_left, la, m * 4, kind, stream));
    HIP_TRY(hipMemcpyAsync(out_right, lb, m * 4, kind, stream));
    HIP_TRY(hipMemcpyAsync(out_size, size, m * 4, kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

}  // namespace

// Both forest entries (capi.cpp refers to it weakly, capi_index.hpp): 1 <= m <= n - 1, n <= 2^31 - 1.  host: every array is host
// memory, and the ends have passed the same checks on the host.  Waits for `stream` before it returns.
int forest_dendrogram(const DendrogramArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const int rc = use_device_ordinal("forest dendrogram", a.device, err);
    if (rc != OK) return rc;
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    return dendrogram_of_edges(a.n, a.m, a.a, a.b, host, host, a.out_left, a.out_right, a.out_size, stream, err);
}

// Both index entries: n >= 2, core_k <= k.  The forest is graph_spanning_forest's own, written to device memory, and stays there
// for the dendrogram.  Waits for `stream` before it returns.
int graph_dendrogram(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphDendrogramArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t n = dev.view().n;
    DevMem m_forest;
    Drain drain{stream};
    ForestArgs f = a.forest;
    uint64_t edges = 0;
    f.out_n = &edges;
    int rc = OK;
    if (host) {
        ScratchLayout lay;
        lay.arrays(n - 1, f.out_a, f.out_b, f.out_w);
        rc = alloc_layout("graph dendrogram", m_forest, lay, err);
        if (rc != OK) return rc;
    }
    rc = graph_spanning_forest(dev, origin_id, f, false, stream_v, err);
    if (rc != OK) return rc;
    if (edges != 0) {
        if (edges > n - 1) {
            err = "graph dendrogram: " + std::to_string(edges) + " edges among " + std::to_string(n) + " vertices";
            return ERR_FORMAT;
        }
        rc = dendrogram_of_edges(n, edges, f.out_a, f.out_b, false, host, a.out_left, a.out_right, a.out_size, stream, err);
        if (rc != OK) return rc == ERR_ARG ? ERR_FORMAT : rc;  // (a forest of this library's own: an internal error)
        if (host) {
            HIP_TRY(hipMemcpyAsync(a.forest.out_a, f.out_a, edges * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(a.forest.out_b, f.out_b, edges * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(a.forest.out_w, f.out_w, edges * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
    }
    *a.forest.out_n = edges;
    return OK;
}

}  // namespace hnswgpu
