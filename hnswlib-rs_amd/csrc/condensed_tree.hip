// condensed_tree.hip -- HDBSCAN on the device (gfx950 only): the condensed tree of a forest's single-linkage dendrogram, the
// stabilities of its clusters, the selection (excess of mass, or the leaves) and the flat labels: the device side of
// hnswhdb_forest(_device) and hnswhdb_graph(_device) of include/hnsw_mi355x_hdbscan.h, which holds the contract word for word
// (the entries and every check that needs no device are in capi.cpp).  DESIGN.md "HDBSCAN".
//
// The dendrogram is dendrogram.hip's, made by forest_dendrogram / graph_dendrogram on device buffers: node x < n is a vertex, node
// n + e the cluster of edge e, N = n + m nodes.  A node is BIG iff it holds mcs vertices or more.  A big node is a HEAD -- the first
// node of a cluster of the condensed tree -- iff its sibling is big too, or it is one of two or more big dendrogram roots; every
// other big node continues the cluster of its parent (a lone big dendrogram root: cluster 0).
//   hd_descent_kernel    one thread per edge: weights that descend under dist_order_bits set a word
//   hd_parent_kernel     one thread per edge: par[left[e]] = par[right[e]] = n + e (par is 0xFF.. before: "no parent")
//   hd_root_kernel       one thread per node: its union-find word is itself; a big node without a parent counts into a word
//   hd_class_kernel      one thread per node: the head flag, by slot; and the CHAINS by the union-find of union_find.hpp over the
//                        slots N - 1 - x (a parent node has the smaller slot, so the top of a chain is its root): x joins par[x]
//                        when both are small (the small subtrees), or when x is big and no head (the cluster chains).  A big node
//                        never joins a small one: one parent array serves both families.
//   cc_compress_kernel   every node's word = the top of its chain: what an O(depth) walk would find (a path has depth n - 1)
//   rocPRIM scan         of the head flags in slot order: the head x is cluster 1 + scan[slot], so a parent cluster has the smaller
//                        index.  K = 1 + the total, read back together with the descent word.
//   hd_cluster_kernel    one thread per head: parent, birth and size of its cluster, its row in the parent (key = the parent, f64
//                        term), max of the parent's lambda bits, min and max of the parent's child indices -- integer atomics
//   hd_point_kernel      one thread per vertex: the top t of its small subtree leaves the cluster of par[t] at w[par[t] - n]
//                        (no parent: cluster 0, +inf): point_cluster, point_w, its row, the max of the lambda bits
//   rocPRIM radix sort   of the n + K - 1 rows (cluster, term) by cluster; stable, so a cluster's terms stand in row order
//   hd_segment_kernel    where each cluster's rows begin and end
//   hd_stability_kernel  a block per cluster: thread t sums the terms t, t + 256, .. in order, then a tree over the 256 sums in
//                        LDS.  The shape is a function of the segment alone: two calls give the same bytes.
//   select_clusters      the selection (excess of mass, or the leaves), the labels' numbers and per vertex label and probability:
//                        cluster_select.hip's, through cluster_tree.hpp, with the options off -- no single cluster, no epsilon, no
//                        size limit, no score.  This library's own tree needs no check.  L is read back at the end.
// Every loop ends: cc_find / cc_unite descend strictly, the selection's climb goes to a smaller cluster index each step, its
// doubling rounds are counted.  No wavefront waits on another; no floating-point atomic; everything is a function of the input.
// Everything is computed into scratch, and the out arrays are written at the very end: a refusal touches none of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "cluster_tree.hpp"
#include "graph_internal.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"
// (the CSR validation kernels that come with the union-find have no caller in this unit)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "union_find.hpp"
#pragma clang diagnostic pop

namespace hnswgpu {
namespace {

constexpr uint32_t W_DESCENT = 0, W_BIGROOTS = 1;  // the words of a call

// a row's term: three separate f64 operations (the unit is compiled with -ffp-contract=off); equal lambdas give 0 (inf - inf too)
__device__ __forceinline__ double row_term(double l_row, double l_birth, uint32_t size) {
    if (l_row == l_birth) return 0.0;
    const double d = l_row - l_birth;
    return d * (double)size;
}

__device__ __forceinline__ uint32_t node_size(const uint32_t* __restrict__ size, uint32_t n, uint32_t x) { return x < n ? 1u : size[x - n]; }

// one thread per edge from 1 on
__global__ __launch_bounds__(256) void hd_descent_kernel(const float* __restrict__ w, uint32_t m, uint32_t* __restrict__ words) {
    const uint64_t e = thread_number() + 1u;
    if (e >= m) return;
    if (dist_order_bits(w[e - 1u]) > dist_order_bits(w[e])) atomicOr(words + W_DESCENT, 1u);
}

// one thread per edge.  A dendrogram names every node at most once as a child; an id that is not below N (never one of
// dendrogram.hip's) is left out.
__global__ __launch_bounds__(256) void hd_parent_kernel(const uint32_t* __restrict__ left, const uint32_t* __restrict__ right, uint32_t n, uint32_t m,
                                                       uint32_t* __restrict__ par) {
    const uint64_t e = thread_number();
    if (e >= m) return;
    const uint32_t l = left[e], r = right[e], nodes = n + m;
    if (l < nodes) par[l] = n + (uint32_t)e;
    if (r < nodes) par[r] = n + (uint32_t)e;
}

// one thread per node
__global__ __launch_bounds__(256) void hd_root_kernel(const uint32_t* __restrict__ par, const uint32_t* __restrict__ size, uint32_t n, uint32_t nodes,
                                                     uint32_t mcs, uint32_t* __restrict__ uf, uint32_t* __restrict__ words) {
    const uint64_t x = thread_number();
    if (x >= nodes) return;
    uf[nodes - 1u - (uint32_t)x] = nodes - 1u - (uint32_t)x;
    if (par[x] == NONE && node_size(size, n, (uint32_t)x) >= mcs) atomicAdd(words + W_BIGROOTS, 1u);
}

// nodes + 1 threads: one per node, and one for the flag behind the last slot, which the scan reads.  par[x] is NONE or in [n, N).
__global__ __launch_bounds__(256) void hd_class_kernel(const uint32_t* __restrict__ par, const uint32_t* __restrict__ left,
                                                      const uint32_t* __restrict__ right, const uint32_t* __restrict__ size, uint32_t n, uint32_t nodes,
                                                      uint32_t mcs, const uint32_t* __restrict__ words, uint32_t* uf, uint32_t* __restrict__ headflag) {
    const uint64_t t = thread_number();
    if (t > nodes) return;
    if (t == nodes) {
        headflag[nodes] = 0u;
        return;
    }
    const uint32_t x = (uint32_t)t, p = par[x];
    const bool big = node_size(size, n, x) >= mcs;
    bool head = false;
    if (p == NONE) {
        head = big && words[W_BIGROOTS] >= 2u;
    } else {
        const uint32_t e = p - n, l = left[e], sib = l == x ? right[e] : l;
        if (big) head = sib < nodes && node_size(size, n, sib) >= mcs;
        const bool parent_big = size[e] >= mcs;
        if (big ? !head : !parent_big) cc_unite(uf, nodes - 1u - x, nodes - 1u - p);
    }
    headflag[nodes - 1u - x] = head ? 1u : 0u;
}

#include "union_find_compress.inc"

// what the kernels below read of the classes: uf is compressed, hscan the exclusive scan of headflag
struct Classes {
    const uint32_t* par;
    const uint32_t* size;
    const float* w;
    const uint32_t* uf;
    const uint32_t* headflag;
    const uint32_t* hscan;
    uint32_t n, nodes;
};

// the cluster that the big node y lies in and the stored bits of that cluster's birth weight
__device__ __forceinline__ void cluster_of_big(const Classes& k, uint32_t y, uint32_t& c, uint32_t& birth) {
    const uint32_t top_slot = k.uf[k.nodes - 1u - y];
    if (k.headflag[top_slot] == 0u) {  // the chain ends in the one big dendrogram root: cluster 0
        c = 0u;
        birth = INF_BITS;
        return;
    }
    c = 1u + k.hscan[top_slot];
    const uint32_t p = k.par[k.nodes - 1u - top_slot];
    birth = p == NONE ? INF_BITS : __float_as_uint(k.w[p - k.n]);
}

// the per-cluster arrays, `slots` of each
struct Clusters {
    uint32_t* parent;
    uint32_t* birth;
    uint32_t* size;
    uint32_t* child_lo;  // 0xFF.. before
    uint32_t* child_hi;  // 0 before: a child's index is 1 or more
    unsigned long long* maxlam;
    uint32_t slots;
};

// nodes + 1 threads: one per node (the heads work), and one for cluster 0.  rows: the vertices' first, then cluster c's at n + c - 1.
__global__ __launch_bounds__(256) void hd_cluster_kernel(Classes k, Clusters cl, uint32_t* __restrict__ row_key, double* __restrict__ row_term_out) {
    const uint64_t t = thread_number();
    if (t > k.nodes) return;
    if (t == k.nodes) {
        cl.parent[0] = NONE;
        cl.birth[0] = INF_BITS;
        cl.size[0] = k.n;
        return;
    }
    const uint32_t x = (uint32_t)t, slot = k.nodes - 1u - x;
    if (k.headflag[slot] == 0u) return;
    const uint32_t c = 1u + k.hscan[slot];
    if (c >= cl.slots) return;  // (never: K is within the bound, checked by the host before this launch)
    const uint32_t p = k.par[x], sz = node_size(k.size, k.n, x);
    uint32_t cp = 0u, parent_birth = INF_BITS, birth = INF_BITS;
    if (p != NONE) {
        cluster_of_big(k, p, cp, parent_birth);
        birth = __float_as_uint(k.w[p - k.n]);
    }
    cl.parent[c] = cp;
    cl.birth[c] = birth;
    cl.size[c] = sz;
    const double lam = lambda_of(birth);
    row_key[k.n + c - 1u] = cp;
    row_term_out[k.n + c - 1u] = row_term(lam, lambda_of(parent_birth), sz);
    raise_lambda(cl.maxlam, cp, lam);
    atomicMin(cl.child_lo + cp, c);
    atomicMax(cl.child_hi + cp, c);
}

// one thread per vertex (a vertex is small: mcs >= 2)
__global__ __launch_bounds__(256) void hd_point_kernel(Classes k, Clusters cl, uint32_t* __restrict__ point_cluster, uint32_t* __restrict__ point_w,
                                                      uint32_t* __restrict__ row_key, double* __restrict__ row_term_out) {
    const uint64_t t = thread_number();
    if (t >= k.n) return;
    const uint32_t v = (uint32_t)t, top = k.nodes - 1u - k.uf[k.nodes - 1u - v], p = k.par[top];
    uint32_t c = 0u, birth = INF_BITS, pw = INF_BITS;
    if (p != NONE) {
        cluster_of_big(k, p, c, birth);
        pw = __float_as_uint(k.w[p - k.n]);
    }
    if (c >= cl.slots) c = 0u;  // (never)
    point_cluster[v] = c;
    point_w[v] = pw;
    const double lam = lambda_of(pw);
    row_key[v] = c;
    row_term_out[v] = row_term(lam, lambda_of(birth), 1u);
    raise_lambda(cl.maxlam, c, lam);
}

// one thread per sorted row; keys are below K
__global__ __launch_bounds__(256) void hd_segment_kernel(const uint32_t* __restrict__ key, uint32_t rows, uint32_t clusters, uint32_t* __restrict__ seg_begin,
                                                        uint32_t* __restrict__ seg_end) {
    const uint64_t i = thread_number();
    if (i >= rows) return;
    const uint32_t c = key[i];
    if (c >= clusters) return;  // (never)
    if (i == 0u || key[i - 1u] != c) seg_begin[c] = (uint32_t)i;
    if (i + 1u == rows || key[i + 1u] != c) seg_end[c] = (uint32_t)i + 1u;
}

// a block per cluster
__global__ __launch_bounds__(256) void hd_stability_kernel(const double* __restrict__ term, const uint32_t* __restrict__ seg_begin,
                                                          const uint32_t* __restrict__ seg_end, double* __restrict__ stability) {
    __shared__ double part[256];
    const uint32_t c = blockIdx.x;
    const uint64_t lo = seg_begin[c], hi = seg_end[c];
    double s = 0.0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u) s += term[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t h = 128u; h >= 1u; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0u) stability[c] = part[0];
}

// a scan that has ended when this returns (its temporary storage goes here)
int scan_u32(const uint32_t* in, uint32_t* out, uint64_t count, hipStream_t stream, std::string& err) {
    DevMem temp;
    const int rc = exclusive_scan_u32(temp, in, out, count, stream, err);
    if (rc != OK) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// hnswhdb_max_clusters for n <= 2^31 - 1, mcs >= 2: leaf clusters are disjoint and hold mcs vertices or more
uint64_t max_clusters(uint64_t n, uint64_t mcs) { return n / mcs == 0 ? 1 : 2 * (n / mcs) - 1; }

// The clusters of the dendrogram (left, right, size) of m edges with weights w over n >= 1 vertices, all device memory; m == 0: no
// array is read.  n + m < 2^32, 2 <= mcs < 2^31.  host_out: the out arrays are host memory.  The device of the call is current.
// ERR_ARG, nothing written, when the weights descend.  Waits for the stream.
int clusters_of_dendrogram(const char* what, uint64_t n, uint64_t m, const float* w, const uint32_t* left, const uint32_t* right, const uint32_t* size,
                           uint64_t mcs, uint32_t method, const HdbscanOut& out, bool host_out, hipStream_t stream, std::string& err) {
    const uint64_t nodes = n + m, slots = max_clusters(n, mcs), rows_max = n + slots - 1;
    const uint32_t n32 = (uint32_t)n, m32 = (uint32_t)m, nodes32 = (uint32_t)nodes, mcs32 = (uint32_t)mcs;
    DevMem mem;
    Drain drain{stream};
    // per node, per vertex, per row (twice: the sort's two sides), per cluster
    uint32_t *words, *par, *uf, *mark, *headflag, *hscan, *point_cluster, *point_w, *key_in, *key_out;
    double *term_in, *term_out, *stability;
    uint32_t *c_parent, *c_birth, *c_size, *child_lo, *child_hi, *seg_begin, *seg_end;
    unsigned long long* maxlam;
    const SelectOptions opt{method, 0u, 0.0f, 0u};  // the first selection: no single cluster, no epsilon, no size limit
    SelectScratch sel;
    ScratchLayout lay;
    lay.array(words, 64);
    lay.arrays(nodes, par, uf, mark);
    lay.arrays(nodes + 1, headflag, hscan);
    lay.arrays(n, point_cluster, point_w);
    lay.arrays(rows_max, key_in, key_out, term_in, term_out);
    lay.arrays(slots, c_parent, c_birth, c_size, child_lo);
    // those that are 0 before their kernels stand together, from child_hi on
    const uint64_t zeroed_from = lay.size();
    lay.arrays(slots, child_hi, seg_begin, seg_end, maxlam);
    sel.zeroed(lay, slots);
    const uint64_t zeroed_bytes = lay.size() - zeroed_from;
    lay.array(stability, slots);
    sel.rest(lay, n, slots, opt, false);
    int rc = alloc_layout(what, mem, lay, err);  // (before anything is written)
    if (rc != OK) return rc;
    uint32_t* zeroed = child_hi;

    HIP_TRY(hipMemsetAsync(words, 0, 256, stream));
    HIP_TRY(hipMemsetAsync(par, 0xFF, nodes * 4, stream));
    HIP_TRY(hipMemsetAsync(child_lo, 0xFF, slots * 4, stream));
    HIP_TRY(hipMemsetAsync(zeroed, 0, zeroed_bytes, stream));
    if (m != 0) {
        if (m > 1) {
            hipLaunchKernelGGL(hd_descent_kernel, grid_of(m - 1), dim3(256), 0, stream, w, m32, words);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(hd_parent_kernel, grid_of(m), dim3(256), 0, stream, left, right, n32, m32, par);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(hd_root_kernel, grid_of(nodes), dim3(256), 0, stream, par, size, n32, nodes32, mcs32, uf, words);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hd_class_kernel, grid_of(nodes + 1), dim3(256), 0, stream, par, left, right, size, n32, nodes32, mcs32, words, uf, headflag);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cc_compress_kernel, grid_of(nodes), dim3(256), 0, stream, uf, nodes32, mark);
    HIP_TRY(hipGetLastError());
    rc = scan_u32(headflag, hscan, nodes + 1, stream, err);
    if (rc != OK) return rc;
    uint32_t descent = 0, heads = 0;
    HIP_TRY(hipMemcpyAsync(&descent, words + W_DESCENT, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&heads, hscan + nodes, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (descent != 0u) {
        err = std::string(what) + ": the weights descend: the edges' order is the merge order, ascending by weight";
        return ERR_ARG;
    }
    const uint64_t clusters = 1 + (uint64_t)heads, rows = n + clusters - 1;
    if (clusters > slots) {
        err = std::string(what) + ": " + std::to_string(clusters) + " clusters, above the bound " + std::to_string(slots);
        return ERR_FORMAT;
    }
    const uint32_t k32 = (uint32_t)clusters;
    const Classes cls{par, size, w, uf, headflag, hscan, n32, nodes32};
    const Clusters cl{c_parent, c_birth, c_size, child_lo, child_hi, maxlam, k32};
    hipLaunchKernelGGL(hd_cluster_kernel, grid_of(nodes + 1), dim3(256), 0, stream, cls, cl, key_in, term_in);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hd_point_kernel, grid_of(n), dim3(256), 0, stream, cls, cl, point_cluster, point_w, key_in, term_in);
    HIP_TRY(hipGetLastError());
    {
        uint32_t end_bit = 1;
        while (end_bit < 32 && (1ull << end_bit) < clusters) ++end_bit;
        DevMem temp;
        rc = radix_sort_pairs(temp, key_in, key_out, term_in, term_out, (size_t)rows, end_bit, stream, err);
        if (rc != OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
    }
    hipLaunchKernelGGL(hd_segment_kernel, grid_of(rows), dim3(256), 0, stream, key_out, (uint32_t)rows, k32, seg_begin, seg_end);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hd_stability_kernel, dim3(k32), dim3(256), 0, stream, term_out, seg_begin, seg_end, stability);
    HIP_TRY(hipGetLastError());
    const ClusterTree tree{c_parent, c_birth, c_size, stability, point_cluster, point_w, n32, k32};
    uint32_t n_labels = 0;
    rc = select_clusters(tree, ClusterKids{child_lo, child_hi, maxlam}, opt, sel, &n_labels, stream, err);
    if (rc != OK) return rc;
    rc = copy_out({{out.labels, sel.labels, n * 4}, {out.prob, sel.prob, n * 4}, {out.point_cluster, point_cluster, n * 4}, {out.point_w, point_w, n * 4},
                   {out.cluster_parent, c_parent, clusters * 4}, {out.cluster_birth_w, c_birth, clusters * 4}, {out.cluster_size, c_size, clusters * 4},
                   {out.stability, stability, clusters * 8}, {out.selected, sel.selected, clusters}},
                  host_out, stream, err);
    if (rc != OK) return rc;
    *out.n_clusters = clusters;
    *out.n_labels = n_labels;
    return OK;
}

}  // namespace

// Both forest entries (capi.cpp refers to it weakly, capi_index.hpp): n >= 1, m <= n - 1, n <= 2^31 - 1, 2 <= mcs <= 2^31 - 1.
// host: every array is host memory, and the ends and weights have passed the same checks on the host.  Waits for `stream`.
int forest_hdbscan(const ForestHdbscanArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = use_device_ordinal("forest hdbscan", a.device, err);
    if (rc != OK) return rc;
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    DevMem mem;
    Drain drain{stream};
    const uint32_t *d_a = a.a, *d_b = a.b;
    const float* d_w = a.w;
    uint32_t *left = nullptr, *right = nullptr, *size = nullptr;
    if (a.m != 0) {
        // the dendrogram; behind it, for the host form, the forest
        Uploads ups;
        ScratchLayout lay;
        lay.arrays(a.m, left, right, size);
        if (host) ups.brings(lay, a.m, d_a, d_b, d_w);
        rc = alloc_layout("forest hdbscan", mem, lay, err);
        if (rc != OK) return rc;
        rc = copy_uploads(ups, stream, err);
        if (rc != OK) return rc;
        const DendrogramArgs d{a.device, a.n, a.m, d_a, d_b, left, right, size};
        rc = forest_dendrogram(d, false, stream_v, err);  // a bad end, a self-loop, a cycle: its refusals, in its words
        if (rc != OK) return rc;
    }
    return clusters_of_dendrogram("forest hdbscan", a.n, a.m, d_w, left, right, size, a.min_cluster_size, a.method, a.out, host, stream, err);
}

// Both index entries: at least one point, core_k <= k.  The forest and the dendrogram are graph_dendrogram's own, written to device
// memory, and stay there; what the caller asked to see of them is copied out at the end.  Waits for `stream`.
int graph_hdbscan(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphHdbscanArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t n = dev.view().n;
    if (n > 0x7FFFFFFFull) {
        err = "graph hdbscan: " + std::to_string(n) + " points, above 2^31 - 1";
        return ERR_ARG;
    }
    const uint64_t most = std::max<uint64_t>(n, 2) - 1;  // the edges of a forest at most
    DevMem mem;
    Drain drain{stream};
    uint32_t *f_a, *f_b, *left, *right, *size;
    float* f_w;
    ScratchLayout lay;
    lay.arrays(most, f_a, f_b, f_w, left, right, size);
    int rc = alloc_layout("graph hdbscan", mem, lay, err);
    if (rc != OK) return rc;
    uint64_t edges = 0;
    if (n >= 2) {
        GraphDendrogramArgs g{a.forest, left, right, size};
        g.forest.out_a = f_a;
        g.forest.out_b = f_b;
        g.forest.out_w = f_w;
        g.forest.out_n = &edges;
        rc = graph_dendrogram(dev, origin_id, g, false, stream_v, err);
        if (rc != OK) return rc;
    }
    rc = clusters_of_dendrogram("graph hdbscan", n, edges, f_w, left, right, size, a.min_cluster_size, a.method, a.out, host, stream, err);
    if (rc != OK) return rc == ERR_ARG ? ERR_FORMAT : rc;  // (a forest of this library's own: an internal error)
    const uint64_t bytes = edges * 4;
    rc = copy_out({{a.forest.out_a, f_a, bytes}, {a.forest.out_b, f_b, bytes}, {a.forest.out_w, f_w, bytes}, {a.out_left, left, bytes},
                   {a.out_right, right, bytes}, {a.out_size, size, bytes}},
                  host, stream, err);
    if (rc != OK) return rc;
    *a.forest.out_n = edges;
    return OK;
}

}  // namespace hnswgpu
