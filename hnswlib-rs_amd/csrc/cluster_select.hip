// cluster_select.hip -- HDBSCAN's second stage on the device (gfx950 only): from a condensed tree that condensed_tree.hip wrote, the
// selection under allow_single_cluster, cluster_selection_epsilon and max_cluster_size, the flat labels and probabilities and the
// GLOSH outlier scores: the device side of hnswhds_select(_device) of include/hnsw_mi355x_hdbscan_select.h, which holds the contract
// word for word (the entries and the host form's checks are in capi.cpp).  DESIGN.md "HDBSCAN: selection options and GLOSH".
// This unit also OWNS THE SELECTION for all three stages: the kernels below tree_jump_init_kernel are launched by the host functions
// that cluster_tree.hpp declares -- select_clusters (this unit after its checks, and condensed_tree.hip with the options off),
// flagged_ancestors and number_selected (cluster_predict.hip too).  What a tree is, and every device helper, is in that header.
//
//   cs_check_kernel      one thread per cluster and per vertex, BEFORE ANY TRAVERSAL: the shared checks of cluster_tree.hpp, and a
//                        stability is neither NaN nor negative.  An index that passes is used at once: a child counts into its
//                        parent (count, min and max of the child indices) -- integer atomics.
//   cs_kids_kernel       one thread per cluster: a cluster other than 0 has no child or two, else a bit of the word.  The word is
//                        read back: with a bit set the call ends here, ERR_ARG.  From here on parent[] is a tree under cluster 0.
//   tree_climb_kernel    one thread per leaf cluster, ONE launch: it stores its S and its death, fences and adds 1 to its parent's
//                        arrival counter.  The first arriver leaves; the second fences, loads both children's S and death
//                        (agent-scope loads), decides the parent -- stability >= S + S and the size test -- and goes on upwards.
//                        Nobody waits.  A cluster other than 0 has no child or two, so the sum is one add.  Children of cluster 0 go
//                        no further.  (HNSWGPU_SELECT_LEAF: a leaf wins, and the climb carries the deaths alone.)
//   tree_root_kernel     ONE block: thread t adds S of the children of 0 whose index is t modulo 256 in ascending index, then a
//                        tree over the 256 sums in LDS (the shape of condensed_tree.hip's hd_stability_kernel): sub(0), a function
//                        of the input alone.  death(0) is a max over the same children.  Cluster 0 wins or not.
//   tree_jump_*_kernel   the pointer doubling of cluster_tree.hpp.  Run on the winners, HIGHEST, it gives E (best[c] == c).
//   tree_end_*_kernel    the epsilon climb as pointer doubling: a cluster whose climb ends in one step holds its end, every other
//                        one its parent; a round replaces "go on from p" by what p holds.
//   tree_f_kernel        one thread per cluster: a member of E marks its end (or itself): F.  The doubling once more on F gives
//                        E' (best[c] == c) and for every cluster its member of E', which is unique: E' is an antichain.
//   tree_flag_kernel     selected, and the flags that rocPRIM scans into the labels' numbers.  L is read back at the end.
//   tree_vertex_kernel   one thread per vertex: label, probability -- with the single-root threshold branch -- and GLOSH score
// Every loop ends: the climb goes to a strictly smaller index each step, checked in the loop; the doubling rounds are counted.  No
// wavefront waits on another; no floating-point atomic; everything is a function of the input.  Everything is computed into scratch,
// and the out arrays are written at the very end: a refusal touches none of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "cluster_tree.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"

namespace hnswgpu {
namespace {

// what the checks gather per cluster beside the max of the lambda bits, `clusters` of each: all 0 before, child_lo 0xFF..
struct Gather {
    uint32_t* count;
    uint32_t* child_lo;
    uint32_t* child_hi;
    unsigned long long* maxlam;
};

// clusters + n threads: the clusters first
__global__ __launch_bounds__(256) void cs_check_kernel(ClusterTree t, Gather g, uint32_t* __restrict__ word) {
    const uint64_t i = thread_number();
    if (i >= (uint64_t)t.clusters + t.n) return;
    if (i >= t.clusters) {
        check_vertex(t.point_cluster, t.point_w, i - t.clusters, t.clusters, g.maxlam, word);
        return;
    }
    const uint32_t c = (uint32_t)i;
    if (!(t.stability[c] >= 0.0)) atomicOr(word, (uint32_t)BAD_STABILITY);  // a NaN too
    if (!check_cluster(t.parent, t.birth, c, g.maxlam, word)) return;
    const uint32_t p = t.parent[c];
    if (p != 0u) {  // (cluster 0 may have any number of children, and nobody asks for their ends)
        atomicAdd(g.count + p, 1u);
        atomicMin(g.child_lo + p, c);
        atomicMax(g.child_hi + p, c);
    }
}

// one thread per cluster from 1 on
__global__ __launch_bounds__(256) void cs_kids_kernel(const uint32_t* __restrict__ count, uint32_t clusters, uint32_t* __restrict__ word) {
    const uint64_t c = thread_number() + 1u;
    if (c >= clusters) return;
    if (count[c] != 0u && count[c] != 2u) atomicOr(word, (uint32_t)BAD_KIDS);
}

__device__ __forceinline__ bool size_fits(const SelectOptions& o, uint32_t size) { return o.max_size == 0u || (uint64_t)size <= o.max_size; }

// one thread per cluster; arrive, wins: 0 before.  The climb goes to a smaller index each step and leaves at a child of cluster 0.
__global__ __launch_bounds__(256) void tree_climb_kernel(ClusterTree t, ClusterKids k, SelectOptions o, uint32_t* arrive, unsigned long long* s_of,
                                                        unsigned long long* death, uint32_t* __restrict__ wins) {
    const uint64_t i = thread_number();
    if (i == 0u || i >= t.clusters) return;
    uint32_t cur = (uint32_t)i;
    if (k.child_hi[cur] != 0u) return;  // not a leaf
    {
        const double own = t.stability[cur];
        const bool win = o.method == HNSWGPU_SELECT_LEAF || size_fits(o, t.size[cur]);  // (own >= 0, the empty sum)
        wins[cur] = win ? 1u : 0u;
        publish_f64(s_of, cur, win ? own : 0.0);
        publish_f64(death, cur, f64_of(k.maxlam[cur]));
    }
    for (;;) {
        const uint32_t p = t.parent[cur];
        if (p == 0u || p >= cur) return;  // (p >= cur: never, the tree has passed its checks or is this library's own)
        __threadfence();  // my S and death before my arrival
        if (__hip_atomic_fetch_add(arrive + p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;  // the sibling's subtree is still to come
        __threadfence();  // the sibling's arrival before its S and death
        const uint32_t lo = k.child_lo[p], hi = k.child_hi[p];
        if (lo >= t.clusters || hi >= t.clusters) return;  // (never)
        const double sum = fetch_f64(s_of, lo) + fetch_f64(s_of, hi), own = t.stability[p];
        const bool win = o.method == HNSWGPU_SELECT_EOM && own >= sum && size_fits(o, t.size[p]);  // a tie goes to the parent
        wins[p] = win ? 1u : 0u;
        publish_f64(s_of, p, win ? own : sum);
        publish_f64(death, p, fmax(f64_of(k.maxlam[p]), fmax(fetch_f64(death, lo), fetch_f64(death, hi))));
        cur = p;
    }
}

// ONE block.  The children of 0 hold their S and death (a kernel before this one wrote them).
__global__ __launch_bounds__(256) void tree_root_kernel(ClusterTree t, ClusterKids k, SelectOptions o, const unsigned long long* __restrict__ s_of,
                                                       unsigned long long* death, uint32_t* __restrict__ wins) {
    __shared__ double part[256];
    __shared__ double high[256];
    double s = 0.0, d = 0.0;
    for (uint64_t c = threadIdx.x; c < t.clusters; c += 256u) {
        if (t.parent[c] != 0u) continue;  // (parent[0] is NONE)
        s += f64_of(s_of[c]);
        d = fmax(d, f64_of(death[c]));
    }
    part[threadIdx.x] = s;
    high[threadIdx.x] = d;
    __syncthreads();
    for (uint32_t h = 128u; h >= 1u; h >>= 1) {
        if (threadIdx.x < h) {
            part[threadIdx.x] += part[threadIdx.x + h];
            high[threadIdx.x] = fmax(high[threadIdx.x], high[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x != 0u) return;
    bool win = o.allow_single != 0u;
    if (o.method == HNSWGPU_SELECT_EOM) win = win && t.stability[0] >= part[0] && size_fits(o, t.size[0]);
    else win = win && t.clusters == 1u;
    wins[0] = win ? 1u : 0u;
    death[0] = (unsigned long long)__double_as_longlong(fmax(f64_of(k.maxlam[0]), high[0]));
}

// (jump << 32) | best: jump is the parent, NONE above cluster 0 (parent[0] is NONE); best is c itself where its flag is set
template <typename Flag>
__global__ __launch_bounds__(256) void tree_jump_init_kernel(const uint32_t* __restrict__ parent, const Flag* __restrict__ flag, uint32_t clusters,
                                                            uint64_t* __restrict__ state) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    state[c] = ((uint64_t)(c == 0u ? NONE : parent[c]) << 32) | (flag[c] != 0u ? (uint32_t)c : NONE);
}

template <bool NEAREST>
__global__ __launch_bounds__(256) void tree_jump_round_kernel(const uint64_t* __restrict__ from, uint32_t clusters, uint64_t* __restrict__ to) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    uint64_t mine = from[c];
    const uint32_t j = (uint32_t)(mine >> 32);
    if (j < clusters) {  // (NONE is not)
        const uint64_t above = from[j];
        // of the two stretches the one that goes first: the higher one, or the nearer one
        const uint32_t first = NEAREST ? (uint32_t)mine : (uint32_t)above, second = NEAREST ? (uint32_t)above : (uint32_t)mine;
        mine = (above & 0xFFFFFFFF00000000ull) | (first != NONE ? first : second);
    }
    to[c] = mine;
}

// The epsilon climb from c != 0, one step: with p = parent(c), p == 0 ends it at 0 (allow_single_cluster) or at c; birth_w(p) > eps
// ends it at p; otherwise it goes on from p.  (jump << 32) | end: jump NONE where the end is known, else end NONE.
__global__ __launch_bounds__(256) void tree_end_init_kernel(ClusterTree t, SelectOptions o, uint64_t* __restrict__ state) {
    const uint64_t i = thread_number();
    if (i >= t.clusters) return;
    const uint32_t c = (uint32_t)i;
    if (c == 0u) {
        state[0] = ((uint64_t)NONE << 32) | 0u;
        return;
    }
    const uint32_t p = t.parent[c];
    uint64_t mine;
    if (p == 0u || p >= c) mine = ((uint64_t)NONE << 32) | (o.allow_single != 0u && p == 0u ? 0u : c);  // (p >= c: never)
    else if (weight_value(t.birth[p]) > o.eps) mine = ((uint64_t)NONE << 32) | p;
    else mine = ((uint64_t)p << 32) | NONE;
    state[c] = mine;
}

__global__ __launch_bounds__(256) void tree_end_round_kernel(const uint64_t* __restrict__ from, uint32_t clusters, uint64_t* __restrict__ to) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    const uint64_t mine = from[c];
    const uint32_t j = (uint32_t)(mine >> 32);
    to[c] = j < clusters ? from[j] : mine;
}

// one thread per cluster; fflag: 0 before.  top: the doubling's state over the winners; ends: over the epsilon climb.
__global__ __launch_bounds__(256) void tree_f_kernel(ClusterTree t, SelectOptions o, const uint64_t* __restrict__ top, const uint64_t* __restrict__ ends,
                                                    uint32_t* __restrict__ fflag) {
    const uint64_t i = thread_number();
    if (i >= t.clusters) return;
    const uint32_t c = (uint32_t)i;
    if ((uint32_t)top[c] != c) return;  // not in E
    uint32_t f = c;
    if (c != 0u && weight_value(t.birth[c]) < o.eps) {  // (c == 0: E is {0}, and stays)
        const uint32_t e = (uint32_t)ends[c];
        if (e < t.clusters) f = e;  // (always)
    }
    fflag[f] = 1u;  // (several members may end at one cluster: they store the same word)
}

// clusters + 1 threads: one per cluster, and one for the flag behind the last, which the scan reads.  selected may be nullptr.
__global__ __launch_bounds__(256) void tree_flag_kernel(const uint64_t* __restrict__ state, uint32_t clusters, uint8_t* __restrict__ selected,
                                                       uint32_t* __restrict__ selflag) {
    const uint64_t c = thread_number();
    if (c > clusters) return;
    const bool sel = c < clusters && (uint32_t)state[c] == (uint32_t)c;
    selflag[c] = sel ? 1u : 0u;
    if (c < clusters && selected != nullptr) selected[c] = sel ? 1u : 0u;
}

// one thread per vertex; score may be nullptr
__global__ __launch_bounds__(256) void tree_vertex_kernel(ClusterTree t, SelectOptions o, const uint64_t* __restrict__ state,
                                                         const uint32_t* __restrict__ label_of, const unsigned long long* __restrict__ maxlam,
                                                         const unsigned long long* __restrict__ death, int32_t* __restrict__ labels,
                                                         float* __restrict__ prob, float* __restrict__ score) {
    const uint64_t v = thread_number();
    if (v >= t.n) return;
    const uint32_t c = t.point_cluster[v];  // below K: checked, or this library's own
    const double lam = lambda_of(t.point_w[v]);
    if (score != nullptr) score[v] = glosh_score(lam, f64_of(death[c]));
    // (state[0] == 0: E' is {0}, for every vertex)
    label_of_point(lam, (uint32_t)state[c], (uint32_t)state[0] == 0u, o.eps, t.clusters, label_of, maxlam, labels[v], prob[v]);
}

}  // namespace

template <typename Flag, bool NEAREST>
int flagged_ancestors(const uint32_t* parent, const Flag* flag, uint64_t clusters, uint64_t*& state_a, uint64_t*& state_b, hipStream_t stream,
                      std::string& err) {
    hipLaunchKernelGGL(tree_jump_init_kernel<Flag>, grid_of(clusters), dim3(256), 0, stream, parent, flag, (uint32_t)clusters, state_a);
    HIP_TRY(hipGetLastError());
    for (uint64_t reach = 1; reach <= clusters; reach *= 2) {  // a cluster's depth is below K, and one jump leads past cluster 0
        hipLaunchKernelGGL(tree_jump_round_kernel<NEAREST>, grid_of(clusters), dim3(256), 0, stream, state_a, (uint32_t)clusters, state_b);
        HIP_TRY(hipGetLastError());
        std::swap(state_a, state_b);
    }
    return OK;
}
template int flagged_ancestors<uint32_t, false>(const uint32_t*, const uint32_t*, uint64_t, uint64_t*&, uint64_t*&, hipStream_t, std::string&);
template int flagged_ancestors<uint8_t, true>(const uint32_t*, const uint8_t*, uint64_t, uint64_t*&, uint64_t*&, hipStream_t, std::string&);

int number_selected(const uint64_t* state, uint64_t clusters, uint8_t* selected, uint32_t* selflag, uint32_t* label_of, DevMem& temp, hipStream_t stream,
                    std::string& err) {
    hipLaunchKernelGGL(tree_flag_kernel, grid_of(clusters + 1), dim3(256), 0, stream, state, (uint32_t)clusters, selected, selflag);
    HIP_TRY(hipGetLastError());
    return exclusive_scan_u32(temp, selflag, label_of, clusters + 1, stream, err);
}

int select_clusters(const ClusterTree& t, const ClusterKids& k, const SelectOptions& o, SelectScratch& s, uint32_t* n_labels, hipStream_t stream,
                    std::string& err) {
    const uint64_t n = t.n, clusters = t.clusters;
    if (clusters > 1) {
        hipLaunchKernelGGL(tree_climb_kernel, grid_of(clusters), dim3(256), 0, stream, t, k, o, s.arrive, s.s_of, s.death, s.wins);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(tree_root_kernel, dim3(1), dim3(256), 0, stream, t, k, o, s.s_of, s.death, s.wins);
    HIP_TRY(hipGetLastError());
    int rc = flagged_ancestors<uint32_t, false>(t.parent, s.wins, clusters, s.state_a, s.state_b, stream, err);  // E
    if (rc != OK) return rc;
    if (o.eps > 0.0f) {  // F, then E'
        hipLaunchKernelGGL(tree_end_init_kernel, grid_of(clusters), dim3(256), 0, stream, t, o, s.end_a);
        HIP_TRY(hipGetLastError());
        for (uint64_t reach = 1; reach < clusters; reach *= 2) {  // a climb has fewer than K steps
            hipLaunchKernelGGL(tree_end_round_kernel, grid_of(clusters), dim3(256), 0, stream, s.end_a, (uint32_t)clusters, s.end_b);
            HIP_TRY(hipGetLastError());
            std::swap(s.end_a, s.end_b);
        }
        hipLaunchKernelGGL(tree_f_kernel, grid_of(clusters), dim3(256), 0, stream, t, o, s.state_a, s.end_a, s.fflag);
        HIP_TRY(hipGetLastError());
        rc = flagged_ancestors<uint32_t, false>(t.parent, s.fflag, clusters, s.state_a, s.state_b, stream, err);
        if (rc != OK) return rc;
    }
    {
        DevMem temp;
        rc = number_selected(s.state_a, clusters, s.selected, s.selflag, s.label_of, temp, stream, err);
        if (rc != OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
    }
    hipLaunchKernelGGL(tree_vertex_kernel, grid_of(n), dim3(256), 0, stream, t, o, s.state_a, s.label_of, k.maxlam, s.death, s.labels, s.prob, s.score);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n_labels, s.label_of + clusters, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// Both entries (capi.cpp refers to it weakly, capi_index.hpp): 1 <= n, K <= 2^31 - 1, a known method, allow_single_cluster 0 or 1,
// eps >= 0, every needed array there.  host: every array is host memory, and has passed the same checks on the host.  Waits for
// `stream`.
int hdbscan_select(const HdbscanSelectArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    int rc = use_device_ordinal("hdbscan select", a.device, err);
    if (rc != OK) return rc;
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    const uint64_t n = a.n, clusters = a.clusters;
    const SelectOptions opt{a.method, a.allow_single_cluster, a.eps, a.max_cluster_size};
    DevMem mem;
    Drain drain{stream};
    ClusterTree t{a.cluster_parent, reinterpret_cast<const uint32_t*>(a.cluster_birth_w), a.cluster_size, a.stability, a.point_cluster,
                  reinterpret_cast<const uint32_t*>(a.point_w), (uint32_t)n, (uint32_t)clusters};
    uint32_t *word, *count, *child_lo, *child_hi;
    unsigned long long* maxlam;
    SelectScratch s;
    Uploads ups;
    ScratchLayout lay;
    lay.array(word, 64);
    lay.array(child_lo, clusters);
    // those that are 0 before their kernels stand together, from count on
    const uint64_t zeroed_from = lay.size();
    lay.arrays(clusters, count, child_hi, maxlam);
    s.zeroed(lay, clusters);
    const uint64_t zeroed_bytes = lay.size() - zeroed_from;
    s.rest(lay, n, clusters, opt, true);
    if (host) {  // the tree comes along in the block
        ups.brings(lay, clusters, t.parent, t.birth, t.size, t.stability);
        ups.brings(lay, n, t.point_cluster, t.point_w);
    }
    rc = alloc_layout("hdbscan select", mem, lay, err);  // (before anything is written)
    if (rc != OK) return rc;
    rc = copy_uploads(ups, stream, err);
    if (rc != OK) return rc;

    HIP_TRY(hipMemsetAsync(word, 0, 256, stream));
    HIP_TRY(hipMemsetAsync(child_lo, 0xFF, clusters * 4, stream));
    HIP_TRY(hipMemsetAsync(count, 0, zeroed_bytes, stream));
    hipLaunchKernelGGL(cs_check_kernel, grid_of(clusters + n), dim3(256), 0, stream, t, Gather{count, child_lo, child_hi, maxlam}, word);
    HIP_TRY(hipGetLastError());
    if (clusters > 1) {
        hipLaunchKernelGGL(cs_kids_kernel, grid_of(clusters - 1), dim3(256), 0, stream, count, (uint32_t)clusters, word);
        HIP_TRY(hipGetLastError());
    }
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, word, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad != 0u) {
        err = tree_refusal("hdbscan select: not a condensed tree:", bad);
        return ERR_ARG;
    }

    uint32_t n_labels = 0;
    rc = select_clusters(t, ClusterKids{child_lo, child_hi, maxlam}, opt, s, &n_labels, stream, err);
    if (rc != OK) return rc;
    rc = copy_out({{a.out_selected, s.selected, clusters}, {a.out_labels, s.labels, n * 4}, {a.out_prob, s.prob, n * 4}, {a.out_score, s.score, n * 4},
                   {a.out_death, s.death, clusters * 8}},
                  host, stream, err);
    if (rc != OK) return rc;
    *a.out_n_labels = n_labels;
    return OK;
}

}  // namespace hnswgpu
