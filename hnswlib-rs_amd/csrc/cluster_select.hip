// cluster_select.hip -- HDBSCAN's second stage on the device (gfx950 only): from a condensed tree that condensed_tree.hip wrote, the
// selection under allow_single_cluster, cluster_selection_epsilon and max_cluster_size, the flat labels and probabilities and the
// GLOSH outlier scores: the device side of hnswhds_select(_device) of include/hnsw_mi355x_hdbscan_select.h, which holds the contract
// word for word (the entries and the host form's checks are in capi.cpp).  DESIGN.md "HDBSCAN: selection options and GLOSH".
//
//   cs_check_kernel      one thread per cluster and per vertex, BEFORE ANY TRAVERSAL: parent[0] is NONE, parent[c] < c, a stability
//                        is neither NaN nor negative, point_cluster[v] < K -- a fault sets a bit of one word.  An index that passes
//                        is used at once: a child counts into its parent (count, min and max of the child indices) and raises the
//                        parent's max of the lambda bits, a vertex raises its cluster's -- integer atomics.
//   cs_kids_kernel       one thread per cluster: a cluster other than 0 has no child or two, else a bit of the word.  The word is
//                        read back: with a bit set the call ends here, ERR_ARG.  From here on parent[] is a tree under cluster 0.
//   cs_climb_kernel      one thread per leaf cluster, ONE launch, hd_eom_kernel's protocol: it stores its S and its death, fences
//                        and adds 1 to its parent's arrival counter.  The first arriver leaves; the second fences, loads both
//                        children's S and death (agent-scope loads), decides the parent -- stability >= S + S and the size test --
//                        and goes on upwards.  Nobody waits.  Children of cluster 0 go no further.
//   cs_root_kernel       ONE block: thread t adds S of the children of 0 whose index is t modulo 256 in ascending index, then a
//                        tree over the 256 sums in LDS (the shape of hd_stability_kernel): sub(0), a function of the input alone.
//                        death(0) is a max over the same children.  Cluster 0 wins or not.
//   cs_jump_*_kernel     pointer doubling over the K clusters, rounds counted on the host: (jump, best) with best the highest
//                        flagged cluster among those from c up to, not including, jump; past cluster 0 jump is NONE.  At the end
//                        best[c] is the highest flagged ancestor-or-self of c.  Run on the winners it gives E (best[c] == c).
//   cs_end_*_kernel      the epsilon climb as pointer doubling: a cluster whose climb ends in one step holds its end, every other
//                        one its parent; a round replaces "go on from p" by what p holds.
//   cs_f_kernel          one thread per cluster: a member of E marks its end (or itself): F.  The doubling once more on F gives
//                        E' (best[c] == c) and for every cluster its member of E', which is unique: E' is an antichain.
//   cs_flag_kernel       selected, and the flags that rocPRIM scans into the labels' numbers.  L is read back at the end.
//   cs_vertex_kernel     one thread per vertex: label, probability -- with the single-root threshold branch -- and GLOSH score
// Every loop ends: the climb goes to a strictly smaller index each step, checked in the loop; the doubling rounds are counted.  No
// wavefront waits on another; no floating-point atomic; everything is a function of the input.  Everything is computed into scratch,
// and the out arrays are written at the very end: a refusal touches none of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"

namespace hnswgpu {
namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu, INF_BITS = 0x7F800000u;
// the bits of a call's check word
constexpr uint32_t BAD_ROOT = 1u, BAD_PARENT = 2u, BAD_STABILITY = 4u, BAD_POINT = 8u, BAD_KIDS = 16u;

__device__ __forceinline__ uint64_t thread_number() { return (uint64_t)blockIdx.x * 256u + threadIdx.x; }

// lambda of a weight's stored bits: 1 / w in f64; +0 for +inf and NaN; +inf for w <= 0, -0 included
__device__ __forceinline__ double lambda_of(uint32_t bits) {
    const float w = __uint_as_float(bits);
    if (w != w || bits == INF_BITS) return 0.0;
    if (w <= 0.0f) return __longlong_as_double(0x7FF0000000000000ll);
    return 1.0 / (double)w;
}

// a weight by value: a NaN counts as +inf (-0 equals +0 under the comparisons as it is)
__device__ __forceinline__ float weight_value(uint32_t bits) {
    const float w = __uint_as_float(bits);
    return w != w ? __uint_as_float(INF_BITS) : w;
}

// lambdas are >= 0: the order of their f64 bits is their order (condensed_tree.hip: raise_lambda)
__device__ __forceinline__ void raise_lambda(unsigned long long* maxlam, uint32_t c, double l) {
    const unsigned long long mine = (unsigned long long)__double_as_longlong(l);
    if (__hip_atomic_load(maxlam + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(maxlam + c, mine);
}

// the condensed tree as the caller gave it
struct Tree {
    const uint32_t* parent;
    const uint32_t* birth;
    const uint32_t* size;
    const double* stability;
    const uint32_t* point_cluster;
    const uint32_t* point_w;
    uint32_t n, clusters;
};

// what the checks gather per cluster, `clusters` of each: all 0 before, child_lo 0xFF..
struct Kids {
    uint32_t* count;
    uint32_t* child_lo;
    uint32_t* child_hi;
    unsigned long long* maxlam;
};

// clusters + n threads: the clusters first
__global__ __launch_bounds__(256) void cs_check_kernel(Tree t, Kids k, uint32_t* __restrict__ word) {
    const uint64_t i = thread_number();
    if (i >= (uint64_t)t.clusters + t.n) return;
    if (i < t.clusters) {
        const uint32_t c = (uint32_t)i, p = t.parent[c];
        const double s = t.stability[c];
        if (!(s >= 0.0)) atomicOr(word, BAD_STABILITY);  // a NaN too
        if (c == 0u) {
            if (p != NONE) atomicOr(word, BAD_ROOT);
            return;
        }
        if (p >= c) {
            atomicOr(word, BAD_PARENT);
            return;
        }
        if (p != 0u) {  // (cluster 0 may have any number of children, and nobody asks for their ends)
            atomicAdd(k.count + p, 1u);
            atomicMin(k.child_lo + p, c);
            atomicMax(k.child_hi + p, c);
        }
        raise_lambda(k.maxlam, p, lambda_of(t.birth[c]));
        return;
    }
    const uint64_t v = i - t.clusters;
    const uint32_t c = t.point_cluster[v];
    if (c >= t.clusters) {
        atomicOr(word, BAD_POINT);
        return;
    }
    raise_lambda(k.maxlam, c, lambda_of(t.point_w[v]));
}

// one thread per cluster from 1 on
__global__ __launch_bounds__(256) void cs_kids_kernel(const uint32_t* __restrict__ count, uint32_t clusters, uint32_t* __restrict__ word) {
    const uint64_t c = thread_number() + 1u;
    if (c >= clusters) return;
    if (count[c] != 0u && count[c] != 2u) atomicOr(word, BAD_KIDS);
}

__device__ __forceinline__ void publish_f64(unsigned long long* s, uint32_t c, double v) {
    __hip_atomic_store(s + c, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double fetch_f64(unsigned long long* s, uint32_t c) {
    return __longlong_as_double((long long)__hip_atomic_load(s + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// the options of a call
struct Options {
    uint32_t method, allow_single;
    float eps;
    uint64_t max_size;  // 0: no limit
};

__device__ __forceinline__ bool size_fits(const Options& o, uint32_t size) { return o.max_size == 0u || (uint64_t)size <= o.max_size; }

// one thread per cluster; arrive, wins: 0 before.  The climb goes to a smaller index each step and leaves at a child of cluster 0.
__global__ __launch_bounds__(256) void cs_climb_kernel(Tree t, Kids k, Options o, uint32_t* arrive, unsigned long long* s_of, unsigned long long* death,
                                                      uint32_t* __restrict__ wins) {
    const uint64_t i = thread_number();
    if (i == 0u || i >= t.clusters) return;
    uint32_t cur = (uint32_t)i;
    if (k.child_hi[cur] != 0u) return;  // not a leaf
    {
        const double own = t.stability[cur];
        const bool win = o.method == HNSWGPU_SELECT_LEAF || size_fits(o, t.size[cur]);  // (own >= 0, the empty sum)
        wins[cur] = win ? 1u : 0u;
        publish_f64(s_of, cur, win ? own : 0.0);
        publish_f64(death, cur, __longlong_as_double((long long)k.maxlam[cur]));
    }
    for (;;) {
        const uint32_t p = t.parent[cur];
        if (p == 0u || p >= cur) return;  // (p >= cur: never, the checks have passed)
        __threadfence();  // my S and death before my arrival
        if (__hip_atomic_fetch_add(arrive + p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;  // the sibling's subtree is still to come
        __threadfence();  // the sibling's arrival before its S and death
        const uint32_t lo = k.child_lo[p], hi = k.child_hi[p];
        if (lo >= t.clusters || hi >= t.clusters) return;  // (never)
        const double sum = fetch_f64(s_of, lo) + fetch_f64(s_of, hi), own = t.stability[p];
        const bool win = o.method == HNSWGPU_SELECT_EOM && own >= sum && size_fits(o, t.size[p]);  // a tie goes to the parent
        wins[p] = win ? 1u : 0u;
        publish_f64(s_of, p, win ? own : sum);
        const double d = fmax(__longlong_as_double((long long)k.maxlam[p]), fmax(fetch_f64(death, lo), fetch_f64(death, hi)));
        publish_f64(death, p, d);
        cur = p;
    }
}

// ONE block.  The children of 0 hold their S and death (a kernel before this one wrote them).
__global__ __launch_bounds__(256) void cs_root_kernel(Tree t, Kids k, Options o, const unsigned long long* __restrict__ s_of, unsigned long long* death,
                                                     uint32_t* __restrict__ wins) {
    __shared__ double part[256];
    __shared__ double high[256];
    double s = 0.0, d = 0.0;
    for (uint64_t c = threadIdx.x; c < t.clusters; c += 256u) {
        if (t.parent[c] != 0u) continue;  // (parent[0] is NONE)
        s += __longlong_as_double((long long)s_of[c]);
        d = fmax(d, __longlong_as_double((long long)death[c]));
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
    death[0] = (unsigned long long)__double_as_longlong(fmax(__longlong_as_double((long long)k.maxlam[0]), high[0]));
}

// (jump << 32) | best: jump is the parent, NONE above cluster 0 (parent[0] is NONE); best is c itself where its flag is set
__global__ __launch_bounds__(256) void cs_jump_init_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ flag, uint32_t clusters,
                                                          uint64_t* __restrict__ state) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    state[c] = ((uint64_t)(c == 0u ? NONE : parent[c]) << 32) | (flag[c] != 0u ? (uint32_t)c : NONE);
}

__global__ __launch_bounds__(256) void cs_jump_round_kernel(const uint64_t* __restrict__ from, uint32_t clusters, uint64_t* __restrict__ to) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    uint64_t mine = from[c];
    const uint32_t j = (uint32_t)(mine >> 32);
    if (j < clusters) {  // (NONE is not)
        const uint64_t above = from[j];
        const uint32_t best = (uint32_t)above != NONE ? (uint32_t)above : (uint32_t)mine;  // the higher stretch goes first
        mine = (above & 0xFFFFFFFF00000000ull) | best;
    }
    to[c] = mine;
}

// The epsilon climb from c != 0, one step: with p = parent(c), p == 0 ends it at 0 (allow_single_cluster) or at c; birth_w(p) > eps
// ends it at p; otherwise it goes on from p.  (jump << 32) | end: jump NONE where the end is known, else end NONE.
__global__ __launch_bounds__(256) void cs_end_init_kernel(Tree t, Options o, uint64_t* __restrict__ state) {
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

__global__ __launch_bounds__(256) void cs_end_round_kernel(const uint64_t* __restrict__ from, uint32_t clusters, uint64_t* __restrict__ to) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    const uint64_t mine = from[c];
    const uint32_t j = (uint32_t)(mine >> 32);
    to[c] = j < clusters ? from[j] : mine;
}

// one thread per cluster; fflag: 0 before.  top: the doubling's state over the winners; ends: over the epsilon climb.
__global__ __launch_bounds__(256) void cs_f_kernel(Tree t, Options o, const uint64_t* __restrict__ top, const uint64_t* __restrict__ ends,
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

// clusters + 1 threads: one per cluster, and one for the flag behind the last, which the scan reads
__global__ __launch_bounds__(256) void cs_flag_kernel(const uint64_t* __restrict__ state, uint32_t clusters, uint8_t* __restrict__ selected,
                                                     uint32_t* __restrict__ selflag) {
    const uint64_t c = thread_number();
    if (c > clusters) return;
    const bool sel = c < clusters && (uint32_t)state[c] == (uint32_t)c;
    selflag[c] = sel ? 1u : 0u;
    if (c < clusters) selected[c] = sel ? 1u : 0u;
}

// one thread per vertex.  (-ffp-contract=off: the score's subtraction and division stay two operations.)
__global__ __launch_bounds__(256) void cs_vertex_kernel(Tree t, Options o, const uint64_t* __restrict__ state, const uint32_t* __restrict__ label_of,
                                                       const unsigned long long* __restrict__ maxlam, const unsigned long long* __restrict__ death,
                                                       int32_t* __restrict__ labels, float* __restrict__ prob, float* __restrict__ score) {
    const uint64_t v = thread_number();
    if (v >= t.n) return;
    const uint32_t c = t.point_cluster[v];  // below K: checked
    const double lam = lambda_of(t.point_w[v]);
    {
        const double d = __longlong_as_double((long long)death[c]);
        float sc;
        if (d == 0.0 || lam >= d) sc = 0.0f;
        else if (d == __longlong_as_double(0x7FF0000000000000ll)) sc = 1.0f;
        else {
            const double gap = d - lam;
            sc = (float)(gap / d);
        }
        score[v] = sc;
    }
    uint32_t q = (uint32_t)state[c];
    if ((uint32_t)state[0] == 0u) {  // E' is {0}: the threshold, for every vertex
        const double thr = o.eps > 0.0f ? 1.0 / (double)o.eps : __longlong_as_double((long long)maxlam[0]);
        q = lam >= thr ? 0u : NONE;
    }
    if (q >= t.clusters) {
        labels[v] = -1;
        prob[v] = 0.0f;
        return;
    }
    labels[v] = (int32_t)label_of[q];
    const double top = __longlong_as_double((long long)maxlam[q]);
    prob[v] = (top == 0.0 || lam >= top) ? 1.0f : (float)(lam / top);
}

// the doubling over `flag` from state_a, which holds the answer at the end (the two buffers take turns)
int highest_flagged(const uint32_t* parent, const uint32_t* flag, uint64_t clusters, uint64_t*& state_a, uint64_t*& state_b, hipStream_t stream,
                    std::string& err) {
    hipLaunchKernelGGL(cs_jump_init_kernel, grid_of(clusters), dim3(256), 0, stream, parent, flag, (uint32_t)clusters, state_a);
    HIP_TRY(hipGetLastError());
    for (uint64_t reach = 1; reach <= clusters; reach *= 2) {  // a cluster's depth is below K, and one jump leads past cluster 0
        hipLaunchKernelGGL(cs_jump_round_kernel, grid_of(clusters), dim3(256), 0, stream, state_a, (uint32_t)clusters, state_b);
        HIP_TRY(hipGetLastError());
        std::swap(state_a, state_b);
    }
    return OK;
}

}  // namespace

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
    DevMem mem;
    Drain drain{stream};
    uint32_t *word, *count, *child_lo, *child_hi, *arrive, *wins, *fflag, *selflag, *label_of;
    unsigned long long *maxlam, *s_of, *death;
    uint64_t *state_a, *state_b, *end_a, *end_b;
    uint8_t* selected;
    int32_t* labels;
    float *prob, *score;
    uint32_t *up_parent = nullptr, *up_birth = nullptr, *up_size = nullptr, *up_pc = nullptr, *up_pw = nullptr;
    double* up_stability = nullptr;
    ScratchLayout lay;
    lay.array(word, 64);
    lay.array(child_lo, clusters);
    // those that are 0 before their kernels stand together, from count on
    const uint64_t zeroed_from = lay.size();
    lay.arrays(clusters, count, child_hi, arrive, wins, fflag, maxlam);
    const uint64_t zeroed_bytes = lay.size() - zeroed_from;
    lay.arrays(clusters, s_of, death, state_a, state_b, end_a, end_b);
    lay.arrays(clusters + 1, selflag, label_of);
    lay.array(selected, clusters);
    lay.arrays(n, labels, prob, score);
    if (host) {
        lay.arrays(clusters, up_parent, up_birth, up_size, up_stability);
        lay.arrays(n, up_pc, up_pw);
    }
    rc = alloc_layout("hdbscan select", mem, lay, err);  // (before anything is written)
    if (rc != OK) return rc;
    Tree t{a.cluster_parent, reinterpret_cast<const uint32_t*>(a.cluster_birth_w), a.cluster_size, a.stability, a.point_cluster,
           reinterpret_cast<const uint32_t*>(a.point_w), (uint32_t)n, (uint32_t)clusters};
    if (host) {
        const struct { void* to; const void* from; uint64_t bytes; } ups[] = {
            {up_parent, a.cluster_parent, clusters * 4}, {up_birth, a.cluster_birth_w, clusters * 4}, {up_size, a.cluster_size, clusters * 4},
            {up_stability, a.stability, clusters * 8},   {up_pc, a.point_cluster, n * 4},              {up_pw, a.point_w, n * 4},
        };
        for (const auto& u : ups) HIP_TRY(hipMemcpyAsync(u.to, u.from, u.bytes, hipMemcpyHostToDevice, stream));
        t = Tree{up_parent, up_birth, up_size, up_stability, up_pc, up_pw, (uint32_t)n, (uint32_t)clusters};
    }
    const Kids kids{count, child_lo, child_hi, maxlam};
    const Options opt{a.method, a.allow_single_cluster, a.eps, a.max_cluster_size};
    const uint32_t k32 = (uint32_t)clusters;

    HIP_TRY(hipMemsetAsync(word, 0, 256, stream));
    HIP_TRY(hipMemsetAsync(child_lo, 0xFF, clusters * 4, stream));
    HIP_TRY(hipMemsetAsync(count, 0, zeroed_bytes, stream));
    hipLaunchKernelGGL(cs_check_kernel, grid_of(clusters + n), dim3(256), 0, stream, t, kids, word);
    HIP_TRY(hipGetLastError());
    if (clusters > 1) {
        hipLaunchKernelGGL(cs_kids_kernel, grid_of(clusters - 1), dim3(256), 0, stream, count, k32, word);
        HIP_TRY(hipGetLastError());
    }
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, word, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad != 0u) {
        err = "hdbscan select: not a condensed tree:";
        if (bad & BAD_ROOT) err += " cluster_parent[0] is not UINT32_MAX;";
        if (bad & BAD_PARENT) err += " a cluster_parent[c] is not below c;";
        if (bad & BAD_STABILITY) err += " a stability is NaN or negative;";
        if (bad & BAD_POINT) err += " a point_cluster[v] is not below K;";
        if (bad & BAD_KIDS) err += " a cluster other than 0 has one child, or more than two;";
        err.pop_back();
        return ERR_ARG;
    }

    if (clusters > 1) {
        hipLaunchKernelGGL(cs_climb_kernel, grid_of(clusters), dim3(256), 0, stream, t, kids, opt, arrive, s_of, death, wins);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cs_root_kernel, dim3(1), dim3(256), 0, stream, t, kids, opt, s_of, death, wins);
    HIP_TRY(hipGetLastError());
    rc = highest_flagged(t.parent, wins, clusters, state_a, state_b, stream, err);  // E
    if (rc != OK) return rc;
    if (a.eps > 0.0f) {  // F, then E'
        hipLaunchKernelGGL(cs_end_init_kernel, grid_of(clusters), dim3(256), 0, stream, t, opt, end_a);
        HIP_TRY(hipGetLastError());
        for (uint64_t reach = 1; reach < clusters; reach *= 2) {  // a climb has fewer than K steps
            hipLaunchKernelGGL(cs_end_round_kernel, grid_of(clusters), dim3(256), 0, stream, end_a, k32, end_b);
            HIP_TRY(hipGetLastError());
            std::swap(end_a, end_b);
        }
        hipLaunchKernelGGL(cs_f_kernel, grid_of(clusters), dim3(256), 0, stream, t, opt, state_a, end_a, fflag);
        HIP_TRY(hipGetLastError());
        rc = highest_flagged(t.parent, fflag, clusters, state_a, state_b, stream, err);
        if (rc != OK) return rc;
    }
    hipLaunchKernelGGL(cs_flag_kernel, grid_of(clusters + 1), dim3(256), 0, stream, state_a, k32, selected, selflag);
    HIP_TRY(hipGetLastError());
    {
        DevMem temp;
        rc = exclusive_scan_u32(temp, selflag, label_of, clusters + 1, stream, err);
        if (rc != OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
    }
    hipLaunchKernelGGL(cs_vertex_kernel, grid_of(n), dim3(256), 0, stream, t, opt, state_a, label_of, maxlam, death, labels, prob, score);
    HIP_TRY(hipGetLastError());
    uint32_t n_labels = 0;
    HIP_TRY(hipMemcpyAsync(&n_labels, label_of + clusters, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));

    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const struct { void* to; const void* from; uint64_t bytes; } copies[] = {
        {a.out_selected, selected, clusters}, {a.out_labels, labels, n * 4},     {a.out_prob, prob, n * 4},
        {a.out_score, score, n * 4},          {a.out_death, death, clusters * 8},
    };
    for (const auto& c : copies)
        if (c.to) HIP_TRY(hipMemcpyAsync(c.to, c.from, c.bytes, kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *a.out_n_labels = n_labels;
    return OK;
}

}  // namespace hnswgpu
