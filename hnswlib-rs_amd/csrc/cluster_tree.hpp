// cluster_tree.hpp -- what a condensed tree is on the device, once, for the three HDBSCAN units (condensed_tree.hip writes one,
// cluster_select.hip selects from one, cluster_predict.hip assigns new points to one): the constants, the lambda of a weight, the
// max of the lambda bits, the published f64 words of the climb, the GLOSH score, the membership probability, the label of a point,
// the checks that come before any traversal with their fault bits and refusal text, and the selection itself, whose kernels live in
// cluster_select.hip and are launched through the host functions declared at the end.  Private, like graph_internal.hpp.
//
// A tree of K clusters over n vertices: parent[0] is NONE and parent[c] < c, so every climb goes to a strictly smaller index and
// ends at cluster 0; birth[c] and point_w[v] are the stored bits of f32 weights; point_cluster[v] < K.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "hip_host.hpp"

namespace hnswgpu {

constexpr uint32_t NONE = 0xFFFFFFFFu, INF_BITS = 0x7F800000u;

// the bits of a call's check word: what a tree's checks (and, for a prediction, the rows' checks) can find
enum TreeFault : uint32_t { BAD_ROOT = 1u, BAD_PARENT = 2u, BAD_STABILITY = 4u, BAD_POINT = 8u, BAD_KIDS = 16u, BAD_COUNT = 32u, BAD_POS = 64u };

// the refusal of a check word that is not 0: the prefix, then a sentence per fault
inline std::string tree_refusal(const char* prefix, uint32_t bad) {
    std::string err = prefix;
    if (bad & BAD_ROOT) err += " cluster_parent[0] is not UINT32_MAX;";
    if (bad & BAD_PARENT) err += " a cluster_parent[c] is not below c;";
    if (bad & BAD_STABILITY) err += " a stability is NaN or negative;";
    if (bad & BAD_POINT) err += " a point_cluster[v] is not below K;";
    if (bad & BAD_KIDS) err += " a cluster other than 0 has one child, or more than two;";
    if (bad & BAD_COUNT) err += " a counts[q] is above knbn;";
    if (bad & BAD_POS) err += " a used nbr_pos is not below n;";
    err.pop_back();
    return err;
}

// nodes can pass 2^32 - 256: a thread's number is taken in 64 bits
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

// a per-cluster f64 kept as its bits (the max of the lambdas, a death): lambdas are >= 0, so the order of their f64 bits is their order
__device__ __forceinline__ double f64_of(unsigned long long bits) { return __longlong_as_double((long long)bits); }

// The words only rise during a kernel, so a value at or above mine, however old, says that mine cannot win: behind the load most
// threads skip the atomic.
__device__ __forceinline__ void raise_lambda(unsigned long long* maxlam, uint32_t c, double l) {
    const unsigned long long mine = (unsigned long long)__double_as_longlong(l);
    if (__hip_atomic_load(maxlam + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(maxlam + c, mine);
}

// what a climbing thread leaves for the one that arrives after it, and how that one reads it: agent-scope, never from a stale line
__device__ __forceinline__ void publish_f64(unsigned long long* s, uint32_t c, double v) {
    __hip_atomic_store(s + c, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double fetch_f64(unsigned long long* s, uint32_t c) {
    return f64_of(__hip_atomic_load(s + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// GLOSH: the outlier score of a point that left at lambda `lam` from a cluster whose subtree dies at `death`.  (The units are
// compiled with -ffp-contract=off: the subtraction and the division stay two operations.)
__device__ __forceinline__ float glosh_score(double lam, double death) {
    if (death == 0.0 || lam >= death) return 0.0f;
    if (death == __longlong_as_double(0x7FF0000000000000ll)) return 1.0f;
    const double gap = death - lam;
    return (float)(gap / death);
}

// the membership probability of a point of lambda `lam` in a cluster whose max of the lambdas is `top`
__device__ __forceinline__ float membership(double lam, double top) { return (top == 0.0 || lam >= top) ? 1.0f : (float)(lam / top); }

// Label and probability of a point of lambda `lam` whose selected ancestor-or-self is q (NONE, or anything not below K: none).
// single_root: the selection is {0}; then q does not count, and the point belongs to cluster 0 iff its lambda reaches the threshold:
// 1 / eps, or without an epsilon the max of cluster 0's lambdas.  label_of: the scan of the selected flags.
__device__ __forceinline__ void label_of_point(double lam, uint32_t q, bool single_root, float eps, uint32_t clusters, const uint32_t* __restrict__ label_of,
                                               const unsigned long long* __restrict__ maxlam, int32_t& label, float& prob) {
    if (single_root) {
        const double thr = eps > 0.0f ? 1.0 / (double)eps : f64_of(maxlam[0]);
        q = lam >= thr ? 0u : NONE;
    }
    if (q >= clusters) {
        label = -1;
        prob = 0.0f;
        return;
    }
    label = (int32_t)label_of[q];
    prob = membership(lam, f64_of(maxlam[q]));
}

// The checks BEFORE ANY TRAVERSAL, the part that every unit that is handed a tree shares.  A fault sets a bit of `word`; an index
// that passes is used at once, for the max of the lambda bits.
// Cluster c: parent[0] is NONE, parent[c] < c; the child raises its parent's lambda.  True iff c is a child whose parent passed.
__device__ __forceinline__ bool check_cluster(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ birth, uint32_t c, unsigned long long* maxlam,
                                              uint32_t* word) {
    const uint32_t p = parent[c];
    if (c == 0u) {
        if (p != NONE) atomicOr(word, (uint32_t)BAD_ROOT);
        return false;
    }
    if (p >= c) {
        atomicOr(word, (uint32_t)BAD_PARENT);
        return false;
    }
    raise_lambda(maxlam, p, lambda_of(birth[c]));
    return true;
}
// Vertex v: point_cluster[v] < K; the vertex raises its cluster's lambda.
__device__ __forceinline__ void check_vertex(const uint32_t* __restrict__ point_cluster, const uint32_t* __restrict__ point_w, uint64_t v, uint32_t clusters,
                                             unsigned long long* maxlam, uint32_t* word) {
    const uint32_t c = point_cluster[v];
    if (c >= clusters) {
        atomicOr(word, (uint32_t)BAD_POINT);
        return;
    }
    raise_lambda(maxlam, c, lambda_of(point_w[v]));
}

// ---- defined in cluster_select.hip, whose code object holds the kernels.  Every array is device memory, the device of the call
// is current, everything goes on `stream` and nobody waits unless it says so.

// Pointer doubling over the K >= 1 clusters of parent[], which has passed its checks, rounds counted on the host.  A state word is
// (jump << 32) | best: best is the HIGHEST (NEAREST: the lowest) flagged cluster among those from c up to, not including, jump;
// past cluster 0 jump is NONE.  At the end state_a -- the two buffers take turns -- holds for every c its highest (nearest)
// flagged ancestor-or-self, NONE where there is none.
template <typename Flag, bool NEAREST>
int flagged_ancestors(const uint32_t* parent, const Flag* flag, uint64_t clusters, uint64_t*& state_a, uint64_t*& state_b, hipStream_t stream,
                      std::string& err);
extern template int flagged_ancestors<uint32_t, false>(const uint32_t*, const uint32_t*, uint64_t, uint64_t*&, uint64_t*&, hipStream_t, std::string&);
extern template int flagged_ancestors<uint8_t, true>(const uint32_t*, const uint8_t*, uint64_t, uint64_t*&, uint64_t*&, hipStream_t, std::string&);

// The numbers of the labels from a doubling's answer: c is selected iff it is its own best.  selected (K bytes, may be nullptr)
// and selflag (K + 1 words) are written, and rocPRIM scans selflag into label_of (K + 1 words): label_of[K] is the number of
// selected clusters.  `temp` gets the scan's storage: it may go once the stream has been waited for.  K == 0: state is not read.
int number_selected(const uint64_t* state, uint64_t clusters, uint8_t* selected, uint32_t* selflag, uint32_t* label_of, DevMem& temp, hipStream_t stream,
                    std::string& err);

// the condensed tree that a selection reads
struct ClusterTree {
    const uint32_t* parent;
    const uint32_t* birth;
    const uint32_t* size;
    const double* stability;
    const uint32_t* point_cluster;
    const uint32_t* point_w;
    uint32_t n, clusters;
};
// what its checks (cluster_select.hip) or its maker (condensed_tree.hip) gathered per cluster: the least and the greatest child of
// every cluster other than 0 that has children (child_hi: 0 for a leaf), the max of the lambda bits of every cluster
struct ClusterKids {
    const uint32_t* child_lo;
    const uint32_t* child_hi;
    const unsigned long long* maxlam;
};
struct SelectOptions {
    uint32_t method, allow_single;
    float eps;
    uint64_t max_size;  // 0: no limit
};
// A selection's scratch, named into the caller's layout: zeroed() among the arrays that the caller clears to 0 before the
// selection, rest() anywhere.  end_a and end_b are there under an epsilon, score when it is wanted.  After select_clusters state_a
// holds the doubling's last answer.
struct SelectScratch {
    uint32_t *arrive, *wins, *fflag, *selflag, *label_of;
    unsigned long long *s_of, *death;
    uint64_t *state_a, *state_b, *end_a = nullptr, *end_b = nullptr;
    uint8_t* selected;
    int32_t* labels;
    float *prob, *score = nullptr;

    void zeroed(ScratchLayout& lay, uint64_t clusters) { lay.arrays(clusters, arrive, wins, fflag); }
    void rest(ScratchLayout& lay, uint64_t n, uint64_t clusters, const SelectOptions& o, bool want_score) {
        lay.arrays(clusters, s_of, death, state_a, state_b);
        if (o.eps > 0.0f) lay.arrays(clusters, end_a, end_b);
        lay.arrays(clusters + 1, selflag, label_of);
        lay.array(selected, clusters);
        lay.arrays(n, labels, prob);
        if (want_score) lay.array(score, n);
    }
};
// The selection: the climb (excess of mass, or the leaves), cluster 0, the doubling that gives E, under an epsilon the climb to F
// and the doubling that gives E', the labels' numbers, and per vertex label, probability and -- with s.score -- GLOSH score, all
// into `s`; death[] holds every cluster's death lambda.  n, K >= 1.  Waits for the stream; *n_labels is written at the end.
int select_clusters(const ClusterTree& t, const ClusterKids& k, const SelectOptions& o, SelectScratch& s, uint32_t* n_labels, hipStream_t stream,
                    std::string& err);

}  // namespace hnswgpu
