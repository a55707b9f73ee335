// cluster_predict.hip -- HDBSCAN's third stage on the device (gfx950 only): new points are assigned to the clusters of a condensed
// tree -- approximate_predict --: the device side of hnswhdp_core_distances(_device), hnswhdp_assign(_device) and
// hnswhdp_predict(_device) of include/hnsw_mi355x_hdbscan_predict.h, which holds the contract word for word (the entries and the host
// forms' checks are in capi.cpp).  DESIGN.md "HDBSCAN: predict".
//
//   cp_core_kernel       one thread per vertex: the stored distance of slot min(core_k, counts[v]) - 1 of row v of D (msf_core_kernel of
//                        spanning_forest.hip, which keeps its own)
//   cp_check_kernel      K + n + nq k threads, BEFORE ANY TRAVERSAL OR GATHER: parent[0] is NONE, parent[c] < c, point_cluster[v] < K,
//                        counts[q] <= k, a used nbr_pos < n -- a fault sets a bit of one word, which is read back.  An index that
//                        passes is used at once: a child raises its parent's max of the lambda bits, a vertex its cluster's (integer
//                        atomic max).
//   cp_jump_*_kernel     ONCE PER CALL, pointer doubling over the K clusters, rounds counted on the host: (jump, best) with best the
//                        lowest selected cluster among those from c up to, not including, jump; past cluster 0 jump is NONE.  At the
//                        end best[c] is the nearest selected ancestor-or-self of c.
//   cp_flag_kernel       the flags that rocPRIM scans into the labels' numbers; the scan's last word is the number of selected clusters
//   cp_position_kernel   (index form) one thread per slot of the staged answers: p_id -> flat id -> position (sym_expand_kernel's rule)
//   cp_assign_kernel     GROUP lanes per query (16: four queries per wavefront), so that a row's nbr_pos / nbr_dist loads are
//                        contiguous across the lanes: a lane strides over the slots, gathers core[pos] and keeps the smallest key
//                        (order bits of mr) << 32 | slot; the group folds the key with __shfl_xor -- no LDS, no atomic --; the key
//                        holds the slot, so the answer does not depend on GROUP.  The group's first lane then climbs: every step goes
//                        to a strictly smaller cluster index, checked in the loop, so a walk has at most depth(cluster tree) steps.
// No floating-point atomic, no grid-wide sync, no wavefront waits on another; everything is a function of the input.  Everything is
// computed into scratch, and the out arrays are written at the very end: a refusal touches none of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "graph_internal.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"
#include "rocprim_host.hpp"

namespace hnswgpu {
namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu, INF_BITS = 0x7F800000u;
// the bits of a call's check word
constexpr uint32_t BAD_ROOT = 1u, BAD_PARENT = 2u, BAD_POINT = 4u, BAD_COUNT = 8u, BAD_POS = 16u;
// lanes per query of cp_assign_kernel: a power of two, at most 64
constexpr uint32_t GROUP = 16u;

__device__ __forceinline__ uint64_t thread_number() { return (uint64_t)blockIdx.x * 256u + threadIdx.x; }

// lambda of a weight's stored bits: 1 / w in f64; +0 for +inf and NaN; +inf for w <= 0, -0 included (condensed_tree.hip)
__device__ __forceinline__ double lambda_of(uint32_t bits) {
    const float w = __uint_as_float(bits);
    if (w != w || bits == INF_BITS) return 0.0;
    if (w <= 0.0f) return __longlong_as_double(0x7FF0000000000000ll);
    return 1.0 / (double)w;
}

// lambdas are >= 0: the order of their f64 bits is their order (condensed_tree.hip: raise_lambda)
__device__ __forceinline__ void raise_lambda(unsigned long long* maxlam, uint32_t c, double l) {
    const unsigned long long mine = (unsigned long long)__double_as_longlong(l);
    if (__hip_atomic_load(maxlam + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(maxlam + c, mine);
}

// the later of two weights' bits under dist_order_bits; a tie keeps the earlier argument
__device__ __forceinline__ uint32_t later_bits(uint32_t w, uint32_t other) {
    return dist_order_bits(__uint_as_float(other)) > dist_order_bits(__uint_as_float(w)) ? other : w;
}

// one thread per vertex: core[v] = the bits of slot min(core_k, counts[v]) - 1 of row v, +0 for an empty row
__global__ __launch_bounds__(256) void cp_core_kernel(const float* __restrict__ dists, const uint32_t* __restrict__ counts, uint32_t k, uint32_t core_k,
                                                     uint32_t n, uint32_t* __restrict__ core) {
    const uint64_t v = thread_number();
    if (v >= n) return;
    uint32_t c = counts[v];
    if (c > k) c = k;  // (a slot of the row, whatever the count holds)
    if (c > core_k) c = core_k;
    core[v] = c == 0u ? 0u : __float_as_uint(dists[v * k + (c - 1u)]);
}

// the tree and the stored points' core distances, in device memory
struct Tree {
    const uint32_t* core;
    const uint32_t* parent;
    const uint32_t* birth;
    const uint32_t* point_cluster;
    const uint32_t* point_w;
    const uint8_t* selected;
    const double* death;  // may be nullptr
    uint32_t n, clusters;
    float eps;
};
// the queries' neighbour rows, in device memory
struct Rows {
    const uint32_t* pos;
    const uint32_t* dist;
    const uint32_t* counts;  // nullptr: every row is empty
    uint32_t nq, k, core_k;
};

// clusters + n + nq k threads: the clusters first, then the vertices, then the slots
__global__ __launch_bounds__(256) void cp_check_kernel(Tree t, Rows r, unsigned long long* maxlam, uint32_t* __restrict__ word) {
    uint64_t i = thread_number();
    if (i < t.clusters) {
        const uint32_t c = (uint32_t)i, p = t.parent[c];
        if (c == 0u) {
            if (p != NONE) atomicOr(word, BAD_ROOT);
            return;
        }
        if (p >= c) {
            atomicOr(word, BAD_PARENT);
            return;
        }
        raise_lambda(maxlam, p, lambda_of(t.birth[c]));
        return;
    }
    i -= t.clusters;
    if (i < t.n) {
        const uint32_t c = t.point_cluster[i];
        if (c >= t.clusters) {
            atomicOr(word, BAD_POINT);
            return;
        }
        raise_lambda(maxlam, c, lambda_of(t.point_w[i]));
        return;
    }
    i -= t.n;
    if (r.counts == nullptr || i >= (uint64_t)r.nq * r.k) return;
    const uint32_t q = (uint32_t)(i / r.k), s = (uint32_t)(i - (uint64_t)q * r.k), cnt = r.counts[q];
    if (cnt > r.k) {
        if (s == 0u) atomicOr(word, BAD_COUNT);
        return;
    }
    if (s < cnt && r.pos[i] >= t.n) atomicOr(word, BAD_POS);
}

// (jump << 32) | best: jump is the parent, NONE above cluster 0 (parent[0] is NONE); best is c itself where it is selected
__global__ __launch_bounds__(256) void cp_jump_init_kernel(const uint32_t* __restrict__ parent, const uint8_t* __restrict__ selected, uint32_t clusters,
                                                          uint64_t* __restrict__ state) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    state[c] = ((uint64_t)(c == 0u ? NONE : parent[c]) << 32) | (selected[c] != 0u ? (uint32_t)c : NONE);
}

__global__ __launch_bounds__(256) void cp_jump_round_kernel(const uint64_t* __restrict__ from, uint32_t clusters, uint64_t* __restrict__ to) {
    const uint64_t c = thread_number();
    if (c >= clusters) return;
    uint64_t mine = from[c];
    const uint32_t j = (uint32_t)(mine >> 32);
    if (j < clusters) {  // (NONE is not)
        const uint64_t above = from[j];
        const uint32_t best = (uint32_t)mine != NONE ? (uint32_t)mine : (uint32_t)above;  // the nearer stretch goes first
        mine = (above & 0xFFFFFFFF00000000ull) | best;
    }
    to[c] = mine;
}

// clusters + 1 threads: one per cluster, and one for the flag behind the last, which the scan reads
__global__ __launch_bounds__(256) void cp_flag_kernel(const uint8_t* __restrict__ selected, uint32_t clusters, uint32_t* __restrict__ selflag) {
    const uint64_t c = thread_number();
    if (c > clusters) return;
    selflag[c] = c < clusters && selected[c] != 0u ? 1u : 0u;
}

// one thread per slot t = q k + s of the staged answers: the position of the slot's p_id (layer, rank); a slot behind counts[q] gets
// 0 and is never read, a p_id that is none of the index gets NONE, which the check refuses
__global__ __launch_bounds__(256) void cp_position_kernel(DeviceIndexView ix, const uint32_t* __restrict__ rank_of, const uint8_t* __restrict__ layer,
                                                         const int32_t* __restrict__ rank, const uint32_t* __restrict__ counts, uint32_t k, uint32_t slots,
                                                         uint32_t* __restrict__ pos) {
    const uint64_t t = thread_number();
    if (t >= slots) return;
    const uint32_t q = (uint32_t)(t / k), s = (uint32_t)(t - (uint64_t)q * k);
    uint32_t p = 0u;
    if (s < counts[q]) {
        const uint32_t l = layer[t] < NB_LAYER_MAX ? layer[t] : NB_LAYER_MAX;
        const uint32_t flat = ix.layer_offset[l] + (uint32_t)rank[t];
        p = flat < ix.n ? rank_of[flat] : NONE;
    }
    pos[t] = p;
}

// a call's answers, nq of each, in scratch
struct Answers {
    int32_t* labels;
    float* prob;
    float* score;
    uint32_t* nearest;
    uint32_t* w;
    uint32_t* cluster;
};

// GROUP lanes per query, 256 / GROUP queries per block.  state: the doubling's answer; label_of: the scan, label_of[clusters] the
// number of selected clusters.  (-ffp-contract=off: the score's subtraction and division stay two operations.)
__global__ __launch_bounds__(256) void cp_assign_kernel(Tree t, Rows r, const uint64_t* __restrict__ state, const uint32_t* __restrict__ label_of,
                                                       const unsigned long long* __restrict__ maxlam, Answers out) {
    const uint64_t q = thread_number() / GROUP;
    if (q >= r.nq) return;  // (the whole group)
    const uint32_t lane = threadIdx.x & (GROUP - 1u);
    uint32_t cnt = r.counts == nullptr ? 0u : r.counts[q];
    if (cnt > r.k) cnt = r.k;  // (never: checked)
    const uint64_t row = q * r.k;
    const uint32_t core_slot = cnt < r.core_k ? cnt : r.core_k;
    const uint32_t core_q = core_slot == 0u ? 0u : r.dist[row + (core_slot - 1u)];
    uint64_t key = ~0ull;  // (above every slot's key: a slot is below 2^32 - 1)
    for (uint32_t s = lane; s < cnt; s += GROUP) {
        const uint32_t j = r.pos[row + s];
        uint32_t w = later_bits(r.dist[row + s], core_q);
        w = later_bits(w, t.core[j < t.n ? j : 0u]);  // (j < n: checked)
        const uint64_t mine = ((uint64_t)dist_order_bits(__uint_as_float(w)) << 32) | s;
        if (mine < key) key = mine;
    }
    for (uint32_t m = GROUP / 2u; m >= 1u; m >>= 1) {  // (the partners are lanes of this group: all of them are here)
        const uint64_t other = __shfl_xor((unsigned long long)key, (int)m);
        if (other < key) key = other;
    }
    if (lane != 0u) return;

    uint32_t nearest = NONE, w = INF_BITS, c = 0u;
    double lam = 0.0;
    if (cnt != 0u) {
        const uint32_t s = (uint32_t)key;  // below cnt
        nearest = r.pos[row + s];
        if (nearest >= t.n) nearest = 0u;  // (never: checked)
        w = later_bits(later_bits(r.dist[row + s], core_q), t.core[nearest]);
        lam = lambda_of(w);
        c = t.point_cluster[nearest];  // below K: checked
        if (!(lambda_of(t.point_w[nearest]) <= lam)) {
            while (c != 0u && lambda_of(t.birth[c]) >= lam) {
                const uint32_t p = t.parent[c];
                if (p >= c) break;  // (never: checked)
                c = p;
            }
        }
    }
    out.nearest[q] = nearest;
    out.w[q] = w;
    out.cluster[q] = c;
    float sc = 0.0f;
    if (t.death != nullptr && t.clusters != 0u) {
        const double d = t.death[c];
        if (d == 0.0 || lam >= d) sc = 0.0f;
        else if (d == __longlong_as_double(0x7FF0000000000000ll)) sc = 1.0f;
        else {
            const double gap = d - lam;
            sc = (float)(gap / d);
        }
    }
    out.score[q] = sc;
    uint32_t L = NONE;
    if (cnt != 0u) {  // (then there is a cluster: K >= 1)
        if (label_of[t.clusters] == 1u && t.selected[0] != 0u) {  // selected is {0}: the threshold
            const double thr = t.eps > 0.0f ? 1.0 / (double)t.eps : __longlong_as_double((long long)maxlam[0]);
            L = lam >= thr ? 0u : NONE;
        } else {
            L = (uint32_t)state[c];
        }
    }
    if (L >= t.clusters) {
        out.labels[q] = -1;
        out.prob[q] = 0.0f;
        return;
    }
    out.labels[q] = (int32_t)label_of[L];
    const double top = __longlong_as_double((long long)maxlam[L]);
    out.prob[q] = (top == 0.0 || lam >= top) ? 1.0f : (float)(lam / top);
}

// The assignment itself, for both forms: `t` and `r` are device memory, `out` is the caller's (host memory for `host`); the device is
// current.  Waits for `stream`.
int assign_rows(const Tree& t, const Rows& r, const PredictOut& out, bool host, hipStream_t stream, std::string& err) {
    const uint64_t clusters = t.clusters, nq = r.nq;
    DevMem mem, temp;
    Drain drain{stream};
    uint32_t *word, *selflag, *label_of;
    unsigned long long* maxlam;
    uint64_t *state_a, *state_b;
    Answers ans;
    ScratchLayout lay;
    lay.array(word, 64);
    lay.array(maxlam, clusters);
    lay.arrays(clusters, state_a, state_b);
    lay.arrays(clusters + 1, selflag, label_of);
    lay.arrays(nq, ans.labels, ans.prob, ans.score, ans.nearest, ans.w, ans.cluster);
    int rc = alloc_layout("hdbscan predict", mem, lay, err);  // (before anything is written)
    if (rc != OK) return rc;
    const uint32_t k32 = (uint32_t)clusters;

    HIP_TRY(hipMemsetAsync(word, 0, 256, stream));
    if (clusters != 0) HIP_TRY(hipMemsetAsync(maxlam, 0, clusters * 8, stream));
    const uint64_t checks = clusters + t.n + (r.counts != nullptr ? nq * r.k : 0);
    if (checks != 0) {
        hipLaunchKernelGGL(cp_check_kernel, grid_of(checks), dim3(256), 0, stream, t, r, maxlam, word);
        HIP_TRY(hipGetLastError());
    }
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, word, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad != 0u) {
        err = "hdbscan predict: refused:";
        if (bad & BAD_ROOT) err += " cluster_parent[0] is not UINT32_MAX;";
        if (bad & BAD_PARENT) err += " a cluster_parent[c] is not below c;";
        if (bad & BAD_POINT) err += " a point_cluster[v] is not below K;";
        if (bad & BAD_COUNT) err += " a counts[q] is above knbn;";
        if (bad & BAD_POS) err += " a used nbr_pos is not below n;";
        err.pop_back();
        return ERR_ARG;
    }

    if (clusters != 0) {  // the table, once per call
        hipLaunchKernelGGL(cp_jump_init_kernel, grid_of(clusters), dim3(256), 0, stream, t.parent, t.selected, k32, state_a);
        HIP_TRY(hipGetLastError());
        for (uint64_t reach = 1; reach <= clusters; reach *= 2) {  // a cluster's depth is below K, and one jump leads past cluster 0
            hipLaunchKernelGGL(cp_jump_round_kernel, grid_of(clusters), dim3(256), 0, stream, state_a, k32, state_b);
            HIP_TRY(hipGetLastError());
            std::swap(state_a, state_b);
        }
    }
    hipLaunchKernelGGL(cp_flag_kernel, grid_of(clusters + 1), dim3(256), 0, stream, t.selected, k32, selflag);
    HIP_TRY(hipGetLastError());
    rc = exclusive_scan_u32(temp, selflag, label_of, clusters + 1, stream, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(cp_assign_kernel, grid_of(nq * GROUP), dim3(256), 0, stream, t, r, state_a, label_of, maxlam, ans);
    HIP_TRY(hipGetLastError());

    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const struct { void* to; const void* from; } copies[] = {
        {out.labels, ans.labels}, {out.prob, ans.prob}, {out.score, ans.score}, {out.nearest, ans.nearest}, {out.w, ans.w}, {out.cluster, ans.cluster},
    };
    for (const auto& c : copies)
        if (c.to) HIP_TRY(hipMemcpyAsync(c.to, c.from, nq * 4, kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// A host form's tree in device memory: the arrays named into the call's layout, copied once the block is there
struct TreeUpload {
    float* core = nullptr;
    uint32_t *parent = nullptr, *pc = nullptr;
    float *birth = nullptr, *pw = nullptr;
    uint8_t* selected = nullptr;
    double* death = nullptr;

    void name(ScratchLayout& lay, const PredictTree& t) {
        lay.arrays(t.n, core, pc, pw);
        lay.arrays(t.clusters, parent, birth);
        lay.array(selected, t.clusters);
        if (t.death) lay.array(death, t.clusters);
    }
    int copy(const PredictTree& t, hipStream_t stream, std::string& err) {
        const struct { void* to; const void* from; uint64_t bytes; } ups[] = {
            {core, t.core, t.n * 4},          {pc, t.point_cluster, t.n * 4},         {pw, t.point_w, t.n * 4},           {parent, t.cluster_parent, t.clusters * 4},
            {birth, t.cluster_birth_w, t.clusters * 4}, {selected, t.selected, t.clusters}, {death, t.death, t.clusters * 8},
        };
        for (const auto& u : ups)
            if (u.from && u.bytes) HIP_TRY(hipMemcpyAsync(u.to, u.from, u.bytes, hipMemcpyHostToDevice, stream));
        return OK;
    }
};

Tree device_tree(const PredictTree& t) {
    return Tree{reinterpret_cast<const uint32_t*>(t.core), t.cluster_parent, reinterpret_cast<const uint32_t*>(t.cluster_birth_w), t.point_cluster,
                reinterpret_cast<const uint32_t*>(t.point_w), t.selected, t.death, (uint32_t)t.n, (uint32_t)t.clusters, t.eps};
}
Tree device_tree(const PredictTree& t, const TreeUpload& u) {
    return Tree{reinterpret_cast<const uint32_t*>(u.core), u.parent, reinterpret_cast<const uint32_t*>(u.birth), u.pc, reinterpret_cast<const uint32_t*>(u.pw),
                u.selected, t.death ? u.death : nullptr, (uint32_t)t.n, (uint32_t)t.clusters, t.eps};
}

}  // namespace

// hnswhdp_core_distances(_device) (capi.cpp refers to it weakly, capi_index.hpp): at least one point, core_k <= k.  Waits for `stream`.
int core_distances(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const CoreDistancesArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t n = dev.view().n;
    StagedGraph d;
    DevMem mem;
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)
    int rc = stage_directed_graph(dev, origin_id, a.k, a.ef, stream_v, d, err);
    if (rc != OK) return rc;
    uint32_t* core;
    ScratchLayout lay;
    lay.array(core, n);
    rc = alloc_layout("core distances", mem, lay, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(cp_core_kernel, grid_of(n), dim3(256), 0, stream, d.dists, d.counts, (uint32_t)a.k, (uint32_t)a.core_k, (uint32_t)n, core);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a.out_core, core, n * 4, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// hnswhdp_assign(_device): nq >= 1; what needs no device has been checked, and in the host form the tree and the rows too.
int hdbscan_assign(const HdbscanAssignArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (a.device >= 0) {
        const int rc = use_device_ordinal("hdbscan predict", a.device, err);
        if (rc != OK) return rc;
    }
    DeviceGuard on(a.device);
    HIP_TRY(on.status());
    const uint64_t nq = a.nq, slots = a.nq * a.k;
    Tree t = device_tree(a.tree);
    Rows r{a.nbr_pos, reinterpret_cast<const uint32_t*>(a.nbr_dist), a.counts, (uint32_t)nq, (uint32_t)a.k, (uint32_t)a.core_k};
    if (!host) return assign_rows(t, r, a.out, false, stream, err);
    DevMem mem;
    Drain drain{stream};
    TreeUpload up;
    uint32_t *up_pos, *up_dist, *up_counts;
    ScratchLayout lay;
    up.name(lay, a.tree);
    lay.arrays(slots, up_pos, up_dist);
    lay.array(up_counts, nq);
    int rc = alloc_layout("hdbscan predict", mem, lay, err);
    if (rc != OK) return rc;
    rc = up.copy(a.tree, stream, err);
    if (rc != OK) return rc;
    t = device_tree(a.tree, up);
    if (a.counts) {
        HIP_TRY(hipMemcpyAsync(up_pos, a.nbr_pos, slots * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(up_dist, a.nbr_dist, slots * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(up_counts, a.counts, nq * 4, hipMemcpyHostToDevice, stream));
        r.pos = up_pos;
        r.dist = up_dist;
        r.counts = up_counts;
    }
    return assign_rows(t, r, a.out, true, stream, err);
}

// hnswhdp_predict(_device): nq >= 1, at least one point, tree.n the index's points; the search's own arguments are the search's to
// check.  The rows are staged, searched, turned into positions and assigned, all in device memory.
int hdbscan_predict(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const HdbscanPredictArgs& a, bool host, void* stream_v, std::string& err) {
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const DeviceIndexView& v = dev.view();
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    const uint64_t nq = a.nq, k = a.k, slots = nq * k;
    DevMem mem;
    Drain drain{stream};
    GraphOrder ord;
    int rc = graph_order(dev, origin_id, ord, err);
    if (rc != OK) return rc;
    TreeUpload up;
    uint64_t* ids;
    float *dists, *up_q = nullptr;
    int32_t* rank;
    uint32_t *pos, *counts;
    uint8_t* layer;
    ScratchLayout lay;
    lay.array(ids, slots);
    lay.arrays(slots, dists, rank, pos);
    lay.array(counts, nq);
    lay.array(layer, slots);
    if (host) {
        up.name(lay, a.tree);
        lay.array(up_q, nq * a.d);
    }
    rc = alloc_layout("hdbscan predict", mem, lay, err);
    if (rc != OK) return rc;
    Tree t = device_tree(a.tree);
    const float* d_q = a.queries;
    if (host) {
        rc = up.copy(a.tree, stream, err);
        if (rc != OK) return rc;
        HIP_TRY(hipMemcpyAsync(up_q, a.queries, nq * a.d * 4, hipMemcpyHostToDevice, stream));
        t = device_tree(a.tree, up);
        d_q = up_q;
    }
    if (a.ef == 0) rc = exact_queries_device(dev, origin_id, d_q, nq, a.d, k, ids, dists, layer, rank, counts, stream_v, err);
    else rc = dev.search_device(d_q, nq, a.d, k, a.ef, ids, dists, layer, rank, counts, nullptr, stream_v, nullptr, 0, nullptr, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(cp_position_kernel, grid_of(slots), dim3(256), 0, stream, v, ord.d_rank, layer, rank, counts, (uint32_t)k, (uint32_t)slots, pos);
    HIP_TRY(hipGetLastError());
    const Rows r{pos, reinterpret_cast<const uint32_t*>(dists), counts, (uint32_t)nq, (uint32_t)k, (uint32_t)a.core_k};
    return assign_rows(t, r, a.out, host, stream, err);
}

}  // namespace hnswgpu
