// cluster_predict.hip -- HDBSCAN's third stage on the device (gfx950 only): new points are assigned to the clusters of a condensed
// tree -- approximate_predict --: the device side of hnswhdp_core_distances(_device), hnswhdp_assign(_device) and
// hnswhdp_predict(_device) of include/hnsw_mi355x_hdbscan_predict.h, which holds the contract word for word (the entries and the host
// forms' checks are in capi.cpp).  DESIGN.md "HDBSCAN: predict".
//
//   core_of_rows         the core distance of every row of D: spanning_forest.hip's kernel, through graph_internal.hpp
//   cp_check_kernel      K + n + nq k threads, BEFORE ANY TRAVERSAL OR GATHER: the tree's shared checks of cluster_tree.hpp, which
//                        also raise every cluster's max of the lambda bits, and counts[q] <= k, a used nbr_pos < n -- a fault sets a
//                        bit of one word, which is read back.
//   flagged_ancestors    ONCE PER CALL, cluster_select.hip's pointer doubling (cluster_tree.hpp) on `selected`, NEAREST: at the end
//                        best[c] is the nearest selected ancestor-or-self of c.
//   number_selected      cluster_select.hip's: the flags that rocPRIM scans into the labels' numbers (c is selected iff it is its own
//                        nearest selected cluster); the scan's last word is the number of selected clusters
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
#include "cluster_tree.hpp"
#include "exact_internal.hpp"
#include "graph_internal.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

// lanes per query of cp_assign_kernel: a power of two, at most 64
constexpr uint32_t GROUP = 16u;

// the later of two weights' bits under dist_order_bits; a tie keeps the earlier argument
__device__ __forceinline__ uint32_t later_bits(uint32_t w, uint32_t other) {
    return dist_order_bits(__uint_as_float(other)) > dist_order_bits(__uint_as_float(w)) ? other : w;
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
        (void)check_cluster(t.parent, t.birth, (uint32_t)i, maxlam, word);
        return;
    }
    i -= t.clusters;
    if (i < t.n) {
        check_vertex(t.point_cluster, t.point_w, i, t.clusters, maxlam, word);
        return;
    }
    i -= t.n;
    if (r.counts == nullptr || i >= (uint64_t)r.nq * r.k) return;
    const uint32_t q = (uint32_t)(i / r.k), s = (uint32_t)(i - (uint64_t)q * r.k), cnt = r.counts[q];
    if (cnt > r.k) {
        if (s == 0u) atomicOr(word, (uint32_t)BAD_COUNT);
        return;
    }
    if (s < cnt && r.pos[i] >= t.n) atomicOr(word, (uint32_t)BAD_POS);
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
// number of selected clusters.
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
    out.score[q] = t.death != nullptr && t.clusters != 0u ? glosh_score(lam, t.death[c]) : 0.0f;
    // a row with a neighbour has a cluster (K >= 1), else it is noise.  selected is {0}: the threshold
    const bool single_root = cnt != 0u && label_of[t.clusters] == 1u && t.selected[0] != 0u;
    label_of_point(lam, cnt != 0u ? (uint32_t)state[c] : NONE, single_root, t.eps, t.clusters, label_of, maxlam, out.labels[q], out.prob[q]);
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
        err = tree_refusal("hdbscan predict: refused:", bad);
        return ERR_ARG;
    }

    if (clusters != 0) {  // the table, once per call
        rc = flagged_ancestors<uint8_t, true>(t.parent, t.selected, clusters, state_a, state_b, stream, err);
        if (rc != OK) return rc;
    }
    rc = number_selected(state_a, clusters, nullptr, selflag, label_of, temp, stream, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(cp_assign_kernel, grid_of(nq * GROUP), dim3(256), 0, stream, t, r, state_a, label_of, maxlam, ans);
    HIP_TRY(hipGetLastError());
    const uint64_t bytes = nq * 4;
    return copy_out({{out.labels, ans.labels, bytes}, {out.prob, ans.prob, bytes}, {out.score, ans.score, bytes}, {out.nearest, ans.nearest, bytes},
                     {out.w, ans.w, bytes}, {out.cluster, ans.cluster, bytes}},
                    host, stream, err);
}

// the caller's tree as the kernels read it; upload_tree: a host form's arrays come along in the call's block
Tree device_tree(const PredictTree& t) {
    return Tree{reinterpret_cast<const uint32_t*>(t.core), t.cluster_parent, reinterpret_cast<const uint32_t*>(t.cluster_birth_w), t.point_cluster,
                reinterpret_cast<const uint32_t*>(t.point_w), t.selected, t.death, (uint32_t)t.n, (uint32_t)t.clusters, t.eps};
}
void upload_tree(Uploads& ups, ScratchLayout& lay, Tree& t) {
    ups.brings(lay, t.n, t.core, t.point_cluster, t.point_w);
    ups.brings(lay, t.clusters, t.parent, t.birth, t.selected, t.death);
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
    rc = core_of_rows(d.dists, d.counts, a.k, a.core_k, n, core, stream_v, err);
    if (rc != OK) return rc;
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
    Uploads ups;
    ScratchLayout lay;
    upload_tree(ups, lay, t);
    ups.brings(lay, slots, r.pos, r.dist);
    ups.bring(lay, r.counts, nq);
    int rc = alloc_layout("hdbscan predict", mem, lay, err);
    if (rc != OK) return rc;
    rc = copy_uploads(ups, stream, err);
    if (rc != OK) return rc;
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
    Tree t = device_tree(a.tree);
    const float* d_q = a.queries;
    Uploads ups;
    uint64_t* ids;
    float* dists;
    int32_t* rank;
    uint32_t *pos, *counts;
    uint8_t* layer;
    ScratchLayout lay;
    lay.array(ids, slots);
    lay.arrays(slots, dists, rank, pos);
    lay.array(counts, nq);
    lay.array(layer, slots);
    if (host) {
        upload_tree(ups, lay, t);
        ups.bring(lay, d_q, nq * a.d);
    }
    rc = alloc_layout("hdbscan predict", mem, lay, err);
    if (rc != OK) return rc;
    rc = copy_uploads(ups, stream, err);
    if (rc != OK) return rc;
    if (a.ef == 0) rc = exact_device(dev, origin_id, ExactCall{d_q, nullptr, nq, a.d, k, nullptr, 0, nullptr, {ids, dists, layer, rank, counts}}, stream, err);
    else rc = dev.search_device(d_q, nq, a.d, k, a.ef, ids, dists, layer, rank, counts, nullptr, stream_v, nullptr, 0, nullptr, err);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(cp_position_kernel, grid_of(slots), dim3(256), 0, stream, v, ord.d_rank, layer, rank, counts, (uint32_t)k, (uint32_t)slots, pos);
    HIP_TRY(hipGetLastError());
    const Rows r{pos, reinterpret_cast<const uint32_t*>(dists), counts, (uint32_t)nq, (uint32_t)k, (uint32_t)a.core_k};
    return assign_rows(t, r, a.out, host, stream, err);
}

}  // namespace hnswgpu
