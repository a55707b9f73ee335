// capi_index.hpp -- what is behind the opaque hnswgpu_index handle of include/hnsw_mi355x.h (and its extensions hnsw_mi355x_hdbscan.h, hnsw_mi355x_hdbscan_select.h, hnsw_mi355x_hdbscan_predict.h and hnsw_mi355x_dbscan.h),
// for the translation units that implement the C ABI: capi.cpp, which holds the entries, and the .hip units that hold their device
// side (exact_knn.hip, which also holds hnswgpu_exact_search_batch(_device) itself; exact_range.hip; knn_graph.hip; range_search.hip; symmetric_graph.hip;
// graph_components.hip; spanning_forest.hip; dendrogram.hip; condensed_tree.hip; cluster_select.hip; cluster_predict.hip; dbscan.hip).  Private: not installed, not part of the ABI.
// Three parts: the handle; the checks that entries share (empty index, resident replica, sorted filter, the limits of an exact call,
// the zeroed k-NN answer, the tail), which live once, in capi.cpp, and are declared here as capi_* for the entries outside it; and
// the device side of every host / _device pair, declared ONCE, here, with its arguments' struct (HNSWGPU_DEVICE_SIDE of
// search_device.hpp makes capi.cpp's references weak).  A pair of entries is one body in capi.cpp that calls both.  The HIP host
// helpers of the .hip units (HIP_TRY, DeviceGuard, DevMem, round_up) are in hip_host.hpp, which this header -- compiled by plain g++
// too -- does not include.
#pragma once
#include <exception>
#include <map>
#include <new>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/hnsw_mi355x.h"
#include "../../include/hnsw_mi355x_hdbscan.h"
#include "../../include/hnsw_mi355x_hdbscan_select.h"
#include "../../include/hnsw_mi355x_hdbscan_predict.h"
#include "../../include/hnsw_mi355x_dbscan.h"
#include "builder.hpp"
#include "flat_index.hpp"
#include "search_device.hpp"

struct hnswgpu_index {
    // Searches take this lock shared (they are `&self` in the reference: concurrent calls on one handle are legal);
    // whatever changes the graph or the set of replicas (insert, upload, dump of a stale flat view) takes it exclusive.
    std::shared_mutex mu;
    std::unique_ptr<hnswgpu::FlatIndex> flat;        // dump-order view; rebuilt from `builder` when stale
    std::unique_ptr<hnswgpu::GraphBuilder> builder;  // construction state (created lazily for reloaded indexes)
    bool flat_stale = false;
    std::map<int, std::unique_ptr<hnswgpu::DeviceIndex>> replicas;  // HBM replicas by HIP device ordinal
    int primary = -1;                       // device of the single-GPU entry points
    bool dev_stale = true;
    int strict_ties = -1;  // -1: library default (env HNSWGPU_STRICT_TIES, else on)
    int arithmetic = 0;    // HNSWGPU_ARITH_*
    int storage = 0;       // HNSWGPU_STORAGE_*: how the replicas hold the rows (handed to each one before its upload)
    hnswgpu::BuildParams params;

    const hnswgpu::FlatIndex* get_flat() {  // exclusive lock held (or the view is known to be fresh)
        if (builder && (flat_stale || !flat)) {
            flat.reset(new hnswgpu::FlatIndex());
            builder->finalize(*flat);
            flat_stale = false;
            dev_stale = true;
        }
        return flat.get();
    }
    bool fresh() const { return flat && !flat_stale; }
    hnswgpu::DeviceIndex* replica(int device) const {
        auto it = replicas.find(device);
        return it == replicas.end() || !it->second->ready() ? nullptr : it->second.get();
    }
};

namespace hnswgpu {
// defined in capi.cpp, for the entry points that live in other translation units:
// sets the calling thread's hnswgpu_last_error() message and returns `code`
int capi_fail(int code, const std::string& msg);
// the replica a call on the primary device uses, uploaded first where need be (`sl`: the handle's lock, held shared), for the entries
// that read rows outside the search path: HNSWGPU_ERR_ARG when the replica turns out to be a half one (the index's storage was changed
// while the lock was given up for the upload)
int capi_primary_f32_replica(hnswgpu_index* idx, std::shared_lock<std::shared_mutex>& sl, DeviceIndex** out);
// HNSWGPU_OK, or -- the index is set to HNSWGPU_STORAGE_F16 -- HNSWGPU_ERR_ARG with a message that names `what`: the calls that
// read rows outside the search path (exact k-NN / range / graph, the stored-point queries) exist for f32 rows only
int capi_refuse_f16(const hnswgpu_index* idx, const char* what);
// the shared checks of capi.cpp that hnswgpu_exact_search_batch(_device) -- defined in exact_knn.hip -- call too.  The handle's lock
// is held where the index is read.
// the end of an entry: HNSWGPU_OK, or `rc` with `err` as the thread's message
int capi_finish(int rc, const std::string& err);
bool capi_index_empty(const hnswgpu_index* idx);
// the primary replica as it is (nothing is uploaded), or HNSWGPU_ERR_DEVICE "index is not resident on a device ...";
// need_flat: the host view has to be there too
int capi_resident_replica(const hnswgpu_index* idx, bool need_flat, DeviceIndex** dev);
// HNSWGPU_ERR_ARG unless ids[0..n) (host memory) ascend
int capi_check_sorted_filter(const uint64_t* ids, uint64_t n);
// the limits of an exact k-NN call: buffers, knbn, nq, d, the filter pointer, the arithmetic, the storage -- in this order
int capi_check_exact_call(const hnswgpu_index* idx, const void* queries, uint64_t nq, uint64_t d, uint64_t k, const void* allowed, uint64_t n_allowed,
                          const void* out_ids, const void* out_dists, const void* out_counts);
// the k-NN answer of an index without a point: counts, ids, dists and (where given) layer and rank of nq rows zeroed
void capi_zero_knn_answers(uint64_t nq, uint64_t k, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts);

// ---- The device side of the batched entries: what capi.cpp calls behind its argument checks, each defined in the .hip unit named.
// One shape for all of them: (the replica and its DataIds, where the call reads an index; the call's arguments in a struct; host;
// stream; err).  host: every buffer of the struct is plain host memory and `stream` is nullptr; else device memory and `stream` is
// the caller's, waited for before the function returns.  The arguments have been checked.  Each declaration carries
// HNSWGPU_DEVICE_SIDE (search_device.hpp): capi.cpp, and only capi.cpp, refers to these functions weakly.

// hnswgpu_exact_search_batch_filter_set(_device), exact_knn.hip: the exact k-NN of every query q under filter filter_of[q] of the set
struct ExactSetArgs {
    const float* queries;  // nq x d
    uint64_t nq, d, k;
    FilterSet set;         // host: validated
    uint64_t* out_ids;     // nq x k, like the three below
    float* out_dists;
    uint8_t* out_layer;    // may be nullptr
    int32_t* out_rank;     // may be nullptr
    uint32_t* out_counts;  // [nq]
};
HNSWGPU_DEVICE_SIDE int exact_filter_set(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactSetArgs& a, bool host, void* stream,
                                         std::string& err);
// hnswgpu_exact_range_search_batch(_device), exact_range.hip.  Returns HNSWGPU_ERR_CAPACITY, the offsets complete and no out slot
// written, when the answers need more than cap slots.
struct ExactRangeCallArgs {
    const float* queries;  // nq x d
    const float* radii;    // [nq]
    uint64_t nq, d;
    const uint64_t* allowed;  // not nullptr: a filter, even when it is empty
    uint64_t n_allowed;
    uint64_t cap;
    uint64_t* out_offsets;  // [nq + 1]
    uint64_t* out_ids;      // cap slots each; may be nullptr with cap == 0, the count-only call
    float* out_dists;
    uint8_t* out_layer;     // may be nullptr
    int32_t* out_rank;      // may be nullptr
};
HNSWGPU_DEVICE_SIDE int exact_range(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactRangeCallArgs& a, bool host, void* stream,
                                    std::string& err);
// hnswgpu_graph_search_batch(_device) and hnswgpu_exact_graph_batch(_device), knn_graph.hip.  They return ERR_ARG, nothing searched
// and no out slot written, when an id of point_ids names no point.
struct GraphCallArgs {
    const uint64_t* point_ids;  // nullptr: every point (np == the number of points, checked by the caller)
    uint64_t np, k;
    uint64_t ef;                // graph_search only
    const uint64_t* allowed;    // exact_graph only, like n_allowed; not nullptr: a filter, even when it is empty
    uint64_t n_allowed;
    uint64_t* out_ids;          // np x k, like the three below
    float* out_dists;
    uint8_t* out_layer;         // may be nullptr
    int32_t* out_rank;          // may be nullptr
    uint32_t* out_counts;       // [np]
};
HNSWGPU_DEVICE_SIDE int graph_search(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, bool host, void* stream, std::string& err);
HNSWGPU_DEVICE_SIDE int exact_graph(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphCallArgs& a, bool host, void* stream,
                                    std::string& err);
// hnswgpu_range_search_batch(_device), range_search.hip: the rounds of every group of queries through DeviceIndex::search_device.
// filtered: allowed is a filter even when it is empty.  dev == nullptr (device form on an empty index, or with no query): the offsets
// are zeroed on the caller's stream.  Returns HNSWGPU_ERR_CAPACITY, the offsets complete, when the answers need more than cap slots.
struct RangeSearchArgs {
    const float* queries;  // nq x d
    const float* radii;    // [nq]
    uint64_t nq, d, ef_first, ef_max;
    const uint64_t* allowed;
    uint64_t n_allowed;
    bool filtered;
    uint64_t cap;
    uint64_t* out_offsets;  // [nq + 1]
    uint64_t* out_ids;      // cap slots each; all four nullptr: the count-only call
    float* out_dists;
    uint8_t* out_layer;
    int32_t* out_rank;
    uint32_t* out_ef;       // [nq], may be nullptr
    uint8_t* out_flags;     // [nq], may be nullptr
};
HNSWGPU_DEVICE_SIDE int range_search(DeviceIndex* dev, const RangeSearchArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswgpu_symmetric_graph(_device), defined in symmetric_graph.hip: the
// directed graph of every point through exact_graph (ef == 0) or graph_search, made undirected (the arguments have been checked).
// host: the out arrays are plain host memory; else device memory and `stream` is the caller's.  Returns HNSWGPU_ERR_CAPACITY, the
// offsets complete and no out slot written, when the answer needs more than cap slots.  dev == nullptr (device entry on an empty
// index): the one offset is zeroed.
struct SymGraphArgs {
    uint64_t k, ef;
    uint32_t mode;          // HNSWGPU_SYM_*
    uint64_t cap;
    uint64_t* out_offsets;  // [n + 1]
    uint32_t* out_pos;      // cap slots each; out_pos == nullptr: the count-only call
    uint64_t* out_ids;      // may be nullptr
    float* out_dists;
    uint8_t* out_layer;     // may be nullptr
    int32_t* out_rank;      // may be nullptr
};
HNSWGPU_DEVICE_SIDE int symmetric_graph(DeviceIndex* dev, const std::vector<uint64_t>& origin_id, const SymGraphArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswgpu_graph_components(_device) and hnswgpu_csr_components(_device), defined in graph_components.hip
// (the arguments have been checked; at least one vertex).  host: the arrays are plain host memory;
// else device memory and `stream` is the caller's.  out_n is host memory either way.  csr_components returns ERR_ARG, no out slot
// written, when its validation kernels refuse the graph.
struct ComponentsArgs {
    uint64_t k, ef;
    uint32_t mode;        // HNSWGPU_SYM_*
    bool has_cut;
    float max_dist;
    uint32_t* out_label;  // [n]
    uint32_t* out_sizes;  // [n], may be nullptr
    uint64_t* out_n;
};
HNSWGPU_DEVICE_SIDE int graph_components(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ComponentsArgs& a, bool host, void* stream, std::string& err);
struct CsrComponentsArgs {
    int device;
    uint64_t n;
    const uint64_t* offsets;  // [n + 1]
    const uint32_t* cols;     // [offsets[n]]
    const float* dists;       // [offsets[n]], read only under a cut
    bool has_cut;
    float max_dist;
    uint32_t* out_label;
    uint32_t* out_sizes;
    uint64_t* out_n;
};
HNSWGPU_DEVICE_SIDE int csr_components(const CsrComponentsArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswgpu_graph_spanning_forest(_device) and hnswgpu_csr_spanning_forest(_device), defined in spanning_forest.hip
// (the arguments have been checked; at least two vertices).  host: the arrays are plain host
// memory; else device memory and `stream` is the caller's.  out_n is host memory either way.  csr_spanning_forest returns ERR_ARG,
// no out slot written, when its validation kernels refuse the graph.
struct ForestArgs {
    uint64_t k, ef;
    uint32_t mode;    // HNSWGPU_SYM_*
    uint64_t core_k;  // 0 .. k
    uint32_t* out_a;  // [n - 1]
    uint32_t* out_b;  // [n - 1]
    float* out_w;     // [n - 1]
    uint64_t* out_n;
};
HNSWGPU_DEVICE_SIDE int graph_spanning_forest(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ForestArgs& a, bool host, void* stream, std::string& err);
struct CsrForestArgs {
    int device;
    uint64_t n;
    const uint64_t* offsets;  // [n + 1]
    const uint32_t* cols;     // [offsets[n]]
    const float* dists;       // [offsets[n]], may be nullptr: every weight +0
    uint32_t* out_a;
    uint32_t* out_b;
    float* out_w;
    uint64_t* out_n;
};
HNSWGPU_DEVICE_SIDE int csr_spanning_forest(const CsrForestArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswgpu_forest_dendrogram(_device) and hnswgpu_graph_dendrogram(_device), defined in dendrogram.hip
// (the arguments have been checked; forest form: 1 <= m <= n - 1; index form: at least two vertices).
// host: the arrays are plain host memory -- a forest form's ends have then passed their checks on the host --; else device memory
// and `stream` is the caller's.  forest_dendrogram returns ERR_ARG, no out slot written, when an end is not below n, an edge joins a
// vertex to itself or the edges hold a cycle.  graph_dendrogram runs graph_spanning_forest into device memory and goes on from there.
struct DendrogramArgs {
    int device;
    uint64_t n, m;
    const uint32_t* a;    // [m]
    const uint32_t* b;    // [m]
    uint32_t* out_left;   // [m]
    uint32_t* out_right;  // [m]
    uint32_t* out_size;   // [m]
};
HNSWGPU_DEVICE_SIDE int forest_dendrogram(const DendrogramArgs& a, bool host, void* stream, std::string& err);
struct GraphDendrogramArgs {
    ForestArgs forest;    // out_n is host memory either way
    uint32_t* out_left;   // [n - 1]
    uint32_t* out_right;  // [n - 1]
    uint32_t* out_size;   // [n - 1]
};
HNSWGPU_DEVICE_SIDE int graph_dendrogram(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphDendrogramArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswhdb_forest(_device) and hnswhdb_graph(_device), defined in condensed_tree.hip
// (the arguments have been checked; forest form: n >= 1, m <= n - 1; index form: at least one point;
// 2 <= min_cluster_size <= 2^31 - 1, a known method).  host: the arrays are plain host memory -- a forest form's ends and weights
// have then passed their checks on the host --; else device memory and `stream` is the caller's.  The two counts are host memory
// either way.  forest_hdbscan runs forest_dendrogram on device buffers and returns what it refuses, and ERR_ARG, no out slot
// written, when the weights descend.  graph_hdbscan runs graph_dendrogram into device scratch and goes on from there.
struct HdbscanOut {
    int32_t* labels;           // [n]
    float* prob;               // [n], may be nullptr, like every array below
    uint32_t* point_cluster;   // [n]
    float* point_w;            // [n]
    uint32_t* cluster_parent;  // [hnswhdb_max_clusters(n, min_cluster_size)], like the four below
    float* cluster_birth_w;
    uint32_t* cluster_size;
    double* stability;
    uint8_t* selected;
    uint64_t* n_clusters;
    uint64_t* n_labels;
};
struct ForestHdbscanArgs {
    int device;
    uint64_t n, m;
    const uint32_t* a;  // [m]
    const uint32_t* b;  // [m]
    const float* w;     // [m]
    uint64_t min_cluster_size;
    uint32_t method;    // HNSWGPU_SELECT_*
    HdbscanOut out;
};
HNSWGPU_DEVICE_SIDE int forest_hdbscan(const ForestHdbscanArgs& a, bool host, void* stream, std::string& err);
struct GraphHdbscanArgs {
    ForestArgs forest;    // out_a, out_b, out_w may be nullptr; out_n is host memory either way
    uint32_t* out_left;   // [n - 1], may be nullptr, like the two below
    uint32_t* out_right;
    uint32_t* out_size;
    uint64_t min_cluster_size;
    uint32_t method;
    HdbscanOut out;
};
HNSWGPU_DEVICE_SIDE int graph_hdbscan(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphHdbscanArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswhds_select(_device), defined in cluster_select.hip (the arguments have been checked: 1 <= n, K <= 2^31 - 1,
// a known method, allow_single_cluster 0 or 1, eps >= 0, the six input arrays and out_labels there).  host: the arrays are plain
// host memory and have passed the tree's checks on the host; else device memory, checked by kernel before anything walks the tree,
// and `stream` is the caller's.  out_n_labels is host memory either way.  ERR_ARG, no out slot written, when the checks refuse.
struct HdbscanSelectArgs {
    int device;
    uint64_t n, clusters;
    const uint32_t* cluster_parent;  // [clusters], like the three below
    const float* cluster_birth_w;
    const uint32_t* cluster_size;
    const double* stability;
    const uint32_t* point_cluster;   // [n]
    const float* point_w;            // [n]
    uint32_t method;                 // HNSWGPU_SELECT_*
    uint32_t allow_single_cluster;
    float eps;
    uint64_t max_cluster_size;       // 0: no limit
    uint8_t* out_selected;           // [clusters], may be nullptr
    int32_t* out_labels;             // [n]
    float* out_prob;                 // [n], may be nullptr, like the two below
    float* out_score;                // [n]
    double* out_death;               // [clusters]
    uint64_t* out_n_labels;
};
HNSWGPU_DEVICE_SIDE int hdbscan_select(const HdbscanSelectArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswhdp_core_distances(_device), hnswhdp_assign(_device) and hnswhdp_predict(_device), defined in
// cluster_predict.hip (the arguments have been checked: what needs no device and, in the host forms, the tree and the rows on the
// host).  host: the arrays are plain host memory; else device memory, checked by kernel before anything walks the tree or gathers, and
// `stream` is the caller's.  ERR_ARG, no out slot written, when the checks refuse.
struct CoreDistancesArgs {
    uint64_t k, ef, core_k;  // core_k <= k
    float* out_core;         // [n]
};
HNSWGPU_DEVICE_SIDE int core_distances(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const CoreDistancesArgs& a, bool host, void* stream, std::string& err);
struct PredictTree {
    uint64_t n, clusters;
    const float* core;               // [n], like point_cluster and point_w
    const uint32_t* cluster_parent;  // [clusters], like the two below
    const float* cluster_birth_w;
    const uint32_t* point_cluster;
    const float* point_w;
    const uint8_t* selected;
    float eps;
    const double* death;             // [clusters], may be nullptr
};
struct PredictOut {
    int32_t* labels;    // [nq]
    float* prob;        // [nq], may be nullptr, like every array below
    float* score;
    uint32_t* nearest;
    float* w;
    uint32_t* cluster;
};
struct HdbscanAssignArgs {
    int device;               // below 0: the caller's current device (predict on an index without a point)
    uint64_t nq, k;
    const uint32_t* nbr_pos;  // nq x k, like nbr_dist
    const float* nbr_dist;
    const uint32_t* counts;   // [nq]; nullptr: every row is empty
    uint64_t core_k;
    PredictTree tree;
    PredictOut out;
};
HNSWGPU_DEVICE_SIDE int hdbscan_assign(const HdbscanAssignArgs& a, bool host, void* stream, std::string& err);
struct HdbscanPredictArgs {
    const float* queries;  // nq x d
    uint64_t nq, d, k, ef, core_k;
    PredictTree tree;      // n: the index's points
    PredictOut out;
};
HNSWGPU_DEVICE_SIDE int hdbscan_predict(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const HdbscanPredictArgs& a, bool host, void* stream, std::string& err);
// the device side of hnswdbs_exact(_device) and hnswdbs_csr(_device), defined in dbscan.hip (the arguments have been checked; at least
// one vertex; 1 <= min_samples, eps no NaN).  host: the arrays are plain host memory -- a CSR form's graph has then passed its checks
// on the host --; else device memory and `stream` is the caller's.  out_n is host memory either way.  csr_dbscan returns ERR_ARG, no
// out slot written, when its validation kernels refuse the graph.
struct DbscanOut {
    int32_t* label;    // [n]
    uint8_t* core;     // [n], may be nullptr, like the two below
    uint32_t* count;
    uint32_t* anchor;
    uint64_t* out_n;
};
struct DbscanArgs {
    float eps;
    uint64_t min_samples;
    DbscanOut out;
};
HNSWGPU_DEVICE_SIDE int exact_dbscan(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const DbscanArgs& a, bool host, void* stream, std::string& err);
struct CsrDbscanArgs {
    int device;
    uint64_t n;
    const uint64_t* offsets;  // [n + 1]
    const uint32_t* cols;     // [offsets[n]]
    const float* dists;       // [offsets[n]], may be nullptr: every entry counts, every weight +0
    uint32_t add_self;        // 0 or 1
    DbscanArgs call;
};
HNSWGPU_DEVICE_SIDE int csr_dbscan(const CsrDbscanArgs& a, bool host, void* stream, std::string& err);
}  // namespace hnswgpu

// No C++ exception may cross the C ABI: every entry point is `try { ... HNSWGPU_CAPI_GUARD_END(ret)`
#define HNSWGPU_CAPI_GUARD_END(ret)                                                                    \
    } catch (const std::bad_alloc&) {                                                                   \
        hnswgpu::capi_fail(HNSWGPU_ERR_ARG, "out of memory");                                           \
        return ret;                                                                                     \
    } catch (const std::exception& e) {                                                                 \
        hnswgpu::capi_fail(HNSWGPU_ERR_FORMAT, std::string("internal error: ") + e.what());             \
        return ret;                                                                                     \
    } catch (...) {                                                                                     \
        hnswgpu::capi_fail(HNSWGPU_ERR_FORMAT, "internal error");                                       \
        return ret;                                                                                     \
    }
