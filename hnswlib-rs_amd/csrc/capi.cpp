// capi.cpp -- the C ABI declared in include/hnsw_mi355x.h: the thin hnswgpu_* entry points and the
// name/layout-compatible replacements of the reference's own f32 FFI (src/libext.rs).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

// (this file's references to the device side are weak: search_device.hpp, HNSWGPU_DEVICE_SIDE)
#define HNSWGPU_WEAK_DEVICE_SIDE
#include "../../include/hnsw_mi355x.h"
#include "builder.hpp"
#include "datamap.hpp"
#include "dist_order.hpp"
#include "flat_index.hpp"
#include "hnswio.hpp"
#include "search_device.hpp"
#include "worker_pool.hpp"
#include "capi_index.hpp"

using namespace hnswgpu;

static thread_local std::string g_last_error;
static int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
// worker threads of one call: whatever was spawned is joined when this goes out of scope -- also when a later spawn throws,
// so that no joinable std::thread is ever destroyed (that would be std::terminate, past every guard)
struct JoinAll {
    std::vector<std::thread> th;
    template <class F> void spawn(F&& f) { th.emplace_back(std::forward<F>(f)); }
    ~JoinAll() {
        for (auto& t : th)
            if (t.joinable()) t.join();
    }
};
// a call that SUCCEEDED with something worth telling (hnswgpu_last_error() returns it until the next failure or note)
static void note(const std::string& msg) { g_last_error = msg; }
// No C++ exception may cross the C ABI (the host may be Rust, Julia or C): every entry point runs inside this guard.
#define CAPI_GUARD_BEGIN try {
#define CAPI_GUARD_END(ret) HNSWGPU_CAPI_GUARD_END(ret)

static int default_device() {
    const char* e = std::getenv("HNSWGPU_DEVICE");
    return e ? std::atoi(e) : 0;
}

// make sure an HBM replica on `device` (< 0: the primary / default one) reflects the host graph.  Exclusive lock held.
static int ensure_device(hnswgpu_index* idx, int device) {
    const FlatIndex* f = idx->get_flat();
    if (!f || f->n == 0) return fail(HNSWGPU_ERR_EMPTY, "index is empty");
    if (idx->dev_stale) {  // the graph changed: every replica is out of date
        idx->replicas.clear();
        idx->dev_stale = false;
    }
    if (device < 0) device = idx->primary >= 0 ? idx->primary : default_device();
    if (!idx->replica(device)) {
        std::unique_ptr<DeviceIndex> dev(new DeviceIndex());
        std::string err;
        dev->set_storage(idx->storage);
        int rc = dev->upload(*f, device, err);
        if (rc != OK) return fail(rc, err);
        if (idx->strict_ties >= 0) dev->set_strict_ties(idx->strict_ties != 0);
        dev->set_arithmetic(idx->arithmetic);
        idx->replicas[device] = std::move(dev);
    }
    if (idx->primary < 0 || !idx->replica(idx->primary)) idx->primary = device;
    return HNSWGPU_OK;
}
// the replica a search on the primary device uses; takes the exclusive lock only when something has to be (re)built
static int primary_replica(hnswgpu_index* idx, std::shared_lock<std::shared_mutex>& sl, DeviceIndex** out) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (idx->fresh() && !idx->dev_stale && idx->primary >= 0 && idx->replica(idx->primary)) {
            *out = idx->replica(idx->primary);
            return HNSWGPU_OK;
        }
        sl.unlock();
        {
            std::unique_lock<std::shared_mutex> xl(idx->mu);
            int rc = ensure_device(idx, -1);
            if (rc != HNSWGPU_OK) { xl.unlock(); sl.lock(); return rc; }
        }
        sl.lock();
    }
    return fail(HNSWGPU_ERR_DEVICE, "index changed while a search was starting");
}

// primary_replica for the entries that read rows outside the search path.  Their argument checks refused an F16 index under the
// shared lock, but primary_replica gives that lock up while it uploads: a hnswgpu_set_storage(F16) in between makes the replica a
// half one, which those kernels would read as f32, past its end.  So the replica itself is asked.
static int primary_f32_replica(hnswgpu_index* idx, std::shared_lock<std::shared_mutex>& sl, DeviceIndex** out) {
    int rc = primary_replica(idx, sl, out);
    if (rc != HNSWGPU_OK) return rc;
    if ((*out)->storage() != STORAGE_F32) {
        *out = nullptr;
        return fail(HNSWGPU_ERR_ARG, "this call reads f32 rows only: the index was set to HNSWGPU_STORAGE_F16 while the call was starting "
                                     "(hnswgpu_set_storage(idx, HNSWGPU_STORAGE_F32) first)");
    }
    return HNSWGPU_OK;
}

// ---- what the batched entries share: a new pair of entries is written by calling these.  Where they read the index the handle's
// lock is held.
static uint64_t index_nb_point(const hnswgpu_index* idx) { return idx->builder ? idx->builder->nb_point() : (idx->flat ? idx->flat->n : 0); }
static uint64_t index_dimension(const hnswgpu_index* idx) { return idx->builder ? idx->builder->dimension() : (idx->flat ? idx->flat->dimension : 0); }
static bool index_empty(const hnswgpu_index* idx) { return index_nb_point(idx) == 0; }
// the end of an entry: the device side's status and message handed on
static int finish(int rc, const std::string& err) { return rc != OK ? fail(rc, err) : HNSWGPU_OK; }
// the replica a _device entry works on: the caller's buffers live on a device already, so nothing is uploaded from here.
// need_flat: the call reads the host view too (its DataIds)
static int resident_replica(const hnswgpu_index* idx, bool need_flat, DeviceIndex** dev) {
    *dev = idx->primary >= 0 ? idx->replica(idx->primary) : nullptr;
    if (!*dev || idx->dev_stale || idx->flat_stale || (need_flat && !idx->flat))
        return fail(HNSWGPU_ERR_DEVICE, "index is not resident on a device: call hnswgpu_upload first");
    return HNSWGPU_OK;
}
// one filter for the batch, in host memory: `impl FilterT for Vec<usize>` is a binary search, so the vector must be sorted
static int check_sorted_filter(const uint64_t* ids, uint64_t n) {
    for (uint64_t i = 1; i < n; ++i)
        if (ids[i - 1] > ids[i]) return fail(HNSWGPU_ERR_ARG, "the id vector of a filter must be sorted ascending");
    return HNSWGPU_OK;
}
// the limits of an exact k-NN call, one filter or a set of them (which hands in no `allowed`)
static int check_exact_call(const hnswgpu_index* idx, const void* queries, uint64_t nq, uint64_t d, uint64_t k, const void* allowed, uint64_t n_allowed,
                            const void* out_ids, const void* out_dists, const void* out_counts) {
    const uint64_t dim = index_dimension(idx);
    if (nq != 0 && (!queries || !out_ids || !out_dists || !out_counts)) return fail(HNSWGPU_ERR_ARG, "null buffer");
    if (k == 0) return fail(HNSWGPU_ERR_ARG, "knbn must be > 0");
    // (list_insert of exact_knn.hip costs O(k / 64) steps per insertion: 4096 is the largest knbn that was run at size)
    if (k > 4096) return fail(HNSWGPU_ERR_ARG, "exact search: knbn above 4096");
    if (nq > 0xFFFFFFF0ull) return fail(HNSWGPU_ERR_ARG, "too many queries in one batch");
    if (dim != 0 && d != dim) return fail(HNSWGPU_ERR_ARG, "query dimension differs from the index dimension");
    if (n_allowed != 0 && !allowed) return fail(HNSWGPU_ERR_ARG, "null filter");
    if (idx->arithmetic != HNSWGPU_ARITH_SCALAR)
        return fail(HNSWGPU_ERR_ARG, "exact search answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
    return capi_refuse_f16(idx, "exact search");
}
// a k-NN answer on an index without a point: every count 0, every slot zeroed
static void zero_knn_answers(uint64_t nq, uint64_t k, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts) {
    if (nq == 0) return;
    std::memset(out_counts, 0, nq * sizeof(uint32_t));
    std::memset(out_ids, 0, nq * k * sizeof(uint64_t));
    std::memset(out_dists, 0, nq * k * sizeof(float));
    if (out_layer) std::memset(out_layer, 0, nq * k);
    if (out_rank) std::memset(out_rank, 0, nq * k * sizeof(int32_t));
}

namespace hnswgpu {
int capi_fail(int code, const std::string& msg) { return fail(code, msg); }
int capi_finish(int rc, const std::string& err) { return finish(rc, err); }
bool capi_index_empty(const hnswgpu_index* idx) { return index_empty(idx); }
int capi_resident_replica(const hnswgpu_index* idx, bool need_flat, DeviceIndex** dev) { return resident_replica(idx, need_flat, dev); }
int capi_check_sorted_filter(const uint64_t* ids, uint64_t n) { return check_sorted_filter(ids, n); }
int capi_check_exact_call(const hnswgpu_index* idx, const void* queries, uint64_t nq, uint64_t d, uint64_t k, const void* allowed, uint64_t n_allowed,
                          const void* out_ids, const void* out_dists, const void* out_counts) {
    return check_exact_call(idx, queries, nq, d, k, allowed, n_allowed, out_ids, out_dists, out_counts);
}
void capi_zero_knn_answers(uint64_t nq, uint64_t k, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts) {
    zero_knn_answers(nq, k, out_ids, out_dists, out_layer, out_rank, out_counts);
}
int capi_primary_f32_replica(hnswgpu_index* idx, std::shared_lock<std::shared_mutex>& sl, DeviceIndex** out) { return primary_f32_replica(idx, sl, out); }
int capi_refuse_f16(const hnswgpu_index* idx, const char* what) {
    if (idx->storage != HNSWGPU_STORAGE_F16) return HNSWGPU_OK;
    return fail(HNSWGPU_ERR_ARG, std::string(what) + " reads f32 rows only: the index is set to HNSWGPU_STORAGE_F16 "
                                 "(hnswgpu_set_storage(idx, HNSWGPU_STORAGE_F32) first)");
}
}  // namespace hnswgpu

extern "C" {

const char* hnswgpu_last_error(void) { return g_last_error.c_str(); }

int hnswgpu_load_dump(const char* dir, const char* basename, int dist, hnswgpu_index** out) {
    CAPI_GUARD_BEGIN
    if (!dir || !basename || !out) return fail(HNSWGPU_ERR_ARG, "null argument");
    *out = nullptr;
    std::unique_ptr<hnswgpu_index> h(new hnswgpu_index());
    h->flat.reset(new FlatIndex());
    std::string err;
    int rc = load_dump(dir, basename, dist, *h->flat, err);
    if (rc != OK) return fail(rc, err);
    *out = h.release();
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_FORMAT)
}

int hnswgpu_file_dump(const hnswgpu_index* cidx, const char* dir, const char* basename) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !dir || !basename) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    const FlatIndex* f = idx->get_flat();
    if (!f) return fail(HNSWGPU_ERR_EMPTY, "entry point not initialized");
    std::string err;
    return finish(write_dump(*f, dir, basename, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_IO)
}

void hnswgpu_free_index(hnswgpu_index* idx) { delete idx; }

static void fill_descr(hnswgpu_description* o, uint32_t ver, uint8_t mode, uint8_t m, uint8_t nbl, double ls, uint64_t ef,
                       uint64_t nbp, uint64_t dim, const std::string& dn, const std::string& tn) {
    std::memset(o, 0, sizeof(*o));
    o->format_version = ver;
    o->dumpmode = mode;
    o->max_nb_connection = m;
    o->nb_layer = nbl;
    o->level_scale = ls;
    o->ef_construction = ef;
    o->nb_point = nbp;
    o->dimension = dim;
    std::strncpy(o->distname, dn.c_str(), sizeof(o->distname) - 1);
    std::strncpy(o->t_name, tn.c_str(), sizeof(o->t_name) - 1);
}

int hnswgpu_load_description(const char* graph_file_path, hnswgpu_description* out) {
    CAPI_GUARD_BEGIN
    if (!graph_file_path || !out) return fail(HNSWGPU_ERR_ARG, "null argument");
    DumpDescription d;
    std::string err;
    int rc = load_description_file(graph_file_path, d, err);
    if (rc != OK) return fail(rc, err);
    fill_descr(out, d.format_version, d.dumpmode, d.max_nb_connection, d.nb_layer, d.level_scale, d.ef, d.nb_point,
               d.dimension, d.distname, d.t_name);
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_FORMAT)
}

int hnswgpu_get_description(const hnswgpu_index* cidx, hnswgpu_description* out) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !out) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    const FlatIndex* f = idx->get_flat();
    if (!f) return fail(HNSWGPU_ERR_EMPTY, "index is empty");
    fill_descr(out, f->format_version, f->dumpmode, (uint8_t)f->max_nb_connection, f->nb_layer, f->level_scale,
               f->ef_construction, f->n, f->dimension, f->distname.empty() ? dist_type_name(f->dist) : f->distname, f->t_name);
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_FORMAT)
}

static BuildParams to_params(const hnswgpu_build_params* p) {
    BuildParams b;
    b.max_nb_connection = p->max_nb_connection;
    b.ef_construction = p->ef_construction;
    b.max_layer = p->max_layer ? p->max_layer : 16;
    b.dist = p->dist;
    b.level_scale_factor = p->level_scale_factor > 0 ? p->level_scale_factor : 1.0;
    b.extend_candidates = p->extend_candidates != 0;
    b.keep_pruned = p->keep_pruned != 0;
    b.nthreads = p->nthreads;
    b.fast_arithmetic = p->fast_arithmetic != 0;
    b.gpu_device = p->gpu_assist ? p->gpu_device : -1;
    b.gpu_window = p->gpu_window;
    return b;
}

int hnswgpu_build(const float* data, uint64_t n, uint64_t d, const uint64_t* ids, const hnswgpu_build_params* params,
                  hnswgpu_index** out) {
    CAPI_GUARD_BEGIN
    if (!params || !out || (n && !data)) return fail(HNSWGPU_ERR_ARG, "null argument");
    *out = nullptr;
    if (params->dist < 0 || params->dist >= DIST_COUNT) return fail(HNSWGPU_ERR_DISTANCE, "unknown distance");
    if (params->max_nb_connection < 2 || params->max_nb_connection > 256)
        return fail(HNSWGPU_ERR_ARG, "error max_nb_connection must be less equal than 256");  // src/hnsw.rs:784-787
    std::unique_ptr<hnswgpu_index> h(new hnswgpu_index());
    h->params = to_params(params);
    h->builder.reset(new GraphBuilder(h->params));
    std::string err;
    int rc;
    if (h->params.gpu_device >= 0) {
        std::unique_ptr<BuildSearchBackend> dev = make_device_build_backend(h->params.gpu_device);
        rc = h->builder->insert_batch_gpu(data, n, d, ids, h->params.nthreads, *dev, h->params.gpu_window, err);
        if (rc == OK && !h->builder->last_warning().empty()) note(h->builder->last_warning());
    } else {
        rc = h->builder->insert_batch(data, n, d, ids, h->params.nthreads, err);
    }
    if (rc != OK) return fail(rc, err);
    h->flat_stale = true;
    *out = h.release();
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

static std::string unrepresentable_message(uint64_t bad, uint64_t data_id, uint64_t dim) {
    return "HNSWGPU_STORAGE_F16: " + std::to_string(bad) + " vector elements are not representable as binary16 (NaN, or (f32)(f16)x != x); "
           "the first is dimension " + std::to_string(dim) + " of the point with DataId " + std::to_string(data_id);
}
// Hnsw::insert / parallel_insert on ANY handle, reloaded ones included (HnswIo::load_hnsw returns a fully insertable
// Hnsw).  Exclusive lock held by the caller.
static int insert_points(hnswgpu_index* idx, const float* data, uint64_t n, uint64_t d, const uint64_t* ids, int nthreads,
                         int gpu_device = -1, uint64_t gpu_window = 0) {
    if (!idx->builder) {
        if (!idx->flat) return fail(HNSWGPU_ERR_EMPTY, "handle holds no index");
        idx->builder.reset(new GraphBuilder(*idx->flat, false));  // continue the reloaded graph (builder.hpp)
        idx->params = idx->builder->params();
    }
    // an F16 index: the NEW vectors first -- one element that a half cannot hold refuses the whole call.  (Rows of another dimension
    // than the index's are the builder's to refuse, below: an element index counted with the caller's d would name the wrong one.)
    const uint64_t dim = idx->builder->dimension();
    if (idx->storage == HNSWGPU_STORAGE_F16 && d != 0 && (dim == 0 || d == dim)) {
        uint64_t first = 0;
        const uint64_t bad = f16_count_unrepresentable(data, n * d, &first);
        if (bad != 0)
            return fail(HNSWGPU_ERR_ARG, unrepresentable_message(bad, ids ? ids[first / d] : index_nb_point(idx) + first / d, first % d) +
                                         "; nothing was inserted");
    }
    std::string err;
    int rc;
    if (gpu_device >= 0) {
        std::unique_ptr<BuildSearchBackend> dev = make_device_build_backend(gpu_device);
        rc = idx->builder->insert_batch_gpu(data, n, d, ids, nthreads, *dev, gpu_window, err);
        if (rc == OK && !idx->builder->last_warning().empty()) note(idx->builder->last_warning());
    } else {
        rc = idx->builder->insert_batch(data, n, d, ids, nthreads, err);
    }
    if (rc != OK) return fail(rc, err);
    idx->flat_stale = true;
    idx->dev_stale = true;
    return HNSWGPU_OK;
}

int hnswgpu_insert(hnswgpu_index* idx, const float* data, uint64_t n, uint64_t d, const uint64_t* ids, int nthreads) {
    CAPI_GUARD_BEGIN
    if (!idx || (n && !data)) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    return insert_points(idx, data, n, d, ids, nthreads);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_insert_gpu(hnswgpu_index* idx, const float* data, uint64_t n, uint64_t d, const uint64_t* ids, int nthreads,
                       int gpu_device, uint64_t gpu_window) {
    CAPI_GUARD_BEGIN
    if (!idx || (n && !data)) return fail(HNSWGPU_ERR_ARG, "null argument");
    if (gpu_device < 0) return fail(HNSWGPU_ERR_ARG, "gpu_device must name a HIP device");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    return insert_points(idx, data, n, d, ids, nthreads, gpu_device, gpu_window);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

uint64_t hnswgpu_nb_point(const hnswgpu_index* cidx) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return 0;
    std::shared_lock<std::shared_mutex> g(idx->mu);
    return index_nb_point(idx);
    CAPI_GUARD_END(0)
}
uint64_t hnswgpu_dimension(const hnswgpu_index* cidx) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return 0;
    std::shared_lock<std::shared_mutex> g(idx->mu);
    return index_dimension(idx);
    CAPI_GUARD_END(0)
}
int hnswgpu_dist(const hnswgpu_index* cidx) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return -1;
    std::shared_lock<std::shared_mutex> g(idx->mu);
    if (idx->builder) return idx->params.dist;
    return idx->flat ? idx->flat->dist : -1;
}
uint64_t hnswgpu_layer_nb_point(const hnswgpu_index* cidx, unsigned layer) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || layer >= NB_LAYER_MAX) return 0;
    std::unique_lock<std::shared_mutex> g(idx->mu);
    const FlatIndex* f = idx->get_flat();
    return f ? f->layer_count(layer) : 0;
    CAPI_GUARD_END(0)
}
int hnswgpu_max_level_observed(const hnswgpu_index* cidx) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return 0;
    std::unique_lock<std::shared_mutex> g(idx->mu);
    const FlatIndex* f = idx->get_flat();
    if (!f || f->entry_flat == NO_POINT) return 0;
    return (int)f->layer_of(f->entry_flat);
    CAPI_GUARD_END(0)
}
int hnswgpu_entry_point(const hnswgpu_index* cidx, uint64_t* origin_id, uint8_t* layer, int32_t* rank) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    const FlatIndex* f = idx->get_flat();
    if (!f || f->entry_flat == NO_POINT) return fail(HNSWGPU_ERR_EMPTY, "index is empty");
    if (origin_id) *origin_id = f->origin_id[f->entry_flat];
    if (layer) *layer = (uint8_t)f->layer_of(f->entry_flat);
    if (rank) *rank = f->rank_of(f->entry_flat);
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}
int64_t hnswgpu_neighbours(const hnswgpu_index* cidx, unsigned layer, int32_t rank, unsigned l, uint64_t cap,
                           uint64_t* origin_ids, uint8_t* layers, int32_t* ranks, float* dists) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || layer >= NB_LAYER_MAX || l >= NB_LAYER_MAX || rank < 0) { fail(HNSWGPU_ERR_ARG, "bad argument"); return -1; }
    std::unique_lock<std::shared_mutex> g(idx->mu);
    const FlatIndex* f = idx->get_flat();
    if (!f || (uint64_t)rank >= f->layer_count(layer)) { fail(HNSWGPU_ERR_ARG, "no such point"); return -1; }
    uint64_t flat = f->layer_offset[layer] + (uint64_t)rank;
    uint64_t b = f->nbr_ptr[flat * NB_LAYER_MAX + l], e = f->nbr_ptr[flat * NB_LAYER_MAX + l + 1];
    for (uint64_t j = b; j < e && j - b < cap; ++j) {
        uint32_t nf = f->nbr_flat[j];
        if (origin_ids) origin_ids[j - b] = f->origin_id[nf];
        if (layers) layers[j - b] = (uint8_t)f->layer_of(nf);
        if (ranks) ranks[j - b] = f->rank_of(nf);
        if (dists) dists[j - b] = f->nbr_dist[j];
    }
    return (int64_t)(e - b);
    CAPI_GUARD_END(-1)
}

int hnswgpu_device_count(void) { return device_count(); }

int hnswgpu_upload(hnswgpu_index* idx, int device) {
    CAPI_GUARD_BEGIN
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    int rc = ensure_device(idx, device);
    if (rc == HNSWGPU_OK && device >= 0) idx->primary = device;  // the last explicit upload names the primary device
    return rc;
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// shared implementation of the host-buffer searches on the primary replica
static int search_host_common(const hnswgpu_index* cidx, const float* queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef,
                              const uint64_t* allowed, uint64_t n_allowed, bool filtered, uint64_t* out_ids, float* out_dists,
                              uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts, uint8_t* out_status, uint32_t* panics) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    if (index_empty(idx)) {  // empty index => every answer is empty (src/hnsw.rs:1498-1503)
        if (out_counts) std::memset(out_counts, 0, nq * sizeof(uint32_t));
        if (out_status) std::memset(out_status, 0, nq);
        if (panics) *panics = 0;
        return HNSWGPU_OK;
    }
    DeviceIndex* dev = nullptr;
    int rc = primary_replica(idx, sl, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    CallInfo info;
    rc = dev->search_host(queries, nq, d, k, ef, out_ids, out_dists, out_layer, out_rank, out_counts, allowed, n_allowed, filtered,
                          out_status, &info, err);
    if (rc != OK) return fail(rc, err);
    if (panics) *panics = info.panics;
    return HNSWGPU_OK;
}

int hnswgpu_search_batch(const hnswgpu_index* cidx, const float* queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef,
                         uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts) {
    CAPI_GUARD_BEGIN
    return search_host_common(cidx, queries, nq, d, k, ef, nullptr, 0, false, out_ids, out_dists, out_layer, out_rank, out_counts,
                              nullptr, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_search_batch_filtered(const hnswgpu_index* cidx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                  uint64_t ef, const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids,
                                  float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts,
                                  uint8_t* out_status) {
    CAPI_GUARD_BEGIN
    if (n_allowed && !allowed_ids) return fail(HNSWGPU_ERR_ARG, "null filter");
    int rc = check_sorted_filter(allowed_ids, n_allowed);
    if (rc != HNSWGPU_OK) return rc;
    uint32_t panics = 0;
    rc = search_host_common(cidx, queries, nq, d, k, ef, allowed_ids, n_allowed, true, out_ids, out_dists, out_layer, out_rank,
                                out_counts, out_status, &panics);
    if (rc != HNSWGPU_OK) return rc;
    if (panics != 0 && !out_status)
        return fail(HNSWGPU_ERR_REF_PANIC, "the reference panics on " + std::to_string(panics) +
                    " of these queries (return_points.peek().unwrap() on a heap the filter emptied, src/hnsw.rs:973); "
                    "pass out_status to learn which");
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

// Replicas on every device of devices[0..n): the missing ones are uploaded AT THE SAME TIME, one host thread per device
// (an upload is a host-side re-layout plus ~0.65 GB over PCIe for BASELINE config 2: eight of them one after the other
// was the first-call cost of an 8-GPU host).  Exclusive lock held.
static int ensure_devices(hnswgpu_index* idx, const int* devices, int n) {
    const FlatIndex* f = idx->get_flat();
    if (!f || f->n == 0) return fail(HNSWGPU_ERR_EMPTY, "index is empty");
    if (idx->dev_stale) {  // the graph changed: every replica is out of date
        idx->replicas.clear();
        idx->dev_stale = false;
    }
    std::vector<int> missing;
    for (int s = 0; s < n; ++s)
        if (!idx->replica(devices[s]) && std::find(missing.begin(), missing.end(), devices[s]) == missing.end()) missing.push_back(devices[s]);
    if (!missing.empty()) {
        std::vector<std::unique_ptr<DeviceIndex>> fresh(missing.size());
        std::vector<int> rcs(missing.size(), OK);
        std::vector<std::string> errs(missing.size());
        auto upload_one = [&](size_t i) {
            try {
                fresh[i].reset(new DeviceIndex());
                fresh[i]->set_storage(idx->storage);
                rcs[i] = fresh[i]->upload(*f, missing[i], errs[i]);
            } catch (const std::exception& e) {
                rcs[i] = ERR_DEVICE;
                errs[i] = e.what();
            }
        };
        {
            JoinAll th;
            for (size_t i = 1; i < missing.size(); ++i) th.spawn([&, i]() { upload_one(i); });
            upload_one(0);
        }
        for (size_t i = 0; i < missing.size(); ++i)
            if (rcs[i] != OK) return fail(rcs[i], "device " + std::to_string(missing[i]) + ": " + errs[i]);
        for (size_t i = 0; i < missing.size(); ++i) {
            if (idx->strict_ties >= 0) fresh[i]->set_strict_ties(idx->strict_ties != 0);
            fresh[i]->set_arithmetic(idx->arithmetic);
            idx->replicas[missing[i]] = std::move(fresh[i]);
        }
    }
    if (n > 0 && (idx->primary < 0 || !idx->replica(idx->primary))) idx->primary = devices[0];
    return HNSWGPU_OK;
}

// shared front of the sharded entry points: argument checks, replicas, then the shared lock for the searches.
// Returns HNSWGPU_OK with *empty = true when the index holds no point (the answer is "no neighbours").
static int sharded_prepare(hnswgpu_index* idx, const int* devices, int n_shards, std::shared_lock<std::shared_mutex>& sl,
                           std::vector<DeviceIndex*>& reps, bool* empty) {
    *empty = false;
    {   // replicas on every device named (exclusive: uploads change the handle)
        std::unique_lock<std::shared_mutex> xl(idx->mu);
        if (index_empty(idx)) { *empty = true; return HNSWGPU_OK; }
        int rc = ensure_devices(idx, devices, n_shards);
        if (rc != HNSWGPU_OK) return rc;
    }
    sl = std::shared_lock<std::shared_mutex>(idx->mu);
    if (!idx->fresh() || idx->dev_stale) return fail(HNSWGPU_ERR_DEVICE, "index changed while a search was starting");
    reps.assign((size_t)n_shards, nullptr);
    for (int s = 0; s < n_shards; ++s) {  // every replica resolved BEFORE the first thread exists
        reps[(size_t)s] = idx->replica(devices[s]);
        if (!reps[(size_t)s]) return fail(HNSWGPU_ERR_DEVICE, "replica missing");
    }
    return HNSWGPU_OK;
}

// Hnsw::parallel_search with the batch sharded over several GPUs of this process: graph replicated (one replica per
// distinct device, uploaded on first use, all at once), contiguous balanced blocks of queries, one host thread per shard,
// every shard copies its answers straight into the caller's arrays -- the gather.  No collective: the shards are independent.
int hnswgpu_search_batch_sharded(const hnswgpu_index* cidx, const int* devices, int n_shards, const float* queries, uint64_t nq,
                                 uint64_t d, uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dists, uint8_t* out_layer,
                                 int32_t* out_rank, uint32_t* out_counts) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !devices || n_shards <= 0) return fail(HNSWGPU_ERR_ARG, "bad argument");
    if (nq && (!queries || !out_ids || !out_dists || !out_counts)) return fail(HNSWGPU_ERR_ARG, "null buffer");
    std::shared_lock<std::shared_mutex> sl;
    std::vector<DeviceIndex*> reps;
    bool empty = false;
    int prc = sharded_prepare(idx, devices, n_shards, sl, reps, &empty);
    if (prc != HNSWGPU_OK) return prc;
    if (empty) {
        if (out_counts) std::memset(out_counts, 0, nq * sizeof(uint32_t));
        return HNSWGPU_OK;
    }
    std::vector<int> rcs((size_t)n_shards, OK);
    std::vector<std::string> errs((size_t)n_shards);
    {
        JoinAll th;  // joins whatever was spawned, also when a spawn throws
        const uint64_t base = nq / (uint64_t)n_shards, rem = nq % (uint64_t)n_shards;  // shard s: base + (s < rem) queries
        uint64_t start = 0;
        for (int s = 0; s < n_shards; ++s) {
            const uint64_t cnt = base + ((uint64_t)s < rem ? 1 : 0);
            DeviceIndex* dev = reps[(size_t)s];
            const uint64_t s0 = start;
            start += cnt;
            if (cnt == 0) continue;
            th.spawn([=, &rcs, &errs]() {
                try {
                    rcs[(size_t)s] = dev->search_host(queries + s0 * d, cnt, d, k, ef, out_ids + s0 * k, out_dists + s0 * k,
                                                      out_layer ? out_layer + s0 * k : nullptr, out_rank ? out_rank + s0 * k : nullptr,
                                                      out_counts + s0, nullptr, 0, false, nullptr, nullptr, errs[(size_t)s]);
                } catch (const std::exception& e) {
                    rcs[(size_t)s] = ERR_DEVICE;
                    errs[(size_t)s] = e.what();
                }
            });
        }
    }
    for (int s = 0; s < n_shards; ++s)
        if (rcs[(size_t)s] != OK) return fail(rcs[(size_t)s], "shard " + std::to_string(s) + ": " + errs[(size_t)s]);
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_search_batch_sharded_device(const hnswgpu_index* cidx, const int* devices, int n_shards, const float* const* d_queries,
                                        const uint64_t* nq_shard, uint64_t d, uint64_t k, uint64_t ef, uint64_t* const* d_out_ids,
                                        float* const* d_out_dists, uint8_t* const* d_out_layer, int32_t* const* d_out_rank,
                                        uint32_t* const* d_out_counts, void* const* streams) {
    CAPI_GUARD_BEGIN
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !devices || n_shards <= 0 || !nq_shard || !d_queries || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(HNSWGPU_ERR_ARG, "bad argument");
    for (int s = 0; s < n_shards; ++s)
        if (nq_shard[s] && (!d_queries[s] || !d_out_ids[s] || !d_out_dists[s] || !d_out_counts[s])) return fail(HNSWGPU_ERR_ARG, "null buffer");
    std::shared_lock<std::shared_mutex> sl;
    std::vector<DeviceIndex*> reps;
    bool empty = false;
    int prc = sharded_prepare(idx, devices, n_shards, sl, reps, &empty);
    if (prc != HNSWGPU_OK) return prc;
    if (empty) return fail(HNSWGPU_ERR_EMPTY, "index is empty");  // (device-resident counters cannot be zeroed from here without a device)
    std::vector<int> rcs((size_t)n_shards, OK);
    std::vector<std::string> errs((size_t)n_shards);
    {
        JoinAll th;
        for (int s = 0; s < n_shards; ++s) {
            if (nq_shard[s] == 0) continue;
            DeviceIndex* dev = reps[(size_t)s];
            th.spawn([=, &rcs, &errs]() {
                try {
                    rcs[(size_t)s] = dev->search_device(d_queries[s], nq_shard[s], d, k, ef, d_out_ids[s], d_out_dists[s],
                                                        d_out_layer ? d_out_layer[s] : nullptr, d_out_rank ? d_out_rank[s] : nullptr,
                                                        d_out_counts[s], nullptr, streams ? streams[s] : nullptr, nullptr, 0, nullptr,
                                                        errs[(size_t)s]);
                } catch (const std::exception& e) {
                    rcs[(size_t)s] = ERR_DEVICE;
                    errs[(size_t)s] = e.what();
                }
            });
        }
    }
    for (int s = 0; s < n_shards; ++s)
        if (rcs[(size_t)s] != OK) return fail(rcs[(size_t)s], "shard " + std::to_string(s) + ": " + errs[(size_t)s]);
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_lane_lab(int device, uint32_t mode, uint32_t p0, uint32_t p1, uint32_t p2, const uint32_t* ops, uint32_t n_ops,
                     const uint32_t* lanes, uint32_t n_lane_sets, uint32_t* out, uint32_t out_words) {
    CAPI_GUARD_BEGIN
    if ((n_ops && !ops) || (n_lane_sets && !lanes) || !out) return fail(HNSWGPU_ERR_ARG, "null buffer");
    std::string err;
    return finish(lane_lab_device(device, mode, p0, p1, p2, ops, n_ops, lanes, n_lane_sets, out, out_words, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_gather_sharded_answers(const int* devices, int n_shards, const uint64_t* nq_shard, uint64_t k,
                                   const uint64_t* const* d_ids, const float* const* d_dists, const uint8_t* const* d_layer,
                                   const int32_t* const* d_rank, const uint32_t* const* d_counts, int root_device,
                                   uint64_t* root_ids, float* root_dists, uint8_t* root_layer, int32_t* root_rank,
                                   uint32_t* root_counts, void* root_stream) {
    CAPI_GUARD_BEGIN
    if (!devices || n_shards <= 0 || !nq_shard || !d_ids || !d_dists || !d_counts || k == 0) return fail(HNSWGPU_ERR_ARG, "bad argument");
    uint64_t total = 0;
    for (int s = 0; s < n_shards; ++s) {
        if (nq_shard[s] && (!d_ids[s] || !d_dists[s] || !d_counts[s])) return fail(HNSWGPU_ERR_ARG, "null buffer");
        total += nq_shard[s];
    }
    if (total && (!root_ids || !root_dists || !root_counts)) return fail(HNSWGPU_ERR_ARG, "null buffer");
    std::string err;
    return finish(hnswgpu::gather_sharded_answers(devices, n_shards, nq_shard, k, d_ids, d_dists, d_layer, d_rank, d_counts, root_device,
                                             root_ids, root_dists, root_layer, root_rank, root_counts, root_stream, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

static int search_device_common(const hnswgpu_index* cidx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef,
                                const uint64_t* d_allowed, uint64_t n_allowed, uint64_t* d_out_ids, float* d_out_dists,
                                uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, uint32_t* d_stats, void* stream,
                                uint32_t* panics) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    DeviceIndex* dev = nullptr;
    int rc = resident_replica(idx, false, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    CallInfo info;
    rc = dev->search_device(d_queries, nq, d, k, ef, d_out_ids, d_out_dists, d_out_layer, d_out_rank, d_out_counts, d_stats,
                                stream, d_allowed, n_allowed, &info, err);
    if (rc != OK) return fail(rc, err);
    if (panics) *panics = info.panics;
    return HNSWGPU_OK;
}

int hnswgpu_search_batch_device(const hnswgpu_index* cidx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                uint64_t ef, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer,
                                int32_t* d_out_rank, uint32_t* d_out_counts, uint32_t* d_stats, void* stream) {
    CAPI_GUARD_BEGIN
    return search_device_common(cidx, d_queries, nq, d, k, ef, nullptr, 0, d_out_ids, d_out_dists, d_out_layer, d_out_rank,
                                d_out_counts, d_stats, stream, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// begin / end: the blocking call as an asynchronous job of the library's worker pool (a long-lived thread: creating one per
// ticket cost tens of microseconds on a ~1 ms call), so the launch path is the one every other entry point uses; searches on
// one handle may run concurrently, each with a private workspace
struct hnswgpu_ticket {
    std::shared_ptr<WorkerPool::Job> job;
    int status = HNSWGPU_OK;
    std::string error;
};
int hnswgpu_search_batch_device_begin(const hnswgpu_index* cidx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                      uint64_t ef, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer,
                                      int32_t* d_out_rank, uint32_t* d_out_counts, uint32_t* d_stats, void* stream,
                                      hnswgpu_ticket** ticket) {
    CAPI_GUARD_BEGIN
    if (!ticket) return fail(HNSWGPU_ERR_ARG, "null ticket");
    *ticket = nullptr;
    if (!cidx) return fail(HNSWGPU_ERR_ARG, "null index");
    std::unique_ptr<hnswgpu_ticket> t(new hnswgpu_ticket());
    hnswgpu_ticket* raw = t.get();
    raw->job = WorkerPool::instance().submit([=]() {
        raw->status = hnswgpu_search_batch_device(cidx, d_queries, nq, d, k, ef, d_out_ids, d_out_dists, d_out_layer, d_out_rank,
                                                  d_out_counts, d_stats, stream);
        if (raw->status != HNSWGPU_OK) raw->error = hnswgpu_last_error();  // this thread's message, handed to the ticket
    });
    *ticket = t.release();
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}
int hnswgpu_search_batch_end(hnswgpu_ticket* ticket) {
    CAPI_GUARD_BEGIN
    if (!ticket) return fail(HNSWGPU_ERR_ARG, "null ticket");
    std::unique_ptr<hnswgpu_ticket> t(ticket);
    if (t->job) t->job->wait();
    if (t->status != HNSWGPU_OK) return fail(t->status, t->error);
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_search_batch_filtered_device(const hnswgpu_index* cidx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                         uint64_t ef, const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids,
                                         float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                                         uint32_t* d_stats, void* stream, uint32_t* n_panics) {
    CAPI_GUARD_BEGIN
    if (!d_allowed_ids && n_allowed) return fail(HNSWGPU_ERR_ARG, "null filter");
    uint32_t panics = 0;
    // an empty filter still is a filter (every point is refused); a null pointer would read as "no filter" below, so
    // hand over a non-null pointer that is never dereferenced (n_allowed == 0)
    const uint64_t* ids = d_allowed_ids ? d_allowed_ids : reinterpret_cast<const uint64_t*>(d_queries);
    int rc = search_device_common(cidx, d_queries, nq, d, k, ef, ids, n_allowed, d_out_ids, d_out_dists, d_out_layer, d_out_rank,
                                  d_out_counts, d_stats, stream, &panics);
    if (n_panics) *n_panics = panics;
    return rc;
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- The host / _device pairs.  A pair is ONE body, a static function that holds the pair's whole sequence -- checks, trivial
// answers, "is there a device side", replica, call, finish -- and takes (host, stream) last: (true, nullptr) from the host-buffer
// entry, (false, the caller's stream) from the _device entry.  Where the two forms part, the body says `if (host)`.  The two C entries
// above it open the guard, build the arguments' struct and close the guard with their own code: an exception that gets there is
// HNSWGPU_ERR_ARG in the host form, HNSWGPU_ERR_DEVICE in the device form.
static const char* const kNoFilterSetDevice = "no HIP device visible (a gfx950 GPU is required; there is no CPU fallback)";

// the replica a pair's call works on; the handle's lock is held (shared).  Host form: the primary one, uploaded on first use (f32: for
// a call that reads rows outside the search path).  Device form: the one that is there; need_flat: the call reads the host view too.
static int call_replica(hnswgpu_index* idx, std::shared_lock<std::shared_mutex>& sl, bool host, bool f32, bool need_flat, DeviceIndex** dev) {
    if (!host) return resident_replica(idx, need_flat, dev);
    return f32 ? primary_f32_replica(idx, sl, dev) : primary_replica(idx, sl, dev);
}

// ---- filter set: every query of the batch under a filter of its own choice (search_device.hpp: FilterSet)
// what both forms of a filter-set pair can check of the set without reading it (unfiltered: the sibling the message points to)
static int check_filter_set_shape(const void* queries, uint64_t nq, const void* filter_offsets, uint64_t n_filters, const void* filter_of,
                                  const void* out_ids, const void* out_dists, const void* out_counts, const char* unfiltered) {
    if (nq != 0 && (!queries || !out_ids || !out_dists || !out_counts)) return fail(HNSWGPU_ERR_ARG, "null buffer");
    if (nq != 0 && !filter_of) return fail(HNSWGPU_ERR_ARG, "null filter_of: every query names its filter");
    if (n_filters != 0 && !filter_offsets) return fail(HNSWGPU_ERR_ARG, "null filter_offsets");
    if (n_filters == 0 && nq != 0)
        return fail(HNSWGPU_ERR_ARG, std::string("a filter set without filters: n_filters is 0 (an unfiltered batch is ") + unfiltered + ")");
    if (n_filters > 0xFFFFFFFFull) return fail(HNSWGPU_ERR_ARG, "too many filters: filter_of is 32 bits wide");
    return HNSWGPU_OK;
}
// ... and what only a host form can, behind the shape: the set itself
static int check_filter_set_contents(const uint64_t* filter_ids, const uint64_t* filter_offsets, uint64_t n_filters, const uint32_t* filter_of,
                                     uint64_t nq) {
    if (n_filters != 0) {
        if (filter_offsets[0] != 0) return fail(HNSWGPU_ERR_ARG, "filter_offsets must start at 0");
        for (uint64_t f = 0; f < n_filters; ++f)
            if (filter_offsets[f] > filter_offsets[f + 1])
                return fail(HNSWGPU_ERR_ARG, "filter_offsets must ascend: filter_offsets[" + std::to_string(f + 1) + "] is below its predecessor");
        if (filter_offsets[n_filters] != 0 && !filter_ids) return fail(HNSWGPU_ERR_ARG, "null filter_ids");
        for (uint64_t f = 0; f < n_filters; ++f)  // `impl FilterT for Vec<usize>` is a binary search: every vector must be sorted
            for (uint64_t i = filter_offsets[f] + 1; i < filter_offsets[f + 1]; ++i)
                if (filter_ids[i - 1] > filter_ids[i])
                    return fail(HNSWGPU_ERR_ARG, "the id vector of filter " + std::to_string(f) + " is not sorted ascending");
    }
    for (uint64_t q = 0; q < nq; ++q)
        if (filter_of[q] >= n_filters)
            return fail(HNSWGPU_ERR_ARG, "filter_of[" + std::to_string(q) + "] = " + std::to_string(filter_of[q]) + " names no filter (n_filters = " +
                        std::to_string(n_filters) + ")");
    return HNSWGPU_OK;
}
// the set as a device form hands it on: filters that are all empty need no id array, so a null one becomes a non-null pointer that is
// never dereferenced
static FilterSet device_filter_set(const ExactSetArgs& a) {
    return FilterSet{a.set.ids ? a.set.ids : reinterpret_cast<const uint64_t*>(a.queries), a.set.offsets, a.set.n_filters, a.set.filter_of};
}

// The search's pair (a: the exact pair's struct serves, k its knbn).  The two forms answer in different places -- out_status on the
// host, d_stats and *n_panics with device buffers -- and the device form reads the handle later than the host form.
static int search_filter_set_pair(const hnswgpu_index* cidx, const ExactSetArgs& a, uint64_t ef, uint8_t* out_status, uint32_t* d_stats,
                                  uint32_t* n_panics, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!host && n_panics) *n_panics = 0;  // (ahead of the null-handle check)
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    int rc = check_filter_set_shape(a.queries, a.nq, a.set.offsets, a.set.n_filters, a.set.filter_of, a.out_ids, a.out_dists, a.out_counts,
                                    host ? "hnswgpu_search_batch" : "hnswgpu_search_batch_device");
    if (rc != HNSWGPU_OK) return rc;
    std::shared_lock<std::shared_mutex> sl(idx->mu, std::defer_lock);
    if (host) {
        rc = check_filter_set_contents(a.set.ids, a.set.offsets, a.set.n_filters, a.set.filter_of, a.nq);
        if (rc != HNSWGPU_OK) return rc;
        sl.lock();
        if (index_empty(idx)) {  // empty index => every answer is empty (src/hnsw.rs:1498-1503)
            if (a.out_counts) std::memset(a.out_counts, 0, a.nq * sizeof(uint32_t));
            if (out_status) std::memset(out_status, 0, a.nq);
            return HNSWGPU_OK;
        }
    }
    if (a.nq == 0) return HNSWGPU_OK;
    if (host ? !hnswgpu::search_filter_set_host : !hnswgpu::search_filter_set_device) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    if (!host) sl.lock();
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, false, false, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    CallInfo info;
    rc = host ? hnswgpu::search_filter_set_host(*dev, a.queries, a.nq, a.d, a.k, ef, a.set, a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts,
                                                out_status, &info, err)
              : hnswgpu::search_filter_set_device(*dev, a.queries, a.nq, a.d, a.k, ef, device_filter_set(a), a.out_ids, a.out_dists, a.out_layer, a.out_rank,
                                                  a.out_counts, d_stats, stream, &info, err);
    if (rc != OK) return fail(rc, err);
    if (!host) {
        if (n_panics) *n_panics = info.panics;
        return HNSWGPU_OK;
    }
    if (info.panics != 0 && !out_status)
        return fail(HNSWGPU_ERR_REF_PANIC, "the reference panics on " + std::to_string(info.panics) +
                    " of these queries (return_points.peek().unwrap() on a heap the filter emptied, src/hnsw.rs:973); "
                    "pass out_status to learn which");
    return HNSWGPU_OK;
}

int hnswgpu_search_batch_filter_set(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef,
                                    const uint64_t* filter_ids, const uint64_t* filter_offsets, uint64_t n_filters,
                                    const uint32_t* filter_of, uint64_t* out_ids, float* out_dists, uint8_t* out_layer,
                                    int32_t* out_rank, uint32_t* out_counts, uint8_t* out_status) {
    CAPI_GUARD_BEGIN
    const ExactSetArgs a{queries, nq, d, k, FilterSet{filter_ids, filter_offsets, n_filters, filter_of}, out_ids, out_dists, out_layer, out_rank, out_counts};
    return search_filter_set_pair(idx, a, ef, out_status, nullptr, nullptr, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_search_batch_filter_set_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                           uint64_t ef, const uint64_t* d_filter_ids, const uint64_t* d_filter_offsets,
                                           uint64_t n_filters, const uint32_t* d_filter_of, uint64_t* d_out_ids, float* d_out_dists,
                                           uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, uint32_t* d_stats,
                                           void* stream, uint32_t* n_panics) {
    CAPI_GUARD_BEGIN
    const ExactSetArgs a{d_queries, nq, d, k, FilterSet{d_filter_ids, d_filter_offsets, n_filters, d_filter_of}, d_out_ids, d_out_dists, d_out_layer,
                         d_out_rank, d_out_counts};
    return search_filter_set_pair(idx, a, ef, nullptr, d_stats, n_panics, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- exact k-NN under a filter set: the ground truth of hnswgpu_search_batch_filter_set (exact_knn.hip holds the device side)
static int exact_filter_set_pair(const hnswgpu_index* cidx, const ExactSetArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    int rc = check_filter_set_shape(a.queries, a.nq, a.set.offsets, a.set.n_filters, a.set.filter_of, a.out_ids, a.out_dists, a.out_counts,
                                    host ? "hnswgpu_exact_search_batch" : "hnswgpu_exact_search_batch_device");
    if (rc != HNSWGPU_OK) return rc;
    if (host) {
        rc = check_filter_set_contents(a.set.ids, a.set.offsets, a.set.n_filters, a.set.filter_of, a.nq);
        if (rc != HNSWGPU_OK) return rc;
    }
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    rc = check_exact_call(idx, a.queries, a.nq, a.d, a.k, nullptr, 0, a.out_ids, a.out_dists, a.out_counts);
    if (rc != HNSWGPU_OK) return rc;
    if (host && index_empty(idx)) {  // no point: every answer is empty
        zero_knn_answers(a.nq, a.k, a.out_ids, a.out_dists, a.out_layer, a.out_rank, a.out_counts);
        return HNSWGPU_OK;
    }
    if (a.nq == 0) return HNSWGPU_OK;
    if (!hnswgpu::exact_filter_set) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    ExactSetArgs b = a;
    if (!host) b.set = device_filter_set(a);
    std::string err;
    return finish(hnswgpu::exact_filter_set(*dev, idx->flat->origin_id, b, host, stream, err), err);
}

int hnswgpu_exact_search_batch_filter_set(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                          const uint64_t* filter_ids, const uint64_t* filter_offsets, uint64_t n_filters,
                                          const uint32_t* filter_of, uint64_t* out_ids, float* out_dists, uint8_t* out_layer,
                                          int32_t* out_rank, uint32_t* out_counts) {
    CAPI_GUARD_BEGIN
    const ExactSetArgs a{queries, nq, d, k, FilterSet{filter_ids, filter_offsets, n_filters, filter_of}, out_ids, out_dists, out_layer, out_rank, out_counts};
    return exact_filter_set_pair(idx, a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_exact_search_batch_filter_set_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                                 const uint64_t* d_filter_ids, const uint64_t* d_filter_offsets, uint64_t n_filters,
                                                 const uint32_t* d_filter_of, uint64_t* d_out_ids, float* d_out_dists,
                                                 uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, void* stream) {
    CAPI_GUARD_BEGIN
    const ExactSetArgs a{d_queries, nq, d, k, FilterSet{d_filter_ids, d_filter_offsets, n_filters, d_filter_of}, d_out_ids, d_out_dists, d_out_layer,
                         d_out_rank, d_out_counts};
    return exact_filter_set_pair(idx, a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- exact range search: every eligible point within a query's radius (exact_range.hip holds the device side)
// the checks both forms share; the handle's lock is held (shared)
static int exact_range_call(const hnswgpu_index* idx, const ExactRangeCallArgs& a) {
    const uint64_t dim = index_dimension(idx);
    if (!a.out_offsets) return fail(HNSWGPU_ERR_ARG, "null out_offsets: the offsets are written by every call");
    if (a.nq != 0 && !a.queries) return fail(HNSWGPU_ERR_ARG, "null queries");
    if (a.nq != 0 && !a.radii) return fail(HNSWGPU_ERR_ARG, "null radii: every query names its radius");
    if (a.cap != 0 && (!a.out_ids || !a.out_dists))
        return fail(HNSWGPU_ERR_ARG, "cap > 0 with null out_ids or out_dists (the count-only call is cap == 0)");
    if (a.nq > 0xFFFFFFF0ull) return fail(HNSWGPU_ERR_ARG, "too many queries in one batch");
    if (dim != 0 && a.d != dim) return fail(HNSWGPU_ERR_ARG, "query dimension differs from the index dimension");
    if (a.n_allowed != 0 && !a.allowed) return fail(HNSWGPU_ERR_ARG, "null filter");
    if (idx->arithmetic != HNSWGPU_ARITH_SCALAR)
        return fail(HNSWGPU_ERR_ARG, "exact range search answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
    return capi_refuse_f16(idx, "exact range search");
}

static int exact_range_pair(const hnswgpu_index* cidx, const ExactRangeCallArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = exact_range_call(idx, a);
    if (rc != HNSWGPU_OK) return rc;
    if (host) {
        rc = check_sorted_filter(a.allowed, a.n_allowed);
        if (rc != HNSWGPU_OK) return rc;
        if (index_empty(idx) || a.nq == 0) {  // no point, or no query: every answer is empty (the device side's to answer in the device form)
            std::memset(a.out_offsets, 0, (a.nq + 1) * sizeof(uint64_t));
            return HNSWGPU_OK;
        }
    }
    if (!hnswgpu::exact_range) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(hnswgpu::exact_range(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswgpu_exact_range_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, const float* radii,
                                     const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t cap, uint64_t* out_offsets, uint64_t* out_ids,
                                     float* out_dists, uint8_t* out_layer, int32_t* out_rank) {
    CAPI_GUARD_BEGIN
    return exact_range_pair(idx, ExactRangeCallArgs{queries, radii, nq, d, allowed_ids, n_allowed, cap, out_offsets, out_ids, out_dists, out_layer, out_rank},
                            true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_exact_range_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, const float* d_radii,
                                            const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t cap, uint64_t* d_out_offsets,
                                            uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, void* stream) {
    CAPI_GUARD_BEGIN
    return exact_range_pair(idx, ExactRangeCallArgs{d_queries, d_radii, nq, d, d_allowed_ids, n_allowed, cap, d_out_offsets, d_out_ids, d_out_dists,
                                                    d_out_layer, d_out_rank},
                            false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- queries by stored point: the k-NN graph of the indexed points, approximate and exact (knn_graph.hip holds the device side)
// the checks all four entries share; the handle's lock is held (shared).  exact: the exact call's own limits behind them.
static int graph_call(const hnswgpu_index* idx, const GraphCallArgs& a, bool exact) {
    const uint64_t n = index_nb_point(idx);
    if (a.np != 0 && (!a.out_ids || !a.out_dists || !a.out_counts)) return fail(HNSWGPU_ERR_ARG, "null buffer");
    if (!a.point_ids && a.np != n)
        return fail(HNSWGPU_ERR_ARG, "point_ids is NULL (every point): np must be nb_point = " + std::to_string(n) + ", not " + std::to_string(a.np));
    if (a.k == 0) return fail(HNSWGPU_ERR_ARG, "knbn must be > 0");
    if (a.np > 0xFFFFFFF0ull) return fail(HNSWGPU_ERR_ARG, "too many points in one batch");
    if (!exact) return capi_refuse_f16(idx, "the graph search (its gather kernel copies stored rows)");
    if (a.k > 4096) return fail(HNSWGPU_ERR_ARG, "exact graph: knbn above 4096");
    if (a.n_allowed != 0 && !a.allowed) return fail(HNSWGPU_ERR_ARG, "null filter");
    if (idx->arithmetic != HNSWGPU_ARITH_SCALAR)
        return fail(HNSWGPU_ERR_ARG, "exact graph answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
    return capi_refuse_f16(idx, "exact graph");
}

// both pairs: exact picks hnswgpu_exact_graph_batch(_device), else hnswgpu_graph_search_batch(_device), which hands in no filter
static int graph_pair(const hnswgpu_index* cidx, const GraphCallArgs& a, bool exact, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = graph_call(idx, a, exact);
    if (rc != HNSWGPU_OK) return rc;
    if (host) {
        rc = check_sorted_filter(a.allowed, a.n_allowed);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (a.np == 0) return HNSWGPU_OK;  // no point asks nothing of a device
    if (host && index_empty(idx))  // an empty index names no point (the device form: it cannot be resident)
        return fail(HNSWGPU_ERR_ARG, std::to_string(a.np) + " of the " + std::to_string(a.np) + " point_ids name no point of the index");
    if (exact ? !hnswgpu::exact_graph : !hnswgpu::graph_search) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(exact ? hnswgpu::exact_graph(*dev, idx->flat->origin_id, a, host, stream, err)
                        : hnswgpu::graph_search(*dev, idx->flat->origin_id, a, host, stream, err),
                  err);
}

int hnswgpu_graph_search_batch(const hnswgpu_index* idx, const uint64_t* point_ids, uint64_t np, uint64_t k, uint64_t ef, uint64_t* out_ids,
                               float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts) {
    CAPI_GUARD_BEGIN
    return graph_pair(idx, GraphCallArgs{point_ids, np, k, ef, nullptr, 0, out_ids, out_dists, out_layer, out_rank, out_counts}, false, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_graph_search_batch_device(const hnswgpu_index* idx, const uint64_t* d_point_ids, uint64_t np, uint64_t k, uint64_t ef,
                                      uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                                      void* stream) {
    CAPI_GUARD_BEGIN
    return graph_pair(idx, GraphCallArgs{d_point_ids, np, k, ef, nullptr, 0, d_out_ids, d_out_dists, d_out_layer, d_out_rank, d_out_counts}, false, false,
                      stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_exact_graph_batch(const hnswgpu_index* idx, const uint64_t* point_ids, uint64_t np, uint64_t k, const uint64_t* allowed_ids,
                              uint64_t n_allowed, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts) {
    CAPI_GUARD_BEGIN
    return graph_pair(idx, GraphCallArgs{point_ids, np, k, 0, allowed_ids, n_allowed, out_ids, out_dists, out_layer, out_rank, out_counts}, true, true,
                      nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_exact_graph_batch_device(const hnswgpu_index* idx, const uint64_t* d_point_ids, uint64_t np, uint64_t k, const uint64_t* d_allowed_ids,
                                     uint64_t n_allowed, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank,
                                     uint32_t* d_out_counts, void* stream) {
    CAPI_GUARD_BEGIN
    return graph_pair(idx, GraphCallArgs{d_point_ids, np, k, 0, d_allowed_ids, n_allowed, d_out_ids, d_out_dists, d_out_layer, d_out_rank, d_out_counts},
                      true, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- approximate range search: the graph's answers cut at a radius, ef doubled until the result set reaches past the ball
// (range_search.hip holds the device side)
// the checks both forms share; the handle's lock is held (shared)
static int range_search_call(const hnswgpu_index* idx, const RangeSearchArgs& a) {
    const uint64_t dim = index_dimension(idx);
    if (!a.out_offsets) return fail(HNSWGPU_ERR_ARG, "null out_offsets: the offsets are written by every call");
    if (a.nq != 0 && !a.queries) return fail(HNSWGPU_ERR_ARG, "null queries");
    if (a.nq != 0 && !a.radii) return fail(HNSWGPU_ERR_ARG, "null radii: every query names its radius");
    if (a.ef_first < 1) return fail(HNSWGPU_ERR_ARG, "ef_first must be >= 1");
    if (a.ef_first > a.ef_max) return fail(HNSWGPU_ERR_ARG, "ef_first is above ef_max");
    if (a.ef_max > 4096) return fail(HNSWGPU_ERR_ARG, "range search: ef_max above 4096");
    if (a.n_allowed != 0 && !a.allowed) return fail(HNSWGPU_ERR_ARG, "null filter");
    if (a.filtered && a.ef_first < 2)
        return fail(HNSWGPU_ERR_ARG, "range search with a filter: ef_first must be >= 2 (the reference panics at ef == 1, src/hnsw.rs:973)");
    if (a.cap != 0 && (!a.out_ids || !a.out_dists))
        return fail(HNSWGPU_ERR_ARG, "cap > 0 with null out_ids or out_dists (the count-only call is cap == 0)");
    if (a.nq > 0xFFFFFFF0ull) return fail(HNSWGPU_ERR_ARG, "too many queries in one batch");
    if (dim != 0 && a.d != dim) return fail(HNSWGPU_ERR_ARG, "query dimension differs from the index dimension");
    return HNSWGPU_OK;
}

static int range_search_pair(const hnswgpu_index* cidx, const RangeSearchArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = range_search_call(idx, a);
    if (rc != HNSWGPU_OK) return rc;
    const bool nothing = index_empty(idx) || a.nq == 0;  // no point, or no query: every answer is empty
    if (host) {
        rc = check_sorted_filter(a.allowed, a.n_allowed);
        if (rc != HNSWGPU_OK) return rc;
        if (nothing) {
            std::memset(a.out_offsets, 0, (a.nq + 1) * sizeof(uint64_t));
            if (a.out_ef && a.nq != 0) std::memset(a.out_ef, 0, a.nq * sizeof(uint32_t));
            if (a.out_flags && a.nq != 0) std::memset(a.out_flags, 0, a.nq);
            return HNSWGPU_OK;
        }
    }
    if (!hnswgpu::range_search) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;  // (stays so in the device form where there is nothing to answer: the offsets are zeroed on the caller's stream)
    if (!nothing) {
        rc = call_replica(idx, sl, host, false, true, &dev);
        if (rc != HNSWGPU_OK) return rc;
    }
    std::string err;
    return finish(hnswgpu::range_search(dev, a, host, stream, err), err);
}

int hnswgpu_range_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, const float* radii, uint64_t ef_first,
                               uint64_t ef_max, const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t cap, uint64_t* out_offsets, uint64_t* out_ids,
                               float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_ef, uint8_t* out_flags) {
    CAPI_GUARD_BEGIN
    const RangeSearchArgs a{queries, radii, nq, d, ef_first, ef_max, allowed_ids, n_allowed, allowed_ids != nullptr, cap, out_offsets, out_ids, out_dists,
                            out_layer, out_rank, out_ef, out_flags};
    return range_search_pair(idx, a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_range_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, const float* d_radii,
                                      uint64_t ef_first, uint64_t ef_max, const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t cap,
                                      uint64_t* d_out_offsets, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank,
                                      uint32_t* d_out_ef, uint8_t* d_out_flags, void* stream) {
    CAPI_GUARD_BEGIN
    const RangeSearchArgs a{d_queries, d_radii, nq, d, ef_first, ef_max, d_allowed_ids, n_allowed, d_allowed_ids != nullptr, cap, d_out_offsets, d_out_ids,
                            d_out_dists, d_out_layer, d_out_rank, d_out_ef, d_out_flags};
    return range_search_pair(idx, a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- the k-NN graph of the indexed points made undirected, in CSR (symmetric_graph.hip holds the device side)
// The checks of the directed graph D that the symmetrised graph and the components share, in two halves (the symmetrised graph
// looks at its capacity in between); the handle's lock is held (shared).  What the source call of D refuses is refused here.
static int directed_graph_shape(uint64_t k, uint32_t mode) {
    if (k == 0) return fail(HNSWGPU_ERR_ARG, "knbn must be > 0");
    if (mode != HNSWGPU_SYM_UNION && mode != HNSWGPU_SYM_MUTUAL)
        return fail(HNSWGPU_ERR_ARG, "unknown mode " + std::to_string(mode) + ": HNSWGPU_SYM_UNION or HNSWGPU_SYM_MUTUAL");
    return HNSWGPU_OK;
}
static int directed_graph_source(const hnswgpu_index* idx, const char* what, uint64_t k, uint64_t ef) {
    const uint64_t n = index_nb_point(idx);
    if (n != 0 && k > (1ull << 30) / n)
        return fail(HNSWGPU_ERR_ARG, std::string(what) + ": nb_point x knbn = " + std::to_string(n) + " x " + std::to_string(k) +
                                         (k <= ~0ull / n ? " = " + std::to_string(n * k) : std::string()) + " slots, above 2^30 = 1073741824");
    if (ef != 0) return capi_refuse_f16(idx, "the graph search (its gather kernel copies stored rows)");
    if (k > 4096) return fail(HNSWGPU_ERR_ARG, "exact graph: knbn above 4096");
    if (idx->arithmetic != HNSWGPU_ARITH_SCALAR)
        return fail(HNSWGPU_ERR_ARG, "exact graph answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
    return capi_refuse_f16(idx, "exact graph");
}
// the checks both forms share
static int symmetric_graph_call(const hnswgpu_index* idx, const SymGraphArgs& a) {
    if (!a.out_offsets) return fail(HNSWGPU_ERR_ARG, "null out_offsets: the offsets are written by every call");
    const int rc = directed_graph_shape(a.k, a.mode);
    if (rc != HNSWGPU_OK) return rc;
    if (a.cap != 0 && (!a.out_pos || !a.out_dists))
        return fail(HNSWGPU_ERR_ARG, "cap > 0 with null out_pos or out_dists (the count-only call is cap == 0)");
    return directed_graph_source(idx, "symmetric graph", a.k, a.ef);
}

static int symmetric_graph_pair(const hnswgpu_index* cidx, const SymGraphArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = symmetric_graph_call(idx, a);
    if (rc != HNSWGPU_OK) return rc;
    const uint64_t n = index_nb_point(idx);
    if (host && n <= 1) {  // no point, or one: no edge
        std::memset(a.out_offsets, 0, (n + 1) * sizeof(uint64_t));
        return HNSWGPU_OK;
    }
    if (!hnswgpu::symmetric_graph) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    static const std::vector<uint64_t> no_ids;
    if (n == 0)  // (the device form) no point: the one offset is zeroed on the caller's stream
        return finish(hnswgpu::symmetric_graph(nullptr, no_ids, a, false, stream, err), err);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    return finish(hnswgpu::symmetric_graph(dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswgpu_symmetric_graph(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t cap, uint64_t* out_offsets, uint32_t* out_pos,
                            uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank) {
    CAPI_GUARD_BEGIN
    return symmetric_graph_pair(idx, SymGraphArgs{k, ef, mode, cap, out_offsets, out_pos, out_ids, out_dists, out_layer, out_rank}, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_symmetric_graph_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t cap, uint64_t* d_out_offsets,
                                   uint32_t* d_out_pos, uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, void* stream) {
    CAPI_GUARD_BEGIN
    return symmetric_graph_pair(idx, SymGraphArgs{k, ef, mode, cap, d_out_offsets, d_out_pos, d_out_ids, d_out_dists, d_out_layer, d_out_rank}, false,
                                stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- connected components: of the k-NN graph of the indexed points, and of any CSR (graph_components.hip holds the device side)
// what all four entries check of the answer's slots and of the cut (n: the number of vertices)
static int components_answer_check(uint64_t n, const float* max_dist, const uint32_t* out_label, const uint64_t* out_n_components) {
    if (!out_n_components) return fail(HNSWGPU_ERR_ARG, "null out_n_components: the number of components is written by every call");
    if (n != 0 && !out_label) return fail(HNSWGPU_ERR_ARG, "null out_label");
    if (max_dist && *max_dist != *max_dist) return fail(HNSWGPU_ERR_ARG, "max_dist is NaN: no distance compares to it (NULL is the call without a cut)");
    return HNSWGPU_OK;
}

static int graph_components_pair(const hnswgpu_index* cidx, uint64_t k, uint64_t ef, uint32_t mode, const float* max_dist, uint32_t* out_label,
                                 uint32_t* out_sizes, uint64_t* out_n_components, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = components_answer_check(index_nb_point(idx), max_dist, out_label, out_n_components);
    if (rc != HNSWGPU_OK) return rc;
    rc = directed_graph_shape(k, mode);
    if (rc != HNSWGPU_OK) return rc;
    rc = directed_graph_source(idx, "graph components", k, ef);
    if (rc != HNSWGPU_OK) return rc;
    if (index_empty(idx)) {  // no vertex: no component, nothing else written
        *out_n_components = 0;
        return HNSWGPU_OK;
    }
    if (!hnswgpu::graph_components) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    const ComponentsArgs a{k, ef, mode, max_dist != nullptr, max_dist ? *max_dist : 0.0f, out_label, out_sizes, out_n_components};
    std::string err;
    return finish(hnswgpu::graph_components(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswgpu_graph_components(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, const float* max_dist, uint32_t* out_label,
                             uint32_t* out_sizes, uint64_t* out_n_components) {
    CAPI_GUARD_BEGIN
    return graph_components_pair(idx, k, ef, mode, max_dist, out_label, out_sizes, out_n_components, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_graph_components_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, const float* max_dist, uint32_t* d_out_label,
                                    uint32_t* d_out_sizes, uint64_t* out_n_components, void* stream) {
    CAPI_GUARD_BEGIN
    return graph_components_pair(idx, k, ef, mode, max_dist, d_out_label, d_out_sizes, out_n_components, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// the graph itself as a host form reads it (n >= 1, offsets not NULL), as the device forms' validation kernels check it
static int csr_graph_check(const char* what, uint64_t n, const uint64_t* offsets, const uint32_t* cols) {
    const std::string w = std::string(what) + ": ";
    if (offsets[0] != 0) return fail(HNSWGPU_ERR_ARG, w + "offsets[0] is not 0");
    for (uint64_t r = 0; r < n; ++r)
        if (offsets[r] > offsets[r + 1]) return fail(HNSWGPU_ERR_ARG, w + "the offsets descend at row " + std::to_string(r));
    const uint64_t total = offsets[n];
    if (total >= (1ull << 32)) return fail(HNSWGPU_ERR_ARG, w + "offsets[n] = " + std::to_string(total) + " is 2^32 or more");
    if (total != 0 && !cols) return fail(HNSWGPU_ERR_ARG, w + "null cols with entries");
    for (uint64_t e = 0; e < total; ++e)
        if (cols[e] >= n) return fail(HNSWGPU_ERR_ARG, w + "col " + std::to_string(cols[e]) + " at entry " + std::to_string(e) + " is not below n");
    return HNSWGPU_OK;
}

static int csr_components_pair(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists, const float* max_dist,
                               uint32_t* out_label, uint32_t* out_sizes, uint64_t* out_n_components, bool host, void* stream) {
    int rc = components_answer_check(n, max_dist, out_label, out_n_components);
    if (rc != HNSWGPU_OK) return rc;
    if (n > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "csr components: n = " + std::to_string(n) + " vertices, above 2^31 - 1");
    if (n != 0 && !offsets) return fail(HNSWGPU_ERR_ARG, "null offsets");
    if (max_dist && !dists) return fail(HNSWGPU_ERR_ARG, "max_dist without dists: a cut needs the entries' distances");
    if (n == 0) {
        *out_n_components = 0;
        return HNSWGPU_OK;
    }
    if (host) {  // (the device form's validation kernels read the graph)
        rc = csr_graph_check("csr components", n, offsets, cols);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (!hnswgpu::csr_components) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    const CsrComponentsArgs a{device, n, offsets, cols, dists, max_dist != nullptr, max_dist ? *max_dist : 0.0f, out_label, out_sizes, out_n_components};
    std::string err;
    return finish(hnswgpu::csr_components(a, host, stream, err), err);
}

int hnswgpu_csr_components(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists, const float* max_dist,
                           uint32_t* out_label, uint32_t* out_sizes, uint64_t* out_n_components) {
    CAPI_GUARD_BEGIN
    return csr_components_pair(device, n, offsets, cols, dists, max_dist, out_label, out_sizes, out_n_components, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_csr_components_device(int device, uint64_t n, const uint64_t* d_offsets, const uint32_t* d_cols, const float* d_dists, const float* max_dist,
                                  uint32_t* d_out_label, uint32_t* d_out_sizes, uint64_t* out_n_components, void* stream) {
    CAPI_GUARD_BEGIN
    return csr_components_pair(device, n, d_offsets, d_cols, d_dists, max_dist, d_out_label, d_out_sizes, out_n_components, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- minimum spanning forest: of the k-NN graph of the indexed points, and of any CSR (spanning_forest.hip holds the device side)
// what all four entries check of the answer's slots (n: the number of vertices)
static int forest_answer_check(uint64_t n, const void* out_a, const void* out_b, const void* out_w, const uint64_t* out_n_edges) {
    if (!out_n_edges) return fail(HNSWGPU_ERR_ARG, "null out_n_edges: the number of edges is written by every call");
    if (n >= 2 && (!out_a || !out_b || !out_w)) return fail(HNSWGPU_ERR_ARG, "null out_a, out_b or out_w");
    return HNSWGPU_OK;
}
// the checks the index entries share; the handle's lock is held (shared)
// (the part behind the answer's slots: what hnswhdb_graph, whose forest arrays are optional, checks too)
static int graph_spanning_forest_source(const hnswgpu_index* idx, const ForestArgs& a) {
    const int rc = directed_graph_shape(a.k, a.mode);
    if (rc != HNSWGPU_OK) return rc;
    if (a.core_k > a.k)
        return fail(HNSWGPU_ERR_ARG, "core_k = " + std::to_string(a.core_k) + " is above knbn = " + std::to_string(a.k) + ": a row of D has knbn slots");
    return directed_graph_source(idx, "graph spanning forest", a.k, a.ef);
}
static int graph_spanning_forest_call(const hnswgpu_index* idx, const ForestArgs& a) {
    const int rc = forest_answer_check(index_nb_point(idx), a.out_a, a.out_b, a.out_w, a.out_n);
    if (rc != HNSWGPU_OK) return rc;
    return graph_spanning_forest_source(idx, a);
}

static int graph_spanning_forest_pair(const hnswgpu_index* cidx, const ForestArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = graph_spanning_forest_call(idx, a);
    if (rc != HNSWGPU_OK) return rc;
    if (index_nb_point(idx) <= 1) {  // no vertex, or one: no edge, nothing else written
        *a.out_n = 0;
        return HNSWGPU_OK;
    }
    if (!hnswgpu::graph_spanning_forest) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(hnswgpu::graph_spanning_forest(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswgpu_graph_spanning_forest(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k, uint32_t* out_a, uint32_t* out_b,
                                  float* out_w, uint64_t* out_n_edges) {
    CAPI_GUARD_BEGIN
    return graph_spanning_forest_pair(idx, ForestArgs{k, ef, mode, core_k, out_a, out_b, out_w, out_n_edges}, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_graph_spanning_forest_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k, uint32_t* d_out_a,
                                         uint32_t* d_out_b, float* d_out_w, uint64_t* out_n_edges, void* stream) {
    CAPI_GUARD_BEGIN
    return graph_spanning_forest_pair(idx, ForestArgs{k, ef, mode, core_k, d_out_a, d_out_b, d_out_w, out_n_edges}, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

static int csr_spanning_forest_pair(const CsrForestArgs& a, bool host, void* stream) {
    int rc = forest_answer_check(a.n, a.out_a, a.out_b, a.out_w, a.out_n);
    if (rc != HNSWGPU_OK) return rc;
    if (a.n > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "csr spanning forest: n = " + std::to_string(a.n) + " vertices, above 2^31 - 1");
    if (a.n != 0 && !a.offsets) return fail(HNSWGPU_ERR_ARG, "null offsets");
    if (a.n <= 1) {  // no vertex, or one: no edge (a self-loop is none); no array is read
        *a.out_n = 0;
        return HNSWGPU_OK;
    }
    if (host) {  // (the device form's validation kernels read the graph)
        rc = csr_graph_check("csr spanning forest", a.n, a.offsets, a.cols);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (!hnswgpu::csr_spanning_forest) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::csr_spanning_forest(a, host, stream, err), err);
}

int hnswgpu_csr_spanning_forest(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists, uint32_t* out_a, uint32_t* out_b,
                                float* out_w, uint64_t* out_n_edges) {
    CAPI_GUARD_BEGIN
    return csr_spanning_forest_pair(CsrForestArgs{device, n, offsets, cols, dists, out_a, out_b, out_w, out_n_edges}, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_csr_spanning_forest_device(int device, uint64_t n, const uint64_t* d_offsets, const uint32_t* d_cols, const float* d_dists, uint32_t* d_out_a,
                                       uint32_t* d_out_b, float* d_out_w, uint64_t* out_n_edges, void* stream) {
    CAPI_GUARD_BEGIN
    return csr_spanning_forest_pair(CsrForestArgs{device, n, d_offsets, d_cols, d_dists, d_out_a, d_out_b, d_out_w, out_n_edges}, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- dendrogram: of a forest given as an edge list, and of the k-NN graph's own forest (dendrogram.hip holds the device side)
// A forest given as an edge list, for the dendrogram and for HDBSCAN, which speaks of it in the dendrogram's words: its shape ...
static int forest_shape_check(uint64_t n, uint64_t m) {
    if (n > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "forest dendrogram: n = " + std::to_string(n) + " vertices, above 2^31 - 1");
    if (m > std::max<uint64_t>(n, 1) - 1)
        return fail(HNSWGPU_ERR_ARG, "forest dendrogram: m = " + std::to_string(m) + " edges among n = " + std::to_string(n) +
                                         " vertices: a forest has at most n - 1");
    return HNSWGPU_OK;
}
// ... and its ends as a host form reads them, as the device form's kernel checks them (a cycle is the device's to find)
static int forest_ends_check(uint64_t n, uint64_t m, const uint32_t* a, const uint32_t* b) {
    for (uint64_t e = 0; e < m; ++e) {
        if (a[e] >= n || b[e] >= n)
            return fail(HNSWGPU_ERR_ARG, "forest dendrogram: edge " + std::to_string(e) + " has an end that is not below n");
        if (a[e] == b[e]) return fail(HNSWGPU_ERR_ARG, "forest dendrogram: edge " + std::to_string(e) + " joins a vertex to itself");
    }
    return HNSWGPU_OK;
}

static int forest_dendrogram_pair(const DendrogramArgs& a, bool host, void* stream) {
    int rc = forest_shape_check(a.n, a.m);
    if (rc != HNSWGPU_OK) return rc;
    if (a.m != 0 && (!a.a || !a.b)) return fail(HNSWGPU_ERR_ARG, "null a or b");
    if (a.m != 0 && (!a.out_left || !a.out_right || !a.out_size)) return fail(HNSWGPU_ERR_ARG, "null out_left, out_right or out_size");
    if (a.m == 0) return HNSWGPU_OK;  // no merge: no array is read or written
    if (host) {
        rc = forest_ends_check(a.n, a.m, a.a, a.b);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (!hnswgpu::forest_dendrogram) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::forest_dendrogram(a, host, stream, err), err);
}

int hnswgpu_forest_dendrogram(int device, uint64_t n, uint64_t m, const uint32_t* a, const uint32_t* b, uint32_t* out_left, uint32_t* out_right,
                              uint32_t* out_size) {
    CAPI_GUARD_BEGIN
    return forest_dendrogram_pair(DendrogramArgs{device, n, m, a, b, out_left, out_right, out_size}, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_forest_dendrogram_device(int device, uint64_t n, uint64_t m, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out_left,
                                     uint32_t* d_out_right, uint32_t* d_out_size, void* stream) {
    CAPI_GUARD_BEGIN
    return forest_dendrogram_pair(DendrogramArgs{device, n, m, d_a, d_b, d_out_left, d_out_right, d_out_size}, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

static int graph_dendrogram_pair(const hnswgpu_index* cidx, const GraphDendrogramArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = graph_spanning_forest_call(idx, a.forest);  // the forest call's own checks, then the three new arrays
    if (rc != HNSWGPU_OK) return rc;
    if (index_nb_point(idx) >= 2 && (!a.out_left || !a.out_right || !a.out_size))
        return fail(HNSWGPU_ERR_ARG, "null out_left, out_right or out_size");
    if (index_nb_point(idx) <= 1) {  // no vertex, or one: no edge, nothing else written
        *a.forest.out_n = 0;
        return HNSWGPU_OK;
    }
    if (!hnswgpu::graph_dendrogram) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(hnswgpu::graph_dendrogram(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswgpu_graph_dendrogram(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k, uint32_t* out_a, uint32_t* out_b,
                             float* out_w, uint32_t* out_left, uint32_t* out_right, uint32_t* out_size, uint64_t* out_n_edges) {
    CAPI_GUARD_BEGIN
    const GraphDendrogramArgs a{ForestArgs{k, ef, mode, core_k, out_a, out_b, out_w, out_n_edges}, out_left, out_right, out_size};
    return graph_dendrogram_pair(idx, a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswgpu_graph_dendrogram_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k, uint32_t* d_out_a,
                                    uint32_t* d_out_b, float* d_out_w, uint32_t* d_out_left, uint32_t* d_out_right, uint32_t* d_out_size,
                                    uint64_t* out_n_edges, void* stream) {
    CAPI_GUARD_BEGIN
    const GraphDendrogramArgs a{ForestArgs{k, ef, mode, core_k, d_out_a, d_out_b, d_out_w, out_n_edges}, d_out_left, d_out_right, d_out_size};
    return graph_dendrogram_pair(idx, a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- HDBSCAN: condensed tree, stabilities and flat clusters of a forest in merge order, and of the k-NN graph's own forest
// (condensed_tree.hip holds the device side)
uint64_t hnswhdb_max_clusters(uint64_t n, uint64_t min_cluster_size) {
    if (min_cluster_size == 0) return 0;
    const uint64_t q = n / min_cluster_size;
    return q == 0 ? 1 : q > (~0ull >> 1) ? ~0ull : 2 * q - 1;
}

// what all four entries check of the clustering's own arguments (n: the number of vertices)
static int hdbscan_answer_check(uint64_t n, uint64_t mcs, uint32_t method, const HdbscanOut& o) {
    if (!o.n_clusters || !o.n_labels) return fail(HNSWGPU_ERR_ARG, "null out_n_clusters or out_n_labels: the two counts are written by every call");
    if (mcs < 2 || mcs > 0x7FFFFFFFull)
        return fail(HNSWGPU_ERR_ARG, "min_cluster_size = " + std::to_string(mcs) + ": it must be in 2 .. 2^31 - 1");
    if (method != HNSWGPU_SELECT_EOM && method != HNSWGPU_SELECT_LEAF)
        return fail(HNSWGPU_ERR_ARG, "unknown method " + std::to_string(method) + ": HNSWGPU_SELECT_EOM or HNSWGPU_SELECT_LEAF");
    if (n != 0 && !o.labels) return fail(HNSWGPU_ERR_ARG, "null out_labels");
    return HNSWGPU_OK;
}
static int forest_hdbscan_pair(const ForestHdbscanArgs& a, bool host, void* stream) {
    int rc = forest_shape_check(a.n, a.m);  // the dendrogram's checks, in its words, then the clustering's
    if (rc != HNSWGPU_OK) return rc;
    if (a.m != 0 && (!a.a || !a.b || !a.w)) return fail(HNSWGPU_ERR_ARG, "null a, b or w");
    rc = hdbscan_answer_check(a.n, a.min_cluster_size, a.method, a.out);
    if (rc != HNSWGPU_OK) return rc;
    if (a.n == 0) {  // no vertex: the two counts, no array is read or written
        *a.out.n_clusters = 0;
        *a.out.n_labels = 0;
        return HNSWGPU_OK;
    }
    if (host) {  // the ends as the dendrogram's kernel checks them, the weights as this call's kernel does
        rc = forest_ends_check(a.n, a.m, a.a, a.b);
        if (rc != HNSWGPU_OK) return rc;
        for (uint64_t e = 1; e < a.m; ++e)
            if (hnswgpu::dist_order_bits(a.w[e - 1]) > hnswgpu::dist_order_bits(a.w[e]))  // (dist_order.hpp: the kernel's order)
                return fail(HNSWGPU_ERR_ARG, "forest hdbscan: the weights descend at edge " + std::to_string(e) +
                                                 ": the edges' order is the merge order, ascending by weight");
    }
    if (!hnswgpu::forest_hdbscan) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::forest_hdbscan(a, host, stream, err), err);
}

int hnswhdb_forest(int device, uint64_t n, uint64_t m, const uint32_t* a, const uint32_t* b, const float* w, uint64_t min_cluster_size,
                           uint32_t method, int32_t* out_labels, float* out_prob, uint32_t* out_point_cluster, float* out_point_w,
                           uint32_t* out_cluster_parent, float* out_cluster_birth_w, uint32_t* out_cluster_size, double* out_stability,
                           uint8_t* out_selected, uint64_t* out_n_clusters, uint64_t* out_n_labels) {
    CAPI_GUARD_BEGIN
    const ForestHdbscanArgs args{device, n, m, a, b, w, min_cluster_size, method,
                                 HdbscanOut{out_labels, out_prob, out_point_cluster, out_point_w, out_cluster_parent, out_cluster_birth_w,
                                            out_cluster_size, out_stability, out_selected, out_n_clusters, out_n_labels}};
    return forest_hdbscan_pair(args, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswhdb_forest_device(int device, uint64_t n, uint64_t m, const uint32_t* d_a, const uint32_t* d_b, const float* d_w,
                                  uint64_t min_cluster_size, uint32_t method, int32_t* d_out_labels, float* d_out_prob,
                                  uint32_t* d_out_point_cluster, float* d_out_point_w, uint32_t* d_out_cluster_parent, float* d_out_cluster_birth_w,
                                  uint32_t* d_out_cluster_size, double* d_out_stability, uint8_t* d_out_selected, uint64_t* out_n_clusters,
                                  uint64_t* out_n_labels, void* stream) {
    CAPI_GUARD_BEGIN
    const ForestHdbscanArgs args{device, n, m, d_a, d_b, d_w, min_cluster_size, method,
                                 HdbscanOut{d_out_labels, d_out_prob, d_out_point_cluster, d_out_point_w, d_out_cluster_parent,
                                            d_out_cluster_birth_w, d_out_cluster_size, d_out_stability, d_out_selected, out_n_clusters, out_n_labels}};
    return forest_hdbscan_pair(args, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

static int graph_hdbscan_pair(const hnswgpu_index* cidx, const GraphHdbscanArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    // the dendrogram call's own checks in its words -- the six arrays of the forest and the dendrogram are optional here --, then the
    // clustering's
    if (!a.forest.out_n) return fail(HNSWGPU_ERR_ARG, "null out_n_edges: the number of edges is written by every call");
    int rc = graph_spanning_forest_source(idx, a.forest);
    if (rc != HNSWGPU_OK) return rc;
    rc = hdbscan_answer_check(index_nb_point(idx), a.min_cluster_size, a.method, a.out);
    if (rc != HNSWGPU_OK) return rc;
    if (index_empty(idx)) {  // no vertex: the three counts, nothing else written
        *a.forest.out_n = *a.out.n_clusters = *a.out.n_labels = 0;
        return HNSWGPU_OK;
    }
    if (!hnswgpu::graph_hdbscan) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(hnswgpu::graph_hdbscan(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswhdb_graph(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k, uint64_t min_cluster_size, uint32_t method,
                          uint32_t* out_a, uint32_t* out_b, float* out_w, uint32_t* out_left, uint32_t* out_right, uint32_t* out_size,
                          int32_t* out_labels, float* out_prob, uint32_t* out_point_cluster, float* out_point_w, uint32_t* out_cluster_parent,
                          float* out_cluster_birth_w, uint32_t* out_cluster_size, double* out_stability, uint8_t* out_selected,
                          uint64_t* out_n_clusters, uint64_t* out_n_labels, uint64_t* out_n_edges) {
    CAPI_GUARD_BEGIN
    const GraphHdbscanArgs a{ForestArgs{k, ef, mode, core_k, out_a, out_b, out_w, out_n_edges}, out_left, out_right, out_size, min_cluster_size, method,
                             HdbscanOut{out_labels, out_prob, out_point_cluster, out_point_w, out_cluster_parent, out_cluster_birth_w,
                                        out_cluster_size, out_stability, out_selected, out_n_clusters, out_n_labels}};
    return graph_hdbscan_pair(idx, a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswhdb_graph_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k, uint64_t min_cluster_size,
                                 uint32_t method, uint32_t* d_out_a, uint32_t* d_out_b, float* d_out_w, uint32_t* d_out_left, uint32_t* d_out_right,
                                 uint32_t* d_out_size, int32_t* d_out_labels, float* d_out_prob, uint32_t* d_out_point_cluster, float* d_out_point_w,
                                 uint32_t* d_out_cluster_parent, float* d_out_cluster_birth_w, uint32_t* d_out_cluster_size, double* d_out_stability,
                                 uint8_t* d_out_selected, uint64_t* out_n_clusters, uint64_t* out_n_labels, uint64_t* out_n_edges, void* stream) {
    CAPI_GUARD_BEGIN
    const GraphHdbscanArgs a{ForestArgs{k, ef, mode, core_k, d_out_a, d_out_b, d_out_w, out_n_edges}, d_out_left, d_out_right, d_out_size,
                             min_cluster_size, method,
                             HdbscanOut{d_out_labels, d_out_prob, d_out_point_cluster, d_out_point_w, d_out_cluster_parent, d_out_cluster_birth_w,
                                        d_out_cluster_size, d_out_stability, d_out_selected, out_n_clusters, out_n_labels}};
    return graph_hdbscan_pair(idx, a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- HDBSCAN, second stage: the selection under its options, labels and GLOSH scores from a condensed tree
// (hnsw_mi355x_hdbscan_select.h; cluster_select.hip holds the device side)
// A condensed tree as a host form reads it, as the device forms' kernels check it (cluster_tree.hpp), in the words of `prefix`:
// cluster_parent, point_cluster and, where it is there, stability -- with it, the number of children of every cluster other than 0.
static int condensed_tree_check(const std::string& prefix, uint64_t n, uint64_t K, const uint32_t* parent, const uint32_t* point_cluster,
                                const double* stability) {
    if (K != 0 && parent[0] != 0xFFFFFFFFu) return fail(HNSWGPU_ERR_ARG, prefix + " cluster_parent[0] is not UINT32_MAX");
    std::vector<uint8_t> kids(stability ? K : 0, 0);
    for (uint64_t c = 0; c < K; ++c) {
        if (stability && !(stability[c] >= 0.0)) return fail(HNSWGPU_ERR_ARG, prefix + " a stability is NaN or negative (cluster " + std::to_string(c) + ")");
        if (c == 0) continue;
        const uint32_t p = parent[c];
        if (p >= c) return fail(HNSWGPU_ERR_ARG, prefix + " a cluster_parent[c] is not below c (cluster " + std::to_string(c) + ")");
        if (stability && p != 0 && kids[p] < 3) ++kids[p];
    }
    for (uint64_t c = 1; c < kids.size(); ++c)
        if (kids[c] != 0 && kids[c] != 2)
            return fail(HNSWGPU_ERR_ARG, prefix + " a cluster other than 0 has one child, or more than two (cluster " + std::to_string(c) + ")");
    for (uint64_t v = 0; v < n; ++v)
        if (point_cluster[v] >= K) return fail(HNSWGPU_ERR_ARG, prefix + " a point_cluster[v] is not below K (vertex " + std::to_string(v) + ")");
    return HNSWGPU_OK;
}

static int hdbscan_select_pair(const HdbscanSelectArgs& a, bool host, void* stream) {
    if (a.method != HNSWGPU_SELECT_EOM && a.method != HNSWGPU_SELECT_LEAF)
        return fail(HNSWGPU_ERR_ARG, "unknown method " + std::to_string(a.method) + ": HNSWGPU_SELECT_EOM or HNSWGPU_SELECT_LEAF");
    if (a.allow_single_cluster > 1)
        return fail(HNSWGPU_ERR_ARG, "allow_single_cluster = " + std::to_string(a.allow_single_cluster) + ": it must be 0 or 1");
    if (!(a.eps >= 0.0f)) return fail(HNSWGPU_ERR_ARG, "cluster_selection_epsilon is NaN or negative: it must be a weight, 0 or more");
    if (a.n > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "hdbscan select: n = " + std::to_string(a.n) + " vertices, above 2^31 - 1");
    if (a.clusters > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "hdbscan select: K = " + std::to_string(a.clusters) + " clusters, above 2^31 - 1");
    if (!a.out_n_labels) return fail(HNSWGPU_ERR_ARG, "null out_n_labels: the number of labels is written by every call");
    if (a.n == 0) {  // no vertex: the count, no array is read or written
        *a.out_n_labels = 0;
        return HNSWGPU_OK;
    }
    if (a.clusters == 0) return fail(HNSWGPU_ERR_ARG, "hdbscan select: K = 0 clusters over " + std::to_string(a.n) + " vertices: cluster 0 is always there");
    if (!a.cluster_parent || !a.cluster_birth_w || !a.cluster_size || !a.stability)
        return fail(HNSWGPU_ERR_ARG, "null cluster_parent, cluster_birth_w, cluster_size or stability");
    if (!a.point_cluster || !a.point_w) return fail(HNSWGPU_ERR_ARG, "null point_cluster or point_w");
    if (!a.out_labels) return fail(HNSWGPU_ERR_ARG, "null out_labels");
    if (host) {
        const int rc = condensed_tree_check("hdbscan select: not a condensed tree:", a.n, a.clusters, a.cluster_parent, a.point_cluster, a.stability);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (!hnswgpu::hdbscan_select) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::hdbscan_select(a, host, stream, err), err);
}

int hnswhds_select(int device, uint64_t n, uint64_t K, const uint32_t* cluster_parent, const float* cluster_birth_w, const uint32_t* cluster_size,
                   const double* stability, const uint32_t* point_cluster, const float* point_w, uint32_t method, uint32_t allow_single_cluster,
                   float cluster_selection_epsilon, uint64_t max_cluster_size, uint8_t* out_selected, int32_t* out_labels, float* out_prob,
                   float* out_outlier_score, double* out_cluster_death_lambda, uint64_t* out_n_labels) {
    CAPI_GUARD_BEGIN
    const HdbscanSelectArgs a{device, n, K, cluster_parent, cluster_birth_w, cluster_size, stability, point_cluster, point_w, method,
                              allow_single_cluster, cluster_selection_epsilon, max_cluster_size, out_selected, out_labels, out_prob,
                              out_outlier_score, out_cluster_death_lambda, out_n_labels};
    return hdbscan_select_pair(a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswhds_select_device(int device, uint64_t n, uint64_t K, const uint32_t* d_cluster_parent, const float* d_cluster_birth_w,
                          const uint32_t* d_cluster_size, const double* d_stability, const uint32_t* d_point_cluster, const float* d_point_w,
                          uint32_t method, uint32_t allow_single_cluster, float cluster_selection_epsilon, uint64_t max_cluster_size,
                          uint8_t* d_out_selected, int32_t* d_out_labels, float* d_out_prob, float* d_out_outlier_score,
                          double* d_out_cluster_death_lambda, uint64_t* out_n_labels, void* stream) {
    CAPI_GUARD_BEGIN
    const HdbscanSelectArgs a{device, n, K, d_cluster_parent, d_cluster_birth_w, d_cluster_size, d_stability, d_point_cluster, d_point_w, method,
                              allow_single_cluster, cluster_selection_epsilon, max_cluster_size, d_out_selected, d_out_labels, d_out_prob,
                              d_out_outlier_score, d_out_cluster_death_lambda, out_n_labels};
    return hdbscan_select_pair(a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- HDBSCAN, third stage: new points assigned to the clusters of a condensed tree
// (hnsw_mi355x_hdbscan_predict.h; cluster_predict.hip holds the device side)
static int core_distances_pair(const hnswgpu_index* cidx, const CoreDistancesArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    // what hnswgpu_graph_spanning_forest refuses of the same knbn, ef and core_k, in its words
    if (a.k == 0) return fail(HNSWGPU_ERR_ARG, "knbn must be > 0");
    if (a.core_k > a.k)
        return fail(HNSWGPU_ERR_ARG, "core_k = " + std::to_string(a.core_k) + " is above knbn = " + std::to_string(a.k) + ": a row of D has knbn slots");
    int rc = directed_graph_source(idx, "core distances", a.k, a.ef);
    if (rc != HNSWGPU_OK) return rc;
    if (index_empty(idx)) return HNSWGPU_OK;  // no point: nothing written
    if (!a.out_core) return fail(HNSWGPU_ERR_ARG, "null out_core");
    if (!hnswgpu::core_distances) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(hnswgpu::core_distances(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswhdp_core_distances(const hnswgpu_index* idx, uint64_t knbn, uint64_t ef, uint64_t core_k, float* out_core) {
    CAPI_GUARD_BEGIN
    return core_distances_pair(idx, CoreDistancesArgs{knbn, ef, core_k, out_core}, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswhdp_core_distances_device(const hnswgpu_index* idx, uint64_t knbn, uint64_t ef, uint64_t core_k, float* d_out_core, void* stream) {
    CAPI_GUARD_BEGIN
    return core_distances_pair(idx, CoreDistancesArgs{knbn, ef, core_k, d_out_core}, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// what both forms of both pairs check without reading an array, in the header's order
static int predict_shape_check(const PredictTree& t, uint64_t nq, uint64_t k, uint64_t core_k) {
    if (!(t.eps >= 0.0f)) return fail(HNSWGPU_ERR_ARG, "cluster_selection_epsilon is NaN or negative: it must be a weight, 0 or more");
    if (core_k > k)
        return fail(HNSWGPU_ERR_ARG, "core_k = " + std::to_string(core_k) + " is above knbn = " + std::to_string(k) + ": a row has knbn slots");
    if (k == 0 && nq != 0) return fail(HNSWGPU_ERR_ARG, "knbn must be > 0");
    if (t.n > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "hdbscan predict: n = " + std::to_string(t.n) + " vertices, above 2^31 - 1");
    if (t.clusters > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "hdbscan predict: K = " + std::to_string(t.clusters) + " clusters, above 2^31 - 1");
    if (nq > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, "hdbscan predict: nq = " + std::to_string(nq) + " queries, above 2^31 - 1");
    if (k != 0 && nq > 0x7FFFFFFFull / k)
        return fail(HNSWGPU_ERR_ARG, "hdbscan predict: nq x knbn = " + std::to_string(nq) + " x " + std::to_string(k) + " slots, above 2^31 - 1");
    if (t.clusters == 0 && t.n != 0)
        return fail(HNSWGPU_ERR_ARG, "hdbscan predict: K = 0 clusters over " + std::to_string(t.n) + " vertices: cluster 0 is always there");
    return HNSWGPU_OK;
}
// ... and the arrays that a call with a query needs
static int predict_arrays_check(const PredictTree& t, const PredictOut& o) {
    if (t.n != 0 && (!t.core || !t.point_cluster || !t.point_w)) return fail(HNSWGPU_ERR_ARG, "null core, point_cluster or point_w");
    if (t.clusters != 0 && (!t.cluster_parent || !t.cluster_birth_w || !t.selected))
        return fail(HNSWGPU_ERR_ARG, "null cluster_parent, cluster_birth_w or selected");
    if (!o.labels) return fail(HNSWGPU_ERR_ARG, "null out_labels");
    if (o.score && !t.death) return fail(HNSWGPU_ERR_ARG, "out_score without cluster_death_lambda: the score is GLOSH's, from each cluster's death");
    return HNSWGPU_OK;
}
static int predict_tree_check(const PredictTree& t) {
    return condensed_tree_check("hdbscan predict: refused:", t.n, t.clusters, t.cluster_parent, t.point_cluster, nullptr);
}

static int hdbscan_assign_pair(const HdbscanAssignArgs& a, bool host, void* stream) {
    int rc = predict_shape_check(a.tree, a.nq, a.k, a.core_k);
    if (rc != HNSWGPU_OK) return rc;
    if (a.nq == 0) return HNSWGPU_OK;  // no query: no array is read or written
    if (!a.nbr_pos || !a.nbr_dist || !a.counts) return fail(HNSWGPU_ERR_ARG, "null nbr_pos, nbr_dist or counts");
    rc = predict_arrays_check(a.tree, a.out);
    if (rc != HNSWGPU_OK) return rc;
    if (host) {
        rc = predict_tree_check(a.tree);
        if (rc != HNSWGPU_OK) return rc;
        for (uint64_t q = 0; q < a.nq; ++q) {
            if (a.counts[q] > a.k)
                return fail(HNSWGPU_ERR_ARG, "hdbscan predict: refused: a counts[q] is above knbn (query " + std::to_string(q) + ")");
            for (uint64_t s = 0; s < a.counts[q]; ++s)
                if (a.nbr_pos[q * a.k + s] >= a.tree.n)
                    return fail(HNSWGPU_ERR_ARG, "hdbscan predict: refused: a used nbr_pos is not below n (query " + std::to_string(q) + ")");
        }
    }
    if (!hnswgpu::hdbscan_assign) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::hdbscan_assign(a, host, stream, err), err);
}

int hnswhdp_assign(int device, uint64_t nq, uint64_t knbn, const uint32_t* nbr_pos, const float* nbr_dist, const uint32_t* counts, uint64_t core_k,
                   uint64_t n, const float* core, uint64_t K, const uint32_t* cluster_parent, const float* cluster_birth_w, const uint32_t* point_cluster,
                   const float* point_w, const uint8_t* selected, float cluster_selection_epsilon, const double* cluster_death_lambda,
                   int32_t* out_labels, float* out_prob, float* out_score, uint32_t* out_nearest, float* out_w, uint32_t* out_cluster) {
    CAPI_GUARD_BEGIN
    const HdbscanAssignArgs a{device, nq, knbn, nbr_pos, nbr_dist, counts, core_k,
                              PredictTree{n, K, core, cluster_parent, cluster_birth_w, point_cluster, point_w, selected, cluster_selection_epsilon,
                                          cluster_death_lambda},
                              PredictOut{out_labels, out_prob, out_score, out_nearest, out_w, out_cluster}};
    return hdbscan_assign_pair(a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswhdp_assign_device(int device, uint64_t nq, uint64_t knbn, const uint32_t* d_nbr_pos, const float* d_nbr_dist, const uint32_t* d_counts,
                          uint64_t core_k, uint64_t n, const float* d_core, uint64_t K, const uint32_t* d_cluster_parent, const float* d_cluster_birth_w,
                          const uint32_t* d_point_cluster, const float* d_point_w, const uint8_t* d_selected, float cluster_selection_epsilon,
                          const double* d_cluster_death_lambda, int32_t* d_out_labels, float* d_out_prob, float* d_out_score, uint32_t* d_out_nearest,
                          float* d_out_w, uint32_t* d_out_cluster, void* stream) {
    CAPI_GUARD_BEGIN
    const HdbscanAssignArgs a{device, nq, knbn, d_nbr_pos, d_nbr_dist, d_counts, core_k,
                              PredictTree{n, K, d_core, d_cluster_parent, d_cluster_birth_w, d_point_cluster, d_point_w, d_selected,
                                          cluster_selection_epsilon, d_cluster_death_lambda},
                              PredictOut{d_out_labels, d_out_prob, d_out_score, d_out_nearest, d_out_w, d_out_cluster}};
    return hdbscan_assign_pair(a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// (b: the call as the entry built it; its tree's n is filled in here, from the index)
static int hdbscan_predict_pair(const hnswgpu_index* cidx, const HdbscanPredictArgs& b, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    HdbscanPredictArgs a = b;
    a.tree.n = index_nb_point(idx);
    int rc = capi_refuse_f16(idx, "hdbscan predict (it names positions)");
    if (rc != HNSWGPU_OK) return rc;
    rc = predict_shape_check(a.tree, a.nq, a.k, a.core_k);
    if (rc != HNSWGPU_OK) return rc;
    if (a.nq == 0) return HNSWGPU_OK;  // no query: no array is read or written
    if (!a.queries) return fail(HNSWGPU_ERR_ARG, "null buffer");
    rc = predict_arrays_check(a.tree, a.out);
    if (rc != HNSWGPU_OK) return rc;
    if (a.ef == 0) {  // the limits of the exact call, in its words (the answers are staged: no buffer of the caller's to check)
        rc = check_exact_call(idx, a.queries, a.nq, a.d, a.k, nullptr, 0, a.queries, a.queries, a.queries);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (host) {
        rc = predict_tree_check(a.tree);
        if (rc != HNSWGPU_OK) return rc;
    }
    std::string err;
    if (a.tree.n == 0) {  // no point: every row is empty, on the handle's device (host form) or the caller's current one
        if (!hnswgpu::hdbscan_assign) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
        const HdbscanAssignArgs rows{host ? std::max(idx->primary, 0) : -1, a.nq, 0, nullptr, nullptr, nullptr, 0, a.tree, a.out};
        return finish(hnswgpu::hdbscan_assign(rows, host, stream, err), err);
    }
    if (!hnswgpu::hdbscan_predict) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    return finish(hnswgpu::hdbscan_predict(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswhdp_predict(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t knbn, uint64_t ef, uint64_t core_k, const float* core,
                    uint64_t K, const uint32_t* cluster_parent, const float* cluster_birth_w, const uint32_t* point_cluster, const float* point_w,
                    const uint8_t* selected, float cluster_selection_epsilon, const double* cluster_death_lambda, int32_t* out_labels, float* out_prob,
                    float* out_score, uint32_t* out_nearest, float* out_w, uint32_t* out_cluster) {
    CAPI_GUARD_BEGIN
    const HdbscanPredictArgs a{queries, nq, d, knbn, ef, core_k,
                               PredictTree{0, K, core, cluster_parent, cluster_birth_w, point_cluster, point_w, selected, cluster_selection_epsilon,
                                           cluster_death_lambda},
                               PredictOut{out_labels, out_prob, out_score, out_nearest, out_w, out_cluster}};
    return hdbscan_predict_pair(idx, a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswhdp_predict_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t knbn, uint64_t ef, uint64_t core_k,
                           const float* d_core, uint64_t K, const uint32_t* d_cluster_parent, const float* d_cluster_birth_w,
                           const uint32_t* d_point_cluster, const float* d_point_w, const uint8_t* d_selected, float cluster_selection_epsilon,
                           const double* d_cluster_death_lambda, int32_t* d_out_labels, float* d_out_prob, float* d_out_score, uint32_t* d_out_nearest,
                           float* d_out_w, uint32_t* d_out_cluster, void* stream) {
    CAPI_GUARD_BEGIN
    const HdbscanPredictArgs a{d_queries, nq, d, knbn, ef, core_k,
                               PredictTree{0, K, d_core, d_cluster_parent, d_cluster_birth_w, d_point_cluster, d_point_w, d_selected,
                                           cluster_selection_epsilon, d_cluster_death_lambda},
                               PredictOut{d_out_labels, d_out_prob, d_out_score, d_out_nearest, d_out_w, d_out_cluster}};
    return hdbscan_predict_pair(idx, a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- DBSCAN: exact over the points of the index, and over any CSR (hnsw_mi355x_dbscan.h; dbscan.hip holds the device side)
// what all four entries check of the parameters and of the answer's slots (n: the number of vertices)
static int dbscan_call_check(const char* what, uint64_t n, const DbscanArgs& a) {
    if (a.min_samples == 0) return fail(HNSWGPU_ERR_ARG, "min_samples must be > 0");
    if (a.eps != a.eps) return fail(HNSWGPU_ERR_ARG, "eps is NaN: no distance compares to it");
    if (n > 0x7FFFFFFFull) return fail(HNSWGPU_ERR_ARG, std::string(what) + ": n = " + std::to_string(n) + " vertices, above 2^31 - 1");
    if (n != 0 && !a.out.label) return fail(HNSWGPU_ERR_ARG, "null out_label");
    if (!a.out.out_n) return fail(HNSWGPU_ERR_ARG, "null out_n_clusters: the number of clusters is written by every call");
    return HNSWGPU_OK;
}

static int exact_dbscan_pair(const hnswgpu_index* cidx, const DbscanArgs& a, bool host, void* stream) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> sl(idx->mu);
    int rc = dbscan_call_check("dbscan", index_nb_point(idx), a);
    if (rc != HNSWGPU_OK) return rc;
    if (idx->arithmetic != HNSWGPU_ARITH_SCALAR)
        return fail(HNSWGPU_ERR_ARG, "dbscan answers in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
    rc = capi_refuse_f16(idx, "dbscan");
    if (rc != HNSWGPU_OK) return rc;
    if (index_empty(idx)) {  // no vertex: no cluster, nothing else written
        *a.out.out_n = 0;
        return HNSWGPU_OK;
    }
    if (!hnswgpu::exact_dbscan) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    DeviceIndex* dev = nullptr;
    rc = call_replica(idx, sl, host, true, true, &dev);
    if (rc != HNSWGPU_OK) return rc;
    std::string err;
    return finish(hnswgpu::exact_dbscan(*dev, idx->flat->origin_id, a, host, stream, err), err);
}

int hnswdbs_exact(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* out_label, uint8_t* out_core, uint32_t* out_count,
                  uint32_t* out_anchor, uint64_t* out_n_clusters) {
    CAPI_GUARD_BEGIN
    return exact_dbscan_pair(idx, DbscanArgs{eps, min_samples, DbscanOut{out_label, out_core, out_count, out_anchor, out_n_clusters}}, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswdbs_exact_device(const hnswgpu_index* idx, float eps, uint64_t min_samples, int32_t* d_out_label, uint8_t* d_out_core, uint32_t* d_out_count,
                         uint32_t* d_out_anchor, uint64_t* out_n_clusters, void* stream) {
    CAPI_GUARD_BEGIN
    return exact_dbscan_pair(idx, DbscanArgs{eps, min_samples, DbscanOut{d_out_label, d_out_core, d_out_count, d_out_anchor, out_n_clusters}}, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

static int csr_dbscan_pair(const CsrDbscanArgs& a, bool host, void* stream) {
    int rc = dbscan_call_check("csr dbscan", a.n, a.call);
    if (rc != HNSWGPU_OK) return rc;
    if (a.add_self > 1) return fail(HNSWGPU_ERR_ARG, "add_self must be 0 or 1, not " + std::to_string(a.add_self));
    if (a.n != 0 && !a.offsets) return fail(HNSWGPU_ERR_ARG, "null offsets");
    if (a.n == 0) {
        *a.call.out.out_n = 0;
        return HNSWGPU_OK;
    }
    if (host) {  // (the device form's validation kernels read the graph)
        rc = csr_graph_check("csr dbscan", a.n, a.offsets, a.cols);
        if (rc != HNSWGPU_OK) return rc;
    }
    if (!hnswgpu::csr_dbscan) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::csr_dbscan(a, host, stream, err), err);
}

int hnswdbs_csr(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists, float eps, uint64_t min_samples,
                uint32_t add_self, int32_t* out_label, uint8_t* out_core, uint32_t* out_count, uint32_t* out_anchor, uint64_t* out_n_clusters) {
    CAPI_GUARD_BEGIN
    const CsrDbscanArgs a{device, n, offsets, cols, dists, add_self,
                          DbscanArgs{eps, min_samples, DbscanOut{out_label, out_core, out_count, out_anchor, out_n_clusters}}};
    return csr_dbscan_pair(a, true, nullptr);
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}

int hnswdbs_csr_device(int device, uint64_t n, const uint64_t* d_offsets, const uint32_t* d_cols, const float* d_dists, float eps,
                       uint64_t min_samples, uint32_t add_self, int32_t* d_out_label, uint8_t* d_out_core, uint32_t* d_out_count,
                       uint32_t* d_out_anchor, uint64_t* out_n_clusters, void* stream) {
    CAPI_GUARD_BEGIN
    const CsrDbscanArgs a{device, n, d_offsets, d_cols, d_dists, add_self,
                          DbscanArgs{eps, min_samples, DbscanOut{d_out_label, d_out_core, d_out_count, d_out_anchor, out_n_clusters}}};
    return csr_dbscan_pair(a, false, stream);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

static DeviceIndex* any_replica(hnswgpu_index* idx) {
    if (idx->primary >= 0 && idx->replica(idx->primary)) return idx->replica(idx->primary);
    return nullptr;
}
int hnswgpu_last_kernel_ms(const hnswgpu_index* cidx, double* ms, uint32_t* launches) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> g(idx->mu);
    DeviceIndex* dev = any_replica(idx);
    if (!dev) return fail(HNSWGPU_ERR_DEVICE, "index is not resident on a device");
    const CallInfo c = dev->last_call();
    if (ms) *ms = c.ms;
    if (launches) *launches = c.launches;
    return HNSWGPU_OK;
}
int hnswgpu_last_search_kernel_ms(const hnswgpu_index* cidx, double* ms) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !ms) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> g(idx->mu);
    DeviceIndex* dev = any_replica(idx);
    if (!dev) return fail(HNSWGPU_ERR_DEVICE, "index is not resident on a device");
    *ms = dev->last_call().main_ms;
    return HNSWGPU_OK;
}
int hnswgpu_set_arithmetic(hnswgpu_index* idx, int arithmetic) {
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    if (arithmetic != HNSWGPU_ARITH_SCALAR && arithmetic != HNSWGPU_ARITH_SIMD8) return fail(HNSWGPU_ERR_ARG, "unknown arithmetic");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    if (arithmetic == HNSWGPU_ARITH_SIMD8 && idx->storage == HNSWGPU_STORAGE_F16)
        return fail(HNSWGPU_ERR_ARG, "HNSWGPU_ARITH_SIMD8 reads f32 rows only: the index is set to HNSWGPU_STORAGE_F16");
    idx->arithmetic = arithmetic;
    for (auto& kv : idx->replicas) kv.second->set_arithmetic(arithmetic);
    return HNSWGPU_OK;
}
int hnswgpu_set_storage(hnswgpu_index* idx, int storage) {
    CAPI_GUARD_BEGIN
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    if (storage != HNSWGPU_STORAGE_F32 && storage != HNSWGPU_STORAGE_F16) return fail(HNSWGPU_ERR_ARG, "unknown storage");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    if (storage == idx->storage) return HNSWGPU_OK;
    if (storage == HNSWGPU_STORAGE_F16) {
        if (!idx->builder && !idx->flat) return fail(HNSWGPU_ERR_EMPTY, "handle holds no index");
        const int dist = idx->builder ? idx->params.dist : idx->flat->dist;
        if (dist != DIST_L2 && dist != DIST_COSINE && dist != DIST_DOT && dist != DIST_L1)
            return fail(HNSWGPU_ERR_ARG, "HNSWGPU_STORAGE_F16 serves DistL2, DistCosine, DistDot and DistL1 only");
        if (idx->arithmetic == HNSWGPU_ARITH_SIMD8)
            return fail(HNSWGPU_ERR_ARG, "HNSWGPU_STORAGE_F16 is read in the scalar arithmetic only: the index is set to HNSWGPU_ARITH_SIMD8");
        // the caller rounds, the library only verifies: every stored vector, on the host
        const FlatIndex* f = idx->get_flat();
        if (f && f->n != 0) {
            uint64_t first = 0;
            const uint64_t bad = f16_count_unrepresentable(f->vectors.data(), f->n * f->dimension, &first);
            if (bad != 0)
                return fail(HNSWGPU_ERR_ARG, unrepresentable_message(bad, f->origin_id[first / f->dimension], first % f->dimension) +
                                             "; the index keeps its storage");
        }
    }
    idx->storage = storage;
    idx->dev_stale = true;  // like an insert: the next upload, explicit or in front of a search, makes replicas of the new kind
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_ARG)
}
int hnswgpu_get_storage(const hnswgpu_index* cidx) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> g(idx->mu);
    return idx->storage;
}
uint64_t hnswgpu_f16_representable(const float* x, uint64_t n, uint64_t* first_bad) {
    if (!x || n == 0) return 0;
    return f16_count_unrepresentable(x, n, first_bad);
}
int hnswgpu_device_bytes(const hnswgpu_index* cidx, int device, uint64_t* bytes) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !bytes) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> g(idx->mu);
    if (device < 0) device = idx->primary;
    DeviceIndex* dev = idx->dev_stale || idx->flat_stale ? nullptr : idx->replica(device);
    if (!dev) return fail(HNSWGPU_ERR_DEVICE, "index is not resident on that device (hnswgpu_upload first)");
    *bytes = dev->bytes();
    return HNSWGPU_OK;
}
int hnswgpu_set_strict_ties(hnswgpu_index* idx, int on) {
    if (!idx) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::unique_lock<std::shared_mutex> g(idx->mu);
    idx->strict_ties = on != 0;
    for (auto& kv : idx->replicas) kv.second->set_strict_ties(idx->strict_ties != 0);
    return HNSWGPU_OK;
}
int hnswgpu_reload_env(void) {
    hnswgpu::reload_knobs();
    return HNSWGPU_OK;
}
int hnswgpu_last_tie_count(const hnswgpu_index* cidx, uint32_t* ties) {
    hnswgpu_index* idx = const_cast<hnswgpu_index*>(cidx);
    if (!idx || !ties) return fail(HNSWGPU_ERR_ARG, "null argument");
    std::shared_lock<std::shared_mutex> g(idx->mu);
    DeviceIndex* dev = any_replica(idx);
    if (!dev) return fail(HNSWGPU_ERR_DEVICE, "index is not resident on a device");
    *ties = dev->last_call().ties;
    return HNSWGPU_OK;
}

int hnswgpu_eval_distances(int dist, const float* a, const float* b, uint64_t n, uint64_t d, float* out) {
    CAPI_GUARD_BEGIN
    if (!a || !b || !out || dist < 0 || dist >= DIST_COUNT) return fail(HNSWGPU_ERR_ARG, "bad argument");
    std::string err;
    return finish(eval_distance_matrix_device(dist, a, n, b, n, d, 1, true, out, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}
int hnswgpu_eval_distance_matrix(int dist, const float* queries, uint64_t nq, const float* rows, uint64_t n, uint64_t d,
                                 uint32_t batch, float* out) {
    CAPI_GUARD_BEGIN
    if (!queries || !rows || !out || dist < 0 || dist >= DIST_COUNT) return fail(HNSWGPU_ERR_ARG, "bad argument");
    std::string err;
    return finish(eval_distance_matrix_device(dist, queries, nq, rows, n, d, batch, false, out, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

int hnswgpu_eval_distance_matrix_arith(int dist, int arithmetic, const float* queries, uint64_t nq, const float* rows, uint64_t n,
                                       uint64_t d, uint32_t batch, float* out) {
    CAPI_GUARD_BEGIN
    if (!queries || !rows || !out || dist < 0 || dist >= DIST_COUNT) return fail(HNSWGPU_ERR_ARG, "bad argument");
    std::string err;
    return finish(eval_distance_matrix_device(dist, queries, nq, rows, n, d, batch, false, out, err, arithmetic), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// the storage of an eval call's rows (the one place these are checked: the device side converts what it is handed)
static int check_eval_storage(int dist, int storage, const float* rows, uint64_t n, uint64_t d) {
    if (storage != HNSWGPU_STORAGE_F32 && storage != HNSWGPU_STORAGE_F16) return fail(HNSWGPU_ERR_ARG, "unknown storage");
    if (storage == HNSWGPU_STORAGE_F16) {
        if (dist != DIST_L2 && dist != DIST_COSINE && dist != DIST_DOT && dist != DIST_L1)
            return fail(HNSWGPU_ERR_ARG, "HNSWGPU_STORAGE_F16 serves DistL2, DistCosine, DistDot and DistL1 only");
        uint64_t first = 0;
        const uint64_t bad = d ? f16_count_unrepresentable(rows, n * d, &first) : 0;
        if (bad != 0)
            return fail(HNSWGPU_ERR_ARG, std::to_string(bad) + " row elements are not representable as binary16; the first is element " +
                                         std::to_string(first % d) + " of row " + std::to_string(first / d));
    }
    return HNSWGPU_OK;
}
int hnswgpu_eval_distance_matrix_storage(int dist, int storage, const float* queries, uint64_t nq, const float* rows, uint64_t n,
                                         uint64_t d, uint32_t batch, float* out) {
    CAPI_GUARD_BEGIN
    if (!queries || !rows || !out || dist < 0 || dist >= DIST_COUNT) return fail(HNSWGPU_ERR_ARG, "bad argument");
    if (const int rc = check_eval_storage(dist, storage, rows, n, d)) return rc;
    if (!hnswgpu::eval_distance_matrix_storage_device) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::eval_distance_matrix_storage_device(dist, storage, queries, nq, rows, n, d, batch, out, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}
int hnswgpu_eval_distance_matrix_variant(int dist, int storage, int variant, const float* queries, uint64_t nq, const float* rows,
                                         uint64_t n, uint64_t d, uint32_t batch, float* out) {
    CAPI_GUARD_BEGIN
    if (!queries || !rows || !out || dist < 0 || dist >= DIST_COUNT) return fail(HNSWGPU_ERR_ARG, "bad argument");
    // a variant names a row loop some search kernel compiles; a combination none has is refused, never served by the plain routine
    if ((variant & ~(HNSWGPU_EVAL_DEEP | HNSWGPU_EVAL_PIPE | HNSWGPU_EVAL_R128)) != 0)
        return fail(HNSWGPU_ERR_ARG, "unknown variant bits: HNSWGPU_EVAL_DEEP, HNSWGPU_EVAL_PIPE and HNSWGPU_EVAL_R128 are defined");
    if ((variant & HNSWGPU_EVAL_DEEP) != 0 && (variant & HNSWGPU_EVAL_PIPE) != 0)
        return fail(HNSWGPU_ERR_ARG, "HNSWGPU_EVAL_DEEP with HNSWGPU_EVAL_PIPE: no search kernel has both");
    if ((variant & HNSWGPU_EVAL_R128) != 0) {
        if ((variant & HNSWGPU_EVAL_PIPE) != 0) return fail(HNSWGPU_ERR_ARG, "HNSWGPU_EVAL_R128 with HNSWGPU_EVAL_PIPE: no search kernel has both");
        if (dist != DIST_L2 || storage != HNSWGPU_STORAGE_F32 || d < 97 || d > 128)
            return fail(HNSWGPU_ERR_ARG, "HNSWGPU_EVAL_R128 serves DistL2 on HNSWGPU_STORAGE_F32 rows of 97 .. 128 elements only");
    }
    if (const int rc = check_eval_storage(dist, storage, rows, n, d)) return rc;
    if (!hnswgpu::eval_distance_matrix_variant_device) return fail(HNSWGPU_ERR_DEVICE, kNoFilterSetDevice);
    std::string err;
    return finish(hnswgpu::eval_distance_matrix_variant_device(dist, storage, variant, queries, nq, rows, n, d, batch, out, err), err);
    CAPI_GUARD_END(HNSWGPU_ERR_DEVICE)
}

// ---- DataMap (src/datamap.rs): the vectors of a dump by DataId, memory-mapped, without loading the graph
struct hnswgpu_datamap {
    DataMap m;
};
int hnswgpu_datamap_open(const char* dir, const char* basename, hnswgpu_datamap** out) {
    CAPI_GUARD_BEGIN
    if (!dir || !basename || !out) return fail(HNSWGPU_ERR_ARG, "null argument");
    *out = nullptr;
    std::unique_ptr<hnswgpu_datamap> h(new hnswgpu_datamap());
    std::string err;
    int rc = h->m.open(dir, basename, err);
    if (rc != OK) return fail(rc, err);
    *out = h.release();
    return HNSWGPU_OK;
    CAPI_GUARD_END(HNSWGPU_ERR_IO)
}
void hnswgpu_datamap_close(hnswgpu_datamap* m) { delete m; }
const float* hnswgpu_datamap_get_data(const hnswgpu_datamap* m, uint64_t data_id) { return m ? m->m.get_data(data_id) : nullptr; }
uint64_t hnswgpu_datamap_nb_data(const hnswgpu_datamap* m) { return m ? m->m.nb_data() : 0; }
uint64_t hnswgpu_datamap_dimension(const hnswgpu_datamap* m) { return m ? m->m.dimension() : 0; }
const char* hnswgpu_datamap_distname(const hnswgpu_datamap* m) { return m ? m->m.distname().c_str() : ""; }
const char* hnswgpu_datamap_typename(const hnswgpu_datamap* m) { return m ? m->m.type_name().c_str() : ""; }
uint64_t hnswgpu_datamap_ids(const hnswgpu_datamap* m, uint64_t* out, uint64_t cap) {
    if (!m) return 0;
    const auto& ids = m->m.ids_in_file_order();
    for (uint64_t i = 0; i < ids.size() && i < cap && out; ++i) out[i] = ids[i];
    return ids.size();
}

// =========================================================================================
// Reference-compatible f32 symbols (src/libext.rs)
// =========================================================================================
struct HnswIo {
    std::string dir;
    std::string basename;
};
struct HnswApif32 {
    hnswgpu_index* idx = nullptr;
};

const HnswIo* get_hnswio(uint64_t flen, const uint8_t* name) {  // directory is always "." (src/libext.rs:31)
    CAPI_GUARD_BEGIN
    if (!name) return nullptr;
    HnswIo* io = new HnswIo();
    io->dir = ".";
    io->basename.assign(reinterpret_cast<const char*>(name), (size_t)flen);
    return io;
    CAPI_GUARD_END(nullptr)
}
void hnswgpu_free_hnswio(const HnswIo* p) { delete p; }

static const HnswApif32* load_with(HnswIo* io, int dist) {
    CAPI_GUARD_BEGIN
    if (!io) return nullptr;
    hnswgpu_index* idx = nullptr;
    if (hnswgpu_load_dump(io->dir.c_str(), io->basename.c_str(), dist, &idx) != HNSWGPU_OK) return nullptr;  // null on failure (:298-301)
    HnswApif32* api = new HnswApif32();
    api->idx = idx;
    return api;
    CAPI_GUARD_END(nullptr)
}
const HnswApif32* load_hnswdump_f32_DistL1(HnswIo* io) { return load_with(io, HNSWGPU_DIST_L1); }
const HnswApif32* load_hnswdump_f32_DistL2(HnswIo* io) { return load_with(io, HNSWGPU_DIST_L2); }
const HnswApif32* load_hnswdump_f32_DistCosine(HnswIo* io) { return load_with(io, HNSWGPU_DIST_COSINE); }
const HnswApif32* load_hnswdump_f32_DistDot(HnswIo* io) { return load_with(io, HNSWGPU_DIST_DOT); }
const HnswApif32* load_hnswdump_f32_DistJensenShannon(HnswIo* io) { return load_with(io, HNSWGPU_DIST_JENSENSHANNON); }  // :334-339
const HnswApif32* load_hnswdump_f32_DistJeffreys(HnswIo* io) { return load_with(io, HNSWGPU_DIST_JEFFREYS); }            // :340-345

static const HnswApif32* new_api(size_t max_nb_conn, size_t ef_const, size_t namelen, const uint8_t* cdistname,
                                 size_t max_elements, size_t max_layer, bool allow_cosine) {
    CAPI_GUARD_BEGIN
    (void)max_elements;
    if (!cdistname) return nullptr;
    std::string dname(reinterpret_cast<const char*>(cdistname), namelen);
    int dist = dist_from_short_name(dname);
    // init_hnsw_f32 has no "DistCosine" arm in the reference (src/libext.rs:468-523); keep that quirk
    if (dist < 0 || (dist == DIST_COSINE && !allow_cosine)) {
        fail(HNSWGPU_ERR_DISTANCE, "init_hnsw_f32 received unknow distance " + dname);
        return nullptr;
    }
    if (max_nb_conn > 256 || max_nb_conn < 2) {
        fail(HNSWGPU_ERR_ARG, "error max_nb_connection must be less equal than 256");
        return nullptr;
    }
    hnswgpu_index* idx = new hnswgpu_index();
    idx->params.max_nb_connection = max_nb_conn;
    idx->params.ef_construction = ef_const;
    idx->params.max_layer = max_layer;
    idx->params.dist = dist;
    idx->params.nthreads = 0;
    idx->builder.reset(new GraphBuilder(idx->params));
    HnswApif32* api = new HnswApif32();
    api->idx = idx;
    return api;
    CAPI_GUARD_END(nullptr)
}
const HnswApif32* init_hnsw_f32(size_t max_nb_conn, size_t ef_const, size_t namelen, const uint8_t* cdistname) {
    return new_api(max_nb_conn, ef_const, namelen, cdistname, 10000, 16, false);  // Hnsw::new(M, 10000, 16, ef_c, D) (:475)
}
const HnswApif32* new_hnsw_f32(size_t max_nb_conn, size_t ef_const, size_t namelen, const uint8_t* cdistname,
                               size_t max_elements, size_t max_layer) {
    return new_api(max_nb_conn, ef_const, namelen, cdistname, max_elements, max_layer, false);
}
const HnswApif32* init_hnsw_ptrdist_f32(size_t, size_t, hnsw_dist_fn_f32) {
    // src/libext.rs:643-655 builds Hnsw<f32, DistCFFI<f32>> around a host function pointer: nothing the device can call
    fail(HNSWGPU_ERR_DISTANCE, "init_hnsw_ptrdist_f32: a host distance callback cannot run on the device and there is no CPU "
                               "search path; use a named distance (DistL2, DistL1, DistCosine, DistDot, DistHellinger, "
                               "DistJeffreys, DistJensenShannon)");
    return nullptr;
}

// The reference's insert_f32 / parallel_insert_f32 return nothing (:661-723).  They work on every handle, reloaded ones
// included; a failure (dimension mismatch, no device, bad ordinal, ...) leaves the index unchanged and is readable through
// hnswgpu_last_error().
void insert_f32(HnswApif32* api, size_t len, const float* data, size_t id) {
    CAPI_GUARD_BEGIN
    if (!api || !api->idx || !data) { fail(HNSWGPU_ERR_ARG, "insert_f32: null argument"); return; }
    hnswgpu_index* idx = api->idx;
    std::unique_lock<std::shared_mutex> g(idx->mu);
    uint64_t id64 = id;
    (void)insert_points(idx, data, 1, len, &id64, 1);
    CAPI_GUARD_END()
}
void parallel_insert_f32(HnswApif32* api, size_t nb_vec, size_t vec_len, const float** datas, const size_t* ids) {
    CAPI_GUARD_BEGIN
    if (!api || !api->idx || !datas || !ids) { fail(HNSWGPU_ERR_ARG, "parallel_insert_f32: null argument"); return; }
    hnswgpu_index* idx = api->idx;
    std::unique_lock<std::shared_mutex> g(idx->mu);
    std::vector<float> flat(nb_vec * vec_len);  // inputs are copied, like the reference (:700-712)
    std::vector<uint64_t> id64(nb_vec);
    for (size_t i = 0; i < nb_vec; ++i) {
        std::memcpy(flat.data() + i * vec_len, datas[i], vec_len * sizeof(float));
        id64[i] = ids[i];
    }
    (void)insert_points(idx, flat.data(), nb_vec, vec_len, id64.data(), 0);
    CAPI_GUARD_END()
}

static Neighbour_api* make_row(const uint64_t* ids, const float* dists, uint32_t cnt) {
    Neighbour_api* row = cnt ? static_cast<Neighbour_api*>(std::malloc(cnt * sizeof(Neighbour_api))) : nullptr;
    for (uint32_t j = 0; j < cnt; ++j) {
        row[j].id = (size_t)ids[j];
        row[j].d = dists[j];
    }
    return row;
}

const Neighbourhood_api* search_neighbours_f32(const HnswApif32* api, size_t len, const float* data, size_t knbn,
                                               size_t ef_search) {
    CAPI_GUARD_BEGIN
    if (!api || !api->idx || !data || knbn == 0) return nullptr;
    std::vector<uint64_t> ids(knbn);
    std::vector<float> dists(knbn);
    uint32_t cnt = 0;
    if (hnswgpu_search_batch(api->idx, data, 1, len, knbn, ef_search, ids.data(), dists.data(), nullptr, nullptr, &cnt) != HNSWGPU_OK)
        return nullptr;
    Neighbourhood_api* ans = static_cast<Neighbourhood_api*>(std::malloc(sizeof(Neighbourhood_api)));
    ans->nbgh = cnt;
    ans->neighbours = make_row(ids.data(), dists.data(), cnt);
    return ans;
    CAPI_GUARD_END(nullptr)
}

// The answer of parallel_search_neighbours_f32 is ONE allocation: a header, the Vec_api, its nb_vec Neighbourhood_api and every
// Neighbour_api row behind them (the reference leaks 1 + nb_vec vectors per call, src/libext.rs:236-253; a caller that frees
// hands the Vec_api pointer to hnswgpu_free_neighbourhood_vec, which finds the header in front of it).
namespace {
constexpr uint64_t SLAB_MAGIC = 0x486E7377536C6162ull;  // "HnswSlab"
// A slab is ordinary memory, or -- the usual case -- page-locked memory the device addresses (hnswgpu::pinned_alloc): the search
// kernels then write ids, distances and counts straight into the Neighbour_api / Neighbourhood_api records and the call has
// no unpacking pass.  The header remembers which, and the shape (nq, k) whose row pointers the records hold.
struct SlabHeader {
    uint64_t magic;
    uint64_t bytes;
    uint64_t dev;      // page-locked: the address of this header as the allocating device sees it (nonzero); 0: ordinary memory
    uint64_t nq, k;    // the shape the Neighbourhood_api records were last laid out for (0, 0: not yet)
    uint64_t reserved;
};
static_assert(sizeof(SlabHeader) % 16 == 0, "the records behind the header stay 16-byte aligned");
struct FfiAnswer {
    size_t nq, k;
    Vec_api_Neighbourhood* out;
    Neighbourhood_api* lists;
    Neighbour_api* rows;
    SlabHeader* slab;
};
// A caller that frees its answers (hnswgpu_free_neighbourhood_vec) and asks again gets the same memory back: a 10 000 x 10
// answer is a 1.9 MB allocation, which malloc serves with mmap / munmap and the kernel with ~470 fresh page faults per call --
// a tenth of a millisecond on a 1.2 ms search -- and page-locking costs more than that.  A few freed slabs (at most 64 MB) are
// kept for the next call of the same size; at most 256 MB of page-locked slabs are out at any time (answers a caller never
// frees -- the reference leaks them, src/libext.rs:236-253 -- are then served from ordinary memory, with an unpacking pass).
class SlabCache {
public:
    SlabHeader* take(size_t bytes, bool pinned_ok) {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < n_; ++i)
                if (slab_[i]->bytes == bytes && (pinned_ok || slab_[i]->dev == 0)) {
                    SlabHeader* h = slab_[i];
                    slab_[i] = slab_[--n_];
                    held_ -= bytes;
                    h->magic = SLAB_MAGIC;
                    return h;
                }
        }
        SlabHeader* h = nullptr;
        if (pinned_ok) {
            if (pinned_out_.fetch_add(bytes) + bytes <= PINNED_LIMIT) {
                void* dev = nullptr;
                h = static_cast<SlabHeader*>(hnswgpu::pinned_alloc(bytes, &dev));
                if (h) {
                    *h = SlabHeader{SLAB_MAGIC, bytes, (uint64_t)(uintptr_t)dev, 0, 0, 0};
                    return h;
                }
            }
            pinned_out_.fetch_sub(bytes);  // refused by the runtime, or over the limit: ordinary memory
        }
        h = static_cast<SlabHeader*>(std::malloc(bytes));
        if (h) *h = SlabHeader{SLAB_MAGIC, bytes, 0, 0, 0, 0};
        return h;
    }
    void give(SlabHeader* h) {
        const size_t bytes = (size_t)h->bytes;
        h->magic = 0;  // (a second free of the same answer is then at least not taken for a slab)
        {
            std::lock_guard<std::mutex> g(mu_);
            if (n_ < KEEP && held_ + bytes <= (64ull << 20)) {
                slab_[n_++] = h;
                held_ += bytes;
                return;
            }
        }
        if (h->dev != 0) {
            hnswgpu::pinned_free(h);
            pinned_out_.fetch_sub(bytes);
        } else {
            std::free(h);
        }
    }
private:
    static constexpr size_t KEEP = 4;
    static constexpr uint64_t PINNED_LIMIT = 256ull << 20;
    std::mutex mu_;
    SlabHeader* slab_[KEEP] = {};
    size_t n_ = 0, held_ = 0;
    std::atomic<uint64_t> pinned_out_{0};
};
SlabCache& slab_cache() {
    static SlabCache* c = new SlabCache();  // (never destroyed: answers may be freed during static destruction)
    return *c;
}
}  // namespace

const Vec_api_Neighbourhood* parallel_search_neighbours_f32(const HnswApif32* api, size_t nb_vec, int64_t vec_len,
                                                            const float** data, size_t knbn, size_t ef_search) {
    CAPI_GUARD_BEGIN
    if (!api || !api->idx || !data || knbn == 0 || vec_len <= 0) return nullptr;
    hnswgpu_index* idx = api->idx;
    for (size_t i = 0; i < nb_vec; ++i)
        if (!data[i]) { fail(HNSWGPU_ERR_ARG, "parallel_search_neighbours_f32: null row pointer"); return nullptr; }
    FfiAnswer ans{nb_vec, knbn, nullptr, nullptr, nullptr, nullptr};
    // the row pointers are gathered straight into pinned staging memory (the reference copies them into Vec<Vec<f32>>,
    // :218-226); the slab is taken before the search starts.  A page-locked slab is written by the search kernels themselves
    // (sink.direct); an ordinary one is filled out of the pinned answer arena by the threads of the call's pool section
    // (HNSWGPU_FFI_UNPACK=1 forces that path: test hook)
    DeviceIndex::AnswerSink sink{
        [](void* ctx, uint64_t nq, uint64_t k) -> bool {
            FfiAnswer& f = *static_cast<FfiAnswer*>(ctx);
            const size_t bytes = sizeof(SlabHeader) + sizeof(Vec_api_Neighbourhood) + nq * sizeof(Neighbourhood_api) + nq * k * sizeof(Neighbour_api);
            const bool unpack_only = hnswgpu::knobs().ffi_unpack;
            SlabHeader* h = slab_cache().take(bytes, !unpack_only);
            if (!h) return false;
            unsigned char* slab = reinterpret_cast<unsigned char*>(h);
            Vec_api_Neighbourhood* v = reinterpret_cast<Vec_api_Neighbourhood*>(slab + sizeof(SlabHeader));
            f.lists = reinterpret_cast<Neighbourhood_api*>(v + 1);
            f.rows = reinterpret_cast<Neighbour_api*>(f.lists + nq);
            v->len = (int64_t)nq;
            v->ptr = f.lists;
            f.out = v;
            f.slab = h;
            if (h->dev != 0 && (h->nq != nq || h->k != k)) {
                // the records the kernels do not write: every list's row pointer, the high word of its count, the rows' padding
                std::memset(f.lists, 0, bytes - sizeof(SlabHeader) - sizeof(Vec_api_Neighbourhood));
                for (size_t i = 0; i < nq; ++i) f.lists[i].neighbours = f.rows + i * k;
                h->nq = nq;
                h->k = k;
            }
            return true;
        },
        [](void* ctx, const DeviceIndex::HostAnswers& a, uint64_t lo, uint64_t hi) {
            FfiAnswer& f = *static_cast<FfiAnswer*>(ctx);
            for (size_t i = lo; i < hi; ++i) {
                const uint32_t c = a.counts[i];
                Neighbour_api* r = f.rows + i * f.k;
                for (uint32_t j = 0; j < c; ++j) {
                    r[j].id = (size_t)a.ids[i * f.k + j];
                    r[j].d = a.dists[i * f.k + j];
                }
                f.lists[i].nbgh = (int64_t)c;
                f.lists[i].neighbours = r;
            }
        },
        &ans,
        [](void* ctx, DeviceIndex::DirectOut* out) -> bool {
            FfiAnswer& f = *static_cast<FfiAnswer*>(ctx);
            if (!f.slab || f.slab->dev == 0) return false;
            static_assert(sizeof(Neighbour_api) == 16 && sizeof(Neighbourhood_api) == 16 && sizeof(size_t) == 8, "the in-place layout");
            out->allocation = f.slab;
            out->ids = &f.rows[0].id;
            out->dists = &f.rows[0].d;
            out->counts = &f.lists[0].nbgh;
            out->layout = hnswgpu::OutLayout{16, 16, 16};
            return true;
        }};
    std::string err;
    int rc;
    {
        std::shared_lock<std::shared_mutex> sl(idx->mu);
        const bool empty = idx->builder ? idx->builder->nb_point() == 0 : (!idx->flat || idx->flat->n == 0);
        if (empty || nb_vec == 0) {  // empty index => every answer is empty (src/hnsw.rs:1498-1503)
            std::vector<uint32_t> zero(std::max<size_t>(1, nb_vec), 0u);
            DeviceIndex::HostAnswers a{};
            a.counts = zero.data();
            if (!sink.begin(&ans, nb_vec, knbn)) { fail(HNSWGPU_ERR_ARG, "out of memory"); return nullptr; }
            sink.rows(&ans, a, 0, nb_vec);
            return ans.out;
        }
        DeviceIndex* dev = nullptr;
        rc = primary_replica(idx, sl, &dev);
        if (rc != HNSWGPU_OK) return nullptr;
        rc = dev->search_host_staged(nullptr, data, nb_vec, (uint64_t)vec_len, knbn, ef_search, nullptr, 0, false, false, sink, nullptr, err);
    }
    if (rc != OK) {
        if (ans.out) hnswgpu_free_neighbourhood_vec(ans.out);  // (taken before the search started)
        fail(rc, err);
        return nullptr;
    }
    if (!ans.out) fail(HNSWGPU_ERR_ARG, "out of memory");
    return ans.out;
    CAPI_GUARD_END(nullptr)
}

void hnswgpu_free_neighbourhood(const Neighbourhood_api* p) {
    if (!p) return;
    std::free(const_cast<Neighbour_api*>(p->neighbours));
    std::free(const_cast<Neighbourhood_api*>(p));
}
// Every Vec_api this library hands out is the head of ONE slab (header | Vec_api | Neighbourhood_api[] | Neighbour_api[]): the
// rows are interior pointers and must never be freed one by one; the whole answer is released here, and only here.
void hnswgpu_free_neighbourhood_vec(const Vec_api_Neighbourhood* p) {
    if (!p) return;
    SlabHeader* h = reinterpret_cast<SlabHeader*>(reinterpret_cast<unsigned char*>(const_cast<Vec_api_Neighbourhood*>(p)) - sizeof(SlabHeader));
    if (h->magic != SLAB_MAGIC) return;  // not an answer of this library, or freed already
    slab_cache().give(h);
}

int64_t file_dump_f32(const HnswApif32* api, size_t namelen, const uint8_t* filename) {
    CAPI_GUARD_BEGIN
    if (!api || !api->idx || !filename) return -1;
    std::string base(reinterpret_cast<const char*>(filename), namelen);
    return hnswgpu_file_dump(api->idx, ".", base.c_str()) == HNSWGPU_OK ? 1 : -1;  // 1 / -1 (:269-272)
    CAPI_GUARD_END(-1)
}

void drop_hnsw_f32(const HnswApif32* p) {
    if (!p) return;
    hnswgpu_free_index(p->idx);
    delete p;
}

const DescriptionFFI* load_hnsw_description(size_t flen, const uint8_t* name) {
    CAPI_GUARD_BEGIN
    if (!name) return nullptr;
    std::string path(reinterpret_cast<const char*>(name), flen);
    DumpDescription d;
    std::string err;
    if (load_description_file(path, d, err) != OK) {
        fail(HNSWGPU_ERR_IO, err);
        return nullptr;
    }
    DescriptionFFI* f = static_cast<DescriptionFFI*>(std::calloc(1, sizeof(DescriptionFFI)));
    f->dumpmode = 1;  // the reference always reports 1 and never fills nb_point (src/libext.rs:1198-1206)
    f->max_nb_connection = d.max_nb_connection;
    f->nb_layer = d.nb_layer;
    f->ef = d.ef;
    f->nb_point = 0;
    f->data_dimension = d.dimension;
    char* dn = static_cast<char*>(std::malloc(d.distname.size() + 1));
    std::memcpy(dn, d.distname.c_str(), d.distname.size() + 1);
    f->distname_len = d.distname.size();
    f->distname = reinterpret_cast<const uint8_t*>(dn);
    char* tn = static_cast<char*>(std::malloc(d.t_name.size() + 1));
    std::memcpy(tn, d.t_name.c_str(), d.t_name.size() + 1);
    f->t_name_len = d.t_name.size();
    f->t_name = reinterpret_cast<const uint8_t*>(tn);
    return f;
    CAPI_GUARD_END(nullptr)
}
void hnswgpu_free_description(const DescriptionFFI* p) {
    if (!p) return;
    std::free(const_cast<uint8_t*>(p->distname));
    std::free(const_cast<uint8_t*>(p->t_name));
    std::free(const_cast<DescriptionFFI*>(p));
}

void init_rust_log(void) {}

hnswgpu_index* hnswgpu_from_api(const HnswApif32* p) { return p ? p->idx : nullptr; }

}  // extern "C"
