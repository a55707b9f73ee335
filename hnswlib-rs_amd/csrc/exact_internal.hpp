// exact_internal.hpp -- the host side that exact_knn.hip (exhaustive k-NN, the filter set), exact_range.hip (exact range search) and
// knn_graph.hip (the queries by stored point) share, and the one declaration of exact_device for them and for cluster_predict.hip:
// the replica's state and its scratch pool, the plan of a call's slabs, an optional filter's way to the device, the rows of a k-NN
// answer and their staging.  The device pieces of the two slab kernels are in exact_tile.hpp.  Private, like graph_internal.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "hip_host.hpp"
#include "search_device.hpp"

namespace hnswgpu {

constexpr int TQ = 16;  // queries per tile: one wavefront holds an accumulator each per lane
constexpr uint32_t MIN_SLAB_ROWS = 256;
constexpr uint32_t MAX_SLABS = 64;  // the k-NN merge keeps one slab per lane

// What a replica keeps for these units (DeviceIndex::extension): the DataId ranks, and scratch blocks that calls take turns with
struct ExactState {
    int device = -1;
    void* d_rank = nullptr;   // [n] u32: position of flat id f in ascending (DataId, flat id) order
    void* d_order = nullptr;  // [n] u32: its inverse
    std::mutex mu;
    std::vector<std::pair<void*, uint64_t>> pool;  // free scratch blocks {address, bytes}
    ~ExactState() {
        DeviceGuard on(device);
        if (d_rank) (void)hipFree(d_rank);
        if (d_order) (void)hipFree(d_order);
        for (auto& b : pool) (void)hipFree(b.first);
    }
    const uint32_t* rank() const { return static_cast<const uint32_t*>(d_rank); }
    const uint32_t* order() const { return static_cast<const uint32_t*>(d_order); }
};
// defined in exact_knn.hip: the replica's state, made on first use (once per replica, on the host) -- or nullptr and `err` set, the
// upload's own message or "<what>: no device state": the caller returns ERR_DEVICE.  The device of `dev` is current.
std::shared_ptr<ExactState> replica_state(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const char* what, std::string& err);

// A call's block from the state's pool, back there when the call ends; alloc_layout (hip_host.hpp) sizes and divides it
struct ScratchLease {
    ExactState* st;
    void* p = nullptr;
    uint64_t bytes = 0;
    explicit ScratchLease(ExactState* s) : st(s) {}
    hipError_t alloc(uint64_t need) {
        {
            std::lock_guard<std::mutex> g(st->mu);
            if (!st->pool.empty()) { p = st->pool.back().first; bytes = st->pool.back().second; st->pool.pop_back(); }
        }
        // (HNSWGPU_POISON_SCRATCH: the block a call takes, reused or new, is nobody's over its whole size)
        if (bytes < need) {
            if (p) (void)hipFree(p);
            p = nullptr, bytes = 0;
            if (const hipError_t e = hipMalloc(&p, need); e != hipSuccess) { p = nullptr; return e; }
            bytes = need;
        }
        return poison_scratch(p, bytes);
    }
    ~ScratchLease() {
        if (!p) return;
        std::lock_guard<std::mutex> g(st->mu);
        st->pool.emplace_back(p, bytes);
    }
};

// How a call of nq queries of d elements against n rows is cut: tiles of TQ queries, slabs of rows -- one wavefront per (tile, slab)
struct SlabPlan {
    uint64_t n, nchunk, tiles_total, words;  // rows; float4 chunks of a row that hold data; tiles of the batch; words of one bitmap
    uint64_t slabs = 0, slab_rows = 0;       // by cut()
    SlabPlan(uint64_t n_, uint64_t d, uint64_t nq) : n(n_), nchunk((d + 3) / 4), tiles_total((nq + TQ - 1) / TQ), words((n_ + 31) / 32) {}
    // enough (tile, slab) wavefronts to fill the device, never more than `most` slabs.  False: most == 0.
    bool cut(uint64_t most = MAX_SLABS) {
        slabs = std::min<uint64_t>({MAX_SLABS, (8192 + tiles_total - 1) / tiles_total, most});
        if (slabs == 0) return false;
        slab_rows = std::max<uint64_t>(MIN_SLAB_ROWS, round_up((n + slabs - 1) / slabs, 64));
        slabs = (n + slab_rows - 1) / slab_rows;
        return true;
    }
    // a tile's queries and their norms, each padded: per-tile arrays lie tile behind tile
    uint64_t qt_bytes() const { return round_up(nchunk * TQ * 16, 256); }
    uint64_t qnorm_bytes() const { return round_up(TQ * 8, 256); }
    void tiles(ScratchLayout& lay, uint64_t chunk_tiles, float*& d_qt, double*& d_qnorm) const {
        lay.bytes(d_qt, chunk_tiles * qt_bytes());
        lay.bytes(d_qnorm, chunk_tiles * qnorm_bytes());
    }
};
// defined in exact_knn.hip, which holds the kernel: cq queries (row qlist[i] of src, nullptr: row i) zero padded into n_slots slots of
// the tiles qt, their squared norms into qnorm; tword != nullptr (filter set): the first word of each slot's bitmap,
// slot_of[row] * words.  On `stream`, nobody waits.
hipError_t exact_prep_queries(hipStream_t stream, const float* d_src, uint64_t cq, uint64_t d, const SlabPlan& plan, uint32_t n_slots, float* d_qt,
                              double* d_qnorm, const uint32_t* qlist = nullptr, const uint32_t* slot_of = nullptr, uint32_t* tword = nullptr);
// defined in exact_knn.hip too: the same tiles from the index's own rows -- slot i holds the stored point of flat id d_flat[i], its
// bits those of the point's vector brought as a query, and self_rank[i] that point's DataId rank (its POSITION; the slots behind
// the last: 0xFFFFFFFF).  For the exact graph and for dbscan.hip.  On `stream`, nobody waits.
hipError_t exact_prep_rows(hipStream_t stream, const DeviceIndexView& ix, const uint32_t* d_flat, const uint32_t* d_rank, uint64_t cq, const SlabPlan& plan,
                           uint32_t n_slots, float* d_qt, double* d_qnorm, uint32_t* d_self_rank);

// The optional filter of a call with host buffers goes to the device once.  A filter that is empty still is a filter: a non-null
// pointer that is never dereferenced.
struct FilterUpload {
    DevMem mem;
    const uint64_t* d_allowed = nullptr;  // nullptr: the call has no filter
    int put(const uint64_t* allowed, uint64_t n_allowed, std::string& err) {
        if (allowed == nullptr) return OK;
        HIP_TRY(mem.alloc(std::max<uint64_t>(1, n_allowed) * sizeof(uint64_t)));
        if (n_allowed != 0) HIP_TRY(hipMemcpy(mem.p, allowed, n_allowed * sizeof(uint64_t), hipMemcpyHostToDevice));
        d_allowed = static_cast<const uint64_t*>(mem.p);
        return OK;
    }
};

struct GraphRows {  // answers, row major
    uint64_t* ids;
    float* dists;
    uint8_t* layer;    // the caller's may be nullptr; the staged ones never are
    int32_t* rank;
    uint32_t* counts;  // nullptr: answers without rows (a range search's)
};
// rows [c0, c0 + ..) of k-wide answers
inline GraphRows rows_at(const GraphRows& r, uint64_t c0, uint64_t k) {
    return GraphRows{r.ids + c0 * k, r.dists + c0 * k, r.layer ? r.layer + c0 * k : nullptr, r.rank ? r.rank + c0 * k : nullptr,
                     r.counts ? r.counts + c0 : nullptr};
}
// The first `slots` answers and `rows` counts of staged device rows out to host rows (what dst lacks is skipped); waits for the
// stream: the staging area is the next chunk's
inline int copy_rows_out(const GraphRows& dst, const GraphRows& src, uint64_t slots, uint64_t rows, hipStream_t stream, std::string& err) {
    return copy_out({{dst.ids, src.ids, slots * 8}, {dst.dists, src.dists, slots * 4}, {dst.rank, src.rank, slots * 4}, {dst.layer, src.layer, slots},
                     {dst.counts, src.counts, rows * 4}},
                    true, stream, err);
}
// The one device staging for a chunk of k-NN answers, k slots a row: ids, dists, rank, counts and layer in one block
struct AnswerStage {
    DevMem mem;
    GraphRows rows{};
    int alloc(const char* what, uint64_t chunk, uint64_t k, std::string& err) {
        ScratchLayout lay;
        lay.arrays(chunk * k, rows.ids, rows.dists, rows.rank);
        lay.array(rows.counts, chunk);
        lay.array(rows.layer, chunk * k);
        return alloc_layout(what, mem, lay, err);
    }
};

// One exact k-NN call, every pointer device memory: nq queries -- d_queries, or (k-NN graph; no set) the stored points of flat ids
// d_self, which are never their own answer --, k, one filter for the batch (d_allowed != nullptr, even when it is empty) or a set of
// filters with each query naming its own (filter_of), or neither, and the five outputs.
struct ExactCall {
    const float* d_queries = nullptr;  // nq x d
    const uint32_t* d_self = nullptr;  // [nq]
    uint64_t nq = 0, d = 0, k = 0;
    const uint64_t* d_allowed = nullptr;
    uint64_t n_allowed = 0;
    const FilterSet* set = nullptr;
    GraphRows out{};  // layer and rank may be nullptr
};
// defined in exact_knn.hip; waits for `stream` before it returns
int exact_device(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const ExactCall& c, hipStream_t stream, std::string& err);

}  // namespace hnswgpu
