// graph_internal.hpp -- what the exact units (exact_knn.hip, knn_graph.hip) share with symmetric_graph.hip, the unit that turns the k-NN graph of the indexed points
// into an undirected one, and what that unit shares with graph_components.hip, which labels the graph's connected components, and
// with spanning_forest.hip, which takes the graph's minimum spanning forest: the
// order of the exact k-NN key, the DataId ranks a replica keeps on the device, the directed graph D staged on the device, and D's
// edge records sorted.  Private, like capi_index.hpp; the graph calls themselves (graph_search, exact_graph) are declared there.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "dist_order.hpp"  // dist_order_bits: the order of the exact k-NN key and of every weight
#include "hip_host.hpp"
#include "search_device.hpp"

namespace hnswgpu {

#if defined(__HIPCC__)
// An edge record's key: the row above bit 33, the col in bits 1 .. 32, the flag in bit 0 (rows and cols are below 2^30: n k <= 2^30)
constexpr uint64_t FLAG_REV = 1ull;
__host__ __device__ inline uint64_t rec_key(uint32_t row, uint32_t col, uint64_t flag) { return ((uint64_t)row << 33) | ((uint64_t)col << 1) | flag; }
#endif

// The two permutations behind "position": rank[f] = position of flat id f in the ascending (DataId, dump order) order, order = its
// inverse.  Device memory of the replica's own state (made on first use); `keep` holds that state alive.
struct GraphOrder {
    std::shared_ptr<void> keep;
    const uint32_t* d_rank = nullptr;
    const uint32_t* d_order = nullptr;
};
// defined in knn_graph.hip: OK, or ERR_DEVICE with `err` set
int graph_order(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, GraphOrder& out, std::string& err);

// defined in spanning_forest.hip, which holds the kernel: core[v] = the stored bits of slot min(core_k, counts[v]) - 1 of row v of n
// rows of k slots (a StagedGraph's dists and counts), +0 for an empty row; one thread per row, numbered in 64 bits.  On `stream`,
// nobody waits.
int core_of_rows(const float* d_dists, const uint32_t* d_counts, uint64_t k, uint64_t core_k, uint64_t n, uint32_t* d_core, void* stream, std::string& err);

// D, staged: the graph path's own answer for every point (exact_graph for ef == 0, else graph_search), row i the point at position
// i, n rows of k slots, counts[i] of them used.  One allocation of 17 n k + 4 n bytes (and padding); a slot's neighbour is the p_id
// (layer, rank).
struct StagedGraph {
    DevMem mem;
    float* dists = nullptr;      // [n k]
    int32_t* rank = nullptr;     // [n k]
    uint32_t* counts = nullptr;  // [n]
    uint8_t* layer = nullptr;    // [n k]
};
// D's 2 n k edge records -- per slot i -> j the forward record (i, j, FWD) and the reverse record (j, i, REV), both carrying the
// slot's distance bits; a slot behind counts[i] gives two records of row n -- sorted by key: by row, then col, FWD before REV.  The
// sorted records are keys_b / vals_b; keys_a (records * 8 + 256 bytes) and vals_a are free for the caller.
struct SortedRecords {
    DevMem keys_a, keys_b, vals_a, vals_b;
    uint64_t records = 0;
};
// defined in symmetric_graph.hip, on `stream`; the device of `dev` is current.  OK, or the graph call's own status with `err` set.
// sorted_edge_records waits for the stream and has released D when it returns; sorted_edge_records_keeping leaves D in `d` for a
// caller that reads it afterwards (spanning_forest.hip: the core distances).
int stage_directed_graph(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, uint64_t k, uint64_t ef, void* stream, StagedGraph& out,
                         std::string& err);
int sorted_edge_records(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphOrder& ord, uint64_t k, uint64_t ef, void* stream,
                        SortedRecords& out, std::string& err);
int sorted_edge_records_keeping(DeviceIndex& dev, const std::vector<uint64_t>& origin_id, const GraphOrder& ord, uint64_t k, uint64_t ef, void* stream,
                                SortedRecords& out, StagedGraph& d, std::string& err);

}  // namespace hnswgpu
