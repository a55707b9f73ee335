// graph_internal.hpp -- what exact_knn.hip shares with symmetric_graph.hip, the unit that turns the k-NN graph of the indexed points
// into an undirected one: the order of the exact k-NN key, and the DataId ranks a replica keeps on the device.  Private, like
// capi_index.hpp; the graph calls themselves (graph_search, exact_graph) are declared there.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "search_device.hpp"

namespace hnswgpu {

#if defined(__HIPCC__)
// f32 -> u32 whose unsigned order is the order of the values, every NaN behind everything (distances are >= 0: then this is the
// bit pattern with the top bit set; the other cases keep the order total whatever a distance returns)
__device__ __forceinline__ uint32_t dist_order_bits(float v) {
    uint32_t b = __float_as_uint(v);
    if (v != v) return 0xFFFFFFFFu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
#endif

// The two permutations behind "position": rank[f] = position of flat id f in the ascending (DataId, dump order) order, order = its
// inverse.  Device memory of the replica's own state (made on first use); `keep` holds that state alive.
struct GraphOrder {
    std::shared_ptr<void> keep;
    const uint32_t* d_rank = nullptr;
    const uint32_t* d_order = nullptr;
};
// defined in exact_knn.hip: OK, or ERR_DEVICE with `err` set
int graph_order(const DeviceIndex& dev, const std::vector<uint64_t>& origin_id, GraphOrder& out, std::string& err);

}  // namespace hnswgpu
