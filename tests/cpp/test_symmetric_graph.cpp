// Hnsw::symmetric_knn_graph of include/hnsw_rs.hpp: "cpu" checks what needs no device (the empty index, the refusals, the "no device"
// answer); "gpu" checks the CSR answer's own invariants on a small built index (tests/test_gpu_symmetric_graph.py checks the values
// against the model through the C ABI).
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "hnsw_rs.hpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

int main(int argc, char** argv) {
    using namespace hnsw_rs;
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    Hnsw<float, DistL2> h(8, 300, 16, 32);
    const auto none = h.symmetric_knn_graph(3);
    CHECK(none.offsets.size() == 1 && none.offsets[0] == 0 && none.pos.empty() && none.neighbours.empty());
    const size_t n = 300, d = 8;
    std::vector<float> x(n * d);
    uint32_t s = 12345;
    for (auto& v : x) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 16777216.f; }
    h.parallel_insert(x, d, {}, 1);
    try { h.symmetric_knn_graph(0); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { h.symmetric_knn_graph(5000); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }   // exact: knbn <= 4096
    if (!gpu) {
        if (hnswgpu_device_count() == 0) {
            try { h.symmetric_knn_graph(3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
        }
        std::printf("cpu mode OK\n");
        return 0;
    }
    for (size_t ef : {(size_t)0, (size_t)32}) {
        const auto u = h.symmetric_knn_graph(4, ef, false), m = h.symmetric_knn_graph(4, ef, true);
        for (const auto* g : {&u, &m}) {
            CHECK(g->offsets.size() == n + 1 && g->offsets[0] == 0 && g->offsets[n] == g->pos.size() && g->pos.size() == g->neighbours.size());
            std::set<std::pair<uint32_t, uint32_t>> edges;
            for (size_t i = 0; i < n; ++i) {
                CHECK(g->offsets[i] <= g->offsets[i + 1]);
                for (uint64_t e = g->offsets[i]; e < g->offsets[i + 1]; ++e) {
                    CHECK(g->pos[e] < n && g->pos[e] != i && g->neighbours[e].d_id == g->pos[e]);   // ids 0 .. n-1: position = id
                    CHECK(e == g->offsets[i] || g->neighbours[e - 1].distance <= g->neighbours[e].distance);
                    CHECK(edges.insert({(uint32_t)i, g->pos[e]}).second);
                }
            }
            for (const auto& e : edges) CHECK(edges.count({e.second, e.first}) == 1);
        }
        CHECK(u.pos.size() + m.pos.size() <= 2 * n * 4 && m.pos.size() < u.pos.size());
        for (size_t i = 0; i < n; ++i) CHECK(u.offsets[i + 1] - u.offsets[i] >= 4 && m.offsets[i + 1] - m.offsets[i] <= 4);
    }
    std::printf("gpu mode OK\n");
    return 0;
}
