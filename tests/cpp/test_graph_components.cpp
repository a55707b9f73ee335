// Hnsw::knn_graph_components and csr_components of include/hnsw_rs.hpp: "cpu" checks what needs no device (the empty index, the
// refusals, the "no device" answer); "gpu" checks the answer's own invariants on a small built index and the components of
// hand-made graphs (tests/test_gpu_graph_components.py checks the values against the model through the C ABI).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "hnsw_rs.hpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

// labels 0 .. c - 1, first occurrences ascending, sizes the labels' counts
static bool well_formed(const hnsw_rs::Components& c, size_t n) {
    if (c.labels.size() != n) return false;
    std::vector<uint32_t> seen(c.n_components(), 0);
    uint32_t next = 0;
    for (uint32_t l : c.labels) {
        if (l > next || l >= c.n_components()) return false;
        if (l == next) ++next;
        ++seen[l];
    }
    return next == c.n_components() && seen == c.sizes;
}

int main(int argc, char** argv) {
    using namespace hnsw_rs;
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    Hnsw<float, DistL2> h(8, 300, 16, 32);
    const auto none = h.knn_graph_components(3);
    CHECK(none.labels.empty() && none.sizes.empty() && none.n_components() == 0);
    const auto no_vertex = csr_components({0}, {});
    CHECK(no_vertex.labels.empty() && no_vertex.n_components() == 0);
    const size_t n = 300, d = 8;
    std::vector<float> x(n * d);
    uint32_t s = 12345;
    for (auto& v : x) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 16777216.f; }
    h.parallel_insert(x, d, {}, 1);
    const float nan = std::numeric_limits<float>::quiet_NaN(), half = 0.5f;
    try { h.knn_graph_components(0); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { h.knn_graph_components(5000); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }   // exact: knbn <= 4096
    try { h.knn_graph_components(3, 0, false, &nan); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    const std::vector<uint64_t> offsets{0, 1, 2, 2, 3};            // 0 - 1 - 2, 3 alone with a self-loop
    const std::vector<uint32_t> cols{1, 2, 3};
    const std::vector<float> dists{0.25f, 0.75f, 0.f};
    try { csr_components(offsets, {1, 4, 3}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { csr_components({0, 2, 1, 2, 3}, cols); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { csr_components({}, cols); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { csr_components(offsets, cols, nullptr, &half); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { csr_components(offsets, cols, &dists, &nan); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    if (!gpu) {
        if (hnswgpu_device_count() == 0) {
            try { h.knn_graph_components(3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
            try { csr_components(offsets, cols); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
        }
        std::printf("cpu mode OK\n");
        return 0;
    }
    auto c = csr_components(offsets, cols);
    CHECK(c.labels == std::vector<uint32_t>({0, 0, 0, 1}) && c.sizes == std::vector<uint32_t>({3, 1}));
    c = csr_components(offsets, cols, &dists, &half);              // 1 - 2 is cut
    CHECK(c.labels == std::vector<uint32_t>({0, 0, 1, 2}) && c.sizes == std::vector<uint32_t>({2, 1, 1}));
    for (size_t ef : {(size_t)0, (size_t)32}) {
        const auto u = h.knn_graph_components(4, ef, false), m = h.knn_graph_components(4, ef, true);
        CHECK(well_formed(u, n) && well_formed(m, n));
        CHECK(u.n_components() <= m.n_components());              // a mutual pair is a union pair
        for (size_t i = 0; i < n; ++i)
            for (size_t j = i + 1; j < n; ++j) CHECK(m.labels[i] != m.labels[j] || u.labels[i] == u.labels[j]);
        const float zero = 0.f, inf = std::numeric_limits<float>::infinity();
        const auto apart = h.knn_graph_components(4, ef, false, &zero);   // distinct points: no distance is 0
        CHECK(well_formed(apart, n) && apart.n_components() == n);
        const auto all = h.knn_graph_components(4, ef, false, &inf);
        CHECK(all.labels == u.labels && all.sizes == u.sizes);
    }
    std::printf("gpu mode OK\n");
    return 0;
}
