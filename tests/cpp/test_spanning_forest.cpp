// Hnsw::knn_graph_spanning_forest and csr_spanning_forest of include/hnsw_rs.hpp: "cpu" checks what needs no device (the empty
// index, the refusals, the "no device" answer); "gpu" checks the answer's own invariants on a small built index against
// knn_graph_components, and the forests of hand-made graphs (tests/test_gpu_spanning_forest.py checks the values against the model
// through the C ABI).
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

static uint32_t find(std::vector<uint32_t>& p, uint32_t v) {
    while (p[v] != v) v = p[v] = p[p[v]];
    return v;
}

// a < b < n, ascending by (weight, a, b) (no NaN or -0 here: plain comparisons), no cycle; returns the number of trees, 0 if malformed
static size_t trees_of(const hnsw_rs::SpanningForest& f, size_t n) {
    if (f.b.size() != f.a.size() || f.weights.size() != f.a.size() || f.n_edges() >= n) return 0;
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    for (size_t e = 0; e < f.n_edges(); ++e) {
        if (!(f.a[e] < f.b[e] && f.b[e] < n)) return 0;
        if (e > 0) {
            const bool up = f.weights[e - 1] < f.weights[e] ||
                            (f.weights[e - 1] == f.weights[e] && (f.a[e - 1] < f.a[e] || (f.a[e - 1] == f.a[e] && f.b[e - 1] < f.b[e])));
            if (!up) return 0;
        }
        const uint32_t ra = find(p, f.a[e]), rb = find(p, f.b[e]);
        if (ra == rb) return 0;  // a cycle
        p[ra > rb ? ra : rb] = ra > rb ? rb : ra;
    }
    return n - f.n_edges();
}

int main(int argc, char** argv) {
    using namespace hnsw_rs;
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    Hnsw<float, DistL2> h(8, 300, 16, 32);
    const auto none = h.knn_graph_spanning_forest(3);
    CHECK(none.a.empty() && none.b.empty() && none.weights.empty() && none.n_edges() == 0);
    for (const auto& offs : {std::vector<uint64_t>{0}, std::vector<uint64_t>{0, 0}}) {
        const auto no_edge = csr_spanning_forest(offs, {});
        CHECK(no_edge.n_edges() == 0 && no_edge.b.empty() && no_edge.weights.empty());
    }
    const size_t n = 300, d = 8;
    std::vector<float> x(n * d);
    uint32_t s = 12345;
    for (auto& v : x) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 16777216.f; }
    h.parallel_insert(x, d, {}, 1);
    try { h.knn_graph_spanning_forest(0); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { h.knn_graph_spanning_forest(5000); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }   // exact: knbn <= 4096
    try { h.knn_graph_spanning_forest(3, 0, false, 4); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }  // core_k > knbn
    const std::vector<uint64_t> offsets{0, 2, 3, 3, 5};            // the triangle 0 - 1 - 2; 3 with a self-loop, joined to 1
    const std::vector<uint32_t> cols{1, 2, 2, 3, 1};
    const std::vector<float> dists{0.25f, 0.75f, 0.5f, 0.f, 1.f};
    try { csr_spanning_forest(offsets, {1, 2, 2, 4, 1}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { csr_spanning_forest({0, 2, 1, 3, 5}, cols); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { csr_spanning_forest({}, cols); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    const std::vector<float> few{0.25f};
    try { csr_spanning_forest(offsets, cols, &few); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    if (!gpu) {
        if (hnswgpu_device_count() == 0) {
            try { h.knn_graph_spanning_forest(3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
            try { csr_spanning_forest(offsets, cols); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
        }
        std::printf("cpu mode OK\n");
        return 0;
    }
    auto f = csr_spanning_forest(offsets, cols, &dists);          // 0 - 1 (0.25), 1 - 2 (0.5), 1 - 3 (1); 0 - 2 (0.75) closes a cycle
    CHECK(f.a == std::vector<uint32_t>({0, 1, 1}) && f.b == std::vector<uint32_t>({1, 2, 3}) && f.weights == std::vector<float>({0.25f, 0.5f, 1.f}));
    f = csr_spanning_forest(offsets, cols);                       // all weights 0: by (lo, hi)
    CHECK(f.a == std::vector<uint32_t>({0, 0, 1}) && f.b == std::vector<uint32_t>({1, 2, 3}) && f.weights == std::vector<float>({0.f, 0.f, 0.f}));
    for (size_t ef : {(size_t)0, (size_t)32}) {
        for (bool mutual : {false, true}) {
            const auto c = h.knn_graph_components(4, ef, mutual);
            for (size_t core_k : {(size_t)0, (size_t)2, (size_t)4}) {
                const auto t = h.knn_graph_spanning_forest(4, ef, mutual, core_k);
                CHECK(trees_of(t, n) == c.n_components());        // n - c edges, whatever the weights
                for (size_t e = 0; e < t.n_edges(); ++e) {
                    CHECK(c.labels[t.a[e]] == c.labels[t.b[e]]);   // a forest edge stays inside a component
                    CHECK(t.weights[e] > 0.f);                    // distinct points
                }
            }
        }
    }
    std::printf("gpu mode OK\n");
    return 0;
}
