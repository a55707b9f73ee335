// forest_dendrogram and Hnsw::knn_graph_dendrogram of include/hnsw_rs.hpp: "cpu" checks what needs no device (no edge, the empty
// index, the refusals, the "no device" answer); "gpu" checks hand-made forests against rows written out here, and on a small built
// index the answer against a sequential union-find over knn_graph_spanning_forest's own edges (tests/test_gpu_dendrogram.py checks
// the values against the model through the C ABI).
#include <cstdio>
#include <cstring>
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

// the dendrogram of the forest's edges by the sequential union-find: true iff d says the same
static bool same_as_sequential(const hnsw_rs::Dendrogram& d, const hnsw_rs::SpanningForest& f, size_t n) {
    const size_t m = f.n_edges();
    if (d.n_edges() != m || d.right.size() != m || d.sizes.size() != m || d.n_vertices != n) return false;
    std::vector<uint32_t> p(n), size(n, 1u);
    std::vector<int64_t> last(n, -1);
    std::iota(p.begin(), p.end(), 0u);
    for (size_t e = 0; e < m; ++e) {
        const uint32_t ra = find(p, f.a[e]), rb = find(p, f.b[e]);
        if (ra == rb) return false;
        const uint32_t left = last[ra] < 0 ? f.a[e] : (uint32_t)(n + last[ra]), right = last[rb] < 0 ? f.b[e] : (uint32_t)(n + last[rb]);
        const uint32_t lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        p[hi] = lo;
        size[lo] += size[hi];
        last[lo] = (int64_t)e;
        if (d.left[e] != left || d.right[e] != right || d.sizes[e] != size[lo]) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    using namespace hnsw_rs;
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    Hnsw<float, DistL2> h(8, 300, 16, 32);
    const auto none = h.knn_graph_dendrogram(3);
    CHECK(none.n_edges() == 0 && none.right.empty() && none.sizes.empty() && none.forest.n_edges() == 0 && none.roots().empty());
    const auto no_edge = forest_dendrogram(3, {}, {});
    CHECK(no_edge.n_edges() == 0 && no_edge.n_vertices == 3 && no_edge.roots() == std::vector<uint32_t>({0, 1, 2}));
    const size_t n = 300, d = 8;
    std::vector<float> x(n * d);
    uint32_t s = 12345;
    for (auto& v : x) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 16777216.f; }
    h.parallel_insert(x, d, {}, 1);
    try { h.knn_graph_dendrogram(0); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { h.knn_graph_dendrogram(5000); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }   // exact: knbn <= 4096
    try { h.knn_graph_dendrogram(3, 0, false, 4); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }  // core_k > knbn
    try { forest_dendrogram(4, {0, 1}, {1}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { forest_dendrogram(4, {0, 4}, {1, 2}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }      // an end at n
    try { forest_dendrogram(4, {0, 2}, {1, 2}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }      // a self-loop
    try { forest_dendrogram(3, {0, 1, 2}, {1, 2, 0}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }  // too many
    if (!gpu) {
        if (hnswgpu_device_count() == 0) {
            try { h.knn_graph_dendrogram(3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
            try { forest_dendrogram(4, {0, 3, 1}, {1, 2, 2}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
        }
        std::printf("cpu mode OK\n");
        return 0;
    }
    auto t = forest_dendrogram(8, {0, 3, 1, 6, 4}, {1, 2, 2, 5, 0});    // 0 - 1, 3 - 2, the two pairs joined, 6 - 5 apart, 4 to the four
    CHECK(t.left == std::vector<uint32_t>({0, 3, 8, 6, 4}) && t.right == std::vector<uint32_t>({1, 2, 9, 5, 10}));
    CHECK(t.sizes == std::vector<uint32_t>({2, 2, 4, 2, 5}) && t.roots() == std::vector<uint32_t>({7, 11, 12}) && t.forest.n_edges() == 0);
    t = forest_dendrogram(5, {0, 1, 2, 3}, {1, 2, 3, 4});               // a chain from one end
    CHECK(t.left == std::vector<uint32_t>({0, 5, 6, 7}) && t.right == std::vector<uint32_t>({1, 2, 3, 4}) && t.sizes == std::vector<uint32_t>({2, 3, 4, 5}));
    try { forest_dendrogram(4, {0, 1, 2}, {1, 2, 0}); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }  // a triangle
    for (size_t ef : {(size_t)0, (size_t)32}) {
        for (bool mutual : {false, true}) {
            const auto c = h.knn_graph_components(4, ef, mutual);
            for (size_t core_k : {(size_t)0, (size_t)2}) {
                const auto f = h.knn_graph_spanning_forest(4, ef, mutual, core_k);
                const auto g = h.knn_graph_dendrogram(4, ef, mutual, core_k);
                CHECK(g.forest.a == f.a && g.forest.b == f.b);
                CHECK(std::memcmp(g.forest.weights.data(), f.weights.data(), f.n_edges() * sizeof(float)) == 0 && g.forest.n_edges() == f.n_edges());
                CHECK(same_as_sequential(g, f, n));
                CHECK(g.roots().size() == c.n_components());
            }
        }
    }
    std::printf("gpu mode OK\n");
    return 0;
}
