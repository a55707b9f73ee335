// forest_hdbscan and Hnsw::hdbscan of include/hnsw_rs.hpp: "cpu" checks what needs no device (no vertex, the empty index, the
// refusals, the "no device" answer); "gpu" checks a hand-made forest against values written out here (the forest of
// tests/test_hdbscan_abi.py, worked out by hand there), an exact tie, and on a small built index that the index form carries
// knn_graph_dendrogram's bytes and agrees with the forest form on them (tests/test_gpu_hdbscan.py checks the values against the
// model through the C ABI).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hnsw_rs.hpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

template <class T>
static bool same_bytes(const std::vector<T>& x, const std::vector<T>& y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv) {
    using namespace hnsw_rs;
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(hnswhdb_max_clusters(12, 3) == 7 && hnswhdb_max_clusters(12, 7) == 1 && hnswhdb_max_clusters(0, 2) == 1);
    Hnsw<float, DistL2> h(8, 300, 16, 32);
    const auto none = h.hdbscan(5, 3);
    CHECK(none.n_clusters() == 0 && none.labels.empty() && none.n_labels == 0 && none.dendrogram.n_edges() == 0);
    const auto nothing = forest_hdbscan(0, {}, {}, {}, 2);
    CHECK(nothing.n_clusters() == 0 && nothing.labels.empty() && nothing.stability.empty());
    const size_t n = 300, d = 8;
    std::vector<float> x(n * d);
    uint32_t s = 12345;
    for (auto& v : x) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 16777216.f; }
    h.parallel_insert(x, d, {}, 1);
    try { h.hdbscan(5, 0); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { h.hdbscan(1, 3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }                      // mcs = 1
    try { h.hdbscan(5, 3, 0, false, 4); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }         // core_k > knbn
    try { forest_hdbscan(4, {0, 1}, {1}, {1, 2}, 2); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }
    try { forest_hdbscan(4, {0, 4}, {1, 2}, {1, 2}, 2); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }     // an end at n
    try { forest_hdbscan(4, {0, 2}, {1, 2}, {1, 2}, 2); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }     // a self-loop
    try { forest_hdbscan(4, {0, 1}, {1, 2}, {2, 1}, 2); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }     // descending
    try { forest_hdbscan(4, {0, 1}, {1, 2}, {1, 2}, 1); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }     // mcs = 1
    const std::vector<uint32_t> ha = {0, 1, 3, 4, 2, 5, 7, 8, 9}, hb = {1, 2, 4, 5, 3, 6, 8, 9, 10};
    const std::vector<float> hw = {0.25f, 0.25f, 0.5f, 0.5f, 1.f, 2.f, 2.f, 2.f, 4.f};
    if (!gpu) {
        if (hnswgpu_device_count() == 0) {
            try { h.hdbscan(5, 3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
            try { forest_hdbscan(12, ha, hb, hw, 3); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_DEVICE); }
        }
        std::printf("cpu mode OK\n");
        return 0;
    }
    // 12 vertices: {0, 1, 2} closes at 1/4, {3, 4, 5} at 1/2, the two join at 1, vertex 6 joins at 2; {7, 8, 9} closes at 2, vertex
    // 10 joins at 4; vertex 11 alone
    auto t = forest_hdbscan(12, ha, hb, hw, 3);
    CHECK(t.n_clusters() == 5 && t.n_labels == 3);
    CHECK(t.cluster_parent == std::vector<uint32_t>({UINT32_MAX, 0, 0, 2, 2}) && t.cluster_size == std::vector<uint32_t>({12, 4, 7, 3, 3}));
    CHECK(t.cluster_birth_w == std::vector<float>({inf, inf, inf, 1.f, 1.f}));
    CHECK(t.point_cluster == std::vector<uint32_t>({4, 4, 4, 3, 3, 3, 2, 1, 1, 1, 1, 0}));
    CHECK(t.point_w == std::vector<float>({.25f, .25f, .25f, .5f, .5f, .5f, 2.f, 2.f, 2.f, 2.f, 4.f, inf}));
    CHECK(t.stability == std::vector<double>({0.0, 1.75, 6.5, 3.0, 9.0}) && t.selected == std::vector<uint8_t>({0, 1, 0, 1, 1}));
    CHECK(t.labels == std::vector<int32_t>({2, 2, 2, 1, 1, 1, -1, 0, 0, 0, 0, -1}));
    CHECK(t.probabilities == std::vector<float>({1, 1, 1, 1, 1, 1, 0, 1, 1, 1, .5f, 0}));
    t = forest_hdbscan(12, ha, hb, hw, 4);
    CHECK(t.n_clusters() == 3 && t.n_labels == 2 && t.stability == std::vector<double>({0.0, 1.0, 6.5}));
    CHECK(t.labels == std::vector<int32_t>({1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, -1}));
    t = forest_hdbscan(12, ha, hb, hw, 3, true);
    CHECK(t.selected == std::vector<uint8_t>({0, 1, 0, 1, 1}));
    // an exact tie goes to the parent: (1 - 0) 6 against (2 - 1) 3 + (2 - 1) 3
    const std::vector<uint32_t> ta = {0, 1, 3, 4, 6, 7, 2}, tb = {1, 2, 4, 5, 7, 8, 3};
    const std::vector<float> tw = {.5f, .5f, .5f, .5f, .5f, .5f, 1.f};
    t = forest_hdbscan(9, ta, tb, tw, 3);
    CHECK(t.n_clusters() == 5 && t.n_labels == 2 && t.stability[1] == 6.0 && t.stability[3] == 3.0 && t.stability[4] == 3.0);
    CHECK(t.selected == std::vector<uint8_t>({0, 1, 1, 0, 0}) && t.labels == std::vector<int32_t>({0, 0, 0, 0, 0, 0, 1, 1, 1}));
    CHECK(forest_hdbscan(9, ta, tb, tw, 3, true).n_labels == 3);
    try { forest_hdbscan(4, {0, 1, 2}, {1, 2, 0}, {1, 1, 1}, 2); CHECK(false); } catch (const Error& e) { CHECK(e.code == HNSWGPU_ERR_ARG); }  // a triangle
    const auto no_edge = forest_hdbscan(3, {}, {}, {}, 2);
    CHECK(no_edge.n_clusters() == 1 && no_edge.labels == std::vector<int32_t>({-1, -1, -1}) && no_edge.point_w == std::vector<float>({inf, inf, inf}));
    for (size_t ef : {(size_t)0, (size_t)32}) {
        for (bool mutual : {false, true}) {
            for (bool leaf : {false, true}) {
                const auto g = h.knn_graph_dendrogram(4, ef, mutual, 3);
                const auto r = h.hdbscan(5, 4, ef, mutual, 3, leaf);
                CHECK(r.dendrogram.forest.a == g.forest.a && r.dendrogram.forest.b == g.forest.b && same_bytes(r.dendrogram.forest.weights, g.forest.weights));
                CHECK(r.dendrogram.left == g.left && r.dendrogram.right == g.right && r.dendrogram.sizes == g.sizes && r.dendrogram.n_vertices == n);
                const auto f = forest_hdbscan(n, g.forest.a, g.forest.b, g.forest.weights, 5, leaf);
                CHECK(r.labels == f.labels && same_bytes(r.probabilities, f.probabilities) && r.point_cluster == f.point_cluster && same_bytes(r.point_w, f.point_w));
                CHECK(r.cluster_parent == f.cluster_parent && same_bytes(r.cluster_birth_w, f.cluster_birth_w) && r.cluster_size == f.cluster_size);
                CHECK(same_bytes(r.stability, f.stability) && r.selected == f.selected && r.n_labels == f.n_labels);
                CHECK(r.labels.size() == n && r.n_clusters() >= 1 && r.cluster_size[0] == n);
                size_t sel = 0;
                for (size_t c = 0; c < r.n_clusters(); ++c) {
                    sel += r.selected[c];
                    CHECK(c == 0 || r.cluster_parent[c] < c);
                }
                CHECK(sel == r.n_labels);
                for (size_t v = 0; v < n; ++v) {
                    CHECK(r.labels[v] >= -1 && r.labels[v] < (int32_t)r.n_labels && r.point_cluster[v] < r.n_clusters());
                    CHECK(r.probabilities[v] >= 0.f && r.probabilities[v] <= 1.f && (r.labels[v] >= 0 || r.probabilities[v] == 0.f));
                }
            }
        }
    }
    const auto dflt = h.hdbscan(5, 4);   // core_k = min(5 - 1, 4)
    CHECK(same_bytes(dflt.dendrogram.forest.weights, h.knn_graph_spanning_forest(4, 0, false, 4).weights));
    std::printf("gpu mode OK\n");
    return 0;
}
