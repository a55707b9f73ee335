// hnswhds_select of include/hnsw_mi355x_hdbscan_select.h called from C++ on what forest_hdbscan of include/hnsw_rs.hpp returns:
// "cpu" checks what needs no device (no vertex, the refusals -- the host form reads the tree on the host --, the "no device" answer);
// "gpu" checks the hand-made forest of tests/test_hdbscan_select_abi.py against the values written out there, and that the defaults
// give the first stage's own bytes (tests/test_gpu_hdbscan_select.py checks the values against the model through the C ABI).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hnsw_mi355x_hdbscan_select.h"
#include "hnsw_rs.hpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

// a condensed tree and the answer of one selection on it
struct Selection {
    int rc = 0;
    std::vector<uint8_t> selected;
    std::vector<int32_t> labels;
    std::vector<float> prob, score;
    std::vector<double> death;
    uint64_t n_labels = 7777;
};

static Selection select(const hnsw_rs::Hdbscan& t, uint32_t method, uint32_t allow, float eps, uint64_t max_size) {
    Selection s;
    const size_t n = t.labels.size(), k = t.n_clusters();
    s.selected.assign(k ? k : 1, 9);
    s.labels.assign(n ? n : 1, -9);
    s.prob.assign(n ? n : 1, -9.f);
    s.score.assign(n ? n : 1, -9.f);
    s.death.assign(k ? k : 1, -9.0);
    s.rc = hnswhds_select(0, n, k, t.cluster_parent.data(), t.cluster_birth_w.data(), t.cluster_size.data(), t.stability.data(), t.point_cluster.data(),
                          t.point_w.data(), method, allow, eps, max_size, s.selected.data(), s.labels.data(), s.prob.data(), s.score.data(),
                          s.death.data(), &s.n_labels);
    return s;
}

int main(int argc, char** argv) {
    using namespace hnsw_rs;
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const float inf = std::numeric_limits<float>::infinity();
    // the hand-made tree, written out: K = 5 over 12 vertices
    Hdbscan hand;
    hand.cluster_parent = {UINT32_MAX, 0, 0, 2, 2};
    hand.cluster_birth_w = {inf, inf, inf, 1.f, 1.f};
    hand.cluster_size = {12, 4, 7, 3, 3};
    hand.stability = {0.0, 1.75, 6.5, 3.0, 9.0};
    hand.point_cluster = {4, 4, 4, 3, 3, 3, 2, 1, 1, 1, 1, 0};
    hand.point_w = {.25f, .25f, .25f, .5f, .5f, .5f, 2.f, 2.f, 2.f, 2.f, 4.f, inf};
    hand.labels.assign(12, -1);
    uint64_t count = 7777;
    CHECK(hnswhds_select(0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, HNSWGPU_SELECT_LEAF, 1, 2.f, 3, nullptr, nullptr, nullptr, nullptr,
                         nullptr, &count) == HNSWGPU_OK && count == 0);                                        // no vertex: no device
    CHECK(select(hand, 2, 0, 0.f, 0).rc == HNSWGPU_ERR_ARG && select(hand, 0, 2, 0.f, 0).rc == HNSWGPU_ERR_ARG);    // method, allow_single_cluster
    CHECK(select(hand, 0, 0, -1.f, 0).rc == HNSWGPU_ERR_ARG && select(hand, 0, 0, std::nanf(""), 0).rc == HNSWGPU_ERR_ARG);
    Hdbscan bad = hand;
    bad.cluster_parent[3] = 3;                                                                                  // a parent that is not below
    Selection s = select(bad, 0, 0, 0.f, 0);
    CHECK(s.rc == HNSWGPU_ERR_ARG && s.n_labels == 7777 && s.labels[0] == -9 && s.selected[0] == 9 && s.death[0] == -9.0);
    bad = hand;
    bad.cluster_parent[4] = 0;                                                                                  // cluster 2 keeps one child
    CHECK(select(bad, 0, 0, 0.f, 0).rc == HNSWGPU_ERR_ARG);
    bad = hand;
    bad.point_cluster[11] = 5;
    CHECK(select(bad, 0, 0, 0.f, 0).rc == HNSWGPU_ERR_ARG);
    bad = hand;
    bad.stability[1] = -0.5;
    CHECK(select(bad, 0, 0, 0.f, 0).rc == HNSWGPU_ERR_ARG && std::strlen(hnswgpu_last_error()) > 0);
    if (!gpu) {
        if (hnswgpu_device_count() == 0) CHECK(select(hand, 0, 0, 0.f, 0).rc == HNSWGPU_ERR_DEVICE);
        std::printf("cpu mode OK\n");
        return 0;
    }
    const std::vector<int32_t> dflt = {2, 2, 2, 1, 1, 1, -1, 0, 0, 0, 0, -1};
    s = select(hand, HNSWGPU_SELECT_EOM, 0, 0.f, 0);
    CHECK(s.rc == HNSWGPU_OK && s.n_labels == 3 && s.selected == std::vector<uint8_t>({0, 1, 0, 1, 1}) && s.labels == dflt);
    CHECK(s.prob == std::vector<float>({1, 1, 1, 1, 1, 1, 0, 1, 1, 1, .5f, 0}));
    CHECK(s.death == std::vector<double>({4.0, 0.5, 4.0, 2.0, 4.0}));
    CHECK(s.score == std::vector<float>({0, 0, 0, 0, 0, 0, .875f, 0, 0, 0, .5f, 1.f}));
    s = select(hand, HNSWGPU_SELECT_EOM, 0, 1.5f, 0);
    CHECK(s.n_labels == 2 && s.selected == std::vector<uint8_t>({0, 1, 1, 0, 0}) && s.labels == std::vector<int32_t>({1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, -1}));
    s = select(hand, HNSWGPU_SELECT_EOM, 0, 1.0f, 0);                                                            // equal to the births of 3 and 4: nothing moves
    CHECK(s.n_labels == 3 && s.labels == dflt);
    s = select(hand, HNSWGPU_SELECT_EOM, 0, 0.f, 3);
    CHECK(s.n_labels == 2 && s.selected == std::vector<uint8_t>({0, 0, 0, 1, 1}) && s.labels == std::vector<int32_t>({1, 1, 1, 0, 0, 0, -1, -1, -1, -1, -1, -1}));
    s = select(hand, HNSWGPU_SELECT_EOM, 0, 0.f, 2);
    CHECK(s.n_labels == 0 && s.labels == std::vector<int32_t>(12, -1));
    s = select(hand, HNSWGPU_SELECT_EOM, 1, 0.f, 0);                                                             // stability[0] = 0 loses
    CHECK(s.n_labels == 3 && s.labels == dflt);
    s = select(hand, HNSWGPU_SELECT_EOM, 1, inf, 0);                                                             // every climb ends at cluster 0
    CHECK(s.n_labels == 1 && s.selected == std::vector<uint8_t>({1, 0, 0, 0, 0}) && s.labels == std::vector<int32_t>(12, 0));
    // on the first stage's own answer the defaults give its bytes, for both methods
    const std::vector<uint32_t> ha = {0, 1, 3, 4, 2, 5, 7, 8, 9}, hb = {1, 2, 4, 5, 3, 6, 8, 9, 10};
    const std::vector<float> hw = {0.25f, 0.25f, 0.5f, 0.5f, 1.f, 2.f, 2.f, 2.f, 4.f};
    for (bool leaf : {false, true}) {
        const Hdbscan t = forest_hdbscan(12, ha, hb, hw, 3, leaf);
        s = select(t, leaf ? HNSWGPU_SELECT_LEAF : HNSWGPU_SELECT_EOM, 0, 0.f, 0);
        CHECK(s.rc == HNSWGPU_OK && s.n_labels == t.n_labels && s.selected == t.selected && s.labels == t.labels);
        CHECK(std::memcmp(s.prob.data(), t.probabilities.data(), 12 * sizeof(float)) == 0);
    }
    const Hdbscan one = forest_hdbscan(12, ha, hb, hw, 7);                                                      // K = 1
    s = select(one, HNSWGPU_SELECT_EOM, 1, 0.f, 0);
    CHECK(s.n_labels == 1 && s.labels == std::vector<int32_t>({0, 0, 0, 0, 0, 0, 0, -1, -1, -1, -1, -1}));
    CHECK(select(one, HNSWGPU_SELECT_EOM, 1, 0.f, 11).n_labels == 0 && select(one, HNSWGPU_SELECT_LEAF, 1, 0.f, 11).n_labels == 1);
    std::printf("gpu mode OK\n");
    return 0;
}
