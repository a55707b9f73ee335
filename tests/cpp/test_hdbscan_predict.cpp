// hnswhdp_assign of include/hnsw_mi355x_hdbscan_predict.h called from C++: "cpu" checks what needs no device (no query, the refusals --
// the host form reads the tree and the rows on the host --, the "no device" answer); "gpu" checks the hand-made case of
// tests/test_hdbscan_predict_abi.py against the values written out there (tests/test_gpu_hdbscan_predict.py checks the values against
// the model through the C ABI).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hnsw_mi355x_hdbscan_predict.h"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

// the condensed tree, its selection and the stored points' core distances
struct Tree {
    std::vector<uint32_t> parent, point_cluster;
    std::vector<float> birth, point_w, core;
    std::vector<uint8_t> selected;
    std::vector<double> death;
};
// nq rows of k slots
struct Rows {
    uint64_t nq, k;
    std::vector<uint32_t> pos, counts;
    std::vector<float> dist;
};
struct Answer {
    int rc = 0;
    std::vector<int32_t> labels;
    std::vector<float> prob, score, w;
    std::vector<uint32_t> nearest, cluster;
};

static Answer assign(const Tree& t, const Rows& r, uint64_t core_k, float eps, bool with_death = true) {
    Answer a;
    a.labels.assign(r.nq, -9);
    a.prob.assign(r.nq, -9.f);
    a.score.assign(r.nq, -9.f);
    a.w.assign(r.nq, -9.f);
    a.nearest.assign(r.nq, 9);
    a.cluster.assign(r.nq, 9);
    a.rc = hnswhdp_assign(0, r.nq, r.k, r.pos.data(), r.dist.data(), r.counts.data(), core_k, t.point_cluster.size(), t.core.data(), t.parent.size(),
                          t.parent.data(), t.birth.data(), t.point_cluster.data(), t.point_w.data(), t.selected.data(), eps,
                          with_death ? t.death.data() : nullptr, a.labels.data(), a.prob.data(), with_death ? a.score.data() : nullptr, a.nearest.data(),
                          a.w.data(), a.cluster.data());
    return a;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const float inf = std::numeric_limits<float>::infinity();
    // the hand-made tree, written out: K = 5 over 12 vertices, selected {1, 3, 4}
    Tree hand;
    hand.parent = {UINT32_MAX, 0, 0, 2, 2};
    hand.birth = {inf, inf, inf, 1.f, 1.f};
    hand.point_cluster = {4, 4, 4, 3, 3, 3, 2, 1, 1, 1, 1, 0};
    hand.point_w = {.25f, .25f, .25f, .5f, .5f, .5f, 2.f, 2.f, 2.f, 2.f, 4.f, inf};
    hand.core = {0, 0, 0, 0, 0, 0, 2.f, 0, 0, 0, 4.f, 0};
    hand.selected = {0, 1, 0, 1, 1};
    hand.death = {4.0, 0.5, 4.0, 2.0, 4.0};
    // the twelve rows of three slots
    Rows rows{12, 3,
              {3, 0, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0, 1, 0, 7, 1, 3, 5, 0, 6, 0, 0, 10, 7, 0},
              {1, 1, 1, 1, 1, 1, 0, 3, 3, 2, 1, 2},
              {.5f, 0, 0, .25f, 0, 0, 1.f, 0, 0, .5f, 0, 0, 2.f, 0, 0, inf, 0, 0, 0, 0, 0, 2.f, 2.f, 2.f, 1.f, 2.f, 2.f, -0.f, 0.f, 0, .5f, 0, 0, 1.f, 3.f, 0}};
    CHECK(hnswhdp_assign(0, 0, 3, nullptr, nullptr, nullptr, 2, 12, nullptr, 5, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr) == HNSWGPU_OK);                                      // no query: no device
    CHECK(assign(hand, rows, 2, -1.f).rc == HNSWGPU_ERR_ARG && assign(hand, rows, 2, std::nanf("")).rc == HNSWGPU_ERR_ARG);
    CHECK(assign(hand, rows, 4, 0.f).rc == HNSWGPU_ERR_ARG);                                                      // core_k above knbn
    Tree bad = hand;
    bad.parent[3] = 3;                                                                                           // a parent that is not below
    Answer a = assign(bad, rows, 2, 0.f);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.labels[0] == -9 && a.prob[0] == -9.f && a.score[0] == -9.f && a.nearest[0] == 9 && a.w[0] == -9.f && a.cluster[0] == 9);
    bad = hand;
    bad.parent[1] = 2;
    bad.parent[2] = 1;                                                                                           // a 2-cycle
    CHECK(assign(bad, rows, 2, 0.f).rc == HNSWGPU_ERR_ARG);
    bad = hand;
    bad.point_cluster[11] = 5;
    CHECK(assign(bad, rows, 2, 0.f).rc == HNSWGPU_ERR_ARG);
    Rows worse = rows;
    worse.counts[4] = 4;
    CHECK(assign(hand, worse, 2, 0.f).rc == HNSWGPU_ERR_ARG);
    worse = rows;
    worse.pos[0] = 12;
    CHECK(assign(hand, worse, 2, 0.f).rc == HNSWGPU_ERR_ARG && std::strlen(hnswgpu_last_error()) > 0);
    if (!gpu) {
        if (hnswgpu_device_count() == 0) CHECK(assign(hand, rows, 2, 0.f).rc == HNSWGPU_ERR_DEVICE);
        std::printf("cpu mode OK\n");
        return 0;
    }
    const float third = (float)((1.0 / 3.0f) / 0.5), gap = (float)((0.5 - 1.0 / 3.0f) / 0.5);
    a = assign(hand, rows, 2, 0.f);
    CHECK(a.rc == HNSWGPU_OK);
    CHECK(a.nearest == std::vector<uint32_t>({3, 3, 3, 0, 0, 0, UINT32_MAX, 7, 0, 3, 6, 7}));
    CHECK(a.cluster == std::vector<uint32_t>({3, 3, 2, 4, 2, 0, 0, 1, 2, 3, 2, 1}));
    CHECK(a.labels == std::vector<int32_t>({1, 1, -1, 2, -1, -1, -1, 0, -1, 1, -1, 0}));
    CHECK(a.w == std::vector<float>({.5f, .25f, 1.f, .5f, 2.f, inf, inf, 2.f, 2.f, -0.f, 2.f, 3.f}) && std::signbit(a.w[9]));
    CHECK(a.prob == std::vector<float>({1, 1, 0, .5f, 0, 0, 0, 1, 0, 1, 0, third}));
    CHECK(a.score == std::vector<float>({0, 0, .75f, .5f, .875f, 1, 1, 0, .875f, 0, .875f, gap}));
    a = assign(hand, rows, 2, 0.f, false);                                                                       // without death: no score
    CHECK(a.rc == HNSWGPU_OK && a.score == std::vector<float>(12, -9.f) && a.labels == std::vector<int32_t>({1, 1, -1, 2, -1, -1, -1, 0, -1, 1, -1, 0}));
    hand.selected = {0, 1, 1, 0, 0};                                                                             // a query in 3 or 4, which lost, is of 2
    a = assign(hand, rows, 2, 1.5f);
    CHECK(a.rc == HNSWGPU_OK && a.labels == std::vector<int32_t>({1, 1, 1, 1, 1, -1, -1, 0, 1, 1, 1, 0}));
    CHECK(a.prob == std::vector<float>({1, 1, 1, 1, .5f, 0, 0, 1, .5f, 1, .5f, third}));
    // K = 1, selected {0}: the threshold is maxlambda(0) = 1/2, or 1 / eps
    Tree one;
    one.parent = {UINT32_MAX};
    one.birth = {inf};
    one.point_cluster.assign(12, 0);
    one.point_w = {2.f, 2.f, 2.f, 2.f, 2.f, 2.f, 2.f, inf, inf, inf, inf, inf};
    one.core = hand.core;
    one.selected = {1};
    one.death = {0.5};
    a = assign(one, rows, 2, 0.f);
    CHECK(a.rc == HNSWGPU_OK && a.labels == std::vector<int32_t>({0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, -1}) && a.cluster == std::vector<uint32_t>(12, 0));
    a = assign(one, rows, 2, 4.f);
    CHECK(a.rc == HNSWGPU_OK && a.labels == std::vector<int32_t>({0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0}) && a.prob[11] == third);
    std::printf("gpu mode OK\n");
    return 0;
}
