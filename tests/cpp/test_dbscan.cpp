// hnswdbs_csr of include/hnsw_mi355x_dbscan.h called from C++: "cpu" checks what needs no device (no vertex, the refusals -- the host
// form reads the graph on the host --, the "no device" answer); "gpu" checks the third hand-made case of tests/test_dbscan_abi.py
// against the values written out there (tests/test_gpu_dbscan.py checks the values against the model through the C ABI).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hnsw_mi355x_dbscan.h"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

struct Graph {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> cols;
    std::vector<float> dists;
};
struct Answer {
    int rc = 0;
    std::vector<int32_t> label;
    std::vector<uint8_t> core;
    std::vector<uint32_t> count, anchor;
    uint64_t c = 77;
    bool untouched() const {
        return label == std::vector<int32_t>(label.size(), -9) && core == std::vector<uint8_t>(core.size(), 9) &&
               count == std::vector<uint32_t>(count.size(), 9) && anchor == std::vector<uint32_t>(anchor.size(), 9) && c == 77;
    }
};

static Answer run(const Graph& g, float eps, uint64_t min_samples, uint32_t add_self, bool with_dists = true) {
    const uint64_t n = g.offsets.size() - 1;
    Answer a;
    a.label.assign(n, -9);
    a.core.assign(n, 9);
    a.count.assign(n, 9);
    a.anchor.assign(n, 9);
    a.rc = hnswdbs_csr(0, n, g.offsets.data(), g.cols.data(), with_dists ? g.dists.data() : nullptr, eps, min_samples, add_self, a.label.data(),
                       a.core.data(), a.count.data(), a.anchor.data(), &a.c);
    return a;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const float inf = std::numeric_limits<float>::infinity();
    const uint32_t none = UINT32_MAX;
    // the third hand-made case, written out: seven vertices, add_self 1, min_samples 4
    const Graph hand{{0, 3, 6, 7, 10, 12, 13, 13}, {1, 1, 0, 0, 1, 1, 3, 3, 3, 3, 1, 0, 2}, {.5f, .5f, 0.f, .25f, .1f, .1f, 1.f, 0.f, 0.f, 0.f, -0.f, 0.f, .1f}};
    uint64_t c = 77;
    CHECK(hnswdbs_csr(0, 0, nullptr, nullptr, nullptr, 1.f, 1, 0, nullptr, nullptr, nullptr, nullptr, &c) == HNSWGPU_OK && c == 0);  // no vertex: no device
    Answer a = run(hand, inf, 0, 1);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.untouched() && std::strstr(hnswgpu_last_error(), "min_samples"));
    a = run(hand, std::nanf(""), 4, 1);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.untouched() && std::strstr(hnswgpu_last_error(), "NaN"));
    a = run(hand, inf, 4, 2);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.untouched() && std::strstr(hnswgpu_last_error(), "add_self"));
    CHECK(hnswdbs_csr(0, 7, hand.offsets.data(), hand.cols.data(), nullptr, inf, 4, 1, nullptr, nullptr, nullptr, nullptr, &c) == HNSWGPU_ERR_ARG);
    CHECK(hnswdbs_csr(0, 7, hand.offsets.data(), hand.cols.data(), nullptr, inf, 4, 1, a.label.data(), nullptr, nullptr, nullptr, nullptr) == HNSWGPU_ERR_ARG);
    CHECK(hnswdbs_csr(0, 1ull << 31, hand.offsets.data(), hand.cols.data(), nullptr, inf, 4, 1, a.label.data(), nullptr, nullptr, nullptr, &c) == HNSWGPU_ERR_ARG);
    Graph bad = hand;
    bad.offsets[0] = 1;
    a = run(bad, inf, 4, 1);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.untouched() && std::strstr(hnswgpu_last_error(), "offsets[0] is not 0"));
    bad = hand;
    bad.offsets[3] = 5;
    a = run(bad, inf, 4, 1);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.untouched() && std::strstr(hnswgpu_last_error(), "the offsets descend"));
    bad = hand;
    bad.cols[12] = 7;
    a = run(bad, inf, 4, 1);
    CHECK(a.rc == HNSWGPU_ERR_ARG && a.untouched() && std::strstr(hnswgpu_last_error(), "is not below n"));
    if (!gpu) {
        if (hnswgpu_device_count() == 0) {
            a = run(hand, inf, 4, 1);
            CHECK(a.rc == HNSWGPU_ERR_DEVICE && a.untouched());
        }
        std::printf("cpu mode OK\n");
        return 0;
    }
    a = run(hand, inf, 4, 1);
    CHECK(a.rc == HNSWGPU_OK && a.c == 2);
    CHECK(a.label == std::vector<int32_t>({0, 0, 1, 1, 0, -1, -1}));
    CHECK(a.core == std::vector<uint8_t>({1, 1, 0, 1, 0, 0, 0}));
    CHECK(a.count == std::vector<uint32_t>({4, 4, 2, 4, 3, 2, 1}));
    CHECK(a.anchor == std::vector<uint32_t>({0, 1, 3, 3, 0, none, none}));
    a = run(hand, -1.f, 1, 1, false);  // without dists eps is not read: every entry counts, every point is core
    CHECK(a.rc == HNSWGPU_OK && a.c == 3 && a.label == std::vector<int32_t>({0, 0, 1, 1, 0, 1, 2}) && a.count == std::vector<uint32_t>({4, 4, 2, 4, 3, 2, 1}));
    a = run(hand, -1.f, 2, 1);  // nothing is within a negative eps: every count is add_self
    CHECK(a.rc == HNSWGPU_OK && a.c == 0 && a.label == std::vector<int32_t>(7, -1) && a.count == std::vector<uint32_t>(7, 1) &&
          a.anchor == std::vector<uint32_t>(7, none));
    std::printf("gpu mode OK\n");
    return 0;
}
