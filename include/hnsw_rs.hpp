// hnsw_rs.hpp -- header-only C++ mirror of the hnsw_rs interface for the search path, on top of the C ABI of
// libhnsw_mi355x.so (include/hnsw_mi355x.h).  The reference is Rust; this image has no Rust toolchain, so
// the host side above the C ABI is written in C++ with the crate's names and argument meaning:
//
//   hnsw_rs::Neighbour / PointId                      src/hnsw.rs:46, :98-107
//   hnsw_rs::DistL2 / DistCosine / DistDot / DistL1   anndists distance type names (src/hnswio.rs:473-490)
//   hnsw_rs::Hnsw<T, D>::search / parallel_search     src/hnsw.rs:1597, :1612
//   hnsw_rs::AnnT<T> (search_neighbours, parallel_search_neighbours, file_dump)   src/api.rs:13-38
//   hnsw_rs::HnswIo(dir, basename).load_hnsw<T, D>()  src/hnswio.rs:317, :431
//
// Errors: anyhow::Result becomes hnsw_rs::Error (carries the C-ABI status); nothing aborts the process.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "hnsw_mi355x.h"
#include "hnsw_mi355x_hdbscan.h"

namespace hnsw_rs {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
    if (rc != HNSWGPU_OK) throw Error(rc, hnswgpu_last_error());
}

struct PointId {  // PointId(pub u8, pub i32)
    uint8_t layer;
    int32_t rank;
    bool operator==(const PointId& o) const { return layer == o.layer && rank == o.rank; }
};
struct Neighbour {  // #[repr(C)] { d_id: usize, distance: f32, p_id: PointId }
    size_t d_id;
    float distance;
    PointId p_id;
};

struct DistL2 { static constexpr int code = HNSWGPU_DIST_L2; };
struct DistCosine { static constexpr int code = HNSWGPU_DIST_COSINE; };
struct DistDot { static constexpr int code = HNSWGPU_DIST_DOT; };
struct DistL1 { static constexpr int code = HNSWGPU_DIST_L1; };

// trait AnnT { type Val; ... }
template <class T>
struct AnnT {
    virtual ~AnnT() = default;
    virtual std::vector<Neighbour> search_neighbours(const std::vector<T>& data, size_t knbn, size_t ef_s) const = 0;
    virtual std::vector<std::vector<Neighbour>> parallel_search_neighbours(const std::vector<std::vector<T>>& data,
                                                                           size_t knbn, size_t ef_s) const = 0;
    virtual std::string file_dump(const std::string& path, const std::string& file_basename) const = 0;
};

// Connected components (an extension: hnswgpu_graph_components, hnswgpu_csr_components): labels[v] is the component of vertex v,
// components numbered 0 .. sizes.size() - 1 by their smallest vertex, ascending; sizes[c] is the number of vertices of c.
struct Components {
    std::vector<uint32_t> labels;
    std::vector<uint32_t> sizes;
    size_t n_components() const { return sizes.size(); }
};
// The components of ANY graph given in CSR (offsets.size() == n + 1, cols.size() >= offsets[n]), labelled on `device`: every entry
// (r, c) joins r and c, whichever row names it.  max_dist (needs dists): an entry counts iff its distance is <= *max_dist.
inline Components csr_components(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& cols, const std::vector<float>* dists = nullptr,
                                 const float* max_dist = nullptr, int device = 0) {
    Components c;
    if (offsets.empty() || offsets.back() > cols.size() || (dists && dists->size() < cols.size()))
        throw Error(HNSWGPU_ERR_ARG, "csr_components: offsets must hold n + 1 entries, cols and dists offsets[n]");
    const size_t n = offsets.size() - 1;
    c.labels.assign(n, 0);
    c.sizes.assign(n, 0);
    uint64_t count = 0;
    check(hnswgpu_csr_components(device, n, offsets.data(), cols.data(), dists ? dists->data() : nullptr, max_dist, c.labels.data(), c.sizes.data(),
                                 &count));
    c.sizes.resize(count);
    return c;
}

// The minimum spanning forest (an extension: hnswgpu_graph_spanning_forest, hnswgpu_csr_spanning_forest): edge e joins vertices
// a[e] < b[e] with weight weights[e] (the bits as the graph stores them); the edges ascend by (weight, a, b), weights ordered by
// value, -0 equal to +0, every NaN behind +inf.  Read in this order they are the merges of the single-linkage hierarchy.
struct SpanningForest {
    std::vector<uint32_t> a;
    std::vector<uint32_t> b;
    std::vector<float> weights;
    size_t n_edges() const { return a.size(); }
};
// The forest of ANY graph given in CSR (offsets.size() == n + 1, cols.size() >= offsets[n]), taken on `device`: every entry (r, c) is
// the undirected pair {r, c} with weight (*dists)[e] (no dists: +0), self-loops are ignored, a repeated pair has the min of its weights.
inline SpanningForest csr_spanning_forest(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& cols, const std::vector<float>* dists = nullptr,
                                          int device = 0) {
    SpanningForest f;
    if (offsets.empty() || offsets.back() > cols.size() || (dists && dists->size() < cols.size()))
        throw Error(HNSWGPU_ERR_ARG, "csr_spanning_forest: offsets must hold n + 1 entries, cols and dists offsets[n]");
    const size_t n = offsets.size() - 1, slots = n > 1 ? n - 1 : 1;
    f.a.assign(slots, 0);
    f.b.assign(slots, 0);
    f.weights.assign(slots, 0.0f);
    uint64_t count = 0;
    check(hnswgpu_csr_spanning_forest(device, n, offsets.data(), cols.data(), dists ? dists->data() : nullptr, f.a.data(), f.b.data(), f.weights.data(),
                                      &count));
    f.a.resize(count);
    f.b.resize(count);
    f.weights.resize(count);
    return f;
}

// The single-linkage dendrogram of a forest (an extension: hnswgpu_forest_dendrogram, hnswgpu_graph_dendrogram): merge e joins the
// clusters left[e] and right[e] into cluster n_vertices + e of sizes[e] vertices.  Cluster ids are scipy's: an id below n_vertices
// is that vertex alone.  forest: the edges and weights where the call had them (knn_graph_dendrogram), else empty.
struct Dendrogram {
    std::vector<uint32_t> left;
    std::vector<uint32_t> right;
    std::vector<uint32_t> sizes;
    size_t n_vertices = 0;
    SpanningForest forest;
    size_t n_edges() const { return left.size(); }
    // the ids of the clusters that are nobody's child, ascending: one per component of the forest
    std::vector<uint32_t> roots() const {
        std::vector<char> child(n_vertices + n_edges(), 0);
        for (size_t e = 0; e < n_edges(); ++e) child[left[e]] = child[right[e]] = 1;
        std::vector<uint32_t> r;
        for (size_t x = 0; x < child.size(); ++x)
            if (!child[x]) r.push_back((uint32_t)x);
        return r;
    }
};
// The dendrogram of the forest whose edge e joins vertices a[e] and b[e] of 0 .. n - 1, built on `device`: the edges' order is the
// merge order.  An end >= n, a self-loop, more than n - 1 edges and a cycle are HNSWGPU_ERR_ARG.
inline Dendrogram forest_dendrogram(size_t n, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, int device = 0) {
    if (a.size() != b.size()) throw Error(HNSWGPU_ERR_ARG, "forest_dendrogram: a and b must hold one entry per edge");
    Dendrogram d;
    const size_t m = a.size();
    d.n_vertices = n;
    d.left.assign(m, 0);
    d.right.assign(m, 0);
    d.sizes.assign(m, 0);
    check(hnswgpu_forest_dendrogram(device, n, m, a.data(), b.data(), d.left.data(), d.right.data(), d.sizes.data()));
    return d;
}

// HDBSCAN's answer (an extension: hnswhdb_forest, hnswhdb_graph; the definitions are hnsw_mi355x_hdbscan.h's).  Per vertex:
// labels (-1: noise), probabilities, point_cluster and point_w (the cluster of the condensed tree that the vertex leaves, and the
// weight at which it does).  Per cluster, cluster 0 the root: cluster_parent (UINT32_MAX for cluster 0), cluster_birth_w, cluster_size,
// stability, selected.  n_labels selected clusters, numbered by ascending cluster index.  dendrogram (with its forest): where the
// call produced it (Hnsw::hdbscan), else empty.
struct Hdbscan {
    std::vector<int32_t> labels;
    std::vector<float> probabilities;
    std::vector<uint32_t> point_cluster;
    std::vector<float> point_w;
    std::vector<uint32_t> cluster_parent;
    std::vector<float> cluster_birth_w;
    std::vector<uint32_t> cluster_size;
    std::vector<double> stability;
    std::vector<uint8_t> selected;
    size_t n_labels = 0;
    Dendrogram dendrogram;
    size_t n_clusters() const { return cluster_parent.size(); }
    // the out arrays of a call over n vertices (at least one slot each: no NULL goes to the C entry)
    void prepare(size_t n, size_t min_cluster_size) {
        const size_t k = (size_t)hnswhdb_max_clusters(n, min_cluster_size);
        labels.assign(n ? n : 1, -1);
        probabilities.assign(n ? n : 1, 0.0f);
        point_cluster.assign(n ? n : 1, 0);
        point_w.assign(n ? n : 1, 0.0f);
        cluster_parent.assign(k ? k : 1, 0);
        cluster_birth_w.assign(k ? k : 1, 0.0f);
        cluster_size.assign(k ? k : 1, 0);
        stability.assign(k ? k : 1, 0.0);
        selected.assign(k ? k : 1, 0);
    }
    void finish(size_t n, uint64_t clusters, uint64_t n_lab) {
        labels.resize(n);
        probabilities.resize(n);
        point_cluster.resize(n);
        point_w.resize(n);
        cluster_parent.resize(clusters);
        cluster_birth_w.resize(clusters);
        cluster_size.resize(clusters);
        stability.resize(clusters);
        selected.resize(clusters);
        n_labels = (size_t)n_lab;
    }
};
// HDBSCAN's clusters of the forest whose edge e joins vertices a[e] and b[e] of 0 .. n - 1 with weight weights[e], on `device`: the
// edges' order is the merge order and the weights must not descend.  leaf: select the leaves of the condensed tree instead of by
// excess of mass.  What forest_dendrogram refuses, weights that descend and a min_cluster_size outside 2 .. 2^31 - 1 are HNSWGPU_ERR_ARG.
inline Hdbscan forest_hdbscan(size_t n, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, const std::vector<float>& weights,
                              size_t min_cluster_size, bool leaf = false, int device = 0) {
    if (a.size() != b.size() || a.size() != weights.size()) throw Error(HNSWGPU_ERR_ARG, "forest_hdbscan: a, b and weights must hold one entry per edge");
    Hdbscan r;
    r.prepare(n, min_cluster_size);
    uint64_t clusters = 0, n_lab = 0;
    check(hnswhdb_forest(device, n, a.size(), a.data(), b.data(), weights.data(), min_cluster_size, leaf ? HNSWGPU_SELECT_LEAF : HNSWGPU_SELECT_EOM,
                                 r.labels.data(), r.probabilities.data(), r.point_cluster.data(), r.point_w.data(), r.cluster_parent.data(),
                                 r.cluster_birth_w.data(), r.cluster_size.data(), r.stability.data(), r.selected.data(), &clusters, &n_lab));
    r.finish(n, clusters, n_lab);
    return r;
}

template <class T, class D>
class Hnsw;

// Hnsw<f32, D>: owns a hnswgpu_index (flat host graph + HBM replica).
template <class D>
class Hnsw<float, D> : public AnnT<float> {
public:
    // Hnsw::new(max_nb_connection, max_elements, max_layer, ef_construction, D{})
    Hnsw(size_t max_nb_connection, size_t /*max_elements*/, size_t max_layer, size_t ef_construction, D = D{}) {
        params_.max_nb_connection = max_nb_connection;
        params_.ef_construction = ef_construction;
        params_.max_layer = max_layer;
        params_.dist = D::code;
        params_.level_scale_factor = 1.0;
        if (max_nb_connection > 256) throw Error(HNSWGPU_ERR_ARG, "error max_nb_connection must be less equal than 256");
    }
    explicit Hnsw(hnswgpu_index* loaded) : idx_(loaded) {}
    Hnsw(Hnsw&& o) noexcept : idx_(o.idx_), params_(o.params_) { o.idx_ = nullptr; }
    Hnsw(const Hnsw&) = delete;
    Hnsw& operator=(const Hnsw&) = delete;
    ~Hnsw() override { hnswgpu_free_index(idx_); }

    void set_extend_candidates(bool f) { params_.extend_candidates = f; }
    void set_keeping_pruned(bool f) { params_.keep_pruned = f; }
    void modify_level_scale(double f) { params_.level_scale_factor = f < 0.2 ? 0.2 : (f > 1.0 ? 1.0 : f); }

    // parallel_insert(&[(&Vec<T>, usize)]): data row-major n x d, ids may be empty (0..n-1)
    void parallel_insert(const std::vector<float>& data, size_t d, const std::vector<uint64_t>& ids = {}, int nthreads = 0) {
        if (idx_) throw Error(HNSWGPU_ERR_ARG, "this binding builds an index in one parallel_insert call");
        params_.nthreads = nthreads;
        check(hnswgpu_build(data.data(), data.size() / d, d, ids.empty() ? nullptr : ids.data(), &params_, &idx_));
    }
    size_t get_nb_point() const { return idx_ ? hnswgpu_nb_point(idx_) : 0; }
    uint8_t get_max_level_observed() const { return idx_ ? (uint8_t)hnswgpu_max_level_observed(idx_) : 0; }

    // replication into the HBM of one device (one process per GPU)
    void upload(int device = 0) { check(hnswgpu_upload(idx_, device)); }
    void set_strict_ties(bool on) { check(hnswgpu_set_strict_ties(idx_, on)); }
    // distances of the following searches summed like the crate's simdeez_f build (true) or its default build (false)
    void set_simd_order_arithmetic(bool on) { check(hnswgpu_set_arithmetic(idx_, on ? HNSWGPU_ARITH_SIMD8 : HNSWGPU_ARITH_SCALAR)); }
    // the replicas hold the vectors as IEEE binary16 (true: half the bytes; every stored element must be representable, the caller
    // rounds and the library verifies) or as f32 (false, the default); the answers of every search are the same bit for bit
    void set_storage(bool half_precision) { check(hnswgpu_set_storage(idx_, half_precision ? HNSWGPU_STORAGE_F16 : HNSWGPU_STORAGE_F32)); }
    bool half_precision_storage() const { return hnswgpu_get_storage(idx_) == HNSWGPU_STORAGE_F16; }

    // search(&[T], knbn, ef) -> Vec<Neighbour>
    std::vector<Neighbour> search(const std::vector<float>& data, size_t knbn, size_t ef) const {
        return flat_search(data.data(), 1, data.size(), knbn, ef)[0];
    }
    // parallel_search(&[Vec<T>], knbn, ef) -> Vec<Vec<Neighbour>>, answers in input order
    std::vector<std::vector<Neighbour>> parallel_search(const std::vector<std::vector<float>>& datas, size_t knbn, size_t ef) const {
        if (datas.empty()) return {};
        const size_t d = datas[0].size();
        std::vector<float> flat;
        flat.reserve(datas.size() * d);
        for (const auto& v : datas) flat.insert(flat.end(), v.begin(), v.end());
        return flat_search(flat.data(), datas.size(), d, knbn, ef);
    }
    // AnnT
    std::vector<Neighbour> search_neighbours(const std::vector<float>& data, size_t knbn, size_t ef_s) const override {
        return search(data, knbn, ef_s);
    }
    std::vector<std::vector<Neighbour>> parallel_search_neighbours(const std::vector<std::vector<float>>& data, size_t knbn,
                                                                   size_t ef_s) const override {
        return parallel_search(data, knbn, ef_s);
    }
    std::string file_dump(const std::string& path, const std::string& file_basename) const override {
        if (!idx_) throw Error(HNSWGPU_ERR_EMPTY, "entry point not initialized");
        check(hnswgpu_file_dump(idx_, path.c_str(), file_basename.c_str()));
        return file_basename;
    }
    // The k-NN graph of the indexed points made undirected (an extension: hnswgpu_symmetric_graph), in CSR.  Vertices are POSITIONS
    // in the ascending (DataId, dump order) order; row i owns the slots offsets[i] .. offsets[i + 1] of pos (the neighbours'
    // positions) and neighbours (their DataIds, the stored f32 distances, their p_ids), ascending by (distance, position).
    struct GraphCsr {
        std::vector<uint64_t> offsets;
        std::vector<uint32_t> pos;
        std::vector<Neighbour> neighbours;
    };
    // ef == 0: from the exact graph, else from the approximate graph at this ef.  mutual: an edge only if both endpoints name the
    // other (HNSWGPU_SYM_MUTUAL), else if either does (HNSWGPU_SYM_UNION).  One counting call, one filling call.
    GraphCsr symmetric_knn_graph(size_t knbn, size_t ef = 0, bool mutual = false) const {
        GraphCsr g;
        const size_t n = get_nb_point();
        g.offsets.assign(n + 1, 0);
        if (!idx_) return g;
        const uint32_t mode = mutual ? HNSWGPU_SYM_MUTUAL : HNSWGPU_SYM_UNION;
        const int rc = hnswgpu_symmetric_graph(idx_, knbn, ef, mode, 0, g.offsets.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc != HNSWGPU_ERR_CAPACITY) check(rc);
        const size_t total = g.offsets[n];
        if (total == 0) return g;
        std::vector<uint64_t> ids(total);
        std::vector<float> dists(total);
        std::vector<uint8_t> layers(total);
        std::vector<int32_t> ranks(total);
        g.pos.resize(total);
        check(hnswgpu_symmetric_graph(idx_, knbn, ef, mode, total, g.offsets.data(), g.pos.data(), ids.data(), dists.data(), layers.data(),
                                      ranks.data()));
        g.neighbours.reserve(total);
        for (size_t e = 0; e < total; ++e) g.neighbours.push_back(Neighbour{(size_t)ids[e], dists[e], PointId{layers[e], ranks[e]}});
        return g;
    }
    // The connected components of the graph symmetric_knn_graph(knbn, ef, mutual) would build, labelled on the device without
    // building it; vertices are POSITIONS.  max_dist: the directed graph is cut first -- an entry counts iff its stored distance is
    // <= *max_dist --, then joined (mutual: iff both directions are left).
    Components knn_graph_components(size_t knbn, size_t ef = 0, bool mutual = false, const float* max_dist = nullptr) const {
        Components c;
        if (!idx_) return c;
        const size_t n = get_nb_point();
        c.labels.assign(n, 0);
        c.sizes.assign(n, 0);
        uint64_t count = 0;
        check(hnswgpu_graph_components(idx_, knbn, ef, mutual ? HNSWGPU_SYM_MUTUAL : HNSWGPU_SYM_UNION, max_dist, c.labels.data(), c.sizes.data(),
                                       &count));
        c.sizes.resize(count);
        return c;
    }
    // The minimum spanning forest of the graph symmetric_knn_graph(knbn, ef, mutual) would build, taken on the device without
    // building it; vertices are POSITIONS.  A pair weighs the min of its directions in the directed graph (mutual: the max of the
    // two); core_k >= 1: mutual-reachability weights, max(pair, core(a), core(b)), core(v) the distance to v's core_k-th neighbour.
    SpanningForest knn_graph_spanning_forest(size_t knbn, size_t ef = 0, bool mutual = false, size_t core_k = 0) const {
        SpanningForest f;
        if (!idx_) return f;
        const size_t n = get_nb_point(), slots = n > 1 ? n - 1 : 1;
        f.a.assign(slots, 0);
        f.b.assign(slots, 0);
        f.weights.assign(slots, 0.0f);
        uint64_t count = 0;
        check(hnswgpu_graph_spanning_forest(idx_, knbn, ef, mutual ? HNSWGPU_SYM_MUTUAL : HNSWGPU_SYM_UNION, core_k, f.a.data(), f.b.data(),
                                            f.weights.data(), &count));
        f.a.resize(count);
        f.b.resize(count);
        f.weights.resize(count);
        return f;
    }
    // knn_graph_spanning_forest(knbn, ef, mutual, core_k) and the dendrogram of that forest in one call, the forest staying on the
    // device in between: .forest is that call's answer, byte for byte.
    Dendrogram knn_graph_dendrogram(size_t knbn, size_t ef = 0, bool mutual = false, size_t core_k = 0) const {
        Dendrogram d;
        if (!idx_) return d;
        const size_t n = get_nb_point(), slots = n > 1 ? n - 1 : 1;
        d.n_vertices = n;
        d.forest.a.assign(slots, 0);
        d.forest.b.assign(slots, 0);
        d.forest.weights.assign(slots, 0.0f);
        d.left.assign(slots, 0);
        d.right.assign(slots, 0);
        d.sizes.assign(slots, 0);
        uint64_t count = 0;
        check(hnswgpu_graph_dendrogram(idx_, knbn, ef, mutual ? HNSWGPU_SYM_MUTUAL : HNSWGPU_SYM_UNION, core_k, d.forest.a.data(), d.forest.b.data(),
                                       d.forest.weights.data(), d.left.data(), d.right.data(), d.sizes.data(), &count));
        d.forest.a.resize(count);
        d.forest.b.resize(count);
        d.forest.weights.resize(count);
        d.left.resize(count);
        d.right.resize(count);
        d.sizes.resize(count);
        return d;
    }
    // HDBSCAN of the indexed points in one call: knn_graph_dendrogram(knbn, ef, mutual, core_k), then the condensed tree for
    // min_cluster_size, the stabilities, the selection and the labels, all on the device; vertices are POSITIONS.  core_k ==
    // SIZE_MAX means min(min_cluster_size - 1, knbn): sklearn's default min_samples = min_cluster_size, which counts the point
    // itself.  .dendrogram (and its .forest) is knn_graph_dendrogram's answer, byte for byte.
    Hdbscan hdbscan(size_t min_cluster_size, size_t knbn, size_t ef = 0, bool mutual = false, size_t core_k = SIZE_MAX, bool leaf = false) const {
        Hdbscan r;
        if (!idx_) return r;
        if (core_k == SIZE_MAX) core_k = min_cluster_size == 0 ? 0 : (min_cluster_size - 1 < knbn ? min_cluster_size - 1 : knbn);
        const size_t n = get_nb_point(), slots = n > 1 ? n - 1 : 1;
        r.prepare(n, min_cluster_size);
        Dendrogram& d = r.dendrogram;
        d.n_vertices = n;
        d.forest.a.assign(slots, 0);
        d.forest.b.assign(slots, 0);
        d.forest.weights.assign(slots, 0.0f);
        d.left.assign(slots, 0);
        d.right.assign(slots, 0);
        d.sizes.assign(slots, 0);
        uint64_t count = 0, clusters = 0, n_lab = 0;
        check(hnswhdb_graph(idx_, knbn, ef, mutual ? HNSWGPU_SYM_MUTUAL : HNSWGPU_SYM_UNION, core_k, min_cluster_size,
                                    leaf ? HNSWGPU_SELECT_LEAF : HNSWGPU_SELECT_EOM, d.forest.a.data(), d.forest.b.data(), d.forest.weights.data(),
                                    d.left.data(), d.right.data(), d.sizes.data(), r.labels.data(), r.probabilities.data(), r.point_cluster.data(),
                                    r.point_w.data(), r.cluster_parent.data(), r.cluster_birth_w.data(), r.cluster_size.data(), r.stability.data(),
                                    r.selected.data(), &clusters, &n_lab, &count));
        d.forest.a.resize(count);
        d.forest.b.resize(count);
        d.forest.weights.resize(count);
        d.left.resize(count);
        d.right.resize(count);
        d.sizes.resize(count);
        r.finish(n, clusters, n_lab);
        return r;
    }
    hnswgpu_index* handle() const { return idx_; }

private:
    std::vector<std::vector<Neighbour>> flat_search(const float* q, size_t nq, size_t d, size_t knbn, size_t ef) const {
        std::vector<std::vector<Neighbour>> out(nq);
        if (!idx_) return out;  // empty index => empty answers (src/hnsw.rs:1498-1503)
        std::vector<uint64_t> ids(nq * knbn);
        std::vector<float> dists(nq * knbn);
        std::vector<uint8_t> layers(nq * knbn);
        std::vector<int32_t> ranks(nq * knbn);
        std::vector<uint32_t> counts(nq);
        check(hnswgpu_search_batch(idx_, q, nq, d, knbn, ef, ids.data(), dists.data(), layers.data(), ranks.data(), counts.data()));
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) {
                const size_t o = i * knbn + j;
                out[i].push_back(Neighbour{(size_t)ids[o], dists[o], PointId{layers[o], ranks[o]}});
            }
        return out;
    }
    hnswgpu_index* idx_ = nullptr;
    hnswgpu_build_params params_{};
};

// HnswIo::new(directory, basename)
class HnswIo {
public:
    HnswIo(std::string directory, std::string basename) : dir_(std::move(directory)), basename_(std::move(basename)) {}
    const std::string& get_basename() const { return basename_; }
    // load_hnsw::<f32, D>(): the dump's distance must match D by its short name (src/hnswio.rs:473-490)
    template <class T, class D>
    Hnsw<T, D> load_hnsw() const {
        hnswgpu_index* idx = nullptr;
        check(hnswgpu_load_dump(dir_.c_str(), basename_.c_str(), D::code, &idx));
        return Hnsw<T, D>(idx);
    }

private:
    std::string dir_, basename_;
};

}  // namespace hnsw_rs
