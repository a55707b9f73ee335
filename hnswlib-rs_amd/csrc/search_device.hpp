// search_device.hpp -- HBM replica of a FlatIndex and the batched-search driver (host API of
// search_device.hip).  Everything here needs a gfx950 device; there is no CPU fallback.
#pragma once
#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include "builder.hpp"
#include "f16_storage.hpp"
#include "flat_index.hpp"

// In front of every function that capi.cpp calls but a host-only build of the C ABI does not hold (the sanitizer build, whose source list
// is fixed, links capi.cpp against stand-ins for the device that stop at the entries that existed when they were written).  capi.cpp
// defines HNSWGPU_WEAK_DEVICE_SIDE ahead of its includes: its references are weak, so it links without the .hip unit behind them,
// finds the function's address null and answers "no device" -- after the argument checks, which are the same everywhere.  Everywhere
// else (the units that define these functions, the stand-ins) this is nothing, and the definitions are strong.
#ifdef HNSWGPU_WEAK_DEVICE_SIDE
#define HNSWGPU_DEVICE_SIDE __attribute__((weak))
#else
#define HNSWGPU_DEVICE_SIDE
#endif

namespace hnswgpu {

constexpr int ARITH_SCALAR = 0, ARITH_SIMD8 = 1;  // DeviceIndex::set_arithmetic

// The HNSWGPU_* tuning / test hooks.  The environment is read ONCE per process (at the first use) -- not on every launch --
// and again only when the caller says it changed it (hnswgpu_reload_env; the tests do).  -1 / false: not set.
struct Knobs {
    int hash_bits = -1;          // HNSWGPU_HASH_BITS: initial visited-table size (6..14)
    bool no_sched = false;       // HNSWGPU_NO_SCHED: searches in input order
    bool no_pair_descent = false;  // HNSWGPU_NO_PAIR_DESCENT: one query per wavefront in the descent kernel whatever the index
    bool no_inkernel = false;    // HNSWGPU_NO_INKERNEL: strict ties resolved by the literal kernel only
    bool no_shape = false;       // HNSWGPU_NO_SHAPE: every search launch on the kernel that takes row stride and ef at run time (SHAPE_ANY), also where
                                 // the fixed-shape kernel applies (A/B switch and test hook: the answers are the same)
    int strict_wg_per_cu = -1;   // HNSWGPU_STRICT_WG_PER_CU
    int cand_lds = -1;           // HNSWGPU_CAND_LDS
    int waves_per_cu = -1;       // HNSWGPU_WAVES_PER_CU
    int exact_first = -1;        // HNSWGPU_EXACT_FIRST (test hook)
    bool trace_launch = false;   // HNSWGPU_TRACE_LAUNCH: one line per kernel launch of a search call
    bool trace_shape = false;    // HNSWGPU_TRACE_LAUNCH=2 (or more): also a "[hnswgpu shape]" line behind the line of every launch of the one-query kernels
    bool trace_host = false;     // HNSWGPU_TRACE_HOST
    int host_threads = -1;       // HNSWGPU_HOST_THREADS
    int host_chunks = -1;        // HNSWGPU_HOST_CHUNKS
    bool ffi_unpack = false;     // HNSWGPU_FFI_UNPACK
    int pair_search = -1;        // HNSWGPU_PAIR_SEARCH: 1 / 0 = two queries per wavefront as the first pass of a batch where the index allows it / never
                                 // (unset: strict DistCosine / DistDot batches of >= 40 000 queries on rows of one 128-byte line)
    int pair_tbits_delta = 0;    // HNSWGPU_PAIR_TBITS_DELTA: the pair kernel's visited tables, in powers of two relative to the one-query kernels'
    int pair_wg_per_cu = -1;     // HNSWGPU_PAIR_WG_PER_CU: cap on its resident workgroups per CU
    int build_wg = -1;           // HNSWGPU_BUILD_WG (test hook): cap on the workgroups of the two construction kernels, so that one wavefront handles many points of a window
    int build_hash_bits = -1;    // HNSWGPU_BUILD_HASH_BITS (test hook): the construction search's visited-table size (clamped like the default)
    int64_t filter_set_bytes = -1;  // HNSWGPU_FILTER_SET_MB (MiB, may be a fraction): bound on the bitmaps one launch of a filter-set search holds (unset: 256 MiB)
    int bitmap_slices = -1;      // HNSWGPU_BITMAP_SLICES (test hook): cap on the HBM visited-bitmap slices of a search launch, in place of what 4 GiB hold (1 ..; the
                                 // pair pass keeps its floor of 2) -- workgroups without a slice hand their overflowing queries back, and the call relaunches
    int literal_cand_cap = -1;   // HNSWGPU_LITERAL_CAND_CAP (test hook): cap on the candidate-heap capacity of the literal kernel's FIRST pass (64 ..; unset:
                                 // min(n, 2^17)) -- queries that outgrow it go through its second pass, which has room for every point
    int max_wg = -1;             // HNSWGPU_MAX_WG (test hook): absolute cap on the workgroups of every persistent launch of a search call (descent, pair pass,
                                 // one-query kernels, literal kernel), applied behind every other bound (1 ..) -- a workgroup then answers many queries in turn
    int64_t range_hits_per_pass = -1;  // HNSWGPU_RANGE_HITS_PER_PASS (test hook): the answers one fill pass of the exact range search holds (1 .. 2^31; unset: 8 Mi) --
                                 // a small batch's chunk plan then takes several turns; a query with more answers still gets a pass of its own
    int64_t graph_chunk = -1;    // HNSWGPU_GRAPH_CHUNK (test hook): the points one chunk of hnswgpu_graph_search_batch gathers and searches at most (1 ..; unset: what
                                 // its 256 MiB of queries and staged answers hold)
    int64_t range_chunk = -1;    // HNSWGPU_RANGE_CHUNK (test hook): the queries one group of hnswgpu_range_search_batch serves at most (1 ..; unset: as many as
                                 // keep a round's staged answers and the group's held answers within 256 MiB each)
    int poison_scratch = -1;     // HNSWGPU_POISON_SCRATCH (test hook, host code only): 0 .. 255 = every device scratch block is filled with this byte where it
                                 // passes from nobody's to a call's -- a fresh allocation, a pooled workspace or exact-unit block as it is taken, the builder
                                 // backend's scratch per window -- and the host waits for the fill (hip_host.hpp: poison_scratch).  Replica data, caller
                                 // buffers and pinned staging are never filled.  Unset or out of range: off, no HIP call more on any path
};
const Knobs& knobs();
void reload_knobs();

// Plain-pointer view handed to the kernels by value.
struct DeviceIndexView {
    const float* vec;          // [n][row_stride] f32, rows zero-padded to 128-byte lines -- or, on a STORAGE_F16 replica, as many
                               // binary16 elements behind the same pointer (64-byte lines; only the *_F16 kernels read them)
    const uint32_t* nbr0;      // [n][deg_stride] flat ids of the SEARCH layer's lists, padded with NO_POINT
    const uint32_t* up_ptr;    // [n_up_layers][n+1] CSR offsets of the lists at layers >= 1
    const uint32_t* up_ids;    // concatenated lists of layers 1..n_up_layers (list order = file order)
    const uint64_t* origin_id; // [n]
    uint32_t n;
    uint32_t d;
    uint32_t row_stride;       // floats per row, multiple of 32
    uint32_t deg_stride;       // ids per nbr0 row, multiple of 16
    uint32_t n_up_layers;      // highest layer index holding any non-empty list
    uint32_t entry;            // flat id of the entry point
    uint32_t entry_level;      // its layer
    uint32_t search_layer;     // lowest non-empty layer (src/hnsw.rs:1534-1540)
    uint32_t layer_offset[NB_LAYER_MAX + 1];
};

// What a search call reports about itself (the timings are HIP events on the launch stream).
struct CallInfo {
    double ms = 0.0;         // all kernels of the call
    double main_ms = 0.0;    // first launch of the search kernel alone
    uint32_t launches = 0;
    uint32_t ties = 0;       // queries whose answer depended on the reference's heap order (resolved or flagged)
    uint32_t pair_retries = 0;  // queries the two-per-wavefront first pass handed back to the one-query kernels
    uint32_t panics = 0;     // filtered search: queries on which the reference panics (src/hnsw.rs:973)
};

// One replica of an index in the HBM of one device.  The replica is immutable after upload(); every search call takes
// a private workspace (scratch buffers, events, counters) from a pool, so concurrent calls on one replica are legal --
// like the reference's `&self` search (SURVEY.md 8b "Threading").
// Where answer j of query q is written, in bytes from the three base addresses a search is given: ids at (q k + j) id_stride,
// distances at (q k + j) dist_stride, counts at q count_stride.  The default is three dense arrays; {16, 16, 16} addresses the
// records of the reference's FFI in place (Neighbour_api {usize id; f32 d}, Neighbourhood_api {i64 nbgh; ptr}: src/libext.rs:58-87).
struct OutLayout {
    uint32_t id_stride = 8, dist_stride = 4, count_stride = 4;
};
// Host memory every device of the process can address (mapped, portable, page-locked): *dev receives the address the kernels
// use.  nullptr when the runtime refuses (no device, limits): the caller falls back to ordinary memory and an unpacking pass.
void* pinned_alloc(size_t bytes, void** dev);
void pinned_free(void* p);

// A set of filters for one batch, in CSR form: filter f is the SORTED id vector ids[offsets[f] .. offsets[f + 1]) (offsets[0] == 0,
// ascending, n_filters + 1 of them; an empty range allows nothing), and query q is searched under filter filter_of[q] < n_filters.
struct FilterSet {
    const uint64_t* ids;
    const uint64_t* offsets;
    uint64_t n_filters;
    const uint32_t* filter_of;  // [nq]
};
class DeviceIndex;
// Hnsw::search_filter(data_q, knbn, ef, Some(&filters[filter_of[q]])) for every query q of a batch (search_device.hip).  capi.cpp
// refers to these two weakly: a host-only build of the C ABI (the sanitizer build, whose source list is fixed) links without
// them and answers "no device", what every device entry answers there (HNSWGPU_DEVICE_SIDE).
// Every buffer in device memory: like DeviceIndex::search_device with a filter.  The arrays cannot be read on the host, so a kernel
// counts the entries of filter_of that are >= n_filters and the call returns ERR_ARG, nothing written, before the search is launched;
// the offsets and the sortedness of the vectors are the caller's promise.
HNSWGPU_DEVICE_SIDE int search_filter_set_device(DeviceIndex& ix, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, const FilterSet& d_set,
                             uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                             uint32_t* d_stats, void* stream, CallInfo* info, std::string& err);
// Host buffers (the set too, already validated): like DeviceIndex::search_host.
HNSWGPU_DEVICE_SIDE int search_filter_set_host(DeviceIndex& ix, const float* queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, const FilterSet& set,
                           uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts,
                           uint8_t* out_status, CallInfo* info, std::string& err);

class DeviceIndex {
public:
    DeviceIndex();
    ~DeviceIndex();
    DeviceIndex(const DeviceIndex&) = delete;
    DeviceIndex& operator=(const DeviceIndex&) = delete;

    // How the next upload() stores the rows: STORAGE_F32 (default), or STORAGE_F16 -- binary16 rows converted on the host (no f32
    // copy of the matrix ever reaches the device), DistL2 / DistCosine / DistDot / DistL1 only, every element representable (else
    // upload() returns ERR_ARG; the C ABI has verified it before).  The search then runs the KM_*_F16 kernels: the same arithmetic
    // on the same f32 values, so the same answers bit for bit.  Whatever reads view().vec outside the search path must ask storage().
    void set_storage(int s) { storage_ = s == STORAGE_F16 ? STORAGE_F16 : STORAGE_F32; }
    int storage() const { return storage_; }
    int upload(const FlatIndex& x, int device, std::string& err);
    bool ready() const { return ready_; }
    int device() const { return device_; }
    int dist() const { return dist_; }
    const DeviceIndexView& view() const { return v_; }
    uint64_t bytes() const { return bytes_; }

    // Hnsw::parallel_search on device-resident buffers.  d_queries: nq x d row-major.
    // d_allowed != nullptr: Hnsw::search_filter with the sorted id vector d_allowed[0..n_allowed) (device memory) for
    // every query of the batch (src/hnsw.rs:1487-1580, src/filter.rs:11-15).
    // feed (may be null): d_queries is mapped pinned host memory that is still being filled -- fill(ctx, lo, hi) makes rows
    // [lo, hi) valid; the call then gathers and launches the descent kernel chunk by chunk, so that the device reads chunk i
    // across PCIe while the host gathers chunk i + 1 (the host-buffer entry points).
    struct RowFeed {
        void (*fill)(void* ctx, uint64_t lo, uint64_t hi);
        void* ctx;
        uint64_t chunk_rows;  // rows per chunk (the feeder's choice: its gather tasks are cut along these)
    };
    // `layout`: where the answers go relative to d_out_ids / d_out_dists / d_out_counts (OutLayout; default: dense arrays)
    int search_device(const float* d_queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, uint64_t* d_out_ids,
                      float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                      uint32_t* d_stats, void* stream, const uint64_t* d_allowed, uint64_t n_allowed, CallInfo* info,
                      std::string& err, const RowFeed* feed = nullptr, OutLayout layout = OutLayout{});
    // same with host buffers (H2D + kernels + D2H); out_status (may be null): per query, 1 = the reference panics
    int search_host(const float* queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, uint64_t* out_ids,
                    float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts,
                    const uint64_t* allowed, uint64_t n_allowed, bool filtered, uint8_t* out_status, CallInfo* info,
                    std::string& err);
    // What search_host is made of, for callers with other shapes of input / output (the reference's FFI: an array of row
    // pointers in, per-query vectors out).  Queries come from `queries` (nq x d) or, when that is null, from rows[0..nq).
    // ONE section of the worker pool lasts the whole call: its threads gather the rows into mapped pinned memory (the descent
    // kernel reads them across PCIe, chunk by chunk, while the next chunk is gathered), stay awake while the device searches,
    // and unpack the answers the kernels wrote into a pinned arena -- a pool thread takes ~50 us to wake up, which a call of
    // 1.2 ms cannot afford twice.  sink.begin (may be null) runs before anything else, on the caller's thread (allocate);
    // sink.rows unpacks the answers of queries [lo, hi) and is called concurrently on disjoint ranges; the HostAnswers are
    // valid only during the call.
    struct HostAnswers {
        const uint64_t* ids;      // [nq][k]
        const float* dists;       // [nq][k]
        const uint8_t* layer;     // [nq][k]
        const int32_t* rank;      // [nq][k]
        const uint32_t* counts;   // [nq]
        const uint8_t* status;    // [nq] filtered search: 1 = the reference panics on this query (else nullptr)
    };
    // A sink whose own memory the device can address (pinned_alloc) may take the answers IN PLACE: `direct` (may be null; called
    // after begin) names the allocation and, inside it, the first id / distance / count slot (host addresses) with their strides
    // and returns true -- the kernels then write there (the device's view of the allocation is looked up per call, on the
    // index's device), rows() is never called and nothing is unpacked (no layer / rank / status).
    struct DirectOut {
        void* allocation;   // what pinned_alloc returned
        void* ids;
        void* dists;
        void* counts;
        OutLayout layout;
    };
    struct AnswerSink {
        bool (*begin)(void* ctx, uint64_t nq, uint64_t k);  // false: out of memory
        void (*rows)(void* ctx, const HostAnswers& a, uint64_t lo, uint64_t hi);
        void* ctx;
        bool (*direct)(void* ctx, DirectOut* out) = nullptr;
    };
    int search_host_staged(const float* queries, const float* const* rows, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef,
                           const uint64_t* allowed, uint64_t n_allowed, bool filtered, bool want_status, const AnswerSink& sink,
                           CallInfo* info, std::string& err);

    // The arithmetic of Distance::eval: ARITH_SCALAR (default) sums like the crate's default build, left to right, bit for
    // bit; ARITH_SIMD8 sums DistL2 / DistCosine / DistDot / DistL1 in the order of its simdeez_f / stdsimd builds (8 vertical
    // accumulators, Cargo.toml:104-111) -- the order behind the reference's published numbers; other distances stay scalar.
    void set_arithmetic(int a) { arith_.store(a == ARITH_SIMD8 ? ARITH_SIMD8 : ARITH_SCALAR); }
    int arithmetic() const { return arith_.load(); }
    // strict ties: decisions that depend on the reference's heap order are resolved with literal heaps
    void set_strict_ties(bool on) { strict_ties_.store(on); }
    bool strict_ties() const { return strict_ties_.load(); }
    CallInfo last_call() const;
    // DistCosine: the side array of per-point squared norms (f64), or nullptr when every row carries its norm in the last
    // 8 bytes of its own padding (norm_fits_row) -- what SearchArgs::nrm2 is given
    const double* side_norms() const { return static_cast<const double*>(d_nrm2_); }
    // Per-replica state of another translation unit (exact_knn.hip: the DataId ranks of the points and its scratch pool),
    // made at first use by make() (null: failed, asked again next time) and dropped with the replica.
    template <class MAKE>
    std::shared_ptr<void> extension(MAKE&& make) const {
        std::lock_guard<std::mutex> g(ext_mu_);
        if (!ext_) ext_ = make();
        return ext_;
    }

private:
    friend int search_filter_set_device(DeviceIndex&, const float*, uint64_t, uint64_t, uint64_t, uint64_t, const FilterSet&, uint64_t*, float*,
                                        uint8_t*, int32_t*, uint32_t*, uint32_t*, void*, CallInfo*, std::string&);
    friend int search_filter_set_host(DeviceIndex&, const float*, uint64_t, uint64_t, uint64_t, uint64_t, const FilterSet&, uint64_t*, float*,
                                      uint8_t*, int32_t*, uint32_t*, uint8_t*, CallInfo*, std::string&);
    struct Workspace;
    class Lease;
    Workspace* acquire(std::string& err);
    void release_ws(Workspace* w);
    void release();
    // what search_device / search_host_staged / search_host and their filter-set counterparts share (search_device.hip): where a
    // call's answers go, its filter (none, one id vector, a FilterSet), and the steps of one call with what they hand to each other
    struct AnswerBufs; struct CallFilter; struct SearchCall;
    int search_device_impl(const float* d_queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, const AnswerBufs& out, void* stream,
                           const CallFilter& filter, CallInfo* info, std::string& err, const RowFeed* feed);
    int search_host_staged_impl(const float* queries, const float* const* rows, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef,
                                const uint64_t* allowed, uint64_t n_allowed, bool filtered, const FilterSet* set, bool want_status,
                                const AnswerSink& sink, CallInfo* info, std::string& err);
    int search_host_impl(const float* queries, uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dists,
                         uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts, const uint64_t* allowed, uint64_t n_allowed,
                         bool filtered, const FilterSet* set, uint8_t* out_status, CallInfo* info, std::string& err);

    DeviceIndexView v_{};
    bool ready_ = false;
    int device_ = -1;
    int dist_ = DIST_L2;
    int storage_ = STORAGE_F32;   // of the rows at d_vec_ (fixed by upload())
    int num_cu_ = 0;
    size_t lds_limit_ = 0;  // hipDeviceAttributeMaxSharedMemoryPerBlock of the replica's device: what a workgroup's LDS may add up to
    uint64_t bytes_ = 0;
    // the replica (read-only after upload)
    void* d_vec_ = nullptr;
    void* d_nbr0_ = nullptr;
    void* d_up_ptr_ = nullptr;
    void* d_up_ids_ = nullptr;
    void* d_origin_ = nullptr;
    void* d_nrm2_ = nullptr;      // DistCosine: per-point squared norms (f64)
    // per-call workspaces
    std::mutex pool_mu_;
    std::vector<std::unique_ptr<Workspace>> all_ws_;
    std::vector<Workspace*> free_ws_;
    // what previous batches taught us (visited-table sizing per ef), and the last call's report
    mutable std::mutex meta_mu_;
    uint64_t adapt_ef_ = 0;
    uint32_t adapt_tbits_ = 0;
    CallInfo last_{};
    std::atomic<bool> strict_ties_{true};
    std::atomic<int> arith_{0};
    int kernel_metric() const;            // dist_, or its SIMD-order / half-storage kernel variant
    std::atomic<int> descend_per_cu_[2] = {{0}, {0}};  // resident workgroups per CU of the descent kernel (asked once; [1]: two queries per wavefront)
    std::vector<std::pair<uint64_t, int>> search_per_cu_;  // ... of the one-query search kernels, per (kernel, LDS bytes): asked once each (under meta_mu_)
    uint32_t up_deg_max_ = 0;  // longest list above the search layer
    mutable std::mutex ext_mu_;
    mutable std::shared_ptr<void> ext_;  // see extension()
};

int device_count();
// The gather of a sharded search without any collective library: shard s's answers (nq_shard[s] x k, resident on
// devices[s]) are copied behind one another -- input order -- into the arrays of `root_device` with hipMemcpyPeerAsync on
// `root_stream` (xGMI between the GPUs of a node, a device-to-device copy when a shard lives on the root), then the stream is
// waited for.  layer / rank arrays and their per-shard entries may be null.
int gather_sharded_answers(const int* devices, int n_shards, const uint64_t* nq_shard, uint64_t k, const uint64_t* const* d_ids,
                           const float* const* d_dists, const uint8_t* const* d_layer, const int32_t* const* d_rank,
                           const uint32_t* const* d_counts, int root_device, uint64_t* root_ids, float* root_dists,
                           uint8_t* root_layer, int32_t* root_rank, uint32_t* root_counts, void* root_stream, std::string& err);
// the device side of GPU-assisted construction (builder.hpp) on HIP device `device`
std::unique_ptr<BuildSearchBackend> make_device_build_backend(int device);
// Distance<f32>::eval on the device through the search kernel's own distance routine: out[q][r] = dist(queries[q],
// rows[r]), rows evaluated in batches of `nf` (1..64) -- the lane-group branches the search takes for nf neighbours.
// pairs: nq == n and out[i] = dist(queries[i], rows[i]) (nf ignored).
// eval_distance_matrix_storage_device (matrix mode, scalar arithmetic; capi.cpp refers to it weakly, like the filter-set pair above),
// storage == STORAGE_F16: `rows` (every element representable, else ERR_ARG) are narrowed to binary16 on the host and read by the
// half-storage kernels, as a STORAGE_F16 replica's are (scalar arithmetic, DistL2 / DistCosine / DistDot / DistL1).
int eval_distance_matrix_device(int dist, const float* queries, uint64_t nq, const float* rows, uint64_t n, uint64_t d,
                                uint32_t nf, bool pairs, float* out, std::string& err, int arithmetic = 0);
HNSWGPU_DEVICE_SIDE int eval_distance_matrix_storage_device(int dist, int storage, const float* queries, uint64_t nq, const float* rows, uint64_t n, uint64_t d,
                                        uint32_t nf, float* out, std::string& err);
// the same through one of the row loops that only the search kernel's expansion loop compiles (variant: EVAL_* of
// search_kernels.hpp, a combination that exists -- else ERR_ARG, never the plain routine); referred to weakly by capi.cpp too
HNSWGPU_DEVICE_SIDE int eval_distance_matrix_variant_device(int dist, int storage, int variant, const float* queries, uint64_t nq, const float* rows, uint64_t n,
                                        uint64_t d, uint32_t nf, float* out, std::string& err);

// The lane lab (search_kernels.hpp, lane_lab.inc): runs a script of wave-level operations of the search kernels on `device`
// (host buffers in, host buffer out; out[0] = words produced).  Test entry.
int lane_lab_device(int device, uint32_t mode, uint32_t p0, uint32_t p1, uint32_t p2, const uint32_t* ops, uint32_t n_ops,
                    const uint32_t* lanes, uint32_t n_lane_sets, uint32_t* out, uint32_t out_words, std::string& err);

}  // namespace hnswgpu
