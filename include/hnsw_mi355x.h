/* hnsw_mi355x.h -- C ABI of libhnsw_mi355x.so
 *
 * MI355X-native drop-in for ONE hot path of the Rust crate hnsw_rs 0.3.4
 * (jean-pierreBoth/hnswlib-rs): the batched k-NN search
 *   AnnT::parallel_search_neighbours          src/api.rs:58-65
 *   -> Hnsw::parallel_search                  src/hnsw.rs:1612-1635
 *   -> Hnsw::search_filter(filter = None)     src/hnsw.rs:1487-1580
 *   -> Hnsw::search_layer                     src/hnsw.rs:922-1064
 *   -> Distance<f32>::eval (DistL2/DistCosine/DistDot/DistL1, crate anndists 0.1)
 * together with the hnswio dump format on either side of it (src/hnswio.rs).
 *
 * Two groups of entry points:
 *   (1) hnswgpu_*  : the thin ABI a Rust `impl AnnT` wrapper (or any host) binds; flat
 *                    row-major matrices in, flat arrays out, integer status codes.
 *   (2) the reference's own f32 C symbols (src/libext.rs), name- and layout-compatible,
 *                    implemented on top of (1) -- existing C / Julia callers relink as is.
 *
 * All pointers are plain host pointers unless the name says `_device`.  No function aborts
 * the process (the reference calls process::exit / panics): failures
 * return a status / NULL and hnswgpu_last_error() explains.
 * The search entry points REQUIRE a gfx950 device: there is no CPU fallback.
 */
#ifndef HNSW_MI355X_H
#define HNSW_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status codes ------- */
enum {
    HNSWGPU_OK = 0,
    HNSWGPU_ERR_ARG = 1,      /* bad argument (null, dimension mismatch, ...)             */
    HNSWGPU_ERR_IO = 2,       /* cannot open / read / write a dump file                   */
    HNSWGPU_ERR_FORMAT = 3,   /* bad magic, truncated file, incoherent ids                */
    HNSWGPU_ERR_DISTANCE = 4, /* dump's distance name differs from the one asked          */
    HNSWGPU_ERR_TYPE = 5,     /* dump's element type is not "f32"                         */
    HNSWGPU_ERR_DEVICE = 6,   /* HIP error, or no gfx950 device / index not uploaded      */
    HNSWGPU_ERR_EMPTY = 7,    /* operation needs a non-empty index                        */
    HNSWGPU_ERR_REF_PANIC = 8, /* filtered search: the reference panics on some of the queries
                                 (src/hnsw.rs:973) and no per-query status array was given  */
    HNSWGPU_ERR_CAPACITY = 9  /* range search: the answers need more slots than `cap`; the offsets
                                 are complete; exact call: no out slot was written; approximate
                                 call (hnswgpu_range_search_batch): the out slots are unspecified */
};

/* metric selector == short type name of the anndists distance */
enum {
    HNSWGPU_DIST_L2 = 0,     /* anndists::dist::distances::DistL2     sqrt(sum (a-b)^2)   */
    HNSWGPU_DIST_COSINE = 1, /* ...::DistCosine   1 - a.b/sqrt(|a|^2 |b|^2), f64 sums     */
    HNSWGPU_DIST_DOT = 2,    /* ...::DistDot      1 - a.b (inputs pre-normalised)         */
    HNSWGPU_DIST_L1 = 3,     /* ...::DistL1       sum |a-b|                               */
    /* distances between probability vectors (the f32 arms of src/libext.rs:334-345, :491-513)        */
    HNSWGPU_DIST_HELLINGER = 4,     /* ...::DistHellinger      sqrt(max(1 - sum sqrt(a) sqrt(b), 0))          */
    HNSWGPU_DIST_JEFFREYS = 5,      /* ...::DistJeffreys       sum (a-b) ln(max(a,1e-30)/max(b,1e-30))        */
    HNSWGPU_DIST_JENSENSHANNON = 6  /* ...::DistJensenShannon  sqrt(0.5 sum [a ln(a/m) + b ln(b/m)]), m=(a+b)/2 */
};

typedef struct hnswgpu_index hnswgpu_index; /* opaque: flat host graph + its HBM replica  */

/* Thread-local message for the last failing call on this thread. */
const char* hnswgpu_last_error(void);

/* ---------------------------------------------------------------- load / dump -------- */
/* HnswIo::new(dir, basename) + load_hnsw::<f32, D>()        src/hnswio.rs:317, :431-524
 * `dist` = HNSWGPU_DIST_* the caller asks for (checked against the dump's distname by the
 * short-name rule of src/hnswio.rs:473-490), or -1 to accept whatever the dump says.     */
int hnswgpu_load_dump(const char* dir, const char* basename, int dist, hnswgpu_index** out);

/* AnnT::file_dump(path, basename) in DumpMode::Full           src/api.rs:70-93,
 * src/hnswio.rs:1355-1387.  Overwrites existing files (no unique-name logic).            */
int hnswgpu_file_dump(const hnswgpu_index* idx, const char* dir, const char* basename);

void hnswgpu_free_index(hnswgpu_index* idx);

/* Description of a dump (load_description, src/hnswio.rs:937-1042).                       */
typedef struct {
    uint32_t format_version; /* 2, 3 or 4 (from the magic)                                */
    uint8_t dumpmode;        /* 1 = Full                                                  */
    uint8_t max_nb_connection;
    uint8_t nb_layer;
    double level_scale;
    uint64_t ef_construction;
    uint64_t nb_point;
    uint64_t dimension;
    char distname[260];
    char t_name[260];
} hnswgpu_description;
int hnswgpu_load_description(const char* graph_file_path, hnswgpu_description* out);
int hnswgpu_get_description(const hnswgpu_index* idx, hnswgpu_description* out);

/* ---------------------------------------------------------------- DataMap ------------ */
/* DataMap (src/datamap.rs:24-319): the vectors of a dump memory-mapped and addressed by DataId, without loading the
 * graph.  open = DataMap::from_hnswdump::<f32>(dir, basename) (:44-231; dumps of format > 2 whose type is f32; where
 * the reference exits the process on a missing file this returns HNSWGPU_ERR_IO); get_data = get_data::<f32>(&id)
 * (:276-297): a pointer to `dimension` floats inside the mapping, valid until close, NULL for an unknown id;
 * ids = get_dataid_iter (:301): the ids in file order (returns their number; fills at most cap).                    */
typedef struct hnswgpu_datamap hnswgpu_datamap;
int hnswgpu_datamap_open(const char* dir, const char* basename, hnswgpu_datamap** out);
void hnswgpu_datamap_close(hnswgpu_datamap* m);
const float* hnswgpu_datamap_get_data(const hnswgpu_datamap* m, uint64_t data_id);
uint64_t hnswgpu_datamap_nb_data(const hnswgpu_datamap* m);
uint64_t hnswgpu_datamap_dimension(const hnswgpu_datamap* m);
const char* hnswgpu_datamap_distname(const hnswgpu_datamap* m);
const char* hnswgpu_datamap_typename(const hnswgpu_datamap* m);
uint64_t hnswgpu_datamap_ids(const hnswgpu_datamap* m, uint64_t* out, uint64_t cap);

/* ---------------------------------------------------------------- construction ------- */
/* Hnsw::<f32, D>::new(max_nb_connection, max_elements, max_layer, ef_construction, D)
 * + (parallel_)insert of n points (src/hnsw.rs:771, :1077-1215, :1224-1238).  Construction on
 * the host cores, or GPU-assisted (gpu_device); levels come from the documented
 * SplitMix64(397) stream.                                                */
typedef struct {
    uint64_t max_nb_connection; /* M; layer-0 lists hold up to 2M                         */
    uint64_t ef_construction;
    uint64_t max_layer;         /* clamped to 16; must be 16 for the index to be dumpable */
    int dist;                   /* HNSWGPU_DIST_*                                         */
    double level_scale_factor;  /* modify_level_scale(), in [0.2, 1]; 1.0 = default       */
    int extend_candidates;      /* set_extend_candidates()                                */
    int keep_pruned;            /* set_keeping_pruned()                                   */
    int nthreads;               /* 1 = serial insert (deterministic); 0 = all host cores  */
    int fast_arithmetic;        /* 0: reference-order scalar sums; 1: 8-lane SIMD sums
                                   (the crate's `simdeez_f` build order)                  */
    int gpu_assist;             /* 1: GPU-assisted construction: the searches of every insertion
                                   (src/hnsw.rs:1114-1197) run on HIP device gpu_device, window by window against a
                                   frozen snapshot of the graph; select_neighbours, list and reverse updates on the
                                   host cores.  0 (default): host only.  Device distances are reference-order.      */
    int gpu_device;
    uint64_t gpu_window;        /* points per window at most (0 = 16384); windows grow with the graph
                                   (max(256, inserted / 8)); 1 = one point at a time: the serial insertion, exactly */
} hnswgpu_build_params;
int hnswgpu_build(const float* data, uint64_t n, uint64_t d, const uint64_t* ids /* NULL: 0..n-1 */,
                  const hnswgpu_build_params* params, hnswgpu_index** out);
/* Hnsw::insert / parallel_insert of n more points into ANY index (src/hnsw.rs:1068-1075, :1224-1238), including one
 * obtained from hnswgpu_load_dump: like the reference's reloaded Hnsw it keeps growing (M, ef_construction and the
 * level scale come from the dump; extend_candidates = true, keep_pruned = false as src/hnswio.rs:510-511 sets them;
 * the reference's reload quirk of treating the dumped absolute level scale as a factor, src/hnswio.rs:773-777, is
 * kept).  nthreads: 1 = serial, 0 = all host cores.  HBM replicas are refreshed by the next search / upload.           */
int hnswgpu_insert(hnswgpu_index* idx, const float* data, uint64_t n, uint64_t d, const uint64_t* ids /* NULL: continue */,
                   int nthreads);
/* the same, GPU-assisted (see hnswgpu_build_params.gpu_assist / gpu_device / gpu_window).  What can be refused up front (no
 * device, bad ordinal, ef_construction > 1024, wrong dimension) is refused before a point is accepted: the index is then
 * unchanged and a retry is safe.  A device failure AFTER the points were accepted (allocation, copy, kernel) does not lose
 * them: the host builder links the rest of the batch, the call returns HNSWGPU_OK and hnswgpu_last_error() holds the device's
 * message as a warning.  Either way hnswgpu_nb_point() counts fully linked points only.                                    */
int hnswgpu_insert_gpu(hnswgpu_index* idx, const float* data, uint64_t n, uint64_t d, const uint64_t* ids, int nthreads,
                       int gpu_device, uint64_t gpu_window);

/* ---------------------------------------------------------------- inspection --------- */
uint64_t hnswgpu_nb_point(const hnswgpu_index* idx);
uint64_t hnswgpu_dimension(const hnswgpu_index* idx);
int hnswgpu_dist(const hnswgpu_index* idx);
uint64_t hnswgpu_layer_nb_point(const hnswgpu_index* idx, unsigned layer);
int hnswgpu_max_level_observed(const hnswgpu_index* idx);
/* entry point as (origin_id, layer, rank); returns HNSWGPU_ERR_EMPTY on an empty index    */
int hnswgpu_entry_point(const hnswgpu_index* idx, uint64_t* origin_id, uint8_t* layer, int32_t* rank);
/* neighbour list of point (layer, rank) at layer `l`: fills up to cap entries, returns the
 * list length (or -1).  Order = stored order (ascending stored distance).                 */
int64_t hnswgpu_neighbours(const hnswgpu_index* idx, unsigned layer, int32_t rank, unsigned l, uint64_t cap,
                           uint64_t* origin_ids, uint8_t* layers, int32_t* ranks, float* dists);

/* ---------------------------------------------------------------- HBM replica -------- */
/* Copies vectors (rows padded to 128-byte lines) and neighbour lists into the HBM of HIP
 * device `device`.  Idempotent.  A handle may hold replicas on several devices (one upload
 * each); the last device uploaded explicitly is the PRIMARY one, used by the single-device
 * search entry points.  Replicas are immutable; they are dropped when the graph changes.    */
int hnswgpu_upload(hnswgpu_index* idx, int device);
int hnswgpu_device_count(void);

/* ---------------------------------------------------------------- search ------------- */
/* Hnsw::parallel_search(datas, knbn, ef) for a flat nq x d row-major query matrix
 * (src/hnsw.rs:1612-1635).  Row i of the outputs holds out_counts[i] <= k valid entries in
 * ascending distance: Neighbour{d_id, distance, p_id(layer, rank)} (src/hnsw.rs:98-107).
 * out_layer / out_rank may be NULL.  Host buffers; includes H2D/D2H copies.               */
int hnswgpu_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                         uint64_t ef, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank,
                         uint32_t* out_counts);

/* Hnsw::search_filter(data, knbn, ef, Some(&Vec<usize>)) for every query of a batch (src/hnsw.rs:1487-1580; the filter
 * is `impl FilterT for Vec<usize>`, a binary search in a SORTED id vector, src/filter.rs:11-15 -- an unsorted vector is
 * HNSWGPU_ERR_ARG).  Same outputs as hnswgpu_search_batch.  The reference panics on some inputs (a filter that empties
 * return_points, then `peek().unwrap()`, src/hnsw.rs:973 -- only reachable with ef == 1): such a query gets count 0
 * and out_status[i] = 1 (0 otherwise); with out_status == NULL the call returns HNSWGPU_ERR_REF_PANIC instead (the other
 * queries' answers are valid).  Never aborts.                                                                      */
int hnswgpu_search_batch_filtered(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                  uint64_t ef, const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids,
                                  float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts,
                                  uint8_t* out_status);

/* A SET of filters for one batch, each query naming its own: query q is answered exactly as
 * Hnsw::search_filter(data_q, knbn, ef, Some(&filters[filter_of[q]])) -- ids, f32 distance bits, p_ids, counts, and the status of a
 * query on which the reference panics.  The vectors are given in CSR form: filter f is filter_ids[filter_offsets[f] ..
 * filter_offsets[f + 1]), sorted ascending like the vector of hnswgpu_search_batch_filtered; filter_offsets has n_filters + 1
 * entries, starts at 0 and ascends; filter_of[0..nq) < n_filters.  An empty vector is a filter that allows nothing.  There is no
 * "no filter" value: a query without a filter belongs in hnswgpu_search_batch.  HNSWGPU_ERR_ARG (the message names what is wrong):
 * a null buffer, n_filters == 0 with nq > 0, offsets that do not start at 0 or that descend, a vector that is not sorted (the
 * filter is named), a filter_of[q] >= n_filters.  out_status / HNSWGPU_ERR_REF_PANIC: as hnswgpu_search_batch_filtered.
 * The device holds one bitmap of ceil(nb_point / 32) words per filter; the bitmaps of one launch are bounded by
 * HNSWGPU_FILTER_SET_MB (MiB, default 256: ~2 000 filters at 1M points).  A larger set is served in groups of consecutive
 * filters -- bitmaps built, the group's queries listed, that list searched -- every query exactly once, the answers in the
 * caller's rows by q.  A bound below one bitmap is HNSWGPU_ERR_ARG.  One filter named by every query costs what
 * hnswgpu_search_batch_filtered costs, and answers the same.                                                              */
int hnswgpu_search_batch_filter_set(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                    uint64_t ef, const uint64_t* filter_ids, const uint64_t* filter_offsets,
                                    uint64_t n_filters, const uint32_t* filter_of, uint64_t* out_ids, float* out_dists,
                                    uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts, uint8_t* out_status);

/* Hnsw::parallel_search with the batch sharded over several GPUs of THIS process (BASELINE config 4 without Python or
 * a collective library): the graph is replicated on every device named in devices[0..n_shards) (uploaded on first use),
 * shard s = the s-th contiguous balanced block of queries (nq / n_shards each, the first nq % n_shards one more), one
 * host thread per shard, and every shard copies its answers straight into its rows of the caller's arrays -- that is
 * the gather.  A device may be named more than once (shards then share its replica and run concurrently).
 * Answers are identical to hnswgpu_search_batch on one device.                                                      */
int hnswgpu_search_batch_sharded(const hnswgpu_index* idx, const int* devices, int n_shards, const float* queries,
                                 uint64_t nq, uint64_t d, uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dists,
                                 uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts);
/* The same for a host that already holds its data in HBM: shard s searches nq_shard[s] queries that sit at d_queries[s] ON
 * devices[s] and leaves its answers in that device's d_out_*[s] arrays (nq_shard[s] x k; d_out_layer / d_out_rank and their
 * entries may be NULL) -- no PCIe traffic but the counters.  One host thread per shard; streams[s] (hipStream_t as void*,
 * may be NULL, the array too) is the stream shard s launches on.  Missing replicas are uploaded first, all devices at once.
 * What is exchanged afterwards (answers only: nq x k x 12 bytes) is the caller's collective, e.g. RCCL all-gather.         */
int hnswgpu_search_batch_sharded_device(const hnswgpu_index* idx, const int* devices, int n_shards, const float* const* d_queries,
                                        const uint64_t* nq_shard, uint64_t d, uint64_t k, uint64_t ef, uint64_t* const* d_out_ids,
                                        float* const* d_out_dists, uint8_t* const* d_out_layer, int32_t* const* d_out_rank,
                                        uint32_t* const* d_out_counts, void* const* streams);
/* The exchange that follows hnswgpu_search_batch_sharded_device when ONE process drives the node's GPUs and holds no collective
 * library (a Rust host): shard s's answers (nq_shard[s] x k on devices[s]) are copied behind one another -- input order, the order
 * Hnsw::parallel_search returns (src/hnsw.rs:1623-1633) -- into the arrays of root_device with hipMemcpyPeerAsync on root_stream
 * (xGMI between the GPUs of a node), and the stream is waited for.  1.2-1.7 MB per shard at BASELINE config 4.  d_layer / d_rank,
 * their entries and root_layer / root_rank may be NULL.                                                                       */
int hnswgpu_gather_sharded_answers(const int* devices, int n_shards, const uint64_t* nq_shard, uint64_t k,
                                   const uint64_t* const* d_ids, const float* const* d_dists, const uint8_t* const* d_layer,
                                   const int32_t* const* d_rank, const uint32_t* const* d_counts, int root_device,
                                   uint64_t* root_ids, float* root_dists, uint8_t* root_layer, int32_t* root_rank,
                                   uint32_t* root_counts, void* root_stream);

/* Same with every buffer already resident in HBM (device pointers), launched on HIP stream
 * `stream` (hipStream_t as void*; NULL = default stream).  Synchronises `stream` once
 * before returning (the visited-set overflow check needs one 4-byte read-back).
 * The stream contract, of this and of every other entry that takes a `stream` (the `_device` forms, _begin / _end, the gather): device
 * inputs are read and device outputs written in the order of `stream`, so work queued on `stream` before the call needs no host
 * wait, and when the call returns the stream has been waited for (tests/test_gpu_stream_order.py).
 * d_stats may be NULL, else uint32[nq*8] per query = {n_dist, n_expand, n_ids_read, status,
 * t_start, t_end (device wall clock, 10 ns ticks), used_hbm_bitmap, flags | (lists scanned by the greedy descent << 8) | (its n_dist << 16)}
 * (flags: 1 equal distances met, 2 a pop was taken from the literal candidate heap).  The work counters are the reference's,
 * query by query, whichever kernel or pass answered (Hnsw::search_filter, src/hnsw.rs:1487-1580, with search_layer :922-1064):
 *   n_dist     = calls of Distance::eval: the entry point (:1506), every id of every list the descent reads (:1518), the
 *                layer-0 entry point once more (:952; the device reuses the descent's value but counts it) and every
 *                neighbour not yet visited (:1026);
 *   n_expand   = neighbour lists read: one per layer above the search layer (:1515) and one per candidate popped and not
 *                ended by the stop rule (:981-993, :1006);
 *   n_ids_read = the ids of those lists;
 *   word 7 bits 8-15 / 16-31 = the descent's (:1506-1529, everything before search_layer) n_expand / n_dist; its ids read are
 *                its n_dist - 1.  The descent runs in a kernel of its own in front of the search kernel.
 * These are the oracle's per-query counters (orc_parallel_search_counted), which tests/test_gpu_counters.py compares them with.
 * status: 0 ok; 2 ok, but the answer depends on the reference's heap order and strict ties are off;
 * 3 ok, resolved with the literal heaps (strict ties; see DESIGN.md "ties").  ef above 1024 (the
 * register-resident result set) is served by the literal-heap kernel: correct, slower.          */
int hnswgpu_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                uint64_t k, uint64_t ef, uint64_t* d_out_ids, float* d_out_dists,
                                uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                                uint32_t* d_stats, void* stream);
/* hnswgpu_search_batch_filtered on device-resident buffers (the sorted id vector too).  d_stats[q*8+3] == 6 marks a
 * query on which the reference panics; *n_panics (may be NULL) counts them.                                        */
int hnswgpu_search_batch_filtered_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                         uint64_t k, uint64_t ef, const uint64_t* d_allowed_ids, uint64_t n_allowed,
                                         uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer,
                                         int32_t* d_out_rank, uint32_t* d_out_counts, uint32_t* d_stats, void* stream,
                                         uint32_t* n_panics);
/* hnswgpu_search_batch_filter_set with every buffer in HBM (ids, offsets and filter_of too); d_stats, stream and n_panics as in
 * hnswgpu_search_batch_filtered_device.  The arrays cannot be read on the host: a kernel counts the entries of d_filter_of that
 * are >= n_filters, and if there are any the call returns HNSWGPU_ERR_ARG BEFORE the search is launched -- no output is written,
 * the handle stays usable.  That d_filter_offsets starts at 0, ascends and ends inside d_filter_ids, and that every vector is
 * sorted, is the caller's promise (as the sortedness is in hnswgpu_search_batch_filtered_device).  The call waits on `stream` once
 * more than the one-filter call (the count), and once per group when the set exceeds HNSWGPU_FILTER_SET_MB.                */
int hnswgpu_search_batch_filter_set_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                           uint64_t k, uint64_t ef, const uint64_t* d_filter_ids,
                                           const uint64_t* d_filter_offsets, uint64_t n_filters, const uint32_t* d_filter_of,
                                           uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer,
                                           int32_t* d_out_rank, uint32_t* d_out_counts, uint32_t* d_stats, void* stream,
                                           uint32_t* n_panics);
/* The same call, not waited for: hnswgpu_search_batch_device_begin returns at once with a ticket (a worker thread of
 * the library issues the launches on `stream` and waits for them), hnswgpu_search_batch_end waits for that call, returns
 * its status (its message is then hnswgpu_last_error() of the caller's thread) and releases the ticket.  Two batches in
 * flight from one host thread keep the device full while a launch drains towards its longest search (DESIGN.md
 * section 8).  Every ticket must be ended exactly once; the buffers and the index must stay alive until then; give
 * concurrent tickets different output buffers (and, to let them overlap on the device, different streams).          */
typedef struct hnswgpu_ticket hnswgpu_ticket;
int hnswgpu_search_batch_device_begin(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                      uint64_t k, uint64_t ef, uint64_t* d_out_ids, float* d_out_dists,
                                      uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts,
                                      uint32_t* d_stats, void* stream, hnswgpu_ticket** ticket);
int hnswgpu_search_batch_end(hnswgpu_ticket* ticket);
/* Concurrency: the search entry points may be called from several host threads on ONE handle at the same time (the
 * reference's search is `&self`); every call takes a private workspace.  Calls that change the index (insert, upload)
 * wait for running searches.                                                                                       */

/* Ties.  Two EQUAL f32 distances can make the reference's answer depend on the internal order of Rust's BinaryHeap.
 * The kernel follows the reference by VALUE and detects the places where values do not decide (two equal nearest
 * candidates at a pop, an equal candidate evicted from the result set that is still the farthest distance, equal
 * distances or an ambiguous survivor among the first k answers).  With strict ties ON (default; env
 * HNSWGPU_STRICT_TIES=0 or this call turns it off) such a query carries on, inside the same launch, with a literal
 * emulation of the heap in question rebuilt from a log of the search so far (stats status 3), so that ids match the
 * reference bit for bit also under ties.  OFF: equals are ordered by arrival and the query is flagged (status 2).
 * hnswgpu_last_tie_count: queries of the last call that met such a place (resolved, or flagged).                   */
int hnswgpu_set_strict_ties(hnswgpu_index* idx, int on);
int hnswgpu_last_tie_count(const hnswgpu_index* idx, uint32_t* ties);

/* The HNSWGPU_* tuning and test hooks (HNSWGPU_HASH_BITS, _NO_SCHED, _NO_INKERNEL, _STRICT_WG_PER_CU, _CAND_LDS, _WAVES_PER_CU,
 * _EXACT_FIRST, _TRACE_LAUNCH, _TRACE_HOST, _HOST_THREADS, _HOST_CHUNKS, _FFI_UNPACK, _FILTER_SET_MB; the test hooks
 * HNSWGPU_BITMAP_SLICES, HNSWGPU_LITERAL_CAND_CAP, HNSWGPU_MAX_WG, HNSWGPU_RANGE_HITS_PER_PASS, HNSWGPU_GRAPH_CHUNK, HNSWGPU_RANGE_CHUNK and
 * HNSWGPU_POISON_SCRATCH) are read from the
 * environment ONCE per process, at the library's first search -- never on the launch path.  A caller that changes them afterwards (the tests do)
 * says so with this call.  Always HNSWGPU_OK.                                                                          */
int hnswgpu_reload_env(void);

/* The arithmetic of Distance<f32>::eval during SEARCH (construction always sums like the scalar build).
 *   HNSWGPU_ARITH_SCALAR (default): the crate's default build -- every sum left to right over the vector index
 *                                   (anndists 0.1 without features, Cargo.toml:104-106); what the parity tests pin.
 *   HNSWGPU_ARITH_SIMD8:            an APPROXIMATION of the summation order of its `simdeez_f` / `stdsimd` builds
 *                                   (Cargo.toml:107-111; the builds behind every number the reference publishes,
 *                                   README.md:46-56): 8 vertical f32 accumulators over the full blocks of 8 elements, their
 *                                   horizontal sum LEFT TO RIGHT, then the d % 8 tail; DistCosine with three such f32 sums.
 *                                   The crate's sources are not available here: its vector width follows the ISA chosen at
 *                                   run time, its horizontal add may fold halves pairwise, and DistCosine may have no SIMD
 *                                   kernel at all -- so this mode is checked against the oracle's dist_simd8 only, and is
 *                                   NOT claimed to reproduce a simdeez_f build bit for bit until oracle/ref_pin has been run
 *                                   with `--features simdeez_f` (.github/workflows/pin.yml does).  DistL2 / DistCosine / DistDot / DistL1 only
 *                                   (other distances keep the scalar order).  Last-bit differences to the scalar build, so
 *                                   near-tie ids may differ from it; the checker for this mode is the oracle's dist_simd8.
 * Opt-in, never the default.  Takes effect for the following search calls on every replica of the index.            */
#define HNSWGPU_ARITH_SCALAR 0
#define HNSWGPU_ARITH_SIMD8 1
int hnswgpu_set_arithmetic(hnswgpu_index* idx, int arithmetic);

/* How the replicas of an index hold its vectors in HBM.  The index itself stays an Hnsw<f32, D> (the dump stays t_name "f32",
 * construction runs on f32, queries are f32 with any values); only the device copy of the rows narrows, and only when that loses
 * nothing:
 *   HNSWGPU_STORAGE_F32 (default, also after hnswgpu_load_dump / hnswgpu_build): n x row_stride f32, rows of 128-byte lines.
 *   HNSWGPU_STORAGE_F16:  n x row_stride IEEE binary16 (64-byte lines), converted on the host at upload -- half the bytes of the rows
 *                         and half the row traffic of a search.  The search kernels widen each element back (binary16 -> binary32
 *                         is exact) and run the unchanged arithmetic, so EVERY search-path answer equals the same call on the same
 *                         index at F32: ids, f32 distance bits, p_ids, counts, the per-query work counters, hnswgpu_last_tie_count
 *                         and the filtered search's panic status, under strict ties and lean.
 * An f32 x is REPRESENTABLE iff it is not NaN and (f32)(f16)x has the bits of x: +-0, the f16 subnormals, everything up to
 * +-65504 that needs no more than 11 significant bits, +-inf.  hnswgpu_f16_representable returns the number of elements of
 * x[0..n) that are not, and the index of the first in *first_bad (may be NULL); it is the host routine the scans below use.
 * hnswgpu_set_storage(F16) scans the index's vectors on the host (the caller rounds, the library only verifies): the first
 * element that is not representable fails the call with HNSWGPU_ERR_ARG -- the message names the point's DataId, the dimension and
 * the number of offending elements -- and the index keeps its previous storage.  Also HNSWGPU_ERR_ARG: a metric other than DistL2 /
 * DistCosine / DistDot / DistL1; F16 on an index set to HNSWGPU_ARITH_SIMD8 (and hnswgpu_set_arithmetic(SIMD8) on an F16 index);
 * an unknown storage value.  Switching back to F32 is always allowed.
 * A change of storage marks every replica stale, like an insert: the next upload, explicit or the lazy one in front of a search,
 * makes replicas of the new kind.
 * Inserts on an F16 index (hnswgpu_insert, hnswgpu_insert_gpu, insert_f32, parallel_insert_f32) check the NEW vectors first: one
 * element that is not representable refuses the whole call with HNSWGPU_ERR_ARG and nothing is inserted (the two FFI symbols
 * have no status: the message is in hnswgpu_last_error).  The build itself runs on f32, host or GPU-assisted, unchanged.
 * Served from an F16 replica: hnswgpu_search_batch(_device), _device_begin / _end, _sharded(_device), _filtered(_device),
 * _filter_set(_device), hnswgpu_range_search_batch(_device), search_neighbours_f32 / parallel_search_neighbours_f32;
 * hnswgpu_file_dump still writes f32.  The calls that read rows outside the search path -- hnswgpu_exact_search_batch*,
 * hnswgpu_exact_range_search_batch*, hnswgpu_exact_graph_batch*, hnswgpu_graph_search_batch* (its gather kernel copies rows) --
 * return HNSWGPU_ERR_ARG on an F16 index before touching any output; the message says to set F32.
 * hnswgpu_get_storage: the index's storage.  hnswgpu_device_bytes: the bytes of the replica on `device` (< 0: the primary one),
 * HNSWGPU_ERR_DEVICE when the index is not resident (or stale) there.                                                            */
#define HNSWGPU_STORAGE_F32 0
#define HNSWGPU_STORAGE_F16 1
int hnswgpu_set_storage(hnswgpu_index* idx, int storage);
int hnswgpu_get_storage(const hnswgpu_index* idx);
uint64_t hnswgpu_f16_representable(const float* x, uint64_t n, uint64_t* first_bad);
int hnswgpu_device_bytes(const hnswgpu_index* idx, int device, uint64_t* bytes);

/* Timing of the kernels of the last search call on this index, measured with HIP events on
 * the launch stream: total milliseconds and number of launches (retries included).        */
int hnswgpu_last_kernel_ms(const hnswgpu_index* idx, double* ms, uint32_t* launches);
/* Same, but only up to the end of the search kernel proper (excludes the exact replay of tied queries). */
int hnswgpu_last_search_kernel_ms(const hnswgpu_index* idx, double* ms);

/* Distance<f32>::eval evaluated ON THE DEVICE by the search kernel's own distance routine (batch_dist: lane groups of
 * 4 or 2 lanes per row, left-to-right sum in the group's first lane) -- for arithmetic parity tests (host buffers).
 *   hnswgpu_eval_distances:       out[i]    = dist(a[i], b[i]), n pairs (each one a batch of a single row)
 *   hnswgpu_eval_distance_matrix: out[q][r] = dist(queries[q], rows[r]); the rows are evaluated in batches of `batch`
 *                                 (1..64) consecutive rows, the branch structure the search takes for that many fresh
 *                                 neighbours (<= 16 rows: 4 lanes per row; more: 32 rows at 2 lanes per row, ...).  */
int hnswgpu_eval_distances(int dist, const float* a, const float* b, uint64_t n, uint64_t d, float* out);
int hnswgpu_eval_distance_matrix(int dist, const float* queries, uint64_t nq, const float* rows, uint64_t n, uint64_t d,
                                 uint32_t batch, float* out);
/* the same in the given arithmetic (HNSWGPU_ARITH_*)                                                                  */
int hnswgpu_eval_distance_matrix_arith(int dist, int arithmetic, const float* queries, uint64_t nq, const float* rows,
                                       uint64_t n, uint64_t d, uint32_t batch, float* out);
/* the same (scalar arithmetic) with `rows` held as the given storage (HNSWGPU_STORAGE_*): F16 narrows them on the host before the
 * kernel reads them, as a replica's are -- every element of rows must be representable, else HNSWGPU_ERR_ARG                      */
int hnswgpu_eval_distance_matrix_storage(int dist, int storage, const float* queries, uint64_t nq, const float* rows,
                                         uint64_t n, uint64_t d, uint32_t batch, float* out);
/* the same through one of the row loops of the distance routine that only the search kernel's expansion loop compiles -- the same
 * left-to-right sum, so the same bits -- `variant` a bit set:
 *   HNSWGPU_EVAL_DEEP  sixteen row loads per lane at two lanes per row: a strict search with ef <= 128
 *   HNSWGPU_EVAL_PIPE  two register sets that take turns, the next round's loads ahead of this round's chain: a strict search with
 *                      ef 129 .. 256
 *   HNSWGPU_EVAL_R128  the row stride 128 as a compile-time fact: a search of ef 64 or 128 on DistL2 / F32 rows of 97 .. 128
 *                      elements, lean; with HNSWGPU_EVAL_DEEP its strict form
 * 0 is hnswgpu_eval_distance_matrix_storage.  DEEP and PIPE exist for the seven distances on F32 rows and the four of F16 rows.
 * HNSWGPU_ERR_ARG, never the plain routine in a variant's place: DEEP with PIPE; R128 with PIPE; R128 with another distance,
 * storage or dimension; unknown bits; and what hnswgpu_eval_distance_matrix_storage refuses.                                      */
#define HNSWGPU_EVAL_DEEP 1
#define HNSWGPU_EVAL_PIPE 2
#define HNSWGPU_EVAL_R128 4
int hnswgpu_eval_distance_matrix_variant(int dist, int storage, int variant, const float* queries, uint64_t nq, const float* rows,
                                         uint64_t n, uint64_t d, uint32_t batch, float* out);

/* ---------------------------------------------------------------- exact k-NN ---------- */
/* Exhaustive exact k-NN over EVERY point of the index (all layers), on the device: the ground truth a recall measurement
 * needs (the reference's protocol: examples/ann-sift1m-128-euclidean.rs:172-186, tests/serpar.rs:305-317), and "brute force on
 * the allowed subset" for a filtered search (tests/filtertest.rs).  The reference has no such function; the contract is:
 *   distance  the f32 Distance<f32>::eval the index's search computes for that pair (HNSWGPU_ARITH_SCALAR: same summation
 *             order, no contraction, f64 sums of DistCosine, the same ln); all seven distances.  An index set to
 *             HNSWGPU_ARITH_SIMD8 is refused with HNSWGPU_ERR_ARG -- the call never answers in the other arithmetic.
 *   answer    per query the min(k, #eligible) points of smallest key (distance as f32 value, origin id ascending, then
 *             dump order), written in that order; out_counts[q] = that number; slots behind it are zero.  The answer is a
 *             function of (vectors, ids, distance, query) alone -- not of the graph, insertion or dump order.  A NaN
 *             distance orders behind every number and is returned as the canonical quiet NaN.
 *   filter    allowed_ids == NULL: every point is eligible.  Else the SORTED id vector of `impl FilterT for Vec<usize>`
 *             (unsorted: HNSWGPU_ERR_ARG); ids naming no point are ignored; an empty vector gives counts of 0.
 *   k         1 .. 4096 (larger: HNSWGPU_ERR_ARG -- the selection costs O(k / 64) steps per insertion, and 4096 is the largest k
 *             that was run at size); k > nb_point is fine.
 * Same outputs as hnswgpu_search_batch (out_layer / out_rank may be NULL).  Scratch memory is a fixed budget: the nq x n
 * distance matrix is never formed, long batches are cut into chunks of queries.  Takes the handle's lock shared, like a
 * search.  Host buffers; uploads the index on first use like hnswgpu_search_batch.                                    */
int hnswgpu_exact_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                               const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dists,
                               uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts);
/* The same on device-resident buffers (d_allowed_ids too; NULL = no filter), launched on HIP stream `stream` and waited
 * for.  The index must be uploaded (else HNSWGPU_ERR_DEVICE).  The sortedness of d_allowed_ids is the caller's promise. */
int hnswgpu_exact_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, uint64_t k,
                                      const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids,
                                      float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank,
                                      uint32_t* d_out_counts, void* stream);
/* The exact answers for a SET of filters, each query naming its own: the ground truth of hnswgpu_search_batch_filter_set.  Row q
 * is exactly what hnswgpu_exact_search_batch returns for query q alone with allowed_ids = filter filter_of[q] -- ids and their
 * order, f32 distance bits (NaN and +-0 as there), p_ids, counts, zeros behind the answers.  The set is given as in
 * hnswgpu_search_batch_filter_set (CSR filter_ids / filter_offsets[0 .. n_filters], every vector sorted; filter_of[0..nq) <
 * n_filters) and checked the same way, each HNSWGPU_ERR_ARG with a message that names the offender; then k, d and the arithmetic
 * as in hnswgpu_exact_search_batch.  Ids naming no point are ignored, an empty vector gives count 0.  No out_status: an
 * exhaustive search has no panic case.  A tile of 16 queries may mix filters (every lane keeps one eligibility bit per query), so
 * one filter per query costs no more vector work than one filter for all.  The bitmaps one launch holds are bounded by
 * HNSWGPU_FILTER_SET_MB as in the search (and by half of this call's 320 MB of scratch); a larger set is served in groups of
 * consecutive filters, every query exactly once; a bound below one bitmap is HNSWGPU_ERR_ARG.  Keys (distance, id rank) are
 * unique, so an answer does NOT depend on how the queries are grouped into tiles, groups or chunks.                          */
int hnswgpu_exact_search_batch_filter_set(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                          const uint64_t* filter_ids, const uint64_t* filter_offsets, uint64_t n_filters,
                                          const uint32_t* filter_of, uint64_t* out_ids, float* out_dists, uint8_t* out_layer,
                                          int32_t* out_rank, uint32_t* out_counts);
/* The same with every buffer in HBM (ids, offsets and filter_of too), on `stream`, waited for.  The arrays cannot be read on the
 * host: a kernel counts the entries of d_filter_of that are >= n_filters, and if there are any the call returns HNSWGPU_ERR_ARG
 * BEFORE anything is searched -- no output is written, the handle stays usable.  Offsets and sortedness are the caller's promise,
 * as in hnswgpu_search_batch_filter_set_device.  The index must be uploaded (else HNSWGPU_ERR_DEVICE).                       */
int hnswgpu_exact_search_batch_filter_set_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                                 uint64_t k, const uint64_t* d_filter_ids, const uint64_t* d_filter_offsets,
                                                 uint64_t n_filters, const uint32_t* d_filter_of, uint64_t* d_out_ids,
                                                 float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank,
                                                 uint32_t* d_out_counts, void* stream);

/* ---------------------------------------------------------------- exact range search --- */
/* Every point within a query's radius, by exhaustive search on the device: the other basic query of a vector index
 * (deduplication, clustering radius, thresholded matching).  There is no k: the answer's size depends on the data, nothing is
 * selected, and the output is variable-length (CSR).  The reference has no such function; the contract is:
 *   distance  as in hnswgpu_exact_search_batch: the f32 the index's search computes for the pair in HNSWGPU_ARITH_SCALAR, all
 *             seven distances; an index set to HNSWGPU_ARITH_SIMD8 is refused with HNSWGPU_ERR_ARG.
 *   match     point p is in query q's answer iff p is eligible and dist(q, p) <= radii[q] as an IEEE f32 comparison of values.
 *             So a NaN distance never matches and a NaN radius matches nothing; a negative radius matches nothing (distances
 *             are >= 0); -0.0 and +0.0 match a distance of +-0; +inf matches every eligible point whose distance is not NaN,
 *             +inf distances included.
 *   order     ascending by the exact k-NN key: the distance's value with -0 folded into +0, then origin id, then dump order.
 *             For any k the first k entries of a query's answer are the exact k-NN answer restricted to the ball.
 *   output    CSR.  out_offsets[0 .. nq] is u64 and out_offsets[0] = 0; query q owns the slots out_offsets[q] .. out_offsets[q + 1]
 *             of out_ids (origin ids), out_dists (f32; a -0 distance comes back as +0), out_layer and out_rank (the point's own
 *             p_id; both may be NULL).
 *   capacity  cap = the number of slots behind the four out arrays.  out_offsets is ALWAYS written completely, so
 *             out_offsets[nq] is the total.  total <= cap: the answers are written, HNSWGPU_OK.  Otherwise NO out slot is touched
 *             and the call returns HNSWGPU_ERR_CAPACITY; hnswgpu_last_error() names the total needed.  cap == 0 with NULL out
 *             arrays is the count-only call: it evaluates every pair once and never runs the fill pass.  cap > 0 with a NULL
 *             out_ids or out_dists is HNSWGPU_ERR_ARG.
 *   filter    allowed_ids == NULL: every point is eligible.  Else the SORTED id vector, as in hnswgpu_exact_search_batch:
 *             unsorted is HNSWGPU_ERR_ARG (host entry), ids naming no point are ignored, an empty vector gives empty answers.
 *   radii     one f32 per query.
 *   The answer is a function of (vectors, ids, distance, query, radius) alone: not of the graph, not of the dump order beyond the
 *   last tie-break, not of how the queries are grouped into tiles or chunks.  An empty index: every answer is empty, HNSWGPU_OK.
 * Two passes over the same pair evaluations (count, then fill), a sort of every query's keys, a decoding pass.  Scratch memory
 * is a fixed budget: neither the nq x n matrix nor the whole answer is held on the device by the host entry -- the fill pass
 * serves consecutive queries whose answers fit 8 Mi slots (or one query, however many points it hits; the test hook
 * HNSWGPU_RANGE_HITS_PER_PASS sets another number) and the host entry copies each pass's answers out.  Takes the handle's lock
 * shared, like a search.  Host buffers; uploads the index on first use.                                                       */
int hnswgpu_exact_range_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                     const float* radii, const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t cap,
                                     uint64_t* out_offsets, uint64_t* out_ids, float* out_dists, uint8_t* out_layer,
                                     int32_t* out_rank);
/* The same on device-resident buffers (radii, filter and offsets too), on HIP stream `stream`, waited for; the same capacity rule
 * (the out arrays hold cap slots in HBM and are written in place).  The index must be uploaded (else HNSWGPU_ERR_DEVICE).  The
 * sortedness of d_allowed_ids is the caller's promise.  The offsets are read back once (the fill pass is planned on the host).  */
int hnswgpu_exact_range_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                            const float* d_radii, const uint64_t* d_allowed_ids, uint64_t n_allowed,
                                            uint64_t cap, uint64_t* d_out_offsets, uint64_t* d_out_ids, float* d_out_dists,
                                            uint8_t* d_out_layer, int32_t* d_out_rank, void* stream);

/* ---------------------------------------------------------------- approximate range search --- */
/* Every point within a query's radius that the GRAPH finds: the range query at the cost of a search, not of a scan over every row
 * (hnswgpu_exact_range_search_batch is its ground truth).  The reference has no such function; the contract is defined step by step
 * through the index's own search, so that every answer is one call of the reference's `search`, bit for bit.
 * Let the ef sequence be e_0 = ef_first, e_{j+1} = min(2 e_j, ef_max).  Query q is defined in rounds j = 0, 1, ...:
 *   1. A_j is the answer hnswgpu_search_batch_device gives for q with knbn = e_j and ef = e_j -- with a filter (allowed_ids !=
 *      NULL), the answer of hnswgpu_search_batch_filtered_device under allowed_ids -- in the index's arithmetic (scalar or SIMD
 *      order) and tie setting: the reference's search / search_filter, its whole final result set, ascending.  c_j is its count.
 *   2. m_j is the length of the longest prefix of A_j whose distances satisfy dist <= radii[q] as an IEEE f32 comparison of
 *      values.  A NaN or negative radius gives 0; -0.0 and +0.0 match a distance of +-0; +inf matches every distance that is
 *      not NaN.
 *   3. q is SETTLED in the first round where one of these holds: (a) m_j < c_j: the result set reached past the ball;
 *      (b) c_j < e_j: the search returned everything it can reach; (c) e_j == ef_max.
 *   4. q's answer is the first m_j entries of that A_j in the search's own order: ids, f32 distance bits and p_ids as the search
 *      wrote them.  out_ef[q] = e_j.  out_flags[q] bit 0 (SATURATED) is set iff q settled with m_j == c_j == e_j -- under rule
 *      (c) only: the ball may hold more, the caller raises ef_max.  out_ef and out_flags may be NULL.
 * Nothing else about the search changes.  A settled query is never searched again; an unsettled one is searched again FROM
 * SCRATCH at the next ef -- there is no continuation, which is what keeps every row equal to one call of the reference.
 *   arguments 1 <= ef_first <= ef_max <= 4096, else HNSWGPU_ERR_ARG (above 1024 the literal-heap kernel serves the round, as in
 *             hnswgpu_search_batch_device).  With a filter ef_first >= 2: the only input on which the reference panics needs
 *             ef == 1 (src/hnsw.rs:973), so this call has no panic status.  The filter is the SORTED id vector of
 *             hnswgpu_search_batch_filtered (unsorted: HNSWGPU_ERR_ARG from the host entry); an empty vector (a non-NULL
 *             pointer, n_allowed == 0) allows nothing.  nq == 0 or an empty index: HNSWGPU_OK, all offsets zero.
 *   output    CSR as in hnswgpu_exact_range_search_batch: out_offsets[0 .. nq] is u64 and is ALWAYS written completely; cap = the
 *             slots behind the four out arrays (out_layer / out_rank may be NULL); cap == 0 with NULL out arrays is the
 *             count-only call, which holds no answers; cap > 0 with a NULL out_ids or out_dists is HNSWGPU_ERR_ARG.
 *   capacity  total > cap: HNSWGPU_ERR_CAPACITY, hnswgpu_last_error() names the total -- and, UNLIKE the exact call, the contents
 *             of the out arrays are then unspecified: the batch is served group by group, the total is not known before the last
 *             group, and from the group that overflows onward the call only counts.
 *   memory    the batch is served in groups of consecutive queries, each group running all its rounds before the next starts.  A
 *             group holds at most HNSWGPU_RANGE_CHUNK queries (a test hook); unset, as many as keep the staged answers of a round
 *             and the group's held answers (each at most group x ef_max x 17 bytes) and its gathered queries within 256 MiB
 *             each.  Device memory is a fixed budget that does not depend on nq, for both entries.
 * Takes the handle's lock shared and is legal from several host threads at once.  Host buffers; uploads the index on first use.
 * Out of scope: filter sets, queries by stored point, sharding over GPUs, tickets (_begin / _end), any slack or ratio in the
 * stop rule, continuing a search instead of restarting it.                                                                  */
int hnswgpu_range_search_batch(const hnswgpu_index* idx, const float* queries, uint64_t nq, uint64_t d, const float* radii,
                               uint64_t ef_first, uint64_t ef_max, const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t cap,
                               uint64_t* out_offsets, uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank,
                               uint32_t* out_ef, uint8_t* out_flags);
/* The same with every buffer in HBM (radii, filter, offsets, ef and flags too), on HIP stream `stream`, waited for; the out arrays
 * hold cap slots and are written in place.  The index must be uploaded (else HNSWGPU_ERR_DEVICE).  The sortedness of
 * d_allowed_ids is the caller's promise.  One word is read back per round and group: the host sizes the next launch.        */
int hnswgpu_range_search_batch_device(const hnswgpu_index* idx, const float* d_queries, uint64_t nq, uint64_t d, const float* d_radii,
                                      uint64_t ef_first, uint64_t ef_max, const uint64_t* d_allowed_ids, uint64_t n_allowed,
                                      uint64_t cap, uint64_t* d_out_offsets, uint64_t* d_out_ids, float* d_out_dists,
                                      uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_ef, uint8_t* d_out_flags, void* stream);

/* ---------------------------------------------------------------- queries by stored point: the k-NN graph --- */
/* The neighbours of points that are ALREADY IN THE INDEX: asked for one point, "more like this"; asked for every point, the
 * k-nearest-neighbour graph of the data set (what embedders, graph clustering and duplicate detection start from).  The stored
 * vectors are the queries and never leave the device, and "without the point itself" is defined by IDENTITY -- the point's own
 * p_id -- not by its DataId and not by distance 0: exact copies of a point and other points that carry its DataId are
 * neighbours like any other.  The reference has no such function; the contract is:
 *   points    point_ids[0 .. np) are DataIds.  An id that several points carry names the FIRST of them in dump order.  The same id
 *             may occur more than once; every occurrence gets its own row.  An id that no point carries: HNSWGPU_ERR_ARG, the
 *             message gives the number of such ids -- BEFORE any out slot is written and before anything is searched (the ids are
 *             resolved on the device, a binary search per id, and the count is read back first).
 *             point_ids == NULL: every point.  np must then be hnswgpu_nb_point (else HNSWGPU_ERR_ARG), and row i is the point at
 *             position i of the ascending (DataId, dump order) order -- with ids 0 .. n-1, row i is the point of id i.
 *   output    as hnswgpu_search_batch: np x k row major, out_counts[i] entries in row i, the slots behind them zero; out_layer /
 *             out_rank (the neighbours' p_ids) may be NULL.  k >= 1 (else HNSWGPU_ERR_ARG).
 *
 * hnswgpu_graph_search_batch -- the approximate graph, by the index's own search.  Row i is defined in four steps:
 *   1. the answer hnswgpu_search_batch_device gives for the stored vector of point p_i (its first d elements) read as a query,
 *      with knbn = k + 1 and this ef, under the index's arithmetic and tie setting: bit for bit the reference's `search`;
 *   2. the entry whose p_id (layer, rank) is p_i's own is removed;
 *   3. if no entry is the point's own (it can be missing: the search is approximate, and k + 1 exact copies may crowd it out) and
 *      the answer has k + 1 entries, its last entry is removed;
 *   4. out_counts[i] is what remains (at most k).
 * Nothing else about the search changes.  The points are served in chunks of at most HNSWGPU_GRAPH_CHUNK (a test hook; unset:
 * as many as keep the gathered queries and the (k + 1)-wide staged answers within 256 MiB): gathered, searched, compacted.
 *
 * hnswgpu_exact_graph_batch -- the exact graph, by exhaustive search as in hnswgpu_exact_search_batch (same distance, same key,
 * same scratch budget).  Row i is the min(k, #candidates) points of smallest key (distance as f32 value, origin id ascending,
 * then dump order) among the candidates: every point other than p_i itself, or, with a filter (allowed_ids: the SORTED id vector
 * as in hnswgpu_exact_search_batch; unsorted: HNSWGPU_ERR_ARG from the host entry), the allowed points other than p_i itself.  A
 * queried point need not be allowed; an allowed queried point is still no candidate of its own row.  The distance bits are those
 * hnswgpu_exact_search_batch returns for the point's vector brought as a query.  An index of one point: count 0.  k is 1 .. 4096
 * and an index set to HNSWGPU_ARITH_SIMD8 is refused, both HNSWGPU_ERR_ARG, as there.
 *
 * Out of scope, all of it: using dist(p, q) == dist(q, p) to halve the exact graph's work; filter sets; k above 4096; sharding
 * over several GPUs; the SIMD-order arithmetic for the exact call.  (The graph made undirected, in CSR: hnswgpu_symmetric_graph.)
 * Host buffers; upload the index on first use like hnswgpu_search_batch; take the handle's lock shared, like a search.      */
int hnswgpu_graph_search_batch(const hnswgpu_index* idx, const uint64_t* point_ids, uint64_t np, uint64_t k, uint64_t ef,
                               uint64_t* out_ids, float* out_dists, uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts);
int hnswgpu_exact_graph_batch(const hnswgpu_index* idx, const uint64_t* point_ids, uint64_t np, uint64_t k,
                              const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dists,
                              uint8_t* out_layer, int32_t* out_rank, uint32_t* out_counts);
/* The same with point_ids, the filter and the outputs in device memory, on HIP stream `stream`, waited for.  The index must be
 * uploaded (else HNSWGPU_ERR_DEVICE).  The sortedness of d_allowed_ids is the caller's promise.                              */
int hnswgpu_graph_search_batch_device(const hnswgpu_index* idx, const uint64_t* d_point_ids, uint64_t np, uint64_t k, uint64_t ef,
                                      uint64_t* d_out_ids, float* d_out_dists, uint8_t* d_out_layer, int32_t* d_out_rank,
                                      uint32_t* d_out_counts, void* stream);
int hnswgpu_exact_graph_batch_device(const hnswgpu_index* idx, const uint64_t* d_point_ids, uint64_t np, uint64_t k,
                                     const uint64_t* d_allowed_ids, uint64_t n_allowed, uint64_t* d_out_ids, float* d_out_dists,
                                     uint8_t* d_out_layer, int32_t* d_out_rank, uint32_t* d_out_counts, void* stream);

/* ---------------------------------------------------------------- the symmetrised k-NN graph, in CSR --- */
/* The k-NN graph of the indexed points made UNDIRECTED on the device: what embedders (annembed, UMAP-style), spectral methods,
 * connected components and mutual-neighbour outlier tests turn the directed graph into before anything else.  A k-NN graph is
 * directed -- j in kNN(i) does not give i in kNN(j) -- and the rows of the undirected one are ragged (a hub is named by up to
 * n - 1 others), so the answer is CSR, not n x k.  The reference has no such function; the contract is defined through the two
 * graph calls above:
 *   rows      row i, i in 0 .. n = hnswgpu_nb_point, is the point at position i of the ascending (DataId, dump order) order:
 *             exactly the row numbering of the graph calls with point_ids == NULL.  POSITIONS, not DataIds, are the vertex names
 *             (DataIds may repeat): out_pos carries each neighbour's position; out_ids, out_layer and out_rank carry its DataId
 *             and p_id, as everywhere else.
 *   D         the directed graph.  ef == 0: row i of D is row i of hnswgpu_exact_graph_batch(idx, NULL, n, k, NULL, 0, ...);
 *             ef >= 1: row i of hnswgpu_graph_search_batch(idx, NULL, n, k, ef, ...) -- bit for bit: the neighbours' p_ids, their
 *             order, their f32 distance bits, the counts.  A neighbour's position is the position of the point that has its p_id.
 *             What those calls refuse this call refuses the same way, HNSWGPU_ERR_ARG before any output is written: k == 0; for
 *             ef == 0, k above 4096 and an index set to HNSWGPU_ARITH_SIMD8; an index set to HNSWGPU_STORAGE_F16.
 *   answer    write i -> j for "j is an entry of row i of D", with distance d(i->j).
 *             HNSWGPU_SYM_UNION:  row i holds j iff i -> j or  j -> i.
 *             HNSWGPU_SYM_MUTUAL: row i holds j iff i -> j and j -> i.
 *             j != i always (D never holds a point in its own row); a pair appears once per row, however it arose.  Any other
 *             mode is HNSWGPU_ERR_ARG.
 *   distance  of entry j in row i: d(i->j) when i -> j, otherwise (UNION only) d(j->i) -- the STORED f32 bits of D, never a
 *             recomputation.  For DistL2, DistL1, DistDot, DistCosine and DistHellinger the two directions are the same
 *             arithmetic and entry (i, j) equals entry (j, i) in its bits.  DistJeffreys (ln(a/b) against ln(b/a)) and
 *             DistJensenShannon (its two terms added in the other order) are NOT symmetric in their bits: for those two, rows i
 *             and j may carry different bits for the same pair.  That is the contract.
 *   order     within a row ascending by the exact k-NN key built from the entry's distance: the distance as an f32 value with -0
 *             folded into +0 and NaN last, then the neighbour's position (= DataId, then dump order).  The distance itself comes
 *             back as stored (a -0 stays -0).
 *   output    CSR.  out_offsets[0 .. n] is u64 and is ALWAYS written completely, so out_offsets[n] is the total; row i owns the
 *             slots out_offsets[i] .. out_offsets[i + 1] of out_pos, out_ids, out_dists, out_layer and out_rank (out_ids,
 *             out_layer and out_rank may each be NULL).
 *   capacity  cap = the number of slots behind the out arrays.  total <= cap: the answers are written, HNSWGPU_OK.  Otherwise NO
 *             out slot is touched and the call returns HNSWGPU_ERR_CAPACITY; hnswgpu_last_error() names the total needed.
 *             cap == 0 with NULL out arrays is the count-only call.  cap > 0 with a NULL out_pos or out_dists is HNSWGPU_ERR_ARG.
 *             An empty index or n == 1: all offsets zero, HNSWGPU_OK.
 *   memory    there is NO fixed scratch budget here: a sorted edge list of the whole graph is the product.  The work is O(n k) on
 *             the device.  With S = n k: D is staged (17 S + 4 n bytes, besides what its own call takes) and released once it is
 *             expanded into 2 S edge records of 12 bytes, held twice by the sort (48 S bytes, plus rocPRIM's temporary storage);
 *             the answer's total <= 2 S entries then take 20 bytes each (sort keys twice, distance bits) -- at most 88 S bytes
 *             and rocPRIM's temporary storage at the peak.  n k above 2^30 is HNSWGPU_ERR_ARG; the message gives the product.
 * The answer is a function of D alone (no float atomics, no write whose place depends on timing): two calls give the same bytes.
 * Takes the handle's lock shared, like a search, and is legal from several host threads at once.  Host buffers; uploads the index
 * on first use.
 * Out of scope: a filter or filter set; a subset of points; weights other than the stored distances (no kernel functions, no
 * perplexity); sharding over GPUs; F16 storage; connected components.                                                        */
#define HNSWGPU_SYM_UNION 0
#define HNSWGPU_SYM_MUTUAL 1
int hnswgpu_symmetric_graph(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t cap,
                            uint64_t* out_offsets, uint32_t* out_pos, uint64_t* out_ids, float* out_dists, uint8_t* out_layer,
                            int32_t* out_rank);
/* The same with every out array in HBM (the offsets too), on HIP stream `stream`, waited for; the out arrays hold cap slots and are
 * written in place.  The index must be uploaded (else HNSWGPU_ERR_DEVICE).  Only the total is read back.                      */
int hnswgpu_symmetric_graph_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t cap,
                                   uint64_t* d_out_offsets, uint32_t* d_out_pos, uint64_t* d_out_ids, float* d_out_dists,
                                   uint8_t* d_out_layer, int32_t* d_out_rank, void* stream);

/* ---------------------------------------------------------------- connected components, cut optional --- */
/* The connected components of the undirected k-NN graph of the section above, labelled on the device WITHOUT building that graph:
 * what an embedder asks before it normalises a Laplacian (is the graph connected?), what a mutual-neighbour outlier test is
 * (components of size 1 of the MUTUAL graph), and -- with the longer edges cut -- single-linkage clusters at a radius.  The
 * answer is all integers and every correct algorithm gives the same bytes.
 *   vertices  POSITIONS: vertex i, i in 0 .. n = hnswgpu_nb_point, is row i of hnswgpu_symmetric_graph, the point at position i
 *             of the ascending (DataId, dump order) order -- the row numbering of the graph calls with point_ids == NULL.
 *   D         the directed graph, exactly as hnswgpu_symmetric_graph takes it: k, ef and mode mean what they mean there (ef == 0:
 *             the exact graph; ef >= 1: the graph search at this ef).  What that call refuses this one refuses the same way,
 *             HNSWGPU_ERR_ARG before any output is written: k == 0; for ef == 0, k above 4096 and an index set to
 *             HNSWGPU_ARITH_SIMD8; an index set to HNSWGPU_STORAGE_F16; n k above 2^30; a mode that is neither HNSWGPU_SYM_UNION nor
 *             HNSWGPU_SYM_MUTUAL.
 *   cut       max_dist is a HOST pointer to one f32, in all four entries.  NULL: every entry of D counts, whatever its distance,
 *             a NaN included.  Otherwise the entry i -> j counts iff d(i->j) <= *max_dist, an ordered f32 comparison of the STORED
 *             bits: a NaN distance never counts, -0 equals +0.  *max_dist NaN is HNSWGPU_ERR_ARG.  The cut is applied to D FIRST;
 *             the definitions of the section above then apply to what is left -- HNSWGPU_SYM_UNION: i and j are joined iff i -> j
 *             or j -> i survives; HNSWGPU_SYM_MUTUAL: iff both survive (for DistJeffreys and DistJensenShannon, whose two directions
 *             differ in their bits, a cut may keep one direction of a pair and drop the other).
 *   answer    two vertices share a label iff a path of such joins connects them.  Components are numbered 0 .. c - 1 by their
 *             smallest position, ascending: out_label[0] == 0 and the first occurrences of the labels ascend.  out_label has n
 *             slots.  out_sizes may be NULL and has n slots: the first c are written (vertices per component), the rest are not
 *             touched.  *out_n_components = c.  An empty index: c = 0, nothing else written, HNSWGPU_OK.  A NULL out_label with
 *             n > 0 and a NULL out_n_components are HNSWGPU_ERR_ARG.  On any error no out slot is touched.
 *   memory    no record sort under UNION: every surviving slot of D is an edge.  With S = n k: D is staged as the section above
 *             stages it (17 S + 4 n bytes, besides what its own call takes) and stays until its slots are hooked; the forest takes
 *             12 n bytes (parents, root marks, their scan) and rocPRIM's temporary storage of one scan of n words.  MUTUAL needs the
 *             pairs named both ways and sorts the section above's 2 S edge records for them (D and the records held twice, 65 S
 *             bytes, and rocPRIM's temporary storage at the peak; 24 S while the forest is built).  The host forms add 4 n + 4 c
 *             bytes of staged answer.
 * The labels are the fixed point of a lock-free union-find over integer atomics (a root is the smallest position of its tree): the
 * answer is a function of D alone, two calls give the same bytes.  Takes the handle's lock shared, like a search, and is legal from
 * several host threads at once.  Host buffers; uploads the index on first use.
 * Out of scope: a filter or a subset of points; labels by DataId; sharding over GPUs; F16 storage; a hierarchy over all radii
 * (single-linkage dendrogram); strongly connected components of D.  (The hierarchy's merge order: the section below.)        */
int hnswgpu_graph_components(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, const float* max_dist,
                             uint32_t* out_label, uint32_t* out_sizes, uint64_t* out_n_components);
/* The same with out_label and out_sizes in HBM, on HIP stream `stream`, waited for; max_dist and out_n_components stay host
 * pointers.  The index must be uploaded (else HNSWGPU_ERR_DEVICE).  Only c is read back.                                      */
int hnswgpu_graph_components_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, const float* max_dist,
                                    uint32_t* d_out_label, uint32_t* d_out_sizes, uint64_t* out_n_components, void* stream);
/* The components of ANY graph given in CSR on `device`: offsets u64[n + 1], cols u32[offsets[n]], optionally dists f32[offsets[n]].
 * Every entry (r, c) joins r and c, whichever row names it: a directed CSR gets its WEAKLY connected components.  Self-loops and
 * repeated entries are legal and change nothing.  The cut, the numbering and the outputs are those above (an entry counts iff
 * dists[e] <= *max_dist); dists is read under a cut only, and dists == NULL with a non-NULL max_dist is HNSWGPU_ERR_ARG.
 * HNSWGPU_ERR_ARG, nothing written: offsets[0] != 0; offsets that descend; a col >= n; n > 2^31 - 1; offsets[n] >= 2^32 (and a NULL
 * offsets, or a NULL cols with offsets[n] > 0).  n == 0: c = 0, HNSWGPU_OK.  The outputs of hnswgpu_symmetric_graph_device
 * (offsets, pos, dists) are valid inputs as they stand.  Scratch: 12 n bytes and one scan's temporary storage; the host form
 * stages its arrays (8 n + 4 or 8 bytes per entry) and its answer.  Needs no index; legal from several host threads at once.    */
int hnswgpu_csr_components(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists,
                           const float* max_dist, uint32_t* out_label, uint32_t* out_sizes, uint64_t* out_n_components);
/* The same with the graph and out_label / out_sizes in HBM of `device`, on HIP stream `stream`, waited for.  The graph is checked
 * by a validation kernel and ONE word read back before any kernel that follows a col runs: a bad graph is HNSWGPU_ERR_ARG, never a
 * fault.  Only that word and c are read back.                                                                                */
int hnswgpu_csr_components_device(int device, uint64_t n, const uint64_t* d_offsets, const uint32_t* d_cols, const float* d_dists,
                                  const float* max_dist, uint32_t* d_out_label, uint32_t* d_out_sizes, uint64_t* out_n_components,
                                  void* stream);

/* ---------------------------------------------------------------- minimum spanning forest --- */
/* The minimum spanning forest (MSF) of the undirected k-NN graph of the two sections above, on the device WITHOUT building that
 * graph: the single-linkage clusters at EVERY radius in one call.  The forest's edges in ascending order are the merge order of the
 * single-linkage hierarchy; the components at a cut r are the components of the forest edges of weight <= r, and they are what
 * hnswgpu_graph_components answers at max_dist = r; with core_k >= 1 the weights are mutual-reachability distances and the forest
 * is what HDBSCAN starts from.  Under a strict total order on the edges the forest is unique: every correct algorithm gives the
 * same bytes.
 *   vertices  POSITIONS, exactly as in hnswgpu_graph_components: vertex i is the point at position i of the ascending (DataId, dump
 *             order) order, row i of hnswgpu_symmetric_graph.
 *   D         the directed graph: k, ef and mode mean what they mean in hnswgpu_graph_components, and what that call refuses of
 *             them this one refuses with the same words, HNSWGPU_ERR_ARG before any output is written.
 *   order     weights are compared as the exact k-NN key compares distances: by f32 value, -0 equal to +0, every NaN equal to
 *             every other NaN and behind +inf.  min and max below are min and max in this order.
 *   weight    of the pair {i, j}.  HNSWGPU_SYM_UNION: the pair exists iff i -> j or j -> i is in D, and weighs the min of the
 *             directions present.  HNSWGPU_SYM_MUTUAL: iff both are in D, and weighs the max of the two.  The weight carries the
 *             STORED bits of the direction chosen; when the two tie in the order, those of lo -> hi (lo < hi the two positions).
 *             ("Either direction survives a cut" is the min, "both survive" is the max: for DistJeffreys and DistJensenShannon,
 *             whose two directions differ in their bits, this is what makes the forest agree with the components at every cut.)
 *   core_k    0: the weights above.  core_k >= 1: weight = max(pair weight, core(lo), core(hi)), where core(v) is the stored
 *             distance in slot min(core_k, counts[v]) - 1 of row v of D (rows of D ascend; +0 for an empty row).  When values tie
 *             in the order the bits are the pair weight's first, then core(lo)'s, then core(hi)'s.  core_k > k is HNSWGPU_ERR_ARG.
 *   answer    the unique minimum spanning forest under the strict total order (weight, lo, hi) on pairs: n - c edges, c the number
 *             of components hnswgpu_graph_components reports with a NULL cut, written ascending by (weight, lo, hi).  Edge e:
 *             out_a[e] = lo, out_b[e] = hi > lo, out_w[e] = the weight's bits.  *out_n_edges = n - c.  The out arrays have
 *             max(n - 1, 0) slots; slots behind the answer are not touched.  n <= 1 (an empty index too): 0 edges, HNSWGPU_OK,
 *             nothing else written.  A NULL out_n_edges, and with n >= 2 a NULL out_a, out_b or out_w, are HNSWGPU_ERR_ARG.  On any
 *             error no out slot is touched.
 *   memory    with S = n k and m <= S pairs: the 2 S sorted edge records of the section above (D and the records held twice, 65 S
 *             bytes, and rocPRIM's temporary storage at the peak; D stays 17 S + 4 n bytes longer when core_k >= 1, for the 4 n
 *             bytes of core distances), then 24 S + 12 m while the pairs are taken out of the records, then the edge list alone:
 *             36 m + 12 n bytes (lo, hi, bits; order keys twice -- the flags and their scan afterwards --, two permutation halves,
 *             the ranked ends; parents, best edges, root marks) and rocPRIM's temporary storage of one sort of m pairs of words.
 *             The host forms add 12 (n - c) bytes of staged answer.
 * Boruvka rounds over the lock-free union-find of the components, integer atomics only: the edges are sorted into the total order
 * once, an edge's index is its rank, and every later comparison is a u32 atomic min.  A round is three kernels and one word read
 * back; there are at most ceil(log2 n) + 1 rounds, and the bound is hard (a round past it would be HNSWGPU_ERR_FORMAT, an internal
 * error).  The answer is a function of D alone, two calls give the same bytes.  Takes the handle's lock shared, like a search, and
 * is legal from several host threads at once.  Host buffers; uploads the index on first use.
 * Out of scope: a filter or a subset of points; F16 storage; (the dendrogram is the next section, HDBSCAN's clusters hnsw_mi355x_hdbscan.h)
 * sharding over GPUs; weights other than stored distances and their core maxima.                                              */
int hnswgpu_graph_spanning_forest(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k,
                                  uint32_t* out_a, uint32_t* out_b, float* out_w, uint64_t* out_n_edges);
/* The same with out_a, out_b and out_w in HBM, on HIP stream `stream`, waited for; out_n_edges stays a host pointer.  The index
 * must be uploaded (else HNSWGPU_ERR_DEVICE).  Only the pair count, one word per round and n - c are read back.               */
int hnswgpu_graph_spanning_forest_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k,
                                         uint32_t* d_out_a, uint32_t* d_out_b, float* d_out_w, uint64_t* out_n_edges, void* stream);
/* The minimum spanning forest of ANY graph given in CSR on `device`: offsets u64[n + 1], cols u32[offsets[n]], optionally dists
 * f32[offsets[n]] (dists == NULL: every weight is +0).  Every entry (r, c) is the undirected pair {r, c} with weight dists[e],
 * whichever row names it; self-loops are ignored; a pair that several entries name has the min of their weights (among entries that tie,
 * the bits of the lowest-numbered one).  The order, the answer and the outputs are those above, c being what
 * hnswgpu_csr_components reports with a NULL cut.  HNSWGPU_ERR_ARG, nothing written, exactly as hnswgpu_csr_components refuses:
 * offsets[0] != 0; offsets that descend; a col >= n; n > 2^31 - 1; offsets[n] >= 2^32 (and a NULL offsets, or a NULL cols with
 * offsets[n] > 0).  n <= 1: 0 edges, HNSWGPU_OK, no array is read.  The outputs of hnswgpu_symmetric_graph_device (offsets, pos,
 * dists) are valid inputs as they stand.  Scratch: 20 bytes per entry while the entries are sorted by (lo, hi), then 36 per entry
 * and 12 n as above; the host form stages its arrays and its answer.  Needs no index; legal from several host threads at once.   */
int hnswgpu_csr_spanning_forest(int device, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists,
                                uint32_t* out_a, uint32_t* out_b, float* out_w, uint64_t* out_n_edges);
/* The same with the graph and out_a / out_b / out_w in HBM of `device`, on HIP stream `stream`, waited for.  The graph is checked
 * by the validation kernels of hnswgpu_csr_components_device and ONE word read back first, before any kernel that follows a col
 * runs: a bad graph is HNSWGPU_ERR_ARG, never a fault.                                                                        */
int hnswgpu_csr_spanning_forest_device(int device, uint64_t n, const uint64_t* d_offsets, const uint32_t* d_cols, const float* d_dists,
                                       uint32_t* d_out_a, uint32_t* d_out_b, float* d_out_w, uint64_t* out_n_edges, void* stream);

/* ---------------------------------------------------------------- dendrogram of a forest --- */
/* The single-linkage dendrogram that a forest's edges, read in their order, encode: for every edge the two clusters it merges and
 * the size of the result -- the table scipy.cluster.hierarchy, HDBSCAN's condensed tree and every "cut into K clusters" start from.
 *   input     m edges over the vertices 0 .. n - 1 on `device`; edge e joins a[e] and b[e].  The order given IS the merge order:
 *             edge e is merge number e.  Weights are no argument: the height of merge e is whatever weight the caller holds for
 *             edge e.  out_a, out_b and *out_n_edges of hnswgpu_graph_spanning_forest(_device) and
 *             hnswgpu_csr_spanning_forest(_device) are valid inputs as they stand.
 *   ids       scipy's convention: id v < n is the vertex v alone, id n + i the cluster made by edge i.
 *   answer    out_left[e]: the id of the cluster that holds a[e] just before merge e, i.e. the component of a[e] under the edges
 *             0 .. e - 1 -- a[e] itself if no earlier edge touches it, else n + the largest edge index inside it.  out_right[e]: the
 *             same for b[e].  out_size[e]: the number of vertices of cluster n + e = size(left) + size(right), a vertex counting 1.
 *             Nothing is written behind slot m - 1.  m == 0: HNSWGPU_OK, no array is read or written.
 *   refused   HNSWGPU_ERR_ARG, no out slot touched: n > 2^31 - 1; m > max(n, 1) - 1 (a forest has at most n - 1 edges); with
 *             m >= 1 a NULL a, b, out_left, out_right or out_size; an end >= n; a[e] == b[e]; a cycle, i.e. an edge whose ends
 *             earlier edges already join (a repeated pair is one).  Ends and self-loops are checked on the host first, so those
 *             refusals need no device; a cycle is the device's to find.
 *   memory    16 (n + m) + 8 m bytes (and padding to 256 per array, and one word): the edges' two current labels, and per cluster
 *             id a parent, a last edge, a sum and a size.  The host form uploads its ends into the labels and downloads its answer
 *             from that scratch: it stages nothing more.
 * ceil(log2 m) levels of eight small launches over the lock-free union-find of the components, integer atomics only: level by level
 * the upper half of every aligned block of edge indices learns what the lower half merged.  The bound is hard; no wavefront waits
 * on another and nothing is read back inside the loop -- one word, at the end, before any out slot is written.  The answer is a
 * function of the edge list alone: two calls give the same bytes.  Needs no index; legal from several host threads at once.
 * Out of scope: a dendrogram of anything that is not a forest (HDBSCAN's condensed tree, stabilities and selection: hnsw_mi355x_hdbscan.h);
 * reordering of the rows (scipy wants ascending heights: an edge list sorted by weight gives them).                            */
int hnswgpu_forest_dendrogram(int device, uint64_t n, uint64_t m, const uint32_t* a, const uint32_t* b,
                              uint32_t* out_left, uint32_t* out_right, uint32_t* out_size);
/* The same with the five arrays in HBM of `device`, on HIP stream `stream`, waited for.  Ends and self-loops are checked by a kernel
 * of its own, which hands the levels scratch copies that are in range: a bad edge list is HNSWGPU_ERR_ARG, never a fault.  That
 * check and the cycle flag share ONE word, the only thing read back.                                                           */
int hnswgpu_forest_dendrogram_device(int device, uint64_t n, uint64_t m, const uint32_t* d_a, const uint32_t* d_b,
                                     uint32_t* d_out_left, uint32_t* d_out_right, uint32_t* d_out_size, void* stream);
/* hnswgpu_graph_spanning_forest followed by the dendrogram of its forest, which never leaves HBM in between.  out_a, out_b, out_w
 * and *out_n_edges are what hnswgpu_graph_spanning_forest writes with the same arguments, byte for byte; out_left, out_right and
 * out_size are the dendrogram of those edges in that order (ascending weight: the rows are scipy's linkage rows in scipy's order),
 * with the same max(n - 1, 0) slots, those behind the answer not touched.  Every refusal is that call's, with the same words; with
 * n >= 2 a NULL out_left, out_right or out_size is HNSWGPU_ERR_ARG too.  n <= 1: 0 edges, HNSWGPU_OK, nothing else written.  On
 * any error no out slot is touched.  Memory: the forest call's, then 12 (n - 1) bytes of forest and the dendrogram's
 * 16 (n + m) + 8 m.  Takes the handle's lock shared; host buffers; uploads the index on first use.                               */
int hnswgpu_graph_dendrogram(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k,
                             uint32_t* out_a, uint32_t* out_b, float* out_w,
                             uint32_t* out_left, uint32_t* out_right, uint32_t* out_size, uint64_t* out_n_edges);
/* The same with the six arrays in HBM, on HIP stream `stream`, waited for; out_n_edges stays a host pointer.  The index must be
 * uploaded (else HNSWGPU_ERR_DEVICE).  The forest is written into the caller's arrays directly: nothing is staged.              */
int hnswgpu_graph_dendrogram_device(const hnswgpu_index* idx, uint64_t k, uint64_t ef, uint32_t mode, uint64_t core_k,
                                    uint32_t* d_out_a, uint32_t* d_out_b, float* d_out_w,
                                    uint32_t* d_out_left, uint32_t* d_out_right, uint32_t* d_out_size, uint64_t* out_n_edges,
                                    void* stream);

/* Test entry: the lane lab. The wave-level algorithms the search kernels are made of -- the reference's BinaryHeap (src/hnsw.rs:940,
 * :958-973, :1035-1053, :1544; std's push / pop / into_sorted_vec) as a memory heap and as a register heap, the sorted result set
 * with its accept rule (:1028-1053), the exact visited table (:955-956, :1016-1017) -- run on `device` by ONE wavefront from a
 * script: ops[n_ops][4] = {op, a, b, c}, lanes[n_lane_sets][64][2] = {f32 bits, id} (the lane vectors of the batch operations).
 * mode 0 memory heap (p0 entries in LDS, p1 pop variant), 1 register heap (p0 slots per lane), 2 result set (p0 slots per lane,
 * p1 ef), 3 visited table (p0 tbits, p1 idbits, p2 restbits).  out[0] = words produced, then every operation's result in script
 * order, then the final state.  Operation codes and layouts: hnswlib-rs_amd/csrc/search_kernels.hpp (LAB_*), lane_lab.inc;
 * tests/test_gpu_lane_lab.py drives it.                                                                                    */
int hnswgpu_lane_lab(int device, uint32_t mode, uint32_t p0, uint32_t p1, uint32_t p2, const uint32_t* ops, uint32_t n_ops,
                     const uint32_t* lanes, uint32_t n_lane_sets, uint32_t* out, uint32_t out_words);


/* =======================================================================================
 * (2) The reference's own C ABI for f32 (src/libext.rs), same names and struct layouts.
 * ======================================================================================= */
typedef struct HnswIo HnswIo;         /* src/hnswio.rs:300-310 (opaque)                   */
typedef struct HnswApif32 HnswApif32; /* src/libext.rs:106 (opaque)                        */

typedef struct { /* src/libext.rs:64-71 */
    size_t id;
    float d;
} Neighbour_api;
typedef struct { /* src/libext.rs:82-87 */
    int64_t nbgh;
    const Neighbour_api* neighbours;
} Neighbourhood_api;
typedef struct { /* Vec_api<Neighbourhood_api>, src/libext.rs:58-62 */
    int64_t len;
    const Neighbourhood_api* ptr;
} Vec_api_Neighbourhood;
typedef struct { /* src/libext.rs:1121-1141 */
    uint8_t dumpmode;
    uint8_t max_nb_connection;
    uint8_t nb_layer;
    size_t ef;
    size_t nb_point;
    size_t data_dimension;
    size_t distname_len;
    const uint8_t* distname;
    size_t t_name_len;
    const uint8_t* t_name;
} DescriptionFFI;

const HnswIo* get_hnswio(uint64_t flen, const uint8_t* name);                      /* :28-33   */
const HnswApif32* load_hnswdump_f32_DistL1(HnswIo* hnswio);                        /* :310-315 */
const HnswApif32* load_hnswdump_f32_DistL2(HnswIo* hnswio);                        /* :316-321 */
const HnswApif32* load_hnswdump_f32_DistCosine(HnswIo* hnswio);                    /* :322-327 */
const HnswApif32* load_hnswdump_f32_DistDot(HnswIo* hnswio);                       /* :328-333 */
const HnswApif32* load_hnswdump_f32_DistJensenShannon(HnswIo* hnswio);             /* :334-339 */
const HnswApif32* load_hnswdump_f32_DistJeffreys(HnswIo* hnswio);                  /* :340-345 */
const HnswApif32* init_hnsw_f32(size_t max_nb_conn, size_t ef_const, size_t namelen,
                                const uint8_t* cdistname);                         /* :458-523 */
const HnswApif32* new_hnsw_f32(size_t max_nb_conn, size_t ef_const, size_t namelen, const uint8_t* cdistname,
                               size_t max_elements, size_t max_layer);             /* :532-580 */
/* The crate's init_hnsw_ptrdist_f32 takes a HOST function pointer as the distance (DistCFFI<f32>).  A host callback
 * cannot be evaluated by the device, and this library has no CPU search path by design: the symbol exists so that a host
 * linking the crate's C interface resolves, it always returns NULL and sets HNSWGPU_ERR_DISTANCE (hnswgpu_last_error()
 * says why).  Use one of the named distances. */
typedef float (*hnsw_dist_fn_f32)(const float* a, const float* b, unsigned long long len);
const HnswApif32* init_hnsw_ptrdist_f32(size_t max_nb_conn, size_t ef_const, hnsw_dist_fn_f32 c_func);  /* :643-655 */
void insert_f32(HnswApif32* hnsw_api, size_t len, const float* data, size_t id);   /* :661-678 */
void parallel_insert_f32(HnswApif32* hnsw_api, size_t nb_vec, size_t vec_len, const float** datas,
                         const size_t* ids);                                       /* :683-723 */
const Neighbourhood_api* search_neighbours_f32(const HnswApif32* hnsw_api, size_t len, const float* data,
                                               size_t knbn, size_t ef_search);     /* :728-767 */
const Vec_api_Neighbourhood* parallel_search_neighbours_f32(const HnswApif32* hnsw_api, size_t nb_vec,
                                                            int64_t vec_len, const float** data, size_t knbn,
                                                            size_t ef_search);     /* :205-254 */
int64_t file_dump_f32(const HnswApif32* hnsw_api, size_t namelen, const uint8_t* filename); /* :257-275 */
void drop_hnsw_f32(const HnswApif32* p);                                           /* :626-630 */
const DescriptionFFI* load_hnsw_description(size_t flen, const uint8_t* name);     /* :1171-1232 */
void init_rust_log(void);                                                          /* :1238-1240 (no-op) */

/* The reference leaks every result buffer to the caller and exports no free function
 * (SURVEY.md 8b "Ownership").  These are additions.
 * hnswgpu_free_neighbourhood releases what search_neighbours_f32 returned (the struct and its row).
 * hnswgpu_free_neighbourhood_vec releases what parallel_search_neighbours_f32 returned, and is the ONLY way to release
 * it: the answer is one allocation (Vec_api | Neighbourhood_api[nb_vec] | every Neighbour_api row) -- usually page-locked
 * memory the search kernels wrote in place, which free() cannot release at all --, so `ptr` and each
 * `neighbours` are interior pointers -- never free() a row or hand one of its Neighbourhood_api to
 * hnswgpu_free_neighbourhood, and never pass a Vec_api this library did not return.                                   */
void hnswgpu_free_neighbourhood(const Neighbourhood_api* p);
void hnswgpu_free_neighbourhood_vec(const Vec_api_Neighbourhood* p);
void hnswgpu_free_hnswio(const HnswIo* p);
void hnswgpu_free_description(const DescriptionFFI* p);
/* access the thin-ABI handle behind a reference-style handle (NULL until built/loaded)    */
hnswgpu_index* hnswgpu_from_api(const HnswApif32* p);

#ifdef __cplusplus
}
#endif
#endif /* HNSW_MI355X_H */
