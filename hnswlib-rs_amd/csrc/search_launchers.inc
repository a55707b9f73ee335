// search_launchers.inc -- host-side launchers of one metric's kernels (included by search_kernels_tu.hip, which is
// compiled once per metric and part; each part instantiates a third of the kernels).
namespace hnswgpu {
// the pieces the parts hand to each other: specialised per metric, defined in exactly one part
template <int METRIC> hipError_t launch_search_strict(int slots, int table, int shape, uint32_t grid, size_t lds, hipStream_t stream,
                                                      const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev);
template <int METRIC> hipError_t occupancy_strict(int slots, int table, int shape, size_t lds, int* per_cu);
template <int METRIC> hipError_t launch_search_lean(int slots, int table, int shape, uint32_t grid, size_t lds, hipStream_t stream,
                                                    const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev);
template <int METRIC> hipError_t occupancy_lean(int slots, int table, int shape, size_t lds, int* per_cu);
template <int METRIC> hipError_t launch_search_pair(uint32_t grid, size_t lds, hipStream_t stream, const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev);
template <int METRIC> hipError_t occupancy_pair(size_t lds, int* per_cu);

namespace {
constexpr int M = HNSW_THIS_METRIC;
using KernelFn = void (*)(DeviceIndexView, SearchArgs);
}  // namespace
template <> hipError_t launch_search_strict<M>(int, int, int, uint32_t, size_t, hipStream_t, const DeviceIndexView&, const SearchArgs&, LaunchEvents);
template <> hipError_t occupancy_strict<M>(int, int, int, size_t, int*);
template <> hipError_t launch_search_lean<M>(int, int, int, uint32_t, size_t, hipStream_t, const DeviceIndexView&, const SearchArgs&, LaunchEvents);
template <> hipError_t occupancy_lean<M>(int, int, int, size_t, int*);
template <> hipError_t launch_search_pair<M>(uint32_t, size_t, hipStream_t, const DeviceIndexView&, const SearchArgs&, LaunchEvents);
template <> hipError_t occupancy_pair<M>(size_t, int*);

#if HNSW_PART == 0 || HNSW_PART == 1
namespace {
constexpr bool STRICT = HNSW_PART == 0;
template <int TABLE>
KernelFn pick_slots(int slots) {
    switch (slots) {
        case 1: return hnsw_search_kernel<M, 1, TABLE, SHAPE_ANY, STRICT>;
        case 2: return hnsw_search_kernel<M, 2, TABLE, SHAPE_ANY, STRICT>;
        case 4: return hnsw_search_kernel<M, 4, TABLE, SHAPE_ANY, STRICT>;
        default: return hnsw_search_kernel<M, 16, TABLE, SHAPE_ANY, STRICT>;
    }
}
// the fixed shape exists where shape_r128_ef_built() says so; asked for anywhere else: nullptr, the launch fails (no silent SHAPE_ANY)
template <int S>
KernelFn pick_r128_ef() {
    if constexpr (shape_r128_ef_built(M, S, TABLE_LDS_CELL16)) return hnsw_search_kernel<M, S, TABLE_LDS_CELL16, SHAPE_R128_EF, STRICT>;
    else return nullptr;
}
KernelFn pick(int slots, int table, int shape) {
    if (shape == SHAPE_R128_EF) return table != TABLE_LDS_CELL16 ? nullptr : slots == 1 ? pick_r128_ef<1>() : slots == 2 ? pick_r128_ef<2>() : nullptr;
#if HNSW_PART == 1
    if (table == TABLE_GLOBAL_BITMAP) return pick_slots<TABLE_GLOBAL_BITMAP>(slots);  // lean only: the host never asks for a strict one
#endif
    return table == TABLE_LDS_CELL16 ? pick_slots<TABLE_LDS_CELL16>(slots) : pick_slots<TABLE_LDS_CELL32>(slots);
}
}  // namespace
#if HNSW_PART == 0
template <> hipError_t launch_search_strict<M>(int slots, int table, int shape, uint32_t grid, size_t lds, hipStream_t stream,
                                               const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev) {
    const KernelFn fn = pick(slots, table, shape);
    if (fn == nullptr) return hipErrorInvalidDeviceFunction;
    hipExtLaunchKernelGGL(fn, dim3(grid), dim3(64), (uint32_t)lds, stream, ev.start, ev.stop, 0, ix, a);
    return hipGetLastError();
}
template <> hipError_t occupancy_strict<M>(int slots, int table, int shape, size_t lds, int* per_cu) {
    const KernelFn fn = pick(slots, table, shape);
    if (fn == nullptr) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, 64, lds);
}
#else
template <> hipError_t launch_search_lean<M>(int slots, int table, int shape, uint32_t grid, size_t lds, hipStream_t stream,
                                             const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev) {
    const KernelFn fn = pick(slots, table, shape);
    if (fn == nullptr) return hipErrorInvalidDeviceFunction;
    hipExtLaunchKernelGGL(fn, dim3(grid), dim3(64), (uint32_t)lds, stream, ev.start, ev.stop, 0, ix, a);
    return hipGetLastError();
}
template <> hipError_t occupancy_lean<M>(int slots, int table, int shape, size_t lds, int* per_cu) {
    const KernelFn fn = pick(slots, table, shape);
    if (fn == nullptr) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, 64, lds);
}
// (the pair kernel lives in the lean unit)
#if HNSW_THIS_METRIC < 7
template <> hipError_t launch_search_pair<M>(uint32_t grid, size_t lds, hipStream_t stream, const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev) {
    hipExtLaunchKernelGGL(hnsw_search_pair_kernel<M>, dim3(grid), dim3(64), (uint32_t)lds, stream, ev.start, ev.stop, 0, ix, a);
    return hipGetLastError();
}
template <> hipError_t occupancy_pair<M>(size_t lds, int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, hnsw_search_pair_kernel<M>, 64, lds);
}
#else
template <> hipError_t launch_search_pair<M>(uint32_t, size_t, hipStream_t, const DeviceIndexView&, const SearchArgs&, LaunchEvents) { return hipErrorNotSupported; }
template <> hipError_t occupancy_pair<M>(size_t, int*) { return hipErrorNotSupported; }
#endif
#endif
#endif  // parts 0, 1

#if HNSW_PART == 2
namespace {
// the HBM-bitmap kernels exist in their lean form only
hipError_t launch_search(int slots, int table, int shape, bool strict, uint32_t grid, size_t lds, hipStream_t stream,
                         const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev) {
    return strict && table != TABLE_GLOBAL_BITMAP ? launch_search_strict<M>(slots, table, shape, grid, lds, stream, ix, a, ev)
                                                  : launch_search_lean<M>(slots, table, shape, grid, lds, stream, ix, a, ev);
}
hipError_t occupancy(int slots, int table, int shape, bool strict, size_t lds, int* per_cu) {
    return strict && table != TABLE_GLOBAL_BITMAP ? occupancy_strict<M>(slots, table, shape, lds, per_cu)
                                                  : occupancy_lean<M>(slots, table, shape, lds, per_cu);
}
hipError_t launch_pair(uint32_t grid, size_t lds, hipStream_t stream, const DeviceIndexView& ix, const SearchArgs& a, LaunchEvents ev) {
    return launch_search_pair<M>(grid, lds, stream, ix, a, ev);
}
hipError_t pair_occupancy(size_t lds, int* per_cu) { return occupancy_pair<M>(lds, per_cu); }
hipError_t launch_exact(int ns, uint32_t grid, size_t lds, hipStream_t stream, const DeviceIndexView& ix,
                        const SearchArgs& a, const ExactArgs& x) {
    if (ns == 1) hipLaunchKernelGGL((hnsw_search_exact_kernel<M, 1>), dim3(grid), dim3(64), lds, stream, ix, a, x);
    else if (ns == 2) hipLaunchKernelGGL((hnsw_search_exact_kernel<M, 2>), dim3(grid), dim3(64), lds, stream, ix, a, x);
    else hipLaunchKernelGGL((hnsw_search_exact_kernel<M, 0>), dim3(grid), dim3(64), lds, stream, ix, a, x);
    return hipGetLastError();
}
hipError_t exact_occupancy(int ns, size_t lds, int* per_cu) {
    if (ns == 1) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, hnsw_search_exact_kernel<M, 1>, 64, lds);
    if (ns == 2) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, hnsw_search_exact_kernel<M, 2>, 64, lds);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, hnsw_search_exact_kernel<M, 0>, 64, lds);
}
hipError_t launch_descend(uint32_t grid, hipStream_t stream, const DeviceIndexView& ix, const DescendArgs& a, LaunchEvents ev) {
    if (a.pair != 0u) hipExtLaunchKernelGGL(hnsw_descend_pair_kernel<M>, dim3(grid), dim3(64), 2u * a.tile_bytes + IDS_BYTES, stream, ev.start, ev.stop, 0, ix, a);
    else hipExtLaunchKernelGGL(hnsw_descend_kernel<M>, dim3(grid), dim3(64), a.tile_bytes + IDS_BYTES, stream, ev.start, ev.stop, 0, ix, a);
    return hipGetLastError();
}
hipError_t descend_occupancy(size_t lds, bool pair, int* per_cu) {
    if (pair) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, hnsw_descend_pair_kernel<M>, 64, lds);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, hnsw_descend_kernel<M>, 64, lds);
}
hipError_t launch_order(hipStream_t stream, const PreDescent* pre, uint32_t n, uint32_t* order) {
    hipLaunchKernelGGL(order_desc_kernel, dim3(1), dim3(1024), 0, stream, pre, n, order);
    return hipGetLastError();
}
hipError_t launch_eval_matrix(hipStream_t stream, const float* queries, uint32_t nq, const float* rows, uint32_t n_rows,
                              const double* nrm2, float* out, uint32_t row_stride, uint32_t d, uint32_t nf, bool pairs, int variant) {
    using EvalFn = void (*)(const float*, const float*, const double*, float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
    EvalFn fn = nullptr;
    if (variant == 0) fn = eval_matrix_kernel<M>;
#if HNSW_THIS_METRIC < 7 || HNSW_THIS_METRIC >= 11  // (eval_variant_built: the SIMD-order routine has no variants)
    else if (variant == EVAL_DEEP) fn = eval_matrix_kernel<M, true, false, 0>;
    else if (variant == EVAL_PIPE) fn = eval_matrix_kernel<M, false, true, 0>;
#endif
#if HNSW_THIS_METRIC == 0  // DistL2 on f32 rows, as shape_r128_ef_built
    else if (variant == EVAL_R128 && row_stride == 128u) fn = eval_matrix_kernel<M, false, false, 128>;
    else if (variant == (EVAL_DEEP | EVAL_R128) && row_stride == 128u) fn = eval_matrix_kernel<M, true, false, 128>;
#endif
    if (fn == nullptr) return hipErrorInvalidDeviceFunction;
    const uint32_t tile_bytes = tile_bytes_for(M, row_stride);
    hipLaunchKernelGGL(fn, dim3(pairs ? 1u : (n_rows + nf - 1) / nf, nq), dim3(64), tile_bytes + IDS_BYTES, stream,
                       queries, rows, nrm2, out, n_rows, row_stride, nf, tile_bytes, pairs ? 1u : 0u, d);
    return hipGetLastError();
}
#if HNSW_THIS_METRIC < 7  // construction runs in the scalar arithmetic on f32 rows only: no build kernels for the SIMD-order and half-storage variants
using BuildFn = void (*)(BuildArgs);
BuildFn pick_build(int slots) {
    switch (slots) {
        case 1: return hnsw_build_search_kernel<M, 1>;
        case 2: return hnsw_build_search_kernel<M, 2>;
        case 4: return hnsw_build_search_kernel<M, 4>;
        default: return hnsw_build_search_kernel<M, 16>;
    }
}
hipError_t launch_build_search(int slots, uint32_t grid, size_t lds, hipStream_t stream, const BuildArgs& a) {
    hipLaunchKernelGGL(pick_build(slots), dim3(grid), dim3(64), lds, stream, a);
    return hipGetLastError();
}
hipError_t build_occupancy(int slots, size_t lds, int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, pick_build(slots), 64, lds);
}
hipError_t launch_build_select(uint32_t grid, size_t lds, hipStream_t stream, const SelectArgs& a) {
    hipLaunchKernelGGL(hnsw_build_select_kernel<M>, dim3(grid), dim3(64), lds, stream, a);
    return hipGetLastError();
}
#else
hipError_t launch_build_search(int, uint32_t, size_t, hipStream_t, const BuildArgs&) { return hipErrorNotSupported; }
hipError_t build_occupancy(int, size_t, int*) { return hipErrorNotSupported; }
hipError_t launch_build_select(uint32_t, size_t, hipStream_t, const SelectArgs&) { return hipErrorNotSupported; }
#endif
}  // namespace

template <> const KernelSet& kernels_for<M>() {
    static const KernelSet k{launch_search, occupancy, launch_pair, pair_occupancy, launch_exact, exact_occupancy, launch_descend, descend_occupancy, launch_order, launch_eval_matrix,
                             launch_build_search, build_occupancy, launch_build_select};
    return k;
}
#ifdef HNSW_SHARED_HELPERS
hipError_t launch_allow_bitmap(hipStream_t stream, const uint64_t* origin_id, uint32_t n, const uint64_t* ids, uint64_t m, uint32_t* allow) {
    hipLaunchKernelGGL(allow_bitmap_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, origin_id, n, ids, m, allow);
    return hipGetLastError();
}
hipError_t launch_allow_bitmap_set(hipStream_t stream, const uint64_t* origin_id, uint32_t n, const uint64_t* ids, const uint64_t* offsets,
                                   uint32_t f0, uint32_t n_slots, uint32_t* allow) {
    const uint64_t waves = (uint64_t)n_slots * ((n + 63u) >> 6);  // (the caller keeps this below 2^31: MAX_FILTER_SET_WAVES)
    hipLaunchKernelGGL(allow_bitmap_set_kernel, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, stream, origin_id, n, ids, offsets, f0, n_slots, allow);
    return hipGetLastError();
}
hipError_t launch_filter_of_check(hipStream_t stream, const uint32_t* filter_of, uint32_t nq, uint64_t n_filters, uint32_t* bad) {
    hipLaunchKernelGGL(filter_of_check_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, filter_of, nq, n_filters, bad);
    return hipGetLastError();
}
hipError_t launch_filter_group(hipStream_t stream, const uint32_t* filter_of, uint32_t nq, uint32_t f0, uint32_t n_slots, uint32_t* qlist,
                               uint32_t* slot_of, uint32_t* count) {
    hipLaunchKernelGGL(filter_group_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, filter_of, nq, f0, n_slots, qlist, slot_of, count);
    return hipGetLastError();
}
hipError_t launch_scatter_lists(hipStream_t stream, const uint32_t* upd, uint32_t n_upd, uint32_t rec_words, const BuildLists& lists) {
    hipLaunchKernelGGL(scatter_lists_kernel, dim3((n_upd + 3) / 4), dim3(256), 0, stream, upd, n_upd, rec_words, lists);
    return hipGetLastError();
}
hipError_t launch_lane_lab(hipStream_t stream, size_t lds, const LaneLabArgs& a) {
    hipLaunchKernelGGL(lane_lab_kernel, dim3(1), dim3(64), lds, stream, a);
    return hipGetLastError();
}
hipError_t launch_row_sq_norms(hipStream_t stream, float* vec, double* out, uint32_t n, uint32_t d, uint32_t row_stride) {
    hipLaunchKernelGGL(row_sq_norms_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, vec, out, n, d, row_stride);
    return hipGetLastError();
}
#endif
#endif  // part 2
}  // namespace hnswgpu
