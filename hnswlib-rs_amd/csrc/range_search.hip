// range_search.hip -- approximate range search through the graph (gfx950 only): the device side of hnswgpu_range_search_batch /
// hnswgpu_range_search_batch_device of include/hnsw_mi355x.h (the entries and every check that needs no device are in capi.cpp).
// DESIGN.md "Approximate range search".
//
// The batch is served in groups of consecutive queries; a group runs rounds at ef = ef_first, 2 ef_first, ... (clamped to ef_max).
// A round is ONE call of DeviceIndex::search_device -- the unchanged batched search, knbn = ef = e -- over the group's pending
// queries, followed by
//   range_cut_kernel      one wavefront per staged row of width e: the longest prefix with dist <= radius (a ballot per 64 entries,
//                         the first failing lane ends it), the stop rule, out_ef / out_flags; a settled row's first m entries are
//                         appended to the group's held answers at a place taken from a running cursor (one atomic add per row: a
//                         scan of m in arrival order), an unsettled row's query number goes to the next round's pending list
//   range_gather_kernel   the pending queries' vectors into the next round's dense query matrix
// and when the group's last query has settled
//   range_offsets_kernel  a scan of m over the group's queries, added to the running total: the CSR offsets
//   range_scatter_kernel  one wavefront per query: its held answers to their CSR slots
// All four are wave-uniform: a row, a query, is one wavefront's.  The pending list's order is arbitrary; answers find their row by
// query number, and a query's answer does not depend on its neighbours in a launch, so the call's output is deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_index.hpp"
#include "hip_host.hpp"
#include "hnswio.hpp"

namespace hnswgpu {
namespace {

constexpr uint64_t RANGE_BUDGET = 256ull << 20;  // bytes of staged answers, of held answers and of gathered queries per group at most
constexpr uint64_t ENTRY_BYTES = 17;             // id, distance, rank, layer
constexpr uint32_t ROWS_PER_WG = 4;              // wavefronts of a workgroup of the row kernels

// answers entry by entry: staged rows of a round (row r, entry j at r e + j), held answers, CSR slots
struct RangeSlots {
    uint64_t* ids;
    float* dists;
    int32_t* rank;   // the caller's may be nullptr; staged and held ones never are
    uint8_t* layer;
};
// `slots` entries behind one another in one block: ids, distances, ranks, layers
ScratchLayout slots_layout(RangeSlots& s, uint64_t slots) {
    ScratchLayout lay;
    lay.arrays(slots, s.ids, s.dists, s.rank, s.layer);
    return lay;
}
uint64_t slots_bytes(uint64_t slots) {
    RangeSlots s{};
    return slots_layout(s, slots).size();
}
// over a block of slots_bytes(at least `slots`): the layout only grows with the slots, so it fits
RangeSlots carve_slots(void* base, uint64_t slots) {
    RangeSlots s{};
    ScratchLayout lay = slots_layout(s, slots);
    (void)lay.place(base, lay.size());
    return s;
}

enum : uint32_t { CTRL_PENDING = 0, CTRL_HELD = 1, CTRL_WORDS = 2 };  // words of the group's control block

struct RangeCutArgs {
    RangeSlots staged;        // the round's answers, rows x e
    const uint32_t* counts;   // [rows] the search's counts
    uint32_t rows, e, ef_max;
    const uint32_t* pend;     // [rows] the query (number in the group) of every row, or nullptr: row r is query r (round 0)
    const float* radii;       // [group] by query
    uint32_t* m_of;           // [group] the answer's length, written when the query settles
    uint32_t* hpos;           // [group] where its held answers start
    uint32_t* out_ef;         // [group] or nullptr
    uint8_t* out_flags;       // [group] or nullptr
    RangeSlots held;          // ids == nullptr: the call only counts
    uint32_t* pend_next;      // the next round's pending list
    uint32_t* ctrl;           // CTRL_PENDING: entries of pend_next; CTRL_HELD: held entries of the group so far
};

// One wavefront per staged row.  Everything that decides a branch is wave-uniform: the row, its count, the ballot.
__global__ __launch_bounds__(64 * ROWS_PER_WG) void range_cut_kernel(RangeCutArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * ROWS_PER_WG + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= a.rows) return;
    const uint32_t q = a.pend ? a.pend[row] : row;
    const float r = a.radii[q];
    const uint32_t c = a.counts[row] < a.e ? a.counts[row] : a.e;
    const size_t s0 = (size_t)row * a.e;
    uint32_t m = 0;
    if (r >= 0.f) {  // (false for NaN and for every negative radius; true for -0.0)
        for (uint32_t j0 = 0; j0 < c; j0 += 64u) {
            const uint32_t valid = c - j0 < 64u ? c - j0 : 64u;
            const bool in = lane < valid && a.staged.dists[s0 + j0 + lane] <= r;  // (a NaN distance fails)
            const uint64_t inside = __ballot(in);
            const uint64_t fail = ~inside & (valid == 64u ? ~0ull : (1ull << valid) - 1ull);
            if (fail != 0ull) {  // the first failing lane ends the prefix
                m += (uint32_t)__ffsll((unsigned long long)fail) - 1u;
                break;
            }
            m += valid;
        }
    }
    const bool settled = m < c || c < a.e || a.e == a.ef_max;
    if (!settled) {
        if (lane == 0u) a.pend_next[atomicAdd(a.ctrl + CTRL_PENDING, 1u)] = q;
        return;
    }
    uint32_t place = 0;
    if (lane == 0u) {
        place = atomicAdd(a.ctrl + CTRL_HELD, m);
        a.m_of[q] = m;
        a.hpos[q] = place;
        if (a.out_ef) a.out_ef[q] = a.e;
        if (a.out_flags) a.out_flags[q] = (m == c && c == a.e) ? (uint8_t)1 : (uint8_t)0;
    }
    if (a.held.ids == nullptr) return;
    place = (uint32_t)__builtin_amdgcn_readfirstlane((int)place);
    for (uint32_t j = lane; j < m; j += 64u) {
        a.held.ids[place + j] = a.staged.ids[s0 + j];
        a.held.dists[place + j] = a.staged.dists[s0 + j];
        a.held.rank[place + j] = a.staged.rank[s0 + j];
        a.held.layer[place + j] = a.staged.layer[s0 + j];
    }
}

// one thread per element of the next round's query matrix: dst[i][j] = src[pend[i]][j]
__global__ __launch_bounds__(256) void range_gather_kernel(const float* __restrict__ src, const uint32_t* __restrict__ pend, uint32_t d, uint64_t total,
                                                          float* __restrict__ dst) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const uint64_t i = e / d;
    const uint32_t j = (uint32_t)(e - i * d);
    dst[e] = src[(size_t)pend[i] * d + j];
}

// ONE workgroup: offsets[q + 1] = base + m_of[0] + ... + m_of[q], goff[q] = m_of[0] + ... + m_of[q - 1], for the n queries of a group.
// Thread t sums a contiguous piece, the 1024 sums are scanned in LDS, the piece is walked again.
__global__ __launch_bounds__(1024) void range_offsets_kernel(const uint32_t* __restrict__ m_of, uint32_t n, uint64_t base, uint64_t* __restrict__ offsets_1,
                                                            uint32_t* __restrict__ goff) {
    __shared__ uint64_t s[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (uint32_t q = lo; q < hi; ++q) sum += m_of[q];
    s[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024u; o <<= 1) {
        const uint64_t v = t >= o ? s[t - o] : 0ull;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    uint64_t run = s[t] - sum;
    for (uint32_t q = lo; q < hi; ++q) {
        goff[q] = (uint32_t)run;
        run += m_of[q];
        offsets_1[q] = base + run;
    }
}

// one wavefront per query of the group: its held answers to the slots goff[q] .. of dst
__global__ __launch_bounds__(64 * ROWS_PER_WG) void range_scatter_kernel(RangeSlots held, const uint32_t* __restrict__ m_of, const uint32_t* __restrict__ hpos,
                                                                        const uint32_t* __restrict__ goff, uint32_t n, RangeSlots dst) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * ROWS_PER_WG + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (q >= n) return;
    const uint32_t m = m_of[q], from = hpos[q], to = goff[q];
    for (uint32_t j = lane; j < m; j += 64u) {
        dst.ids[to + j] = held.ids[from + j];
        dst.dists[to + j] = held.dists[from + j];
        if (dst.rank) dst.rank[to + j] = held.rank[from + j];
        if (dst.layer) dst.layer[to + j] = held.layer[from + j];
    }
}

// the queries of one group at most: the hook, and what keeps every buffer of a group within its budget
uint64_t range_group_size(uint64_t nq, uint64_t d, uint64_t ef_max) {
    const int64_t knob = knobs().range_chunk;
    const uint64_t by_answers = RANGE_BUDGET / (ef_max * ENTRY_BYTES), by_queries = RANGE_BUDGET / (d * 4);
    return std::max<uint64_t>(1, std::min<uint64_t>({nq, by_answers, by_queries, knob > 0 ? (uint64_t)knob : nq}));
}

// both entries.  host: every buffer of `a` but the filter is plain host memory (the filter has been copied); else device memory.
int range_rounds(DeviceIndex& dev, const RangeSearchArgs& a, bool host, hipStream_t stream, std::string& err) {
    const uint64_t nq = a.nq, d = a.d;
    DeviceGuard on(dev.device());
    HIP_TRY(on.status());
    DevMem m_small, m_staged, m_held;
    Drain drain{stream};  // (destroyed first: nothing of this call is running when its memory is freed)

    const uint64_t group = range_group_size(nq, d, a.ef_max);
    const uint64_t slots = group * a.ef_max;  // of a round's staged answers and of the group's held answers at most
    const bool keep = a.out_ids != nullptr;   // (else the count-only call)
    // the group's small arrays, one block
    float *d_qround, *d_qgroup = nullptr, *d_radii;
    uint32_t *d_pend[2], *d_counts, *d_m, *d_hpos, *d_goff, *d_ef, *d_ctrl;
    uint64_t* d_offs;
    uint8_t* d_flags;
    ScratchLayout lay;
    lay.array(d_qround, group * d);
    if (host) lay.array(d_qgroup, group * d);
    // (d_radii, d_ef, d_offs, d_flags: host calls)
    lay.arrays(group, d_radii, d_pend[0], d_pend[1], d_counts, d_m, d_hpos, d_goff, d_ef, d_offs, d_flags);
    lay.array(d_ctrl, 64);
    const int rc_small = alloc_layout("range search", m_small, lay, err);
    if (rc_small != OK) return rc_small;
    HIP_TRY(m_staged.alloc(slots_bytes(slots)));
    if (keep) HIP_TRY(m_held.alloc(slots_bytes(slots)));
    const RangeSlots held = keep ? carve_slots(m_held.p, slots) : RangeSlots{};

    if (host) a.out_offsets[0] = 0;
    else HIP_TRY(hipMemsetAsync(a.out_offsets, 0, 8, stream));
    // (a filter that is empty still is a filter: a non-null pointer that is never dereferenced)
    const uint64_t* d_allowed = a.filtered ? (a.allowed ? a.allowed : reinterpret_cast<const uint64_t*>(d_ctrl)) : nullptr;

    uint64_t total = 0;
    bool overflow = false;  // the answers no longer fit cap: the groups from here on only count
    for (uint64_t g0 = 0; g0 < nq; g0 += group) {
        const uint64_t gq = std::min(group, nq - g0);
        const float* q_group = a.queries + g0 * d;
        const float* r_group = a.radii + g0;
        if (host) {
            HIP_TRY(hipMemcpyAsync(d_qgroup, q_group, gq * d * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_radii, r_group, gq * 4, hipMemcpyHostToDevice, stream));
            q_group = d_qgroup;
            r_group = d_radii;
        }
        const bool hold = keep && !overflow;
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, CTRL_WORDS * 4, stream));
        uint32_t h_ctrl[CTRL_WORDS] = {0, 0};
        uint64_t rows = gq, e = a.ef_first;
        const uint32_t* pend = nullptr;  // round 0: the group's rows in place
        for (unsigned round = 0;; ++round) {
            const RangeSlots staged = carve_slots(m_staged.p, rows * e);
            int rc = dev.search_device(pend ? d_qround : q_group, rows, d, e, e, staged.ids, staged.dists, staged.layer, staged.rank, d_counts, nullptr, stream,
                                       d_allowed, a.n_allowed, nullptr, err);
            if (rc != OK) return rc;
            uint32_t* pend_next = d_pend[round & 1u];
            RangeCutArgs c{};
            c.staged = staged; c.counts = d_counts; c.rows = (uint32_t)rows; c.e = (uint32_t)e; c.ef_max = (uint32_t)a.ef_max;
            c.pend = pend; c.radii = r_group; c.m_of = d_m; c.hpos = d_hpos;
            c.out_ef = host ? (a.out_ef ? d_ef : nullptr) : (a.out_ef ? a.out_ef + g0 : nullptr);
            c.out_flags = host ? (a.out_flags ? d_flags : nullptr) : (a.out_flags ? a.out_flags + g0 : nullptr);
            c.held = hold ? held : RangeSlots{};
            c.pend_next = pend_next; c.ctrl = d_ctrl;
            HIP_TRY(hipMemsetAsync(d_ctrl + CTRL_PENDING, 0, 4, stream));
            hipLaunchKernelGGL(range_cut_kernel, dim3((uint32_t)((rows + ROWS_PER_WG - 1) / ROWS_PER_WG)), dim3(64 * ROWS_PER_WG), 0, stream, c);
            HIP_TRY(hipGetLastError());
            // the one read-back of a round: how many queries the next launch searches (and how much the group holds so far)
            HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, CTRL_WORDS * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (h_ctrl[CTRL_PENDING] == 0) break;
            if (e >= a.ef_max || h_ctrl[CTRL_PENDING] > rows) { err = "range search: a query is pending behind the last round"; return ERR_DEVICE; }
            rows = h_ctrl[CTRL_PENDING];
            e = std::min<uint64_t>(2 * e, a.ef_max);
            pend = pend_next;
            hipLaunchKernelGGL(range_gather_kernel, dim3((uint32_t)((rows * d + 255) / 256)), dim3(256), 0, stream, q_group, pend, (uint32_t)d, rows * d, d_qround);
            HIP_TRY(hipGetLastError());
        }
        const uint64_t gtotal = h_ctrl[CTRL_HELD];
        if (gtotal > slots) { err = "range search: a group holds more answers than its bound"; return ERR_DEVICE; }
        hipLaunchKernelGGL(range_offsets_kernel, dim3(1), dim3(1024), 0, stream, d_m, (uint32_t)gq, total, host ? d_offs : a.out_offsets + g0 + 1, d_goff);
        HIP_TRY(hipGetLastError());
        if (total + gtotal > a.cap) overflow = true;
        if (hold && !overflow && gtotal != 0) {
            // (the round's staged answers are done with: a host call's CSR slots are staged in their place)
            const RangeSlots dst = host ? carve_slots(m_staged.p, gtotal)
                                        : RangeSlots{a.out_ids + total, a.out_dists + total, a.out_rank ? a.out_rank + total : nullptr,
                                                     a.out_layer ? a.out_layer + total : nullptr};
            hipLaunchKernelGGL(range_scatter_kernel, dim3((uint32_t)((gq + ROWS_PER_WG - 1) / ROWS_PER_WG)), dim3(64 * ROWS_PER_WG), 0, stream, held, d_m, d_hpos,
                               d_goff, (uint32_t)gq, dst);
            HIP_TRY(hipGetLastError());
            if (host) {
                HIP_TRY(hipMemcpyAsync(a.out_ids + total, dst.ids, gtotal * 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipMemcpyAsync(a.out_dists + total, dst.dists, gtotal * 4, hipMemcpyDeviceToHost, stream));
                if (a.out_rank) HIP_TRY(hipMemcpyAsync(a.out_rank + total, dst.rank, gtotal * 4, hipMemcpyDeviceToHost, stream));
                if (a.out_layer) HIP_TRY(hipMemcpyAsync(a.out_layer + total, dst.layer, gtotal, hipMemcpyDeviceToHost, stream));
            }
        }
        if (host) {
            HIP_TRY(hipMemcpyAsync(a.out_offsets + g0 + 1, d_offs, gq * 8, hipMemcpyDeviceToHost, stream));
            if (a.out_ef) HIP_TRY(hipMemcpyAsync(a.out_ef + g0, d_ef, gq * 4, hipMemcpyDeviceToHost, stream));
            if (a.out_flags) HIP_TRY(hipMemcpyAsync(a.out_flags + g0, d_flags, gq, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));  // the group's buffers are the next group's
        total += gtotal;
    }
    if (total > a.cap) {
        err = "the answers need " + std::to_string(total) + " slots, cap is " + std::to_string(a.cap);
        return HNSWGPU_ERR_CAPACITY;
    }
    return OK;
}

}  // namespace

// The device side of hnswgpu_range_search_batch(_device); capi.cpp holds the entries and every argument check (capi_index.hpp).
// Waits for the stream before it returns.
int range_search(DeviceIndex* dev, const RangeSearchArgs& a, bool host, void* stream_v, std::string& err) {
    if (!host) {
        hipStream_t stream = static_cast<hipStream_t>(stream_v);
        if (dev == nullptr || a.nq == 0) {  // no point, or no query: every answer is empty
            HIP_TRY(hipMemsetAsync(a.out_offsets, 0, (a.nq + 1) * 8, stream));
            if (a.out_ef && a.nq != 0) HIP_TRY(hipMemsetAsync(a.out_ef, 0, a.nq * 4, stream));
            if (a.out_flags && a.nq != 0) HIP_TRY(hipMemsetAsync(a.out_flags, 0, a.nq, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            return OK;
        }
        return range_rounds(*dev, a, false, stream, err);
    }
    // host buffers (the caller has answered an empty index and an empty batch itself): the filter goes to the device once
    DeviceGuard on(dev->device());
    HIP_TRY(on.status());
    DevMem m_allowed;
    RangeSearchArgs b = a;
    if (a.filtered && a.n_allowed != 0) {
        HIP_TRY(m_allowed.alloc(a.n_allowed * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(m_allowed.p, a.allowed, a.n_allowed * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    b.allowed = static_cast<const uint64_t*>(m_allowed.p);
    return range_rounds(*dev, b, true, nullptr, err);
}

}  // namespace hnswgpu
