// lane_lab.inc -- included at the end of search_kernels.inc by the one translation unit that carries the metric-independent helpers.
// =======================================================================================
// Lane lab: the wave-level algorithms of the search kernels -- the memory heap (heap_push / heap_push_batch / heap_pop / heap_pop3 /
// heap_push_lds / heap_pop_lds / heap_sift_down_range), the register heap (RegHeap), the result set (r_insert, merge_list) and the 16-bit-cell visited table
// (cell16_test / cell16_insert / visit_cell16) -- run from a SCRIPT by one wavefront; every observable result and the final state
// come back.  tests/test_gpu_lane_lab.py fuzzes these very functions against the oracle's BinaryHeap (src/hnsw.rs:283-297 orders
// its entries), a sequential accept rule (src/hnsw.rs:1028-1053) and a Python set; the Python models of rounds 3-4 only generate
// the scripts now.  hnswgpu_lane_lab is the C-ABI hook (a test entry like hnswgpu_eval_distance_matrix).
// ops[i] = {op, a, b, c}; lanes[set][lane] = {f32 bits, id}: the lane vectors (de / idc) of the batch operations.
// =======================================================================================
struct LabEmit {
    uint32_t* out;
    uint32_t cap, pos;
    __device__ __forceinline__ void put(uint32_t w, int lane) {
        if (lane == 0 && pos < cap) out[pos] = w;
        pos += 1;
    }
    __device__ __forceinline__ void put_h(hent_t e, int lane) {
        put((uint32_t)(e >> 32), lane);
        put((uint32_t)e, lane);
    }
};
__device__ __forceinline__ void lab_load_lanes(const uint32_t* lanes, uint32_t set, int lane, float& de, uint32_t& idc) {
    de = __uint_as_float(lanes[((size_t)set * 64u + (uint32_t)lane) * 2u]);
    idc = lanes[((size_t)set * 64u + (uint32_t)lane) * 2u + 1u];
}
// mode 0: BinaryHeap in memory (top p0 entries in LDS, the rest in the global slice); p1: pops through heap_pop (0) / heap_pop3 (1) /
// heap_pop_lds (2; 3: the form a replayed pop uses, whose root is neither read nor reported); p2 = 2: pushes through heap_push_lds.
// The LDS-only operations need the whole heap in LDS: the host refuses a script whose heap would outgrow p0 entries with them.
__device__ void lab_memheap(const LaneLabArgs& A, LabEmit& E, hent_t* lds, int lane) {
    const HeapMem H{lds, A.scratch, A.p0};
    uint32_t len = 0;
    for (uint32_t i = 0; i < A.n_ops; ++i) {
        const uint32_t op = A.ops[4u * i], a = A.ops[4u * i + 1u], b = A.ops[4u * i + 2u], c = A.ops[4u * i + 3u];
        if (op == LAB_PUSH) {  // p2 != 0: without the parent probe (the form a log replay uses)
            if (len < A.scratch_cap) {
                if (A.p2 == 0u) heap_push(H, len, ((hent_t)a << 32) | b, lane);
                else if (A.p2 == 1u) heap_push<false>(H, len, ((hent_t)a << 32) | b, lane);
                else if (len < A.p0) heap_push_lds(lds, len, ((hent_t)a << 32) | b, lane);
            }
        } else if (op == LAB_POP) {
            if (len == 0u) { E.put_h(~0ull, lane); continue; }
            if (A.p1 >= 2u) {
                if (len > A.p0) continue;
                if (A.p1 == 2u) E.put_h(heap_pop_lds<true>(lds, len, lane), lane);
                else (void)heap_pop_lds<false>(lds, len, lane);
            } else {
                E.put_h(A.p1 == 0u ? heap_pop(H, len, lane) : heap_pop3(H, len, lane), lane);
            }
        } else if (op == LAB_PUSH_LANES) {  // BinaryHeap::push of {-de, idc} for the lanes of the mask, lowest lane first
            float de;
            uint32_t idc;
            lab_load_lanes(A.lanes, c, lane, de, idc);
            const unsigned long long mask = ((unsigned long long)b << 32) | a;
            if (len + popc64(mask) <= A.scratch_cap) heap_push_batch(H, len, mask, de, idc, lane);
        }
    }
    uint32_t end = len;  // into_sorted_vec: swap(0, end), sift_down_range(0, end)
    while (end > 1u) {
        end -= 1;
        const hent_t r0 = hload(H, 0u), re = hload(H, end);
        hfence();
        if (lane == 0) { hstore(H, 0u, re); hstore(H, end, r0); }
        hfence();
        heap_sift_down_range(H, end, lane);
    }
    E.put(len, lane);
    for (uint32_t i = 0; i < len; ++i) E.put_h(hload(H, i), lane);
}
// mode 1: BinaryHeap in registers (return_points of a literal search), p0 = slots per lane
template <int NS>
__device__ void lab_regheap(const LaneLabArgs& A, LabEmit& E, int lane) {
    RegHeap<NS> RR;
#pragma unroll
    for (int s = 0; s < NS; ++s) RR.s[s] = 0ull;
    uint32_t len = 0;
    for (uint32_t i = 0; i < A.n_ops; ++i) {
        const uint32_t op = A.ops[4u * i], a = A.ops[4u * i + 1u], b = A.ops[4u * i + 2u];
        if (op == LAB_PUSH) {  // a full heap takes push-then-pop fused, as literal_return_points does (ef == CAP)
            if (len == RegHeap<NS>::CAP) RR.push_then_pop_full(((hent_t)a << 32) | b, lane);
            else RR.push(len, ((hent_t)a << 32) | b, lane);
        } else if (op == LAB_POP) {
            if (len == 0u) { E.put_h(~0ull, lane); continue; }
            E.put_h(RR.pop(len, lane), lane);
        }
    }
    uint32_t end = len;
    while (end > 1u) {
        end -= 1;
        const hent_t r0 = RR.get(0u), re = RR.get(end);
        RR.set(0u, re, lane);
        RR.set(end, r0, lane);
        RR.sift_down_range(end, lane);
    }
    E.put(len, lane);
    for (uint32_t i = 0; i < len; ++i) E.put_h(RR.get(i), lane);
}
// mode 2: the result set (sorted array in registers, p0 = slots per lane, p1 = ef): r_insert one neighbour at a time, the kernel's
// accept step for a whole list (merge_list when the set is full, one at a time otherwise or when merge_list declines)
template <int S>
__device__ void lab_rset(const LaneLabArgs& A, LabEmit& E, hent_t* merge_buf, int lane) {
    const uint32_t ef = A.p1;  // (the name merge_list_body.inc and the search kernel use)
    float rd[S];
    uint32_t ri[S];
#pragma unroll
    for (int s = 0; s < S; ++s) { rd[s] = 0.f; ri[s] = 0u; }
    uint32_t len = 0;
    float de = 0.f;
    uint32_t idc = 0;
    bool tie_here_out = false;
    unsigned long long acc_out = 0ull;
    auto merge_list = [&](unsigned long long cand) __attribute__((always_inline)) -> bool {
        tie_here_out = false;
        acc_out = 0ull;
#include "merge_list_body.inc"
        tie_here_out = tie_here;
        acc_out = acc;
        return true;
    };
    for (uint32_t i = 0; i < A.n_ops; ++i) {
        const uint32_t op = A.ops[4u * i], x = A.ops[4u * i + 1u], y = A.ops[4u * i + 2u], c = A.ops[4u * i + 3u];
        if (op == LAB_INSERT) {
            const bool tie = r_insert<S>(rd, ri, len, ef, __uint_as_float(x), y, lane);
            E.put(tie ? 1u : 0u, lane);
        } else if (op == LAB_MERGE) {
            lab_load_lanes(A.lanes, c, lane, de, idc);
            const unsigned long long fm = ((unsigned long long)y << 32) | x;
            float worst = len > 0u ? r_worst<S>(rd, len) : INFINITY;
            unsigned long long cand = fm & __ballot(len < ef || de < worst);
            uint32_t taken = 2u;  // 2: merge_list not tried
            if (len == ef && cand != 0ull) {
                taken = merge_list(cand) ? 1u : 0u;
                if (taken == 1u) cand = 0ull;
            }
            E.put(taken, lane);
            E.put(taken == 1u && tie_here_out ? 1u : 0u, lane);
            E.put(taken == 1u ? (uint32_t)acc_out : 0u, lane);
            E.put(taken == 1u ? (uint32_t)(acc_out >> 32) : 0u, lane);
            while (cand != 0ull) {
                const int jl = ctz64(cand);
                const float xd = readlane_f(de, jl);
                if (xd < worst || len < ef) {
                    (void)r_insert<S>(rd, ri, len, ef, xd, readlane_u(idc, jl), lane);
                    worst = r_worst<S>(rd, len);
                }
                cand &= cand - 1ull;
            }
        }
    }
    E.put(len, lane);
    for (uint32_t i = 0; i < len; ++i) {
        E.put(__float_as_uint(r_dist_at<S>(rd, i)), lane);
        E.put(r_id_flag_at<S>(ri, i), lane);
    }
}
// mode 3: the visited table (16-bit cells; p0 = tbits, p1 = idbits, p2 = restbits), the kernel's protocol per batch: test every
// id, the long way for the ids whose home bucket is full, then the insertions of the fresh ones
__device__ void lab_table(const LaneLabArgs& A, LabEmit& E, uint32_t* table, int lane) {
    const uint32_t tbits = A.p0, idbits = A.p1, restbits = A.p2;
    const uint32_t words = (1u << tbits) >> 1;
    for (uint32_t i = (uint32_t)lane; i < words; i += 64) table[i] = 0u;
    __syncthreads();
    for (uint32_t i = 0; i < A.n_ops; ++i) {
        const uint32_t op = A.ops[4u * i], x = A.ops[4u * i + 1u], c = A.ops[4u * i + 3u];
        if (op == LAB_BATCH) {
            float de;
            uint32_t id;
            lab_load_lanes(A.lanes, c, lane, de, id);
            const bool valid = (uint32_t)lane < x;
            bool fresh = false, noroom = false;
            Probe16 pr{};
            int t = 1;
            if (valid) t = cell16_test(table, restbits, idbits, id, pr);
            if (__ballot(t == 2) != 0ull) {
                if (t == 2) {
                    const int vr = visit_cell16(table, tbits, idbits, restbits, id);
                    fresh = vr == 1;
                    noroom = vr == 2;
                }
            }
            wave_lds_fence();
            if (t == 0) {
                fresh = true;
                noroom = cell16_insert(table, tbits, restbits, pr) == 2;
            }
            wave_lds_fence();
            const unsigned long long fm = __ballot(fresh), nm = __ballot(noroom);
            E.put((uint32_t)fm, lane);
            E.put((uint32_t)(fm >> 32), lane);
            E.put((uint32_t)nm, lane);
            E.put((uint32_t)(nm >> 32), lane);
        } else if (op == LAB_VISIT) {  // test + insertion in one go by one lane (the entry point's mark)
            int vr = 0;
            if (lane == 0) vr = visit_cell16(table, tbits, idbits, restbits, x);
            wave_lds_fence();
            E.put((uint32_t)__builtin_amdgcn_readfirstlane(vr), lane);
        }
    }
    __syncthreads();
    E.put(words, lane);
    for (uint32_t i = 0; i < words; ++i) E.put(table[i], lane);
}
__global__ __launch_bounds__(64) void lane_lab_kernel(LaneLabArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = (int)threadIdx.x;
    LabEmit E{A.out, A.out_cap, 1u};
    if (A.mode == 0u) {
        lab_memheap(A, E, reinterpret_cast<hent_t*>(lds_raw), lane);
    } else if (A.mode == 1u) {
        if (A.p0 == 1u) lab_regheap<1>(A, E, lane);
        else if (A.p0 == 2u) lab_regheap<2>(A, E, lane);
        else lab_regheap<4>(A, E, lane);
    } else if (A.mode == 2u) {
        if (A.p0 == 1u) lab_rset<1>(A, E, reinterpret_cast<hent_t*>(lds_raw), lane);
        else if (A.p0 == 2u) lab_rset<2>(A, E, reinterpret_cast<hent_t*>(lds_raw), lane);
        else lab_rset<4>(A, E, reinterpret_cast<hent_t*>(lds_raw), lane);
    } else {
        lab_table(A, E, reinterpret_cast<uint32_t*>(lds_raw), lane);
    }
    __syncthreads();
    if (lane == 0) A.out[0] = E.pos;  // words the script produced (more than out_cap: the buffer was too small)
}
