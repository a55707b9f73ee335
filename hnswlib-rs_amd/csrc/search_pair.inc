// search_pair.inc -- search_layer (src/hnsw.rs:922-1064) for TWO queries per wavefront (included by search_kernels.inc).
//
// Why.  A search of a short-row index (BASELINE config 3: d = 25, M = 24, ef = 128) is bound by the instructions of an expansion, not
// by bytes: ~400 vector + ~300 scalar instructions to consume the nine fresh 100-byte rows of a list, and most of them do not get
// cheaper when the row is short -- the selection of the next candidate, the visited test, the accept rule are wave-wide steps that
// keep 64 lanes busy with one query's 28 ids.  Here lanes 0-31 and 32-63 each own a query and share the instruction stream:
//   * return_points / candidate_points of a query: ONE array sorted by distance with an EXPANDED flag per entry (as in
//     hnsw_search_kernel), 32 lanes x 4 slots (ef <= 128), ALWAYS ef entries long -- the entries a shorter reference heap does not
//     have are (+inf, EXPANDED) sentinels, so "fewer than ef entries" and "nearer than the farthest" (:1028-1037) are one test --
//     and mirrored in LDS, where a lane can read any entry;
//   * per-query ("per-half") quantities that come out of a vote are the two 32-bit halves of the 64-bit ballot: no loop over halves;
//   * the accept rule of a whole round of <= 16 fresh rows per query is evaluated by the candidates' own lanes (merge_list, DESIGN.md
//     section 4.4, without its loop over candidates): neighbour j of the list is accepted iff cr_j + cb_j < ef, cr_j = entries of R not
//     farther than it (votes over the registers for <= 4 candidates, else a binary search in the LDS mirror, one per lane),
//     cb_j = EARLIER candidates of the round not farther than it
//     (<= 15 DPP row shifts: a round's candidates sit in one row of 16 lanes).  [Counting all earlier candidates instead of the
//     accepted ones is the same rule: i < j, d_i <= d_j and i refused => cr_j + cb_j >= cr_i + cb_i >= ef, j is refused either way.]
//     The new array is written with one scatter into the mirror (an entry of R moves up by the number of accepted candidates whose
//     cr is <= its index, an accepted candidate lands at cr + its rank among the accepted) and read back.
// What it does not do: resolve ties.  It watches for the places where equal distances make the reference's answer depend on its
// heaps' internal order -- the three of hnsw_search_kernel: (A) a pop with two equal nearest candidates, (B) here simply: equal
// entries on both sides of the cut at ef when the array is rebuilt, (C) equal distances inside the first k answers or across their
// end -- and hands such a query on: a strict call searches it again with hnsw_search_kernel (a.pair_ties_to_retry; the half stops
// at once), a lean call reports status 2 like the lean kernel.  Equal distances that never reach one of the three cost nothing.  A visited table that fills up
// moves to the half's HBM bitmap slice inside the launch (no slice: the query goes to the retry list).  The host (search_device.hip) runs this kernel as a first
// pass over the whole batch and the one-query kernels over what it hands back.
#ifndef HNSW_LB_PAIR
#define HNSW_LB_PAIR 3  // waves per SIMD the pair kernel is built for
#endif

constexpr uint32_t PAIR_NONE = 0xFFu;  // no unexpanded entry left (entry indices are < 128)

template <int K>
__device__ __forceinline__ float dpp_row_shr_inf(float v) {  // value of lane - K of the same row of 16 lanes, +inf where the row ends
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0x7F800000, __builtin_bit_cast(int, v), 0x110 + K, 0xf, 0xf, false));
}
template <int K>
__device__ __forceinline__ float dpp_row_shl_inf(float v) {  // value of lane + K
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0x7F800000, __builtin_bit_cast(int, v), 0x100 + K, 0xf, 0xf, false));
}
// candidates 0 .. n - 1 of a round in lanes 0 .. n - 1 of a row (the lanes behind them hold +inf):
// cnt = earlier candidates not farther than this lane's, eq = one of them at exactly its distance
template <int K>
__device__ __forceinline__ void pair_count_before(float xd, uint32_t nmax, uint32_t& cnt, bool& eq) {
    if constexpr (K < 16) {
        if ((uint32_t)K < nmax) {  // (wave-uniform)
            const float o = dpp_row_shr_inf<K>(xd);
            cnt += o <= xd ? 1u : 0u;
            eq = eq || o == xd;
            pair_count_before<K + 1>(xd, nmax, cnt, eq);
        }
    }
}
// cnt = LATER accepted candidates (xa: their distance, +inf in the other lanes) strictly nearer than this lane's
template <int K>
__device__ __forceinline__ void pair_count_after(float xa, float xd, uint32_t nmax, uint32_t& cnt) {
    if constexpr (K < 16) {
        if ((uint32_t)K < nmax) {
            const float o = dpp_row_shl_inf<K>(xa);
            cnt += o < xd ? 1u : 0u;
            pair_count_after<K + 1>(xa, xd, nmax, cnt);
        }
    }
}
__device__ __forceinline__ uint32_t lo32(unsigned long long m) { return (uint32_t)m; }
__device__ __forceinline__ uint32_t hi32(unsigned long long m) { return (uint32_t)(m >> 32); }
// rank of this lane among the set lanes of ITS half (ma / mb: the vote's halves)
__device__ __forceinline__ uint32_t half_rank(bool hi, uint32_t ma, uint32_t mb) {
    const uint32_t ra = __builtin_amdgcn_mbcnt_lo(ma, 0u), rb = __builtin_amdgcn_mbcnt_hi(mb, 0u);
    return hi ? rb : ra;
}
__device__ __forceinline__ uint32_t pair_first(unsigned long long m01, unsigned long long m23) {
    return m01 != 0ull ? (uint32_t)ctz64(m01) : m23 != 0ull ? 64u + (uint32_t)ctz64(m23) : PAIR_NONE;
}

// A half whose visited set outgrows its LDS table carries on in an HBM bitmap slice (as migrate_table_to_bitmap: the cells identify
// their ids exactly); all 64 lanes help.  Out of line: a few queries in a hundred.
__device__ __attribute__((noinline, unused)) void pair_migrate_to_bitmap(uint32_t* bitmap, uint32_t words, const uint32_t* table, uint32_t table_cells,
                                                                 uint32_t restbits, uint32_t idbits) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < words; i += 64u) bitmap[i] = 0u;
    __syncthreads();
    for (uint32_t i = lane; i < table_cells; i += 64u) {
        const uint32_t cell = (table[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
        if (cell != 0u) {
            const uint32_t bdisp = (cell & 0x7FFFu) >> restbits;
            const uint32_t rest = cell & ((1u << restbits) - 1u);
            const uint32_t home = ((i >> 3) - bdisp) & ((table_cells >> 3) - 1u);  // home bucket
            const uint32_t id = unmix_id((home << restbits) | rest, idbits);
            atomicOr(&bitmap[id >> 5], 1u << (id & 31u));
        }
    }
    __syncthreads();
}
#ifndef HNSW_PAIR_PHASES
#define HNSW_PAIR_PHASES 0  // 1: cycles per phase of the expansion loop into stats words 4-7 (profiling builds: tools/pair_phases.py)
#endif
#if HNSW_PAIR_PHASES
#define PP_T(var) const unsigned long long var = clock64()
#define PP_ACC(idx, t0, t1) pph[idx] += (uint32_t)((t1) - (t0))
#else
#define PP_T(var)
#define PP_ACC(idx, t0, t1)
#endif

template <int METRIC>
__global__ __launch_bounds__(64, HNSW_LB_PAIR) void hnsw_search_pair_kernel(DeviceIndexView ix, SearchArgs a) {
    if constexpr (METRIC < KM_SIMD8_FIRST) {
        extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
        const int lane = (int)threadIdx.x;
        const uint32_t half = (uint32_t)lane >> 5, hl = (uint32_t)lane & 31u;
        const bool hi = half != 0u;
        const uint32_t ef = a.ef, k = a.k;
        const uint32_t table_cells = 1u << a.tbits, table_words = table_cells >> 1;
        const uint32_t table_limit = table_cells - (table_cells >> 2);  // stop at 75 % load
        const uint32_t ef_pad = (ef + 2u) & ~1u;  // ef entries + the nearest one that left at the last rebuild (position ef)
        uint32_t ef_pow2 = 1u;
        while (ef_pow2 < ef) ef_pow2 <<= 1;
        // LDS: [query A][query B][ids A: 64][ids B: 64][table A][table B][R mirror A: ef_pad][R mirror B][candidates A: 16][B][cr list A: 16][B]
        unsigned char* p = lds_raw;
        float4* tile = reinterpret_cast<float4*>(p + (size_t)half * a.tile_bytes);
        p += 2u * (size_t)a.tile_bytes;
        uint32_t* ids_h = reinterpret_cast<uint32_t*>(p) + half * 64u;
        p += 2u * IDS_BYTES;
        uint32_t* table_h = reinterpret_cast<uint32_t*>(p) + half * table_words;
        p += 2u * (size_t)table_words * 4u;
        hent_t* rm_h = reinterpret_cast<hent_t*>(p) + half * ef_pad;
        p += 2u * (size_t)ef_pad * sizeof(hent_t);
        hent_t* cb_h = reinterpret_cast<hent_t*>(p) + half * 16u;
        p += 2u * 16u * sizeof(hent_t);
        uint32_t* ab_h = reinterpret_cast<uint32_t*>(p) + half * 16u;
        const float* rm_f = reinterpret_cast<const float*>(rm_h);  // key of entry j: rm_f[2 j + 1]; id word: [2 j]
        const nrm_ptr_t nrm2 = (nrm_ptr_t)a.nrm2;
        const uint32_t row_stride = ix.row_stride, nchunk = row_stride >> 2, deg = ix.deg_stride;
        const uint32_t npairs = (a.nq + 1u) >> 1;
        uint32_t* const counters = a.overflow_count;
        // HBM bitmap slices for the halves whose table fills up: two per workgroup (none: such a query goes to the retry list)
        const bool have_bm = 2u * blockIdx.x + 1u < a.bitmap_blocks;
        uint32_t* const bm_a = a.bitmap + (size_t)(2u * blockIdx.x) * a.bitmap_words;
        uint32_t* const bm_h = bm_a + (size_t)half * a.bitmap_words;
        uint32_t* const tables = table_h - half * table_words;
        const kernargs_t ka = (kernargs_t)__builtin_amdgcn_kernarg_segment_ptr();  // (layer_offset[] is indexed at run time: read from the kernarg segment)

        bool first_item = true;
        for (;;) {
            uint32_t wi;
            if (first_item) {
                wi = blockIdx.x;
            } else {
                uint32_t t = 0;
                if (lane == 0) t = atomicAdd(a.work_counter, 1u);
                wi = readlane_u(t, 0) + gridDim.x;
            }
            first_item = false;
            if (wi >= npairs) break;
            const uint32_t t_start = (uint32_t)wall_clock64();
            const bool mine_b = 2u * wi + 1u < a.nq;  // (an odd count: the last wave's second half idles)
            const bool mine = !hi || mine_b;
            const uint32_t wq = 2u * wi + (mine ? half : 0u);
            const uint32_t q = a.qlist ? a.qlist[wq] : wq;
            // ---- the query's row, its visited table, what the descent left (hnsw_descend_kernel)
            const float4* src = reinterpret_cast<const float4*>(a.queries + (size_t)q * row_stride);
            for (uint32_t c = hl; c < nchunk; c += 32u) tile[c] = src[c];
            {
                uint4* t4 = reinterpret_cast<uint4*>(table_h);
                for (uint32_t i = hl; i < (table_words >> 2); i += 32u) t4[i] = make_uint4(0u, 0u, 0u, 0u);
            }
            const PreDescent pd = a.pre[q];
            __syncthreads();
            if constexpr (METRIC == DIST_COSINE) {  // finish_staged_query, per half
                double s1 = 0.;
                for (uint32_t c = 0; c < nchunk; ++c) {
                    const float4 v = tile[c];
                    s1 = s1 + (double)(v.x * v.x); s1 = s1 + (double)(v.y * v.y); s1 = s1 + (double)(v.z * v.z); s1 = s1 + (double)(v.w * v.w);
                }
                if (hl == 0u) *reinterpret_cast<double*>(tile + nchunk) = s1;
            }
            const uint32_t pivot = pd.pivot;
            const float dcur = __uint_as_float(pd.dcur_bits);
            float rd[4];
            uint32_t ri[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) { rd[s] = INFINITY; ri[s] = EXPANDED; }
            if (hl == 0u) { rd[0] = dcur; ri[0] = pivot; }  // dist_to_entry_point (:952); a half that idles starts with nothing to expand
            if (!mine) ri[0] = EXPANDED;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint32_t j = (uint32_t)s * 32u + hl;
                if (j < ef) rm_h[j] = hmake(rd[s], ri[s]);
            }
            if (hl == 0u) {
                rm_h[ef] = hmake(-1.f, 0u);  // (position ef: nothing has left yet)
                ids_h[0] = pivot;
                (void)visit_cell16(table_h, a.tbits, a.idbits, a.restbits, pivot);
            }
            wave_lds_fence();
            float worst_v = rm_f[2u * (ef - 1u) + 1u];  // the farthest entry (+inf while the reference's heap is not full)
            // per-half scalars: A = lanes 0-31, B = lanes 32-63
            uint32_t done = 0u;          // bit 0 / 1: the half has finished (or given up)
            uint32_t st_a = 0u, st_b = 0u;      // 1: visited table full -> retry list
            uint32_t tie_a = 0u, tie_b = 0u;    // an accepted neighbour met an equal distance
            uint32_t nvis_a = 1u, nvis_b = 1u, nexp_a = 0u, nexp_b = 0u, len_a = 1u, len_b = 1u;
            uint32_t my_ids = 0u;        // ids this lane read (summed per half at the end)
            uint32_t bm = 0u;            // bit 0 / 1: the half's visited set lives in its HBM bitmap slice
#if HNSW_PAIR_PHASES
            uint32_t pph[4] = {0u, 0u, 0u, 0u};
#endif
            auto to_bitmap = [&](uint32_t h) __attribute__((always_inline)) {  // (h: wave-uniform)
                pair_migrate_to_bitmap(bm_a + (size_t)h * a.bitmap_words, a.bitmap_words, tables + h * table_words, table_cells, a.restbits, a.idbits);
                bm |= 1u << h;
            };
            uint32_t spec_for = EMPTY_SLOT, spec0 = EMPTY_SLOT, spec1 = EMPTY_SLOT;  // prefetched id row of the likely next candidate
            float spec_key = INFINITY;   // ... and that candidate's distance

            for (;;) {
                PP_T(pt0);
                // ---- c = nearest unexpanded entry (candidate_points.pop(), :971); none left: the search of that half is over (:981-993)
                unsigned long long m[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) m[s] = __ballot((ri[s] & EXPANDED) == 0u);
                unsigned long long a01 = (m[0] & 0xFFFFFFFFull) | (m[1] << 32), a23 = (m[2] & 0xFFFFFFFFull) | (m[3] << 32);
                unsigned long long b01 = (m[0] >> 32) | (m[1] & 0xFFFFFFFF00000000ull), b23 = (m[2] >> 32) | (m[3] & 0xFFFFFFFF00000000ull);
                uint32_t cj_a = (done & 1u) ? PAIR_NONE : pair_first(a01, a23);
                uint32_t cj_b = (done & 2u) ? PAIR_NONE : pair_first(b01, b23);
                if (cj_a == PAIR_NONE) done |= 1u;
                if (cj_b == PAIR_NONE) done |= 2u;
                if (done == 3u) break;
                const uint32_t cj_v = hi ? cj_b : cj_a;
                const bool act = cj_v != PAIR_NONE;
                uint32_t c_v = 0u;
                float c_key = -1.f;
                if (act) {
                    c_v = reinterpret_cast<const uint32_t*>(rm_h)[2u * cj_v];  // (unexpanded: no flag in the word)
                    c_key = rm_f[2u * cj_v + 1u];
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (cj_v == (uint32_t)s * 32u + hl) {
                        ri[s] |= EXPANDED;
                        reinterpret_cast<uint32_t*>(rm_h)[2u * cj_v] = ri[s];
                    }
                nexp_a += cj_a != PAIR_NONE ? 1u : 0u;
                nexp_b += cj_b != PAIR_NONE ? 1u : 0u;
                // a table about to fill up: the half's visited set moves to its HBM bitmap slice (none: the query goes to the retry list)
                {
                    const bool full_a = cj_a != PAIR_NONE && (bm & 1u) == 0u && nvis_a + 64u > table_limit;
                    const bool full_b = cj_b != PAIR_NONE && (bm & 2u) == 0u && nvis_b + 64u > table_limit;
                    if (full_a || full_b) {
                        if (have_bm) {
                            if (full_a) to_bitmap(0u);
                            if (full_b) to_bitmap(1u);
                        } else {
                            if (full_a) { st_a = 1u; done |= 1u; cj_a = PAIR_NONE; }
                            if (full_b) { st_b = 1u; done |= 2u; cj_b = PAIR_NONE; }
                            if (done == 3u) break;
                        }
                    }
                }
                const bool go = (hi ? cj_b : cj_a) != PAIR_NONE;
                uint32_t id0 = EMPTY_SLOT, id1 = EMPTY_SLOT;
                if (go) {
                    if (spec_for == c_v) {
                        id0 = spec0;
                        id1 = spec1;
                    } else {
                        const uint32_t* nrow = ix.nbr0 + (size_t)c_v * deg;
                        if (hl < deg) id0 = nrow[hl];
                        if (hl + 32u < deg) id1 = nrow[hl + 32u];
                    }
                }
                const bool val0 = id0 != EMPTY_SLOT, val1 = id1 != EMPTY_SLOT;
                my_ids += (val0 ? 1u : 0u) + (val1 ? 1u : 0u);
                const unsigned long long anyid = __ballot(val0);  // (lists are padded at the end only; the ids are in registers from here on)
                {   // the likely next candidate's id row: requested now, behind this list's ids, used one expansion later
                    if (cj_a < 64u) a01 &= ~(1ull << cj_a); else if (cj_a < 128u) a23 &= ~(1ull << (cj_a - 64u));
                    if (cj_b < 64u) b01 &= ~(1ull << cj_b); else if (cj_b < 128u) b23 &= ~(1ull << (cj_b - 64u));
                    const uint32_t nj_a = (done & 1u) ? PAIR_NONE : pair_first(a01, a23);
                    const uint32_t nj_b = (done & 2u) ? PAIR_NONE : pair_first(b01, b23);
                    const uint32_t nj_v = hi ? nj_b : nj_a;
                    spec_for = EMPTY_SLOT;
                    spec_key = INFINITY;
                    if (nj_v != PAIR_NONE) {
                        spec_for = reinterpret_cast<const uint32_t*>(rm_h)[2u * nj_v];
                        spec_key = rm_f[2u * nj_v + 1u];
                    }
                    // (A) of hnsw_search_kernel: candidate_points.pop() with two equal nearest candidates -- the popped entry has an
                    // equal, still unexpanded successor: which one the reference's heap hands out is its internal order
                    const unsigned long long pa = __ballot(go && nj_v != PAIR_NONE && spec_key == c_key);
                    if (pa != 0ull) {
                        if (lo32(pa) != 0u) { tie_a = 1u; if (a.pair_ties_to_retry != 0u) done |= 1u; }
                        if (hi32(pa) != 0u) { tie_b = 1u; if (a.pair_ties_to_retry != 0u) done |= 2u; }
                    }
                    if (nj_v != PAIR_NONE) {
                        const uint32_t* srow = ix.nbr0 + (size_t)spec_for * deg;
                        spec0 = hl < deg ? srow[hl] : EMPTY_SLOT;
                        spec1 = hl + 32u < deg ? srow[hl + 32u] : EMPTY_SLOT;
                    }
                }
                PP_T(pt1);
                PP_ACC(0, pt0, pt1);  // selection, the wait for the id row, the prefetch
                if (anyid == 0ull) continue;
                // ---- visited test of every id (LDS table: nothing written yet, the fresh ones are inserted behind their row loads;
                // HBM bitmap: tested and marked in one atomic)
                Probe16 p0{}, p1{};
                int t0 = 1, t1 = 1;
                bool fresh0 = false, fresh1 = false;
                const bool on_bm = ((bm >> half) & 1u) != 0u;
                if (bm == 0u) {  // (wave-uniform, the usual case) no divergence: an EMPTY slot probes some bucket and its result is dropped
                    const int u0 = cell16_test(table_h, a.restbits, a.idbits, id0, p0);
                    const int u1 = cell16_test(table_h, a.restbits, a.idbits, id1, p1);
                    t0 = val0 ? u0 : 1;
                    t1 = val1 ? u1 : 1;
                    fresh0 = t0 == 0;
                    fresh1 = t1 == 0;
                } else if (!on_bm) {
                    if (val0) t0 = cell16_test(table_h, a.restbits, a.idbits, id0, p0);
                    if (val1) t1 = cell16_test(table_h, a.restbits, a.idbits, id1, p1);
                    fresh0 = t0 == 0;
                    fresh1 = t1 == 0;
                } else {
                    if (val0) fresh0 = visit_bitmap(bm_h, id0) == 1;
                    if (val1) fresh1 = visit_bitmap(bm_h, id1) == 1;
                }
                bool ins0 = !on_bm && fresh0, ins1 = !on_bm && fresh1;
                if (__ballot(t0 == 2 || t1 == 2) != 0ull) {  // a full home bucket: looked up (and marked) the long way, now
                    int vr0 = 0, vr1 = 0;
                    if (t0 == 2) vr0 = visit_cell16(table_h, a.tbits, a.idbits, a.restbits, id0);
                    if (t1 == 2) vr1 = visit_cell16(table_h, a.tbits, a.idbits, a.restbits, id1);
                    fresh0 = fresh0 || vr0 == 1;
                    fresh1 = fresh1 || vr1 == 1;
                    const unsigned long long ovf = __ballot(vr0 == 2 || vr1 == 2);  // displacement budget exhausted (rare)
                    if (ovf != 0ull) {
                        const bool mine_ovf = hi ? hi32(ovf) != 0u : lo32(ovf) != 0u;
                        if (have_bm) {  // the set moves to the bitmap (with what this list already placed); the ids on their way are marked there
                            if (lo32(ovf) != 0u) to_bitmap(0u);
                            if (hi32(ovf) != 0u) to_bitmap(1u);
                            if (mine_ovf) {
                                if (vr0 == 2 || t0 == 0) fresh0 = visit_bitmap(bm_h, id0) == 1;
                                if (vr1 == 2 || t1 == 0) fresh1 = visit_bitmap(bm_h, id1) == 1;
                                ins0 = ins1 = false;
                            }
                        } else {
                            if (lo32(ovf) != 0u) { st_a = 1u; done |= 1u; }
                            if (hi32(ovf) != 0u) { st_b = 1u; done |= 2u; }
                            if (mine_ovf) { fresh0 = fresh1 = ins0 = ins1 = false; }
                        }
                    }
                }
                const unsigned long long fm0 = __ballot(fresh0), fm1 = __ballot(fresh1);
                if ((fm0 | fm1) == 0ull) continue;
                const uint32_t f0_a = (uint32_t)__popc(lo32(fm0)), f0_b = (uint32_t)__popc(hi32(fm0));
                const uint32_t nf_a = f0_a + (uint32_t)__popc(lo32(fm1)), nf_b = f0_b + (uint32_t)__popc(hi32(fm1));
                nvis_a += nf_a;
                nvis_b += nf_b;
                // compaction in list order: positions 0-31 of the list sit in id0, 32-63 in id1
                const uint32_t r0 = half_rank(hi, lo32(fm0), hi32(fm0));
                const uint32_t r1 = (hi ? f0_b : f0_a) + half_rank(hi, lo32(fm1), hi32(fm1));
                wave_lds_fence();
                if (fresh0) ids_h[r0] = id0;
                if (fresh1) ids_h[r1] = id1;
                wave_lds_fence();
                const uint32_t nf_v = hi ? nf_b : nf_a;
                const uint32_t nf_max = nf_a > nf_b ? nf_a : nf_b;
                int irc0 = 1, irc1 = 1;
                PP_T(pt2);
                PP_ACC(1, pt1, pt2);  // visited tests, compaction
                // ---- rounds of 16 rows per half: two lanes per row (row_dist<2>), then the accept rule for the round's rows in list order
                for (uint32_t s0 = 0; s0 < nf_max; s0 += 16u) {
                    PP_T(pr0);
                    const uint32_t rk = s0 + (hl >> 1);
                    const uint32_t rid = ids_h[rk < nf_v ? rk : 0u];  // (slots behind the list re-read a row that is being read anyway)
                    float v = row_dist<METRIC, 2>(ix.vec, row_stride, nrm2, tile, rid, hl & 1u, [&]() __attribute__((always_inline)) {
                        if (ins0) irc0 = cell16_insert(table_h, a.tbits, a.restbits, p0);
                        if (ins1) irc1 = cell16_insert(table_h, a.tbits, a.restbits, p1);
                    }, s0 == 0u);
                    // slot r of the round: computed in lane 32 half + 2 r, wanted in lane 32 half + r (one row of 16 lanes per half)
                    v = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((((uint32_t)lane & 32u) + 2u * ((uint32_t)lane & 15u)) << 2), __builtin_bit_cast(int, v)));
                    const uint32_t ck = s0 + hl;
                    const bool cv = hl < 16u && ck < nf_v;
                    const float de = cv ? v : INFINITY;
                    const uint32_t idc = ids_h[cv ? ck : 0u];
                    // (:1028-1037) only a neighbour nearer than the farthest entry can enter
                    const bool pass = de < worst_v;
                    const unsigned long long pm = __ballot(pass);
                    PP_T(pr1);
                    PP_ACC(2, pr0, pr1);  // row loads, table insertions, distance chains
                    if (pm == 0ull) continue;
                    const uint32_t nc_a = (uint32_t)__popc(lo32(pm)), nc_b = (uint32_t)__popc(hi32(pm));
                    const uint32_t nc_max = nc_a > nc_b ? nc_a : nc_b, nc_v = hi ? nc_b : nc_a;
                    const uint32_t prk = half_rank(hi, lo32(pm), hi32(pm));
                    wave_lds_fence();
                    if (pass) cb_h[prk] = hmake(de, idc);
                    wave_lds_fence();
                    const hent_t ce = hl < nc_v ? cb_h[hl & 15u] : hmake(INFINITY, 0u);
                    const float xd = hkey(ce);
                    const uint32_t xi = hid(ce);
                    {   // The next candidate is known HERE, before the array is rebuilt: a passing neighbour nearer than the nearest
                        // unexpanded entry (the one whose id row was requested at the top) is accepted -- the first lane among equal
                        // nearest ones has no earlier candidate in front of it -- and is the next pop; its id row is requested now
                        // and arrives while the accept rule runs (an iteration later the request would be a full round trip).
                        float mn = xd;  // prefix minimum along the row of 16 candidate lanes: lane 15 ends with the minimum
                        mn = fminf(mn, dpp_row_shr_inf<1>(mn));
                        mn = fminf(mn, dpp_row_shr_inf<2>(mn));
                        mn = fminf(mn, dpp_row_shr_inf<4>(mn));
                        mn = fminf(mn, dpp_row_shr_inf<8>(mn));
                        const float m_a = readlane_f(mn, 15), m_b = readlane_f(mn, 47);
                        const float m_v = hi ? m_b : m_a;
                        const bool nearer = m_v < spec_key;
                        if (__ballot(nearer) != 0ull) {
                            const unsigned long long who = __ballot(hl < nc_v && xd == m_v);
                            const uint32_t wa = lo32(who), wb = hi32(who);
                            const uint32_t id_a = readlane_u(xi, wa != 0u ? (int)__builtin_ctz(wa) : 0);
                            const uint32_t id_b = readlane_u(xi, wb != 0u ? 32 + (int)__builtin_ctz(wb) : 32);
                            if (nearer) {
                                spec_for = hi ? id_b : id_a;
                                spec_key = m_v;
                                const uint32_t* srow = ix.nbr0 + (size_t)spec_for * deg;
                                spec0 = hl < deg ? srow[hl] : EMPTY_SLOT;
                                spec1 = hl + 32u < deg ? srow[hl + 32u] : EMPTY_SLOT;
                            }
                        }
                    }
                    // cr = entries of R not farther than xd (< ef: xd is nearer than the farthest)
                    uint32_t cr = 0u;
                    if (nc_max <= 4u) {
                        // a few candidates (the usual case): each against the entries in registers, the votes counted per half
                        const float* cbf = reinterpret_cast<const float*>(cb_h);
                        for (uint32_t t = 0; t < nc_max; ++t) {
                            const float xt = cbf[2u * t + 1u];  // (behind a half's last candidate: a stale slot, the count goes nowhere)
                            uint32_t ca = 0u, cbn = 0u;
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const unsigned long long mm = __ballot(rd[s] <= xt);
                                ca += (uint32_t)__popc(lo32(mm));
                                cbn += (uint32_t)__popc(hi32(mm));
                            }
                            if (hl == t) cr = hi ? cbn : ca;
                        }
                    } else {  // binary search in the LDS mirror, every candidate lane its own
                        for (uint32_t step = ef_pow2 >> 1; step != 0u; step >>= 1) {
                            const uint32_t idx = cr + step - 1u;
                            float kv = INFINITY;
                            if (idx < ef) kv = rm_f[2u * idx + 1u];
                            if (kv <= xd) cr += step;
                        }
                    }
                    uint32_t cb = 0u;
                    bool eq_unused = false;
                    pair_count_before<1>(xd, nc_max, cb, eq_unused);
                    const bool acc = hl < nc_v && cr + cb < ef;
                    const unsigned long long am = __ballot(acc);
                    uint32_t aft = 0u;
                    pair_count_after<1>(acc ? xd : INFINITY, xd, nc_max, aft);
                    const uint32_t fpos = cr + cb + aft;  // where an accepted candidate ends up (>= ef: pushed out again by later ones)
                    const uint32_t na_a = (uint32_t)__popc(lo32(am)), na_b = (uint32_t)__popc(hi32(am));
                    const uint32_t na_max = na_a > na_b ? na_a : na_b, na_v = hi ? na_b : na_a;
                    const uint32_t ark = half_rank(hi, lo32(am), hi32(am));
                    if (acc) ab_h[ark] = cr;
                    wave_lds_fence();
                    // an entry of R moves up by the accepted candidates that are nearer than it: those whose cr is <= its index
                    uint32_t shift[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t t = 0; t < na_max; ++t) {
                        const uint32_t crt = t < na_v ? ab_h[t] : 0xFFFFFFFFu;
#pragma unroll
                        for (int s = 0; s < 4; ++s) shift[s] += crt <= (uint32_t)s * 32u + hl ? 1u : 0u;
                    }
                    // (position ef of the merged order -- the nearest entry that leaves -- is written too: the cut is looked at below)
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const uint32_t j = (uint32_t)s * 32u + hl + shift[s];
                        if (shift[s] != 0u && j <= ef) rm_h[j] = hmake(rd[s], ri[s]);
                    }
                    if (acc && fpos <= ef) rm_h[fpos] = hmake(xd, xi);
                    wave_lds_fence();
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const uint32_t j = (uint32_t)s * 32u + hl;
                        if (j < ef) {
                            const hent_t e = rm_h[j];
                            rd[s] = hkey(e);
                            ri[s] = hid(e);
                        }
                    }
                    worst_v = rm_f[2u * (ef - 1u) + 1u];
                    {   // equal entries on both sides of the cut at ef: which of them the reference evicts (:1051-1053) is its heap's
                        // internal order (hnsw_search_kernel keeps ghosts and a tainted distance for this; here the query is handed on)
                        // (a half that accepted nothing sees the pair it saw at its last rebuild again; a sentinel that left: +inf on both sides)
                        const unsigned long long ct = __ballot(rm_f[2u * ef + 1u] == worst_v && worst_v < INFINITY);
                        if (ct != 0ull) {
                            if (lo32(ct) != 0u) { tie_a = 1u; if (a.pair_ties_to_retry != 0u) done |= 1u; }
                            if (hi32(ct) != 0u) { tie_b = 1u; if (a.pair_ties_to_retry != 0u) done |= 2u; }
                        }
                    }
                    len_a = len_a + na_a > ef ? ef : len_a + na_a;
                    len_b = len_b + na_b > ef ? ef : len_b + na_b;
                    PP_T(pr2);
                    PP_ACC(3, pr1, pr2);  // accept rule, the array rebuilt
                }
                {
                    const unsigned long long ovf = __ballot(irc0 == 2 || irc1 == 2);  // no cell within the displacement budget (rare)
                    if (ovf != 0ull) {
                        if (have_bm) {
                            if (lo32(ovf) != 0u) to_bitmap(0u);
                            if (hi32(ovf) != 0u) to_bitmap(1u);
                            if (irc0 == 2) (void)visit_bitmap(bm_h, id0);
                            if (irc1 == 2) (void)visit_bitmap(bm_h, id1);
                        } else {
                            if (lo32(ovf) != 0u) { st_a = 1u; done |= 1u; }
                            if (hi32(ovf) != 0u) { st_b = 1u; done |= 2u; }
                        }
                    }
                }
            }

            // ---- into_sorted_vec + truncate to min(knbn, ef, len) (:1544-1547, :1567-1578); flagged and failed queries to their lists
            {
                const uint32_t len_v = hi ? len_b : len_a, nvis_v = hi ? nvis_b : nvis_a, nexp_v = hi ? nexp_b : nexp_a;
                {   // (C) of hnsw_search_kernel: two equal distances inside the first k answers or across their end -- into_sorted_vec
                    // (:1544) decides ids there, not values
                    const uint32_t kk = k < len_v ? k : len_v;
                    bool bad = false;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const uint32_t j = (uint32_t)s * 32u + hl;
                        if (j < kk && j + 1u < len_v) bad = bad || rd[s] == rm_f[2u * (j + 1u) + 1u];
                    }
                    const unsigned long long cm = __ballot(bad);
                    if (lo32(cm) != 0u) tie_a = 1u;
                    if (hi32(cm) != 0u) tie_b = 1u;
                }
                const uint32_t st_v = hi ? st_b : st_a, tie_v = hi ? tie_b : tie_a;
                const bool retry = st_v == 1u || (tie_v != 0u && a.pair_ties_to_retry != 0u);
                uint32_t nids = my_ids;
#pragma unroll
                for (int off = 1; off < 32; off <<= 1) nids += __shfl_xor(nids, off);
                if (mine) {
                    uint32_t out_status = 0u;
                    if (retry) {
                        out_status = 1u;
                        if (hl == 0u) a.retry_out[atomicAdd(counters, 1u)] = q;
                    } else {
                        if (tie_v != 0u) {
                            out_status = 2u;
                            if (a.tie_list != nullptr && hl == 0u) a.tie_list[atomicAdd(counters + 3, 1u)] = q;
                        }
                        const uint32_t cnt = len_v < k ? len_v : k;
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const uint32_t j = (uint32_t)s * 32u + hl;
                            if (j < k) {
                                const size_t o = (size_t)q * k + j;
                                if (j < cnt) {
                                    const uint32_t flat = ri[s] & ~EXPANDED;
                                    uint32_t l = 0;
                                    while (l + 1 < NB_LAYER_MAX && flat >= ka->ix.layer_offset[l + 1]) ++l;
                                    put_answer(a.out_ids, a.id_stride, a.out_dists, a.dist_stride, o, ix.origin_id[flat], rd[s]);
                                    if (a.out_layer) a.out_layer[o] = (uint8_t)l;
                                    if (a.out_rank) a.out_rank[o] = (int32_t)(flat - ka->ix.layer_offset[l]);
                                } else {
                                    put_answer(a.out_ids, a.id_stride, a.out_dists, a.dist_stride, o, 0ull, 0.f);
                                    if (a.out_layer) a.out_layer[o] = 0;
                                    if (a.out_rank) a.out_rank[o] = 0;
                                }
                            }
                        }
                        if (hl == 0u) put_count(a.out_counts, a.count_stride, q, cnt);
                    }
                    if (hl == 0u) {
                        // feedback for the host's table sizing (ctrl[2], ctrl[3]), as finish_query
                        if (st_v == 1u || ((bm >> half) & 1u) != 0u) atomicAdd(counters + 1, 1u);
                        if (nvis_v > (table_limit >> 1)) atomicAdd(counters + 2, 1u);
                        uint32_t* st = a.stats + (size_t)q * 8;
                        // n_dist: the descent's, the entry point once more (:952) and the nvis_v - 1 fresh ids
                        st[0] = pd.n_dist + nvis_v; st[1] = pd.n_expand + nexp_v; st[2] = pd.n_dist - 1u + nids; st[3] = out_status;
                        st[4] = t_start; st[5] = (uint32_t)wall_clock64(); st[6] = ((bm >> half) & 1u) != 0u ? 1u : 0u;
                        st[7] = (tie_v != 0u ? 1u : 0u) | ((pd.n_expand & 0xFFu) << 8) | (pd.n_dist << 16);
#if HNSW_PAIR_PHASES
                        st[4] = pph[0]; st[5] = pph[1]; st[6] = pph[2]; st[7] = pph[3];
#endif
                    }
                }
            }
            __syncthreads();  // the tiles and tables are rewritten by the next pair
        }
    }
}
