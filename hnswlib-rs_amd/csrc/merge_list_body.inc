// merge_list_body.inc -- the body of merge_list, the accept rule for a whole neighbour list at once (DESIGN.md section 4.4;
// src/hnsw.rs:1028-1053).  Textually included, so that the code under test is the code that runs: by hnsw_search_kernel's
// `merge_list` lambda (search_kernels.inc) and by the lane lab's wrapper (lane_lab_kernel, tests/test_gpu_lane_lab.py).
// Expects in scope: S, rd[S], ri[S], ef, de, idc (the candidates: lanes of de / idc, ascending lane = list order), cand (the
// candidate lanes, consumed), merge_buf (LDS, 64 S + 64 entries), lane.  Leaves `acc` (the lanes accepted) and `tie_here` (one of
// them met an equal distance); returns true from the enclosing function when nothing is accepted, false -- nothing changed -- when
// equal entries end up on both sides of the cut at ef; falls through with rd / ri rebuilt otherwise.
            // slot s of lane l holds entry 64 s + l; the set is full: exactly the entries below ef exist
            unsigned long long slotmask[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const uint32_t lo = (uint32_t)s * 64u;
                slotmask[s] = ef >= lo + 64u ? ~0ull : (ef > lo ? (1ull << (ef - lo)) - 1ull : 0ull);
            }
            unsigned long long acc = 0ull;
            bool tie_here = false;
            uint32_t shift[S];   // lanes of R: accepted neighbours that go in front of this entry
#pragma unroll
            for (int s = 0; s < S; ++s) shift[s] = 0u;
            uint32_t pos_c = 0;  // lanes of accepted neighbours: final position
            while (cand != 0ull) {
                const int j = ctz64(cand);
                cand &= cand - 1ull;
                const float xd = readlane_f(de, j);
                uint32_t cr = 0;
                unsigned long long eqm = 0ull;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    cr += popc64(__ballot(rd[s] <= xd) & slotmask[s]);
                    eqm |= __ballot(rd[s] == xd) & slotmask[s];
                }
                const uint32_t cb = popc64(__ballot(de <= xd) & acc);
                if (cr + cb >= ef) continue;  // not nearer than the farthest entry at its turn
                if ((eqm | (__ballot(de == xd) & acc)) != 0ull) tie_here = true;
#pragma unroll
                for (int s = 0; s < S; ++s) shift[s] += xd < rd[s] ? 1u : 0u;
                pos_c += xd < de ? 1u : 0u;  // counts only in lanes accepted earlier; a later acceptance overwrites it
                if (lane == j) pos_c = cr + cb;
                acc |= 1ull << j;
            }
            if (acc == 0ull) return true;
            const bool is_acc = ((acc >> lane) & 1ull) != 0ull;
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < S; ++s)
                if ((slotmask[s] >> lane) & 1ull) merge_buf[(uint32_t)s * 64u + (uint32_t)lane + shift[s]] = hmake(rd[s], ri[s]);
            if (is_acc) merge_buf[pos_c] = hmake(de, idc);
            wave_lds_fence();
            hent_t mine[S];
#pragma unroll
            for (int s = 0; s < S; ++s) mine[s] = merge_buf[(uint32_t)s * 64u + (uint32_t)lane];
            const hent_t out0 = merge_buf[ef];  // the nearest entry that leaves (ef + popc(acc) entries were written)
            wave_lds_fence();
            float w_new = 0.f;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (((ef - 1u) >> 6) == (uint32_t)s) w_new = readlane_f(hkey(mine[s]), (int)((ef - 1u) & 63u));
            if (hkey(out0) == w_new) return false;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if ((slotmask[s] >> lane) & 1ull) { rd[s] = hkey(mine[s]); ri[s] = hid(mine[s]); }
