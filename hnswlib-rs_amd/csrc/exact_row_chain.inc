// exact_row_chain.inc -- the chain of a slab kernel's loop over its rows, 64 at a time: from the row's address to the sums (exact_tile.hpp).
// Included, not called: as a force-inlined function that takes acc[TQ] by reference the same text costs registers
// (exact_range_slab_kernel: DistL2 40 -> 51 VGPRs, DistCosine 57 -> 63, DistL1 37 -> 48).
// Expects METRIC and ACC, ix, a (SlabArgs at least), T (SlabTile), for this lane the row r, and nchunk, a local copy of
// a.nchunk: with the field itself in the loop's bounds the DistCosine kernels take 21 VGPRs more.  Leaves acc[t], the chain of
// (query t of the tile, row r) summed left to right from the search's own per-element terms, and s2, the row's squared norm
// (DistCosine).
        const float* rowf = ix.vec + (size_t)r * ix.row_stride;
        const float4* row = reinterpret_cast<const float4*>(rowf);
        double s2 = 0.;
        if constexpr (METRIC == DIST_COSINE)
            s2 = a.nrm2 != nullptr ? a.nrm2[r] : *reinterpret_cast<const double*>(rowf + ix.row_stride - 2u);
        ACC acc[TQ];
#pragma unroll
        for (int t = 0; t < TQ; ++t) acc[t] = 0;
        float4 x = row[0];
        for (uint32_t c = 0; c < nchunk; ++c) {
            const float4 xn = row[c + 1u < nchunk ? c + 1u : c];  // (written as a prefetch; as compiled the load sits at the head of the loop and is waited for at once)
            if (T.norm_in_tail && c + 1u == nchunk) { x.z = 0.f; x.w = 0.f; }
#pragma unroll
            for (int t = 0; t < TQ; ++t) {
                const v4f q = T.qc[(size_t)c * TQ + t];
                chain4<METRIC, ACC>(acc[t], make_float4(q.x, q.y, q.z, q.w), x);
            }
            x = xn;
        }
