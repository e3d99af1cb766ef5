// The scores of one workgroup of a filter -- a FRAGMENT of kernel body, included inside k_range_filter (range_kernels.h)
// and k_large_bound (search_large.hip) so that both compile the same statements; not a header of its own.
// In scope at the point of inclusion: T, RowMask... row_mask, bank, ks, nqt, qpacked, q0.  Defines tile, qt, lane, wave,
// r16, grp, row0 and
//   acc[m][nb][j] = score of bank row row0 + 16 m + j with query 16 nb + r16 of the query tile qt,
// -inf for a row the row filter (RowMask, search_common.h) disallows or, with IscGroups, a row of the query's own group.
// Rows >= n are NOT marked: the epilogue skips them.
    const int64_t tile = blockIdx.x / nqt;
    const int qt = blockIdx.x % nqt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, grp = lane >> 4;
    // MFMA operand fragments: lane (r16, grp) feeds row r16 of a 16-row block, chunk grp (first half of the K step) and
    // chunk 4 + grp (second half); the same K permutation on both operands leaves the dots unchanged
    const unsigned char* a_base = bank + ((tile * ks * ISC_TILE_ROWS) + wave * 64 + r16) * ISC_KSTEP_BYTES + grp * 16;
    const unsigned char* b_base = qpacked + ((size_t)qt * ks * RQT + r16) * ISC_KSTEP_BYTES + grp * 16;
    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[m][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](int s, u32x4 (&av)[4][2], u32x4 (&bv)[4][2]) {
        const unsigned char* ap = a_base + (size_t)s * ISC_TILE_KSTEP_BYTES;
        const unsigned char* bp = b_base + (size_t)s * RQT * ISC_KSTEP_BYTES;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            av[m][0] = *reinterpret_cast<const u32x4*>(ap + m * 16 * ISC_KSTEP_BYTES);
            av[m][1] = *reinterpret_cast<const u32x4*>(ap + m * 16 * ISC_KSTEP_BYTES + 64);
            bv[m][0] = *reinterpret_cast<const u32x4*>(bp + m * 16 * ISC_KSTEP_BYTES);
            bv[m][1] = *reinterpret_cast<const u32x4*>(bp + m * 16 * ISC_KSTEP_BYTES + 64);
        }
    };
    auto mma = [&](const u32x4 (&av)[4][2], const u32x4 (&bv)[4][2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) Mma<T>::step(av[m][h], bv[nb][h], acc[m][nb]);
    };
    u32x4 a0[4][2], b0[4][2], a1[4][2], b1[4][2];
    load(0, a0, b0);
    for (int s = 0; s < ks; s += 2) {
        if (s + 1 < ks) load(s + 1, a1, b1);
        mma(a0, b0);
        if (s + 1 >= ks) break;
        if (s + 2 < ks) load(s + 2, a0, b0);
        mma(a1, b1);
    }

    // acc[m][nb][j] = score of bank row 16 m + 4 grp + j (of this wave's 64) with query 16 nb + r16 of the tile
    const int64_t row0 = tile * ISC_TILE_ROWS + wave * 64 + grp * 4;
    // row filter: disallowed rows score -inf, which no tau lets through ("A > tau" is false even for tau = -inf).  This
    // wave's 64 rows are two words; row 16 m + 4 grp + j is bit 16 (m & 1) + 4 grp + j of word m / 2.
    if constexpr (sizeof...(RowMask) > 0) {
        const uint32_t* mb = isc_row_mask_ptr(row_mask...);  // (NULL only in a grouped call without a row filter)
        if (!isc_grouped<RowMask...>() || mb != nullptr) {
            const uint32_t* mw = mb + tile * (ISC_TILE_ROWS / 32) + wave * 2;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint32_t nib = mw[m >> 1] >> ((m & 1) * 16 + grp * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!((nib >> j) & 1u)) {
#pragma unroll
                        for (int nb = 0; nb < 4; ++nb) acc[m][nb][j] = -INFINITY;
                    }
            }
        }
    }
    // group exclusion: a row of the query's own group scores -inf for that query.  Row 16 m + 4 grp + j's code is element j
    // of one 16-byte load per m; query column 16 nb + r16's code is read once.
    if constexpr (isc_grouped<RowMask...>()) {
        const IscGroups& gr = (row_mask, ...);
        int qc[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) qc[nb] = isc_query_code(gr, q0 + qt * RQT + nb * 16 + r16);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const i32x4 rc = *reinterpret_cast<const i32x4*>(gr.row_group + row0 + m * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    if (rc[j] == qc[nb]) acc[m][nb][j] = -INFINITY;
        }
    }
