// The row body of the pack kernels (isc_bank_pack, isc_bank_append, isc_bank_replace) and of isc_bank_project's packed
// output: whatever stores a row into a packed bank stores it through this one function, so the stored bytes agree.
#pragma once

#include "bank_layout.h"
#include "isc_common.h"

// One wave per row: optional L2 normalisation (float32, the F.normalize formula), cast, scatter the row's
// 16-byte chunks to their K-step blocks at the row's PERMUTED position; columns past D are zero.  The norm of the
// row AS STORED (after the cast) feeds `norm_bound` (atomic max): the search's rounding-error guard needs an upper
// bound of the stored rows' norms.  The body of k_bank_pack and k_bank_append: this wave stores source row `p` at packed
// position `row`.
template <typename TIN, typename TOUT>
__device__ __forceinline__ void isc_pack_row(const TIN* __restrict__ p, int d, int64_t row, int normalize, float eps,
                                             unsigned char* __restrict__ packed, int ks,
                                             unsigned* __restrict__ norm_bound, int lane) {
    float denom = 1.f;
    if (normalize) {  // (element order of the sum: lane, lane + 64, ... -- kept as it was: the stored values depend on it)
        float acc = 0.f;
        for (int i = lane; i < d; i += 64) {
            const float v = (float)p[i];
            acc += v * v;
        }
        denom = fmaxf(sqrtf(isc_wave_sum(acc)), eps);
    }
    constexpr int PER_CHUNK = 16 / (int)sizeof(TOUT);
    constexpr int IN_VECS = PER_CHUNK * (int)sizeof(TIN) / 16;  // 16-byte input loads per output chunk: 1, 2, or 0 (f16 -> f32)
    const int chunks = ks * 8;
    // rows whose chunks can be fetched with 16-byte loads (a wave instruction then reads 1 KiB of the row instead of 64
    // scattered 2- or 4-byte elements)
    const bool vec_ok = IN_VECS > 0 && ((reinterpret_cast<uintptr_t>(p) & 15) == 0);
    float stored_sq = 0.f, stored_max = 0.f;
    for (int c = lane; c < chunks; c += 64) {
        TOUT v[PER_CHUNK];
        float f[PER_CHUNK];
        const int e0 = c * PER_CHUNK;
        if (vec_ok && e0 + PER_CHUNK <= d) {
            TIN raw[PER_CHUNK];
#pragma unroll
            for (int u = 0; u < (IN_VECS > 0 ? IN_VECS : 1); ++u)
                reinterpret_cast<uint4*>(raw)[u] = reinterpret_cast<const uint4*>(p + e0)[u];
#pragma unroll
            for (int j = 0; j < PER_CHUNK; ++j) f[j] = (float)raw[j];
        } else {
#pragma unroll
            for (int j = 0; j < PER_CHUNK; ++j) f[j] = e0 + j < d ? (float)p[e0 + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < PER_CHUNK; ++j) {
            if (normalize && e0 + j < d) f[j] = __fdiv_rn(f[j], denom);
            v[j] = (TOUT)f[j];
            const float s = (float)v[j];
            stored_sq = fmaf(s, s, stored_sq);
            stored_max = fmaxf(stored_max, fabsf(s));  // (a NaN is dropped here; the sum keeps it)
        }
        unsigned char* dst = packed + isc_packed_offset(row, c >> 3, ks) + (c & 7) * 16;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(v);
    }
    if (norm_bound) {
        stored_sq = isc_wave_sum(stored_sq);
        // float32 summation of d squares: relative error <= d * 2^-24 -- cover it (and the sqrt) with a factor
        float nb = sqrtf(stored_sq) * (1.f + 1e-3f);
        // Below 2^-64 the sum is no bound any more: the squares of a float32 row of tiny scale lose bits to underflow, or
        // vanish altogether (entries under 1e-23), and a bound of 0 for a bank of positive norms would switch the search's
        // guard off.  ||row|| <= max|s| sqrt(Dpad) needs no square; the factor 2 covers the rounding of the square root
        // and of the product, which in the subnormal range is absolute (2^-150 <= half of any non-zero product).  A row
        // of zeros still publishes 0.  (wave-uniform: every lane holds the same sum)
        if (stored_sq < 0x1p-64f) nb = 2.f * (isc_wave_max(stored_max) * sqrtf((float)(chunks * PER_CHUNK)));
        // non-negative floats order as uints; a row holding NaN makes the bound +inf: the search then trusts no filter
        // result on this bank and answers through its exhaustive pass.  The atomic goes out only when this row RAISES the
        // bound as this wave sees it (a plain read first): one atomic per row on the one word was the whole kernel --
        // 88 atomics per microsecond on one address, 11.4 ms per 2^20 rows whatever their size.
        if (lane == 0) {
            const unsigned mine = nb == nb ? __float_as_uint(nb) : 0x7f800000u;
            if (mine > __hip_atomic_load(norm_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(norm_bound, mine);
        }
    }
}
