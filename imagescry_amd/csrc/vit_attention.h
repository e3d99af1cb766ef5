// What the three attention kernels share (head size 64): k_attention_f16 / k_attention_f16_p (vit.hip, keys and values of
// a head whole in LDS) and k_attention_f16_stream (vit_attention_stream.hip, keys and values streamed in chunks).  They
// differ in how they stage and schedule; the arithmetic on a block of 16 queries, and the lane mapping it rests on, is here.
//
// qkv [B * T, 3 * D] fp16 with D = heads * 64: query / key / value of head h at columns h*64, D + h*64, 2D + h*64; out
// [B * T, D] fp16; both row-major or packed (packed_matrix.h).  A wave works on 16 queries, lane = 16 g + qi holds query
// qi; staged key and value rows are row-major in LDS, ATT_STRIDE halves apart.
#pragma once

#include "isc_common.h"
#include "packed_matrix.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef short tr4 __attribute__((__vector_size__(4 * sizeof(short))));  // what ds_read_b64_tr_b16 returns: four 16-bit values
typedef short tr8 __attribute__((__vector_size__(8 * sizeof(short))));

constexpr int ATT_STRIDE = 72;  // halves per staged key / value row (64 + 8 pad)

// 8-half chunk c of part 0/1/2 = q/k/v of head h in row `row` (= image * T + token; 64-bit throughout).  In the packed
// layout a head's 64 values are exactly one 128-byte K-step segment of the row.
template <bool PACKED>
__device__ __forceinline__ const _Float16* att_qkv_at(const _Float16* qkv, long long row, int D, int h, int part, int c) {
    if (PACKED) return qkv + pk_offset(row, part * D + h * 64, 3 * D) + c * 8;
    return qkv + (size_t)row * ((size_t)3 * D) + (size_t)(part * D + h * 64 + c * 8);
}
// the 64 outputs of head h in row `row`
template <bool PACKED>
__device__ __forceinline__ _Float16* att_out_row(_Float16* out, long long row, int D, int h) {
    return PACKED ? out + pk_offset(row, h * 64, D) : out + (size_t)row * (size_t)D + h * 64;
}

// The parts of a qkv row.  QPART / KPART of the kernels name the part the "query" operand and the staged "key" rows are
// read from: (0, 1) is attention; (0, 0) and (1, 1) are SELF attention, softmax(z z^T / 8) v with z the query or the key
// columns (isc_attention_f16_self*), which never reads the other of the two.
constexpr int ATT_PART_QUERY = 0;
constexpr int ATT_PART_KEY = 1;
constexpr int ATT_PART_VALUE = 2;
static_assert(ATT_PART_QUERY == ISC_ATT_PART_QUERY && ATT_PART_KEY == ISC_ATT_PART_KEY, "the header's part numbers");

// A lane's two query fragments, the "B" operand of the score MFMAs: chunks g and 4 + g of its query's row ...
template <bool PACKED, int QPART = ATT_PART_QUERY>
__device__ __forceinline__ void att_load_query(half8 (&q)[2], const _Float16* qkv, long long row, int D, int h, int g) {
    static_assert(QPART == ATT_PART_QUERY || QPART == ATT_PART_KEY, "the query operand is the q or the k columns");
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) q[kk] = *reinterpret_cast<const half8*>(att_qkv_at<PACKED>(qkv, row, D, h, QPART, kk * 4 + g));
}
// ... times 1/sqrt(64): a power of two, so the scaling is exact
__device__ __forceinline__ void att_scale_query(half8 (&qf)[2], const half8 (&q)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[kk][j] = q[kk][j] * (_Float16)0.125f;
}

// S^T[key][query] = K . Q^T / 8 of the 16-key block kb: two MFMAs.  The lane gets the scores of its query against keys
// 16 kb + 4 g + r, r = 0 .. 3.
__device__ __forceinline__ f32x4 att_score_block(const _Float16* Ks, int kb, const half8 (&qf)[2], int qi, int g) {
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const half8 kf = *reinterpret_cast<const half8*>(&Ks[(kb * 16 + qi) * ATT_STRIDE + (kk * 4 + g) * 8]);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[kk], a, 0, 0, 0);
    }
    return a;
}

// O^T[d][query] += V^T . P^T over the 32 keys of step ks; p_lo / p_hi = the lane's probabilities of key blocks 2 ks and
// 2 ks + 1.  The contraction runs over keys, and the order in which a lane's 8 k-slots map to keys is free as long as
// both operands agree: slot (g, j) <-> key 32 ks + 4 g + j (j < 4) or 32 ks + 16 + 4 g + (j - 4).  With that mapping
// the P^T operand is exactly what the lane holds after the softmax, rounded to fp16 -- the probabilities never leave
// registers -- and the values stay row-major in LDS: the V^T fragment of value column 16 db + qi comes out of two
// transposed reads (ds_read_b64_tr_b16).  One such read hands every lane of a 16-lane group ITS column of a 4-row block;
// lane 4 q + p of the group supplies the address of row q, columns 4 p .. 4 p + 3 (EXEC must be all ones: branches
// around a call are wave-uniform).
__device__ __forceinline__ void att_pv_step(const _Float16* Vs, int ks, const f32x4& p_lo, const f32x4& p_hi, int qi, int g,
                                            f32x4 (&o)[4]) {
    half8 pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pf[r] = (_Float16)p_lo[r];
        pf[4 + r] = (_Float16)p_hi[r];
    }
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        const _Float16* vb = &Vs[(ks * 32 + g * 4 + (qi >> 2)) * ATT_STRIDE + db * 16 + (qi & 3) * 4];
        const tr4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4*)vb);
        const tr4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4*)(vb + 16 * ATT_STRIDE));
        const half8 vf = __builtin_bit_cast(half8, tr8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[db], 0, 0, 0);
    }
}

// the lane's 16 outputs (columns 16 db + 4 g + r of its query's row), normalised by inv = 1 / (sum of probabilities)
__device__ __forceinline__ void att_store_row(_Float16* orow, const f32x4 (&o)[4], float inv, int g) {
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        half4 hv;
#pragma unroll
        for (int r = 0; r < 4; ++r) hv[r] = (_Float16)(o[db][r] * inv);
        *reinterpret_cast<half4*>(orow + db * 16 + g * 4) = hv;
    }
}
