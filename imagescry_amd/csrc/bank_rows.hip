// Access to the stored rows of a packed bank BY ROW INDEX (include/imagescry_hip.h: isc_bank_gather, isc_cosine_scores):
// the stored bytes of a list of rows, and the exact float64 scores of queries against a list of rows.  Both address the
// packed image through the bank's permutation and, when given, its fill bitmap; neither needs a workspace, a status word
// or the host, so both are capturable.
#include "bank_layout.h"
#include "isc_common.h"
#include "search_common.h"

namespace {

// isc_bank_gather: one wave per listed row, a lane per 16-byte chunk of the row (8 lanes per 128-byte K-step segment, as
// k_bank_repack reads them).  E is an unsigned integer of the element's size: the bytes move untouched.  A chunk that lies
// inside the row goes out as one 16-byte store when the output rows are 16-byte aligned (`vec_ok`); the ragged last chunk,
// and every chunk of an unaligned output, element by element.  A dead row is written as zeros.
template <typename E>
__global__ __launch_bounds__(256) void k_bank_gather(const unsigned char* __restrict__ packed, int d, int ks, IscPerm pm,
                                                     const int64_t* __restrict__ rows, int64_t m,
                                                     const uint32_t* __restrict__ fill_mask, E* __restrict__ out,
                                                     int64_t ldo, int vec_ok) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const int lane = threadIdx.x & 63;
    const int64_t p = isc_live_pos(rows[i], pm, fill_mask);
    constexpr int PER = 16 / (int)sizeof(E);
    E* dst = out + i * ldo;
    const int chunks = (d + PER - 1) / PER;  // <= 8 * ks
    for (int c = lane; c < chunks; c += 64) {
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (p >= 0) raw = *reinterpret_cast<const uint4*>(packed + isc_packed_offset(p, c >> 3, ks) + (c & 7) * 16);
        const int e0 = c * PER;
        if (vec_ok && e0 + PER <= d) {
            *reinterpret_cast<uint4*>(dst + e0) = raw;
        } else {
            const E* v = reinterpret_cast<const E*>(&raw);
#pragma unroll
            for (int j = 0; j < PER; ++j)
                if (e0 + j < d) dst[e0 + j] = v[j];
        }
    }
}

// isc_cosine_scores: the exact score of every (query, listed row) pair, without a search around it: the staged form of
// exact_dots.h, hence the bits isc_cosine_topk_exhaustive returns for the pair.
//
// A workgroup owns SC_ROWS = 64 listed rows (a wave 8 of them: lane l holds row l >> 3, 16-byte chunk l & 7 of every K
// step) and a group of 8 queries, staged 8 K steps at a time (isc_staged_scores): the LDS image does not depend on D, so
// neither does the query-group size, and LDS never limits the four 512-thread workgroups a CU can hold.  The grid is
// (row blocks) x (query groups), the query group running fastest: the workgroups that share a row block are neighbours
// and re-read it from the cache.
constexpr int SC_ROWS = ISC_ST_THREADS / 64 * 8;

template <typename T>
__global__ __launch_bounds__(ISC_ST_THREADS) void k_row_scores(const unsigned char* __restrict__ bank, int ks, IscPerm pm,
                                                               const void* __restrict__ queries, int q_f32, int64_t ldq,
                                                               int d, int nq, int qgroups, const int64_t* __restrict__ rows,
                                                               int64_t m, const uint32_t* __restrict__ fill_mask,
                                                               float* __restrict__ scores, int64_t lds) {
    __shared__ __attribute__((aligned(16))) double qd[ISC_ST_GQ * isc_st_elems<T>()];
    __shared__ double denom_sh[ISC_ST_GQ];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane >> 3, ch = lane & 7;
    const int q0 = (int)(blockIdx.x % (unsigned)qgroups) * ISC_ST_GQ;
    const int gn = min(ISC_ST_GQ, nq - q0);
    const int64_t j = (int64_t)(blockIdx.x / (unsigned)qgroups) * SC_ROWS + wave * 8 + sub;
    const int64_t p = j < m ? isc_live_pos(rows[j], pm, fill_mask) : -1;
    const unsigned char* src = bank + (p >= 0 ? isc_packed_offset(p, 0, ks) : 0) + ch * 16;

    // lane `ch` of the row's 8 lanes gets, and writes, query `ch`
    const float mine = isc_staged_scores<T, false>(src, p >= 0, ks, queries, q_f32, ldq, d, q0, gn, qd, denom_sh);
    if (j < m && ch < gn) scores[(int64_t)(q0 + ch) * lds + j] = p >= 0 ? mine : -INFINITY;
}

bool rows_dtype_ok(int dtype) { return dtype == ISC_F16 || dtype == ISC_F32; }

}  // namespace

extern "C" int isc_bank_gather(const void* packed, int dtype, int D, int64_t capacity, const int64_t* rows, int64_t m,
                               const uint32_t* fill_mask, void* out, int64_t ldo, void* stream) {
    ISC_REQUIRE(rows_dtype_ok(dtype) && D > 0 && m >= 0 && ldo >= D);
    ISC_REQUIRE(capacity > 0 && capacity <= 0x7ffffffe);
    if (m == 0) return ISC_OK;
    ISC_REQUIRE(packed && rows && out);
    const int esz = dtype == ISC_F16 ? 2 : 4;
    if (!isc_aligned(packed, 16) || !isc_aligned(rows, 8) || !isc_aligned(fill_mask, 4) || !isc_aligned(out, esz))
        return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(m, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    const int vec_ok = isc_aligned(out, 16) && (ldo * esz) % 16 == 0 ? 1 : 0;
    const unsigned char* in = static_cast<const unsigned char*>(packed);
    const IscPerm pm = isc_make_perm(capacity);
    if (dtype == ISC_F16)
        hipLaunchKernelGGL(k_bank_gather<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream), in, D,
                           isc_ksteps(D, 2), pm, rows, m, fill_mask, static_cast<uint16_t*>(out), ldo, vec_ok);
    else
        hipLaunchKernelGGL(k_bank_gather<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream), in, D,
                           isc_ksteps(D, 4), pm, rows, m, fill_mask, static_cast<uint32_t*>(out), ldo, vec_ok);
    return isc_launch_status();
}

extern "C" int isc_cosine_scores(const void* bank, int dtype, int64_t capacity, int D, const void* queries, int q_dtype,
                                 int Q, int64_t ldq, const int64_t* rows, int64_t M, const uint32_t* fill_mask,
                                 float* scores, int64_t lds, void* stream) {
    ISC_REQUIRE(rows_dtype_ok(dtype) && rows_dtype_ok(q_dtype) && D > 0 && Q >= 0 && M >= 0 && ldq >= D && lds >= M);
    ISC_REQUIRE(capacity > 0 && capacity <= 0x7ffffffe);
    if (D > ISC_SEARCH_MAX_D || Q > ISC_SEARCH_MAX_Q) return ISC_ERR_UNSUPPORTED;
    if (Q == 0 || M == 0) return ISC_OK;
    ISC_REQUIRE(bank && queries && rows && scores);
    if (!isc_aligned(bank, 16) || !isc_aligned(queries, q_dtype == ISC_F16 ? 2 : 4) || !isc_aligned(rows, 8) ||
        !isc_aligned(fill_mask, 4) || !isc_aligned(scores, 4))
        return ISC_ERR_ALIGNMENT;
    const int qgroups = isc_ceil_div(Q, ISC_ST_GQ);
    const int64_t blocks = isc_ceil_div<int64_t>(M, SC_ROWS) * qgroups;
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    const unsigned char* in = static_cast<const unsigned char*>(bank);
    const IscPerm pm = isc_make_perm(capacity);
    const int qf = q_dtype == ISC_F32 ? 1 : 0;
    if (dtype == ISC_F16)
        hipLaunchKernelGGL(k_row_scores<_Float16>, dim3((unsigned)blocks), dim3(ISC_ST_THREADS), 0, isc_stream(stream), in,
                           isc_ksteps(D, 2), pm, queries, qf, ldq, D, Q, qgroups, rows, M, fill_mask, scores, lds);
    else
        hipLaunchKernelGGL(k_row_scores<float>, dim3((unsigned)blocks), dim3(ISC_ST_THREADS), 0, isc_stream(stream), in,
                           isc_ksteps(D, 4), pm, queries, qf, ldq, D, Q, qgroups, rows, M, fill_mask, scores, lds);
    return isc_launch_status();
}
