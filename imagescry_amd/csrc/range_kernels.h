// The stages the exact range search (search_range.hip) and the large-k top-k search (search_large.hip) share: the packed
// query image of a pass, the filter threshold below a float32 score, the matrix-core filter against per-query thresholds,
// the float64 re-score of its candidates and the segmented sort of (score, original row) keys.  One copy of each, so the
// error bound eps, the candidate format and the bits of every score are the same in both searches.  search_range.hip's
// header comment describes the pipeline and proves that the filter loses no row.
#pragma once

#include <math.h>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "bank_layout.h"
#include "isc_common.h"
#include "search_common.h"

namespace {

constexpr int RQT = 64;                          // queries per filter workgroup (one query tile)

enum : int32_t { MODE_FILTER = 0, MODE_SCAN = 1, MODE_NONE = 2, MODE_ALL = 3 };

// rocPRIM's default segmented sort for this architecture (it has no tuned gfx950 entry: 6 radix bits, 128 x 17 items,
// warp sorts of 32 x 4 and 32 x 4) with the partitioning of segments by size switched off.  With partitioning the sort
// reads the segment counts back to the host (hipMemcpyWithStream) once a call has 3000 segments or more, i.e. a range
// search of >= 3000 queries would synchronise the host and could not be captured into a hipGraph.
using SortConfig = rocprim::segmented_radix_sort_config<6, rocprim::kernel_config<128, 17>,
                                                        rocprim::WarpSortConfig<32, 4, 256, 0xffffffffu, 32, 4, 256>, true>;

hipError_t sort_keys_desc(void* tmp, size_t& bytes, const unsigned long long* in, unsigned long long* out, int64_t cap,
                          int q, const int64_t* begin, const int64_t* end, hipStream_t stream) {
    return rocprim::segmented_radix_sort_keys_desc<SortConfig>(tmp, bytes, in, out, (unsigned)cap, (unsigned)q, begin, end,
                                                               0, 64, stream);
}

size_t sort_temp_bytes(int q, int64_t cap) {
    size_t bytes = 0;
    if (sort_keys_desc(nullptr, bytes, nullptr, nullptr, cap, q, nullptr, nullptr, (hipStream_t)0) != hipSuccess) return 0;
    return bytes;
}

// Wave-aggregated append: `cnt` entries of this lane go to slots [base + prefix, ...) of the candidate buffer; one atomic
// per wave.  Returns this lane's first slot (every lane of the wave must call it).
__device__ __forceinline__ unsigned long long wave_reserve(int cnt, unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    const int total = __shfl(incl, 63, 64);
    unsigned long long base = 0;
    if (lane == 0 && total > 0) base = atomicAdd(count, (unsigned long long)total);
    const unsigned lo = __shfl((unsigned)base, 0, 64), hi = __shfl((unsigned)(base >> 32), 0, 64);
    return (((unsigned long long)hi << 32) | lo) + (unsigned long long)(incl - cnt);
}

__device__ __forceinline__ const unsigned char* qrow_of(const unsigned char* qpacked, int w, int ks) {
    return qpacked + ((size_t)(w / RQT) * ks * RQT + (w % RQT)) * ISC_KSTEP_BYTES;
}

// The filter threshold that keeps every row whose score float32(E / denom) is >= t, for a trusted query (search_range.hip's
// header): E > prevfloat(t) * denom and |A - E| <= eps, less a 1e-12 relative margin for the float64 product, rounded DOWN
// to float32; the filter keeps A > tau.
__device__ __forceinline__ float range_tau(float t, double denom, double eps) {
    const double ed = (double)nextafterf(t, -INFINITY) * denom;
    const double t2 = ed - eps - fabs(ed) * 1e-12;
    if (t2 > 3.0e38) return INFINITY;    // above every filter score and every reachable dot (|E| <= 1e37): nothing can pass
    if (t2 < -3.0e38) return -INFINITY;  // every row (the filter scores of a trusted query are finite)
    float tf = (float)t2;
    if ((double)tf >= t2) tf = nextafterf(tf, -INFINITY);
    return tf;
}

// queries [qb][ldq] of TQ -> packed [qtile][K step][64 rows][128 B] of T (rows >= qb and columns >= d are zero); float32 ->
// fp16 rounds to nearest even, as k_prep of cosine_topk.hip does.  Thread 0 also opens the pass.
template <typename T, typename TQ>
__global__ __launch_bounds__(256) void k_range_pack(const TQ* __restrict__ queries, int64_t ldq, int qb, int d, int ks,
                                                    int qpad, unsigned char* __restrict__ packed,
                                                    int32_t* __restrict__ fb_count,
                                                    unsigned long long* __restrict__ pass_begin,
                                                    const unsigned long long* __restrict__ count) {
    constexpr int PER = 16 / (int)sizeof(T);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        *fb_count = 0;
        *pass_begin = *count;
    }
    if (i >= qpad * ks * 8) return;
    const int c = i & 7;
    const int row = (i >> 3) % RQT;
    const int blk = (i >> 3) / RQT;  // qtile * ks + kstep
    const int kstep = blk % ks;
    const int qrow = (blk / ks) * RQT + row;
    T v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int e = (kstep * 8 + c) * PER + j;
        v[j] = (qrow < qb && e < d) ? (T)queries[(int64_t)qrow * ldq + e] : (T)0.f;
    }
    *reinterpret_cast<uint4*>(packed + (size_t)i * 16) = *reinterpret_cast<const uint4*>(v);
}

// One workgroup = one 256-row bank tile x one 64-query tile; wave w owns rows 64 w .. 64 w + 63 of the tile (4 x 4 blocks of
// 16 x 16 scores).  Fragments come straight from global memory (the bank tile's K step is 32 KiB of contiguous HBM, a
// wave's share 8 KiB), one K step ahead of the matrix cores; consecutive workgroups are the query tiles of one bank tile,
// so a bank tile read by several of them is served from L2.  Scores above tau are appended (wave_reserve); with a row filter
// (RowMask, search_common.h) only those of allowed rows.
template <typename T, typename... RowMask>
__global__ __launch_bounds__(256) void k_range_filter(const unsigned char* __restrict__ bank, int64_t n, int ks, int nqt,
                                                      const unsigned char* __restrict__ qpacked,
                                                      const float* __restrict__ tau, int q0,
                                                      unsigned long long* __restrict__ count, int64_t capacity,
                                                      int32_t* __restrict__ cand_q, int32_t* __restrict__ cand_r,
                                                      float* __restrict__ cand_a, RowMask... row_mask) {
    // (the tile's statements are shared with k_large_bound as an included fragment, not as a function: behind a call --
    // even a forced-inline one -- the compiler scheduled this kernel differently and the range search lost 6 - 9 %)
#include "range_tile_body.h"
    float tq[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) tq[nb] = tau[qt * RQT + nb * 16 + r16];
    int cnt = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += (row0 + m * 16 + j < n && acc[m][nb][j] > tq[nb]) ? 1 : 0;
    if (__ballot(cnt > 0) == 0ull) return;
    unsigned long long pos = wave_reserve(cnt, count);
    if (cnt == 0) return;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = row0 + m * 16 + j;
                if (row < n && acc[m][nb][j] > tq[nb]) {
                    if (pos < (unsigned long long)capacity) {
                        cand_q[pos] = q0 + qt * RQT + nb * 16 + r16;
                        cand_r[pos] = (int32_t)row;
                        cand_a[pos] = acc[m][nb][j];
                    }
                    ++pos;
                }
            }
}

// The epilogue of the large-k search's bound pass (k_large_bound): the scores of a tile folded into a bucket table.
struct RangeBound {
    int gran, buckets, qpad;   // rows per unit, buckets (a power of two), query stride of the table
    unsigned* table;           // [buckets][qpad] bucket maxima, isc_score_bits; 0 = empty
};

// gran = 16: the best score of each 16-row block (the lane's four rows, then the four lane groups) goes to the table from
// lane group 0; gran = 4: the best of the lane's four rows; gran = 1: every score.  Rows >= n, disallowed rows (-inf) and
// NaN leave the table alone.  Entry [bucket][query]: the 16 lanes of a group hold 16 consecutive queries, so their atomics
// fall into one 64-byte line.
__device__ __forceinline__ void range_bound_fold(const f32x4 (&acc)[4][4], int64_t row0, int64_t n, int qt, int r16, int grp,
                                                 const RangeBound& bd) {
    const unsigned bmask = (unsigned)bd.buckets - 1u;
    auto put = [&](int64_t unit, int nb, float v) {
        if (v > -INFINITY)  // (false for NaN)
            atomicMax(bd.table + (size_t)((unsigned)unit & bmask) * bd.qpad + qt * RQT + nb * 16 + r16, isc_score_bits(v));
    };
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int64_t r = row0 + m * 16;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = r + j < n ? acc[m][nb][j] : -INFINITY;
            if (bd.gran == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) put(r + j, nb, v[j]);
            } else {
                float best = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                if (bd.gran == 4) {
                    put(r >> 2, nb, best);
                } else {
                    best = fmaxf(best, __shfl_xor(best, 16, 64));
                    best = fmaxf(best, __shfl_xor(best, 32, 64));
                    if (grp == 0) put(r >> 4, nb, best);
                }
            }
        }
    }
}

// Every candidate of the pass re-scored in float64, one wave per candidate: the packed-row form of exact_dots.h with the
// top-k's lane mapping, so E is bit for bit the top-k's and a range result and a top-k result agree on every score.
template <typename T>
__global__ __launch_bounds__(256) void k_range_rescore(const unsigned char* __restrict__ bank, int ks,
                                                       const unsigned char* __restrict__ qpacked, int q0,
                                                       const unsigned long long* __restrict__ pass_begin,
                                                       const unsigned long long* __restrict__ count, int64_t capacity,
                                                       int32_t* __restrict__ cand_q, const int32_t* __restrict__ cand_r,
                                                       float* __restrict__ cand_a, const double* __restrict__ denom,
                                                       const double* __restrict__ eps, const int32_t* __restrict__ mode,
                                                       const float* __restrict__ min_score, int32_t* __restrict__ qcount,
                                                       int32_t* __restrict__ status) {
    const unsigned long long end = *count;
    if (end > (unsigned long long)capacity) return;  // the call has overflowed: nothing of it is usable
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 3, ch = lane & 7;
    const unsigned long long nw = (unsigned long long)gridDim.x * 4;
    for (unsigned long long c = *pass_begin + blockIdx.x * 4 + (threadIdx.x >> 6); c < end; c += nw) {
        const int qg = cand_q[c];
        const int w = qg - q0;
        const int64_t row = cand_r[c];
        const unsigned char* qrow = qrow_of(qpacked, w, ks);
        double acc = 0.0;
        for (int s0 = 0; s0 < ks; s0 += 8) {
            const int s = s0 + sub;
            if (s < ks)
                acc = isc_packed_dot<T>(bank + isc_packed_offset(row, s, ks) + ch * 16,
                                        qrow + (size_t)s * RQT * ISC_KSTEP_BYTES + ch * 16, acc);
        }
        const double e = isc_wave_sum(acc);
        if (lane == 0) {
            // how far the filter scores are from the exact dots, in units of the bound (status[2], diagnostics)
            if (mode[qg] == MODE_FILTER && eps[w] > 0.0) {
                const float ratio = (float)(fabs((double)cand_a[c] - e) / eps[w]);
                if (ratio == ratio) atomicMax(reinterpret_cast<unsigned*>(&status[2]), __float_as_uint(ratio));
            }
            const float sc = (float)(e / denom[w]);
            if (sc >= min_score[qg]) {
                cand_a[c] = sc;
                atomicAdd(&qcount[qg], 1);
            } else {
                cand_q[c] = -1;
            }
        }
    }
}

int grid_for(int64_t items, int per_block, int cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

}  // namespace
