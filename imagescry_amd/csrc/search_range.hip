// Exact cosine range search over a packed embedding bank (include/imagescry_hip.h: isc_cosine_range).
//
// Every row whose score reaches the query's threshold t, ordered by (score desc, original row asc).  The top-k search's
// redo pass (cosine_topk.hip) with the threshold given by the caller instead of derived from a k-th
// score, and a result list of no fixed size.  Pipeline per call (one stream, no host synchronisation):
//
//   k_range_init       zero the per-query counters, the candidate counter and the status words
//   per pass of <= 1024 queries:
//     k_range_pack     queries -> packed [query tile of 64][K step][64 rows][128 B], rounded to the bank dtype
//     k_range_qinfo    one wave per query: float64 norm, the filter threshold tau, the per-query mode
//     k_range_filter   fp32 matrix-core scores A of 256 bank rows x 64 queries per workgroup (Mma<T>::step of
//                      search_common.h: the instructions of the top-k filter, so the same eps bounds A); every A > tau is
//                      appended as a candidate (query, packed row, A)
//     k_range_scan     float64 sweep of the whole bank for the queries the filter cannot serve (normally none)
//     k_range_rescore  every candidate of the pass re-scored in float64 (exact_dots.h: the packed-row form); kept iff
//                      float32(E / denom) >= t
//   k_range_offsets    per-query counts -> exclusive scan -> offsets[Q + 1]; needed = candidates + rows of all-row queries
//   k_range_scatter    kept candidates -> (score, original row) keys in their query's segment
//   segmented radix sort of the keys, descending (rocPRIM)
//   k_range_fill_all   segments of zero queries with t <= 0 (every row ties at 0: already in order)
//   k_range_emit       keys -> scores, indices + index_base
//
// Why the filter loses no row.  float32 rounding is monotone, so float32(E / denom) >= t implies E / denom > prevfloat(t),
// i.e. E > prevfloat(t) * denom; the filter score satisfies |A - E| <= eps = Dpad * 2^-23 * ||q|| * max||b|| (the top-k
// guard's bound), so A > prevfloat(t) * denom - eps.  tau is that value less a 1e-12 relative margin for the float64
// product, rounded DOWN to float32, and the filter keeps A > tau.  The bound holds while every partial sum stays in
// float32's normal range: queries with ||q|| < 1e-30 or ||q|| * max||b|| > 1e37 (a bank with a NaN / inf row has an
// infinite bound) take the float64 scan instead.  A zero query scores 0 against every row of a finite bank and a query
// with a NaN / inf element NaN: neither needs a scan.
//
// A masked call (isc_cosine_range_masked) hands the row filter to the filter and the scan, which skip the rows it disallows.
// Its zero queries with t <= 0 take the scan as well: it collects every ALLOWED row (all score 0), and the sort puts them
// in row order, so their segments need no row-order fill.
//
// k_range_pack, k_range_filter, k_range_rescore, the threshold (range_tau) and the sort live in range_kernels.h: the large-k
// top-k search (search_large.hip) runs them behind a threshold it derives itself.
//
// If the candidates outgrow `capacity` the counter keeps counting, every later stage sees empty segments, and the caller
// learns the exact size to re-issue with from `needed`.
#include "range_kernels.h"

namespace {

constexpr int RPASS = ISC_SEARCH_PASS_QUERIES;   // queries per pass: the workspace holds one pass's packed queries
constexpr int64_t R_MAX_CAPACITY = 0x7fffffff;   // the segmented sort counts items in int

struct RangeWs {
    unsigned char* qpacked;           // [qpad][ks] x 128 B: one pass's queries, packed
    float* tau;                       // [qpad] filter threshold of each pass query (raw dot units); +inf = never
    double* denom;                    // [RPASS] max(||q||, 1e-12)
    double* eps;                      // [RPASS] filter error bound
    int32_t* fb_count;                // [1] scan list of the pass
    int32_t* fb_list;                 // [RPASS]
    int32_t* all_count;               // [1] queries whose result is every row
    int32_t* all_list;                // [Q]
    int32_t* mode;                    // [Q]
    int32_t* qcount;                  // [Q] kept rows per query
    int32_t* fill;                    // [Q] scatter cursors
    int64_t* seg_end;                 // [Q] end of the segment the sort sees
    unsigned long long* count;        // [1] candidates appended (counts past capacity)
    unsigned long long* all_rows;     // [1] rows of all-row queries
    unsigned long long* pass_begin;   // [passes] value of *count when each pass started
    int32_t* cand_q;                  // [cap] query (global index; -1 = dropped by the re-score)
    int32_t* cand_r;                  // [cap] packed row
    float* cand_a;                    // [cap] filter score, then the exact float32 score
    unsigned long long* keys_in;      // [cap]
    unsigned long long* keys_out;     // [cap]
    void* sort_tmp;
    size_t sort_bytes;
    size_t bytes;
};

RangeWs carve(int ks, int q, int64_t cap, void* base) {
    RangeWs w{};
    unsigned char* b = static_cast<unsigned char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) -> void* {
        void* p = b ? b + off : nullptr;
        off = isc_align_up(off + bytes, 256);
        return p;
    };
    const int qb = q < RPASS ? q : RPASS;
    const int qpad = isc_ceil_div(qb, RQT) * RQT;
    const int passes = isc_ceil_div(q, RPASS);
    w.qpacked = static_cast<unsigned char*>(take((size_t)qpad * ks * ISC_KSTEP_BYTES));
    w.tau = static_cast<float*>(take(sizeof(float) * qpad));
    w.denom = static_cast<double*>(take(sizeof(double) * RPASS));
    w.eps = static_cast<double*>(take(sizeof(double) * RPASS));
    w.fb_count = static_cast<int32_t*>(take(sizeof(int32_t)));
    w.fb_list = static_cast<int32_t*>(take(sizeof(int32_t) * RPASS));
    w.all_count = static_cast<int32_t*>(take(sizeof(int32_t)));
    w.all_list = static_cast<int32_t*>(take(sizeof(int32_t) * q));
    w.mode = static_cast<int32_t*>(take(sizeof(int32_t) * q));
    w.qcount = static_cast<int32_t*>(take(sizeof(int32_t) * q));
    w.fill = static_cast<int32_t*>(take(sizeof(int32_t) * q));
    w.seg_end = static_cast<int64_t*>(take(sizeof(int64_t) * q));
    w.count = static_cast<unsigned long long*>(take(8));
    w.all_rows = static_cast<unsigned long long*>(take(8));
    w.pass_begin = static_cast<unsigned long long*>(take(8 * (size_t)passes));
    w.cand_q = static_cast<int32_t*>(take(sizeof(int32_t) * cap));
    w.cand_r = static_cast<int32_t*>(take(sizeof(int32_t) * cap));
    w.cand_a = static_cast<float*>(take(sizeof(float) * cap));
    w.keys_in = static_cast<unsigned long long*>(take(8 * (size_t)cap));
    w.keys_out = static_cast<unsigned long long*>(take(8 * (size_t)cap));
    w.sort_bytes = sort_temp_bytes(q, cap);
    w.sort_tmp = take(w.sort_bytes);
    w.bytes = off;
    return w;
}

__global__ __launch_bounds__(256) void k_range_init(int q, int32_t* __restrict__ mode, int32_t* __restrict__ qcount,
                                                    int32_t* __restrict__ fill, unsigned long long* __restrict__ count,
                                                    unsigned long long* __restrict__ all_rows,
                                                    int32_t* __restrict__ all_count, int32_t* __restrict__ status) {
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    for (int i = i0; i < q; i += gridDim.x * 256) {
        mode[i] = MODE_NONE;
        qcount[i] = 0;
        fill[i] = 0;
    }
    if (i0 == 0) {
        *count = 0;
        *all_rows = 0;
        *all_count = 0;
    }
    if (i0 < 4) status[i0] = 0;
}

// One wave per query slot of the pass: norm, mode, threshold (see the file header).  MASK: a masked call, whose all-row
// queries are scanned (see the file header).
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_range_qinfo(const unsigned char* __restrict__ qpacked, int ks, int qb, int qpad,
                                                     int q0, int64_t n, const float* __restrict__ min_score,
                                                     const float* __restrict__ norm_bound, float* __restrict__ tau,
                                                     double* __restrict__ denom_out, double* __restrict__ eps_out,
                                                     int32_t* __restrict__ mode, int32_t* __restrict__ qcount,
                                                     int32_t* __restrict__ fb_count, int32_t* __restrict__ fb_list,
                                                     int32_t* __restrict__ all_count, int32_t* __restrict__ all_list,
                                                     unsigned long long* __restrict__ all_rows,
                                                     int32_t* __restrict__ status) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= qpad) return;
    if (w >= qb) {
        if (lane == 0) tau[w] = INFINITY;  // padding queries never pass the filter
        return;
    }
    const double qnorm = sqrt(wave_query_norm<T>(qrow_of(qpacked, w, ks), ks, RQT));
    if (lane != 0) return;
    const int qg = q0 + w;
    const float t = min_score[qg];
    const double denom = fmax(qnorm, 1e-12);
    const double bmax = norm_bound ? (double)*norm_bound : 1.001;
    const double eps = (double)(ks * (ISC_KSTEP_BYTES / (int)sizeof(T))) * (1.0 / 8388608.0) * qnorm * bmax;
    int m;
    float tf = INFINITY;
    if (t != t) {
        m = MODE_NONE;  // no score is >= NaN
    } else if ((qnorm == 0.0 || !(qnorm <= 1.7e308)) && bmax <= 1.7e308) {
        // every score is 0 (zero query) or NaN (non-finite query)
        m = qnorm == 0.0 && 0.f >= t ? (MASK ? MODE_SCAN : MODE_ALL) : MODE_NONE;
    } else if (!(qnorm >= 1e-30 && qnorm * bmax <= 1e37)) {
        m = MODE_SCAN;  // outside the range where eps bounds the filter (a NaN / inf bound included)
    } else {
        m = MODE_FILTER;
        tf = range_tau(t, denom, eps);
    }
    tau[w] = tf;
    denom_out[w] = denom;
    eps_out[w] = eps;
    mode[qg] = m;
    if (m == MODE_SCAN) {
        fb_list[atomicAdd(fb_count, 1)] = w;
        atomicAdd(&status[1], 1);
    } else if (m == MODE_ALL) {
        all_list[atomicAdd(all_count, 1)] = qg;
        qcount[qg] = (int32_t)n;
        atomicAdd(all_rows, (unsigned long long)n);
    }
}

// The float64 scan of the queries the filter cannot serve: one thread per bank row, the whole bank per listed query.  A row
// is appended when its score is >= prevfloat(t) (one float32 step of margin for the summation order): the re-score decides.
// Rows a row filter disallows (RowMask) are skipped, and with IscGroups the rows of the listed query's own group.
template <typename T, typename... RowMask>
__global__ __launch_bounds__(256) void k_range_scan(const unsigned char* __restrict__ bank, int64_t n, int ks,
                                                    const unsigned char* __restrict__ qpacked,
                                                    const int32_t* __restrict__ fb_count,
                                                    const int32_t* __restrict__ fb_list, const double* __restrict__ denom,
                                                    const float* __restrict__ min_score, int q0,
                                                    unsigned long long* __restrict__ count, int64_t capacity,
                                                    int32_t* __restrict__ cand_q, int32_t* __restrict__ cand_r,
                                                    float* __restrict__ cand_a, RowMask... row_mask) {
    const int nfb = *fb_count;
    for (int li = 0; li < nfb; ++li) {
        const int w = fb_list[li];
        const unsigned char* qrow = qrow_of(qpacked, w, ks);
        const float t_dn = nextafterf(min_score[q0 + w], -INFINITY);
        const double dn = denom[w];
        [[maybe_unused]] int qc = -1;
        if constexpr (isc_grouped<RowMask...>()) qc = isc_query_code((row_mask, ...), q0 + w);
        for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
            const int64_t row = base + threadIdx.x;
            double e = 0.0;
            bool keep = false;
            if (row < n && isc_row_allowed_for(row, qc, row_mask...)) {
                for (int s = 0; s < ks; ++s) {
#pragma unroll
                    for (int ch = 0; ch < 8; ++ch)
                        e = isc_packed_dot<T>(bank + isc_packed_offset(row, s, ks) + ch * 16,
                                              qrow + (size_t)s * RQT * ISC_KSTEP_BYTES + ch * 16, e);
                }
                keep = (float)(e / dn) >= t_dn;  // false for NaN
            }
            const unsigned long long pos = wave_reserve(keep ? 1 : 0, count);
            if (keep && pos < (unsigned long long)capacity) {
                cand_q[pos] = q0 + w;
                cand_r[pos] = (int32_t)row;
                cand_a[pos] = (float)e;
            }
        }
    }
}

// One workgroup: offsets = exclusive scan of the per-query counts (all zero when the call overflowed, so every later stage
// sees empty segments), the segment ends the sort sees, needed and status[0].
__global__ __launch_bounds__(1024) void k_range_offsets(int q, const int32_t* __restrict__ qcount,
                                                        const int32_t* __restrict__ mode,
                                                        const unsigned long long* __restrict__ count,
                                                        const unsigned long long* __restrict__ all_rows,
                                                        int64_t capacity, int64_t* __restrict__ offsets,
                                                        int64_t* __restrict__ seg_end, int64_t* __restrict__ needed,
                                                        int32_t* __restrict__ status) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const unsigned long long cand = *count;
    const unsigned long long need = cand + *all_rows;
    const bool ok = need <= (unsigned long long)capacity;
    long long carry = 0;
    for (int base = 0; base < q; base += 1024) {
        const int i = base + tid;
        const long long v = (ok && i < q) ? qcount[i] : 0;
        part[tid] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const long long t = tid >= off ? part[tid - off] : 0;
            __syncthreads();
            part[tid] += t;
            __syncthreads();
        }
        if (i < q) {
            const long long begin = carry + part[tid] - v;
            offsets[i] = begin;
            seg_end[i] = mode[i] == MODE_ALL ? begin : begin + v;  // all-row segments are written in order, not sorted
        }
        carry += part[1023];
        __syncthreads();
    }
    if (tid == 0) {
        offsets[q] = carry;
        *needed = (int64_t)need;
        status[0] = cand > 0x7fffffffull ? 0x7fffffff : (int32_t)cand;
    }
}

__global__ __launch_bounds__(256) void k_range_scatter(const int32_t* __restrict__ cand_q,
                                                       const int32_t* __restrict__ cand_r,
                                                       const float* __restrict__ cand_a,
                                                       const unsigned long long* __restrict__ count, int64_t capacity,
                                                       const int64_t* __restrict__ needed,
                                                       const int64_t* __restrict__ offsets, int32_t* __restrict__ fill,
                                                       IscPerm pm, unsigned long long* __restrict__ keys) {
    if (*needed > capacity) return;
    const unsigned long long end = *count;
    for (unsigned long long c = blockIdx.x * 256ull + threadIdx.x; c < end; c += gridDim.x * 256ull) {
        const int qg = cand_q[c];
        if (qg < 0) continue;
        const int64_t pos = offsets[qg] + atomicAdd(&fill[qg], 1);
        keys[pos] = isc_make_key(cand_a[c], (int)isc_perm_orig(pm, cand_r[c]));
    }
}

__global__ __launch_bounds__(256) void k_range_fill_all(int64_t n, const int32_t* __restrict__ all_count,
                                                        const int32_t* __restrict__ all_list,
                                                        const int64_t* __restrict__ needed, int64_t capacity,
                                                        const int64_t* __restrict__ offsets,
                                                        unsigned long long* __restrict__ keys) {
    if (*needed > capacity) return;
    const int na = *all_count;
    for (int li = 0; li < na; ++li) {
        const int64_t o = offsets[all_list[li]];
        for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll)
            keys[o + i] = isc_make_key(0.f, (int)i);
    }
}

__global__ __launch_bounds__(256) void k_range_emit(int q, const int64_t* __restrict__ offsets,
                                                    const unsigned long long* __restrict__ keys, int64_t index_base,
                                                    float* __restrict__ scores, int64_t* __restrict__ indices) {
    const int64_t total = offsets[q];  // 0 when the call overflowed
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        const unsigned long long k = keys[i];
        scores[i] = isc_key_score(k);
        indices[i] = (int64_t)isc_key_row(k) + index_base;
    }
}

template <typename T, typename TQ, typename... RowMask>
int run(const void* bank, int64_t n, int d, const void* queries, int q, int64_t ldq, const float* min_score,
        int64_t index_base, const float* norm_bound, int64_t capacity, int64_t* offsets, float* scores,
        int64_t* indices, int64_t* needed, int32_t* status, void* workspace, hipStream_t stream, RowMask... rm) {
    const int ks = isc_ksteps(d, (int)sizeof(T));
    const RangeWs w = carve(ks, q, capacity, workspace);
    const IscPerm pm = isc_make_perm(n);
    const unsigned char* bk = static_cast<const unsigned char*>(bank);
    const int64_t ntiles = (n + ISC_TILE_ROWS - 1) / ISC_TILE_ROWS;
    const int cus = isc_device_cus();
    k_range_init<<<grid_for(q, 256, 1024), 256, 0, stream>>>(q, w.mode, w.qcount, w.fill, w.count, w.all_rows,
                                                            w.all_count, status);
    int pass = 0;
    for (int p0 = 0; p0 < q; p0 += RPASS, ++pass) {
        const int qb = q - p0 < RPASS ? q - p0 : RPASS;
        const int nqt = isc_ceil_div(qb, RQT);
        const int qpad = nqt * RQT;
        k_range_pack<T, TQ><<<isc_ceil_div(qpad * ks * 8, 256), 256, 0, stream>>>(
            static_cast<const TQ*>(queries) + (int64_t)p0 * ldq, ldq, qb, d, ks, qpad, w.qpacked, w.fb_count,
            w.pass_begin + pass, w.count);
        k_range_qinfo<T, (sizeof...(RowMask) > 0)><<<qpad / 4, 256, 0, stream>>>(w.qpacked, ks, qb, qpad, p0, n, min_score, norm_bound, w.tau,
                                                       w.denom, w.eps, w.mode, w.qcount, w.fb_count, w.fb_list,
                                                       w.all_count, w.all_list, w.all_rows, status);
        k_range_filter<T, RowMask...><<<(unsigned)(ntiles * nqt), 256, 0, stream>>>(
            bk, n, ks, nqt, w.qpacked, w.tau, p0, w.count, capacity, w.cand_q, w.cand_r, w.cand_a, rm...);
        k_range_scan<T, RowMask...><<<grid_for(n, 256, 4 * cus), 256, 0, stream>>>(
            bk, n, ks, w.qpacked, w.fb_count, w.fb_list, w.denom, min_score, p0, w.count, capacity, w.cand_q, w.cand_r,
            w.cand_a, rm...);
        k_range_rescore<T><<<grid_for(capacity, 4, 8 * cus), 256, 0, stream>>>(
            bk, ks, w.qpacked, p0, w.pass_begin + pass, w.count, capacity, w.cand_q, w.cand_r, w.cand_a, w.denom, w.eps,
            w.mode, min_score, w.qcount, status);
    }
    k_range_offsets<<<1, 1024, 0, stream>>>(q, w.qcount, w.mode, w.count, w.all_rows, capacity, offsets, w.seg_end,
                                            needed, status);
    k_range_scatter<<<grid_for(capacity, 256, 8 * cus), 256, 0, stream>>>(w.cand_q, w.cand_r, w.cand_a, w.count,
                                                                          capacity, needed, offsets, w.fill, pm,
                                                                          w.keys_in);
    size_t sort_bytes = w.sort_bytes;
    if (sort_keys_desc(w.sort_tmp, sort_bytes, w.keys_in, w.keys_out, capacity, q, offsets, w.seg_end, stream) !=
        hipSuccess)
        return ISC_ERR_LAUNCH;
    k_range_fill_all<<<grid_for(n, 256, 4 * cus), 256, 0, stream>>>(n, w.all_count, w.all_list, needed, capacity,
                                                                    offsets, w.keys_out);
    k_range_emit<<<grid_for(capacity, 256, 8 * cus), 256, 0, stream>>>(q, offsets, w.keys_out, index_base, scores,
                                                                       indices);
    return isc_launch_status();
}

int check_args(int dtype, int64_t n, int d, int q, int64_t capacity) {
    if (dtype != ISC_F16 && dtype != ISC_F32) return ISC_ERR_INVALID_ARG;
    if (n <= 0 || d <= 0 || q <= 0 || capacity <= 0) return ISC_ERR_INVALID_ARG;
    if (n > 0x7ffffffe) return ISC_ERR_UNSUPPORTED;  // row ids are int32 inside a shard
    if (d > ISC_SEARCH_MAX_D || q > ISC_SEARCH_MAX_Q || capacity > R_MAX_CAPACITY) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

}  // namespace

extern "C" int isc_cosine_range_workspace_bytes(int dtype, int64_t N, int D, int Q, int64_t capacity, size_t* bytes) {
    ISC_REQUIRE(bytes);
    const int st = check_args(dtype, N, D, Q, capacity);
    if (st != ISC_OK) return st;
    *bytes = carve(isc_ksteps(D, dtype == ISC_F16 ? 2 : 4), Q, capacity, nullptr).bytes;
    return ISC_OK;
}

namespace {

int range(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q, int64_t ldq,
          const float* min_score, int64_t index_base, const float* norm_bound, int64_t capacity, int64_t* offsets,
          float* scores, int64_t* indices, int64_t* needed, int32_t* status, void* workspace, size_t workspace_bytes,
          const uint32_t* row_mask, void* stream, const IscGroups* groups = nullptr) {
    ISC_REQUIRE(bank && queries && min_score && offsets && scores && indices && needed && status);
    ISC_REQUIRE(q_dtype == ISC_F16 || q_dtype == ISC_F32);
    const int st = check_args(dtype, N, D, Q, capacity);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(ldq >= D);
    if (!isc_aligned(bank, 16) || !isc_aligned(workspace, 256)) return ISC_ERR_ALIGNMENT;
    size_t need = 0;
    isc_cosine_range_workspace_bytes(dtype, N, D, Q, capacity, &need);
    if (!workspace || workspace_bytes < need) return ISC_ERR_WORKSPACE;
#define ISC_RUN(T_, TQ_)                                                                                              \
    return groups   ? run<T_, TQ_>(bank, N, D, queries, Q, ldq, min_score, index_base, norm_bound, capacity, offsets,   \
                                   scores, indices, needed, status, workspace, isc_stream(stream), *groups)             \
           : row_mask ? run<T_, TQ_>(bank, N, D, queries, Q, ldq, min_score, index_base, norm_bound, capacity, offsets,   \
                                   scores, indices, needed, status, workspace, isc_stream(stream), row_mask)            \
                    : run<T_, TQ_>(bank, N, D, queries, Q, ldq, min_score, index_base, norm_bound, capacity, offsets,   \
                                   scores, indices, needed, status, workspace, isc_stream(stream))
    if (dtype == ISC_F16) {
        if (q_dtype == ISC_F16) ISC_RUN(_Float16, _Float16);
        ISC_RUN(_Float16, float);
    }
    if (q_dtype == ISC_F16) ISC_RUN(float, _Float16);
    ISC_RUN(float, float);
#undef ISC_RUN
}

}  // namespace

extern "C" int isc_cosine_range(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                                int64_t ldq, const float* min_score, int64_t index_base, const float* norm_bound,
                                int64_t capacity, int64_t* offsets, float* scores, int64_t* indices, int64_t* needed,
                                int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    return range(bank, dtype, N, D, queries, q_dtype, Q, ldq, min_score, index_base, norm_bound, capacity, offsets, scores,
                 indices, needed, status, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int isc_cosine_range_masked(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                       int Q, int64_t ldq, const float* min_score, int64_t index_base,
                                       const float* norm_bound, int64_t capacity, int64_t* offsets, float* scores,
                                       int64_t* indices, int64_t* needed, int32_t* status, void* workspace,
                                       size_t workspace_bytes, const uint32_t* row_mask, void* stream) {
    ISC_REQUIRE(row_mask);
    return range(bank, dtype, N, D, queries, q_dtype, Q, ldq, min_score, index_base, norm_bound, capacity, offsets, scores,
                 indices, needed, status, workspace, workspace_bytes, row_mask, stream);
}

extern "C" int isc_cosine_range_grouped(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                        int Q, int64_t ldq, const float* min_score, int64_t index_base,
                                        const float* norm_bound, int64_t capacity, int64_t* offsets, float* scores,
                                        int64_t* indices, int64_t* needed, int32_t* status, void* workspace,
                                        size_t workspace_bytes, const uint32_t* row_mask, const int32_t* row_group,
                                        const int32_t* query_group, void* stream) {
    ISC_REQUIRE(row_group && query_group);
    if (!isc_aligned(row_group, 16) || !isc_aligned(query_group, 4) || !isc_aligned(row_mask, 4))
        return ISC_ERR_ALIGNMENT;
    const IscGroups g{row_mask, row_group, query_group, nullptr, Q};
    return range(bank, dtype, N, D, queries, q_dtype, Q, ldq, min_score, index_base, norm_bound, capacity, offsets, scores,
                 indices, needed, status, workspace, workspace_bytes, row_mask, stream, &g);
}
