// Exact cosine top-k for 120 < k <= 4096 (include/imagescry_hip.h: isc_cosine_topk_large, isc_cosine_topk_exhaustive_large).
//
// The selection kernels of cosine_topk.hip and search_exact.hip keep a query's candidates in LDS arrays of k entries, which
// is where ISC_TOPK_MAX_K comes from.  Here nothing of size k lives in LDS.  The fast path is the range search
// (range_kernels.h) behind a PROVEN lower bound of the k-th score, computed on the device; the last resort is a radix select
// over float64 scores whose memory is O(k) per query and whose launch sequence is fixed.  Per pass of queries (one stream, no
// host synchronisation; the passes shrink as k grows so that the workspace stays O(queries per pass x k)):
//
//   k_large_begin     zero the pass's counters, the bucket table and the histograms
//   k_range_pack      queries -> packed query tiles of 64, rounded to the bank dtype
//   k_large_qinfo     one wave per query: float64 norm, eps = Dpad 2^-23 ||q|| max||b||; a query outside the range where
//                     eps bounds the filter (||q|| < 1e-30, ||q|| max||b|| > 1e37, a NaN / inf bound, a zero or non-finite
//                     query) is LISTED for the last resort
//   k_large_bound     the tile of k_range_filter (range_tile_body.h: same loads, same matrix-core instructions, same row
//                     filter and group exclusion), but instead of appending candidates it folds the best filter score A of
//                     every unit of `gran` consecutive packed rows into bucket (unit mod B) of a [B][queries] table: atomic
//                     max on the order-preserving integer image of the float (isc_score_bits).  Buckets are disjoint row sets.
//   k_large_select    one workgroup per query: A_k = the k-th largest bucket maximum (radix select over <= 8192 words in LDS),
//                     then tau (below).  Fewer than k non-empty buckets: tau = -inf, every allowed row is kept.
//   k_range_filter    candidates (query, packed row, A) with A > tau
//   k_range_rescore   every candidate re-scored in float64 (exact_dots.h: the packed-row form), float32(E / denom)
//   k_large_offsets   per-query counts -> segments; a pass whose candidates overflowed lists ALL its queries, a query whose
//                     segment is shorter than k although its tau was finite is listed too
//   k_large_scatter   candidates -> (score, original row) keys in their query's segment
//   8 x (k_lr_sweep, k_lr_pick), k_lr_sweep(collect)      the last resort for the listed queries (exit at once when none)
//   segmented radix sort of the keys, descending (rocPRIM, the range search's configuration)
//   k_large_emit      the first k keys of every segment -> scores, indices + index_base; padding (NaN, INT64_MAX) behind a
//                     segment shorter than k (only a filtered call has one)
//
// Why no row of the answer is lost.  Let the query be trusted, so |A - E| <= eps for every row (search_common.h: Mma).  The k
// buckets with the largest maxima each hold a row with A >= A_k, and buckets are disjoint: k distinct rows have E >= A_k - eps.
// Let x be a float64 lower bound of (A_k - eps) / denom and t = x rounded DOWN to float32.  float32 rounding is monotone, so
// those k rows score float32(E / denom) >= t: the k-th best score is >= t, and every row of the answer scores >= t.  From
// here on it is the range search's argument with threshold t: score >= t implies E > prevfloat(t) * denom, hence
// A > prevfloat(t) * denom - eps, and tau = range_tau(t, denom, eps) is just below that.  In dot units tau sits 2 eps (and one
// float32 step of the score) under A_k.  Ties at the k-th score are all kept, so the sort breaks them by row.
//
// How many candidates.  The bank is stored in pseudo-random row order (bank_layout.h), so the k best rows spread over the
// buckets: about -B ln(1 - k / B) rows reach the k-th bucket maximum, 1.39 k at B = 2 k and 1.15 k at B = 4 k.  The pass's
// candidate buffer holds 2 k + 512 per query.  `gran` is 16 (one MFMA block of rows: the reduction is two lane exchanges)
// while the bank has at least B such units, else 4 (a lane's own four rows), else 1: with one row per bucket A_k is the k-th
// filter score itself, so banks that are small against k are served here as well.
//
// The last resort evaluates every score in float64 with the STAGED form of exact_dots.h, the bits of
// isc_cosine_topk_exhaustive, and finds the k-th largest 64-bit key isc_make_key(score, original row) by radix select: each
// round one sweep of the bank that histograms one 8-bit digit of the keys that match the digits chosen so far, and one
// pick.  Keys of distinct rows are distinct, so exactly k keys are >= the k-th; a ninth sweep collects them.  Thousands of
// rows tied at the k-th score, NaN scores (they rank last) and zero queries are nothing special to it.
#include "range_kernels.h"

namespace {

constexpr int L_PASS_WORK = 1 << 20;   // queries per pass x k stays within this (256 queries at k = 4096)
constexpr int L_MIN_PASS = 64;
constexpr int L_MIN_BUCKETS = 1024;
constexpr int L_MAX_BUCKETS = 8192;    // 32 KiB of LDS in k_large_select
constexpr int LR_BINS = 256;           // 8-bit digits
constexpr int LR_ROUNDS = 8;

int large_pass_queries(int q, int k) {
    int p = ISC_SEARCH_PASS_QUERIES;
    while (p > L_MIN_PASS && (int64_t)p * k > L_PASS_WORK) p >>= 1;
    return q < p ? q : p;
}
int large_buckets(int k) {
    int b = L_MIN_BUCKETS;
    while (b < 4 * k && b < L_MAX_BUCKETS) b <<= 1;
    return b;
}
int large_gran(int64_t n, int buckets) { return n / 16 >= buckets ? 16 : n / 4 >= buckets ? 4 : 1; }
int64_t large_capacity(int qb, int k) { return (int64_t)qb * (2 * k + 512); }

struct LargeWs {
    unsigned char* qpacked;        // [qpad][ks] x 128 B: one pass's queries, packed
    float* tau;                    // [qpad] filter threshold (raw dot units); +inf = never
    double* denom;                 // [P] max(||q||, 1e-12)
    double* eps;                   // [P] filter error bound
    float* neg_inf;                // [P] the re-score keeps every candidate with a score (not NaN)
    int32_t* mode;                 // [P] MODE_FILTER, or MODE_SCAN: listed for the last resort
    int32_t* qcount;               // [P] re-scored candidates per query
    int32_t* fill;                 // [P] scatter cursors
    unsigned long long* count;     // [1] candidates appended (counts past the capacity)
    unsigned long long* zero;      // [1] 0: where the pass's candidates begin
    unsigned* table;               // [B][qpad] bucket maxima, isc_score_bits; 0 = empty
    int32_t* cand_q;               // [cap] query of the pass (-1 = dropped by the re-score)
    int32_t* cand_r;               // [cap] packed row
    float* cand_a;                 // [cap] filter score, then the exact float32 score
    int32_t* lr_count;             // [1] queries listed for the last resort
    int32_t* lr_list;              // [P]
    unsigned long long* lr_prefix; // [P] the digits of the k-th key chosen so far
    int32_t* lr_krem;              // [P] rank of the k-th key among the keys that match the prefix
    int32_t* lr_short;             // [P] -1, or the number of allowed rows when it is below k
    int32_t* lr_fill;              // [P] collect cursors
    int32_t* hist;                 // [P][256]
    int64_t* seg_begin;            // [P] the query's segment of keys
    int64_t* seg_end;              // [P]
    unsigned long long* keys_in;   // [cap + P k]: the filter's segments, then k keys per listed query
    unsigned long long* keys_out;  // [cap + P k]
    void* sort_tmp;
    size_t sort_bytes;
    int pass, qpad, buckets;
    int64_t cap;
    size_t bytes;
};

// fast: the workspace of isc_cosine_topk_large; else of isc_cosine_topk_exhaustive_large (no filter stages, cap = 0)
LargeWs carve(int ks, int q, int k, bool fast, void* base) {
    LargeWs w{};
    unsigned char* b = static_cast<unsigned char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) -> void* {
        void* p = b ? b + off : nullptr;
        off = isc_align_up(off + bytes, 256);
        return p;
    };
    const int P = large_pass_queries(q, k);
    w.pass = P;
    w.qpad = isc_ceil_div(P, RQT) * RQT;
    w.buckets = large_buckets(k);
    w.cap = fast ? large_capacity(P, k) : 0;
    const size_t cap = (size_t)w.cap, keys = cap + (size_t)P * k;
    if (fast) {
        w.qpacked = static_cast<unsigned char*>(take((size_t)w.qpad * ks * ISC_KSTEP_BYTES));
        w.tau = static_cast<float*>(take(sizeof(float) * w.qpad));
        w.denom = static_cast<double*>(take(sizeof(double) * P));
        w.eps = static_cast<double*>(take(sizeof(double) * P));
        w.neg_inf = static_cast<float*>(take(sizeof(float) * P));
        w.table = static_cast<unsigned*>(take(sizeof(unsigned) * (size_t)w.buckets * w.qpad));
        w.cand_q = static_cast<int32_t*>(take(sizeof(int32_t) * cap));
        w.cand_r = static_cast<int32_t*>(take(sizeof(int32_t) * cap));
        w.cand_a = static_cast<float*>(take(sizeof(float) * cap));
    }
    w.mode = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.qcount = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.fill = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.count = static_cast<unsigned long long*>(take(8));
    w.zero = static_cast<unsigned long long*>(take(8));
    w.lr_count = static_cast<int32_t*>(take(sizeof(int32_t)));
    w.lr_list = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.lr_prefix = static_cast<unsigned long long*>(take(8 * (size_t)P));
    w.lr_krem = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.lr_short = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.lr_fill = static_cast<int32_t*>(take(sizeof(int32_t) * P));
    w.hist = static_cast<int32_t*>(take(sizeof(int32_t) * (size_t)P * LR_BINS));
    w.seg_begin = static_cast<int64_t*>(take(sizeof(int64_t) * P));
    w.seg_end = static_cast<int64_t*>(take(sizeof(int64_t) * P));
    w.keys_in = static_cast<unsigned long long*>(take(8 * keys));
    w.keys_out = static_cast<unsigned long long*>(take(8 * keys));
    w.sort_bytes = sort_temp_bytes(P, (int64_t)keys);
    w.sort_tmp = take(w.sort_bytes);
    w.bytes = off;
    return w;
}

// Opens a pass of qb queries.  list_all: every query goes to the last resort (isc_cosine_topk_exhaustive_large; the pass has
// no filter stages, so nothing else opens the list).  first: the call's first pass zeroes the status words.
__global__ __launch_bounds__(256) void k_large_begin(LargeWs w, int qb, int list_all, int first, int32_t* __restrict__ status) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < qb; i += stride) {
        w.mode[i] = list_all ? MODE_SCAN : MODE_FILTER;
        w.qcount[i] = 0;
        w.fill[i] = 0;
        w.lr_fill[i] = 0;
        w.lr_short[i] = -1;
        w.seg_begin[i] = 0;
        w.seg_end[i] = 0;
        if (list_all) w.lr_list[i] = (int32_t)i;
    }
    for (int64_t i = i0; i < (int64_t)qb * LR_BINS; i += stride) w.hist[i] = 0;
    if (w.table)
        for (int64_t i = i0; i < (int64_t)w.buckets * w.qpad; i += stride) w.table[i] = 0u;
    if (i0 == 0) {
        *w.count = 0;
        *w.zero = 0;
        *w.lr_count = list_all ? qb : 0;
    }
    if (status && first && i0 < 4) status[i0] = 0;
}

// One wave per query of the pass: norm, eps, and whether eps bounds the filter (see the file header).
template <typename T>
__global__ __launch_bounds__(256) void k_large_qinfo(LargeWs w, int ks, int qb, const float* __restrict__ norm_bound,
                                                     int32_t* __restrict__ status) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= qb) return;
    const double qnorm = sqrt(wave_query_norm<T>(qrow_of(w.qpacked, q, ks), ks, RQT));
    if ((threadIdx.x & 63) != 0) return;
    const double bmax = norm_bound ? (double)*norm_bound : 1.001;
    w.denom[q] = fmax(qnorm, 1e-12);
    w.eps[q] = (double)(ks * (ISC_KSTEP_BYTES / (int)sizeof(T))) * (1.0 / 8388608.0) * qnorm * bmax;
    w.neg_inf[q] = -INFINITY;
    if (!(qnorm >= 1e-30 && qnorm * bmax <= 1e37)) {  // (false for a NaN norm or bound)
        w.mode[q] = MODE_SCAN;
        w.lr_list[atomicAdd(w.lr_count, 1)] = q;
        atomicAdd(&status[1], 1);
    }
}

// One workgroup = one tile of the range filter (range_tile_body.h: k_range_filter's statements) with the bucket fold as its
// epilogue.  The queries are the pass's own: q0 = 0.
template <typename T, typename... RowMask>
__global__ __launch_bounds__(256) void k_large_bound(const unsigned char* __restrict__ bank, int64_t n, int ks, int nqt,
                                                     const unsigned char* __restrict__ qpacked, RangeBound bd,
                                                     RowMask... row_mask) {
    constexpr int q0 = 0;
#include "range_tile_body.h"
    range_bound_fold(acc, row0, n, qt, r16, grp, bd);
}

// One workgroup per query slot: the k-th largest bucket maximum by radix select in LDS, then tau (see the file header).
__global__ __launch_bounds__(256) void k_large_select(LargeWs w, int qb, int k) {
    __shared__ unsigned vals[L_MAX_BUCKETS];
    __shared__ int hist[LR_BINS];
    __shared__ int nonempty;
    __shared__ unsigned prefix_sh;
    __shared__ int krem_sh;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (q >= qb || w.mode[q] != MODE_FILTER) {  // padding and listed queries never pass the filter
        if (tid == 0) w.tau[q] = INFINITY;
        return;
    }
    if (tid == 0) {
        nonempty = 0;
        prefix_sh = 0u;
        krem_sh = k;
    }
    __syncthreads();
    int mine = 0;
    for (int b = tid; b < w.buckets; b += 256) {
        const unsigned v = w.table[(size_t)b * w.qpad + q];
        vals[b] = v;
        mine += v != 0u ? 1 : 0;
    }
    if (mine) atomicAdd(&nonempty, mine);
    __syncthreads();
    if (nonempty < k) {
        if (tid == 0) w.tau[q] = -INFINITY;  // every allowed row
        return;
    }
    for (int round = 0; round < 4; ++round) {
        const int shift = 24 - 8 * round;
        hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = prefix_sh;
        for (int b = tid; b < w.buckets; b += 256) {
            const unsigned v = vals[b];
            if (v != 0u && (round == 0 || (v >> (shift + 8)) == (prefix >> (shift + 8))))
                atomicAdd(&hist[(v >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int above = 0, d = 255;
            while (d > 0 && above + hist[d] < krem_sh) above += hist[d--];
            prefix_sh = prefix | ((unsigned)d << shift);
            krem_sh -= above;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double a_k = (double)isc_key_score((unsigned long long)prefix_sh << 32);
        double x = (a_k - w.eps[q]) / w.denom[q];
        x -= fabs(x) * 1e-12;  // the float64 subtraction and division
        float t;
        if (!(x > -3.0e38)) {
            t = -INFINITY;
        } else if (x > 3.0e38) {
            t = 3.4028234e38f;
        } else {
            t = (float)x;
            if ((double)t > x) t = nextafterf(t, -INFINITY);
        }
        w.tau[q] = range_tau(t, w.denom[q], w.eps[q]);
    }
}

// One workgroup of 1024 threads (a pass has at most 1024 queries): the segments of the queries the filter served, and the
// list of those it did not.
__global__ __launch_bounds__(1024) void k_large_offsets(LargeWs w, int qb, int k, int32_t* __restrict__ status) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const bool over = *w.count > (unsigned long long)w.cap;
    long long v = 0;
    if (tid < qb && w.mode[tid] == MODE_FILTER) {
        v = over ? 0 : w.qcount[tid];
        if (over || (v < k && w.tau[tid] != -INFINITY)) {
            v = 0;
            w.mode[tid] = MODE_SCAN;
            w.lr_list[atomicAdd(w.lr_count, 1)] = tid;
            atomicAdd(&status[1], 1);
        }
    }
    part[tid] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long t = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    if (tid < qb) {
        w.seg_begin[tid] = part[tid] - v;
        w.seg_end[tid] = part[tid];
    }
    if (tid == 0) {
        if (over) atomicAdd(&status[0], 1);
        // the candidates the filter kept, summed over the passes (saturating): how tight the bound is
        const unsigned long long c = *w.count;
        const int add = c > 0x7fffffffull ? 0x7fffffff : (int)c;
        status[3] = status[3] > 0x7fffffff - add ? 0x7fffffff : status[3] + add;
    }
}

__global__ __launch_bounds__(256) void k_large_scatter(LargeWs w, IscPerm pm) {
    const unsigned long long end = *w.count;
    if (end > (unsigned long long)w.cap) return;
    for (unsigned long long c = blockIdx.x * 256ull + threadIdx.x; c < end; c += gridDim.x * 256ull) {
        const int q = w.cand_q[c];
        if (q < 0 || w.mode[q] != MODE_FILTER) continue;
        const int64_t pos = w.seg_begin[q] + atomicAdd(&w.fill[q], 1);
        w.keys_in[pos] = isc_make_key(w.cand_a[c], (int)isc_perm_orig(pm, w.cand_r[c]));
    }
}

// One sweep of the last resort: k_exact's loop (512 threads, GQ listed queries whole in LDS as float64, a wave per 8 bank
// rows, lane = row l >> 3, chunk l & 7) over the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  round < LR_ROUNDS: the keys
// that match the listed query's prefix above digit `round` are counted by that digit (LDS, then one atomic per non-empty
// bin).  round == LR_ROUNDS: the keys >= the prefix, by then the k-th key, are collected.
template <typename T, int GQ, typename... RowMask>
__global__ __launch_bounds__(EX_THREADS) void k_lr_sweep(const unsigned char* __restrict__ bank, int ks, IscPerm pm,
                                                         int ntiles, const void* __restrict__ queries, int q_f32,
                                                         int64_t ldq, int d, int k, int round, LargeWs w,
                                                         RowMask... row_mask) {
    const int nf = *w.lr_count;
    if (nf <= 0) return;  // the normal case
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int dp = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));  // the padded query length
    double* qd = reinterpret_cast<double*>(dyn);                     // [GQ][dp]
    int* hist = reinterpret_cast<int*>(qd + (size_t)GQ * dp);        // [GQ][256]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane >> 3, ch = lane & 7;
    const bool collect = round >= LR_ROUNDS;
    const int shift = collect ? 0 : 56 - 8 * round;

    for (int g0 = 0; g0 < nf; g0 += GQ) {
        const int gn = min(GQ, nf - g0);
        __syncthreads();  // the previous group's histograms have been flushed
        ex_stage_group<T, GQ>(queries, q_f32, ldq, d, dp, w.lr_list, g0, gn, qd);
        for (int i = tid; i < GQ * LR_BINS; i += EX_THREADS) hist[i] = 0;
        __syncthreads();
        double denom[GQ];
        ex_group_denoms<GQ>(qd, dp, denom);
        int qi[GQ];
        unsigned long long prefix[GQ];
        [[maybe_unused]] int qcode[GQ];
#pragma unroll
        for (int g = 0; g < GQ; ++g) {
            qi[g] = g < gn ? w.lr_list[g0 + g] : 0;
            prefix[g] = round == 0 ? 0ull : w.lr_prefix[qi[g]];
            if constexpr (isc_grouped<RowMask...>()) qcode[g] = g < gn ? isc_query_code((row_mask, ...), qi[g]) : -1;
        }
        for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            for (int grp = wave; grp < ISC_TILE_ROWS / 8; grp += EX_WAVES) {
                const int64_t p = (int64_t)tile * ISC_TILE_ROWS + grp * 8 + sub;
                const unsigned char* src =
                    bank + ((int64_t)tile * ks * ISC_TILE_ROWS + grp * 8 + sub) * ISC_KSTEP_BYTES + ch * 16;
                double acc[GQ];
                isc_row_dots<T, GQ>(src, ks, qd, dp, acc);
#pragma unroll
                for (int g = 0; g < GQ; ++g) {
                    if (g >= gn) break;
                    const float sc = isc_exact_score(acc[g], denom[g]);
                    bool real = ch == 0 && p < pm.n;
                    if constexpr (isc_grouped<RowMask...>()) real = real && isc_row_allowed_for(p, qcode[g], row_mask...);
                    else real = real && isc_row_allowed(p, row_mask...);
                    if (!real) continue;
                    const unsigned long long key = isc_make_key(sc, (int)isc_perm_orig(pm, p));
                    if (collect) {
                        if (key >= prefix[g]) {
                            const int pos = atomicAdd(&w.lr_fill[qi[g]], 1);
                            if (pos < k) w.keys_in[w.cap + (int64_t)qi[g] * k + pos] = key;
                        }
                    } else if (round == 0 || (key >> (shift + 8)) == (prefix[g] >> (shift + 8))) {
                        atomicAdd(&hist[g * LR_BINS + (int)((key >> shift) & 255ull)], 1);
                    }
                }
            }
        }
        __syncthreads();
        if (!collect)
            for (int i = tid; i < gn * LR_BINS; i += EX_THREADS)
                if (hist[i] != 0)
                    atomicAdd(&w.hist[(size_t)w.lr_list[g0 + i / LR_BINS] * LR_BINS + i % LR_BINS], hist[i]);
    }
}

// One workgroup per listed query: the digit of the k-th key in this round's histogram (which it zeroes for the next round).
// Fewer than k keys in all (round 0; only a filtered call): the query is short, its prefix stays 0 and the collect sweep
// takes every allowed row.  The last round fixes the query's segment: k keys (or fewer) from keys[cap + query k].
__global__ __launch_bounds__(LR_BINS) void k_lr_pick(LargeWs w, int k, int round) {
    __shared__ int h[LR_BINS];
    if ((int)blockIdx.x >= *w.lr_count) return;
    const int q = w.lr_list[blockIdx.x], tid = threadIdx.x;
    h[tid] = w.hist[(size_t)q * LR_BINS + tid];
    w.hist[(size_t)q * LR_BINS + tid] = 0;
    __syncthreads();
    if (tid != 0) return;
    unsigned long long prefix = round == 0 ? 0ull : w.lr_prefix[q];
    int krem = round == 0 ? k : w.lr_krem[q];
    int shrt = w.lr_short[q];
    if (shrt < 0) {
        int above = 0, d = LR_BINS - 1;
        while (d >= 0 && above + h[d] < krem) above += h[d--];
        if (d < 0) {
            shrt = above;  // every key there is
            prefix = 0ull;
        } else {
            prefix |= (unsigned long long)d << (56 - 8 * round);
            krem -= above;
        }
    }
    w.lr_prefix[q] = prefix;
    w.lr_krem[q] = krem;
    w.lr_short[q] = shrt;
    if (round == LR_ROUNDS - 1) {
        w.seg_begin[q] = w.cap + (int64_t)q * k;
        w.seg_end[q] = w.cap + (int64_t)q * k + (shrt < 0 ? k : shrt);
    }
}

__global__ __launch_bounds__(256) void k_large_emit(LargeWs w, int qb, int k, int64_t index_base, float* __restrict__ scores,
                                                    int64_t* __restrict__ indices) {
    const int64_t total = (int64_t)qb * k;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        const int q = (int)(i / k), j = (int)(i % k);
        const int64_t begin = w.seg_begin[q];
        if (j < w.seg_end[q] - begin) {
            const unsigned long long key = w.keys_out[begin + j];
            scores[i] = isc_key_score(key);
            indices[i] = (int64_t)isc_key_row(key) + index_base;
        } else {  // fewer than k allowed rows
            scores[i] = __uint_as_float(0x7fc00000u);
            indices[i] = INT64_MAX;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct LargeCall {
    const unsigned char* bank;
    int64_t n;
    int d, ks;
    const void* queries;  // of the pass
    int q_f32;
    int64_t ldq;
    int k;
    int64_t index_base;
    hipStream_t stream;
};

template <typename T, int GQ, typename... RowMask>
int lr_sweeps(const LargeCall& c, const LargeWs& w, int qb, RowMask... rm) {
    const int dp = c.ks * (ISC_KSTEP_BYTES / (int)sizeof(T));
    const size_t lds = (size_t)GQ * dp * 8 + (size_t)GQ * LR_BINS * 4;
    const int ntiles = (int)isc_ceil_div<int64_t>(c.n, ISC_TILE_ROWS);
    static unsigned long long attr_done = 0ull;
    const int st = ex_lds_opt_in(reinterpret_cast<const void*>(&k_lr_sweep<T, GQ, RowMask...>), attr_done);
    if (st != ISC_OK) return st;
    const int grid = grid_for(ntiles, 1, 2 * isc_device_cus());
    const IscPerm pm = isc_make_perm(c.n);
    for (int round = 0; round <= LR_ROUNDS; ++round) {
        hipLaunchKernelGGL((k_lr_sweep<T, GQ, RowMask...>), dim3(grid), dim3(EX_THREADS), lds, c.stream, c.bank, c.ks, pm,
                           ntiles, c.queries, c.q_f32, c.ldq, c.d, c.k, round, w, rm...);
        if (round < LR_ROUNDS) k_lr_pick<<<qb, LR_BINS, 0, c.stream>>>(w, c.k, round);
    }
    return ISC_OK;
}

template <typename T, typename... RowMask>
int last_resort(const LargeCall& c, const LargeWs& w, int qb, RowMask... rm) {
    const int dp = c.ks * (ISC_KSTEP_BYTES / (int)sizeof(T));
    // the LDS of GQ float64 query rows, as k_exact sizes its groups
    if (dp <= 3072) return lr_sweeps<T, 4>(c, w, qb, rm...);
    if (dp <= 6144) return lr_sweeps<T, 2>(c, w, qb, rm...);
    return lr_sweeps<T, 1>(c, w, qb, rm...);
}

// sort the pass's segments and write its rows of the result
int sort_and_emit(const LargeCall& c, const LargeWs& w, int qb, float* out_s, int64_t* out_i) {
    size_t sort_bytes = w.sort_bytes;
    if (sort_keys_desc(w.sort_tmp, sort_bytes, w.keys_in, w.keys_out, w.cap + (int64_t)w.pass * c.k, qb, w.seg_begin,
                       w.seg_end, c.stream) != hipSuccess)
        return ISC_ERR_LAUNCH;
    k_large_emit<<<grid_for((int64_t)qb * c.k, 256, 8 * isc_device_cus()), 256, 0, c.stream>>>(w, qb, c.k, c.index_base,
                                                                                             out_s, out_i);
    return ISC_OK;
}

// the RowMask pack of pass [p0, p0 + qb): the query codes of a grouped call move with the queries
inline const uint32_t* pass_mask(const uint32_t* m, int, int) { return m; }
inline IscGroups pass_mask(IscGroups g, int p0, int qb) {
    g.query_group += p0;
    g.nq = qb;
    return g;
}

template <typename T, typename TQ, typename... RowMask>
int run(bool fast, const void* bank, int64_t n, int d, const void* queries, int q, int64_t ldq, int k, int64_t index_base,
        const float* norm_bound, float* out_s, int64_t* out_i, int32_t* status, void* workspace, hipStream_t stream,
        RowMask... rm_call) {
    const int ks = isc_ksteps(d, (int)sizeof(T));
    const LargeWs w = carve(ks, q, k, fast, workspace);
    const IscPerm pm = isc_make_perm(n);
    const unsigned char* bk = static_cast<const unsigned char*>(bank);
    const int64_t ntiles = (n + ISC_TILE_ROWS - 1) / ISC_TILE_ROWS;
    const int cus = isc_device_cus();
    const int gran = large_gran(n, w.buckets);
    for (int p0 = 0; p0 < q; p0 += w.pass) {
        const int qb = q - p0 < w.pass ? q - p0 : w.pass;
        const int nqt = isc_ceil_div(qb, RQT);
        const int qpad = nqt * RQT;
        const TQ* qp = static_cast<const TQ*>(queries) + (int64_t)p0 * ldq;
        const LargeCall c{bk, n, d, ks, qp, std::is_same<TQ, float>::value ? 1 : 0, ldq, k, index_base, stream};
        const int64_t zero_items = (int64_t)w.buckets * w.qpad > (int64_t)qb * LR_BINS ? (int64_t)w.buckets * w.qpad
                                                                                      : (int64_t)qb * LR_BINS;
        k_large_begin<<<grid_for(zero_items, 256, 4 * cus), 256, 0, stream>>>(w, qb, fast ? 0 : 1, p0 == 0 ? 1 : 0, status);
        if (fast) {
            k_range_pack<T, TQ><<<isc_ceil_div(qpad * ks * 8, 256), 256, 0, stream>>>(qp, ldq, qb, d, ks, qpad, w.qpacked,
                                                                                      w.lr_count, w.zero, w.zero);
            k_large_qinfo<T><<<qpad / 4, 256, 0, stream>>>(w, ks, qb, norm_bound, status);
            // (the table's query stride is the workspace's w.qpad whatever this pass's qpad)
            k_large_bound<T, decltype(pass_mask(rm_call, p0, qb))...><<<(unsigned)(ntiles * nqt), 256, 0, stream>>>(
                bk, n, ks, nqt, w.qpacked, RangeBound{gran, w.buckets, w.qpad, w.table}, pass_mask(rm_call, p0, qb)...);
            k_large_select<<<qpad, 256, 0, stream>>>(w, qb, k);
            k_range_filter<T, decltype(pass_mask(rm_call, p0, qb))...><<<(unsigned)(ntiles * nqt), 256, 0, stream>>>(
                bk, n, ks, nqt, w.qpacked, w.tau, 0, w.count, w.cap, w.cand_q, w.cand_r, w.cand_a,
                pass_mask(rm_call, p0, qb)...);
            k_range_rescore<T><<<grid_for(w.cap, 4, 8 * cus), 256, 0, stream>>>(
                bk, ks, w.qpacked, 0, w.zero, w.count, w.cap, w.cand_q, w.cand_r, w.cand_a, w.denom, w.eps, w.mode,
                w.neg_inf, w.qcount, status);
            k_large_offsets<<<1, 1024, 0, stream>>>(w, qb, k, status);
            k_large_scatter<<<grid_for(w.cap, 256, 8 * cus), 256, 0, stream>>>(w, pm);
        }
        int st = last_resort<T>(c, w, qb, pass_mask(rm_call, p0, qb)...);
        if (st != ISC_OK) return st;
        st = sort_and_emit(c, w, qb, out_s + (size_t)p0 * k, out_i + (size_t)p0 * k);
        if (st != ISC_OK) return st;
    }
    return isc_launch_status();
}

int check_args(int dtype, int64_t n, int d, int q, int k) {
    if (dtype != ISC_F16 && dtype != ISC_F32) return ISC_ERR_INVALID_ARG;
    if (n <= 0 || d <= 0 || q <= 0 || k <= 0 || k > n) return ISC_ERR_INVALID_ARG;
    if (k > ISC_TOPK_LARGE_MAX_K || q > ISC_SEARCH_MAX_Q || d > ISC_SEARCH_MAX_D || n > 0x7ffffffe)
        return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

int workspace_bytes(bool fast, int dtype, int64_t n, int d, int q, int k, size_t* bytes) {
    ISC_REQUIRE(bytes);
    const int st = check_args(dtype, n, d, q, k);
    if (st != ISC_OK) return st;
    *bytes = carve(isc_ksteps(d, dtype == ISC_F16 ? 2 : 4), q, k, fast, nullptr).bytes;
    return ISC_OK;
}

int large(bool fast, const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q, int64_t ldq,
          int k, int64_t index_base, const float* norm_bound, float* out_scores, int64_t* out_indices, int32_t* status,
          void* workspace, size_t workspace_bytes_, const uint32_t* row_mask, const int32_t* row_group,
          const int32_t* query_group, void* stream) {
    ISC_REQUIRE(bank && queries && out_scores && out_indices && (status || !fast));
    ISC_REQUIRE(q_dtype == ISC_F16 || q_dtype == ISC_F32);
    ISC_REQUIRE((row_group == nullptr) == (query_group == nullptr));
    const int st = check_args(dtype, N, D, Q, k);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(ldq >= D);
    if (!isc_aligned(bank, 16) || !isc_aligned(workspace, 256) || !isc_aligned(row_mask, 4) ||
        !isc_aligned(row_group, 16) || !isc_aligned(query_group, 4))
        return ISC_ERR_ALIGNMENT;
    size_t need = 0;
    workspace_bytes(fast, dtype, N, D, Q, k, &need);
    if (!workspace || workspace_bytes_ < need) return ISC_ERR_WORKSPACE;
    const IscGroups g{row_mask, row_group, query_group, nullptr, Q};
#define ISC_RUN(T_, TQ_)                                                                                                \
    return row_group ? run<T_, TQ_>(fast, bank, N, D, queries, Q, ldq, k, index_base, norm_bound, out_scores, out_indices, \
                                    status, workspace, isc_stream(stream), g)                                             \
           : row_mask ? run<T_, TQ_>(fast, bank, N, D, queries, Q, ldq, k, index_base, norm_bound, out_scores,            \
                                     out_indices, status, workspace, isc_stream(stream), row_mask)                        \
                      : run<T_, TQ_>(fast, bank, N, D, queries, Q, ldq, k, index_base, norm_bound, out_scores,            \
                                     out_indices, status, workspace, isc_stream(stream))
    if (dtype == ISC_F16) {
        if (q_dtype == ISC_F16) ISC_RUN(_Float16, _Float16);
        ISC_RUN(_Float16, float);
    }
    if (q_dtype == ISC_F16) ISC_RUN(float, _Float16);
    ISC_RUN(float, float);
#undef ISC_RUN
}

}  // namespace

extern "C" int isc_cosine_topk_large_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes) {
    return workspace_bytes(true, dtype, N, D, Q, k, bytes);
}

extern "C" int isc_cosine_topk_exhaustive_large_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes) {
    return workspace_bytes(false, dtype, N, D, Q, k, bytes);
}

extern "C" int isc_cosine_topk_large(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                                     int64_t ldq, int k, int64_t index_base, const float* norm_bound, float* out_scores,
                                     int64_t* out_indices, int32_t* status, void* workspace, size_t workspace_bytes,
                                     const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group,
                                     void* stream) {
    return large(true, bank, dtype, N, D, queries, q_dtype, Q, ldq, k, index_base, norm_bound, out_scores, out_indices,
                 status, workspace, workspace_bytes, row_mask, row_group, query_group, stream);
}

extern "C" int isc_cosine_topk_exhaustive_large(const void* bank, int dtype, int64_t N, int D, const void* queries,
                                                int q_dtype, int Q, int64_t ldq, int k, int64_t index_base,
                                                float* out_scores, int64_t* out_indices, void* workspace,
                                                size_t workspace_bytes, const uint32_t* row_mask, const int32_t* row_group,
                                                const int32_t* query_group, void* stream) {
    return large(false, bank, dtype, N, D, queries, q_dtype, Q, ldq, k, index_base, nullptr, out_scores, out_indices,
                 nullptr, workspace, workspace_bytes, row_mask, row_group, query_group, stream);
}
