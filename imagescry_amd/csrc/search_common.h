// Pieces shared by the search kernels (cosine_topk.hip, search_range.hip), the exact float64 search (search_exact.hip) and
// the row-major kernels (bank_rows.hip, bank_assign.hip).  The float64 arithmetic of every exact score is in exact_dots.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bank_layout.h"
#include "exact_dots.h"
#include "isc_common.h"

// ---- (score, row) as one 64-bit key whose unsigned order is the search order ------------------------------------
// larger key = better candidate: higher score first, then LOWER row.  Keys of distinct rows are distinct.  A NaN
// score ranks below every number (the oracle's lexsort puts NaN last), and -0.0 is the same score as +0.0 (as it is to
// the oracle's comparison: a zero query scores -0.0 against a row with no positive entry, and that row ties every
// other).  0 is "empty": a real entry has row <= 2^31 - 2, so its low word is >= 1.
__device__ __forceinline__ unsigned isc_score_bits(float s) {
    if (s != s) return 0u;
    unsigned u = s == 0.f ? 0u : __float_as_uint(s);  // the bits of +0.0 for both zeros
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;  // monotone float -> unsigned; -inf -> 0x007fffff
    return u;
}
__device__ __forceinline__ unsigned long long isc_make_key(float s, int row) {
    return ((unsigned long long)isc_score_bits(s) << 32) | (unsigned)(0x7fffffff - row);
}
__device__ __forceinline__ float isc_key_score(unsigned long long k) {
    unsigned u = (unsigned)(k >> 32);
    if (u == 0u) return __uint_as_float(0x7fc00000u);  // NaN
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(u);
}
__device__ __forceinline__ int isc_key_row(unsigned long long k) {
    return 0x7fffffff - (int)(unsigned)(k & 0xffffffffu);
}
__device__ __forceinline__ unsigned long long isc_bcast_key(unsigned long long k, int src_lane) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)k, src_lane);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(k >> 32), src_lane);
    return ((unsigned long long)hi << 32) | lo;
}
// Maximum over the wave, left in every lane.  Inside a 16-lane row the partner's key comes through a DPP move (quad
// permutes, then the half-row and row mirrors: any exchange that pairs the right sub-groups does for a maximum); only
// the two steps across rows go through the LDS permute unit.  k_select / k_final call this kp times per query to peel
// off the kp largest lane maxima: with __shfl_xor at all six steps that was a third of k_select's time at Q <= 64.
template <int CTRL>
__device__ __forceinline__ void isc_key_max_dpp(unsigned& lo, unsigned& hi) {
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, 0xf, 0xf, true);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, 0xf, 0xf, true);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    const unsigned long long m = ((unsigned long long)hi << 32) | lo;
    if (o > m) {
        lo = olo;
        hi = ohi;
    }
}
__device__ __forceinline__ unsigned long long isc_wave_max_key(unsigned long long k) {
    unsigned lo = (unsigned)k, hi = (unsigned)(k >> 32);
    isc_key_max_dpp<0xB1>(lo, hi);   // quad_perm [1,0,3,2]
    isc_key_max_dpp<0x4E>(lo, hi);   // quad_perm [2,3,0,1]
    isc_key_max_dpp<0x141>(lo, hi);  // row_half_mirror
    isc_key_max_dpp<0x140>(lo, hi);  // row_mirror
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const unsigned olo = __shfl_xor(lo, off, 64), ohi = __shfl_xor(hi, off, 64);
        const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
        const unsigned long long m = ((unsigned long long)hi << 32) | lo;
        if (o > m) {
            lo = olo;
            hi = ohi;
        }
    }
    return ((unsigned long long)hi << 32) | lo;
}

// ---- row filter of a masked search (isc_row_mask_pack) ------------------------------------------------------------
// Bit p of word p / 32 allows packed position p; a tile's 256 bits are the 8 words from 8 * tile, padding bits 0.  The masked
// kernels take the bitmap as a trailing parameter PACK, empty in their unmasked instantiations: those keep their argument
// list, and with it their code (kernels that read the grid size load it from just past the explicit arguments).
//
// Per-query group exclusion (isc_*_grouped) passes ONE IscGroups in the same pack: query q may not return a row whose code
// equals its own.  Row codes are >= 0 (isc_row_groups_pack stores -2 for a negative code and the padding), and a query
// code < 0 is read as -1, so it matches no row.
struct IscGroups {
    const uint32_t* mask;        // the packed row filter as above, or NULL: every row is allowed
    const int32_t* row_group;    // int32 [ceil(N / 256) * 256]: code of packed position p (isc_row_groups_pack)
    const int32_t* query_group;  // int32: code of query i of the pass (the pass's offset applied)
    const int32_t* slot_query;   // NULL, or the slot -> query map of a redo filter launch (cosine_topk.hip, r_list)
    int nq;                      // queries of the pass: columns >= nq carry no group
};
template <typename... RowMask>
constexpr bool isc_grouped() {
    if constexpr (sizeof...(RowMask) == 1) return (std::is_same<RowMask, IscGroups>::value && ...);
    else return false;
}
template <typename... RowMask>
__host__ __device__ __forceinline__ const uint32_t* isc_row_mask_ptr(RowMask... row_mask) {
    if constexpr (sizeof...(RowMask) == 0) return nullptr;
    else if constexpr (isc_grouped<RowMask...>()) return (row_mask, ...).mask;
    else return (row_mask, ...);
}
// bit p of a packed bitmap (a row filter, a bank's fill bitmap); ... of one that may be NULL: every position is set
__device__ __forceinline__ bool isc_mask_bit(const uint32_t* m, int64_t p) { return (m[p >> 5] >> (p & 31)) & 1u; }
__device__ __forceinline__ bool isc_mask_allows(const uint32_t* m, int64_t p) {
    return m == nullptr || isc_mask_bit(m, p);
}
template <typename... RowMask>
__device__ __forceinline__ bool isc_row_allowed(int64_t p, RowMask... row_mask) {
    if constexpr (sizeof...(RowMask) == 0) return true;
    else if constexpr (isc_grouped<RowMask...>()) return isc_mask_allows(isc_row_mask_ptr(row_mask...), p);
    else return isc_mask_bit(isc_row_mask_ptr(row_mask...), p);
}
template <typename... RowMask>
__host__ __device__ __forceinline__ const int32_t* isc_row_group_ptr(RowMask... row_mask) {
    if constexpr (isc_grouped<RowMask...>()) return (row_mask, ...).row_group;
    else return nullptr;
}
// the group code of query i of the pass (-1: none), and whether query code qc may return packed position p
__device__ __forceinline__ int isc_query_code(const IscGroups& g, int i) {
    const int c = i < g.nq ? g.query_group[i] : -1;
    return c < 0 ? -1 : c;
}
template <typename... RowMask>
__device__ __forceinline__ bool isc_row_allowed_for(int64_t p, int qc, RowMask... row_mask) {
    if constexpr (isc_grouped<RowMask...>()) return isc_row_allowed(p, row_mask...) && (row_mask, ...).row_group[p] != qc;
    else return isc_row_allowed(p, row_mask...);
}

// ---- matrix-core operand traits of the filters (k_dots_filter, k_range_filter, k_assign_filter) ----------------------
// One definition of the instructions a filter issues per 16-byte chunk, so one error bound holds for all of them:
// |A - E| <= eps = Dpad 2^-23 ||q|| max||b|| for the float32 accumulator A of a dot E (the guard of k_final, the tau of the
// range search, the margin m of isc_bank_assign).
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <typename T>
struct Mma;

template <>
struct Mma<_Float16> {
    typedef f32x4 Acc;
    // acc[n] += A(16 rows) . B(16 queries x n) over the 64 halves of one K step.  One 16-byte chunk = 8 halves = the
    // k-slice one lane feeds to v_mfma_f32_16x16x32_f16; a0/b[0] hold chunks 0-3, a1/b[1] chunks 4-7.
    static __device__ __forceinline__ void half(const u32x4& a, const u32x4 (&b)[4], f32x4 (&acc)[4]) {
#pragma unroll
        for (int n = 0; n < 4; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a),
                                                            __builtin_bit_cast(half8, b[n]), acc[n], 0, 0, 0);
    }
    static __device__ __forceinline__ void row(const u32x4& a0, const u32x4& a1, const u32x4 (&b)[2][4],
                                               f32x4 (&acc)[4]) {
        half(a0, b[0], acc);
        half(a1, b[1], acc);
    }
    // query blocks N0 .. N1 - 1 of `half` (the same instructions in the same order per accumulator)
    template <int N0, int N1>
    static __device__ __forceinline__ void part(const u32x4& a, const u32x4 (&b)[4], f32x4 (&acc)[4]) {
#pragma unroll
        for (int n = N0; n < N1; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a),
                                                            __builtin_bit_cast(half8, b[n]), acc[n], 0, 0, 0);
    }
    // one block of `half`: acc += A(16 rows) . B(16 rows) over one 16-byte chunk of each
    static __device__ __forceinline__ void step(const u32x4& a, const u32x4& b, f32x4& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), acc, 0, 0,
                                                     0);
    }
};

template <>
struct Mma<float> {
    typedef f32x4 Acc;
    // one 16-byte chunk = 4 floats: element j of every lane's chunk goes to the j-th v_mfma_f32_16x16x4_f32.
    // Lane group g therefore supplies k = 4 * chunk + j instead of k = g: a permutation of the K axis applied
    // identically to both operands, which leaves the dot products unchanged.
    static __device__ __forceinline__ void half(const u32x4& a, const u32x4 (&b)[4], f32x4 (&acc)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int n = 0; n < 4; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[n][j]), acc[n],
                                                              0, 0, 0);
    }
    static __device__ __forceinline__ void row(const u32x4& a0, const u32x4& a1, const u32x4 (&b)[2][4],
                                               f32x4 (&acc)[4]) {
        half(a0, b[0], acc);
        half(a1, b[1], acc);
    }
    template <int N0, int N1>
    static __device__ __forceinline__ void part(const u32x4& a, const u32x4 (&b)[4], f32x4 (&acc)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int n = N0; n < N1; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[n][j]), acc[n],
                                                              0, 0, 0);
    }
    static __device__ __forceinline__ void step(const u32x4& a, const u32x4& b, f32x4& acc) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[j]), acc, 0, 0, 0);
    }
};

// int8 (the shadow bank of an fp16 bank, bank_layout.h): one 16-byte chunk = 16 int8 = the k-slice one lane feeds to
// v_mfma_i32_16x16x64_i8, so a 128-byte K step is 128 dimensions in the same two halves of four chunks and the loop
// around it is the fp16 one, instruction for instruction.  Only the half-major loop (`part`) is instantiated.
template <>
struct Mma<signed char> {
    typedef i32x4 Acc;
    template <int N0, int N1>
    static __device__ __forceinline__ void part(const u32x4& a, const u32x4 (&b)[4], i32x4 (&acc)[4]) {
#pragma unroll
        for (int n = N0; n < N1; ++n)
            acc[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b[n]),
                                                           acc[n], 0, 0, 0);
    }
    // `part` as the first instructions of a tile: acc[n] = A . B[n], the C operand being the constant 0 instead of a
    // register that holds 0 (the same integers, and nobody has to clear the accumulators between tiles)
    template <int N0, int N1>
    static __device__ __forceinline__ void part_first(const u32x4& a, const u32x4 (&b)[4], i32x4 (&acc)[4]) {
#pragma unroll
        for (int n = N0; n < N1; ++n)
            acc[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b[n]),
                                                           i32x4{0, 0, 0, 0}, 0, 0, 0);
    }
};

// ---- the packed image of a call's queries (k_prep of the searches, k_assign_prep of isc_bank_assign) ----------------
// queries row-major [q][ldq] -> packed [qtile][K step][tnq rows][128 B]; rows >= q and columns >= d are zero.  Thread i
// of the launch writes 16-byte chunk i of the image (i < padded queries * ks * 8).
// TQ = element type of the caller's queries: they are rounded to the bank type T while they are packed (float32 -> fp16:
// v_cvt_f16_f32, round to nearest even = `Tensor.to(float16)`; fp16 -> float32 is exact), so no cast kernel runs in front.
template <typename T, typename TQ>
__device__ __forceinline__ void isc_pack_query_chunk(const TQ* __restrict__ queries, int64_t ldq, int q, int d, int ks,
                                                     int tnq, int i, unsigned char* __restrict__ packed) {
    constexpr int PER = 16 / (int)sizeof(T);
    const int c = i & 7;
    const int row = (i >> 3) % tnq;
    const int blk = (i >> 3) / tnq;  // qtile * ks + kstep
    const int kstep = blk % ks;
    const int qrow = (blk / ks) * tnq + row;
    T v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int e = (kstep * 8 + c) * PER + j;
        v[j] = (qrow < q && e < d) ? (T)queries[(int64_t)qrow * ldq + e] : (T)0.f;
    }
    *reinterpret_cast<uint4*>(packed + (size_t)i * 16) = *reinterpret_cast<const uint4*>(v);
}

// The packed position of listed row r, or -1 for a DEAD row: one outside [0, capacity), or one whose fill bit is clear
// (empty or removed).  A dead row is never dereferenced.
__device__ __forceinline__ int64_t isc_live_pos(int64_t r, const IscPerm& pm, const uint32_t* __restrict__ fill_mask) {
    if (r < 0 || r >= pm.n) return -1;
    const int64_t p = isc_perm_pos(pm, r);
    if (fill_mask && !isc_mask_bit(fill_mask, p)) return -1;
    return p;
}

// ---- what the exact sweeps share (k_exact, k_exact_collapse, the radix sweeps of search_large.hip) -----------------
// The staged form of exact_dots.h with the listed queries whole in LDS: 512 threads, a wave per 8 bank rows.
constexpr int EX_THREADS = 512;
constexpr int EX_WAVES = EX_THREADS / 64;

// More than 64 KiB of dynamic LDS needs the opt-in, once per kernel AND device (a process may drive several GPUs):
// `attr_done` is the kernel's mask with one bit per device id, set only after the call succeeded; a failure is reported,
// not discarded.
static inline int ex_lds_opt_in(const void* kernel, unsigned long long& attr_done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ISC_ERR_NO_DEVICE;
    const bool tracked = dev >= 0 && dev < 64;
    if (!tracked || !((__atomic_load_n(&attr_done, __ATOMIC_RELAXED) >> dev) & 1ull)) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess) {
            (void)hipGetLastError();
            return ISC_ERR_UNSUPPORTED;
        }
        if (tracked) __atomic_fetch_or(&attr_done, 1ull << dev, __ATOMIC_RELAXED);
    }
    return ISC_OK;
}

// listed queries redo_list[g0 .. g0 + gn) -> qd[GQ][dp] (no barrier)
template <typename T, int GQ>
__device__ __forceinline__ void ex_stage_group(const void* __restrict__ queries, int q_f32, int64_t ldq, int d, int dp,
                                               const int32_t* __restrict__ redo_list, int g0, int gn,
                                               double* __restrict__ qd) {
    isc_stage_queries<T, GQ, EX_THREADS>(queries, q_f32, ldq, d, gn, 0, dp, dp, qd,
                                         [&](int g) { return g < gn ? redo_list[g0 + g] : 0; });
}

// the denominators of the staged group (wave g sums query g); called after the barrier that ends the staging, ends with one
template <int GQ>
__device__ __forceinline__ void ex_group_denoms(const double* __restrict__ qd, int dp, double (&denom)[GQ]) {
    static_assert(GQ <= EX_WAVES, "wave g sums the norm of query g");
    __shared__ double denom_sh[GQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < GQ) {
        const double dn = isc_norm_denom(isc_norm_partial(qd + (size_t)wave * dp, dp, 0.0));
        if (lane == 0) denom_sh[wave] = dn;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GQ; ++g) denom[g] = denom_sh[g];
}

// ---- exact float64 search of a LIST of queries (search_exact.hip) -------------------------------------------------
// Workspace of k_exact: the device-side list of queries to search (filled by k_final, or with every query by
// isc_cosine_topk_exhaustive), one sorted partial list of k keys per (listed query, chunk of bank tiles), and the
// arrival counter of the last-workgroup merge.
struct IscExactWs {
    int32_t* redo_count;       // [1]  number of listed queries
    int32_t* redo_list;        // [q]  their indices (into this pass's queries)
    int32_t* done;             // [1]  workgroups that have published their partial lists
    unsigned long long* part;  // [q][chunks][k]  keys (exact float32 score, ORIGINAL row), best first
    int chunks;                // workgroups of k_exact
    int tiles_per_chunk;
};
size_t isc_exact_ws_bytes(int64_t n, int q, int k);
IscExactWs isc_exact_ws_carve(void* base, int64_t n, int q, int k);
// enqueue k_exact: searches queries redo_list[0 .. *redo_count) and writes rows redo_list[i] of out_s / out_i
// (leading dimension k).  Queries of `q_dtype` at `queries` with leading dimension ldq (elements of q_dtype); every
// element is rounded to the bank's `dtype` first, as isc_cosine_topk does when it packs them.
// row_mask: NULL, or a packed row filter -- disallowed rows are skipped, and a query with fewer than k allowed rows gets
// the ABI's padding (score NaN, index INT64_MAX) in its last positions
int isc_exact_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq, int k,
                     int64_t index_base, const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status,
                     const uint32_t* row_mask, hipStream_t stream);
// ... of a grouped search: `groups` with the query codes of these queries (redo_list indexes them)
int isc_exact_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq, int k,
                     int64_t index_base, const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status,
                     const IscGroups& groups, hipStream_t stream);

// ---- exact float64 search of a list of queries with the rows collapsed by group (isc_cosine_topk_collapse) ---------
// The workspace of isc_exact_ws_bytes followed by the group codes of the partial lists ([q][chunks][k] int32).
size_t isc_exact_collapse_ws_bytes(int64_t n, int q, int k);
int32_t* isc_exact_collapse_codes(void* base, int64_t n, int q, int k);
// enqueue k_exact_collapse: the best k GROUPS of the listed queries (every row of `groups` carries a code; the query codes
// may be NULL: nothing excluded), rows redo_list[i] of out_s / out_i / out_c written, short answers padded with score
// NaN, index INT64_MAX, code -1
int isc_exact_collapse_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq,
                              int k, int64_t index_base, const IscExactWs& ws, int32_t* part_code, float* out_s,
                              int64_t* out_i, int32_t* out_c, const IscGroups& groups, hipStream_t stream);
