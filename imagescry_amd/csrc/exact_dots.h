// The float64 arithmetic that makes every answer exact, in ONE place (included through search_common.h).
//
// THE ORDER.  Every score the library returns is float32(E / denom) of a float64 dot E and a float64 denominator.  Two
// forms compute E; each is a fixed sequence of IEEE operations (fma, add, divide, sqrt are deterministic), so two kernels
// that call the same form return the same bits for the same (query, row).  The query is rounded to the bank type T first.
//
//   STAGED form (k_exact, k_exact_collapse, k_lr_sweep, k_row_scores, k_assign_exact, k_farthest_pass): lane l holds the 16-byte
//   chunk l & 7 of every K step of bank row l >> 3; the queries sit in LDS as float64, zero beyond d.
//     1. per lane, acc = 0, then acc = fma(q[e], a[e], acc) over the K steps in order and the chunk's elements in order
//        (isc_row_step; the zero padding contributes fma(0, x, acc));
//     2. the xor-sum over the row's 8 lanes, offsets 1, 2, 4 (group8_sum);
//     3. denom = max(sqrt(n), 1e-12), n = isc_wave_sum of the per-lane chains nacc = fma(q[e], q[e], nacc) over elements
//        lane, lane + 64, ... of the padded query (isc_norm_partial, isc_norm_denom);
//     4. float32(sum / denom) (isc_exact_score).
//   Staging the queries a few K steps at a time (isc_staged_scores) changes nothing: the accumulators live in registers
//   across the stages, so a lane's chain still runs over all K steps in order, and a stage starts at a multiple of 64
//   elements (a K step is 64 halves or 32 floats, a stage 8 of them), so the norm's per-lane element sets are the same.
//
//   PACKED-ROW form (exact_dots of cosine_topk.hip, k_range_rescore, k_assign_finish; wave_query_norm for a row with
//   itself): both operands are packed rows.  A lane's chain is acc = fma(a[j], b[j], acc) over the elements of a 16-byte
//   chunk in order (isc_packed_dot), over the chunks the kernel gives the lane in K-step order; the lanes are then summed by
//   isc_wave_sum (one wave per pair: lane l holds chunk l & 7 of K steps l >> 3, l >> 3 + 8, ...) or by group8_sum (8 lanes
//   per pair: k_assign_finish, whose chain over ALL K steps is step 1 of the staged form on the same values, so its scores
//   have k_row_scores' bits).  k_range_scan runs the whole chain in one thread; it only nominates rows for k_range_rescore.
//
// The kernels refer to this comment instead of to each other; DESIGN.md ("Bit equality") quotes it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bank_layout.h"
#include "isc_common.h"

// 16 bytes of a packed row as float64 values
template <typename T>
struct Chunk16;
template <>
struct Chunk16<_Float16> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const unsigned char* p, double (&v)[8]) {
        const uint4 raw = *reinterpret_cast<const uint4*>(p);
        const _Float16* h = reinterpret_cast<const _Float16*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (double)(float)h[j];
    }
};
template <>
struct Chunk16<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const unsigned char* p, double (&v)[8]) {
        const float4 raw = *reinterpret_cast<const float4*>(p);
        v[0] = (double)raw.x;
        v[1] = (double)raw.y;
        v[2] = (double)raw.z;
        v[3] = (double)raw.w;
    }
};

// sum over the 8 lanes that share a bank row, left in all 8
__device__ __forceinline__ double group8_sum(double v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// ---- the staged form -------------------------------------------------------------------------------------------------
// Elements [e0, e0 + en) of GQ caller queries -> LDS as float64: qd[g * stride + e] = element e0 + e of query query_of(g),
// rounded to T first (fp16 or float32 caller elements, `q_f32`), zero beyond d and for the slots g >= gn.  query_of is
// evaluated for every slot; the row of a slot >= gn is never read.  All THREADS threads of the workgroup call it.
template <typename T, int GQ, int THREADS, typename QueryOf>
__device__ __forceinline__ void isc_stage_queries(const void* __restrict__ queries, int q_f32, int64_t ldq, int d, int gn,
                                                  int e0, int en, int stride, double* __restrict__ qd, QueryOf query_of) {
    for (int g = 0; g < GQ; ++g) {
        const int64_t qi = query_of(g);
        const float* qp32 = static_cast<const float*>(queries) + qi * ldq;
        const _Float16* qp16 = static_cast<const _Float16*>(queries) + qi * ldq;
        for (int e = threadIdx.x; e < en; e += THREADS) {
            double v = 0.0;
            if (g < gn && e0 + e < d) v = (double)(float)(T)(q_f32 ? qp32[e0 + e] : (float)qp16[e0 + e]);
            qd[(size_t)g * stride + e] = v;
        }
    }
}

// step 3: this lane's chain over the staged elements lane, lane + 64, ... < en of one query, and the denominator
__device__ __forceinline__ double isc_norm_partial(const double* __restrict__ q, int en, double nacc) {
    for (int e = threadIdx.x & 63; e < en; e += 64) nacc = fma(q[e], q[e], nacc);
    return nacc;
}
__device__ __forceinline__ double isc_norm_denom(double nacc) { return fmax(sqrt(isc_wave_sum(nacc)), 1e-12); }

// step 1 for one K step: the lane's chunk `a` against its elements of GQ staged queries (qs = the chunk's first element
// of query 0); the element loop is the outer one
template <typename T, int GQ>
__device__ __forceinline__ void isc_row_step(const double (&a)[8], const double* qs, int stride, double (&acc)[GQ]) {
#pragma unroll
    for (int j = 0; j < Chunk16<T>::N; ++j)
#pragma unroll
        for (int g = 0; g < GQ; ++g) acc[g] = fma(qs[(size_t)g * stride + j], a[j], acc[g]);
}

// step 1 for a whole row against GQ queries staged whole (stride = the padded query length): src = the lane's chunk of
// K step 0
template <typename T, int GQ>
__device__ __forceinline__ void isc_row_dots(const unsigned char* src, int ks, const double* qd, int stride,
                                             double (&acc)[GQ]) {
    constexpr int EPK = ISC_KSTEP_BYTES / (int)sizeof(T);  // elements per K step
    const int ch = threadIdx.x & 7;
#pragma unroll
    for (int g = 0; g < GQ; ++g) acc[g] = 0.0;
    for (int s = 0; s < ks; ++s) {
        double a[8];
        Chunk16<T>::load(src + (size_t)s * ISC_TILE_KSTEP_BYTES, a);
        isc_row_step<T, GQ>(a, qd + s * EPK + ch * Chunk16<T>::N, stride, acc);
    }
}

// steps 2 and 4
__device__ __forceinline__ float isc_exact_score(double acc, double denom) { return (float)(group8_sum(acc) / denom); }

// The stage loop of k_row_scores and k_assign_exact: 512 threads, a wave per 8 rows, ISC_ST_GQ = 8 queries staged
// ISC_ST_KC = 8 K steps at a time (the LDS image is 32 KiB for fp16, 16 KiB for fp32, whatever D), the accumulators live
// across the stages.  `src`: this lane's chunk of K step 0 of its row, read only when `live` (a dead row's chunks are
// zero).  FIRST_BARRIER: the caller has read qd / denom_sh since the workgroup last met (it loops over query groups).
// Returns the score of query q0 + (lane & 7) in lane l: after group8_sum each of the row's 8 lanes holds all 8 sums.
constexpr int ISC_ST_THREADS = 512;
constexpr int ISC_ST_GQ = 8;
constexpr int ISC_ST_KC = 8;
static_assert(ISC_ST_GQ == 8, "lane l & 7 of a row's 8 lanes keeps query l & 7 of the group");
static_assert(ISC_ST_GQ <= ISC_ST_THREADS / 64, "wave g sums the norm of query g");
template <typename T>
constexpr int isc_st_elems() {  // elements of one staged query
    return ISC_ST_KC * (ISC_KSTEP_BYTES / (int)sizeof(T));
}

template <typename T, bool FIRST_BARRIER>
__device__ __forceinline__ float isc_staged_scores(const unsigned char* __restrict__ src, bool live, int ks,
                                                   const void* __restrict__ queries, int q_f32, int64_t ldq, int d, int q0,
                                                   int gn, double* __restrict__ qd, double* __restrict__ denom_sh) {
    constexpr int EPK = ISC_KSTEP_BYTES / (int)sizeof(T);  // elements per K step
    constexpr int PER = Chunk16<T>::N;
    constexpr int CE = isc_st_elems<T>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ch = lane & 7;
    double acc[ISC_ST_GQ];
#pragma unroll
    for (int g = 0; g < ISC_ST_GQ; ++g) acc[g] = 0.0;
    double nacc = 0.0;  // wave g: this lane's part of the squared norm of query g
    for (int s0 = 0; s0 < ks; s0 += ISC_ST_KC) {
        const int sn = min(ISC_ST_KC, ks - s0);
        if (FIRST_BARRIER || s0 > 0) __syncthreads();  // the previous stage has been read
        isc_stage_queries<T, ISC_ST_GQ, ISC_ST_THREADS>(queries, q_f32, ldq, d, gn, s0 * EPK, sn * EPK, CE, qd,
                                                        [&](int g) { return q0 + g; });
        __syncthreads();
        if (wave < ISC_ST_GQ) nacc = isc_norm_partial(qd + wave * CE, sn * EPK, nacc);
        for (int s = 0; s < sn; ++s) {
            double a[8];
            if (live) {
                Chunk16<T>::load(src + (size_t)(s0 + s) * ISC_TILE_KSTEP_BYTES, a);
            } else {
#pragma unroll
                for (int e = 0; e < PER; ++e) a[e] = 0.0;
            }
            isc_row_step<T, ISC_ST_GQ>(a, qd + s * EPK + ch * PER, CE, acc);
        }
    }
    if (wave < ISC_ST_GQ) {
        const double dn = isc_norm_denom(nacc);
        if (lane == 0) denom_sh[wave] = dn;
    }
    __syncthreads();
    float mine = 0.f;
#pragma unroll
    for (int g = 0; g < ISC_ST_GQ; ++g) {
        const float sc = isc_exact_score(acc[g], denom_sh[g]);
        if (ch == g) mine = sc;
    }
    return mine;
}

// ---- the packed-row form ---------------------------------------------------------------------------------------------
// One 16-byte chunk of U packed rows (ap) against the same chunk of one packed row (bp): all loads first (they are
// independent), then the U chains acc[u] = fma(a[u][j], b[j], acc[u]) in element order.  The searches pass bank rows as
// `ap` and the query as `bp`; k_assign_finish passes the centroid as `ap`, the staged form's operand order (the product
// commutes, so only the payload of a NaN x NaN product could tell).
template <typename T, int U>
__device__ __forceinline__ void isc_packed_dot(const unsigned char* (&ap)[U], const unsigned char* bp, double (&acc)[U]) {
    double a[U][8], b[8];
#pragma unroll
    for (int u = 0; u < U; ++u) Chunk16<T>::load(ap[u], a[u]);
    Chunk16<T>::load(bp, b);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < Chunk16<T>::N; ++j) acc[u] = fma(a[u][j], b[j], acc[u]);
}
template <typename T>
__device__ __forceinline__ double isc_packed_dot(const unsigned char* ap, const unsigned char* bp, double acc) {
    const unsigned char* a1[1] = {ap};
    double acc1[1] = {acc};
    isc_packed_dot<T, 1>(a1, bp, acc1);
    return acc1[0];
}

// float64 squared norm of the packed query row at `qrow_base` (K step s at + s * tnq * 128 B): the row's dot with itself;
// called by ONE wave, result in every lane
template <typename T>
__device__ double wave_query_norm(const unsigned char* qrow_base, int ks, int tnq) {
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 3, ch = lane & 7;
    double acc = 0.0;
    for (int s0 = 0; s0 < ks; s0 += 8) {
        const int s = s0 + sub;
        if (s < ks) {
            const unsigned char* p = qrow_base + (size_t)s * tnq * ISC_KSTEP_BYTES + ch * 16;
            acc = isc_packed_dot<T>(p, p, acc);
        }
    }
    return isc_wave_sum(acc);
}
