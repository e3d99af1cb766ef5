// Exact float64 search of a device-side LIST of queries, the merge of partial top-k lists, and the data-independent
// exhaustive search (include/imagescry_hip.h: isc_topk_merge, isc_cosine_topk_exhaustive).
//
// k_exact is the safety net of isc_cosine_topk: k_final lists the queries whose result the float32 filter cannot
// prove (rounding guard, overflowed candidate buffers, NaN scores) and k_exact searches exactly those again, every
// score evaluated in float64, overwriting their output rows.  It is launched after every search and exits at once
// when the list is empty, so the host never has to look at a status word.
#include "bank_layout.h"
#include "isc_common.h"
#include "search_common.h"

namespace {

constexpr int EX_MAX_CHUNKS = 256;
constexpr int EX_PASS = 1024;  // listed queries per pass of isc_cosine_topk_exhaustive

int ex_chunks(int64_t n, int k) {
    const int64_t ntiles = isc_ceil_div<int64_t>(n, ISC_TILE_ROWS);
    int want = 4096 / k;  // keeps the partial lists of a query <= 32 KiB
    if (want < 32) want = 32;
    if (want > EX_MAX_CHUNKS) want = EX_MAX_CHUNKS;
    if (want > ntiles) want = (int)ntiles;
    return want;
}

// Publish this workgroup's partial lists and tell whether it is the last of `chunks` to arrive: the last one merges
// (cdna_hip_programming.md guideline 16: every storing wave drains its stores, workgroup barrier, one agent-scope release,
// asm wait, then the counter; the last arrival acquires before it reads the others' lists).  Called by every thread.
__device__ __forceinline__ bool ex_publish_is_last(int32_t* __restrict__ done, int chunks) {
    __shared__ int last_sh;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = atomicAdd(done, 1);
        last_sh = old == chunks - 1 ? 1 : 0;
        if (last_sh) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return last_sh != 0;
}

// grid = chunks of consecutive bank tiles, 512 threads.  GQ listed queries are scored per sweep of the chunk: the
// queries sit in LDS as float64, a wave takes 8 bank rows at a time (lane = row l >> 3, 16-byte chunk l & 7 of every K
// step: each load instruction reads 1 KiB of contiguous HBM), every product and sum is float64.  Each wave keeps a
// sorted list of its best k keys (exact float32 score, ORIGINAL row) per query; per chunk they are merged into one sorted
// list per query and published; the workgroup that publishes last merges the chunks' lists (k-way merge of sorted
// lists by one wave per query) and writes the result rows.
// RowMask: empty, or the row filter of a masked search (isc_row_allowed): disallowed rows are never candidates, and a query
// with fewer than k allowed rows ends in the ABI's padding (score NaN, index INT64_MAX) instead of empty keys.  Or the
// IscGroups of a grouped search: the same, with the rows of the query's own group disallowed for that query.
template <typename T, int GQ, typename... RowMask>
__global__ __launch_bounds__(EX_THREADS) void k_exact(const unsigned char* __restrict__ bank, int ks, IscPerm pm,
                                                      int ntiles, int tiles_per_chunk, const void* __restrict__ queries,
                                                      int q_f32, int64_t ldq, int d, int k, int64_t index_base,
                                                      const int32_t* __restrict__ redo_count,
                                                      const int32_t* __restrict__ redo_list,
                                                      unsigned long long* __restrict__ part, int32_t* __restrict__ done,
                                                      float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                      int32_t* __restrict__ status, RowMask... row_mask) {
    constexpr bool MASK = sizeof...(RowMask) > 0;
    const int nf = *redo_count;
    if (nf <= 0) return;  // the normal case
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int dp = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));  // the padded query length
    double* qd = reinterpret_cast<double*>(dyn);                                     // [GQ][dp]
    unsigned long long* lists = reinterpret_cast<unsigned long long*>(qd + (size_t)GQ * dp);  // [GQ][EX_WAVES][k]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tile_begin = chunk * tiles_per_chunk;
    const int tile_end = min(ntiles, tile_begin + tiles_per_chunk);
    const int sub = lane >> 3, ch = lane & 7;

    for (int g0 = 0; g0 < nf; g0 += GQ) {
        const int gn = min(GQ, nf - g0);
        __syncthreads();  // the previous group's lists have been merged
        ex_stage_group<T, GQ>(queries, q_f32, ldq, d, dp, redo_list, g0, gn, qd);
        for (int i = tid; i < GQ * EX_WAVES * k; i += EX_THREADS) lists[i] = 0ull;
        __syncthreads();
        double denom[GQ];
        ex_group_denoms<GQ>(qd, dp, denom);
        [[maybe_unused]] int qcode[GQ];
        if constexpr (isc_grouped<RowMask...>()) {
#pragma unroll
            for (int g = 0; g < GQ; ++g) qcode[g] = g < gn ? isc_query_code((row_mask, ...), redo_list[g0 + g]) : -1;
        }

        for (int tile = tile_begin; tile < tile_end; ++tile) {
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
                    unsigned long long* wl = lists + ((size_t)g * EX_WAVES + wave) * k;
                    const unsigned long long worst = wl[k - 1];  // 0 while the list is not full
                    bool cand = ch == 0 && p < pm.n && isc_score_bits(sc) >= (unsigned)(worst >> 32);
                    if constexpr (isc_grouped<RowMask...>()) cand = cand && isc_row_allowed_for(p, qcode[g], row_mask...);
                    else if constexpr (MASK) cand = cand && isc_row_allowed(p, row_mask...);
                    unsigned long long mask = __ballot(cand);
                    if (mask == 0ull) continue;
                    const unsigned long long key = cand ? isc_make_key(sc, (int)isc_perm_orig(pm, p)) : 0ull;
                    while (mask != 0ull) {
                        const int b = __builtin_ctzll(mask);
                        mask &= mask - 1ull;
                        const unsigned long long kb = isc_bcast_key(key, b);
                        if (kb > wl[k - 1]) {  // wave-uniform
                            if (lane == 0) {
                                int pos = k - 1;
                                while (pos > 0 && kb > wl[pos - 1]) {
                                    wl[pos] = wl[pos - 1];
                                    --pos;
                                }
                                wl[pos] = kb;
                            }
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        }
                    }
                }
            }
        }
        __syncthreads();
        // the chunk's list of every query of the group: rank sort of the EX_WAVES sorted lists (empty slots are 0)
        for (int g = wave; g < gn; g += EX_WAVES) {
            const unsigned long long* all = lists + (size_t)g * EX_WAVES * k;
            unsigned long long* dst = part + ((size_t)(g0 + g) * chunks + chunk) * k;
            const int tot = EX_WAVES * k;
            for (int e = lane; e < tot; e += 64) {
                const unsigned long long mine = all[e];
                int rank = 0;
                for (int j = 0; j < tot; ++j) {
                    const unsigned long long o = all[j];
                    rank += (o > mine || (o == mine && j < e)) ? 1 : 0;
                }
                if (rank < k) dst[rank] = mine;
            }
        }
    }

    if (!ex_publish_is_last(done, chunks)) return;

    // k-way merge: a lane holds the heads of lists lane, lane + 64, ... (chunks <= 256: at most four)
    for (int f = wave; f < nf; f += EX_WAVES) {
        const int qi = redo_list[f];
        const unsigned long long* base = part + (size_t)f * chunks * k;
        int pos[4];
        unsigned long long cur[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            pos[j] = 0;
            cur[j] = c < chunks ? __hip_atomic_load(base + (size_t)c * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
        for (int r = 0; r < k; ++r) {
            unsigned long long best = cur[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) best = cur[j] > best ? cur[j] : best;
            const unsigned long long win = isc_wave_max_key(best);
            if (lane == 0) {
                if (MASK && win == 0ull) {  // fewer than k allowed rows
                    out_s[(size_t)qi * k + r] = __uint_as_float(0x7fc00000u);
                    out_i[(size_t)qi * k + r] = INT64_MAX;
                } else {
                    out_s[(size_t)qi * k + r] = isc_key_score(win);
                    out_i[(size_t)qi * k + r] = (int64_t)isc_key_row(win) + index_base;
                }
            }
            if (win != 0ull) {  // keys of distinct rows are distinct: exactly one head matches
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cur[j] == win) {
                        const int c = lane + 64 * j;
                        ++pos[j];
                        cur[j] = pos[j] < k ? __hip_atomic_load(base + (size_t)c * k + pos[j], __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT)
                                            : 0ull;
                    }
            }
        }
    }
    if (tid == 0) *done = 0;  // ready for the next launch
    (void)status;
}

__global__ void k_list_all(int32_t* redo_count, int32_t* redo_list, int32_t* done, int q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) redo_list[i] = i;
    if (i == 0) {
        *redo_count = q;
        *done = 0;
    }
}

// ---- merge of partial top-k lists ------------------------------------------------------------------------------
constexpr int MERGE_CAP = 4096;

// (score desc with NaN last, index asc)
__device__ __forceinline__ bool merge_better(float sa, int64_t ia, float sb, int64_t ib) {
    const unsigned ua = isc_score_bits(sa), ub = isc_score_bits(sb);
    return ua > ub || (ua == ub && ia < ib);
}

// One workgroup per query.  Rank sort: entry i lands at position #{j better than i}.  Entries are
// distinct (score, index) pairs unless the same row appears in two partial lists; duplicates of an
// identical pair are broken by position so every rank is still unique.
__global__ __launch_bounds__(256) void k_topk_merge(const float* __restrict__ scores,
                                                    const int64_t* __restrict__ indices, int G, int Q, int kin,
                                                    int kout, int64_t gs_scores, int64_t gs_indices,
                                                    float* __restrict__ out_s, int64_t* __restrict__ out_i) {
    __shared__ float s[MERGE_CAP];
    __shared__ int64_t ix[MERGE_CAP];
    const int q = blockIdx.x;
    const int n = G * kin;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int g = e / kin, j = e - g * kin;
        const size_t inner = (size_t)q * kin + j;
        s[e] = scores[(size_t)g * gs_scores + inner];
        ix[e] = indices[(size_t)g * gs_indices + inner];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const float se = s[e];
        const int64_t ie = ix[e];
        const unsigned ue = isc_score_bits(se);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = s[j];
            const int64_t ij = ix[j];
            rank += (merge_better(sj, ij, se, ie) || (isc_score_bits(sj) == ue && ij == ie && j < e)) ? 1 : 0;
        }
        if (rank < kout) {
            out_s[(size_t)q * kout + rank] = se;
            out_i[(size_t)q * kout + rank] = ie;
        }
    }
}

int ex_check(int dtype, int64_t n, int d, int q, int k) {
    if (dtype != ISC_F16 && dtype != ISC_F32) return ISC_ERR_INVALID_ARG;
    if (n <= 0 || d <= 0 || q <= 0 || k <= 0 || k > n) return ISC_ERR_INVALID_ARG;
    if (k > ISC_TOPK_MAX_K || q > ISC_SEARCH_MAX_Q || d > ISC_SEARCH_MAX_D || n > 0x7ffffffe) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

template <typename T, int GQ, typename... RowMask>
int launch_exact(const void* bank, int64_t n, int d, const void* queries, int q_f32, int64_t ldq, int k, int64_t index_base,
                  const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status, hipStream_t stream,
                  RowMask... row_mask) {
    const int ks = isc_ksteps(d, (int)sizeof(T));
    const int dp = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));
    const size_t lds = (size_t)GQ * dp * 8 + (size_t)GQ * EX_WAVES * k * 8;
    const int ntiles = (int)isc_ceil_div<int64_t>(n, ISC_TILE_ROWS);
    static unsigned long long attr_done = 0ull;
    const int st = ex_lds_opt_in(reinterpret_cast<const void*>(&k_exact<T, GQ, RowMask...>), attr_done);
    if (st != ISC_OK) return st;
    hipLaunchKernelGGL((k_exact<T, GQ, RowMask...>), dim3(ws.chunks), dim3(EX_THREADS), lds, stream,
                       static_cast<const unsigned char*>(bank), ks, isc_make_perm(n), ntiles, ws.tiles_per_chunk,
                       queries, q_f32, ldq, d, k, index_base, ws.redo_count, ws.redo_list, ws.part,
                       ws.done, out_s, out_i, status, row_mask...);
    return ISC_OK;
}

template <typename T, typename... RowMask>
int launch_exact_t(const void* bank, int64_t n, int d, const void* queries, int q_f32, int64_t ldq, int k, int64_t index_base,
                    const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status, hipStream_t stream,
                    RowMask... rm) {
    const int dp = isc_ksteps(d, (int)sizeof(T)) * (ISC_KSTEP_BYTES / (int)sizeof(T));
    if (dp <= 3072)
        return launch_exact<T, 4>(bank, n, d, queries, q_f32, ldq, k, index_base, ws, out_s, out_i, status, stream, rm...);
    if (dp <= 6144)
        return launch_exact<T, 2>(bank, n, d, queries, q_f32, ldq, k, index_base, ws, out_s, out_i, status, stream, rm...);
    return launch_exact<T, 1>(bank, n, d, queries, q_f32, ldq, k, index_base, ws, out_s, out_i, status, stream, rm...);
}

template <typename... RowMask>
int exact_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq, int k,
                 int64_t index_base, const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status,
                 hipStream_t stream, RowMask... rm) {
    const int qf = q_dtype == ISC_F32 ? 1 : 0;
    const int st = dtype == ISC_F16
                       ? launch_exact_t<_Float16>(bank, n, d, queries, qf, ldq, k, index_base, ws, out_s, out_i, status,
                                                  stream, rm...)
                       : launch_exact_t<float>(bank, n, d, queries, qf, ldq, k, index_base, ws, out_s, out_i, status,
                                               stream, rm...);
    return st != ISC_OK ? st : isc_launch_status();
}

}  // namespace

size_t isc_exact_ws_bytes(int64_t n, int q, int k) {
    return 256 + isc_align_up((size_t)q * 4, 256) + isc_align_up((size_t)q * ex_chunks(n, k) * k * 8, 256);
}

IscExactWs isc_exact_ws_carve(void* base, int64_t n, int q, int k) {
    IscExactWs w;
    char* b = static_cast<char*>(base);
    w.redo_count = base ? reinterpret_cast<int32_t*>(b) : nullptr;
    w.done = base ? reinterpret_cast<int32_t*>(b + 128) : nullptr;
    w.redo_list = base ? reinterpret_cast<int32_t*>(b + 256) : nullptr;
    w.part = base ? reinterpret_cast<unsigned long long*>(b + 256 + isc_align_up((size_t)q * 4, 256)) : nullptr;
    const int ntiles = (int)isc_ceil_div<int64_t>(n, ISC_TILE_ROWS);
    const int want = ex_chunks(n, k);
    w.tiles_per_chunk = isc_ceil_div(ntiles, want);
    w.chunks = isc_ceil_div(ntiles, w.tiles_per_chunk);
    return w;
}

int isc_exact_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq, int k,
                     int64_t index_base, const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status,
                     const uint32_t* row_mask, hipStream_t stream) {
    if (row_mask)
        return exact_launch(dtype, bank, n, d, queries, q_dtype, ldq, k, index_base, ws, out_s, out_i, status, stream,
                            row_mask);
    return exact_launch(dtype, bank, n, d, queries, q_dtype, ldq, k, index_base, ws, out_s, out_i, status, stream);
}

int isc_exact_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq, int k,
                     int64_t index_base, const IscExactWs& ws, float* out_s, int64_t* out_i, int32_t* status,
                     const IscGroups& groups, hipStream_t stream) {
    return exact_launch(dtype, bank, n, d, queries, q_dtype, ldq, k, index_base, ws, out_s, out_i, status, stream, groups);
}

extern "C" int isc_topk_merge(const float* scores, const int64_t* indices, int G, int Q, int kin, int kout,
                              int64_t stride_g_scores, int64_t stride_g_indices, float* out_scores,
                              int64_t* out_indices, void* stream) {
    ISC_REQUIRE(scores && indices && out_scores && out_indices);
    ISC_REQUIRE(G > 0 && Q > 0 && kin > 0 && kout > 0);
    if ((int64_t)G * kin > MERGE_CAP) return ISC_ERR_UNSUPPORTED;
    ISC_REQUIRE(kout <= G * kin);
    const int64_t dense = (int64_t)Q * kin;
    if (stride_g_scores == 0) stride_g_scores = dense;
    if (stride_g_indices == 0) stride_g_indices = dense;
    ISC_REQUIRE(stride_g_scores >= dense && stride_g_indices >= dense);
    hipLaunchKernelGGL(k_topk_merge, dim3(Q), dim3(256), 0, isc_stream(stream), scores, indices, G, Q, kin, kout,
                       stride_g_scores, stride_g_indices, out_scores, out_indices);
    return isc_launch_status();
}

extern "C" int isc_cosine_topk_exhaustive_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes) {
    ISC_REQUIRE(bytes);
    const int st = ex_check(dtype, N, D, Q, k);
    if (st != ISC_OK) return st;
    *bytes = isc_exact_ws_bytes(N, Q < EX_PASS ? Q : EX_PASS, k);
    return ISC_OK;
}

namespace {

int exhaustive(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q, int64_t ldq, int k,
               int64_t index_base, float* out_scores, int64_t* out_indices, void* workspace, size_t workspace_bytes,
               const uint32_t* row_mask, void* stream, const IscGroups* groups = nullptr) {
    ISC_REQUIRE(bank && queries && out_scores && out_indices);
    ISC_REQUIRE(q_dtype == ISC_F16 || q_dtype == ISC_F32);
    const int st = ex_check(dtype, N, D, Q, k);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(ldq >= D);
    const int qb = Q < EX_PASS ? Q : EX_PASS;
    if (!workspace || workspace_bytes < isc_exact_ws_bytes(N, qb, k)) return ISC_ERR_WORKSPACE;
    if (!isc_aligned(workspace, 256)) return ISC_ERR_ALIGNMENT;
    const IscExactWs ws = isc_exact_ws_carve(workspace, N, qb, k);
    hipStream_t s = isc_stream(stream);
    const size_t esz = q_dtype == ISC_F16 ? 2 : 4;
    for (int q0 = 0; q0 < Q; q0 += qb) {
        const int q = Q - q0 < qb ? Q - q0 : qb;
        hipLaunchKernelGGL(k_list_all, dim3(isc_ceil_div(q, 256)), dim3(256), 0, s, ws.redo_count, ws.redo_list, ws.done,
                           q);
        const void* qp = static_cast<const char*>(queries) + (size_t)q0 * ldq * esz;
        int st2;
        if (groups) {
            IscGroups g = *groups;
            g.query_group += q0;
            g.nq = q;
            st2 = isc_exact_launch(dtype, bank, N, D, qp, q_dtype, ldq, k, index_base, ws, out_scores + (size_t)q0 * k,
                                   out_indices + (size_t)q0 * k, nullptr, g, s);
        } else {
            st2 = isc_exact_launch(dtype, bank, N, D, qp, q_dtype, ldq, k, index_base, ws, out_scores + (size_t)q0 * k,
                                   out_indices + (size_t)q0 * k, nullptr, row_mask, s);
        }
        if (st2 != ISC_OK) return st2;
    }
    return isc_launch_status();
}

}  // namespace

extern "C" int isc_cosine_topk_exhaustive(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                          int Q, int64_t ldq, int k, int64_t index_base, float* out_scores,
                                          int64_t* out_indices, void* workspace, size_t workspace_bytes, void* stream) {
    return exhaustive(bank, dtype, N, D, queries, q_dtype, Q, ldq, k, index_base, out_scores, out_indices, workspace,
                      workspace_bytes, nullptr, stream);
}

extern "C" int isc_cosine_topk_exhaustive_masked(const void* bank, int dtype, int64_t N, int D, const void* queries,
                                                 int q_dtype, int Q, int64_t ldq, int k, int64_t index_base,
                                                 float* out_scores, int64_t* out_indices, void* workspace,
                                                 size_t workspace_bytes, const uint32_t* row_mask, void* stream) {
    ISC_REQUIRE(row_mask);
    return exhaustive(bank, dtype, N, D, queries, q_dtype, Q, ldq, k, index_base, out_scores, out_indices, workspace,
                      workspace_bytes, row_mask, stream);
}

extern "C" int isc_cosine_topk_exhaustive_grouped(const void* bank, int dtype, int64_t N, int D, const void* queries,
                                                  int q_dtype, int Q, int64_t ldq, int k, int64_t index_base,
                                                  float* out_scores, int64_t* out_indices, void* workspace,
                                                  size_t workspace_bytes, const uint32_t* row_mask,
                                                  const int32_t* row_group, const int32_t* query_group, void* stream) {
    ISC_REQUIRE(row_group && query_group);
    if (!isc_aligned(row_group, 16) || !isc_aligned(query_group, 4) || !isc_aligned(row_mask, 4))
        return ISC_ERR_ALIGNMENT;
    const IscGroups g{row_mask, row_group, query_group, nullptr, Q};
    return exhaustive(bank, dtype, N, D, queries, q_dtype, Q, ldq, k, index_base, out_scores, out_indices, workspace,
                      workspace_bytes, row_mask, stream, &g);
}

// ---- collapsed (distinct-group) search: the exact pass and the merge of sharded lists ------------------------------
// isc_cosine_topk_collapse answers, per query, the k GROUPS with the best keys, a group's key being the best key
// (exact float32 score desc with NaN last, ORIGINAL row asc) among the rows the query may return: its leader.
namespace {

// the group code of query i of the pass: -1 (none) without query codes (a collapsed search may exclude nothing)
__device__ __forceinline__ int collapse_query_code(const IscGroups& g, int i) {
    return g.query_group == nullptr ? -1 : isc_query_code(g, i);
}

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// k_exact with the rows collapsed by group.  Each wave keeps a list of its best k DISTINCT groups per query (key of the
// group's best row so far, and its code): a row of a group already in the list replaces that entry when it is better, any
// other row is inserted when it beats the k-th entry.  That list is exact: the leader of a group among the
// wave's k best groups beats the k-th entry whenever it arrives, and once in the list the group can only be pushed out by
// k better groups.  Per chunk the waves' lists are merged with a per-group dedupe, and the last workgroup merges the chunks'
// lists the same way.  Padding: score NaN, index INT64_MAX, code -1.
template <typename T, int GQ>
__global__ __launch_bounds__(EX_THREADS) void k_exact_collapse(
    const unsigned char* __restrict__ bank, int ks, IscPerm pm, int ntiles, int tiles_per_chunk,
    const void* __restrict__ queries, int q_f32, int64_t ldq, int d, int k, int64_t index_base,
    const int32_t* __restrict__ redo_count, const int32_t* __restrict__ redo_list, unsigned long long* __restrict__ part,
    int32_t* __restrict__ part_code, int32_t* __restrict__ done, float* __restrict__ out_s, int64_t* __restrict__ out_i,
    int32_t* __restrict__ out_c, IscGroups grp) {
    const int nf = *redo_count;
    if (nf <= 0) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int dp = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));  // the padded query length
    double* qd = reinterpret_cast<double*>(dyn);                                                 // [GQ][dp]
    unsigned long long* lists = reinterpret_cast<unsigned long long*>(qd + (size_t)GQ * dp);    // [GQ][EX_WAVES][k]
    int* lcode = reinterpret_cast<int*>(lists + (size_t)GQ * EX_WAVES * k);                     // [GQ][EX_WAVES][k]
    __shared__ int ocode[EX_WAVES][ISC_TOPK_MAX_K];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tile_begin = chunk * tiles_per_chunk;
    const int tile_end = min(ntiles, tile_begin + tiles_per_chunk);
    const int sub = lane >> 3, ch = lane & 7;

    for (int g0 = 0; g0 < nf; g0 += GQ) {
        const int gn = min(GQ, nf - g0);
        __syncthreads();  // the previous group's lists have been merged
        ex_stage_group<T, GQ>(queries, q_f32, ldq, d, dp, redo_list, g0, gn, qd);
        for (int i = tid; i < GQ * EX_WAVES * k; i += EX_THREADS) {
            lists[i] = 0ull;
            lcode[i] = -1;
        }
        __syncthreads();
        double denom[GQ];
        ex_group_denoms<GQ>(qd, dp, denom);
        int qcode[GQ];
#pragma unroll
        for (int g = 0; g < GQ; ++g) qcode[g] = g < gn ? collapse_query_code(grp, redo_list[g0 + g]) : -1;

        for (int tile = tile_begin; tile < tile_end; ++tile) {
            for (int rg = wave; rg < ISC_TILE_ROWS / 8; rg += EX_WAVES) {
                const int64_t p = (int64_t)tile * ISC_TILE_ROWS + rg * 8 + sub;
                const unsigned char* src =
                    bank + ((int64_t)tile * ks * ISC_TILE_ROWS + rg * 8 + sub) * ISC_KSTEP_BYTES + ch * 16;
                double acc[GQ];
                isc_row_dots<T, GQ>(src, ks, qd, dp, acc);
                const bool real = ch == 0 && p < pm.n && isc_row_allowed(p, grp);
                const int code = real ? grp.row_group[p] : -1;
#pragma unroll
                for (int g = 0; g < GQ; ++g) {
                    if (g >= gn) break;
                    const float sc = isc_exact_score(acc[g], denom[g]);
                    unsigned long long* wl = lists + ((size_t)g * EX_WAVES + wave) * k;
                    int* wc = lcode + ((size_t)g * EX_WAVES + wave) * k;
                    const unsigned long long worst = wl[k - 1];  // 0 while the list is not full
                    const bool cand = real && code != qcode[g] && isc_score_bits(sc) >= (unsigned)(worst >> 32);
                    unsigned long long mask = __ballot(cand);
                    if (mask == 0ull) continue;
                    const unsigned long long key = cand ? isc_make_key(sc, (int)isc_perm_orig(pm, p)) : 0ull;
                    while (mask != 0ull) {
                        const int b = __builtin_ctzll(mask);
                        mask &= mask - 1ull;
                        const unsigned long long kb = isc_bcast_key(key, b);
                        if (kb <= wl[k - 1]) continue;  // wave-uniform: cannot change the list
                        const int cb = __builtin_amdgcn_readlane(code, b);
                        // the group's entry, if the list holds it (k <= 128: two entries per lane)
                        const unsigned long long m0 = __ballot(lane < k && wl[lane] != 0ull && wc[lane] == cb);
                        const unsigned long long m1 =
                            __ballot(lane + 64 < k && wl[lane + 64] != 0ull && wc[lane + 64] == cb);
                        int pos = m0 ? __builtin_ctzll(m0) : m1 ? 64 + __builtin_ctzll(m1) : k - 1;
                        if ((m0 | m1) != 0ull && kb <= wl[pos]) continue;  // the group already has a better row
                        if (lane == 0) {
                            while (pos > 0 && kb > wl[pos - 1]) {
                                wl[pos] = wl[pos - 1];
                                wc[pos] = wc[pos - 1];
                                --pos;
                            }
                            wl[pos] = kb;
                            wc[pos] = cb;
                        }
                        wave_sync_lds();
                    }
                }
            }
        }
        __syncthreads();
        // the chunk's list of every query of the group: a wave list's entry whose group has a better entry in another
        // wave's list is dropped (the same row is in one wave's list only), then a rank sort of what is left
        for (int g = wave; g < gn; g += EX_WAVES) {
            unsigned long long* all = lists + (size_t)g * EX_WAVES * k;
            int* allc = lcode + (size_t)g * EX_WAVES * k;
            unsigned long long* dst = part + ((size_t)(g0 + g) * chunks + chunk) * k;
            int32_t* dstc = part_code + ((size_t)(g0 + g) * chunks + chunk) * k;
            const int tot = EX_WAVES * k;
            unsigned drop = 0u;  // bit i: entry lane + 64 i (tot <= 960)
            for (int e = lane, i = 0; e < tot; e += 64, ++i) {
                const unsigned long long mine = all[e];
                if (mine == 0ull) continue;
                const int c = allc[e];
                for (int j = 0; j < tot; ++j)
                    if (allc[j] == c && all[j] > mine) {
                        drop |= 1u << i;
                        break;
                    }
            }
            wave_sync_lds();
            for (int e = lane, i = 0; e < tot; e += 64, ++i)
                if ((drop >> i) & 1u) all[e] = 0ull;
            wave_sync_lds();
            for (int e = lane; e < tot; e += 64) {
                const unsigned long long mine = all[e];
                int rank = 0;
                for (int j = 0; j < tot; ++j) {
                    const unsigned long long o = all[j];
                    rank += (o > mine || (o == mine && j < e)) ? 1 : 0;
                }
                if (rank < k) {
                    dst[rank] = mine;
                    dstc[rank] = mine != 0ull ? allc[e] : -1;
                }
            }
        }
    }

    if (!ex_publish_is_last(done, chunks)) return;

    // k-way merge of the chunks' lists, best key first; a group already written is skipped (its first appearance was its
    // best row).  A lane holds the heads of lists lane, lane + 64, ... (chunks <= 256: at most four)
    for (int f = wave; f < nf; f += EX_WAVES) {
        const int qi = redo_list[f];
        const unsigned long long* base = part + (size_t)f * chunks * k;
        const int32_t* basec = part_code + (size_t)f * chunks * k;
        int pos[4];
        unsigned long long cur[4];
        int curc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            pos[j] = 0;
            cur[j] = c < chunks ? __hip_atomic_load(base + (size_t)c * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            curc[j] = c < chunks ? __hip_atomic_load(basec + (size_t)c * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
        }
        int r = 0;
        while (r < k) {
            unsigned long long best = cur[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) best = cur[j] > best ? cur[j] : best;
            const unsigned long long win = isc_wave_max_key(best);
            if (win == 0ull) break;  // every list is exhausted: fewer than k groups
            int mc = -1;
            bool mine = false;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cur[j] == win) {  // keys of distinct rows are distinct: exactly one head matches
                    const int c = lane + 64 * j;
                    mc = curc[j];
                    mine = true;
                    ++pos[j];
                    const bool more = pos[j] < k;
                    cur[j] = more ? __hip_atomic_load(base + (size_t)c * k + pos[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                  : 0ull;
                    curc[j] = more ? __hip_atomic_load(basec + (size_t)c * k + pos[j], __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT)
                                   : -1;
                }
            const int wc = __builtin_amdgcn_readlane(mc, __builtin_ctzll(__ballot(mine)));
            const bool seen = (lane < r && ocode[wave][lane] == wc) || (lane + 64 < r && ocode[wave][lane + 64] == wc);
            if (__ballot(seen) != 0ull) continue;
            if (lane == 0) {
                out_s[(size_t)qi * k + r] = isc_key_score(win);
                out_i[(size_t)qi * k + r] = (int64_t)isc_key_row(win) + index_base;
                out_c[(size_t)qi * k + r] = wc;
                ocode[wave][r] = wc;
            }
            wave_sync_lds();
            ++r;
        }
        for (int e = r + lane; e < k; e += 64) {
            out_s[(size_t)qi * k + e] = __uint_as_float(0x7fc00000u);
            out_i[(size_t)qi * k + e] = INT64_MAX;
            out_c[(size_t)qi * k + e] = -1;
        }
    }
    if (tid == 0) *done = 0;  // ready for the next launch
}

template <typename T, int GQ>
int launch_exact_collapse(const void* bank, int64_t n, int d, const void* queries, int q_f32, int64_t ldq, int k,
                          int64_t index_base, const IscExactWs& ws, int32_t* part_code, float* out_s, int64_t* out_i,
                          int32_t* out_c, const IscGroups& g, hipStream_t stream) {
    const int ks = isc_ksteps(d, (int)sizeof(T));
    const int dp = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));
    const size_t lds = (size_t)GQ * dp * 8 + (size_t)GQ * EX_WAVES * k * 12;
    const int ntiles = (int)isc_ceil_div<int64_t>(n, ISC_TILE_ROWS);
    static unsigned long long attr_done = 0ull;
    const int st = ex_lds_opt_in(reinterpret_cast<const void*>(&k_exact_collapse<T, GQ>), attr_done);
    if (st != ISC_OK) return st;
    hipLaunchKernelGGL((k_exact_collapse<T, GQ>), dim3(ws.chunks), dim3(EX_THREADS), lds, stream,
                       static_cast<const unsigned char*>(bank), ks, isc_make_perm(n), ntiles, ws.tiles_per_chunk, queries,
                       q_f32, ldq, d, k, index_base, ws.redo_count, ws.redo_list, ws.part, part_code, ws.done, out_s, out_i,
                       out_c, g);
    return ISC_OK;
}

template <typename T>
int launch_exact_collapse_t(const void* bank, int64_t n, int d, const void* queries, int q_f32, int64_t ldq, int k,
                            int64_t index_base, const IscExactWs& ws, int32_t* part_code, float* out_s, int64_t* out_i,
                            int32_t* out_c, const IscGroups& g, hipStream_t stream) {
    const int dp = isc_ksteps(d, (int)sizeof(T)) * (ISC_KSTEP_BYTES / (int)sizeof(T));
    // the LDS of GQ float64 query rows plus GQ x 8 wave lists of k 12-byte entries stays within 150 KiB
    if (dp <= 3072)
        return launch_exact_collapse<T, 4>(bank, n, d, queries, q_f32, ldq, k, index_base, ws, part_code, out_s, out_i,
                                           out_c, g, stream);
    if (dp <= 6144)
        return launch_exact_collapse<T, 2>(bank, n, d, queries, q_f32, ldq, k, index_base, ws, part_code, out_s, out_i,
                                           out_c, g, stream);
    return launch_exact_collapse<T, 1>(bank, n, d, queries, q_f32, ldq, k, index_base, ws, part_code, out_s, out_i, out_c,
                                       g, stream);
}

// ---- merge of sharded collapsed lists: the best entry per label, then the best kout ----------------------------------
constexpr int MERGE_GROUPS_CAP = 2048;

// One workgroup per query.  An entry is dropped when another entry of the same label ranks before it (the padding,
// index INT64_MAX, is never dropped and ranks last); what is left is rank-sorted as in k_topk_merge.
__global__ __launch_bounds__(256) void k_topk_merge_groups(const float* __restrict__ scores,
                                                           const int64_t* __restrict__ indices,
                                                           const int64_t* __restrict__ labels, int G, int Q, int kin,
                                                           int kout, int64_t gs_scores, int64_t gs_indices,
                                                           int64_t gs_labels, float* __restrict__ out_s,
                                                           int64_t* __restrict__ out_i, int64_t* __restrict__ out_l) {
    __shared__ float s[MERGE_GROUPS_CAP];
    __shared__ int64_t ix[MERGE_GROUPS_CAP];
    __shared__ int64_t lb[MERGE_GROUPS_CAP];
    __shared__ unsigned char keep[MERGE_GROUPS_CAP];
    __shared__ int nkeep;
    const int q = blockIdx.x;
    const int n = G * kin;
    if (threadIdx.x == 0) nkeep = 0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int g = e / kin, j = e - g * kin;
        const size_t inner = (size_t)q * kin + j;
        s[e] = scores[(size_t)g * gs_scores + inner];
        ix[e] = indices[(size_t)g * gs_indices + inner];
        lb[e] = labels[(size_t)g * gs_labels + inner];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const float se = s[e];
        const int64_t ie = ix[e], le = lb[e];
        const unsigned ue = isc_score_bits(se);
        bool k_ = true;
        if (ie != INT64_MAX)
            for (int j = 0; j < n && k_; ++j)
                if (lb[j] == le && ix[j] != INT64_MAX && j != e &&
                    (merge_better(s[j], ix[j], se, ie) || (isc_score_bits(s[j]) == ue && ix[j] == ie && j < e)))
                    k_ = false;
        keep[e] = k_ ? 1 : 0;
        if (k_) atomicAdd(&nkeep, 1);
    }
    __syncthreads();
    const int nk = nkeep;
    for (int e = threadIdx.x; e < n; e += 256) {
        if (!keep[e]) continue;
        const float se = s[e];
        const int64_t ie = ix[e];
        const unsigned ue = isc_score_bits(se);
        int rank = 0;
        for (int j = 0; j < n; ++j)
            rank += (keep[j] && (merge_better(s[j], ix[j], se, ie) || (isc_score_bits(s[j]) == ue && ix[j] == ie && j < e)))
                        ? 1
                        : 0;
        if (rank < kout) {
            out_s[(size_t)q * kout + rank] = se;
            out_i[(size_t)q * kout + rank] = ie;
            out_l[(size_t)q * kout + rank] = ie == INT64_MAX ? -1 : lb[e];
        }
    }
    for (int r = nk + (int)threadIdx.x; r < kout; r += 256) {  // fewer distinct groups than kout
        out_s[(size_t)q * kout + r] = __uint_as_float(0x7fc00000u);
        out_i[(size_t)q * kout + r] = INT64_MAX;
        out_l[(size_t)q * kout + r] = -1;
    }
}

}  // namespace

size_t isc_exact_collapse_ws_bytes(int64_t n, int q, int k) {
    return isc_exact_ws_bytes(n, q, k) + isc_align_up((size_t)q * ex_chunks(n, k) * k * 4, 256);
}

int32_t* isc_exact_collapse_codes(void* base, int64_t n, int q, int k) {
    return reinterpret_cast<int32_t*>(static_cast<char*>(base) + isc_exact_ws_bytes(n, q, k));
}

int isc_exact_collapse_launch(int dtype, const void* bank, int64_t n, int d, const void* queries, int q_dtype, int64_t ldq,
                              int k, int64_t index_base, const IscExactWs& ws, int32_t* part_code, float* out_s,
                              int64_t* out_i, int32_t* out_c, const IscGroups& groups, hipStream_t stream) {
    const int qf = q_dtype == ISC_F32 ? 1 : 0;
    const int st = dtype == ISC_F16 ? launch_exact_collapse_t<_Float16>(bank, n, d, queries, qf, ldq, k, index_base, ws,
                                                                         part_code, out_s, out_i, out_c, groups, stream)
                                    : launch_exact_collapse_t<float>(bank, n, d, queries, qf, ldq, k, index_base, ws,
                                                                      part_code, out_s, out_i, out_c, groups, stream);
    return st != ISC_OK ? st : isc_launch_status();
}

extern "C" int isc_topk_merge_groups(const float* scores, const int64_t* indices, const int64_t* labels, int G, int Q,
                                     int kin, int kout, int64_t stride_g_scores, int64_t stride_g_indices,
                                     int64_t stride_g_labels, float* out_scores, int64_t* out_indices,
                                     int64_t* out_labels, void* stream) {
    ISC_REQUIRE(scores && indices && labels && out_scores && out_indices && out_labels);
    ISC_REQUIRE(G > 0 && Q > 0 && kin > 0 && kout > 0);
    if ((int64_t)G * kin > MERGE_GROUPS_CAP) return ISC_ERR_UNSUPPORTED;
    ISC_REQUIRE(kout <= G * kin);
    const int64_t dense = (int64_t)Q * kin;
    if (stride_g_scores == 0) stride_g_scores = dense;
    if (stride_g_indices == 0) stride_g_indices = dense;
    if (stride_g_labels == 0) stride_g_labels = dense;
    ISC_REQUIRE(stride_g_scores >= dense && stride_g_indices >= dense && stride_g_labels >= dense);
    hipLaunchKernelGGL(k_topk_merge_groups, dim3(Q), dim3(256), 0, isc_stream(stream), scores, indices, labels, G, Q, kin,
                       kout, stride_g_scores, stride_g_indices, stride_g_labels, out_scores, out_indices, out_labels);
    return isc_launch_status();
}

extern "C" int isc_cosine_topk_exhaustive_collapse_workspace_bytes(int dtype, int64_t N, int D, int Q, int k,
                                                                    size_t* bytes) {
    ISC_REQUIRE(bytes);
    const int st = ex_check(dtype, N, D, Q, k);
    if (st != ISC_OK) return st;
    *bytes = isc_exact_collapse_ws_bytes(N, Q < EX_PASS ? Q : EX_PASS, k);
    return ISC_OK;
}

extern "C" int isc_cosine_topk_exhaustive_collapse(const void* bank, int dtype, int64_t N, int D, const void* queries,
                                                   int q_dtype, int Q, int64_t ldq, int k, int64_t index_base,
                                                   float* out_scores, int64_t* out_indices, void* workspace,
                                                   size_t workspace_bytes, const uint32_t* row_mask,
                                                   const int32_t* row_group, const int32_t* query_group,
                                                   int32_t* out_codes, void* stream) {
    ISC_REQUIRE(bank && queries && out_scores && out_indices && out_codes && row_group);
    ISC_REQUIRE(q_dtype == ISC_F16 || q_dtype == ISC_F32);
    if (!isc_aligned(row_group, 16) || !isc_aligned(query_group, 4) || !isc_aligned(row_mask, 4))
        return ISC_ERR_ALIGNMENT;
    const int st = ex_check(dtype, N, D, Q, k);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(ldq >= D);
    const int qb = Q < EX_PASS ? Q : EX_PASS;
    if (!workspace || workspace_bytes < isc_exact_collapse_ws_bytes(N, qb, k)) return ISC_ERR_WORKSPACE;
    if (!isc_aligned(workspace, 256)) return ISC_ERR_ALIGNMENT;
    const IscExactWs ws = isc_exact_ws_carve(workspace, N, qb, k);
    int32_t* part_code = isc_exact_collapse_codes(workspace, N, qb, k);
    hipStream_t s = isc_stream(stream);
    const size_t esz = q_dtype == ISC_F16 ? 2 : 4;
    for (int q0 = 0; q0 < Q; q0 += qb) {
        const int q = Q - q0 < qb ? Q - q0 : qb;
        hipLaunchKernelGGL(k_list_all, dim3(isc_ceil_div(q, 256)), dim3(256), 0, s, ws.redo_count, ws.redo_list, ws.done,
                           q);
        const void* qp = static_cast<const char*>(queries) + (size_t)q0 * ldq * esz;
        const IscGroups g{row_mask, row_group, query_group ? query_group + q0 : nullptr, nullptr, q};
        const int st2 = isc_exact_collapse_launch(dtype, bank, N, D, qp, q_dtype, ldq, k, index_base, ws, part_code,
                                                  out_scores + (size_t)q0 * k, out_indices + (size_t)q0 * k,
                                                  out_codes + (size_t)q0 * k, g, s);
        if (st2 != ISC_OK) return st2;
    }
    return isc_launch_status();
}
