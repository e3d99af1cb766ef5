// Greedy farthest-point selection on a packed bank (include/imagescry_hip.h: isc_bank_farthest): M times the live, allowed
// row whose best score against the centres so far is the WORST, which then becomes a centre itself.  All on one stream, in
// stream order, nothing read back:
//
//   k_farthest_init   near[p] = -inf for every packed position, cand[p] = 1 where the row is live and allowed
//   k_farthest_pass   ONE centre against every live row, once per start row and once per pick.  The centre's packed position
//                     comes from device memory: a listed start row, or the pick of the pass before, which EVERY workgroup
//                     reduces for itself from that pass's per-workgroup keys (at most FP_MAX_BLOCKS 8-byte words in L2; the
//                     two key buffers alternate between launches).  The workgroup that owns the centre's tile publishes the
//                     pick -- out_rows[t], and out_cover[t] = near of the pick BEFORE this pass touches it -- and takes the
//                     row out of the candidates.  Then near[p] = best(near[p], S(centre, p)) for every live p, and one key
//                     per workgroup, (score bits of near << 32) | original row, MINIMISED over its candidates: lowest score
//                     first (NaN below every number, -0.0 = +0.0: the score half of isc_make_key), then the lower row.
//   k_farthest_last   one workgroup: the last pick from the last pass's keys.  When the caller wants `near` the last pick
//                     runs as one more k_farthest_pass instead, which also writes near in original row order.
//
// Launches: 1 + max(S, 1) + M.  No floating-point atomics and no atomics at all: a position's near / cand entries are read
// and written by the one workgroup that owns its tile, a key slot by one workgroup, so two calls give the same bits.
//
// The score.  S(c, r) is the staged form of exact_dots.h with ONE query staged whole: the centre's stored row is copied
// from the packed image to LDS, staged as float64 by isc_stage_queries (one stage of all K steps: it starts at element 0),
// its denominator is ex_group_denoms<1> (isc_norm_partial over the padded row, isc_norm_denom), a lane runs isc_row_step
// over its row's K steps in order (lane l: chunk l & 7 of row l >> 3 of an 8-row block) and isc_exact_score finishes.  Those
// are k_row_scores' operations in its order on the same values -- a stored row is already rounded to the bank type -- so S
// has the bits of isc_cosine_scores(row c as the query, row r).
#include <math.h>

#include "bank_layout.h"
#include "isc_common.h"
#include "search_common.h"

namespace {

constexpr int FP_THREADS = EX_THREADS;
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int FP_U = 4;  // 8-row blocks a wave holds at once: 8 waves x 4 x 8 rows = one tile per iteration
static_assert(FP_WAVES * FP_U * 8 == ISC_TILE_ROWS, "a workgroup walks the bank tile by tile");
constexpr int FP_MAX_BLOCKS = 2048;  // workgroups of a pass = keys the next pass reduces
constexpr unsigned long long FP_NONE = ~0ull;  // no candidate (a real key's low word is a row <= 2^31 - 2)

struct FarthestWs {
    float* near;                  // [npad] best score of packed position p against the centres so far
    unsigned char* cand;          // [npad] 1: p may still be picked
    unsigned long long* part[2];  // [FP_MAX_BLOCKS] the keys of a pass, alternating
    size_t bytes;
};

FarthestWs farthest_carve(void* base, int64_t n) {
    FarthestWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? static_cast<unsigned char*>(base) + off : nullptr;
        off += isc_align_up(bytes, 256);
        return p;
    };
    const size_t npad = isc_align_up((size_t)n, ISC_TILE_ROWS);
    w.part[0] = static_cast<unsigned long long*>(take(FP_MAX_BLOCKS * sizeof(unsigned long long)));
    w.part[1] = static_cast<unsigned long long*>(take(FP_MAX_BLOCKS * sizeof(unsigned long long)));
    w.near = static_cast<float*>(take(npad * sizeof(float)));
    w.cand = static_cast<unsigned char*>(take(npad));
    w.bytes = off;
    return w;
}

__global__ __launch_bounds__(256) void k_farthest_init(IscPerm pm, int64_t npad, const uint32_t* __restrict__ fill_mask,
                                                       const uint32_t* __restrict__ row_mask, float* __restrict__ near,
                                                       unsigned char* __restrict__ cand) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npad) return;
    near[p] = -INFINITY;
    cand[p] = (p < pm.n && isc_mask_allows(fill_mask, p) && isc_mask_allows(row_mask, p)) ? 1 : 0;
}

// minimum over the workgroup, in every thread (`sh`: one word per wave; begins with a barrier, so it may be called again)
__device__ __forceinline__ unsigned long long fp_block_min(unsigned long long k, unsigned long long* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    k = sh[0];
#pragma unroll
    for (int w = 1; w < FP_WAVES; ++w) k = sh[w] < k ? sh[w] : k;
    return k;
}

// the pick a pass left behind: the smallest of its keys (FP_NONE: no candidate was left)
__device__ __forceinline__ unsigned long long fp_reduce_keys(const unsigned long long* __restrict__ prev, int nprev,
                                                             unsigned long long* sh) {
    unsigned long long k = FP_NONE;
    for (int i = threadIdx.x; i < nprev; i += FP_THREADS) k = prev[i] < k ? prev[i] : k;
    return fp_block_min(k, sh);
}
__device__ __forceinline__ int64_t fp_key_row(unsigned long long k) { return (int64_t)(k & 0xffffffffull); }

// `start_row`: the centre is that listed row (a dead one: no centre); else `prev`: the centre is the pick of those keys,
// published as pick `slot`; neither: no centre (the pass before the first pick of a call without start rows).
// (4 waves per SIMD = at most 128 registers: two workgroups per CU, which is what the host sizes the grid for)
template <typename T>
__global__ __launch_bounds__(FP_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_farthest_pass(
    const unsigned char* __restrict__ bank, int d, int ks, IscPerm pm, const uint32_t* __restrict__ fill_mask,
    const int64_t* __restrict__ start_row, const unsigned long long* __restrict__ prev, int nprev, int64_t slot,
    int64_t* __restrict__ out_rows, float* __restrict__ out_cover, float* __restrict__ near,
    unsigned char* __restrict__ cand, unsigned long long* __restrict__ next, float* __restrict__ out_near) {
    constexpr int EPK = ISC_KSTEP_BYTES / (int)sizeof(T);  // elements per K step
    constexpr int PER = Chunk16<T>::N;
    extern __shared__ __attribute__((aligned(16))) double fp_lds[];  // [dp] the centre as float64, [dp] of T: its stored row
    __shared__ unsigned long long key_sh[FP_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane >> 3, ch = lane & 7;
    const int dp = ks * EPK;
    double* qd = fp_lds;
    unsigned char* crow = reinterpret_cast<unsigned char*>(fp_lds + dp);

    // ---- the centre (the same in every thread of every workgroup)
    int64_t pc = -1;
    if (start_row) {
        pc = isc_live_pos(*start_row, pm, fill_mask);
    } else if (prev) {
        const unsigned long long key = fp_reduce_keys(prev, nprev, key_sh);
        if (key != FP_NONE) {
            pc = isc_perm_pos(pm, fp_key_row(key));
        } else if (blockIdx.x == 0 && tid == 0) {  // exhausted: the padding
            out_rows[slot] = -1;
            out_cover[slot] = -INFINITY;
        }
    }
    double denom = 1.0;
    if (pc >= 0) {
        for (int c = tid; c < ks * 8; c += FP_THREADS)
            *reinterpret_cast<uint4*>(crow + (size_t)c * 16) =
                *reinterpret_cast<const uint4*>(bank + isc_packed_offset(pc, c >> 3, ks) + (c & 7) * 16);
        __syncthreads();
        isc_stage_queries<T, 1, FP_THREADS>(crow, std::is_same<T, float>::value ? 1 : 0, 0, d, 1, 0, dp, dp, qd,
                                            [](int) { return (int64_t)0; });
        __syncthreads();
        double dn[1];
        ex_group_denoms<1>(qd, dp, dn);
        denom = dn[0];
    }

    // ---- every live row of this workgroup's tiles against it
    unsigned long long best = FP_NONE;
    const int64_t ntiles = (pm.n + ISC_TILE_ROWS - 1) / ISC_TILE_ROWS;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int p[FP_U];  // (packed positions lie below 2^31: N <= 2^31 - 2)
        bool live[FP_U];
        float sc[FP_U];
#pragma unroll
        for (int u = 0; u < FP_U; ++u) {
            p[u] = (int)(tile * ISC_TILE_ROWS) + wave * (FP_U * 8) + u * 8 + sub;
            live[u] = p[u] < pm.n && isc_mask_allows(fill_mask, p[u]);
            sc[u] = 0.f;
        }
        if (pc >= 0) {
            const unsigned char* src = bank + (size_t)tile * ks * ISC_TILE_KSTEP_BYTES +
                                       (size_t)(wave * (FP_U * 8) + sub) * ISC_KSTEP_BYTES + ch * 16;
            double acc[FP_U][1];
#pragma unroll
            for (int u = 0; u < FP_U; ++u) acc[u][0] = 0.0;
            // the raw chunks of K step s + 1 are in flight while step s is converted and multiplied; a dead position is
            // never dereferenced: its chunk is zero bits, which both types read as 0.0
            uint4 raw[FP_U], ahead[FP_U];
            auto fetch = [&](int s, uint4(&r)[FP_U]) {
#pragma unroll
                for (int u = 0; u < FP_U; ++u)
                    r[u] = live[u] ? *reinterpret_cast<const uint4*>(src + (size_t)s * ISC_TILE_KSTEP_BYTES +
                                                                     u * 8 * ISC_KSTEP_BYTES)
                                   : make_uint4(0u, 0u, 0u, 0u);
            };
            fetch(0, raw);
            for (int s = 0; s < ks; ++s) {
                if (s + 1 < ks) fetch(s + 1, ahead);
#pragma unroll
                for (int u = 0; u < FP_U; ++u) {
                    double a[8];
                    Chunk16<T>::load(reinterpret_cast<const unsigned char*>(&raw[u]), a);
                    isc_row_step<T, 1>(a, qd + s * EPK + ch * PER, dp, acc[u]);
                }
#pragma unroll
                for (int u = 0; u < FP_U; ++u) raw[u] = ahead[u];
            }
#pragma unroll
            for (int u = 0; u < FP_U; ++u) sc[u] = isc_exact_score(acc[u][0], denom);
        }
        if (ch == 0) {
#pragma unroll
            for (int u = 0; u < FP_U; ++u) {
                if (p[u] >= pm.n) continue;
                const int64_t orig = isc_perm_orig(pm, p[u]);
                if (!live[u]) {
                    if (out_near) out_near[orig] = -INFINITY;
                    continue;
                }
                float cur = near[p[u]];
                const bool centre = p[u] == pc;
                if (centre && slot >= 0) {
                    out_rows[slot] = orig;
                    out_cover[slot] = cur;
                }
                if (pc >= 0 && isc_score_bits(sc[u]) > isc_score_bits(cur)) {  // a tie keeps the earlier value
                    cur = sc[u];
                    near[p[u]] = cur;
                }
                if (out_near) out_near[orig] = cur;
                if (centre) {
                    cand[p[u]] = 0;
                } else if (cand[p[u]]) {
                    const unsigned long long key = ((unsigned long long)isc_score_bits(cur) << 32) | (unsigned)orig;
                    best = key < best ? key : best;
                }
            }
        }
    }
    best = fp_block_min(best, key_sh);
    if (tid == 0) next[blockIdx.x] = best;
}

__global__ __launch_bounds__(FP_THREADS) void k_farthest_last(IscPerm pm, const unsigned long long* __restrict__ prev,
                                                              int nprev, int64_t slot, const float* __restrict__ near,
                                                              int64_t* __restrict__ out_rows, float* __restrict__ out_cover) {
    __shared__ unsigned long long key_sh[FP_WAVES];
    const unsigned long long key = fp_reduce_keys(prev, nprev, key_sh);
    if (threadIdx.x != 0) return;
    if (key == FP_NONE) {
        out_rows[slot] = -1;
        out_cover[slot] = -INFINITY;
    } else {
        out_rows[slot] = fp_key_row(key);
        out_cover[slot] = near[isc_perm_pos(pm, fp_key_row(key))];
    }
}

bool farthest_dtype_ok(int dtype) { return dtype == ISC_F16 || dtype == ISC_F32; }

int farthest_check(int dtype, int64_t n, int d) {
    ISC_REQUIRE(farthest_dtype_ok(dtype) && d > 0 && n >= 0 && n <= 0x7ffffffe);
    if (d > ISC_SEARCH_MAX_D) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

template <typename T>
int farthest_run(const void* bank, int64_t n, int d, const int64_t* start, int64_t ns, int64_t m,
                 const uint32_t* fill_mask, const uint32_t* row_mask, int64_t* out_rows, float* out_cover, float* out_near,
                 void* ws_base, hipStream_t stream) {
    static unsigned long long attr_done = 0;  // (one per T)
    const int ks = isc_ksteps(d, (int)sizeof(T));
    const int dp = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));
    const size_t lds = (size_t)dp * (sizeof(double) + sizeof(T));
    if (lds > 60 * 1024) {
        const int st = ex_lds_opt_in(reinterpret_cast<const void*>(&k_farthest_pass<T>), attr_done);
        if (st != ISC_OK) return st;
    }
    const FarthestWs w = farthest_carve(ws_base, n);
    const IscPerm pm = isc_make_perm(n);
    const unsigned char* bytes = static_cast<const unsigned char*>(bank);
    const int64_t npad = (int64_t)isc_align_up((size_t)n, ISC_TILE_ROWS);
    const int64_t ntiles = npad / ISC_TILE_ROWS;
    // one resident round of workgroups (two of 512 threads per CU at the kernel's register count), every one with the
    // same number of tiles but the last
    int64_t slots = (int64_t)isc_device_cus() * 2;
    if (slots > FP_MAX_BLOCKS) slots = FP_MAX_BLOCKS;
    const int grid = (int)isc_ceil_div<int64_t>(ntiles, isc_ceil_div<int64_t>(ntiles, slots));
    hipLaunchKernelGGL(k_farthest_init, dim3((unsigned)(npad / 256)), dim3(256), 0, stream, pm, npad, fill_mask, row_mask,
                       w.near, w.cand);
    auto pass = [&](const int64_t* start_row, const unsigned long long* prev, int64_t slot, unsigned long long* next,
                    float* near_out) {
        hipLaunchKernelGGL(k_farthest_pass<T>, dim3(grid), dim3(FP_THREADS), lds, stream, bytes, d, ks, pm, fill_mask,
                           start_row, prev, grid, slot, out_rows, out_cover, w.near, w.cand, next, near_out);
    };
    if (ns == 0) pass(nullptr, nullptr, -1, w.part[0], nullptr);
    for (int64_t i = 0; i < ns; ++i) pass(start + i, nullptr, -1, w.part[0], nullptr);
    for (int64_t t = 0; t + 1 < m; ++t) pass(nullptr, w.part[t & 1], t, w.part[(t + 1) & 1], nullptr);
    if (out_near)
        pass(nullptr, w.part[(m - 1) & 1], m - 1, w.part[m & 1], out_near);
    else
        hipLaunchKernelGGL(k_farthest_last, dim3(1), dim3(FP_THREADS), 0, stream, pm, w.part[(m - 1) & 1], grid, m - 1,
                           w.near, out_rows, out_cover);
    return isc_launch_status();
}

}  // namespace

extern "C" int isc_bank_farthest_workspace_bytes(int dtype, int64_t N, int D, size_t* bytes) {
    ISC_REQUIRE(bytes != nullptr);
    const int st = farthest_check(dtype, N, D);
    if (st != ISC_OK) return st;
    *bytes = farthest_carve(nullptr, N).bytes;
    return ISC_OK;
}

extern "C" int isc_bank_farthest(const void* bank, int dtype, int64_t N, int D, const int64_t* start, int64_t S, int64_t M,
                                 const uint32_t* fill_mask, const uint32_t* row_mask, int64_t* out_rows, float* out_cover,
                                 float* out_near, void* workspace, size_t workspace_bytes, void* stream) {
    const int st = farthest_check(dtype, N, D);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(S >= 0 && M >= 0);
    if (M > ISC_FARTHEST_MAX_PICKS) return ISC_ERR_UNSUPPORTED;
    if (M == 0) return ISC_OK;
    ISC_REQUIRE(N > 0);
    ISC_REQUIRE(bank && out_rows && out_cover && workspace && (S == 0 || start));
    if (!isc_aligned(bank, 16) || !isc_aligned(start, 8) || !isc_aligned(fill_mask, 4) || !isc_aligned(row_mask, 4) ||
        !isc_aligned(out_rows, 8) || !isc_aligned(out_cover, 4) || !isc_aligned(out_near, 4) ||
        !isc_aligned(workspace, 256))
        return ISC_ERR_ALIGNMENT;
    if (workspace_bytes < farthest_carve(nullptr, N).bytes) return ISC_ERR_WORKSPACE;
    hipStream_t s = isc_stream(stream);
    if (dtype == ISC_F16)
        return farthest_run<_Float16>(bank, N, D, start, S, M, fill_mask, row_mask, out_rows, out_cover, out_near,
                                      workspace, s);
    return farthest_run<float>(bank, N, D, start, S, M, fill_mask, row_mask, out_rows, out_cover, out_near, workspace, s);
}
