// Row-major questions to a packed bank (include/imagescry_hip.h: isc_bank_assign, isc_bank_assign_exhaustive,
// isc_bank_group_sums): for EVERY stored row the best of a small set of centroids, and float64 sums of listed rows per group.
//
// isc_bank_assign, per pass of at most 1024 centroids (all on one stream, no host synchronisation):
//
//   k_assign_prep     centroids -> the packed K-step-major image the searches give their queries (isc_pack_query_chunk)
//   k_assign_norms    one wave per centroid: the float64 denominator max(||q||, 1e-12) in isc_cosine_scores' summation
//                     order, its float32 reciprocal for the filter, and the filter_trusted test of k_final on the norm of
//                     the packed row (wave_query_norm)
//   k_assign_filter   one workgroup per 256-row bank tile, which it streams once per centroid tile: S = centroids . rows^T
//                     on the matrix cores with the CENTROIDS as the row operand, so that a lane holds one bank row and
//                     4 * NB centroids of it and the reduction along the centroids runs in registers.  Per row it keeps
//                     the best normalised filter score F and, in LDS, the short list of centroids within 2 m of it
//   k_assign_finish   8 lanes per row: rows with one candidate are final; rows with several are re-scored in float64 with
//                     isc_cosine_scores' operations and ranked by key; rows the filter could not prove are listed
//   k_assign_exact    the data-independent float64 kernel (also isc_bank_assign_exhaustive) answers the listed rows
//
// The proof.  f_c = float32(acc_c * float32(1 / denom_c)) is the filter's normalised score of centroid c; s_c the exact
// float32 score.  |acc_c - q_c . b| <= eps_c = Dpad 2^-23 ||q_c|| ||b||_max (k_final's bound), so after the division
// |f_c - s_c| <= Dpad 2^-23 ||b||_max plus four roundings of relative size 2^-24 (the reciprocal, the product, the float32
// rounding of s_c, and the subtraction F - 2 m below), each of a magnitude <= ||b||_max (1 + 2^-10):
//     |f_c - s_c| <= m = (Dpad + 8) 2^-23 ||b||_max            (Dpad >= 32: the eight extra steps cover the four roundings)
// A centroid is dropped only when f_c < F - 2 m for the F of that moment, F being the filter score of a real centroid w:
// then s_c <= f_c + m < F - m <= s_w, STRICTLY, so c loses to w whatever their indices.  A centroid that merely ties is
// never dropped.  The list has 8 slots while the tile streams (compacted against the risen F between centroid tiles) and
// must end with at most 4; a row whose list overflowed, that met a non-finite filter score, or that belongs to a pass with
// an untrusted centroid or a non-finite norm bound goes to k_assign_exact.
#include <math.h>

#include "bank_layout.h"
#include "isc_common.h"
#include "search_common.h"

namespace {

constexpr int AS_PASS = ISC_SEARCH_PASS_QUERIES;
constexpr int AS_LIST = 8;  // candidate slots of a row while its tile streams (LDS)
constexpr int AS_KEEP = 4;  // candidates a row may hand to k_assign_finish
constexpr int AS_FIN_ROWS = 32;  // rows per workgroup of k_assign_finish (8 lanes each)

// centroid tile: 16 when the whole call has at most 16 centroids (the bank stream is then the whole cost), else 64
int tile_centroids(int c) { return c <= 16 ? 16 : 64; }

struct AssignWs {
    unsigned char* cpacked;  // [centroid tiles][K steps][tile][128 B]
    double* denom;           // [cpad] max(||q_c||, 1e-12)
    float* inv;              // [cpad] float32(1 / denom), 0 for the padding
    int32_t* untrusted;      // [1] a centroid of some pass, or the norm bound, is outside the filter's trust range
    int32_t* ncand;          // [npad] candidates of packed position p; -1: not proven
    int32_t* cand;           // [npad][AS_KEEP] centroid of the pass
    float* cand_f;           // [npad][AS_KEEP] its filter score
    unsigned char* redo;     // [npad] 1: k_assign_exact answers the row
    float* score_tmp;        // [n] the scores between passes when the caller wants none
    size_t bytes;
};

AssignWs assign_carve(void* base, int64_t n, int d, int esz, int c) {
    AssignWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? static_cast<unsigned char*>(base) + off : nullptr;
        off += isc_align_up(bytes, 256);
        return p;
    };
    const int cb = c < AS_PASS ? c : AS_PASS;
    const int tnc = tile_centroids(c);
    const size_t cpad = isc_align_up((size_t)(cb > 0 ? cb : 1), (size_t)tnc);
    const size_t npad = isc_align_up((size_t)n, ISC_TILE_ROWS);
    const int ks = isc_ksteps(d, esz);
    w.cpacked = static_cast<unsigned char*>(take(cpad * ks * ISC_KSTEP_BYTES));
    w.denom = static_cast<double*>(take(cpad * sizeof(double)));
    w.inv = static_cast<float*>(take(cpad * sizeof(float)));
    w.untrusted = static_cast<int32_t*>(take(sizeof(int32_t)));
    w.ncand = static_cast<int32_t*>(take(npad * sizeof(int32_t)));
    w.cand = static_cast<int32_t*>(take(npad * AS_KEEP * sizeof(int32_t)));
    w.cand_f = static_cast<float*>(take(npad * AS_KEEP * sizeof(float)));
    w.redo = static_cast<unsigned char*>(take(npad));
    w.score_tmp = static_cast<float*>(take(npad * sizeof(float)));
    w.bytes = off;
    return w;
}

// ---- prep -----------------------------------------------------------------------------------------------------------
template <typename T, typename TQ>
__global__ __launch_bounds__(256) void k_assign_prep(const TQ* __restrict__ centroids, int64_t ldc, int cn, int d, int ks,
                                                     int cpad, int tnc, unsigned char* __restrict__ cpacked,
                                                     int32_t* __restrict__ status, int32_t* __restrict__ untrusted,
                                                     int first_pass) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (first_pass && i < 4) status[i] = 0;
    if (first_pass && i == 0) *untrusted = 0;
    if (i >= cpad * ks * 8) return;
    isc_pack_query_chunk<T, TQ>(centroids, ldc, cn, d, ks, tnc, i, cpacked);
}

template <typename T, typename TQ>
__global__ __launch_bounds__(256) void k_assign_norms(const TQ* __restrict__ centroids, int64_t ldc, int cn, int cpad, int d,
                                                      int ks, int tnc, const unsigned char* __restrict__ cpacked,
                                                      const float* __restrict__ norm_bound, double* __restrict__ denom,
                                                      float* __restrict__ inv, int32_t* __restrict__ untrusted) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= cpad) return;
    if (c >= cn) {
        if (lane == 0) {
            denom[c] = 1.0;
            inv[c] = 0.f;
        }
        return;
    }
    // the denominator of the exact score (exact_dots.h, step 3 of the staged form, on the unpadded centroid: the padding
    // adds fma(0, 0, nacc) = nacc)
    const TQ* src = centroids + (int64_t)c * ldc;
    double nacc = 0.0;
    for (int e = lane; e < d; e += 64) {
        const double v = (double)(float)(T)src[e];
        nacc = fma(v, v, nacc);
    }
    const double dn = isc_norm_denom(nacc);
    // the trust range of the filter's bound (k_final: filter_trusted), on the norm of the packed row
    const unsigned char* qrow = cpacked + ((size_t)(c / tnc) * ks * tnc + (c % tnc)) * ISC_KSTEP_BYTES;
    const double qnorm = sqrt(wave_query_norm<T>(qrow, ks, tnc));
    const double bmax = norm_bound ? (double)*norm_bound : 1.001;
    const bool trusted = qnorm >= 1e-30 && qnorm * bmax <= 1e37;
    if (lane == 0) {
        denom[c] = dn;
        inv[c] = (float)(1.0 / dn);
        if (!trusted) atomicOr(untrusted, 1);
    }
}

// m of the proof above (float32, every factor a power of two or exact: Dpad + 8 <= 8200)
__device__ __forceinline__ float assign_margin(int dpad, const float* __restrict__ norm_bound) {
    const float bmax = norm_bound ? *norm_bound : 1.001f;
    return (float)(dpad + 8) * 1.1920928955078125e-7f * bmax;
}

// ---- the matrix-core filter -------------------------------------------------------------------------------------------
// One workgroup = one 256-row bank tile; wave w owns its rows 64 w .. 64 w + 63 as four 16-row blocks and, per centroid
// tile, NB 16-centroid blocks.  Every bank byte is used by exactly one wave, so the bank fragments go from global memory
// straight to registers (a lane reads the 16-byte chunks fg and 4 + fg of its row's 128-byte K-step segment: the wave
// consumes whole segments); the centroid fragments are read the same way from the packed image, which stays in the
// caches.  An accumulator lane holds bank row (lane & 15) of a row block and centroids 4 (lane >> 4) .. + 3 of a centroid
// block: the maximum along the centroids is 4 NB register compares and two cross-lane steps.
template <typename T, int NB>
__global__ __launch_bounds__(256) void k_assign_filter(const unsigned char* __restrict__ bank, int ks,
                                                       const unsigned char* __restrict__ cpacked,
                                                       const float* __restrict__ inv, int cn, int ctiles,
                                                       const float* __restrict__ norm_bound, int dpad,
                                                       int32_t* __restrict__ ncand, int32_t* __restrict__ cand,
                                                       float* __restrict__ cand_f) {
    constexpr int TNC = NB * 16;
    __shared__ int l_cnt[ISC_TILE_ROWS];
    __shared__ int l_bad[ISC_TILE_ROWS];
    __shared__ int l_idx[ISC_TILE_ROWS * AS_LIST];
    __shared__ float l_f[ISC_TILE_ROWS * AS_LIST];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fg = lane >> 4;
    l_cnt[tid] = 0;
    l_bad[tid] = 0;
    __syncthreads();

    const float m2 = 2.f * assign_margin(dpad, norm_bound);
    const unsigned char* abase =
        bank + (size_t)blockIdx.x * ks * ISC_TILE_KSTEP_BYTES + (size_t)(wave * 64 + frow) * ISC_KSTEP_BYTES + fg * 16;
    float best[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) best[mb] = -INFINITY;

    for (int ct = 0; ct < ctiles; ++ct) {
        const unsigned char* bbase = cpacked + (size_t)ct * ks * TNC * ISC_KSTEP_BYTES + frow * ISC_KSTEP_BYTES + fg * 16;
        f32x4 acc[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

        u32x4 a[4][2], b[NB][2];
        auto load = [&](int s, u32x4(&av)[4][2], u32x4(&bv)[NB][2]) {
            const unsigned char* ap = abase + (size_t)s * ISC_TILE_KSTEP_BYTES;
            const unsigned char* bp = bbase + (size_t)s * TNC * ISC_KSTEP_BYTES;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    av[mb][h] = *reinterpret_cast<const u32x4*>(ap + mb * 16 * ISC_KSTEP_BYTES + h * 64);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    bv[nb][h] = *reinterpret_cast<const u32x4*>(bp + nb * 16 * ISC_KSTEP_BYTES + h * 64);
        };
        load(0, a, b);
        for (int s = 0; s < ks; ++s) {
            u32x4 an[4][2], bn[NB][2];
            if (s + 1 < ks) load(s + 1, an, bn);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) Mma<T>::step(b[nb][h], a[mb][h], acc[nb][mb]);
            if (s + 1 < ks) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int h = 0; h < 2; ++h) a[mb][h] = an[mb][h];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int h = 0; h < 2; ++h) b[nb][h] = bn[nb][h];
            }
        }

        // ---- the tile's scores against the row's best so far
        const int c0 = ct * TNC + 4 * fg;
        float4 iv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) iv[nb] = *reinterpret_cast<const float4*>(inv + c0 + nb * 16);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            float v[NB][4];
            float lmax = -INFINITY;
            bool bad = false;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float ivv[4] = {iv[nb].x, iv[nb].y, iv[nb].z, iv[nb].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool valid = c0 + nb * 16 + r < cn;
                    const float x = acc[nb][mb][r] * ivv[r];
                    if (valid && !(fabsf(x) <= 3.0e38f)) bad = true;
                    v[nb][r] = valid ? x : -INFINITY;
                    lmax = fmaxf(lmax, v[nb][r]);
                }
            }
            lmax = fmaxf(lmax, __shfl_xor(lmax, 16, 64));
            lmax = fmaxf(lmax, __shfl_xor(lmax, 32, 64));
            best[mb] = fmaxf(best[mb], lmax);
            const float thr = best[mb] - m2;
            const int row = wave * 64 + mb * 16 + frow;
            if (bad) l_bad[row] = 1;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (v[nb][r] >= thr) {
                        const int slot = atomicAdd(&l_cnt[row], 1);
                        if (slot < AS_LIST) {
                            l_idx[row * AS_LIST + slot] = c0 + nb * 16 + r;
                            l_f[row * AS_LIST + slot] = v[nb][r];
                        }
                    }
        }
        __syncthreads();
        // thread tid = (wave, lane) compacts the list of row tid = wave * 64 + 16 * (lane >> 4) + (lane & 15): its best is
        // best[fg] of this very lane
        const bool last = ct + 1 == ctiles;
        int n = l_cnt[tid];
        if (n > AS_LIST / 2 || last) {
            const float mine = fg == 0 ? best[0] : fg == 1 ? best[1] : fg == 2 ? best[2] : best[3];
            const float thr = mine - m2;
            if (n > AS_LIST) {
                l_bad[tid] = 1;  // overflowed: entries were lost
                n = AS_LIST;
            }
            int k = 0;
            for (int i = 0; i < n; ++i) {
                const float f = l_f[tid * AS_LIST + i];
                const int c = l_idx[tid * AS_LIST + i];
                if (f >= thr) {
                    l_f[tid * AS_LIST + k] = f;
                    l_idx[tid * AS_LIST + k] = c;
                    ++k;
                }
            }
            l_cnt[tid] = k;
            if (last) {
                const int64_t p = (int64_t)blockIdx.x * ISC_TILE_ROWS + tid;
                const bool ok = !l_bad[tid] && k >= 1 && k <= AS_KEEP;
                ncand[p] = ok ? k : -1;
                if (ok)
                    for (int i = 0; i < k; ++i) {
                        cand[p * AS_KEEP + i] = l_idx[tid * AS_LIST + i];
                        cand_f[p * AS_KEEP + i] = l_f[tid * AS_LIST + i];
                    }
            }
        }
        __syncthreads();
    }
}

// ---- the exact finish -------------------------------------------------------------------------------------------------
// 8 lanes per packed position (lane ch: 16-byte chunk ch of every K step, the staged form's mapping).  The score of a
// candidate is the packed-row form of exact_dots.h summed by group8_sum and divided by the stored denominator: the staged
// form's operations on the same values, hence k_row_scores' bits.
template <typename T>
__global__ __launch_bounds__(256) void k_assign_finish(
    const unsigned char* __restrict__ bank, int ks, IscPerm pm, const uint32_t* __restrict__ row_mask,
    const unsigned char* __restrict__ cpacked, int tnc, const double* __restrict__ denom,
    const int32_t* __restrict__ untrusted, const float* __restrict__ norm_bound, int dpad,
    const int32_t* __restrict__ ncand, const int32_t* __restrict__ cand, const float* __restrict__ cand_f, int c_base,
    int first_pass, int want_scores, int32_t* __restrict__ out_labels, float* __restrict__ out_scores,
    unsigned char* __restrict__ redo, int32_t* __restrict__ status) {
    const int ch = threadIdx.x & 7;
    const int64_t p = (int64_t)blockIdx.x * AS_FIN_ROWS + (threadIdx.x >> 3);
    if (p >= pm.n) return;
    const bool live = isc_mask_allows(row_mask, p);
    const int64_t orig = isc_perm_orig(pm, p);
    const int nc = ncand[p];
    const bool need_redo = live && (nc < 0 || *untrusted != 0);
    if (ch == 0) redo[p] = (unsigned char)((first_pass ? 0 : redo[p]) | (need_redo ? 1 : 0));
    if (!live) {
        if (ch == 0 && first_pass) {
            out_labels[orig] = -1;
            if (out_scores) out_scores[orig] = -INFINITY;
        }
        return;
    }
    if (need_redo) return;
    if (nc == 1 && !want_scores) {
        if (ch == 0) out_labels[orig] = cand[p * AS_KEEP] + c_base;
        return;
    }
    const float mbase = assign_margin(dpad, norm_bound);
    const unsigned char* bsrc = bank + isc_packed_offset(p, 0, ks) + ch * 16;
    unsigned long long bkey = 0;
    float bscore = 0.f, ratio = 0.f;
    for (int i = 0; i < nc; ++i) {
        const int c = cand[p * AS_KEEP + i];
        const unsigned char* qsrc = cpacked + ((size_t)(c / tnc) * ks * tnc + (c % tnc)) * ISC_KSTEP_BYTES + ch * 16;
        double acc = 0.0;
        for (int s = 0; s < ks; ++s)
            acc = isc_packed_dot<T>(qsrc + (size_t)s * tnc * ISC_KSTEP_BYTES, bsrc + (size_t)s * ISC_TILE_KSTEP_BYTES, acc);
        const float sc = isc_exact_score(acc, denom[c]);
        const unsigned long long key = isc_make_key(sc, c + c_base);
        if (key > bkey) {
            bkey = key;
            bscore = sc;
        }
        ratio = fmaxf(ratio, fabsf(cand_f[p * AS_KEEP + i] - sc) / mbase);  // (a NaN never replaces the maximum)
    }
    if (ch != 0) return;
    if (nc > 1) atomicAdd(&status[0], 1);
    if (ratio > 0.f) atomicMax(reinterpret_cast<unsigned*>(&status[2]), __float_as_uint(ratio));
    int label = isc_key_row(bkey);
    if (!first_pass) {  // merge with the passes before: the earlier pass holds the lower indices and wins a tie
        const int ol = out_labels[orig];
        const float os = out_scores[orig];
        if (isc_make_key(os, ol) > bkey) {
            label = ol;
            bscore = os;
        }
    }
    out_labels[orig] = label;
    if (out_scores) out_scores[orig] = bscore;
}

// ---- the exhaustive float64 kernel ------------------------------------------------------------------------------------
// The staged form of exact_dots.h over ALL centroids: a workgroup owns 64 consecutive PACKED positions (a wave 8 of them,
// lane l: row l >> 3, chunk l & 7) and walks the centroids in groups of 8 (isc_staged_scores, the stage loop of
// k_row_scores: the scores have its bits).  Each row keeps the best key (isc_make_key(score, centroid)) and that score's
// bits.  With `redo` only the listed rows are answered, and a workgroup that holds none leaves at once.
constexpr int AX_ROWS = ISC_ST_THREADS / 64 * 8;

template <typename T>
__global__ __launch_bounds__(ISC_ST_THREADS) void k_assign_exact(const unsigned char* __restrict__ bank, int ks, IscPerm pm,
                                                                 const uint32_t* __restrict__ row_mask,
                                                                 const void* __restrict__ centroids, int c_f32, int64_t ldc,
                                                                 int d, int nc, const unsigned char* __restrict__ redo,
                                                                 int32_t* __restrict__ out_labels,
                                                                 float* __restrict__ out_scores,
                                                                 int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) double qd[ISC_ST_GQ * isc_st_elems<T>()];
    __shared__ double denom_sh[ISC_ST_GQ];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane >> 3, ch = lane & 7;
    const int64_t p = (int64_t)blockIdx.x * AX_ROWS + wave * 8 + sub;
    const bool inside = p < pm.n;
    const bool live = inside && isc_mask_allows(row_mask, p);
    const bool need = live && (redo == nullptr || redo[p] != 0);
    const int64_t orig = inside ? isc_perm_orig(pm, p) : 0;
    if (redo == nullptr && inside && !live && ch == 0) {
        out_labels[orig] = -1;
        if (out_scores) out_scores[orig] = -INFINITY;
    }
    if (!__syncthreads_or(need ? 1 : 0)) return;
    const unsigned char* src = bank + (need ? isc_packed_offset(p, 0, ks) : 0) + ch * 16;

    unsigned long long bkey = 0;
    float bscore = 0.f;
    for (int g0 = 0; g0 < nc; g0 += ISC_ST_GQ) {
        const int gn = min(ISC_ST_GQ, nc - g0);
        // (its leading barrier: the previous group's denominators have been read)
        const float mine = isc_staged_scores<T, true>(src, need, ks, centroids, c_f32, ldc, d, g0, gn, qd, denom_sh);
        // the group's best over the row's 8 lanes (lane ch holds centroid g0 + ch)
        unsigned long long key = ch < gn ? isc_make_key(mine, g0 + ch) : 0ull;
        unsigned long long gk = key;
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            const unsigned long long o = __shfl_xor(gk, off, 64);
            gk = o > gk ? o : gk;
        }
        const float gs = __shfl(mine, (lane & ~7) | ((isc_key_row(gk) - g0) & 7), 64);
        if (gk > bkey) {
            bkey = gk;
            bscore = gs;
        }
    }
    if (need && ch == 0) {
        out_labels[orig] = isc_key_row(bkey);
        if (out_scores) out_scores[orig] = bscore;
        atomicAdd(&status[1], 1);
    }
}

__global__ void k_assign_status_zero(int32_t* status) {
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// ---- float64 sums of listed rows per group ------------------------------------------------------------------------------
// The list `rows` is sorted by group; chunk j is its entries [GS_CHUNK j, GS_CHUNK (j + 1)).  A workgroup (chunk, block of
// 256 columns) first resolves its entries -- packed position or dead, and the group by bisection of `offsets` -- into LDS,
// then walks them IN LIST ORDER with one column per thread (a wave reads the 128-byte K-step segments of the row, as
// k_bank_gather does).  The entries of a group are a run; a group that lies inside one chunk is summed there and written
// straight to `sums`.  A group that spans chunks leaves one partial per chunk in the workspace -- slot 0 when its run opens
// the chunk, slot 1 when it only closes it -- and k_group_sums_reduce adds them in chunk order.  No atomics: the order of
// every addition is fixed by the list.
constexpr int GS_CHUNK = 1024;
constexpr int GS_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(GS_THREADS) void k_group_sums_part(const unsigned char* __restrict__ bank, int d, int ks,
                                                                IscPerm pm, const int64_t* __restrict__ rows, int64_t m,
                                                                const int64_t* __restrict__ offsets, int64_t ng,
                                                                const uint32_t* __restrict__ fill_mask,
                                                                double* __restrict__ sums, int64_t ld,
                                                                int64_t* __restrict__ counts, double* __restrict__ part,
                                                                int64_t* __restrict__ pcount, int dcols) {
    __shared__ int pos[GS_CHUNK];
    __shared__ int grp[GS_CHUNK];
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    const int64_t i0 = chunk * GS_CHUNK;
    const int cn = (int)min((int64_t)GS_CHUNK, m - i0);
    for (int i = tid; i < cn; i += GS_THREADS) {
        pos[i] = (int)isc_live_pos(rows[i0 + i], pm, fill_mask);
        // the group of list entry i0 + i: the last g with offsets[g] <= i0 + i (-1: outside [offsets[0], offsets[ng]))
        int64_t lo = 0, hi = ng + 1;  // first index with offsets[.] > idx lies in [lo, hi]
        const int64_t idx = i0 + i;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (offsets[mid] <= idx) lo = mid + 1;
            else hi = mid;
        }
        grp[i] = (lo == 0 || lo > ng) ? -1 : (int)(lo - 1);
    }
    __syncthreads();
    const int e = blockIdx.y * GS_THREADS + tid;
    const bool active = e < d;
    const bool counter = blockIdx.y == 0 && tid == 0;
    double acc = 0.0;
    int64_t cnt = 0;
    int cur = grp[0];
    bool at_start = true;
    auto flush = [&]() {
        if (cur < 0) return;
        const int64_t a = offsets[cur] / GS_CHUNK, b = (offsets[cur + 1] - 1) / GS_CHUNK;
        if (a == b) {
            if (active) sums[(int64_t)cur * ld + e] = acc;
            if (counter) counts[cur] = cnt;
        } else {
            const int slot = at_start ? 0 : 1;
            part[(chunk * 2 + slot) * dcols + e] = acc;
            if (counter) pcount[chunk * 2 + slot] = cnt;
        }
    };
    for (int i = 0; i < cn; ++i) {
        const int g = grp[i];
        if (g != cur) {
            flush();
            acc = 0.0;
            cnt = 0;
            cur = g;
            at_start = false;
        }
        const int p = pos[i];
        if (p >= 0 && g >= 0) {
            if (active) acc += (double)(float)isc_packed_load<T>(bank, p, e, ks);
            ++cnt;
        }
    }
    flush();
}

__global__ __launch_bounds__(GS_THREADS) void k_group_sums_reduce(const int64_t* __restrict__ offsets,
                                                                  const double* __restrict__ part,
                                                                  const int64_t* __restrict__ pcount, int dcols, int d,
                                                                  double* __restrict__ sums, int64_t ld,
                                                                  int64_t* __restrict__ counts) {
    const int64_t g = blockIdx.x;
    const int e = blockIdx.y * GS_THREADS + threadIdx.x;
    const bool counter = blockIdx.y == 0 && threadIdx.x == 0;
    const int64_t lo = offsets[g], hi = offsets[g + 1];
    if (lo >= hi) {
        if (e < d) sums[g * ld + e] = 0.0;
        if (counter) counts[g] = 0;
        return;
    }
    const int64_t a = lo / GS_CHUNK, b = (hi - 1) / GS_CHUNK;
    if (a == b) return;  // k_group_sums_part wrote it
    double acc = 0.0;
    int64_t cnt = 0;
    for (int64_t c = a; c <= b; ++c) {
        const int slot = (c == a && lo > a * GS_CHUNK) ? 1 : 0;
        acc += part[(c * 2 + slot) * dcols + e];
        cnt += pcount[c * 2 + slot];
    }
    if (e < d) sums[g * ld + e] = acc;
    if (counter) counts[g] = cnt;
}

struct GroupSumsWs {
    double* part;     // [chunks][2][dcols]
    int64_t* pcount;  // [chunks][2]
    int64_t chunks;
    int dcols;
    size_t bytes;
};
GroupSumsWs group_sums_carve(void* base, int64_t m, int d) {
    GroupSumsWs w{};
    w.chunks = isc_ceil_div<int64_t>(m, GS_CHUNK);
    w.dcols = isc_ceil_div(d, GS_THREADS) * GS_THREADS;
    const size_t pb = isc_align_up((size_t)w.chunks * 2 * w.dcols * sizeof(double), 256);
    const size_t cb = isc_align_up((size_t)w.chunks * 2 * sizeof(int64_t), 256);
    w.part = static_cast<double*>(base);
    w.pcount = base ? reinterpret_cast<int64_t*>(static_cast<unsigned char*>(base) + pb) : nullptr;
    w.bytes = pb + cb;
    return w;
}

bool assign_dtype_ok(int dtype) { return dtype == ISC_F16 || dtype == ISC_F32; }

int assign_check(int dtype, int64_t n, int d, int c) {
    ISC_REQUIRE(assign_dtype_ok(dtype) && d > 0 && c >= 0 && n >= 0 && n <= 0x7ffffffe);
    if (d > ISC_SEARCH_MAX_D || c > ISC_SEARCH_MAX_Q) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

template <typename T, typename TQ>
int assign_run(const void* bank, int64_t n, int d, const void* centroids, int c, int64_t ldc, const float* norm_bound,
               const uint32_t* row_mask, int32_t* out_labels, float* out_scores, int32_t* status, void* ws_base,
               hipStream_t stream) {
    const int ks = isc_ksteps(d, (int)sizeof(T));
    const int dpad = ks * (ISC_KSTEP_BYTES / (int)sizeof(T));
    const AssignWs w = assign_carve(ws_base, n, d, (int)sizeof(T), c);
    const IscPerm pm = isc_make_perm(n);
    const unsigned char* bytes = static_cast<const unsigned char*>(bank);
    const int ntiles = (int)isc_ceil_div<int64_t>(n, ISC_TILE_ROWS);
    const int tnc = tile_centroids(c);
    const bool multi = c > AS_PASS;
    float* scores = out_scores ? out_scores : multi ? w.score_tmp : nullptr;
    for (int c0 = 0, pass = 0; c0 < c; c0 += AS_PASS, ++pass) {
        const int cn = c - c0 < AS_PASS ? c - c0 : AS_PASS;
        const int cpad = (int)isc_align_up((size_t)cn, (size_t)tnc);
        const TQ* cptr = static_cast<const TQ*>(centroids) + (int64_t)c0 * ldc;
        hipLaunchKernelGGL((k_assign_prep<T, TQ>), dim3(isc_ceil_div(cpad * ks * 8, 256)), dim3(256), 0, stream, cptr, ldc,
                           cn, d, ks, cpad, tnc, w.cpacked, status, w.untrusted, pass == 0 ? 1 : 0);
        hipLaunchKernelGGL((k_assign_norms<T, TQ>), dim3(isc_ceil_div(cpad, 4)), dim3(256), 0, stream, cptr, ldc, cn, cpad,
                           d, ks, tnc, w.cpacked, norm_bound, w.denom, w.inv, w.untrusted);
        if (tnc == 16)
            hipLaunchKernelGGL((k_assign_filter<T, 1>), dim3(ntiles), dim3(256), 0, stream, bytes, ks, w.cpacked, w.inv, cn,
                               cpad / tnc, norm_bound, dpad, w.ncand, w.cand, w.cand_f);
        else
            hipLaunchKernelGGL((k_assign_filter<T, 4>), dim3(ntiles), dim3(256), 0, stream, bytes, ks, w.cpacked, w.inv, cn,
                               cpad / tnc, norm_bound, dpad, w.ncand, w.cand, w.cand_f);
        hipLaunchKernelGGL(k_assign_finish<T>, dim3((unsigned)isc_ceil_div<int64_t>(n, AS_FIN_ROWS)), dim3(256), 0, stream,
                           bytes, ks, pm, row_mask, w.cpacked, tnc, w.denom, w.untrusted, norm_bound, dpad, w.ncand, w.cand,
                           w.cand_f, c0, pass == 0 ? 1 : 0, scores != nullptr ? 1 : 0, out_labels, scores, w.redo, status);
    }
    hipLaunchKernelGGL(k_assign_exact<T>, dim3((unsigned)isc_ceil_div<int64_t>(n, AX_ROWS)), dim3(ISC_ST_THREADS), 0, stream,
                       bytes, ks, pm, row_mask, centroids, std::is_same<TQ, float>::value ? 1 : 0, ldc, d, c, w.redo,
                       out_labels, scores, status);
    return isc_launch_status();
}

int assign_pointers(const void* bank, const void* centroids, int c_dtype, const uint32_t* row_mask,
                    const int32_t* out_labels, const float* out_scores, const int32_t* status) {
    ISC_REQUIRE(bank && centroids && out_labels && status);
    if (!isc_aligned(bank, 16) || !isc_aligned(centroids, c_dtype == ISC_F16 ? 2 : 4) || !isc_aligned(row_mask, 4) ||
        !isc_aligned(out_labels, 4) || !isc_aligned(out_scores, 4) || !isc_aligned(status, 4))
        return ISC_ERR_ALIGNMENT;
    return ISC_OK;
}

}  // namespace

extern "C" int isc_bank_assign_workspace_bytes(int dtype, int64_t N, int D, int C, size_t* bytes) {
    ISC_REQUIRE(bytes != nullptr);
    const int st = assign_check(dtype, N, D, C);
    if (st != ISC_OK) return st;
    *bytes = assign_carve(nullptr, N, D, dtype == ISC_F16 ? 2 : 4, C).bytes;
    return ISC_OK;
}

extern "C" int isc_bank_assign(const void* bank, int dtype, int64_t N, int D, const void* centroids, int c_dtype, int C,
                               int64_t ldc, const float* norm_bound, const uint32_t* row_mask, int32_t* out_labels,
                               float* out_scores, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    int st = assign_check(dtype, N, D, C);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(assign_dtype_ok(c_dtype) && ldc >= D);
    if (C == 0 || N == 0) return ISC_OK;
    st = assign_pointers(bank, centroids, c_dtype, row_mask, out_labels, out_scores, status);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(workspace != nullptr);
    if (!isc_aligned(workspace, 256) || !isc_aligned(norm_bound, 4)) return ISC_ERR_ALIGNMENT;
    if (workspace_bytes < assign_carve(nullptr, N, D, dtype == ISC_F16 ? 2 : 4, C).bytes) return ISC_ERR_WORKSPACE;
    hipStream_t s = isc_stream(stream);
#define ISC_ASSIGN(T_, TQ_) \
    return assign_run<T_, TQ_>(bank, N, D, centroids, C, ldc, norm_bound, row_mask, out_labels, out_scores, status, workspace, s)
    if (dtype == ISC_F16) {
        if (c_dtype == ISC_F16) ISC_ASSIGN(_Float16, _Float16);
        ISC_ASSIGN(_Float16, float);
    }
    if (c_dtype == ISC_F16) ISC_ASSIGN(float, _Float16);
    ISC_ASSIGN(float, float);
#undef ISC_ASSIGN
}

extern "C" int isc_bank_assign_exhaustive(const void* bank, int dtype, int64_t N, int D, const void* centroids, int c_dtype,
                                          int C, int64_t ldc, const uint32_t* row_mask, int32_t* out_labels,
                                          float* out_scores, int32_t* status, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    int st = assign_check(dtype, N, D, C);
    if (st != ISC_OK) return st;
    ISC_REQUIRE(assign_dtype_ok(c_dtype) && ldc >= D);
    if (C == 0 || N == 0) return ISC_OK;
    st = assign_pointers(bank, centroids, c_dtype, row_mask, out_labels, out_scores, status);
    if (st != ISC_OK) return st;
    hipStream_t s = isc_stream(stream);
    const IscPerm pm = isc_make_perm(N);
    const unsigned char* bytes = static_cast<const unsigned char*>(bank);
    const unsigned blocks = (unsigned)isc_ceil_div<int64_t>(N, AX_ROWS);
    const int cf = c_dtype == ISC_F32 ? 1 : 0;
    hipLaunchKernelGGL(k_assign_status_zero, dim3(1), dim3(64), 0, s, status);
    if (dtype == ISC_F16)
        hipLaunchKernelGGL(k_assign_exact<_Float16>, dim3(blocks), dim3(ISC_ST_THREADS), 0, s, bytes, isc_ksteps(D, 2), pm,
                           row_mask, centroids, cf, ldc, D, C, nullptr, out_labels, out_scores, status);
    else
        hipLaunchKernelGGL(k_assign_exact<float>, dim3(blocks), dim3(ISC_ST_THREADS), 0, s, bytes, isc_ksteps(D, 4), pm,
                           row_mask, centroids, cf, ldc, D, C, nullptr, out_labels, out_scores, status);
    return isc_launch_status();
}

extern "C" int isc_bank_group_sums_workspace_bytes(int dtype, int64_t M, int D, size_t* bytes) {
    ISC_REQUIRE(bytes != nullptr && assign_dtype_ok(dtype) && M >= 0 && D > 0);
    if (D > ISC_SEARCH_MAX_D) return ISC_ERR_UNSUPPORTED;
    *bytes = group_sums_carve(nullptr, M, D).bytes;
    return ISC_OK;
}

extern "C" int isc_bank_group_sums(const void* bank, int dtype, int64_t N, int D, const int64_t* rows, int64_t M,
                                   const int64_t* offsets, int64_t G, const uint32_t* fill_mask, double* sums, int64_t ld,
                                   int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    ISC_REQUIRE(assign_dtype_ok(dtype) && D > 0 && M >= 0 && G >= 0 && ld >= D);
    ISC_REQUIRE(N > 0 && N <= 0x7ffffffe);
    if (D > ISC_SEARCH_MAX_D || G > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    if (G == 0) return ISC_OK;
    ISC_REQUIRE(bank && offsets && sums && counts && (M == 0 || (rows && workspace)));
    if (!isc_aligned(bank, 16) || !isc_aligned(rows, 8) || !isc_aligned(offsets, 8) || !isc_aligned(fill_mask, 4) ||
        !isc_aligned(sums, 8) || !isc_aligned(counts, 8) || !isc_aligned(workspace, 256))
        return ISC_ERR_ALIGNMENT;
    const GroupSumsWs w = group_sums_carve(workspace, M, D);
    if (M > 0 && workspace_bytes < w.bytes) return ISC_ERR_WORKSPACE;
    if (w.chunks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    hipStream_t s = isc_stream(stream);
    const IscPerm pm = isc_make_perm(N);
    const unsigned char* bytes = static_cast<const unsigned char*>(bank);
    const dim3 cols((unsigned)(w.dcols / GS_THREADS));
    if (M > 0) {
        const dim3 grid((unsigned)w.chunks, cols.x);
        if (dtype == ISC_F16)
            hipLaunchKernelGGL(k_group_sums_part<_Float16>, grid, dim3(GS_THREADS), 0, s, bytes, D, isc_ksteps(D, 2), pm,
                               rows, M, offsets, G, fill_mask, sums, ld, counts, w.part, w.pcount, w.dcols);
        else
            hipLaunchKernelGGL(k_group_sums_part<float>, grid, dim3(GS_THREADS), 0, s, bytes, D, isc_ksteps(D, 4), pm, rows,
                               M, offsets, G, fill_mask, sums, ld, counts, w.part, w.pcount, w.dcols);
    }
    hipLaunchKernelGGL(k_group_sums_reduce, dim3((unsigned)G, cols.x), dim3(GS_THREADS), 0, s, offsets, w.part, w.pcount,
                       w.dcols, D, sums, ld, counts);
    return isc_launch_status();
}
