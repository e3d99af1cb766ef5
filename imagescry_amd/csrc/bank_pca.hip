// PCA on a packed bank (include/imagescry_hip.h: isc_bank_gram, isc_bank_project): the centred Gram matrix of the live rows
// and the projection of every live row, both read from the packed image, the projection written as the packed image of
// the narrower bank.  In both the centred operand is a_r = float32(b_r) - mean, one float32 subtraction of the stored value
// widened exactly, and the products run on v_mfma_f32_16x16x4_f32: a k-ordered float32 fma chain, no reduced precision.
//
// isc_bank_gram.  The reduction axis is the ROW axis, the strided axis of [tile][K step][row][128 B], and the MFMA wants
// lane l to hold feature (l & 15) of row (l >> 4).  No transpose is made: lane l = (c, rr) = (l & 15, l >> 4) loads the
// 16-byte chunk c of a 256-byte GROUP (two K steps) of row rr -- E = 8 fp16 or 4 fp32 features -- and the MFMA (t, u) takes
// element t of every lane's A chunk and element u of every lane's B chunk: it multiplies the 16 features {E c + t} of group A
// by the 16 features {E c + u} of group B over 4 rows.  That fixed permutation of the features of a group is undone when the
// partial is stored.  A workgroup owns one 128 x 128 tile of the upper triangle and one chunk of GR_CHUNK packed rows; a wave
// holds 16 accumulators (fp16: 2 of the 8 values of t, all 8 of u; fp32: one of the 2 x 2 pairs of 64-feature groups, all
// 4 x 4 of (t, u)), so a wave issues 16 MFMAs per two 16-byte loads.  A dead row's lanes load nothing and feed 0 to BOTH
// operands: neither the zeros of a padding row nor the stale vector of a removed row is ever centred.  The float32 partial
// of every chunk goes to the workspace; k_bank_gram_reduce adds them in chunk order in float64 and mirrors the upper
// triangle, so the result is symmetric bit for bit and two calls give the same bits (no floating-point atomics).
//
// isc_bank_project.  The bank rows are the M operand and the reduction runs along the features: lane (row, q) = (l & 15,
// l >> 4) loads chunks q and 4 + q of its row's K-step segment, and the MFMA (h, t) takes element t of chunk 4 h + q, with
// the matching row of w as the other operand.  A workgroup owns 16 MB packed rows; wave w computes the 16-column blocks
// w, w + 4, ... of all of them into an LDS image [row][K] of p_r.  Then one wave per row writes out_rows from that image and
// hands the same image row to isc_pack_row, the row body of isc_bank_pack / isc_bank_append: both outputs come from the
// one p_r.
#include <math.h>

#include "bank_layout.h"
#include "bank_pack_row.h"
#include "isc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int PCA_MAX_D = 2048;
constexpr int GR_CHUNK = 32768;  // packed rows (live or dead) per float32 partial Gram
constexpr int GR_TILE = 128;     // features per side of a workgroup's Gram tile

template <typename T>
struct Elems;
template <>
struct Elems<_Float16> {
    static constexpr int E = 8;  // elements of a 16-byte chunk
    static __device__ __forceinline__ float get(const u32x4& v, int e) {
        const unsigned w = v[e >> 1];
        const unsigned short bits = (unsigned short)((e & 1) ? (w >> 16) : (w & 0xffffu));
        return (float)__builtin_bit_cast(_Float16, bits);
    }
};
template <>
struct Elems<float> {
    static constexpr int E = 4;
    static __device__ __forceinline__ float get(const u32x4& v, int e) { return __uint_as_float(v[e]); }
};

__device__ __forceinline__ bool live_bit(const uint32_t* __restrict__ m, int64_t p, int64_t n) {
    return p < n && (m == nullptr || ((m[p >> 5] >> (p & 31)) & 1u));
}

// ---- Gram ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_bank_gram_part(const unsigned char* __restrict__ bank, int ks, int d, int64_t n,
                                                        int64_t npad, const float* __restrict__ mean,
                                                        const uint32_t* __restrict__ row_mask, float* __restrict__ part,
                                                        int64_t* __restrict__ pcount, int dpad, int ntile) {
    constexpr int E = Elems<T>::E;
    constexpr bool F16 = E == 8;
    constexpr int NT = F16 ? 2 : 4;  // values of t this wave holds
    constexpr int NU = E;
    constexpr int GF = 16 * E;  // features of a 256-byte group
    __shared__ int cnt_sh;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, rr = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * GR_CHUNK;
    const int64_t pend = p0 + GR_CHUNK < npad ? p0 + GR_CHUNK : npad;

    if (blockIdx.y == 0) {  // the chunk's live rows (integers: any order)
        if (tid == 0) cnt_sh = 0;
        __syncthreads();
        int cnt = 0;
        for (int64_t w = (p0 >> 5) + tid; w < (pend >> 5); w += 256) {
            const int64_t left = n - w * 32;
            if (left <= 0) break;
            const uint32_t valid = left >= 32 ? 0xffffffffu : ((1u << (int)left) - 1u);
            cnt += __popc((row_mask ? row_mask[w] : 0xffffffffu) & valid);
        }
        if (cnt) atomicAdd(&cnt_sh, cnt);
        __syncthreads();
        if (tid == 0) pcount[blockIdx.x] = cnt_sh;
    }

    // tile (ti, tj), ti <= tj, of the upper triangle
    int ti = 0, rem = blockIdx.y;
    while (rem >= ntile - ti) {
        rem -= ntile - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int ga = F16 ? ti : 2 * ti + (wave >> 1);
    const int gb = F16 ? tj : 2 * tj + (wave & 1);
    const int t0 = F16 ? 2 * wave : 0;
    const int ksa = 2 * ga + (c >> 3), ksb = 2 * gb + (c >> 3);
    const bool oka = ksa < ks, okb = ksb < ks;
    float ma[NT], mb[NU];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int f = ga * GF + c * E + t0 + t;
        ma[t] = f < d ? mean[f] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int f = gb * GF + c * E + u;
        mb[u] = f < d ? mean[f] : 0.f;
    }

    f32x4 acc[NT][NU];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};

    // 16 rows an iteration: row 4 j + rr of them is this lane's in the j-th group of MFMAs
    auto load = [&](int64_t pb, u32x4(&av)[4], u32x4(&bv)[4], unsigned& lv) {
        lv = 0;
        const size_t tile_base = (size_t)(pb >> 8) * ks * ISC_TILE_KSTEP_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t p = pb + 4 * j + rr;
            const bool live = live_bit(row_mask, p, n);
            av[j] = u32x4{0u, 0u, 0u, 0u};
            bv[j] = u32x4{0u, 0u, 0u, 0u};
            if (live) {
                lv |= 1u << j;
                const size_t in_tile = (size_t)(p & 255) * ISC_KSTEP_BYTES + (size_t)(c & 7) * 16;
                if (oka) av[j] = *reinterpret_cast<const u32x4*>(bank + tile_base + (size_t)ksa * ISC_TILE_KSTEP_BYTES + in_tile);
                if (okb) bv[j] = *reinterpret_cast<const u32x4*>(bank + tile_base + (size_t)ksb * ISC_TILE_KSTEP_BYTES + in_tile);
            }
        }
    };

    u32x4 ra[4], rb[4];
    unsigned lv = 0;
    if (p0 < pend) load(p0, ra, rb, lv);
    for (int64_t pb = p0; pb < pend; pb += 16) {
        u32x4 na[4], nb[4];
        unsigned nlv = 0;
        const bool more = pb + 16 < pend;
        if (more) load(pb + 16, na, nb, nlv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool live = (lv >> j) & 1u;
            float a[NT], b[NU];
#pragma unroll
            for (int t = 0; t < NT; ++t) a[t] = live ? Elems<T>::get(ra[j], t0 + t) - ma[t] : 0.f;
#pragma unroll
            for (int u = 0; u < NU; ++u) b[u] = live ? Elems<T>::get(rb[j], u) - mb[u] : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int u = 0; u < NU; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[u], acc[t][u], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ra[j] = na[j];
                rb[j] = nb[j];
            }
            lv = nlv;
        }
    }

    // accumulator register `reg` of lane (c, rr): feature E (4 rr + reg) + t of group A by feature E c + u of group B
    float* dst = part + (size_t)blockIdx.x * dpad * dpad;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = ga * GF + E * (4 * rr + reg) + t0 + t;
            float* row = dst + (size_t)i * dpad + gb * GF + E * c;
#pragma unroll
            for (int u = 0; u < NU; ++u) row[u] = acc[t][u][reg];
        }
}

__global__ __launch_bounds__(256) void k_bank_gram_reduce(const float* __restrict__ part, const int64_t* __restrict__ pcount,
                                                          int64_t chunks, int dpad, int d, double* __restrict__ gram,
                                                          int64_t ld, int64_t* __restrict__ count) {
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4);
    const int j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        int64_t cnt = 0;
        for (int64_t ch = 0; ch < chunks; ++ch) cnt += pcount[ch];
        count[0] = cnt;
    }
    if (i >= d || j >= d) return;
    const int lo = i < j ? i : j, hi = i < j ? j : i;  // the upper triangle holds the value of both
    const float* src = part + (size_t)lo * dpad + hi;
    double acc = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) acc += (double)src[(size_t)ch * dpad * dpad];
    gram[(int64_t)i * ld + j] = acc;
}

struct GramWs {
    float* part;      // [chunks][dpad][dpad]
    int64_t* pcount;  // [chunks] live rows of the chunk
    int64_t chunks;
    int dpad;
    size_t bytes;
};
GramWs gram_carve(void* base, int64_t n, int d) {
    GramWs w{};
    const int64_t npad = isc_ceil_div<int64_t>(n, ISC_TILE_ROWS) * ISC_TILE_ROWS;
    w.chunks = isc_ceil_div<int64_t>(npad, GR_CHUNK);
    w.dpad = isc_ceil_div(d, GR_TILE) * GR_TILE;
    const size_t pb = (size_t)w.chunks * w.dpad * w.dpad * sizeof(float);  // a multiple of 256
    w.part = static_cast<float*>(base);
    w.pcount = base ? reinterpret_cast<int64_t*>(static_cast<unsigned char*>(base) + pb) : nullptr;
    w.bytes = pb + isc_align_up((size_t)w.chunks * sizeof(int64_t), 256);
    return w;
}

bool pca_dtype_ok(int dtype) { return dtype == ISC_F16 || dtype == ISC_F32; }

// ---- projection -----------------------------------------------------------------------------------------------------------
constexpr int PJ_MEAN = PCA_MAX_D;  // floats of the staged mean: D <= 2048 covers every K step of either dtype

__host__ __device__ inline int proj_ld(int k) { return (k + 15) / 16 * 16 + 4; }  // floats per row of the LDS image

template <typename T, typename TOUT, int MB>
__global__ __launch_bounds__(256) void k_bank_project(const unsigned char* __restrict__ bank, int ks, int d, IscPerm pm,
                                                      const float* __restrict__ mean, const float* __restrict__ w, int k,
                                                      int64_t ldw, const uint32_t* __restrict__ row_mask,
                                                      float* __restrict__ out_rows, int64_t ldo,
                                                      unsigned char* __restrict__ out_packed, int ks_out, int normalize,
                                                      float eps, unsigned* __restrict__ norm_bound) {
    constexpr int E = Elems<T>::E;
    constexpr int EPK = ISC_KSTEP_BYTES / (int)sizeof(T);
    constexpr int RB = 16 * MB;
    extern __shared__ __attribute__((aligned(16))) float p_lds[];  // [RB][kp]
    __shared__ float mean_sh[PJ_MEAN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, q = lane >> 4;
    const int kp = proj_ld(k);
    const int64_t base = (int64_t)blockIdx.x * RB;
    for (int e = tid; e < ks * EPK; e += 256) mean_sh[e] = e < d ? mean[e] : 0.f;
    __syncthreads();

    bool live[MB];
    const unsigned char* src[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int64_t p = base + mb * 16 + row;
        live[mb] = live_bit(row_mask, p, pm.n);
        src[mb] = bank + (size_t)(p >> 8) * ks * ISC_TILE_KSTEP_BYTES + (size_t)(p & 255) * ISC_KSTEP_BYTES + q * 16;
    }

    for (int cb = wave; cb * 16 < k; cb += 4) {
        const int col = cb * 16 + row;  // this lane's column of w (the B operand's j = lane & 15)
        const bool col_ok = col < k;
        f32x4 acc[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto load = [&](int s, u32x4(&av)[MB][2], float(&bv)[2][E]) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    av[mb][h] = u32x4{0u, 0u, 0u, 0u};
                    if (live[mb]) av[mb][h] = *reinterpret_cast<const u32x4*>(src[mb] + (size_t)s * ISC_TILE_KSTEP_BYTES + h * 64);
                }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int t = 0; t < E; ++t) {
                    const int f = s * EPK + E * (4 * h + q) + t;
                    bv[h][t] = (col_ok && f < d) ? w[(int64_t)f * ldw + col] : 0.f;
                }
        };
        u32x4 a[MB][2];
        float b[2][E];
        load(0, a, b);
        for (int s = 0; s < ks; ++s) {
            u32x4 an[MB][2];
            float bn[2][E];
            if (s + 1 < ks) load(s + 1, an, bn);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float* mp = mean_sh + s * EPK + E * (4 * h + q);
#pragma unroll
                for (int t = 0; t < E; ++t) {
                    const float m = mp[t];
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Elems<T>::get(a[mb][h], t) - m, b[h][t], acc[mb], 0, 0, 0);
                }
            }
            if (s + 1 < ks) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int h = 0; h < 2; ++h) a[mb][h] = an[mb][h];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int t = 0; t < E; ++t) b[h][t] = bn[h][t];
            }
        }
        // accumulator register `reg` of lane (row, q): bank row 4 q + reg of the block, column `col`
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) p_lds[(mb * 16 + 4 * q + reg) * kp + col] = acc[mb][reg];
    }
    __syncthreads();

    for (int r = wave; r < RB; r += 4) {
        const int64_t p = base + r;
        if (p >= pm.n) break;
        const bool alive = live_bit(row_mask, p, pm.n);
        const float* pr = p_lds + r * kp;
        if (out_rows) {
            float* dst = out_rows + isc_perm_orig(pm, p) * ldo;
            for (int e = lane; e < k; e += 64) dst[e] = alive ? pr[e] : 0.f;
        }
        if (out_packed && alive) isc_pack_row<float, TOUT>(pr, k, p, normalize, eps, out_packed, ks_out, norm_bound, lane);
    }
}

template <typename T, typename TOUT, int MB>
int project_launch(const unsigned char* bank, int ks, int d, const IscPerm& pm, const float* mean, const float* w, int k,
                   int64_t ldw, const uint32_t* row_mask, float* out_rows, int64_t ldo, unsigned char* out_packed,
                   int ks_out, int normalize, float eps, float* norm_bound, hipStream_t stream) {
    const size_t lds = (size_t)16 * MB * proj_ld(k) * sizeof(float);
    if (lds > 64 * 1024) {  // more than 64 KiB of dynamic LDS needs the opt-in, once per kernel and device
        static unsigned long long attr_done = 0ull;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return ISC_ERR_NO_DEVICE;
        const bool tracked = dev >= 0 && dev < 64;
        if (!tracked || !((__atomic_load_n(&attr_done, __ATOMIC_RELAXED) >> dev) & 1ull)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bank_project<T, TOUT, MB>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    16 * proj_ld(PCA_MAX_D) * (int)sizeof(float)) != hipSuccess) {
                (void)hipGetLastError();
                return ISC_ERR_UNSUPPORTED;
            }
            if (tracked) __atomic_fetch_or(&attr_done, 1ull << dev, __ATOMIC_RELAXED);
        }
    }
    const int64_t npad = isc_ceil_div<int64_t>(pm.n, ISC_TILE_ROWS) * ISC_TILE_ROWS;
    hipLaunchKernelGGL((k_bank_project<T, TOUT, MB>), dim3((unsigned)(npad / (16 * MB))), dim3(256), lds, stream, bank, ks, d,
                       pm, mean, w, k, ldw, row_mask, out_rows, ldo, out_packed, ks_out, normalize, eps,
                       reinterpret_cast<unsigned*>(norm_bound));
    return isc_launch_status();
}

// rows per workgroup: the most whose LDS image [16 MB][K] stays within 64 KiB; a wider K keeps 16 rows (up to 129 KiB)
template <typename T, typename TOUT, typename... A>
int project_rows(int k, A... args) {
    const int kp = proj_ld(k);
    if (64 * kp * 4 <= 64 * 1024) return project_launch<T, TOUT, 4>(args...);
    if (32 * kp * 4 <= 64 * 1024) return project_launch<T, TOUT, 2>(args...);
    return project_launch<T, TOUT, 1>(args...);
}

}  // namespace

extern "C" int isc_bank_gram_chunk_rows(void) { return GR_CHUNK; }

extern "C" int isc_bank_gram_workspace_bytes(int dtype, int64_t N, int D, size_t* bytes) {
    ISC_REQUIRE(bytes != nullptr && pca_dtype_ok(dtype) && D > 0 && N >= 0 && N <= 0x7ffffffe);
    if (D > PCA_MAX_D) return ISC_ERR_UNSUPPORTED;
    *bytes = gram_carve(nullptr, N, D).bytes;
    return ISC_OK;
}

extern "C" int isc_bank_gram(const void* bank, int dtype, int64_t N, int D, const float* mean, const uint32_t* row_mask,
                             double* gram, int64_t ld, int64_t* count, void* workspace, size_t workspace_bytes,
                             void* stream) {
    ISC_REQUIRE(pca_dtype_ok(dtype) && D > 0 && N >= 0 && N <= 0x7ffffffe);
    if (D > PCA_MAX_D) return ISC_ERR_UNSUPPORTED;
    ISC_REQUIRE(ld >= D);
    if (N == 0) return ISC_OK;
    ISC_REQUIRE(bank && mean && gram && count && workspace);
    if (!isc_aligned(bank, 16) || !isc_aligned(mean, 4) || !isc_aligned(row_mask, 4) || !isc_aligned(gram, 8) ||
        !isc_aligned(count, 8) || !isc_aligned(workspace, 256))
        return ISC_ERR_ALIGNMENT;
    const GramWs w = gram_carve(workspace, N, D);
    if (workspace_bytes < w.bytes) return ISC_ERR_WORKSPACE;
    hipStream_t s = isc_stream(stream);
    const unsigned char* bytes = static_cast<const unsigned char*>(bank);
    const int64_t npad = isc_ceil_div<int64_t>(N, ISC_TILE_ROWS) * ISC_TILE_ROWS;
    const int ntile = w.dpad / GR_TILE;
    const dim3 grid((unsigned)w.chunks, (unsigned)(ntile * (ntile + 1) / 2));
    if (dtype == ISC_F16)
        hipLaunchKernelGGL(k_bank_gram_part<_Float16>, grid, dim3(256), 0, s, bytes, isc_ksteps(D, 2), D, N, npad, mean,
                           row_mask, w.part, w.pcount, w.dpad, ntile);
    else
        hipLaunchKernelGGL(k_bank_gram_part<float>, grid, dim3(256), 0, s, bytes, isc_ksteps(D, 4), D, N, npad, mean,
                           row_mask, w.part, w.pcount, w.dpad, ntile);
    const unsigned rb = (unsigned)isc_ceil_div(D, 16);
    hipLaunchKernelGGL(k_bank_gram_reduce, dim3(rb, rb), dim3(256), 0, s, w.part, w.pcount, w.chunks, w.dpad, D, gram, ld,
                       count);
    return isc_launch_status();
}

extern "C" int isc_bank_project(const void* bank, int dtype, int64_t N, int D, const float* mean, const float* w, int K,
                                int64_t ldw, const uint32_t* row_mask, float* out_rows, int64_t ldo, void* out_packed,
                                int out_dtype, int normalize, float eps, float* norm_bound, void* stream) {
    ISC_REQUIRE(pca_dtype_ok(dtype) && D > 0 && N >= 0 && N <= 0x7ffffffe);
    if (D > PCA_MAX_D) return ISC_ERR_UNSUPPORTED;
    ISC_REQUIRE(K > 0 && K <= D && ldw >= K);
    ISC_REQUIRE(out_rows || out_packed);
    ISC_REQUIRE(!out_rows || ldo >= K);
    ISC_REQUIRE(!out_packed || pca_dtype_ok(out_dtype));
    if (N == 0) return ISC_OK;
    ISC_REQUIRE(bank && mean && w);
    if (!isc_aligned(bank, 16) || !isc_aligned(mean, 4) || !isc_aligned(w, 4) || !isc_aligned(row_mask, 4) ||
        !isc_aligned(out_rows, 4) || !isc_aligned(out_packed, 16) || !isc_aligned(norm_bound, 4))
        return ISC_ERR_ALIGNMENT;
    hipStream_t s = isc_stream(stream);
    const unsigned char* bytes = static_cast<const unsigned char*>(bank);
    unsigned char* outp = static_cast<unsigned char*>(out_packed);
    const IscPerm pm = isc_make_perm(N);
    const bool out16 = out_packed && out_dtype == ISC_F16;
    const int ks_out = isc_ksteps(K, out16 ? 2 : 4);
#define ISC_PROJECT(T_, TOUT_)                                                                                          \
    return project_rows<T_, TOUT_>(K, bytes, isc_ksteps(D, (int)sizeof(T_)), D, pm, mean, w, K, ldw, row_mask, out_rows, \
                                   ldo, outp, ks_out, normalize, eps, norm_bound, s)
    if (dtype == ISC_F16) {
        if (out16) ISC_PROJECT(_Float16, _Float16);
        ISC_PROJECT(_Float16, float);
    }
    if (out16) ISC_PROJECT(float, _Float16);
    ISC_PROJECT(float, float);
#undef ISC_PROJECT
}
