// Patch-token output of the ViT encoder (include/imagescry_hip.h: isc_vit_pos_resample, isc_vit_pos_resample_aa,
// isc_vit_tokens_out, isc_vit_tokens_out_skip, isc_tokens_to_map): the position table of an h x w token grid, and the head that turns the residual stream into the channels-first
// embedding map [B, D, h, w] every other embedder returns.
#include "aa_filter.h"
#include "isc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------
// Bicubic resampling of the g x g patch rows of a position table to h x w (torch upsample_bicubic2d, align_corners =
// False, no antialias): A = -0.75, source coordinate (dst + 0.5) * g / h - 0.5, tap indices clamped to the table.
// Row 0 (the class token) is copied.  One thread per (output row, four channels); runs once per grid.
__device__ __forceinline__ void cubic_taps(int dst, float scale, int n, int (&idx)[4], float (&wgt)[4]) {
    constexpr float A = -0.75f;
    const float src = scale * ((float)dst + 0.5f) - 0.5f;
    const float fl = floorf(src);
    const float t = src - fl;
    const int i0 = (int)fl;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    wgt[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    wgt[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    wgt[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    wgt[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(i0 - 1 + k, 0), n - 1);
}

__global__ __launch_bounds__(256) void k_vit_pos_resample(const float* __restrict__ pos, int g, int h, int w, int D,
                                                          float scale_h, float scale_w, float* __restrict__ out) {
    const int dv = D >> 2;
    const int total = (1 + h * w) * dv;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = i % dv;
    const int row = i / dv;
    if (row == 0) {
        *reinterpret_cast<f32x4*>(out + 4 * c) = *reinterpret_cast<const f32x4*>(pos + 4 * c);
        return;
    }
    const int oy = (row - 1) / w, ox = (row - 1) - oy * w;
    int iy[4], ix[4];
    float wy[4], wx[4];
    cubic_taps(oy, scale_h, g, iy, wy);
    cubic_taps(ox, scale_w, g, ix, wx);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        f32x4 line = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 4; ++b)
            line += wx[b] * *reinterpret_cast<const f32x4*>(pos + (size_t)(1 + iy[a] * g + ix[b]) * D + 4 * c);
        acc += wy[a] * line;
    }
    *reinterpret_cast<f32x4*>(out + (size_t)row * D + 4 * c) = acc;
}

// ---------------------------------------------------------------------------------------------------------
// The ANTIALIASED form (torch _upsample_bicubic2d_aa, align_corners = False): the filter of aa_filter.h (cubic_aa, AaTaps)
// on both axes of the table.
// One thread per (output row, four channels), rows of the source first (as the separable passes of torch go), runs
// once per grid: up to g x g taps a thread.
__global__ __launch_bounds__(256) void k_vit_pos_resample_aa(const float* __restrict__ pos, int g, int h, int w, int D,
                                                             float scale_h, float scale_w, float* __restrict__ out) {
    const int dv = D >> 2;
    const int total = (1 + h * w) * dv;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = i % dv;
    const int row = i / dv;
    if (row == 0) {
        *reinterpret_cast<f32x4*>(out + 4 * c) = *reinterpret_cast<const f32x4*>(pos + 4 * c);
        return;
    }
    const int oy = (row - 1) / w, ox = (row - 1) - oy * w;
    const AaTaps ty(oy, scale_h, g), tx(ox, scale_w, g);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < ty.n; ++a) {
        f32x4 line = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < tx.n; ++b)
            line += tx.weight(b) * *reinterpret_cast<const f32x4*>(pos + (size_t)(1 + (ty.lo + a) * g + tx.lo + b) * D + 4 * c);
        acc += ty.weight(a) * line;
    }
    *reinterpret_cast<f32x4*>(out + (size_t)row * D + 4 * c) = acc;
}

// ---------------------------------------------------------------------------------------------------------
// out[b][e][t - skip] = normalize?( LayerNorm(tokens[b][t]) )[e] for the patch tokens t = skip .. T - 1 of every image
// (skip = the rows in front of the patches: the class token and any register tokens).
//
// A workgroup owns a tile of 32 consecutive cells of one image and all D channels of them:
//   phase 1  LayerNorm, one wave per token (k_layernorm's arithmetic: the same lane -> channel map, the same two passes
//            over registers), four tokens per wave, all their loads requested before the first is used; the result goes
//            to LDS as [channel / 4][cell][4] -- a lane's four channels are one 16-byte store, rows padded by 16 bytes so
//            that the eight lanes of a store group (528 bytes apart) fall on eight different slots; without LN
//            (isc_tokens_to_map: rows that are final already, a projection's output) the loaded row goes to LDS as it is;
//            a third copy of that arithmetic (vit.hip: k_layernorm, layernorm_row) -- change them together:
//            tests/test_gpu_vit_tokens_exact.py holds the un-normalised map to the bits isc_layernorm gives on the same
//            rows, for every NV, with and without a partly empty last lane row;
//   phase 2  (normalize) the arithmetic of k_l2norm_spatial, bit for bit: per cell four partial sums of squares over the
//            channels e = g, g + 4, ... in ascending order, denominator max(sqrt(r0 + r1 + r2 + r3), eps) (the same test
//            file: the bits of isc_l2norm_channels on the un-normalised map);
//   phase 3  the transposed store: a 32-lane half of a wave reads four channels of 32 consecutive cells (one 16-byte LDS
//            read per lane, consecutive slots) and writes, per channel, 32 consecutive floats -- 128 contiguous bytes of
//            the channels-first map.  (A store per token would put 4-byte elements (T - 1) * 4 bytes apart.)
constexpr int TO_CELLS = 32;
constexpr int TO_THREADS = 512;
constexpr int TO_WAVES = TO_THREADS / 64;
constexpr int TO_TOKENS = TO_CELLS / TO_WAVES;  // tokens per wave
constexpr int TO_PITCH = TO_CELLS * 4 + 4;      // floats per LDS row (four channels of 32 cells + 16 bytes)
constexpr int TO_MAX_D = 1024;
constexpr int TO_MAX_LDS = (TO_MAX_D / 4) * TO_PITCH * 4 + TO_CELLS * 4;

template <int NV, bool LN = true>
__global__ __launch_bounds__(TO_THREADS) void k_vit_tokens_out(const float* __restrict__ tokens, int T, int D,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int normalize,
                                                               float l2_eps, float* __restrict__ out, int tiles,
                                                               int skip) {
    extern __shared__ __attribute__((aligned(16))) float to_lds[];
    const int nvec = D >> 2;
    float* const tile = to_lds;                     // [nvec][TO_PITCH]
    float* const denom = to_lds + nvec * TO_PITCH;  // [TO_CELLS]
    const int b = blockIdx.x / tiles;
    const int c0 = (blockIdx.x - b * tiles) * TO_CELLS;
    const int cells = T - skip;
    const int ncell = min(TO_CELLS, cells - c0);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // ---- phase 1
    f32x4 v[TO_TOKENS][NV];
#pragma unroll
    for (int k = 0; k < TO_TOKENS; ++k) {
        const int j = wave + TO_WAVES * k;
        const float* xr = tokens + ((size_t)b * T + skip + c0 + min(j, ncell - 1)) * D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            v[k][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < ncell && c < nvec) v[k][i] = *reinterpret_cast<const f32x4*>(xr + 4 * c);
        }
    }
#pragma unroll
    for (int k = 0; k < TO_TOKENS; ++k) {
        const int j = wave + TO_WAVES * k;
        if (j >= ncell) continue;  // wave-uniform
        if (!LN) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = lane + 64 * i;
                if (c < nvec) *reinterpret_cast<f32x4*>(tile + c * TO_PITCH + j * 4) = v[k][i];
            }
            continue;
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += (v[k][i][0] + v[k][i][1]) + (v[k][i][2] + v[k][i][3]);
        const float mean = isc_wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nvec) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = v[k][i][r] - mean;
                    q += d * d;
                }
            }
        }
        const float rstd = 1.f / sqrtf(isc_wave_sum(q) / (float)D + eps);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c >= nvec) continue;
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + 4 * c);
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (v[k][i][r] - mean) * rstd * g[r] + bt[r];
            *reinterpret_cast<f32x4*>(tile + c * TO_PITCH + j * 4) = o;
        }
    }
    __syncthreads();

    // ---- phase 2: thread 4 * cell + g sums the squares of channels g, g + 4, ... of its cell
    if (normalize) {
        if (tid < TO_CELLS * 4) {  // waves 0 and 1, whole
            const int cell = tid >> 2;
            float acc = 0.f;
            if (cell < ncell)
                for (int c = 0; c < nvec; ++c) {
                    const float x = tile[c * TO_PITCH + tid];
                    acc += x * x;
                }
            const int l0 = lane & ~3;
            const float r0 = __shfl(acc, l0, 64), r1 = __shfl(acc, l0 + 1, 64), r2 = __shfl(acc, l0 + 2, 64),
                        r3 = __shfl(acc, l0 + 3, 64);
            if ((tid & 3) == 0) denom[cell] = fmaxf(sqrtf(r0 + r1 + r2 + r3), l2_eps);
        }
        __syncthreads();
    }

    // ---- phase 3
    const int cell = tid & (TO_CELLS - 1);
    if (cell >= ncell) return;
    const float dn = normalize ? denom[cell] : 1.f;
    float* const obase = out + (size_t)b * D * cells + c0 + cell;
#pragma unroll 4
    for (int c = tid >> 5; c < nvec; c += TO_THREADS / TO_CELLS) {
        f32x4 o = *reinterpret_cast<const f32x4*>(tile + c * TO_PITCH + cell * 4);
        if (normalize) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = __fdiv_rn(o[r], dn);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) obase[(size_t)(4 * c + r) * cells] = o[r];
    }
}

// more than 64 KiB of dynamic LDS has to be allowed once per (instantiation, device)
bool tokens_out_prepare(const void* fn, unsigned long long* done) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const bool tracked = dev >= 0 && dev < 64;
    if (tracked && ((__atomic_load_n(done, __ATOMIC_RELAXED) >> dev) & 1ull)) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, TO_MAX_LDS) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (tracked) __atomic_fetch_or(done, 1ull << dev, __ATOMIC_RELAXED);
    return true;
}

}  // namespace

extern "C" int isc_vit_pos_resample(const float* pos_embed, int g, int h, int w, int D, float* out, void* stream) {
    ISC_REQUIRE(pos_embed && out && g > 0 && h > 0 && w > 0 && D > 0);
    if (D % 4 != 0) return ISC_ERR_UNSUPPORTED;
    if ((long long)g * g >= (1 << 24) || (long long)h * w >= (1 << 24) || (1ll + (long long)h * w) * (D / 4) > 0x7fffffffLL)
        return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(pos_embed, 16) || !isc_aligned(out, 16)) return ISC_ERR_ALIGNMENT;
    const int total = (1 + h * w) * (D / 4);
    hipLaunchKernelGGL(k_vit_pos_resample, dim3(isc_ceil_div(total, 256)), dim3(256), 0, isc_stream(stream), pos_embed, g,
                       h, w, D, (float)g / (float)h, (float)g / (float)w, out);
    return isc_launch_status();
}

extern "C" int isc_vit_pos_resample_aa(const float* pos_embed, int g, int h, int w, int D, float* out, void* stream) {
    ISC_REQUIRE(pos_embed && out && g > 0 && h > 0 && w > 0 && D > 0);
    if (D % 4 != 0) return ISC_ERR_UNSUPPORTED;
    if ((long long)g * g >= (1 << 24) || (long long)h * w >= (1 << 24) || (1ll + (long long)h * w) * (D / 4) > 0x7fffffffLL)
        return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(pos_embed, 16) || !isc_aligned(out, 16)) return ISC_ERR_ALIGNMENT;
    const int total = (1 + h * w) * (D / 4);
    hipLaunchKernelGGL(k_vit_pos_resample_aa, dim3(isc_ceil_div(total, 256)), dim3(256), 0, isc_stream(stream), pos_embed,
                       g, h, w, D, (float)g / (float)h, (float)g / (float)w, out);
    return isc_launch_status();
}

// LN: gamma / beta / eps are LayerNorm's; without it they are not looked at (nullptr, nullptr, 0)
template <bool LN>
static int tokens_out_launch(const float* tokens, int B, int T, int skip, int D, const float* gamma, const float* beta,
                             float eps, int normalize, float l2_eps, float* out, void* stream) {
    ISC_REQUIRE(tokens && out && B > 0 && skip >= 1 && T > skip && D > 0 && l2_eps >= 0.f);
    if (LN) ISC_REQUIRE(gamma && beta && eps >= 0.f);
    if (D % 4 != 0 || D > TO_MAX_D) return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(tokens, 16) || !isc_aligned(out, 16)) return ISC_ERR_ALIGNMENT;
    if (LN && (!isc_aligned(gamma, 16) || !isc_aligned(beta, 16))) return ISC_ERR_ALIGNMENT;
    const int tiles = isc_ceil_div(T - skip, TO_CELLS);
    if ((long long)B * tiles > 0x7fffffffLL) return ISC_ERR_UNSUPPORTED;
    const int nv = (D / 4 + 63) / 64;
    const size_t lds = (size_t)(D / 4) * TO_PITCH * 4 + TO_CELLS * 4;
#define ISC_TO_LAUNCH(NV_)                                                                                          \
    do {                                                                                                            \
        auto kern = k_vit_tokens_out<NV_, LN>;                                                                      \
        static unsigned long long attr_done = 0;                                                                    \
        if (!tokens_out_prepare(reinterpret_cast<const void*>(kern), &attr_done)) return ISC_ERR_UNSUPPORTED;       \
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * tiles)), dim3(TO_THREADS), lds, isc_stream(stream), tokens, T, D, \
                           gamma, beta, eps, normalize ? 1 : 0, l2_eps, out, tiles, skip);                          \
    } while (0)
    if (nv <= 1) ISC_TO_LAUNCH(1);
    else if (nv <= 2) ISC_TO_LAUNCH(2);
    else if (nv <= 3) ISC_TO_LAUNCH(3);
    else ISC_TO_LAUNCH(4);
#undef ISC_TO_LAUNCH
    return isc_launch_status();
}

extern "C" int isc_vit_tokens_out_skip(const float* tokens, int B, int T, int skip, int D, const float* gamma,
                                       const float* beta, float eps, int normalize, float l2_eps, float* out,
                                       void* stream) {
    return tokens_out_launch<true>(tokens, B, T, skip, D, gamma, beta, eps, normalize, l2_eps, out, stream);
}

extern "C" int isc_tokens_to_map(const float* tokens, int B, int T, int skip, int D, int normalize, float l2_eps,
                                 float* out, void* stream) {
    return tokens_out_launch<false>(tokens, B, T, skip, D, nullptr, nullptr, 0.f, normalize, l2_eps, out, stream);
}

extern "C" int isc_vit_tokens_out(const float* tokens, int B, int T, int D, const float* gamma, const float* beta,
                                  float eps, int normalize, float l2_eps, float* out, void* stream) {
    return isc_vit_tokens_out_skip(tokens, B, T, 1, D, gamma, beta, eps, normalize, l2_eps, out, stream);
}
