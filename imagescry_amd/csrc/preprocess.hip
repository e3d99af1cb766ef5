// Preprocess kernels: batch-statistics normalisation, bilinear resize, L2 normalisation.
// All three are HBM-bound byte/float streams; they are written for coalesced 16-byte lanes,
// not for the matrix cores.  Reference arithmetic: src/imagescry/image/transforms.py:58-126 and
// src/imagescry/models/embedding.py:74.
#include "aa_filter.h"
#include "bilinear_tap.h"
#include "isc_common.h"

namespace {

constexpr int kStatsThreads = 256;
constexpr int kStatsChunk = 16384;  // elements of one plane handled by one workgroup

struct StatPartial {
    double s;   // sum x      (exact integer value for u8 input)
    double ss;  // sum x * x
};

// One workgroup reduces one chunk of one (b, c) plane.  u8 pixels are summed as integers (v_dot4_u32_u8),
// so the partials -- and therefore mean / std -- do not depend on the launch geometry.
__global__ __launch_bounds__(kStatsThreads) void k_stats_partial_u8(const uint8_t* __restrict__ x, int C, int HW,
                                                                    int chunks_per_plane, StatPartial* __restrict__ part,
                                                                    int items_per_channel, int vec_ok) {
    const int item = blockIdx.x;  // (b, chunk)
    const int c = blockIdx.y;
    const int b = item / chunks_per_plane;
    const int chunk = item - b * chunks_per_plane;
    const int begin = chunk * kStatsChunk;
    const int end = min(HW, begin + kStatsChunk);
    const uint8_t* p = x + ((size_t)b * C + c) * HW;
    unsigned s = 0, ss = 0;  // <= 64 * 65025 per thread: no overflow
    if (vec_ok) {
        for (int i = begin + threadIdx.x * 16; i < end; i += kStatsThreads * 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + i);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s = __builtin_amdgcn_udot4(w[j], 0x01010101u, s, false);
                ss = __builtin_amdgcn_udot4(w[j], w[j], ss, false);
            }
        }
    } else {
        for (int i = begin + threadIdx.x; i < end; i += kStatsThreads) {
            const unsigned v = p[i];
            s += v;
            ss += v * v;
        }
    }
    unsigned long long s64 = isc_wave_sum((unsigned long long)s);
    unsigned long long ss64 = isc_wave_sum((unsigned long long)ss);
    __shared__ unsigned long long red[2][kStatsThreads / ISC_WAVE];
    const int wave = threadIdx.x / ISC_WAVE;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = s64;
        red[1][wave] = ss64;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0, q = 0;
        for (int w = 0; w < kStatsThreads / ISC_WAVE; ++w) {
            a += red[0][w];
            q += red[1][w];
        }
        part[(size_t)c * items_per_channel + item] = StatPartial{(double)a, (double)q};
    }
}

__global__ __launch_bounds__(kStatsThreads) void k_stats_partial_f32(const float* __restrict__ x, int C, int HW,
                                                                     int chunks_per_plane, StatPartial* __restrict__ part,
                                                                     int items_per_channel, int vec_ok) {
    const int item = blockIdx.x;
    const int c = blockIdx.y;
    const int b = item / chunks_per_plane;
    const int chunk = item - b * chunks_per_plane;
    const int begin = chunk * kStatsChunk;
    const int end = min(HW, begin + kStatsChunk);
    const float* p = x + ((size_t)b * C + c) * HW;
    double s = 0.0, ss = 0.0;
    if (vec_ok) {
        for (int i = begin + threadIdx.x * 4; i < end; i += kStatsThreads * 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + i);
            s += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
            ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    } else {
        for (int i = begin + threadIdx.x; i < end; i += kStatsThreads) {
            const double v = p[i];
            s += v;
            ss += v * v;
        }
    }
    s = isc_wave_sum(s);
    ss = isc_wave_sum(ss);
    __shared__ double red[2][kStatsThreads / ISC_WAVE];
    const int wave = threadIdx.x / ISC_WAVE;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = s;
        red[1][wave] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, q = 0;
        for (int w = 0; w < kStatsThreads / ISC_WAVE; ++w) {
            a += red[0][w];
            q += red[1][w];
        }
        part[(size_t)c * items_per_channel + item] = StatPartial{a, q};
    }
}

// One workgroup per channel: fixed-order sum of the partials, then mean and unbiased std in float64.
// `integer_data` (the u8 path): a = sum x and q = sum x^2 are exact integers, and q - a * a / n would cancel once a * a
// passes 2^53 (a near-constant batch: std 17 float32 ulp off at 8 x 224 x 224 pixels of 255 and one of 254).  The sums
// are therefore shifted by the integer m0 = rint(a / n) first: S1 = sum (x - m0) = a - n m0 and S2 = sum (x - m0)^2 =
// q - m0 (a + S1) are again exact integers in float64 (n < 2^36), |S1| <= n / 2, and S2 >= |S1| >= 2 S1^2 / n for
// integer deviations, so S2 - S1^2 / n loses at most one bit.  The float32 path keeps the plain formula: its partial
// sums are not integers, and its error is bounded in tests/preprocess_exact.py instead.
__global__ __launch_bounds__(kStatsThreads) void k_stats_final(const StatPartial* __restrict__ part, int items_per_channel,
                                                               double n, int integer_data, float* __restrict__ mean,
                                                               float* __restrict__ stdev) {
    const int c = blockIdx.x;
    double s = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < items_per_channel; i += kStatsThreads) {
        const StatPartial p = part[(size_t)c * items_per_channel + i];
        s += p.s;
        ss += p.ss;
    }
    s = isc_wave_sum(s);
    ss = isc_wave_sum(ss);
    __shared__ double red[2][kStatsThreads / ISC_WAVE];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x / ISC_WAVE] = s;
        red[1][threadIdx.x / ISC_WAVE] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, q = 0;
        for (int w = 0; w < kStatsThreads / ISC_WAVE; ++w) {
            a += red[0][w];
            q += red[1][w];
        }
        const double m = a / n;
        if (integer_data) {
            const double m0 = rint(m);
            const double s1 = a - n * m0;
            q -= m0 * (a + s1);
            a = s1;
        }
        double var = (q - a * a / n) / (n - 1.0);  // n == 1 -> NaN, as torch's unbiased std
        if (var < 0.0) var = 0.0;
        mean[c] = (float)m;
        stdev[c] = (float)sqrt(var);
    }
}

__device__ __forceinline__ float norm_clip(float v, float mu, float denom, float lo, float hi) {
    const float r = __fdiv_rn(v - mu, denom);
    return r != r ? r : fminf(fmaxf(r, lo), hi);
}

// 16 pixels per lane: one 16-byte load, four 16-byte stores.  Requires HW % 16 == 0 so a vector never
// straddles two planes (224*224 = 16 * 3136).
__global__ __launch_bounds__(256) void k_normalize_u8_vec16(const uint8_t* __restrict__ x, size_t nvec, int C, int HW,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ stdev, int per_image, float eps,
                                                            float lo, float hi, float* __restrict__ y) {
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t e = v * 16;
        const size_t plane = e / HW;
        const int st = per_image ? (int)plane : (int)(plane % C);
        const float mu = mean[st];
        const float denom = stdev[st] + eps;
        const uint4 in = *reinterpret_cast<const uint4*>(x + e);
        const unsigned w[4] = {in.x, in.y, in.z, in.w};
        float4* out = reinterpret_cast<float4*>(y + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4 o;
            o.x = norm_clip((float)(w[j] & 0xffu), mu, denom, lo, hi);
            o.y = norm_clip((float)((w[j] >> 8) & 0xffu), mu, denom, lo, hi);
            o.z = norm_clip((float)((w[j] >> 16) & 0xffu), mu, denom, lo, hi);
            o.w = norm_clip((float)(w[j] >> 24), mu, denom, lo, hi);
            out[j] = o;
        }
    }
}

// 4 pixels per lane: one 4-byte load, ONE 16-byte store -- a wave reads 256 contiguous bytes and writes one contiguous KiB per
// instruction.  (k_normalize_u8_vec16's four stores per lane each write 64 pieces of 16 bytes 64 bytes apart, every 128-byte
// line four times over: 116 us against this kernel's ~75 at 512 x 3 x 224 x 224; the 16-pixel form is no longer launched.)
__global__ __launch_bounds__(256) void k_normalize_u8_vec4(const uint8_t* __restrict__ x, size_t nvec, int C, int HW,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ stdev, int per_image, float eps,
                                                           float lo, float hi, float* __restrict__ y) {
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t e = v * 4;
        const size_t plane = e / HW;
        const int st = per_image ? (int)plane : (int)(plane % C);
        const float mu = mean[st];
        const float denom = stdev[st] + eps;
        const unsigned w = *reinterpret_cast<const unsigned*>(x + e);
        float4 o;
        o.x = norm_clip((float)(w & 0xffu), mu, denom, lo, hi);
        o.y = norm_clip((float)((w >> 8) & 0xffu), mu, denom, lo, hi);
        o.z = norm_clip((float)((w >> 16) & 0xffu), mu, denom, lo, hi);
        o.w = norm_clip((float)(w >> 24), mu, denom, lo, hi);
        *reinterpret_cast<float4*>(y + e) = o;
    }
}

__global__ __launch_bounds__(256) void k_normalize_f32_vec4(const float* __restrict__ x, size_t nvec, int C, int HW,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ stdev, int per_image, float eps,
                                                            float lo, float hi, float* __restrict__ y) {
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t e = v * 4;
        const size_t plane = e / HW;
        const int st = per_image ? (int)plane : (int)(plane % C);
        const float mu = mean[st];
        const float denom = stdev[st] + eps;
        const float4 in = *reinterpret_cast<const float4*>(x + e);
        float4 o;
        o.x = norm_clip(in.x, mu, denom, lo, hi);
        o.y = norm_clip(in.y, mu, denom, lo, hi);
        o.z = norm_clip(in.z, mu, denom, lo, hi);
        o.w = norm_clip(in.w, mu, denom, lo, hi);
        *reinterpret_cast<float4*>(y + e) = o;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_normalize_scalar(const T* __restrict__ x, size_t n, int C, int HW,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ stdev, int per_image, float eps,
                                                          float lo, float hi, float* __restrict__ y) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t plane = e / HW;
        const int st = per_image ? (int)plane : (int)(plane % C);
        y[e] = norm_clip((float)x[e], mean[st], stdev[st] + eps, lo, hi);
    }
}

// The same normalisation written channels-last for the convolution stems: y[b][hw][0..C) = norm_clip(x[b][c][hw]),
// channels C..3 zero.  PX consecutive pixels per thread (PX = 4 needs HW % 4 == 0): one PX-wide load per plane,
// PX 16-byte stores (a wave writes 64 * PX * 16 contiguous bytes).
template <typename T, int PX>
__global__ __launch_bounds__(256) void k_normalize_nhwc4(const T* __restrict__ x, size_t ngroups, int C, int HW,
                                                         const float* __restrict__ mean, const float* __restrict__ stdev,
                                                         int per_image, float eps, float lo, float hi,
                                                         float* __restrict__ y) {
    const size_t groups_per_image = (size_t)HW / PX;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t b = g / groups_per_image;
        const size_t hw = (g - b * groups_per_image) * PX;
        float o[PX][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < C) {
                const int st = per_image ? (int)(b * C + c) : c;
                const float mu = mean[st];
                const float denom = stdev[st] + eps;
                const T* src = x + (b * C + c) * (size_t)HW + hw;
                T v[PX];
                if constexpr (PX == 4 && sizeof(T) == 1) {
                    const unsigned w = *reinterpret_cast<const unsigned*>(src);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (T)((w >> (8 * j)) & 0xffu);
                } else if constexpr (PX == 4) {
                    const float4 w = *reinterpret_cast<const float4*>(src);
                    v[0] = (T)w.x; v[1] = (T)w.y; v[2] = (T)w.z; v[3] = (T)w.w;
                } else {
#pragma unroll
                    for (int j = 0; j < PX; ++j) v[j] = src[j];
                }
#pragma unroll
                for (int j = 0; j < PX; ++j) o[j][c] = norm_clip((float)v[j], mu, denom, lo, hi);
            } else {
#pragma unroll
                for (int j = 0; j < PX; ++j) o[j][c] = 0.f;
            }
        }
        float4* dst = reinterpret_cast<float4*>(y + (b * (size_t)HW + hw) * 4);
#pragma unroll
        for (int j = 0; j < PX; ++j) dst[j] = make_float4(o[j][0], o[j][1], o[j][2], o[j][3]);
    }
}

// bilinear_tap (bilinear_tap.h): torch's align_corners=False source index with one rounding.
template <typename T>
__global__ __launch_bounds__(256) void k_resize_bilinear(const T* __restrict__ x, int H1, int W1, int H2, int W2,
                                                         float scale_h, float scale_w, float* __restrict__ y) {
    const int ox = blockIdx.x * blockDim.x + threadIdx.x;
    const int oy = blockIdx.y;
    const int plane = blockIdx.z;
    if (ox >= W2) return;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_tap(oy, scale_h, H1, y0, y1, ly0, ly1);
    bilinear_tap(ox, scale_w, W1, x0, x1, lx0, lx1);
    const T* p = x + (size_t)plane * H1 * W1;
    const float v00 = (float)p[(size_t)y0 * W1 + x0];
    const float v01 = (float)p[(size_t)y0 * W1 + x1];
    const float v10 = (float)p[(size_t)y1 * W1 + x0];
    const float v11 = (float)p[(size_t)y1 * W1 + x1];
    const float top = lx0 * v00 + lx1 * v01;
    const float bot = lx0 * v10 + lx1 * v11;
    y[((size_t)plane * H2 + oy) * W2 + ox] = ly0 * top + ly1 * bot;
}

// S == 1: one workgroup per row of E contiguous floats.
__global__ __launch_bounds__(256) void k_l2norm_rows(const float* __restrict__ x, int E, float eps,
                                                     float* __restrict__ y) {
    const float* p = x + (size_t)blockIdx.x * E;
    float* o = y + (size_t)blockIdx.x * E;
    float acc = 0.f;
    for (int i = threadIdx.x; i < E; i += 256) {
        const float v = p[i];
        acc += v * v;
    }
    acc = isc_wave_sum(acc);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    const float denom = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), eps);
    for (int i = threadIdx.x; i < E; i += 256) o[i] = __fdiv_rn(p[i], denom);
}

// S > 1: x [B, E, S]; a workgroup owns 64 consecutive spatial positions of one image, 4 channel groups.
__global__ __launch_bounds__(256) void k_l2norm_spatial(const float* __restrict__ x, int E, int S, float eps,
                                                        float* __restrict__ y) {
    const int s = blockIdx.x * 64 + (threadIdx.x & 63);
    const int g = threadIdx.x >> 6;
    const size_t base = (size_t)blockIdx.y * E * S;
    float acc = 0.f;
    if (s < S)
        for (int e = g; e < E; e += 4) {
            const float v = x[base + (size_t)e * S + s];
            acc += v * v;
        }
    __shared__ float red[4][64];
    red[g][threadIdx.x & 63] = acc;
    __syncthreads();
    if (s >= S) return;
    const int l = threadIdx.x & 63;
    const float denom = fmaxf(sqrtf(red[0][l] + red[1][l] + red[2][l] + red[3][l]), eps);
    for (int e = g; e < E; e += 4) {
        const size_t i = base + (size_t)e * S + s;
        y[i] = __fdiv_rn(x[i], denom);
    }
}

int grid_for(size_t work_items, int threads, int cap_blocks = 256 * 8) {
    size_t blocks = isc_ceil_div(work_items, (size_t)threads);
    if (blocks > (size_t)cap_blocks) blocks = cap_blocks;
    if (blocks == 0) blocks = 1;
    return (int)blocks;
}

}  // namespace

extern "C" int isc_channel_stats_workspace_bytes(int dtype, int B, int C, int H, int W, size_t* bytes) {
    ISC_REQUIRE(bytes && B > 0 && C > 0 && H > 0 && W > 0);
    ISC_REQUIRE(dtype == ISC_U8 || dtype == ISC_F32);
    const size_t hw = (size_t)H * W;
    const size_t items = (size_t)B * isc_ceil_div(hw, (size_t)kStatsChunk);
    *bytes = isc_align_up((size_t)C * items * sizeof(StatPartial), 256);
    return ISC_OK;
}

extern "C" int isc_channel_stats(const void* x, int dtype, int B, int C, int H, int W, float* mean, float* stdev,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    ISC_REQUIRE(x && mean && stdev);
    size_t need = 0;
    const int st = isc_channel_stats_workspace_bytes(dtype, B, C, H, W, &need);
    if (st != ISC_OK) return st;
    if (!workspace || workspace_bytes < need) return ISC_ERR_WORKSPACE;
    const size_t hw64 = (size_t)H * W;
    if (hw64 > 0x7fffffffu || C > 65535) return ISC_ERR_UNSUPPORTED;
    const int HW = (int)hw64;
    const int chunks = (int)isc_ceil_div(HW, kStatsChunk);
    const size_t items64 = (size_t)B * chunks;
    if (items64 > 0x7fffffffu) return ISC_ERR_UNSUPPORTED;
    const int items = (int)items64;
    StatPartial* part = static_cast<StatPartial*>(workspace);
    const dim3 grid(items, C);
    if (dtype == ISC_U8) {
        const int vec_ok = (HW % 16 == 0) && isc_aligned(x, 16);
        hipLaunchKernelGGL(k_stats_partial_u8, grid, dim3(kStatsThreads), 0, isc_stream(stream),
                           static_cast<const uint8_t*>(x), C, HW, chunks, part, items, vec_ok);
    } else {
        const int vec_ok = (HW % 4 == 0) && isc_aligned(x, 16);
        hipLaunchKernelGGL(k_stats_partial_f32, grid, dim3(kStatsThreads), 0, isc_stream(stream),
                           static_cast<const float*>(x), C, HW, chunks, part, items, vec_ok);
    }
    hipLaunchKernelGGL(k_stats_final, dim3(C), dim3(kStatsThreads), 0, isc_stream(stream), part, items,
                       (double)B * (double)HW, dtype == ISC_U8 ? 1 : 0, mean, stdev);
    return isc_launch_status();
}

#ifdef ISC_ABLATION
static bool normalize_vec16() {
    static const bool v = getenv("ISC_NORMALIZE_VEC16") != nullptr;  // A/B aid: the 16-pixels-per-lane form, as before
    return v;
}
#else
static constexpr bool normalize_vec16() { return false; }
#endif

extern "C" int isc_normalize_clip(const void* x, int dtype, int B, int C, int H, int W, const float* mean,
                                  const float* stdev, int stat_batch, float eps, float lo, float hi, float* y,
                                  void* stream) {
    ISC_REQUIRE(x && mean && stdev && y && B > 0 && C > 0 && H > 0 && W > 0);
    ISC_REQUIRE(dtype == ISC_U8 || dtype == ISC_F32);
    ISC_REQUIRE(stat_batch == 1 || stat_batch == B);
    const size_t hw64 = (size_t)H * W;
    if (hw64 > 0x7fffffffu) return ISC_ERR_UNSUPPORTED;
    const int HW = (int)hw64;
    const size_t n = (size_t)B * C * HW;
    const int per_image = (stat_batch == B && B > 1) ? 1 : 0;
    hipStream_t s = isc_stream(stream);
    if (dtype == ISC_U8) {
        const uint8_t* p = static_cast<const uint8_t*>(x);
        if (HW % 4 == 0 && isc_aligned(p, 4) && isc_aligned(y, 16) && !normalize_vec16()) {
            const size_t nvec = n / 4;
            hipLaunchKernelGGL(k_normalize_u8_vec4, dim3(grid_for(nvec, 256)), dim3(256), 0, s, p, nvec, C, HW, mean,
                               stdev, per_image, eps, lo, hi, y);
        } else if (HW % 16 == 0 && isc_aligned(p, 16) && isc_aligned(y, 16)) {
            const size_t nvec = n / 16;
            hipLaunchKernelGGL(k_normalize_u8_vec16, dim3(grid_for(nvec, 256)), dim3(256), 0, s, p, nvec, C, HW, mean,
                               stdev, per_image, eps, lo, hi, y);
        } else {
            hipLaunchKernelGGL(k_normalize_scalar<uint8_t>, dim3(grid_for(n, 256)), dim3(256), 0, s, p, n, C, HW, mean,
                               stdev, per_image, eps, lo, hi, y);
        }
    } else {
        const float* p = static_cast<const float*>(x);
        if (HW % 4 == 0 && isc_aligned(p, 16) && isc_aligned(y, 16)) {
            const size_t nvec = n / 4;
            hipLaunchKernelGGL(k_normalize_f32_vec4, dim3(grid_for(nvec, 256)), dim3(256), 0, s, p, nvec, C, HW, mean,
                               stdev, per_image, eps, lo, hi, y);
        } else {
            hipLaunchKernelGGL(k_normalize_scalar<float>, dim3(grid_for(n, 256)), dim3(256), 0, s, p, n, C, HW, mean,
                               stdev, per_image, eps, lo, hi, y);
        }
    }
    return isc_launch_status();
}

#ifdef ISC_ABLATION
static bool normalize_no_transpose() {
    static const bool v = getenv("ISC_NORMALIZE_NO_TRANSPOSE") != nullptr;  // A/B aid: strided 16-byte stores, as before
    return v;
}
#else
static constexpr bool normalize_no_transpose() { return false; }
#endif

// The four-pixels-per-thread form with the stores TRANSPOSED through LDS: a thread still reads its four consecutive pixels of
// each plane with one load, but a store instruction of k_normalize_nhwc4<T, 4> writes 64 pieces of 16 bytes that lie 64 bytes
// apart (every 128-byte line is written by four instructions), and the float32 output is 5/6 of this kernel's traffic.  Here
// the 1 024 pixels of a workgroup pass through 16 KiB of LDS and thread t stores pixels t, t + 256, ...: a wave writes one
// contiguous KiB per instruction.  Same arithmetic, bit-identical output.
template <typename T>
__global__ __launch_bounds__(256) void k_normalize_nhwc4_t(const T* __restrict__ x, size_t ngroups, int C, int HW,
                                                           const float* __restrict__ mean, const float* __restrict__ stdev,
                                                           int per_image, float eps, float lo, float hi,
                                                           float* __restrict__ y) {
    __shared__ float4 px[1024];
    const int tid = threadIdx.x;
    const size_t groups_per_image = (size_t)HW / 4;
    for (size_t base = (size_t)blockIdx.x * 256; base < ngroups; base += (size_t)gridDim.x * 256) {
        const size_t g = base + tid;
        if (g < ngroups) {
            const size_t b = g / groups_per_image;
            const size_t hw = (g - b * groups_per_image) * 4;
            float o[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < C) {
                    const int st = per_image ? (int)(b * C + c) : c;
                    const float mu = mean[st];
                    const float denom = stdev[st] + eps;
                    const T* src = x + (b * C + c) * (size_t)HW + hw;
                    T v[4];
                    if constexpr (sizeof(T) == 1) {
                        const unsigned w = *reinterpret_cast<const unsigned*>(src);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = (T)((w >> (8 * j)) & 0xffu);
                    } else {
                        const float4 w = *reinterpret_cast<const float4*>(src);
                        v[0] = (T)w.x; v[1] = (T)w.y; v[2] = (T)w.z; v[3] = (T)w.w;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j][c] = norm_clip((float)v[j], mu, denom, lo, hi);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j][c] = 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) px[tid * 4 + j] = make_float4(o[j][0], o[j][1], o[j][2], o[j][3]);
        }
        __syncthreads();
        // y is [B][HW][4]: the workgroup's 1 024 pixels are consecutive in it whatever image they belong to
        const size_t npx = (ngroups - base < 256 ? ngroups - base : 256) * 4;
        float4* dst = reinterpret_cast<float4*>(y) + base * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((size_t)(j * 256 + tid) < npx) dst[j * 256 + tid] = px[j * 256 + tid];
        __syncthreads();
    }
}

extern "C" int isc_normalize_clip_nhwc4(const void* x, int dtype, int B, int C, int H, int W, const float* mean,
                                        const float* stdev, int stat_batch, float eps, float lo, float hi, float* y,
                                        void* stream) {
    ISC_REQUIRE(x && mean && stdev && y && B > 0 && C > 0 && C <= 4 && H > 0 && W > 0);
    ISC_REQUIRE(dtype == ISC_U8 || dtype == ISC_F32);
    ISC_REQUIRE(stat_batch == 1 || stat_batch == B);
    const size_t hw64 = (size_t)H * W;
    if (hw64 > 0x7fffffffu) return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(y, 16)) return ISC_ERR_ALIGNMENT;
    const int HW = (int)hw64;
    const int per_image = (stat_batch == B && B > 1) ? 1 : 0;
    hipStream_t s = isc_stream(stream);
    const bool vec = HW % 4 == 0 && isc_aligned(x, 16);
    const size_t ngroups = (size_t)B * (vec ? HW / 4 : HW);
    const dim3 grid(grid_for(ngroups, 256)), block(256);
    if (dtype == ISC_U8) {
        const uint8_t* p = static_cast<const uint8_t*>(x);
        if (vec && !normalize_no_transpose()) hipLaunchKernelGGL((k_normalize_nhwc4_t<uint8_t>), grid, block, 0, s, p, ngroups, C, HW, mean, stdev, per_image, eps, lo, hi, y);
        else if (vec) hipLaunchKernelGGL((k_normalize_nhwc4<uint8_t, 4>), grid, block, 0, s, p, ngroups, C, HW, mean, stdev, per_image, eps, lo, hi, y);
        else hipLaunchKernelGGL((k_normalize_nhwc4<uint8_t, 1>), grid, block, 0, s, p, ngroups, C, HW, mean, stdev, per_image, eps, lo, hi, y);
    } else {
        const float* p = static_cast<const float*>(x);
        if (vec && !normalize_no_transpose()) hipLaunchKernelGGL((k_normalize_nhwc4_t<float>), grid, block, 0, s, p, ngroups, C, HW, mean, stdev, per_image, eps, lo, hi, y);
        else if (vec) hipLaunchKernelGGL((k_normalize_nhwc4<float, 4>), grid, block, 0, s, p, ngroups, C, HW, mean, stdev, per_image, eps, lo, hi, y);
        else hipLaunchKernelGGL((k_normalize_nhwc4<float, 1>), grid, block, 0, s, p, ngroups, C, HW, mean, stdev, per_image, eps, lo, hi, y);
    }
    return isc_launch_status();
}

extern "C" int isc_resize_bilinear(const void* x, int dtype, int planes, int H1, int W1, int H2, int W2, float* y,
                                   void* stream) {
    ISC_REQUIRE(x && y && planes > 0 && H1 > 0 && W1 > 0 && H2 > 0 && W2 > 0);
    ISC_REQUIRE(dtype == ISC_U8 || dtype == ISC_F32);
    if (H2 > 65535 || planes > 65535) return ISC_ERR_UNSUPPORTED;
    const float scale_h = (float)H1 / (float)H2;
    const float scale_w = (float)W1 / (float)W2;
    const dim3 grid(isc_ceil_div(W2, 256), H2, planes);
    if (dtype == ISC_U8)
        hipLaunchKernelGGL(k_resize_bilinear<uint8_t>, grid, dim3(256), 0, isc_stream(stream),
                           static_cast<const uint8_t*>(x), H1, W1, H2, W2, scale_h, scale_w, y);
    else
        hipLaunchKernelGGL(k_resize_bilinear<float>, grid, dim3(256), 0, isc_stream(stream),
                           static_cast<const float*>(x), H1, W1, H2, W2, scale_h, scale_w, y);
    return isc_launch_status();
}

extern "C" int isc_l2norm_channels(const float* x, int B, int E, int S, float eps, float* y, void* stream) {
    ISC_REQUIRE(x && y && B > 0 && E > 0 && S > 0);
    if (S == 1) {
        hipLaunchKernelGGL(k_l2norm_rows, dim3(B), dim3(256), 0, isc_stream(stream), x, E, eps, y);
    } else {
        if (B > 65535) return ISC_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(k_l2norm_spatial, dim3(isc_ceil_div(S, 64), B), dim3(256), 0, isc_stream(stream), x, E, S,
                           eps, y);
    }
    return isc_launch_status();
}

// ---------------------------------------------------------------------------------------------------------
// isc_resize_aa: antialiased bicubic resize (the filter of aa_filter.h with each axis' own input size) of the crop
// rectangle only, the quantisation and the per-channel normalisation fused into the store.
//
// Two launches.  k_resize_aa_tables writes, per output row and column of the CROP, the first tap, the tap count and the
// normalised weights (a thread per index; the index is the absolute one in the resized image, so a weight does not
// know the crop).  k_resize_aa then gives a workgroup `band` output rows x `tw` output columns of one plane.  The input
// rows of the band's vertical support pass through LDS 64 at a time:
//   1  staging: a wave copies a row's segment (the tile's horizontal support, nothing else) as it is -- uint8 rows as
//      the row's own aligned 4-byte words, the ragged first and last one put together byte by byte; four rows' loads are
//      issued before the first is stored;
//   2  horizontal pass, lane = INPUT ROW, wave = output column (four columns in flight): the taps and weights of a
//      column are the same for every lane, so they are scalar loads from the table, and the lanes read the same
//      offset of 64 different lines, whose pitch is an odd number of words: no two on one bank at any scale.  Taps in
//      ASCENDING order, one fmaf each from 0, into line [row][column] of LDS (pitch tw + 1);
//   3  after the last chunk a wave per output row combines the lines vertically, taps ASCENDING, one fmaf each from 0,
//      the weights scalar loads again, and stores tw consecutive floats per instruction.
// (Lane = output column in the horizontal pass, the obvious map, makes lanes read words `scale` apart: at 3000 x 2000
// -> 224 that ran 1.9 ms against this form's time in DESIGN.md, bound by LDS bank conflicts.)
// The order of the two sums is torch's (the horizontal pass first), and a pixel's bits depend on its own taps and
// weights only: not on the crop, the plane, or the band and tile it falls in.
// The host picks tw in {64, 32, 16, 8} and band <= 32 so that the lines fit in LDS at the call's scale.
namespace {

constexpr int kAaThreads = 256;
constexpr int kAaWaves = kAaThreads / ISC_WAVE;
constexpr int kAaInFlight = 8;               // rows whose loads a wave issues before it stores the first
constexpr int kAaTapBlock = 8;               // taps are taken in whole blocks: the tables pad a row with zero weights
constexpr int kAaPre = 2;                    // 4-byte pieces (floats: pixels) of a row a lane holds meanwhile
constexpr float kAaMaxScale = 64.f;          // downscale factor per axis: at most 258 taps
constexpr int kAaLdsTarget = 48 * 1024;      // three workgroups per CU
constexpr int kAaLdsLimit = 64 * 1024;
constexpr int kAaMaxPlanesPerLaunch = 65535;
constexpr size_t kAaMaxBlocks = (size_t)1 << 23;  // tiles of one plane; a launch stays below 2^32 threads

struct AaArgs {
    int H1, W1, Hc, Wc, C;
    int taps_y, taps_x;      // table pitch = the most taps an output of that axis can have
    int band, tw, tiles_x;   // output rows and columns of a workgroup; column tiles per band
    int chunk;               // input rows filtered at a time, one a lane: 64, fewer where 64 staged rows do not fit
    int rows_cap, span_cap;  // filtered lines, and staged pixels per row, the launch was sized for
    int hb, sp;              // pitch of a filtered line (floats) and of a staged row (input elements)
    int stage_offset;        // bytes from the start of LDS to the staged rows
    int quantize;
    const int* meta;         // lo_y[Hc], n_y[Hc], lo_x[Wc], n_x[Wc]
    const float* wy;         // [Hc][taps_y]
    const float* wx;         // [Wc][taps_x]
    const float* mean;
    const float* stdev;
};

// the most taps AaTaps gives an output at this scale: the window is 4 max(s, 1) wide, plus its two roundings; whole blocks
inline int aa_tap_bound(float scale) {
    return isc_ceil_div((int)(4.f * fmaxf(scale, 1.f)) + 2, kAaTapBlock) * kAaTapBlock;
}

__global__ __launch_bounds__(256) void k_resize_aa_tables(int H1, int top, int Hc, float scale_h, int taps_y, int W1,
                                                          int left, int Wc, float scale_w, int taps_x,
                                                          int* __restrict__ meta, float* __restrict__ wy,
                                                          float* __restrict__ wx) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)Hc + (unsigned)Wc) return;
    const bool col = i >= (unsigned)Hc;
    const int idx = col ? (int)(i - (unsigned)Hc) : (int)i;
    const int pitch = col ? taps_x : taps_y;
    const AaTaps t(col ? left + idx : top + idx, col ? scale_w : scale_h, col ? W1 : H1);
    const int n = min(t.n, pitch);
    int* lo = meta + (col ? 2 * (size_t)Hc : 0);
    lo[idx] = t.lo;
    lo[(size_t)(col ? Wc : Hc) + idx] = n;
    float* w = (col ? wx : wy) + (size_t)idx * pitch;
    for (int j = 0; j < n; ++j) w[j] = t.weight(j);
    // the tap loops run in whole blocks: a zero weight leaves a sum as it is (fmaf(0, finite, acc) == acc)
    for (int j = n; j < (n + kAaTapBlock - 1) / kAaTapBlock * kAaTapBlock; ++j) w[j] = 0.f;
}

// bytes [off, total) from the 4-byte aligned `pa`, four at q: the word itself, or its bytes inside the segment
__device__ __forceinline__ unsigned aa_load_piece(const uint8_t* pa, int q, int off, int total) {
    if (q >= off && q + 4 <= total) return *reinterpret_cast<const unsigned*>(pa + q);
    // four independent loads from addresses clamped into the segment (a guarded load each would wait for the one before)
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned v = pa[min(max(q + j, off), total - 1)];
        w |= (q + j >= off && q + j < total ? v : 0u) << (8 * j);
    }
    return w;
}

// where a row's first pixel sits in its staged line: uint8 lines start at the row's 4-byte boundary
__device__ __forceinline__ int aa_line_offset(const uint8_t* p) { return (int)(reinterpret_cast<uintptr_t>(p) & 3u); }
__device__ __forceinline__ int aa_line_offset(const float*) { return 0; }

// One wave copies `len` pixels of rows wave, wave + 4, ... < nrows (W1 apart from `first`) to their lines.
__device__ __forceinline__ void aa_stage_rows(const uint8_t* first, int W1, int nrows, int len, uint8_t* stage, int sp,
                                              int wave, int lane) {
    for (int r = wave; r < nrows; r += kAaWaves * kAaInFlight) {
        unsigned pre[kAaInFlight][kAaPre];
#pragma unroll
        for (int i = 0; i < kAaInFlight; ++i) {
            const int rr = r + kAaWaves * i;
            if (rr >= nrows) break;
            const uint8_t* p = first + (size_t)rr * W1;
            const int off = aa_line_offset(p), total = off + len;
#pragma unroll
            for (int j = 0; j < kAaPre; ++j) {
                const int q = 4 * (lane + ISC_WAVE * j);
                pre[i][j] = q < total ? aa_load_piece(p - off, q, off, total) : 0u;
            }
        }
#pragma unroll
        for (int i = 0; i < kAaInFlight; ++i) {
            const int rr = r + kAaWaves * i;
            if (rr >= nrows) break;
            const uint8_t* p = first + (size_t)rr * W1;
            const int off = aa_line_offset(p), total = off + len;
            uint8_t* line = stage + rr * sp;  // sp % 4 == 0
#pragma unroll
            for (int j = 0; j < kAaPre; ++j) {
                const int q = 4 * (lane + ISC_WAVE * j);
                if (q < total) *reinterpret_cast<unsigned*>(line + q) = pre[i][j];
            }
            for (int q = 4 * (lane + ISC_WAVE * kAaPre); q < total; q += 4 * ISC_WAVE)
                *reinterpret_cast<unsigned*>(line + q) = aa_load_piece(p - off, q, off, total);
            if (lane < kAaTapBlock - 1) line[((total + 3) & ~3) + lane] = 0;  // what the last block's zero weights meet
        }
    }
}

__device__ __forceinline__ void aa_stage_rows(const float* first, int W1, int nrows, int len, float* stage, int sp,
                                              int wave, int lane) {
    for (int r = wave; r < nrows; r += kAaWaves * kAaInFlight) {
        float pre[kAaInFlight][kAaPre];
#pragma unroll
        for (int i = 0; i < kAaInFlight; ++i) {
            const int rr = r + kAaWaves * i;
            if (rr >= nrows) break;
            const float* p = first + (size_t)rr * W1;
#pragma unroll
            for (int j = 0; j < kAaPre; ++j) {
                const int q = lane + ISC_WAVE * j;
                pre[i][j] = q < len ? p[q] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < kAaInFlight; ++i) {
            const int rr = r + kAaWaves * i;
            if (rr >= nrows) break;
            const float* p = first + (size_t)rr * W1;
            float* line = stage + rr * sp;
#pragma unroll
            for (int j = 0; j < kAaPre; ++j) {
                const int q = lane + ISC_WAVE * j;
                if (q < len) line[q] = pre[i][j];
            }
            for (int q = lane + ISC_WAVE * kAaPre; q < len; q += ISC_WAVE) line[q] = p[q];
            if (lane < kAaTapBlock - 1) line[len + lane] = 0.f;  // what the last block's zero weights meet: finite
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kAaThreads) void k_resize_aa(const T* __restrict__ x, AaArgs a, size_t plane0,
                                                          float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char aa_lds[];
    const int tid = threadIdx.x, lane = tid & (ISC_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / ISC_WAVE);  // uniform: the weights are scalar loads
    const int tile = blockIdx.x % a.tiles_x, bandi = blockIdx.x / a.tiles_x;
    const size_t plane = plane0 + blockIdx.z;
    const int c0 = tile * a.tw, i0 = bandi * a.band;
    const int ncol = min(a.tw, a.Wc - c0), nrow = min(a.band, a.Hc - i0);
    const int* lo_y = a.meta;
    const int* n_y = lo_y + a.Hc;
    const int* lo_x = n_y + a.Hc;
    const int* n_x = lo_x + a.Wc;
    float* hbuf = reinterpret_cast<float*>(aa_lds);          // [rows_cap][hb]
    T* stage = reinterpret_cast<T*>(aa_lds + a.stage_offset);  // [chunk][sp]

    // the input rows and columns this tile reads (first taps and ends are non-decreasing along an axis)
    const int rbase = lo_y[i0];
    const int R = min(lo_y[i0 + nrow - 1] + n_y[i0 + nrow - 1] - rbase, a.rows_cap);
    const int xlo = lo_x[c0];
    const int len = min(lo_x[c0 + ncol - 1] + n_x[c0 + ncol - 1] - xlo, a.span_cap);

    const T* xp = x + plane * ((size_t)a.H1 * a.W1) + (size_t)rbase * a.W1 + xlo;
    for (int r0 = 0; r0 < R; r0 += a.chunk) {
        const int nrows = min(a.chunk, R - r0);
        const T* first = xp + (size_t)r0 * a.W1;
        aa_stage_rows(first, a.W1, nrows, len, stage, a.sp, wave, lane);
        __syncthreads();
        // lanes past the chunk's rows read a line of an earlier chunk, or unwritten LDS, and store nothing
        const T* line = stage + (lane < a.chunk ? lane : 0) * a.sp +
                        (lane < nrows ? aa_line_offset(first + (size_t)lane * a.W1) : 0);
        for (int c = wave; c < ncol; c += kAaWaves) {
            const int lo = lo_x[c0 + c] - xlo;
            const int n = min(n_x[c0 + c], len - lo);
            const float* w = a.wx + (size_t)(c0 + c) * a.taps_x;
            const T* px = line + lo;
            float acc = 0.f;
            for (int b = 0; b < n; b += kAaTapBlock) {
#pragma unroll
                for (int j = 0; j < kAaTapBlock; ++j) acc = fmaf(w[b + j], (float)px[b + j], acc);
            }
            if (lane < nrows) hbuf[(r0 + lane) * a.hb + c] = acc;
        }
        __syncthreads();
    }

    // the lines the last block's zero weights meet
    for (int e = tid; e < (kAaTapBlock - 1) * a.hb; e += kAaThreads) hbuf[R * a.hb + e] = 0.f;
    __syncthreads();

    float mu = 0.f, sd = 1.f;
    if (a.mean) {
        const int c = (int)(plane % (size_t)a.C);
        mu = a.mean[c];
        sd = a.stdev[c];
    }
    for (int i = wave; i < nrow; i += kAaWaves) {
        const int gi = i0 + i;
        const int lo = lo_y[gi] - rbase;
        const int n = min(n_y[gi], R - lo);
        if (lane >= ncol) continue;
        const float* wrow = a.wy + (size_t)gi * a.taps_y;
        const float* h = hbuf + lo * a.hb + lane;
        float v = 0.f;
        for (int k = 0; k < n; k += kAaTapBlock) {
#pragma unroll
            for (int j = 0; j < kAaTapBlock; ++j) v = fmaf(wrow[k + j], h[(k + j) * a.hb], v);
        }
        if (a.quantize) v = rintf(fminf(fmaxf(v, 0.f), 255.f));
        if (a.mean) v = __fdiv_rn(v - mu, sd);
        y[(plane * a.Hc + gi) * a.Wc + c0 + lane] = v;
    }
}

// LDS bytes of a (band, tw) geometry for input elements of `elem` bytes; fills the capacities and pitches it implies
size_t aa_lds_bytes(AaArgs& a, float scale_h, float scale_w, int band, int tw, int chunk, int elem) {
    // first taps of outputs k apart differ by at most s k + 1 (+ 1: the float roundings of the centres)
    const long long rows = (long long)ceilf(scale_h * (float)(band - 1)) + 2 + a.taps_y;
    const long long span = (long long)ceilf(scale_w * (float)(tw - 1)) + 2 + a.taps_x;
    a.band = band;
    a.tw = tw;
    a.chunk = chunk;
    a.rows_cap = (int)(rows < a.H1 ? rows : a.H1);
    a.span_cap = (int)(span < a.W1 ? span : a.W1);
    a.hb = tw + 1;  // odd: the horizontal pass writes a column of it, a lane a line
    // a staged row: whole words, an ODD number of them, so that the lines' equal offsets fall on different banks;
    // a uint8 line starts up to three bytes before the segment
    // ... and ends with the kAaTapBlock - 1 zeros the last block of taps may reach
    int words = elem == 1 ? (a.span_cap + 3 + 3) / 4 + kAaTapBlock / 4 : a.span_cap + kAaTapBlock - 1;
    words |= 1;
    a.sp = elem == 1 ? 4 * words : words;
    a.stage_offset = (int)isc_align_up(sizeof(float) * (size_t)(a.rows_cap + kAaTapBlock - 1) * a.hb, 16);
    return (size_t)a.stage_offset + (size_t)chunk * words * 4;
}

// The geometry of a call, or ISC_ERR_UNSUPPORTED.  Needs a.H1, a.W1, a.Hc, a.Wc.  Among the geometries that fit, the
// one with the fewest lane slots of the horizontal pass per output row (64 a chunk of rows, used or not); a narrower tile only
// where it saves a tenth.
int aa_plan(AaArgs& a, int H2, int W2, int elem, float& scale_h, float& scale_w, size_t& lds) {
    if ((size_t)a.H1 * a.W1 > 0x7fffffffu || (size_t)a.Hc * a.Wc > 0x7fffffffu) return ISC_ERR_UNSUPPORTED;
    scale_h = (float)a.H1 / (float)H2;
    scale_w = (float)a.W1 / (float)W2;
    if (scale_h > kAaMaxScale || scale_w > kAaMaxScale) return ISC_ERR_UNSUPPORTED;
    a.taps_y = aa_tap_bound(scale_h);
    a.taps_x = aa_tap_bound(scale_w);
    for (const int limit : {kAaLdsTarget, kAaLdsLimit}) {
        int best_tw = 0, best_band = 0, best_chunk = 0;
        float best = 0.f;
        for (const int tw : {64, 32, 16, 8})
            for (const int chunk : {64, 32, 16})
                for (int band = 32; band >= 1; --band) {
                    if (aa_lds_bytes(a, scale_h, scale_w, band, tw, chunk, elem) > (size_t)limit) continue;
                    const float cost = (float)(isc_ceil_div(a.rows_cap, chunk) * ISC_WAVE) / (float)band;
                    if (best_tw == 0 || cost < (tw == best_tw ? best : 0.9f * best))
                        best_tw = tw, best_band = band, best_chunk = chunk, best = cost;
                }
        if (best_tw == 0) continue;
        lds = aa_lds_bytes(a, scale_h, scale_w, best_band, best_tw, best_chunk, elem);
        a.tiles_x = isc_ceil_div(a.Wc, best_tw);
        if ((size_t)a.tiles_x * isc_ceil_div(a.Hc, best_band) > kAaMaxBlocks) return ISC_ERR_UNSUPPORTED;
        return ISC_OK;
    }
    return ISC_ERR_UNSUPPORTED;
}

struct AaWorkspace {
    size_t meta, wy, wx, bytes;  // byte offsets
};

AaWorkspace aa_workspace(const AaArgs& a) {
    AaWorkspace w;
    w.meta = 0;
    w.wy = isc_align_up(sizeof(int) * 2 * ((size_t)a.Hc + a.Wc), 16);
    w.wx = w.wy + isc_align_up(sizeof(float) * (size_t)a.Hc * a.taps_y, 16);
    w.bytes = isc_align_up(w.wx + sizeof(float) * (size_t)a.Wc * a.taps_x, 256);
    return w;
}

int aa_check_shape(int H1, int W1, int H2, int W2, int top, int left, int Hc, int Wc) {
    ISC_REQUIRE(H1 > 0 && W1 > 0 && H2 > 0 && W2 > 0 && Hc > 0 && Wc > 0 && top >= 0 && left >= 0);
    ISC_REQUIRE((long long)top + Hc <= H2 && (long long)left + Wc <= W2);
    return ISC_OK;
}

}  // namespace

extern "C" int isc_resize_aa_workspace_bytes(int H1, int W1, int H2, int W2, int top, int left, int Hc, int Wc,
                                             size_t* bytes) {
    ISC_REQUIRE(bytes);
    int st = aa_check_shape(H1, W1, H2, W2, top, left, Hc, Wc);
    if (st != ISC_OK) return st;
    AaArgs a = {};
    a.H1 = H1, a.W1 = W1, a.Hc = Hc, a.Wc = Wc;
    float sh, sw;
    size_t lds;
    st = aa_plan(a, H2, W2, 4, sh, sw, lds);  // the limits are those of float input, the tables the same for both
    if (st != ISC_OK) return st;
    *bytes = aa_workspace(a).bytes;
    return ISC_OK;
}

extern "C" int isc_resize_aa(const void* x, int dtype, int B, int C, int H1, int W1, int H2, int W2, int top, int left,
                             int Hc, int Wc, const float* mean, const float* stdev, int quantize, float* y,
                             void* workspace, size_t workspace_bytes, void* stream) {
    ISC_REQUIRE(x && y && B > 0 && C > 0);
    ISC_REQUIRE(dtype == ISC_U8 || dtype == ISC_F32);
    ISC_REQUIRE((mean == nullptr) == (stdev == nullptr));
    int st = aa_check_shape(H1, W1, H2, W2, top, left, Hc, Wc);
    if (st != ISC_OK) return st;
    AaArgs a = {};
    a.H1 = H1, a.W1 = W1, a.Hc = Hc, a.Wc = Wc, a.C = C;
    float scale_h, scale_w;
    size_t lds;
    st = aa_plan(a, H2, W2, 4, scale_h, scale_w, lds);  // what the workspace query refuses, the call refuses
    if (st == ISC_OK && dtype == ISC_U8) st = aa_plan(a, H2, W2, 1, scale_h, scale_w, lds);
    if (st != ISC_OK) return st;
    if (!isc_aligned(y, 4) || !isc_aligned(mean, 4) || !isc_aligned(stdev, 4) || !isc_aligned(workspace, 16) ||
        (dtype == ISC_F32 && !isc_aligned(x, 4)))
        return ISC_ERR_ALIGNMENT;
    const AaWorkspace w = aa_workspace(a);
    if (!workspace || workspace_bytes < w.bytes) return ISC_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    int* meta = reinterpret_cast<int*>(ws + w.meta);
    float* wy = reinterpret_cast<float*>(ws + w.wy);
    float* wx = reinterpret_cast<float*>(ws + w.wx);
    a.meta = meta, a.wy = wy, a.wx = wx, a.mean = mean, a.stdev = stdev, a.quantize = quantize != 0;
    hipStream_t s = isc_stream(stream);
    const unsigned entries = (unsigned)Hc + (unsigned)Wc;
    hipLaunchKernelGGL(k_resize_aa_tables, dim3(isc_ceil_div(entries, 256u)), dim3(256), 0, s, H1, top, Hc, scale_h,
                       a.taps_y, W1, left, Wc, scale_w, a.taps_x, meta, wy, wx);
    const size_t planes = (size_t)B * C;
    const unsigned blocks = (unsigned)((size_t)a.tiles_x * isc_ceil_div(Hc, a.band));
    size_t per_launch = (((size_t)1 << 24) - 1) / blocks;  // blocks * z * 256 < 2^32
    if (per_launch > (size_t)kAaMaxPlanesPerLaunch) per_launch = kAaMaxPlanesPerLaunch;
    for (size_t p0 = 0; p0 < planes; p0 += per_launch) {
        const unsigned z = (unsigned)(planes - p0 < per_launch ? planes - p0 : per_launch);
        if (dtype == ISC_U8)
            hipLaunchKernelGGL(k_resize_aa<uint8_t>, dim3(blocks, 1, z), dim3(kAaThreads), lds, s,
                               static_cast<const uint8_t*>(x), a, p0, y);
        else
            hipLaunchKernelGGL(k_resize_aa<float>, dim3(blocks, 1, z), dim3(kAaThreads), lds, s,
                               static_cast<const float*>(x), a, p0, y);
    }
    return isc_launch_status();
}
