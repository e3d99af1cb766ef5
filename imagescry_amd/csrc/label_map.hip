// isc_label_map, isc_map_class_scores: dense patch scores -> pixel label maps (include/imagescry_hip.h has the
// arithmetic, which the tests hold these kernels to bit for bit).
#include "bilinear_tap.h"
#include "isc_common.h"

#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------------
// k_label_map: a workgroup owns kTileW x kTileH output pixels of one image, a thread one pixel (a wave = one row
// segment of 64 pixels, so a wave's float stores are 256 contiguous bytes).  The low-resolution cells the tile's taps
// touch form a rectangle, the footprint; it passes through LDS as [cell][prompt chunk] (row stride chunk + kPad floats:
// a 16-byte read per tap and four prompts, neighbouring cells on other banks, lanes on one cell broadcast).  The chunk is
// kPromptChunk prompts, fewer where the footprint is large (a scale ratio near 1 or a mild downscale) so that footprint
// x (chunk + kPad) stays inside kLdsFloats; a footprint above 1024 cells (a steep downscale, where a pixel's four cells
// are shared with no neighbour anyway) is read from memory directly.  The running (best, its class, best of another
// class) stays in registers over the chunks; its comparisons are exact and ascending in the prompt, so neither the
// chunking nor the path changes a bit.
constexpr int kTileW = 64;
constexpr int kTileH = 4;
constexpr int kLabelThreads = kTileW * kTileH;
constexpr int kPromptChunk = 32;
constexpr int kPad = 4;
constexpr int kLdsFloats = 8192;
constexpr int kMaxPrompts = 1024;
constexpr int kUnlabeled = 255;
static_assert(kLabelThreads == 256 && kTileW == ISC_WAVE, "one wave per tile row; the histogram has a thread per label");

// The running choice: `best` / `cls` by v descending, NaN last, ties to the lower prompt (prompts arrive
// ascending, so only a strictly better value replaces); `other` = the largest number among the prompts of another class
// than `cls`, NaN while there is none.  When a prompt of another class takes over, the old best is the largest value seen
// and belongs to another class than the new one: it is the new `other` (a NaN old best means no number was seen yet).
struct Running {
    float best, other;
    int cls;
};

__device__ __forceinline__ void consider(Running& r, float v, int cls) {
    if (v > r.best || (r.best != r.best && v == v)) {
        if (cls != r.cls) r.other = r.best;
        r.best = v;
        r.cls = cls;
    } else if (cls != r.cls && v == v && !(v <= r.other)) {
        r.other = v;
    }
}

__device__ __forceinline__ float blend(float w00, float w01, float w10, float w11, float s00, float s01, float s10,
                                       float s11) {
    return __fmaf_rn(w11, s11, __fmaf_rn(w10, s10, __fmaf_rn(w01, s01, __fmul_rn(w00, s00))));
}

__global__ __launch_bounds__(kLabelThreads) void k_label_map(const float* __restrict__ scores, int64_t ldc,
                                                             const int32_t* __restrict__ class_of, int C, int h, int w,
                                                             int H, int W, float scale_h, float scale_w, float min_score,
                                                             uint8_t* __restrict__ labels, float* __restrict__ best_out,
                                                             float* __restrict__ margin_out, int32_t* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float tile[kLdsFloats];
    __shared__ int hist[256];
    const int tid = threadIdx.x;
    const int tx = tid & (kTileW - 1), ty = tid / kTileW;
    const int X0 = blockIdx.x * kTileW, Y0 = blockIdx.y * kTileH, b = blockIdx.z;
    const int x = X0 + tx, y = Y0 + ty;
    const bool valid = x < W && y < H;
    hist[tid] = 0;

    // a thread outside the image computes the last pixel of its row / column again and stores nothing
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_tap(min(y, H - 1), scale_h, h, y0, y1, ly0, ly1);
    bilinear_tap(min(x, W - 1), scale_w, w, x0, x1, lx0, lx1);
    const float w00 = __fmul_rn(ly0, lx0), w01 = __fmul_rn(ly0, lx1);
    const float w10 = __fmul_rn(ly1, lx0), w11 = __fmul_rn(ly1, lx1);

    // the footprint: first tap of the tile's first pixel .. second tap of its last one (the taps are monotone)
    int fy0, fy1, fx0, fx1, unused_i;
    float unused_l0, unused_l1;
    bilinear_tap(Y0, scale_h, h, fy0, unused_i, unused_l0, unused_l1);
    bilinear_tap(min(Y0 + kTileH, H) - 1, scale_h, h, unused_i, fy1, unused_l0, unused_l1);
    bilinear_tap(X0, scale_w, w, fx0, unused_i, unused_l0, unused_l1);
    bilinear_tap(min(X0 + kTileW, W) - 1, scale_w, w, unused_i, fx1, unused_l0, unused_l1);
    const int fw = fx1 - fx0 + 1;
    const int64_t cells64 = (int64_t)(fy1 - fy0 + 1) * fw;
    const int chunk = cells64 <= kLdsFloats / (4 + kPad)
                          ? min(kPromptChunk, (kLdsFloats / (int)cells64 - kPad) & ~3)
                          : 0;

    const float* img = scores + (size_t)b * h * w * ldc;
    Running r;
    r.best = r.other = __builtin_nanf("");
    r.cls = class_of ? class_of[0] : 0;

    if (chunk > 0) {
        const int cells = (int)cells64;
        const int stride = chunk + kPad;
        const float* p00 = tile + ((y0 - fy0) * fw + (x0 - fx0)) * stride;
        const float* p01 = tile + ((y0 - fy0) * fw + (x1 - fx0)) * stride;
        const float* p10 = tile + ((y1 - fy0) * fw + (x0 - fx0)) * stride;
        const float* p11 = tile + ((y1 - fy0) * fw + (x1 - fx0)) * stride;
        for (int c0 = 0; c0 < C; c0 += chunk) {
            const int n = min(chunk, C - c0);
            __syncthreads();  // the previous chunk is consumed (and, the first time, hist is zero)
            for (int i = tid; i < cells * n; i += kLabelThreads) {
                const int cell = i / n, p = i - cell * n;
                const int cy = cell / fw, cx = cell - cy * fw;
                tile[cell * stride + p] = img[((size_t)(fy0 + cy) * w + (fx0 + cx)) * ldc + c0 + p];
            }
            __syncthreads();
            int p = 0;
            for (; p + 4 <= n; p += 4) {
                const float4 a = *reinterpret_cast<const float4*>(p00 + p);
                const float4 bb = *reinterpret_cast<const float4*>(p01 + p);
                const float4 cc = *reinterpret_cast<const float4*>(p10 + p);
                const float4 d = *reinterpret_cast<const float4*>(p11 + p);
                const int c = c0 + p;
                consider(r, blend(w00, w01, w10, w11, a.x, bb.x, cc.x, d.x), class_of ? class_of[c] : c);
                consider(r, blend(w00, w01, w10, w11, a.y, bb.y, cc.y, d.y), class_of ? class_of[c + 1] : c + 1);
                consider(r, blend(w00, w01, w10, w11, a.z, bb.z, cc.z, d.z), class_of ? class_of[c + 2] : c + 2);
                consider(r, blend(w00, w01, w10, w11, a.w, bb.w, cc.w, d.w), class_of ? class_of[c + 3] : c + 3);
            }
            for (; p < n; ++p) {
                const int c = c0 + p;
                consider(r, blend(w00, w01, w10, w11, p00[p], p01[p], p10[p], p11[p]), class_of ? class_of[c] : c);
            }
        }
    } else {
        const float* g00 = img + ((size_t)y0 * w + x0) * ldc;
        const float* g01 = img + ((size_t)y0 * w + x1) * ldc;
        const float* g10 = img + ((size_t)y1 * w + x0) * ldc;
        const float* g11 = img + ((size_t)y1 * w + x1) * ldc;
        for (int c = 0; c < C; ++c)
            consider(r, blend(w00, w01, w10, w11, g00[c], g01[c], g10[c], g11[c]), class_of ? class_of[c] : c);
        __syncthreads();  // hist is zero
    }

    const bool unlabeled = r.best != r.best || r.best < min_score;
    const unsigned label = unlabeled ? kUnlabeled : (unsigned)r.cls;
    const size_t row = ((size_t)b * H + min(y, H - 1)) * W;
    if (valid) {
        if (best_out) best_out[row + x] = r.best;
        if (margin_out) margin_out[row + x] = r.other == r.other ? __fsub_rn(r.best, r.other) : INFINITY;
    }
    if (labels) {
        // four pixels a dword where the row allows it: the quad's first lane stores for its three neighbours
        const unsigned l1 = __shfl_down(label, 1, 64), l2 = __shfl_down(label, 2, 64), l3 = __shfl_down(label, 3, 64);
        const int xq = x & ~3;
        uint8_t* q = labels + row + xq;
        if (y < H && xq + 3 < W && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
            if ((tx & 3) == 0) *reinterpret_cast<uint32_t*>(q) = label | (l1 << 8) | (l2 << 16) | (l3 << 24);
        } else if (valid) {
            labels[row + x] = (uint8_t)label;
        }
    }
    if (counts) {
        if (valid) atomicAdd(&hist[label], 1);
        __syncthreads();
        if (hist[tid] != 0) atomicAdd(&counts[(size_t)b * 256 + tid], hist[tid]);
    }
}

__global__ __launch_bounds__(256) void k_zero_counts(int32_t* __restrict__ counts) {
    counts[(size_t)blockIdx.x * 256 + threadIdx.x] = 0;
}

// ---------------------------------------------------------------------------------------------------------
// k_map_class_scores: a workgroup owns kScoreCells consecutive cells of one image and kScorePrompts prompts; lane = cell,
// and each of the four waves carries kScorePrompts / 4 float64 accumulators (prompts wave, wave + 4, ...).  The
// embedding axis passes through LDS kScoreDepth channels at a time: the map tile as [channel][cell], read from the
// [E][S] map with the cells of a channel contiguous, and the vectors as [prompt][channel], which a wave reads at one
// address.  Every lane also carries the chains of its prompts' squared norms (the same for all lanes).  The results
// leave through LDS so that a cell's prompts are stored contiguously.
constexpr int kScoreCells = 64;
constexpr int kScorePrompts = 32;
constexpr int kScoreDepth = 32;
constexpr int kScorePerWave = kScorePrompts / 4;

__global__ __launch_bounds__(256) void k_map_class_scores(const float* __restrict__ maps, int E, int S,
                                                          const float* __restrict__ vectors, int C, int64_t ldv,
                                                          float* __restrict__ out, int64_t ldc) {
    __shared__ float mt[kScoreDepth][kScoreCells];
    __shared__ float vt[kScorePrompts][kScoreDepth + 1];
    __shared__ float ot[kScoreCells][kScorePrompts + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = blockIdx.x * kScoreCells, c0 = blockIdx.y * kScorePrompts, b = blockIdx.z;
    const float* m = maps + (size_t)b * E * S;
    double acc[kScorePerWave], nrm[kScorePerWave];
#pragma unroll
    for (int j = 0; j < kScorePerWave; ++j) acc[j] = nrm[j] = 0.0;

    for (int e0 = 0; e0 < E; e0 += kScoreDepth) {
        const int ne = min(kScoreDepth, E - e0);
        __syncthreads();
        for (int i = tid; i < kScoreDepth * kScoreCells; i += 256) {
            const int e = i / kScoreCells, s = i - e * kScoreCells;
            mt[e][s] = (e < ne && s0 + s < S) ? m[(size_t)(e0 + e) * S + s0 + s] : 0.f;
        }
        for (int i = tid; i < kScorePrompts * kScoreDepth; i += 256) {
            const int c = i / kScoreDepth, e = i - c * kScoreDepth;
            vt[c][e] = (e < ne && c0 + c < C) ? vectors[(size_t)(c0 + c) * ldv + e0 + e] : 0.f;
        }
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const double mv = (double)mt[e][lane];
#pragma unroll
            for (int j = 0; j < kScorePerWave; ++j) {
                const double tv = (double)vt[wave + 4 * j][e];
                acc[j] = __fma_rn(mv, tv, acc[j]);
                nrm[j] = __fma_rn(tv, tv, nrm[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kScorePerWave; ++j) {
        const double denom = fmax(__dsqrt_rn(nrm[j]), 1e-12);
        ot[lane][wave + 4 * j] = (float)__ddiv_rn(acc[j], denom);
    }
    __syncthreads();
    for (int i = tid; i < kScoreCells * kScorePrompts; i += 256) {
        const int s = i / kScorePrompts, c = i - s * kScorePrompts;
        if (s0 + s < S && c0 + c < C) out[((size_t)b * S + s0 + s) * ldc + c0 + c] = ot[s][c];
    }
}

}  // namespace

extern "C" int isc_label_map_geometry(int* tile_w, int* tile_h, int* prompt_chunk) {
    ISC_REQUIRE(tile_w && tile_h && prompt_chunk);
    *tile_w = kTileW;
    *tile_h = kTileH;
    *prompt_chunk = kPromptChunk;
    return ISC_OK;
}

extern "C" int isc_label_map(const float* scores, int B, int h, int w, int C, int64_t ldc, const int32_t* class_of, int H,
                             int W, float min_score, uint8_t* labels, float* best, float* margin, int32_t* counts,
                             void* stream) {
    ISC_REQUIRE(B >= 0 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C >= 1 && ldc >= C);
    ISC_REQUIRE(min_score == min_score);
    if (C > kMaxPrompts) return ISC_ERR_UNSUPPORTED;
    if ((int64_t)h * w >= (int64_t)1 << 31 || (int64_t)H * W >= (int64_t)1 << 31) return ISC_ERR_UNSUPPORTED;
    const int tiles_y = isc_ceil_div(H, kTileH);
    if (tiles_y > 65535 || B > 65535) return ISC_ERR_UNSUPPORTED;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(scores && (labels || best));
    if (!isc_aligned(scores, 16) || !isc_aligned(best, 4) || !isc_aligned(margin, 4) || !isc_aligned(counts, 4) ||
        !isc_aligned(class_of, 4))
        return ISC_ERR_ALIGNMENT;
    hipStream_t s = isc_stream(stream);
    if (counts) {  // a launch of its own ahead of the histogram's atomics: a kernel node when the stream is captured
        hipLaunchKernelGGL(k_zero_counts, dim3(B), dim3(256), 0, s, counts);
        if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH;
    }
    const dim3 grid(isc_ceil_div(W, kTileW), tiles_y, B);
    hipLaunchKernelGGL(k_label_map, grid, dim3(kLabelThreads), 0, s, scores, ldc, class_of, C, h, w, H, W,
                       (float)h / (float)H, (float)w / (float)W, min_score, labels, best, margin, counts);
    return isc_launch_status();
}

extern "C" int isc_map_class_scores(const float* maps, int B, int E, int S, const float* vectors, int C, int64_t ldv,
                                    float* out, int64_t ldc, void* stream) {
    ISC_REQUIRE(B >= 0 && E >= 1 && S >= 1 && C >= 1 && ldv >= E && ldc >= C);
    const int blocks_c = isc_ceil_div(C, kScorePrompts);
    if (blocks_c > 65535 || B > 65535) return ISC_ERR_UNSUPPORTED;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(maps && vectors && out);
    if (!isc_aligned(maps, 4) || !isc_aligned(vectors, 4) || !isc_aligned(out, 4)) return ISC_ERR_ALIGNMENT;
    const dim3 grid(isc_ceil_div(S, kScoreCells), blocks_c, B);
    hipLaunchKernelGGL(k_map_class_scores, grid, dim3(256), 0, isc_stream(stream), maps, E, S, vectors, C, ldv, out, ldc);
    return isc_launch_status();
}
