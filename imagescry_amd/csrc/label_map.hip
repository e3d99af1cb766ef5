// isc_label_map, isc_label_map_windows, isc_map_class_scores: dense patch scores -> pixel label maps
// (include/imagescry_hip.h has the arithmetic, which the tests hold these kernels to bit for bit).
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

// What leaves a pixel (steps 6 - 7 and the stores): thread `tid` of the tile holds the choice `r` of pixel (y, x) of image
// b; a thread outside the image holds a copy of the last pixel of its row / column and stores nothing.  `hist` is the
// workgroup's 256 zeroed counters; every thread of the workgroup calls this.
__device__ __forceinline__ void publish(const Running& r, float min_score, int b, int H, int W, int x, int y, int tid,
                                        uint8_t* __restrict__ labels, float* __restrict__ best_out,
                                        float* __restrict__ margin_out, int32_t* __restrict__ counts, int* hist) {
    const int tx = tid & (kTileW - 1);
    const bool valid = x < W && y < H;
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

    publish(r, min_score, b, H, W, x, y, tid, labels, best_out, margin_out, counts, hist);
}

__global__ __launch_bounds__(256) void k_zero_counts(int32_t* __restrict__ counts) {
    counts[(size_t)blockIdx.x * 256 + threadIdx.x] = 0;
}

// ---------------------------------------------------------------------------------------------------------
// The window grid of isc_label_map_windows along one axis of length L (include/imagescry_hip.h), host and device.
__host__ __device__ inline int window_count(int L, int win, int stride) {
    const int over = L - win + stride - 1;
    return (over > 0 ? over : 0) / stride + 1;
}

__host__ __device__ inline int window_start(int i, int L, int win, int stride) {
    const int s = i * stride;
    return s < L - win ? s : L - win;
}

// The windows [lo, hi] that meet the pixels a .. b_ (a pixel: a == b_): start_i <= b_ and start_i + win > a.  Starts and
// ends both ascend with i, so they are a range; it is not empty, every pixel being covered.  Only the last window's start
// is not i * stride: it lies at L - win, at or before (n - 1) * stride.
__host__ __device__ inline void windows_over(int a, int b_, int L, int win, int stride, int n, int& lo, int& hi) {
    hi = b_ >= L - win ? n - 1 : b_ / stride;
    const int t = a - win + 1;
    const int first = t <= 0 ? 0 : (t + stride - 1) / stride;
    lo = first < n - 1 ? first : n - 1;
}

struct WindowGrid {
    int H, W, win_h, win_w, stride_y, stride_x, ny, nx;
};

// ---------------------------------------------------------------------------------------------------------
// k_label_map_windows: k_label_map's tile (a workgroup 64 x 4 pixels of one image, a thread one pixel), but a pixel's
// value for a prompt is the average of its blends in every window that covers it.  The windows a tile meets are a range
// per axis, uniform over the workgroup; a pixel's own covering windows are a sub-range per axis, i major.
//   Staged path (no pixel of the tile in more than kMaxCover windows, at most kMaxAxisWindows windows an axis, all
// footprints together at most kLdsFloats / (4 + kPad) cells): the tile's footprint in each window is a rectangle, rows x
// columns separately, so the footprints of all windows form one virtual grid -- the row ranges of the tile's window rows
// one below the other, the column ranges side by side -- held in LDS as [cell][chunk + kPad] like k_label_map's.  `src`
// maps a virtual cell to its cell in the image's [ny][nx][h][w] scores once; a chunk is then staged with kPromptChunk
// lanes a cell (no division).  A thread keeps tap offsets and weights of its up to kMaxCover windows in registers and
// sums over them inside the prompt loop.
//   Direct path (everything else): a thread walks its covering windows per group of kDirectPrompts prompts, taps
// recomputed per window, cells read from memory; any number of windows.
constexpr int kMaxCover = 4;
constexpr int kMaxAxisWindows = 16;
constexpr int kMaxCells = kLdsFloats / (4 + kPad);
constexpr int kDirectPrompts = 8;
static_assert(kPromptChunk == 32 && kLabelThreads % kPromptChunk == 0, "the staging loop gives a cell 32, 16, 8 or 4 lanes");

__global__ __launch_bounds__(kLabelThreads) void k_label_map_windows(
    const float* __restrict__ scores, int64_t ldc, const int32_t* __restrict__ class_of, int C, int h, int w, WindowGrid g,
    float scale_h, float scale_w, float min_score, uint8_t* __restrict__ labels, float* __restrict__ best_out,
    float* __restrict__ margin_out, int32_t* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float tile[kLdsFloats];
    __shared__ int hist[256];
    __shared__ int src[kMaxCells];
    // per axis (0 = y, 1 = x) and window of the tile: the first cell of the footprint, and where it starts in the virtual
    // grid (entry [count] = the grid's extent)
    __shared__ int first_cell[2][kMaxAxisWindows];
    __shared__ int virt[2][kMaxAxisWindows + 1];
    __shared__ int cover;
    const int tid = threadIdx.x;
    const int tx = tid & (kTileW - 1), ty = tid / kTileW;
    const int X0 = blockIdx.x * kTileW, Y0 = blockIdx.y * kTileH, b = blockIdx.z;
    const int x = X0 + tx, y = Y0 + ty;
    const int Y1 = min(Y0 + kTileH, g.H) - 1, X1 = min(X0 + kTileW, g.W) - 1;
    // a thread outside the image computes the last pixel of its row / column again and stores nothing
    const int yc = min(y, g.H - 1), xc = min(x, g.W - 1);
    hist[tid] = 0;
    if (tid == 0) cover = 0;

    int iy_lo, iy_hi, ix_lo, ix_hi;  // the pixel's windows
    windows_over(yc, yc, g.H, g.win_h, g.stride_y, g.ny, iy_lo, iy_hi);
    windows_over(xc, xc, g.W, g.win_w, g.stride_x, g.nx, ix_lo, ix_hi);
    const int n = (iy_hi - iy_lo + 1) * (ix_hi - ix_lo + 1);
    const float fn = (float)n;
    int wy_lo, wy_hi, wx_lo, wx_hi;  // the tile's windows
    windows_over(Y0, Y1, g.H, g.win_h, g.stride_y, g.ny, wy_lo, wy_hi);
    windows_over(X0, X1, g.W, g.win_w, g.stride_x, g.nx, wx_lo, wx_hi);
    const int nwy = wy_hi - wy_lo + 1, nwx = wx_hi - wx_lo + 1;
    const size_t grid_cells = (size_t)h * w;
    const bool tables = nwy <= kMaxAxisWindows && nwx <= kMaxAxisWindows &&
                        (int64_t)g.ny * g.nx * (int64_t)grid_cells < ((int64_t)1 << 31);

    int unused_i;
    float unused_l0, unused_l1;
    if (tables) {  // wave 0 has the window rows, wave 1 the window columns: the footprint of the tile's part of each
        const int axis = tid >> 6, k = tid & 63;
        if (axis < 2 && k < (axis ? nwx : nwy)) {
            const int L = axis ? g.W : g.H, win = axis ? g.win_w : g.win_h, stride = axis ? g.stride_x : g.stride_y;
            const int T0 = axis ? X0 : Y0, T1 = axis ? X1 : Y1, cells = axis ? w : h;
            const float scale = axis ? scale_w : scale_h;
            const int s = window_start((axis ? wx_lo : wy_lo) + k, L, win, stride);
            int f0, f1;
            bilinear_tap(max(T0, s) - s, scale, cells, f0, unused_i, unused_l0, unused_l1);
            bilinear_tap(min(T1, s + win - 1) - s, scale, cells, unused_i, f1, unused_l0, unused_l1);
            first_cell[axis][k] = f0;
            virt[axis][k + 1] = f1 - f0 + 1;  // the extent; the prefix sum below turns it into the next window's start
        }
    }
    __syncthreads();  // hist and cover are zero, the extents are written
    atomicMax(&cover, n);
    if (tables && (tid == 0 || tid == 64)) {
        const int axis = tid >> 6, count = axis ? nwx : nwy;
        int at = 0;
        virt[axis][0] = 0;
        for (int k = 1; k <= count; ++k) {
            at += virt[axis][k];
            virt[axis][k] = at;
        }
    }
    __syncthreads();
    const int most = cover;
    const int fw = tables ? virt[1][nwx] : 0;
    const int64_t cells64 = tables ? (int64_t)virt[0][nwy] * fw : 0;
    const int chunk = tables && most <= kMaxCover && cells64 <= kMaxCells
                          ? min(kPromptChunk, (kLdsFloats / (int)cells64 - kPad) & ~3)
                          : 0;

    const float* img = scores + (size_t)b * g.ny * g.nx * grid_cells * ldc;
    Running r;
    r.best = r.other = __builtin_nanf("");
    r.cls = class_of ? class_of[0] : 0;

    if (chunk > 0) {
        const int cells = (int)cells64;
        const int stride = chunk + kPad;
        for (int cell = tid; cell < cells; cell += kLabelThreads) {
            const int vy = cell / fw, vx = cell - vy * fw;
            int ky = 0, kx = 0;
            while (vy >= virt[0][ky + 1]) ++ky;
            while (vx >= virt[1][kx + 1]) ++kx;
            const int cy = first_cell[0][ky] + vy - virt[0][ky], cx = first_cell[1][kx] + vx - virt[1][kx];
            src[cell] = ((wy_lo + ky) * g.nx + wx_lo + kx) * (int)grid_cells + cy * w + cx;
        }
        // the thread's windows, i major: where its four taps lie in the tile (in floats) and their weights
        int o00[kMaxCover], o01[kMaxCover], o10[kMaxCover], o11[kMaxCover];
        float w00[kMaxCover], w01[kMaxCover], w10[kMaxCover], w11[kMaxCover];
        int iy = iy_lo, ix = ix_lo;
#pragma unroll
        for (int k = 0; k < kMaxCover; ++k) {
            o00[k] = o01[k] = o10[k] = o11[k] = 0;
            w00[k] = w01[k] = w10[k] = w11[k] = 0.f;
            if (k < n) {
                int y0, y1, x0, x1;
                float ly0, ly1, lx0, lx1;
                bilinear_tap(yc - window_start(iy, g.H, g.win_h, g.stride_y), scale_h, h, y0, y1, ly0, ly1);
                bilinear_tap(xc - window_start(ix, g.W, g.win_w, g.stride_x), scale_w, w, x0, x1, lx0, lx1);
                w00[k] = __fmul_rn(ly0, lx0), w01[k] = __fmul_rn(ly0, lx1);
                w10[k] = __fmul_rn(ly1, lx0), w11[k] = __fmul_rn(ly1, lx1);
                const int ky = iy - wy_lo, kx = ix - wx_lo;
                const int row0 = (virt[0][ky] + y0 - first_cell[0][ky]) * fw, row1 = (virt[0][ky] + y1 - first_cell[0][ky]) * fw;
                const int col0 = virt[1][kx] + x0 - first_cell[1][kx], col1 = virt[1][kx] + x1 - first_cell[1][kx];
                o00[k] = (row0 + col0) * stride, o01[k] = (row0 + col1) * stride;
                o10[k] = (row1 + col0) * stride, o11[k] = (row1 + col1) * stride;
                if (++ix > ix_hi) {
                    ix = ix_lo;
                    ++iy;
                }
            }
        }
        // staging: 32, 16, 8 or 4 lanes a cell, whichever holds the chunk
        const int shift = chunk > 16 ? 5 : chunk > 8 ? 4 : chunk > 4 ? 3 : 2;
        const int lane_p = tid & ((1 << shift) - 1), lane_cell = tid >> shift, cells_a_pass = kLabelThreads >> shift;
        for (int c0 = 0; c0 < C; c0 += chunk) {
            const int np = min(chunk, C - c0);
            __syncthreads();  // the previous chunk is consumed (and, the first time, src is written)
            if (lane_p < np)
                for (int cell = lane_cell; cell < cells; cell += cells_a_pass)
                    tile[cell * stride + lane_p] = img[(size_t)src[cell] * ldc + c0 + lane_p];
            __syncthreads();
            int p = 0;
            for (; p + 4 <= np; p += 4) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < kMaxCover; ++k) {
                    if (k < most && k < n) {
                        const float4 a = *reinterpret_cast<const float4*>(tile + o00[k] + p);
                        const float4 bb = *reinterpret_cast<const float4*>(tile + o01[k] + p);
                        const float4 cc = *reinterpret_cast<const float4*>(tile + o10[k] + p);
                        const float4 d = *reinterpret_cast<const float4*>(tile + o11[k] + p);
                        const float ux = blend(w00[k], w01[k], w10[k], w11[k], a.x, bb.x, cc.x, d.x);
                        const float uy = blend(w00[k], w01[k], w10[k], w11[k], a.y, bb.y, cc.y, d.y);
                        const float uz = blend(w00[k], w01[k], w10[k], w11[k], a.z, bb.z, cc.z, d.z);
                        const float uw = blend(w00[k], w01[k], w10[k], w11[k], a.w, bb.w, cc.w, d.w);
                        if (k == 0) {
                            acc = make_float4(ux, uy, uz, uw);
                        } else {
                            acc.x = __fadd_rn(acc.x, ux), acc.y = __fadd_rn(acc.y, uy);
                            acc.z = __fadd_rn(acc.z, uz), acc.w = __fadd_rn(acc.w, uw);
                        }
                    }
                }
                const int c = c0 + p;
                consider(r, __fdiv_rn(acc.x, fn), class_of ? class_of[c] : c);
                consider(r, __fdiv_rn(acc.y, fn), class_of ? class_of[c + 1] : c + 1);
                consider(r, __fdiv_rn(acc.z, fn), class_of ? class_of[c + 2] : c + 2);
                consider(r, __fdiv_rn(acc.w, fn), class_of ? class_of[c + 3] : c + 3);
            }
            for (; p < np; ++p) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < kMaxCover; ++k) {
                    if (k < most && k < n) {
                        const float u = blend(w00[k], w01[k], w10[k], w11[k], tile[o00[k] + p], tile[o01[k] + p],
                                              tile[o10[k] + p], tile[o11[k] + p]);
                        acc = k == 0 ? u : __fadd_rn(acc, u);
                    }
                }
                consider(r, __fdiv_rn(acc, fn), class_of ? class_of[c0 + p] : c0 + p);
            }
        }
    } else {
        for (int c0 = 0; c0 < C; c0 += kDirectPrompts) {
            float acc[kDirectPrompts] = {};
            bool later = false;
            for (int iy = iy_lo; iy <= iy_hi; ++iy) {
                int y0, y1, x0, x1;
                float ly0, ly1, lx0, lx1;
                bilinear_tap(yc - window_start(iy, g.H, g.win_h, g.stride_y), scale_h, h, y0, y1, ly0, ly1);
                for (int ix = ix_lo; ix <= ix_hi; ++ix) {
                    bilinear_tap(xc - window_start(ix, g.W, g.win_w, g.stride_x), scale_w, w, x0, x1, lx0, lx1);
                    const float w00 = __fmul_rn(ly0, lx0), w01 = __fmul_rn(ly0, lx1);
                    const float w10 = __fmul_rn(ly1, lx0), w11 = __fmul_rn(ly1, lx1);
                    const float* win = img + ((size_t)iy * g.nx + ix) * grid_cells * ldc + c0;
                    const float* g00 = win + ((size_t)y0 * w + x0) * ldc;
                    const float* g01 = win + ((size_t)y0 * w + x1) * ldc;
                    const float* g10 = win + ((size_t)y1 * w + x0) * ldc;
                    const float* g11 = win + ((size_t)y1 * w + x1) * ldc;
#pragma unroll
                    for (int j = 0; j < kDirectPrompts; ++j) {
                        if (c0 + j < C) {
                            const float u = blend(w00, w01, w10, w11, g00[j], g01[j], g10[j], g11[j]);
                            acc[j] = later ? __fadd_rn(acc[j], u) : u;
                        }
                    }
                    later = true;
                }
            }
#pragma unroll
            for (int j = 0; j < kDirectPrompts; ++j)
                if (c0 + j < C) consider(r, __fdiv_rn(acc[j], fn), class_of ? class_of[c0 + j] : c0 + j);
        }
    }

    publish(r, min_score, b, g.H, g.W, x, y, tid, labels, best_out, margin_out, counts, hist);
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

namespace {

bool window_grid_ok(int H, int W, int win_h, int win_w, int stride_y, int stride_x) {
    return H >= 1 && W >= 1 && win_h >= 1 && win_w >= 1 && win_h <= H && win_w <= W && stride_y >= 1 && stride_x >= 1 &&
           stride_y <= win_h && stride_x <= win_w;
}

// The most windows on one pixel of an axis: the count only rises at a window's start.
int axis_cover(int L, int win, int stride, int n) {
    int most = 1;
    for (int i = 0; i < n; ++i) {
        const int s = window_start(i, L, win, stride);
        int lo, hi;
        windows_over(s, s, L, win, stride, n, lo, hi);
        if (hi - lo + 1 > most) most = hi - lo + 1;
    }
    return most;
}

}  // namespace

extern "C" int isc_label_map_window_grid(int H, int W, int win_h, int win_w, int stride_y, int stride_x, int* ny, int* nx,
                                         int* max_cover) {
    ISC_REQUIRE(ny && nx && max_cover);
    ISC_REQUIRE(window_grid_ok(H, W, win_h, win_w, stride_y, stride_x));
    *ny = window_count(H, win_h, stride_y);
    *nx = window_count(W, win_w, stride_x);
    const int64_t most = (int64_t)axis_cover(H, win_h, stride_y, *ny) * axis_cover(W, win_w, stride_x, *nx);
    *max_cover = most > INT32_MAX ? INT32_MAX : (int)most;
    return ISC_OK;
}

extern "C" int isc_label_map_windows(const float* scores, int B, int h, int w, int C, int64_t ldc, const int32_t* class_of,
                                     int H, int W, int win_h, int win_w, int stride_y, int stride_x, float min_score,
                                     uint8_t* labels, float* best, float* margin, int32_t* counts, void* stream) {
    ISC_REQUIRE(B >= 0 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C >= 1 && ldc >= C);
    ISC_REQUIRE(window_grid_ok(H, W, win_h, win_w, stride_y, stride_x));
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
    if (counts) {  // as in isc_label_map: a kernel node of its own ahead of the histogram's atomics
        hipLaunchKernelGGL(k_zero_counts, dim3(B), dim3(256), 0, s, counts);
        if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH;
    }
    const WindowGrid g = {H, W, win_h, win_w, stride_y, stride_x, window_count(H, win_h, stride_y),
                          window_count(W, win_w, stride_x)};
    const dim3 grid(isc_ceil_div(W, kTileW), tiles_y, B);
    hipLaunchKernelGGL(k_label_map_windows, grid, dim3(kLabelThreads), 0, s, scores, ldc, class_of, C, h, w, g,
                       (float)h / (float)win_h, (float)w / (float)win_w, min_score, labels, best, margin, counts);
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
