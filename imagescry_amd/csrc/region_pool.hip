// isc_region_cell_weights / isc_region_pool: mask-pooled vectors per region (include/imagescry_hip.h has the
// definitions, which the tests hold these kernels to bit for bit).
//
// Bilinear upsampling is linear, so the sum of the upsampled map over a region's pixels is a weighted sum over CELLS,
// and with the taps written as rationals over 2L the weights are integers:
//
//   k_region_weights  a workgroup owns a 64 x 16 tile of pixels, a wave one row of it a round.  Along a row the pixels
//                     of one (region, left column cell) are a run of lanes: a wave prefix sum gives the run's column
//                     weights, its last lane multiplies them with the row's two row weights and adds the (at most) four
//                     products to an LDS table keyed by (region, cell) -- ds_add_u64 behind a compare-and-swap on the key.
//                     What finds no slot in a few probes goes to memory directly.  After a barrier every used slot is ONE
//                     global 64-bit integer atomic: a region that fills the image costs a handful per tile, not four
//                     per pixel.  Integer sums only: the order in which they land does not matter.
//   k_region_pool     a workgroup per (image, region) row: the row's mass, then per block of 256 embedding dimensions a
//                     scan of the weight row that compacts the non-zero (cell, weight) pairs into LDS in ascending cell
//                     order, stages the gathered cells of the NCHW map through LDS (loaded with lanes along the cells,
//                     read with lanes along e) and runs the float64 chains, a lane per e.
#include "isc_common.h"

#include <limits.h>
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------ weights
constexpr int kPoolTileW = 64;
constexpr int kPoolTileH = 16;
constexpr int kPoolThreads = 256;
constexpr int kPoolRounds = kPoolTileW * kPoolTileH / kPoolThreads;  // a wave = one tile row a round
constexpr int kPoolSlots = 1024;                                     // (region, cell) keys a tile combines in LDS
constexpr int kPoolProbes = 8;                                       // slots tried before an add goes to memory
static_assert(kPoolTileW == ISC_WAVE && kPoolThreads == 4 * ISC_WAVE, "a wave owns one tile row a round");
static_assert((kPoolSlots & (kPoolSlots - 1)) == 0 && kPoolSlots % kPoolThreads == 0, "the table is probed with a mask");

constexpr int64_t kPoolMaxPixels = (int64_t)1 << 24;  // H * W: every weight below 4 (HW)^2 = 2^50
constexpr int64_t kPoolMaxTable = (int64_t)1 << 25;   // R * h * w: a (region, cell) key is a non-negative int32

struct AxisTap {
    int i0, i1;
    unsigned w0, w1;  // over 2L: w0 + w1 = 2L
};

// The taps of pixel d of an axis of L pixels over l cells (the header's formulas).  `narrow`: (2L - 1) * l fits 31 bits.
__device__ __forceinline__ AxisTap axis_tap(int d, int L, int l, bool narrow) {
    AxisTap t;
    unsigned f;
    if (narrow) {
        const int n = max((2 * d + 1) * l - L, 0);
        t.i0 = (int)((unsigned)n / (unsigned)(2 * L));
        f = (unsigned)n - (unsigned)t.i0 * (unsigned)(2 * L);
    } else {
        const int64_t n = max((int64_t)(2 * d + 1) * l - L, (int64_t)0);
        t.i0 = (int)(n / (2 * (int64_t)L));
        f = (unsigned)(n - (int64_t)t.i0 * (2 * (int64_t)L));
    }
    t.i1 = min(t.i0 + 1, l - 1);
    t.w0 = 2u * (unsigned)L - f;
    t.w1 = f;
    return t;
}

__device__ __forceinline__ void pool_add(int* keys, unsigned long long* vals, unsigned long long* __restrict__ row0, int key,
                                         unsigned long long v) {
    unsigned slot = ((unsigned)key * 2654435761u) >> 22;  // the top 10 bits: kPoolSlots
    static_assert(kPoolSlots == 1 << 10, "the hash keeps log2(kPoolSlots) bits");
#pragma unroll 1
    for (int probe = 0; probe < kPoolProbes; ++probe) {
        const int old = atomicCAS(&keys[slot], -1, key);
        if (old == -1 || old == key) {
            atomicAdd(&vals[slot], v);
            return;
        }
        slot = (slot + 1) & (kPoolSlots - 1);
    }
    atomicAdd(row0 + key, v);
}

// The table before the atomics: a launch of its own, which a captured graph replays like every other launch of the call.
__global__ __launch_bounds__(256) void k_region_zero(unsigned long long* __restrict__ weights, size_t n) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) weights[i] = 0;
}

// grid (tiles_x * tiles_y, B).  weights is zero on entry.
__global__ __launch_bounds__(kPoolThreads) void k_region_weights(const int32_t* __restrict__ ids, int H, int W, int h, int w,
                                                                 int R, int tiles_x, int narrow_y, int narrow_x,
                                                                 unsigned long long* __restrict__ weights) {
    __shared__ int keys[kPoolSlots];
    __shared__ unsigned long long vals[kPoolSlots];
    const int tid = threadIdx.x, lx = tid & 63;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int X0 = tx * kPoolTileW, Y0 = ty * kPoolTileH;
    const int S = h * w;
    const int32_t* img = ids + (size_t)blockIdx.y * H * W;
    unsigned long long* row0 = weights + (size_t)blockIdx.y * R * S;  // + key = the image's (region, cell) entry
#pragma unroll
    for (int k = 0; k < kPoolSlots / kPoolThreads; ++k) {
        keys[k * kPoolThreads + tid] = -1;
        vals[k * kPoolThreads + tid] = 0;
    }
    __syncthreads();
    const int x = X0 + lx;
    const AxisTap cx = axis_tap(min(x, W - 1), W, w, narrow_x != 0);
#pragma unroll 1
    for (int k = 0; k < kPoolRounds; ++k) {
        const int y = Y0 + k * (kPoolThreads / kPoolTileW) + (tid >> 6);  // one row a wave: uniform in the wave
        if (y >= H) continue;                                             // the whole wave
        int r = -1;
        if (x < W) {
            r = img[(size_t)y * W + x];
            if (r >= R) r = -1;
        }
        // runs of one (region, left cell) along the row; a skipped pixel (r = -1) ends a run and starts none that adds
        const int left_r = __shfl_up(r, 1, 64), left_j = __shfl_up(cx.i0, 1, 64);
        const unsigned long long starts = __ballot(lx == 0 || left_r != r || left_j != cx.i0);
        const int start = 63 - __builtin_clzll(starts & (~0ull >> (63 - lx)));  // bit 0 is set: never zero
        const bool last = lx == 63 || ((starts >> (lx + 1)) & 1);
        unsigned incl = cx.w1;  // at most 2W <= 2^25 a lane: 64 of them fit 32 bits
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)incl, off, 64);
            if (lx >= off) incl += up;
        }
        const unsigned before = (unsigned)__shfl((int)incl, max(start - 1, 0), 64);
        if (r < 0 || !last) continue;
        const unsigned n = (unsigned)(lx - start + 1);
        unsigned s1 = incl - (start > 0 ? before : 0u);       // the run's weight on column cell i1
        unsigned s0 = n * 2u * (unsigned)W - s1;              // ... and on i0
        if (cx.i1 == cx.i0) {
            s0 += s1;
            s1 = 0;
        }
        const AxisTap cy = axis_tap(y, H, h, narrow_y != 0);
        unsigned wy0 = cy.w0, wy1 = cy.w1;
        if (cy.i1 == cy.i0) {
            wy0 += wy1;
            wy1 = 0;
        }
        const int at = r * S;
        pool_add(keys, vals, row0, at + cy.i0 * w + cx.i0, (unsigned long long)wy0 * s0);  // wy0, s0 >= 1
        if (s1) pool_add(keys, vals, row0, at + cy.i0 * w + cx.i1, (unsigned long long)wy0 * s1);
        if (wy1) {
            pool_add(keys, vals, row0, at + cy.i1 * w + cx.i0, (unsigned long long)wy1 * s0);
            if (s1) pool_add(keys, vals, row0, at + cy.i1 * w + cx.i1, (unsigned long long)wy1 * s1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPoolSlots / kPoolThreads; ++k) {
        const int key = keys[k * kPoolThreads + tid];
        if (key >= 0) atomicAdd(row0 + key, vals[k * kPoolThreads + tid]);
    }
}

// --------------------------------------------------------------------------------------------------------------- pool
constexpr int kPoolDims = 256;    // embedding dimensions a pass over the weight row serves: a lane each
constexpr int kPoolCells = 16;    // gathered cells staged at a time
constexpr int kPoolKeep = 1024;   // sums kept in LDS for the unit norm; a longer row is summed a second time
static_assert(kPoolDims == kPoolThreads, "a thread owns one embedding dimension of a block");

struct PoolShared {
    float stage[kPoolDims][kPoolCells + 1];  // [e][cell], a row padded to 17 words: reads along e hit 64 banks
    int cell[kPoolThreads];
    double weight[kPoolThreads];
    double sum[kPoolKeep];
    unsigned long long wave_mass[4];
    int wave_count[4];
    double norm2;
};

// The non-zero weights of cells [c0, c0 + 256) of the row, compacted in ascending cell order -> their number.
__device__ __forceinline__ int pool_compact(PoolShared& sh, const long long* __restrict__ wrow, int c0, int S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = c0 + tid;
    const long long wt = c < S ? wrow[c] : 0;
    const unsigned long long set = __ballot(wt != 0);
    __syncthreads();  // the pairs and counts of the chunk before are consumed
    if (lane == 0) sh.wave_count[wave] = __popcll(set);
    __syncthreads();
    int at = __popcll(set & ((1ull << lane) - 1)), total = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (v < wave) at += sh.wave_count[v];
        total += sh.wave_count[v];
    }
    if (wt != 0) {
        sh.cell[at] = c;
        sh.weight[at] = (double)wt;
    }
    return total;  // the pairs are visible behind the next barrier
}

// s[e] of the header for e = e0 + threadIdx.x: the chain over the row's non-zero cells, ascending.
__device__ __forceinline__ double pool_chain(PoolShared& sh, const float* __restrict__ map, const long long* __restrict__ wrow,
                                             int e0, int E, int S) {
    const int tid = threadIdx.x;
    double acc = 0.0;
#pragma unroll 1
    for (int c0 = 0; c0 < S; c0 += kPoolThreads) {
        const int count = pool_compact(sh, wrow, c0, S);
#pragma unroll 1
        for (int k0 = 0; k0 < count; k0 += kPoolCells) {
            __syncthreads();  // the pairs are written; the stage before is consumed
            const int cells = min(count - k0, kPoolCells);
#pragma unroll
            for (int it = 0; it < kPoolDims * kPoolCells / kPoolThreads; ++it) {
                const int idx = it * kPoolThreads + tid, k = idx & (kPoolCells - 1), el = idx / kPoolCells;
                if (k < cells && e0 + el < E) sh.stage[el][k] = map[(size_t)(e0 + el) * S + sh.cell[k0 + k]];
            }
            __syncthreads();
            if (e0 + tid < E)
                for (int k = 0; k < cells; ++k) acc = fma(sh.weight[k0 + k], (double)sh.stage[tid][k], acc);
        }
    }
    return acc;
}

// grid (R, B).
__global__ __launch_bounds__(kPoolThreads) void k_region_pool(const float* __restrict__ maps, int E, int S,
                                                              const long long* __restrict__ weights, int R, int mode,
                                                              float* __restrict__ out, long long* __restrict__ mass_out) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)blockIdx.y * R + blockIdx.x;
    const long long* wrow = weights + row * S;
    const float* map = maps + (size_t)blockIdx.y * E * S;
    float* orow = out + row * E;

    unsigned long long part = 0;
    for (int c = tid; c < S; c += kPoolThreads) part += (unsigned long long)wrow[c];
    part = isc_wave_sum(part);
    if (lane == 0) sh.wave_mass[wave] = part;
    __syncthreads();
    const long long mass = (long long)(sh.wave_mass[0] + sh.wave_mass[1] + sh.wave_mass[2] + sh.wave_mass[3]);
    if (mass_out && tid == 0) mass_out[row] = mass;
    if (mass == 0) {
        for (int e = tid; e < E; e += kPoolThreads) orow[e] = 0.f;
        return;
    }
    if (mode == ISC_POOL_MEAN) {
        const double m = (double)mass;
        for (int e0 = 0; e0 < E; e0 += kPoolDims) {
            const double s = pool_chain(sh, map, wrow, e0, E, S);
            if (e0 + tid < E) orow[e0 + tid] = (float)__ddiv_rn(s, m);
        }
        return;
    }
    // ISC_POOL_UNIT: n is ONE chain over e, so a block's sums go through LDS to thread 0, which continues it
    const bool keep = E <= kPoolKeep;
    double n = 0.0;
    for (int e0 = 0; e0 < E; e0 += kPoolDims) {
        const double s = pool_chain(sh, map, wrow, e0, E, S);
        __syncthreads();  // a longer row: the block before is consumed
        if (e0 + tid < E) sh.sum[keep ? e0 + tid : tid] = s;
        __syncthreads();
        if (tid == 0) {
            const double* v = sh.sum + (keep ? e0 : 0);
            const int m = min(E - e0, kPoolDims);
            for (int e = 0; e < m; ++e) n = fma(v[e], v[e], n);
        }
    }
    if (tid == 0) sh.norm2 = n;
    __syncthreads();
    n = sh.norm2;
    if (n == 0.0) {
        for (int e = tid; e < E; e += kPoolThreads) orow[e] = 0.f;
        return;
    }
    const double norm = __dsqrt_rn(n);
    if (keep) {
        for (int e = tid; e < E; e += kPoolThreads) orow[e] = (float)__ddiv_rn(sh.sum[e], norm);
        return;
    }
    for (int e0 = 0; e0 < E; e0 += kPoolDims) {  // the same chains again: the same bits
        const double s = pool_chain(sh, map, wrow, e0, E, S);
        if (e0 + tid < E) orow[e0 + tid] = (float)__ddiv_rn(s, norm);
    }
}

// The limits both entry points share (h * w as S): everything but the pixels.
int pool_table_status(int B, int64_t S, int R) {
    ISC_REQUIRE(B >= 0 && S >= 1 && R >= 1);
    if (S >= (int64_t)1 << 31 || (int64_t)R * S > kPoolMaxTable || B > 65535) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

}  // namespace

extern "C" int isc_region_pool_geometry(int* tile_w, int* tile_h) {
    ISC_REQUIRE(tile_w && tile_h);
    *tile_w = kPoolTileW;
    *tile_h = kPoolTileH;
    return ISC_OK;
}

extern "C" int isc_region_cell_weights(const int32_t* ids, int B, int H, int W, int h, int w, int R, int64_t* weights,
                                       void* stream) {
    ISC_REQUIRE(H >= 1 && W >= 1 && h >= 1 && w >= 1);
    if ((int64_t)H * W > kPoolMaxPixels) return ISC_ERR_UNSUPPORTED;
    const int table = pool_table_status(B, (int64_t)h * w, R);
    if (table != ISC_OK) return table;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(ids && weights);
    if (!isc_aligned(ids, 4) || !isc_aligned(weights, 8)) return ISC_ERR_ALIGNMENT;

    hipStream_t s = isc_stream(stream);
    unsigned long long* cells = reinterpret_cast<unsigned long long*>(weights);
    const size_t entries = (size_t)B * R * h * w;
    const size_t zero_blocks = isc_ceil_div(entries, (size_t)1024);  // four stores a thread, up to 2^20 workgroups
    hipLaunchKernelGGL(k_region_zero, dim3((unsigned)(zero_blocks < ((size_t)1 << 20) ? zero_blocks : (size_t)1 << 20)),
                       dim3(256), 0, s, cells, entries);
    if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH;
    const int tiles_x = isc_ceil_div(W, kPoolTileW), tiles_y = isc_ceil_div(H, kPoolTileH);  // at most 2^24 / 16 + 1 tiles
    const int narrow_y = (2 * (int64_t)H - 1) * h <= INT_MAX, narrow_x = (2 * (int64_t)W - 1) * w <= INT_MAX;
    hipLaunchKernelGGL(k_region_weights, dim3(tiles_x * tiles_y, B), dim3(kPoolThreads), 0, s, ids, H, W, h, w, R, tiles_x,
                       narrow_y, narrow_x, cells);
    return isc_launch_status();
}

extern "C" int isc_region_pool(const float* maps, int B, int E, int S, const int64_t* weights, int R, int mode, float* out,
                               int64_t* mass, void* stream) {
    ISC_REQUIRE(E >= 1);
    ISC_REQUIRE(mode == ISC_POOL_UNIT || mode == ISC_POOL_MEAN);
    const int table = pool_table_status(B, S, R);
    if (table != ISC_OK) return table;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(maps && weights && out);
    if (!isc_aligned(maps, 4) || !isc_aligned(weights, 8) || !isc_aligned(out, 4) || !isc_aligned(mass, 8))
        return ISC_ERR_ALIGNMENT;
    hipLaunchKernelGGL(k_region_pool, dim3(R, B), dim3(kPoolThreads), 0, isc_stream(stream), maps, E, S,
                       reinterpret_cast<const long long*>(weights), R, mode, out, reinterpret_cast<long long*>(mass));
    return isc_launch_status();
}
