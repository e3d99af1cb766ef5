// isc_overlap_table / isc_overlap_best: two rasters compared (include/imagescry_hip.h has the definitions, which the
// tests hold these kernels to value for value).
//
//   k_overlap       the 2-D histogram of (a-index, b-index) pairs.  A workgroup owns a 64 x 16 tile of pixels, a wave one
//                   row of it a round.  Along a row the pixels of one pair are a run of lanes: a ballot of the run starts
//                   gives every run its length, and its last lane adds the length to an LDS table keyed by
//                   i * (Rb + 1) + j -- ds_add_u32 behind a compare-and-swap on the key.  What finds no slot in a few
//                   probes goes to memory directly.  After a barrier every used slot is ONE global 64-bit integer atomic:
//                   a class that fills the tile costs one, not one per pixel.  An image has at most kOverlapBlocks
//                   workgroups; with more tiles than that a workgroup strides over them and keeps its table.  Integer
//                   sums only: the order in which they land does not matter.
//   k_overlap_best  a workgroup per image.  Row sums first (a wave per row), kept in the upper half of `uni`; then per
//                   chunk of 1024 columns the column sums into LDS (a thread per column) and every row's best column of
//                   the chunk (a wave per row, lanes along the columns, a butterfly of exact comparisons), merged into
//                   the running best that the outputs hold.  A row belongs to one wave throughout.  For axis == 1 the
//                   same code walks the table with the strides swapped.
#include "isc_common.h"

#include <limits.h>

namespace {

// -------------------------------------------------------------------------------------------------------------- table
constexpr int kOverlapTileW = 64;
constexpr int kOverlapTileH = 16;
constexpr int kOverlapThreads = 256;
constexpr int kOverlapRounds = kOverlapTileW * kOverlapTileH / kOverlapThreads;  // a wave = one tile row a round
constexpr int kOverlapSlots = 512;                                               // pairs a workgroup combines in LDS
constexpr int kOverlapProbes = 8;                                                // slots tried before an add goes to memory
constexpr int kOverlapBlocks = 1024;                                             // workgroups an image at the most
static_assert(kOverlapTileW == ISC_WAVE && kOverlapThreads == 4 * ISC_WAVE, "a wave owns one tile row a round");
static_assert((kOverlapSlots & (kOverlapSlots - 1)) == 0 && kOverlapSlots % kOverlapThreads == 0,
              "the table is probed with a mask");

constexpr int64_t kOverlapMaxTable = (int64_t)1 << 25;  // (Ra + 1) * (Rb + 1): a pair's key is a non-negative int32

// A workgroup sees fewer than 2^31 pixels (H * W < 2^31), so its partial counts fit 32 bits.
__device__ __forceinline__ void overlap_add(int* keys, unsigned* vals, unsigned long long* __restrict__ tab, int key,
                                            unsigned n) {
    unsigned slot = ((unsigned)key * 2654435761u) >> 23;  // the top 9 bits: kOverlapSlots
    static_assert(kOverlapSlots == 1 << 9, "the hash keeps log2(kOverlapSlots) bits");
#pragma unroll 1
    for (int probe = 0; probe < kOverlapProbes; ++probe) {
        const int old = atomicCAS(&keys[slot], -1, key);
        if (old == -1 || old == key) {
            atomicAdd(&vals[slot], n);
            return;
        }
        slot = (slot + 1) & (kOverlapSlots - 1);
    }
    atomicAdd(tab + key, (unsigned long long)n);
}

// The table before the atomics: a launch of its own, which a captured graph replays like every other launch of the call.
__global__ __launch_bounds__(256) void k_overlap_zero(unsigned long long* __restrict__ table, size_t n) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) table[i] = 0;
}

// The index of value v on an axis of R regions: v itself in [0, R), else the "none" slot R.
__device__ __forceinline__ int overlap_index(uint8_t v, int R) { return (int)v < R ? (int)v : R; }
__device__ __forceinline__ int overlap_index(int32_t v, int R) { return (unsigned)v < (unsigned)R ? v : R; }

// grid (min(tiles, kOverlapBlocks), B).  image_entries: (Ra + 1) * (Rb + 1) for per-image tables, 0 for one table.
template <typename TA, typename TB>
__global__ __launch_bounds__(kOverlapThreads) void k_overlap(const TA* __restrict__ a, const TB* __restrict__ b, int H, int W,
                                                             int Ra, int Rb, int tiles_x, int tiles, size_t image_entries,
                                                             unsigned long long* __restrict__ table) {
    __shared__ int keys[kOverlapSlots];
    __shared__ unsigned vals[kOverlapSlots];
    const int tid = threadIdx.x, lx = tid & 63;
    const size_t pixel0 = (size_t)blockIdx.y * H * W;
    unsigned long long* tab = table + (size_t)blockIdx.y * image_entries;
#pragma unroll
    for (int k = 0; k < kOverlapSlots / kOverlapThreads; ++k) {
        keys[k * kOverlapThreads + tid] = -1;
        vals[k * kOverlapThreads + tid] = 0;
    }
    __syncthreads();
#pragma unroll 1
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x = tx * kOverlapTileW + lx, Y0 = ty * kOverlapTileH;
#pragma unroll 1
        for (int k = 0; k < kOverlapRounds; ++k) {
            const int y = Y0 + k * (kOverlapThreads / kOverlapTileW) + (tid >> 6);  // one row a wave: uniform in the wave
            if (y >= H) break;                                                      // the whole wave
            int key = -1;
            if (x < W) {
                const size_t p = pixel0 + (size_t)y * W + x;
                key = overlap_index(a[p], Ra) * (Rb + 1) + overlap_index(b[p], Rb);
            }
            // runs of one pair along the row; the lanes past the image's edge (key = -1) are a run that adds nothing
            const int left = __shfl_up(key, 1, 64);
            const unsigned long long starts = __ballot(lx == 0 || left != key);
            const bool last = lx == 63 || ((starts >> (lx + 1)) & 1);
            if (key < 0 || !last) continue;
            const int start = 63 - __builtin_clzll(starts & (~0ull >> (63 - lx)));  // bit 0 is set: never zero
            overlap_add(keys, vals, tab, key, (unsigned)(lx - start + 1));
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kOverlapSlots / kOverlapThreads; ++k) {
        const int key = keys[k * kOverlapThreads + tid];
        if (key >= 0) atomicAdd(tab + key, (unsigned long long)vals[k * kOverlapThreads + tid]);
    }
}

template <typename TA, typename TB>
void overlap_launch(const void* a, const void* b, int B, int H, int W, int Ra, int Rb, size_t image_entries,
                    unsigned long long* table, hipStream_t s) {
    const int tiles_x = isc_ceil_div(W, kOverlapTileW);
    const int tiles = tiles_x * isc_ceil_div(H, kOverlapTileH);  // below H * W / 1024 + H / 16 + W / 64 + 2 < 2^28
    hipLaunchKernelGGL((k_overlap<TA, TB>), dim3(tiles < kOverlapBlocks ? tiles : kOverlapBlocks, B), dim3(kOverlapThreads),
                       0, s, static_cast<const TA*>(a), static_cast<const TB*>(b), H, W, Ra, Rb, tiles_x, tiles,
                       image_entries, table);
}

// --------------------------------------------------------------------------------------------------------------- best
constexpr int kBestThreads = 256;
constexpr int kBestColumns = 1024;  // column sums held in LDS at a time
constexpr int kBestNone = INT_MAX;  // the "column" of a candidate that overlaps nothing: loses every tie

struct BestPick {
    unsigned long long inter, uni;  // inter / uni is the IoU; (0, 1) overlaps nothing
    int at;
};

// Whether `o` beats `p`: the larger IoU by exact cross-multiplication (inter < 2^31, uni < 2^32), then the lower column.
__device__ __forceinline__ bool best_beats(const BestPick& o, const BestPick& p) {
    const unsigned long long lhs = o.inter * p.uni, rhs = p.inter * o.uni;
    return lhs > rhs || (lhs == rhs && o.at < p.at);
}

// grid (B).  Rows r < nr against columns c < nc of the table walked as tab[r * sr + c * sc]; the row sums run over
// sum_c columns and the column sums over sum_r rows (nc / nr, or one more with the "none" slot counted).
__global__ __launch_bounds__(kBestThreads) void k_overlap_best(const long long* __restrict__ tables, size_t image_entries,
                                                               int nr, int nc, size_t sr, size_t sc, int sum_r, int sum_c,
                                                               int* __restrict__ best, long long* __restrict__ inter,
                                                               unsigned long long* __restrict__ uni) {
    __shared__ unsigned long long colsum[kBestColumns];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long* tab = tables + (size_t)blockIdx.x * image_entries;
    best += (size_t)blockIdx.x * nr;
    inter += (size_t)blockIdx.x * nr;
    uni += (size_t)blockIdx.x * nr;

    // area of row r in the upper half of uni[r], the running best's union in the lower: both below 2^32
#pragma unroll 1
    for (int r = wave; r < nr; r += kBestThreads / 64) {
        unsigned long long s = 0;
        for (int c = lane; c < sum_c; c += 64) s += (unsigned long long)tab[r * sr + c * sc];
        s = isc_wave_sum(s);
        if (lane == 0) {
            best[r] = -1;
            inter[r] = 0;
            uni[r] = (s << 32) | 1u;
        }
    }
#pragma unroll 1
    for (int c0 = 0; c0 < nc; c0 += kBestColumns) {
        const int cn = min(kBestColumns, nc - c0);
        __syncthreads();  // the sums of the chunk before are consumed; the first time, the rows' state is written
        for (int c = tid; c < cn; c += kBestThreads) {
            const long long* col = tab + (size_t)(c0 + c) * sc;
            unsigned long long s = 0;
#pragma unroll 4
            for (int r = 0; r < sum_r; ++r) s += (unsigned long long)col[r * sr];
            colsum[c] = s;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = wave; r < nr; r += kBestThreads / 64) {
            unsigned long long state = lane == 0 ? uni[r] : 0;  // lane 0 wrote it, lane 0 reads it
            const unsigned long long area = __shfl(state, 0, 64) >> 32;
            BestPick pick = {0, 1, kBestNone};
            for (int c = lane; c < cn; c += 64) {  // ascending: a later column needs a strictly larger IoU
                const unsigned long long i = (unsigned long long)tab[r * sr + (size_t)(c0 + c) * sc];
                if (i == 0) continue;
                const BestPick here = {i, area + colsum[c] - i, c0 + c};
                if (best_beats(here, pick)) pick = here;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const BestPick other = {__shfl_xor(pick.inter, off, 64), __shfl_xor(pick.uni, off, 64),
                                        __shfl_xor(pick.at, off, 64)};
                if (best_beats(other, pick)) pick = other;
            }
            if (lane == 0 && pick.at != kBestNone) {
                const BestPick held = {(unsigned long long)inter[r], state & 0xffffffffull, best[r] < 0 ? kBestNone : best[r]};
                if (best_beats(pick, held)) {
                    best[r] = pick.at;
                    inter[r] = (long long)pick.inter;
                    uni[r] = (area << 32) | pick.uni;
                }
            }
        }
    }
    // the state becomes the answer: the union of the best pair, or the row's area where there is none
#pragma unroll 1
    for (int r = wave; r < nr; r += kBestThreads / 64) {
        if (lane != 0) continue;
        const unsigned long long state = uni[r];
        uni[r] = best[r] >= 0 ? (state & 0xffffffffull) : (state >> 32);
    }
}

bool overlap_dtype(int dtype) { return dtype == ISC_U8 || dtype == ISC_I32; }

// The limits both entry points share.
int overlap_table_status(int B, int Ra, int Rb) {
    ISC_REQUIRE(B >= 0 && Ra >= 1 && Rb >= 1);
    if (B > 65535 || ((int64_t)Ra + 1) * ((int64_t)Rb + 1) > kOverlapMaxTable) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

}  // namespace

extern "C" int isc_overlap_geometry(int* tile_w, int* tile_h, int* slots) {
    ISC_REQUIRE(tile_w && tile_h && slots);
    *tile_w = kOverlapTileW;
    *tile_h = kOverlapTileH;
    *slots = kOverlapSlots;
    return ISC_OK;
}

extern "C" int isc_overlap_best_geometry(int* columns) {
    ISC_REQUIRE(columns);
    *columns = kBestColumns;
    return ISC_OK;
}

extern "C" int isc_overlap_table(const void* a, int a_dtype, const void* b, int b_dtype, int B, int H, int W, int Ra, int Rb,
                                 int per_image, int accumulate, int64_t* table, void* stream) {
    ISC_REQUIRE(H >= 1 && W >= 1);
    ISC_REQUIRE(overlap_dtype(a_dtype) && overlap_dtype(b_dtype));
    const int limits = overlap_table_status(B, Ra, Rb);
    if (limits != ISC_OK) return limits;
    if ((int64_t)H * W >= (int64_t)1 << 31) return ISC_ERR_UNSUPPORTED;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(a && b && table);
    if (!isc_aligned(a, a_dtype == ISC_I32 ? 4 : 1) || !isc_aligned(b, b_dtype == ISC_I32 ? 4 : 1) || !isc_aligned(table, 8))
        return ISC_ERR_ALIGNMENT;

    hipStream_t s = isc_stream(stream);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(table);
    const size_t image_entries = (size_t)(Ra + 1) * (size_t)(Rb + 1);
    if (!accumulate) {
        const size_t entries = image_entries * (per_image ? (size_t)B : 1);  // at most 2^25 * 65535
        const size_t zero_blocks = isc_ceil_div(entries, (size_t)1024);      // four stores a thread, up to 2^20 workgroups
        hipLaunchKernelGGL(k_overlap_zero, dim3((unsigned)(zero_blocks < ((size_t)1 << 20) ? zero_blocks : (size_t)1 << 20)),
                           dim3(256), 0, s, counts, entries);
        if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH;
    }
    const size_t stride = per_image ? image_entries : 0;
    if (a_dtype == ISC_U8 && b_dtype == ISC_U8)
        overlap_launch<uint8_t, uint8_t>(a, b, B, H, W, Ra, Rb, stride, counts, s);
    else if (a_dtype == ISC_U8)
        overlap_launch<uint8_t, int32_t>(a, b, B, H, W, Ra, Rb, stride, counts, s);
    else if (b_dtype == ISC_U8)
        overlap_launch<int32_t, uint8_t>(a, b, B, H, W, Ra, Rb, stride, counts, s);
    else
        overlap_launch<int32_t, int32_t>(a, b, B, H, W, Ra, Rb, stride, counts, s);
    return isc_launch_status();
}

extern "C" int isc_overlap_best(const int64_t* table, int B, int Ra, int Rb, int axis, int exclude_none, int32_t* best,
                                int64_t* inter, int64_t* uni, void* stream) {
    ISC_REQUIRE(axis == 0 || axis == 1);
    const int limits = overlap_table_status(B, Ra, Rb);
    if (limits != ISC_OK) return limits;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(table && best && inter && uni);
    if (!isc_aligned(table, 8) || !isc_aligned(best, 4) || !isc_aligned(inter, 8) || !isc_aligned(uni, 8))
        return ISC_ERR_ALIGNMENT;
    const size_t image_entries = (size_t)(Ra + 1) * (size_t)(Rb + 1);
    const int nr = axis == 0 ? Ra : Rb, nc = axis == 0 ? Rb : Ra;
    const size_t sr = axis == 0 ? (size_t)Rb + 1 : 1, sc = axis == 0 ? 1 : (size_t)Rb + 1;
    const int none = exclude_none ? 0 : 1;
    hipLaunchKernelGGL(k_overlap_best, dim3(B), dim3(kBestThreads), 0, isc_stream(stream),
                       reinterpret_cast<const long long*>(table), image_entries, nr, nc, sr, sc, nr + none, nc + none, best,
                       reinterpret_cast<long long*>(inter), reinterpret_cast<unsigned long long*>(uni));
    return isc_launch_status();
}
