// isc_rasterize_polygons: ROI polygons burnt onto a pixel grid as region ids (include/imagescry_hip.h has the definition,
// which the tests hold these kernels to value for value).  Integers only: fixed-point vertices, int64 edge functions.
//
//   k_raster_boxes   a wave per ring: the clamped bounding box of its vertices into the workspace.
//   k_rasterize      a workgroup owns a 64 x 16 tile of pixels, a thread one column of four rows of it (a wave = one tile
//                    row a round).  The workgroup walks the image's rings in order -- the loop, the shape boundaries and
//                    every branch around a barrier are uniform -- skips a ring whose box misses the tile, and stages the
//                    others' edges through LDS in chunks of kEdgeChunk: a thread loads one edge, drops it if it cannot
//                    count for any pixel of the tile, and the survivors are compacted with a ballot.  Every thread then
//                    reads the kept edges (one LDS address a wave: a broadcast) and updates, per pixel, the crossing
//                    parity, the winding and the touched flag of the current shape, which live in registers across
//                    chunks and rings; at a shape boundary the covered pixels take the shape's region.  The edge function
//                    is linear, so its value at a pixel's corner costs two 64-bit products a thread and edge; the other
//                    three corners, the centre and the other three rows are additions.
//                    counts: runs of one id along a wave's row go to an LDS table, a used slot to memory once.
#include "isc_common.h"

#include <limits.h>

namespace {

constexpr int kTileW = 64;
constexpr int kTileH = 16;
constexpr int kThreads = 256;
constexpr int kRows = kTileW * kTileH / kThreads;  // pixels a thread: rows wave, wave + 4, .. of the tile
constexpr int kRowStep = kThreads / kTileW;        // rows between two pixels of a thread
constexpr int kEdgeChunk = 256;                    // edges staged at a time: one a thread
constexpr int kCountSlots = 256;                   // region ids a tile combines in LDS
constexpr int kCountProbes = 8;
constexpr int kMaxSide = 32768;
constexpr int kBoxBlocks = 4096;                   // the most workgroups of the box pass: it strides over the rings
static_assert(kTileW == ISC_WAVE && kThreads == 4 * ISC_WAVE, "a wave owns one tile row a round");
static_assert(kEdgeChunk == kThreads, "a thread stages one edge of a chunk");
static_assert(kCountSlots == kThreads && (kCountSlots & (kCountSlots - 1)) == 0, "a thread owns one slot of the table");
static_assert(256 * kMaxSide == ISC_RASTER_MAX_COORD, "every pixel corner is a legal coordinate");

__device__ __forceinline__ int clamp_coord(int q) { return min(max(q, -ISC_RASTER_MAX_COORD), ISC_RASTER_MAX_COORD); }

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// boxes[r] = (min x, min y, max x, max y) of ring r, for the rings of images 0 .. B - 1 that the workspace has room for;
// a ring without vertices gets an empty box (min > max), which misses every tile.
__global__ __launch_bounds__(kThreads) void k_raster_boxes(const int2* __restrict__ vertices,
                                                           const int32_t* __restrict__ ring_start,
                                                           const int32_t* __restrict__ image_start, int B, int64_t capacity,
                                                           int4* __restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    const int64_t first = image_start[0];
    const int64_t last = min((int64_t)image_start[B], capacity);
    const int64_t step = (int64_t)gridDim.x * (kThreads / 64);
    for (int64_t r = first + (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); r < last; r += step) {
        const int s = ring_start[r], e = ring_start[r + 1];
        int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
        for (int i = s + lane; i < e; i += 64) {
            const int2 v = vertices[i];
            const int x = clamp_coord(v.x), y = clamp_coord(v.y);
            x0 = min(x0, x);
            y0 = min(y0, y);
            x1 = max(x1, x);
            y1 = max(y1, y);
        }
        x0 = wave_min(x0);
        y0 = wave_min(y0);
        x1 = wave_max(x1);
        y1 = wave_max(y1);
        if (lane == 0) boxes[r] = make_int4(x0, y0, x1, y1);
    }
}

__global__ __launch_bounds__(256) void k_raster_zero(int32_t* __restrict__ counts, size_t n) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) counts[i] = 0;
}

__device__ __forceinline__ void count_add(int* keys, unsigned* vals, int32_t* __restrict__ row, int key, unsigned n) {
    unsigned slot = ((unsigned)key * 2654435761u) >> 24;  // the top 8 bits: kCountSlots
    static_assert(kCountSlots == 1 << 8, "the hash keeps log2(kCountSlots) bits");
#pragma unroll 1
    for (int probe = 0; probe < kCountProbes; ++probe) {
        const int old = atomicCAS(&keys[slot], -1, key);
        if (old == -1 || old == key) {
            atomicAdd(&vals[slot], n);
            return;
        }
        slot = (slot + 1) & (kCountSlots - 1);
    }
    atomicAdd(row + key, (int)n);
}

// What a thread keeps per pixel for the shape that is open, and the pixel's winner so far.
struct PixelState {
    int parity[kRows], wind[kRows], touched[kRows], winner[kRows];
};

// The staged edges [0, count) against the thread's pixels.  x0 = 256 x, y0 = 256 y of its first row.
template <bool kTouch>
__device__ __forceinline__ void apply_edges(const int4* edges, int count, int x0, int y0, PixelState& px) {
#pragma unroll 1
    for (int k = 0; k < count; ++k) {
        const int4 ed = edges[k];  // (Ax, Ay, Bx, By): one address a wave
        const int dx = ed.z - ed.x, dy = ed.w - ed.y;
        // e at the top-left corner of the first pixel; a row further down adds 256 * kRowStep * dx
        int64_t e00 = (int64_t)dx * (y0 - ed.y) - (int64_t)dy * (x0 - ed.x);
        const int64_t row_step = (int64_t)dx * (256 * kRowStep);
        const int64_t to_centre = ((int64_t)dx - dy) * 128;
        const int ylo = min(ed.y, ed.w), yhi = max(ed.y, ed.w);
        int64_t lo = 0, hi = 0;
        bool in_x = false;
        if (kTouch) {
            lo = min((int64_t)dx * 256, (int64_t)0) + min((int64_t)dy * -256, (int64_t)0);
            hi = max((int64_t)dx * 256, (int64_t)0) + max((int64_t)dy * -256, (int64_t)0);
            in_x = min(ed.x, ed.z) < x0 + 256 && max(ed.x, ed.z) > x0;
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int yq = y0 + j * 256 * kRowStep, cy = yq + 128;
            const int64_t d = e00 + to_centre;
            const bool up = ed.y <= cy && cy < ed.w && d > 0;
            const bool down = ed.w <= cy && cy < ed.y && d < 0;
            px.parity[j] ^= (int)(up || down);
            px.wind[j] += (int)up - (int)down;
            if (kTouch) px.touched[j] |= (int)(in_x && ylo < yq + 256 && yhi > yq && e00 + lo < 0 && e00 + hi > 0);
            e00 += row_step;
        }
    }
}

// grid (tiles_x * tiles_y, B).  `capacity`: the rings that have a box.
template <bool kTouch>
__global__ __launch_bounds__(kThreads) void k_rasterize(const int2* __restrict__ vertices,
                                                        const int32_t* __restrict__ ring_start,
                                                        const int32_t* __restrict__ ring_region,
                                                        const int32_t* __restrict__ image_start, int H, int W, int R,
                                                        int fill_rule, int tiles_x, const int4* __restrict__ boxes,
                                                        int64_t capacity, int32_t* __restrict__ ids,
                                                        int32_t* __restrict__ counts) {
    __shared__ int4 edges[kEdgeChunk];
    __shared__ int wave_count[kThreads / 64];
    __shared__ int keys[kCountSlots];
    __shared__ unsigned vals[kCountSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int X0 = tx * kTileW, Y0 = ty * kTileH;
    const int X1 = min(X0 + kTileW, W), Y1 = min(Y0 + kTileH, H);  // the tile's pixels inside the image
    const int x = X0 + lane, y = Y0 + wave;
    const int b = blockIdx.y;

    // what an edge or a ring must reach to count for a pixel of the tile: the centres, or with kTouch the open squares
    const int left = kTouch ? 256 * X0 : 256 * X0 + 128;    // max x must exceed it
    const int top = kTouch ? 256 * Y0 : 256 * Y0 + 128;     // max y must exceed it
    const int right = kTouch ? 256 * X1 : 256 * X1 - 128;   // kTouch: min x must be below it; else: not above it
    const int bottom = kTouch ? 256 * Y1 : 256 * Y1 - 128;  // the same for min y

    PixelState px;
#pragma unroll
    for (int j = 0; j < kRows; ++j) px.parity[j] = px.wind[j] = px.touched[j] = 0, px.winner[j] = -1;

    const int ring_first = __builtin_amdgcn_readfirstlane(image_start[b]);
    const int ring_last = __builtin_amdgcn_readfirstlane(image_start[b + 1]);
    int open_region = -1;  // the region of the shape whose state the registers hold; -1: none
    int prev_value = 0;
#pragma unroll 1
    for (int r = ring_first; r < ring_last; ++r) {
        const int value = __builtin_amdgcn_readfirstlane(ring_region[r]);
        if (r == ring_first || value != prev_value) {  // a shape ends: its pixels take its region
            if (open_region >= 0) {
#pragma unroll
                for (int j = 0; j < kRows; ++j) {
                    const bool in = (fill_rule == ISC_FILL_NONZERO ? px.wind[j] != 0 : px.parity[j] != 0) || px.touched[j];
                    if (in) px.winner[j] = open_region;
                    px.parity[j] = px.wind[j] = px.touched[j] = 0;
                }
            }
            open_region = -1;
            prev_value = value;
        }
        if (value < 0 || value >= R) continue;
        if (r < capacity) {
            const int4 box = boxes[r];
            const int bx0 = __builtin_amdgcn_readfirstlane(box.x), by0 = __builtin_amdgcn_readfirstlane(box.y);
            const int bx1 = __builtin_amdgcn_readfirstlane(box.z), by1 = __builtin_amdgcn_readfirstlane(box.w);
            // a closed ring adds no crossing parity and no winding to a centre outside its box, and touches no square
            // that its box does not overlap
            const bool miss = bx1 <= left || by1 <= top || (kTouch ? bx0 >= right || by0 >= bottom : bx0 > right || by0 > bottom);
            if (miss) continue;
        }
        open_region = value;
        const int s = __builtin_amdgcn_readfirstlane(ring_start[r]);
        const int e = __builtin_amdgcn_readfirstlane(ring_start[r + 1]);
#pragma unroll 1
        for (int base = s; base < e; base += kEdgeChunk) {
            const int i = base + tid;
            bool keep = false;
            int4 ed = make_int4(0, 0, 0, 0);
            if (i < e) {
                const int2 a = vertices[i], c = vertices[i + 1 < e ? i + 1 : s];
                ed = make_int4(clamp_coord(a.x), clamp_coord(a.y), clamp_coord(c.x), clamp_coord(c.y));
                const int ylo = min(ed.y, ed.w), yhi = max(ed.y, ed.w);
                keep = (ed.x != ed.z || ed.y != ed.w) && yhi > top && (kTouch ? ylo < bottom : ylo <= bottom);
                // the centre rule alone: horizontal edges never count, nor does an edge that is not right of a centre
                if (!kTouch) keep = keep && ed.y != ed.w && max(ed.x, ed.z) > left;
            }
            const unsigned long long kept = __ballot(keep);
            __syncthreads();  // the edges and counts of the chunk before are consumed
            if (lane == 0) wave_count[wave] = __popcll(kept);
            __syncthreads();
            int at = __popcll(kept & ((1ull << lane) - 1)), total = 0;
#pragma unroll
            for (int v = 0; v < kThreads / 64; ++v) {
                if (v < wave) at += wave_count[v];
                total += wave_count[v];
            }
            if (keep) edges[at] = ed;
            __syncthreads();
            apply_edges<kTouch>(edges, total, 256 * x, 256 * y, px);
        }
    }
    if (open_region >= 0) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const bool in = (fill_rule == ISC_FILL_NONZERO ? px.wind[j] != 0 : px.parity[j] != 0) || px.touched[j];
            if (in) px.winner[j] = open_region;
        }
    }

    int32_t* img = ids + (size_t)b * H * W;
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int yy = y + j * kRowStep;
        if (x < W && yy < H) img[(size_t)yy * W + x] = px.winner[j];
    }
    if (!counts) return;  // the whole grid

    int32_t* row = counts + (size_t)b * R;
    keys[tid] = -1;
    vals[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int yy = y + j * kRowStep;
        const int id = x < W && yy < H ? px.winner[j] : -1;
        // runs of one id along the row: the last lane of a run adds its length
        const int left_id = __shfl_up(id, 1, 64);
        const unsigned long long starts = __ballot(lane == 0 || left_id != id);
        const int start = 63 - __builtin_clzll(starts & (~0ull >> (63 - lane)));  // bit 0 is set: never zero
        const bool last = lane == 63 || ((starts >> (lane + 1)) & 1);
        if (id >= 0 && last) count_add(keys, vals, row, id, (unsigned)(lane - start + 1));
    }
    __syncthreads();
    if (keys[tid] >= 0) atomicAdd(row + keys[tid], (int)vals[tid]);
}

int raster_shape_status(int B, int H, int W, int R) {
    ISC_REQUIRE(B >= 0 && H >= 1 && W >= 1 && R >= 1);
    if (H > kMaxSide || W > kMaxSide || (int64_t)H * W >= (int64_t)1 << 31 || B > 65535) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

}  // namespace

extern "C" int isc_rasterize_polygons_geometry(int* tile_w, int* tile_h, int* edge_chunk) {
    ISC_REQUIRE(tile_w && tile_h && edge_chunk);
    *tile_w = kTileW;
    *tile_h = kTileH;
    *edge_chunk = kEdgeChunk;
    return ISC_OK;
}

extern "C" int isc_rasterize_polygons_workspace_bytes(int64_t num_rings, size_t* bytes) {
    ISC_REQUIRE(bytes && num_rings >= 0);
    if (num_rings > INT32_MAX) return ISC_ERR_UNSUPPORTED;  // ring_start holds int32 offsets
    *bytes = sizeof(int4) * (size_t)(num_rings > 0 ? num_rings : 1);
    return ISC_OK;
}

extern "C" int isc_rasterize_polygons(const int32_t* vertices, const int32_t* ring_start, const int32_t* ring_region,
                                      const int32_t* image_start, int B, int H, int W, int R, int fill_rule, int all_touched,
                                      int32_t* ids, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    const int shape = raster_shape_status(B, H, W, R);
    if (shape != ISC_OK) return shape;
    ISC_REQUIRE(fill_rule == ISC_FILL_EVENODD || fill_rule == ISC_FILL_NONZERO);
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(vertices && ring_start && ring_region && image_start && ids);
    if (!workspace || workspace_bytes < sizeof(int4)) return ISC_ERR_WORKSPACE;
    if (!isc_aligned(vertices, 8) || !isc_aligned(ring_start, 4) || !isc_aligned(ring_region, 4) ||
        !isc_aligned(image_start, 4) || !isc_aligned(ids, 4) || !isc_aligned(counts, 4) || !isc_aligned(workspace, 16))
        return ISC_ERR_ALIGNMENT;

    hipStream_t s = isc_stream(stream);
    const int2* verts = reinterpret_cast<const int2*>(vertices);
    int4* boxes = reinterpret_cast<int4*>(workspace);
    const int64_t capacity = (int64_t)(workspace_bytes / sizeof(int4) < (size_t)INT32_MAX ? workspace_bytes / sizeof(int4)
                                                                                         : (size_t)INT32_MAX);
    const int64_t box_blocks = isc_ceil_div(capacity, (int64_t)(kThreads / 64));
    hipLaunchKernelGGL(k_raster_boxes, dim3((unsigned)(box_blocks < kBoxBlocks ? box_blocks : kBoxBlocks)), dim3(kThreads), 0, s,
                       verts, ring_start, image_start, B, capacity, boxes);
    if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH;
    if (counts) {  // a launch of its own ahead of the atomics: a replayed graph starts from zero
        const size_t entries = (size_t)B * R;
        const size_t zero_blocks = isc_ceil_div(entries, (size_t)1024);
        hipLaunchKernelGGL(k_raster_zero, dim3((unsigned)(zero_blocks < ((size_t)1 << 20) ? zero_blocks : (size_t)1 << 20)),
                           dim3(256), 0, s, counts, entries);
        if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH;
    }
    const int tiles_x = isc_ceil_div(W, kTileW), tiles_y = isc_ceil_div(H, kTileH);  // below 2^31 / 1024 + 2^16 tiles
    const dim3 grid(tiles_x * tiles_y, B);
    if (all_touched)
        hipLaunchKernelGGL(k_rasterize<true>, grid, dim3(kThreads), 0, s, verts, ring_start, ring_region, image_start, H, W, R,
                           fill_rule, tiles_x, boxes, capacity, ids, counts);
    else
        hipLaunchKernelGGL(k_rasterize<false>, grid, dim3(kThreads), 0, s, verts, ring_start, ring_region, image_start, H, W, R,
                           fill_rule, tiles_x, boxes, capacity, ids, counts);
    return isc_launch_status();
}
