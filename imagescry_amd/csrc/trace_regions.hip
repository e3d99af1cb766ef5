// isc_trace_regions: a raster of region ids back to polygon rings on the pixel lattice (include/imagescry_hip.h has the
// definition, which the tests hold these kernels to value for value).  Integers only.
//
// A NODE is a corner edge: a boundary edge whose predecessor runs in another direction; its start vertex is a vertex of
// its ring.  Nodes are numbered per image in the order of their edge keys (raster order of the pixel, then the side), so
// the smallest node of a ring is the ring's smallest corner key: its LEADER.
//
//   k_trace_count / k_trace_offsets / k_trace_number
//                     corner edges per chunk of 1024 pixels in raster order, their exclusive scan per image
//                     (-> num_vertices), the first node of every pixel and the key of every node
//   k_trace_link      a thread per node walks its straight run to the next corner and makes itself that node's predecessor
//   k_trace_jump      pointer jumping over the predecessors, ceil(log2(4 H W)) rounds between two buffers: after round k a
//                     node knows the smallest node among itself and the 2^k - 1 nodes behind it, and how far behind it is.
//                     When the window covers the ring that is the leader and the node's place in ring order
//   k_trace_leaders / k_trace_offsets / k_trace_rings
//                     leaders per chunk of 1024 nodes, their scan (-> num_rings), and per ring its length and order key
//   k_trace_rank      an image that fits: the place of each of its (at most N) rings by counting the smaller keys
//   k_trace_starts    ring_start (a scan of the lengths in ring order), the unused rows, image_start, area2 = 0
//   k_trace_write     a thread per node: its vertex into its ring's slot, its term of area2 with a 64-bit integer atomic
//
// Every launch reads only what an earlier launch wrote; no thread waits for another.
#include "isc_common.h"

#include <limits.h>

namespace {

constexpr int kTraceThreads = 256;
constexpr int kTraceRounds = 4;
constexpr int kTraceChunk = kTraceThreads * kTraceRounds;  // pixels a counting chunk, nodes a leader chunk
constexpr int kTraceRankTile = 256;                        // ring keys staged in LDS at a time
constexpr int kTraceNodeBlocks = 1024;                     // the most workgroups an image in the per-node launches
constexpr int kTraceMaxSide = 32768;
static_assert(kTraceRankTile == kTraceThreads, "a thread stages one key of a tile");

__device__ __forceinline__ int dir_y(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }
__device__ __forceinline__ int dir_x(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
// the left of the direction of travel is the direction of side s - 1: north of east, east of south, ..

__device__ __forceinline__ bool of_region(const int32_t* img, int H, int W, int y, int x, int r) {
    return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && img[(size_t)y * W + x] == r;
}

// Bit s: side s of pixel (y, x) of region r is a corner edge.  It is a boundary edge if the pixel on its left is not of
// r, and its predecessor runs the same way iff the pixel behind is of r and the one behind on the left is not.
__device__ __forceinline__ int corner_mask(const int32_t* img, int H, int W, int y, int x, int r) {
    unsigned near = 0;  // bit (dy + 1) * 3 + dx + 1
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            if ((dy | dx) != 0 && of_region(img, H, W, y + dy, x + dx, r)) near |= 1u << ((dy + 1) * 3 + dx + 1);
    int mask = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int ly = dir_y((s + 3) & 3), lx = dir_x((s + 3) & 3);
        const int by = -dir_y(s), bx = -dir_x(s);
        const bool across = (near >> ((ly + 1) * 3 + lx + 1)) & 1;
        const bool behind = (near >> ((by + 1) * 3 + bx + 1)) & 1;
        const bool behind_left = (near >> ((by + ly + 1) * 3 + bx + lx + 1)) & 1;
        if (!across && !(behind && !behind_left)) mask |= 1 << s;
    }
    return mask;
}

__device__ __forceinline__ int2 start_vertex(int y, int x, int s) { return make_int2(x + (s == 1 || s == 2), y + (s >= 2)); }

// From edge s of pixel (y, x) of region r along its straight run: (y, x) becomes the run's last pixel; -> the successor
// of the run's last edge as (pixel index, side).  That successor is a corner edge.
__device__ __forceinline__ int2 run_end(const int32_t* img, int H, int W, int r, int eight, int& y, int& x, int s) {
    const int dy = dir_y(s), dx = dir_x(s), ly = dir_y((s + 3) & 3), lx = dir_x((s + 3) & 3);
    for (;;) {
        const bool ahead = of_region(img, H, W, y + dy, x + dx, r);
        const bool ahead_left = of_region(img, H, W, y + dy + ly, x + dx + lx, r);
        if (ahead && !ahead_left) {  // straight on
            y += dy;
            x += dx;
            continue;
        }
        // a left turn onto the pixel ahead on the left: always when the pixel ahead is of r too, at a saddle (it is not)
        // under connectivity 8 only; otherwise a right turn onto the next side of the same pixel
        if (ahead_left && (ahead || eight)) return make_int2((y + dy + ly) * W + x + dx + lx, (s + 3) & 3);
        return make_int2(y * W + x, (s + 1) & 3);
    }
}

__global__ __launch_bounds__(kTraceThreads) void k_trace_count(const int32_t* __restrict__ ids, int H, int W, int R,
                                                               int nchunks, int32_t* __restrict__ chunk_count) {
    __shared__ int wave_sums[4];
    const int hw = H * W;
    const int32_t* img = ids + (size_t)blockIdx.y * hw;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTraceRounds; ++k) {
        const int p = blockIdx.x * kTraceChunk + k * kTraceThreads + threadIdx.x;
        if (p >= hw) continue;
        const int r = img[p];
        if ((unsigned)r < (unsigned)R) mine += __popc(corner_mask(img, H, W, p / W, p % W, r));
    }
    int total;
    isc_block_exclusive_scan(mine, wave_sums, total);
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * nchunks + blockIdx.x] = total;
}

// One workgroup an image: counts -> the sum before each chunk, in place; totals[b] = the sum of all.
__global__ __launch_bounds__(256) void k_trace_offsets(int32_t* __restrict__ counts, int nchunks,
                                                       int32_t* __restrict__ totals) {
    __shared__ int wave_sums[4];
    int32_t* c = counts + (size_t)blockIdx.x * nchunks;
    int running = 0;
    for (int i0 = 0; i0 < nchunks; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const int v = i < nchunks ? c[i] : 0;
        int total;
        const int before = isc_block_exclusive_scan(v, wave_sums, total);
        if (i < nchunks) c[i] = running + before;
        running += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = running;
}

__global__ __launch_bounds__(kTraceThreads) void k_trace_number(const int32_t* __restrict__ ids, int H, int W, int R,
                                                                int nchunks, const int32_t* __restrict__ chunk_offset,
                                                                int32_t* __restrict__ pix_first,
                                                                int32_t* __restrict__ node_key) {
    __shared__ int wave_sums[4];
    const int hw = H * W, b = blockIdx.y;
    const int32_t* img = ids + (size_t)b * hw;
    int32_t* keys = node_key + (size_t)b * 4 * hw;
    int at = chunk_offset[(size_t)b * nchunks + blockIdx.x];
#pragma unroll
    for (int k = 0; k < kTraceRounds; ++k) {
        const int p = blockIdx.x * kTraceChunk + k * kTraceThreads + threadIdx.x;
        int mask = 0;
        if (p < hw) {
            const int r = img[p];
            if ((unsigned)r < (unsigned)R) mask = corner_mask(img, H, W, p / W, p % W, r);
        }
        int total;
        int first = at + isc_block_exclusive_scan(__popc(mask), wave_sums, total);
        at += total;
        if (p >= hw) continue;
        pix_first[(size_t)b * hw + p] = first;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if ((mask >> s) & 1) keys[first++] = 4 * p + s;
    }
}

// state = (the node 2^k behind, the smallest node of the window, how far behind the node it is, the node's predecessor)
__global__ __launch_bounds__(kTraceThreads) void k_trace_link(const int32_t* __restrict__ ids, int H, int W, int eight,
                                                              const int32_t* __restrict__ num_nodes,
                                                              const int32_t* __restrict__ pix_first,
                                                              const int32_t* __restrict__ node_key,
                                                              int4* __restrict__ state) {
    const int hw = H * W, b = blockIdx.y, n = num_nodes[b];
    const int32_t* img = ids + (size_t)b * hw;
    const size_t nodes = (size_t)b * 4 * hw;
    for (int i = blockIdx.x * kTraceThreads + threadIdx.x; i < n; i += gridDim.x * kTraceThreads) {
        const int key = node_key[nodes + i], p = key >> 2, s = key & 3;
        int y = p / W, x = p - y * W;
        const int r = img[p];
        const int2 next = run_end(img, H, W, r, eight, y, x, s);
        const int ny = next.x / W, nx = next.x - ny * W;
        const int mask = corner_mask(img, H, W, ny, nx, r);
        const int j = pix_first[(size_t)b * hw + next.x] + __popc(mask & ((1 << next.y) - 1));
        state[nodes + j] = make_int4(i, j, 0, i);
    }
}

__global__ __launch_bounds__(kTraceThreads) void k_trace_jump(const int4* __restrict__ src, int4* __restrict__ dst,
                                                              size_t image_nodes, const int32_t* __restrict__ num_nodes,
                                                              int span) {
    const int n = num_nodes[blockIdx.y];
    src += (size_t)blockIdx.y * image_nodes;
    dst += (size_t)blockIdx.y * image_nodes;
    for (int i = blockIdx.x * kTraceThreads + threadIdx.x; i < n; i += gridDim.x * kTraceThreads) {
        const int4 a = src[i];
        const int4 c = src[a.x];
        const bool further = c.y < a.y;  // a node seen again (the window has gone round the ring) changes nothing
        dst[i] = make_int4(c.x, further ? c.y : a.y, further ? c.z + span : a.z, a.w);
    }
}

__global__ __launch_bounds__(kTraceThreads) void k_trace_leaders(const int4* __restrict__ fin, size_t image_nodes,
                                                                 const int32_t* __restrict__ num_nodes, int nchunks,
                                                                 int32_t* __restrict__ chunk_count) {
    __shared__ int wave_sums[4];
    const int n = num_nodes[blockIdx.y];
    fin += (size_t)blockIdx.y * image_nodes;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTraceRounds; ++k) {
        const unsigned i = (unsigned)blockIdx.x * kTraceChunk + k * kTraceThreads + threadIdx.x;
        if (i < (unsigned)n && fin[i].y == (int)i) ++mine;
    }
    int total;
    isc_block_exclusive_scan(mine, wave_sums, total);
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * nchunks + blockIdx.x] = total;
}

struct TraceFit {
    const int32_t* num_rings;
    const int32_t* num_nodes;
    int N, V;
    __device__ __forceinline__ bool operator()(int b) const { return num_rings[b] <= N && num_nodes[b] <= V; }
};

// A leader numbers its ring (the order of the leaders), leaves the number in the idle buffer's first word, and writes the
// ring's length -- one more than the place of the leader's predecessor -- and its key: region, then the start vertex.  A
// leader on side 0 starts at the start vertex; one on side 2 (a hole) ends its run there.
__global__ __launch_bounds__(kTraceThreads) void k_trace_rings(const int32_t* __restrict__ ids, int H, int W, int eight,
                                                               const int4* __restrict__ fin, int4* __restrict__ idle,
                                                               const int32_t* __restrict__ node_key, TraceFit fits,
                                                               int nchunks, const int32_t* __restrict__ chunk_offset,
                                                               int64_t* __restrict__ ring_key,
                                                               int32_t* __restrict__ ring_len) {
    __shared__ int wave_sums[4];
    const int hw = H * W, b = blockIdx.y;
    if (!fits(b)) return;
    const int n = fits.num_nodes[b];
    if (blockIdx.x * kTraceChunk >= n) return;
    const int32_t* img = ids + (size_t)b * hw;
    const size_t nodes = (size_t)b * 4 * hw;
    int at = chunk_offset[(size_t)b * nchunks + blockIdx.x];
#pragma unroll
    for (int k = 0; k < kTraceRounds; ++k) {
        const int i = blockIdx.x * kTraceChunk + k * kTraceThreads + threadIdx.x;
        const bool leader = i < n && fin[nodes + i].y == i;
        int total;
        const int j = at + isc_block_exclusive_scan(leader ? 1 : 0, wave_sums, total);
        at += total;
        if (!leader) continue;
        reinterpret_cast<int32_t*>(idle + nodes + i)[0] = j;
        ring_len[(size_t)b * hw + j] = fin[nodes + fin[nodes + i].w].z + 1;
        const int key = node_key[nodes + i], p = key >> 2, s = key & 3;
        int y = p / W, x = p - y * W;
        const int r = img[p];
        int2 v = make_int2(x, y);
        if (s != 0) {
            run_end(img, H, W, r, eight, y, x, s);
            v = start_vertex(y, x, (s + 1) & 3);
        }
        ring_key[(size_t)b * hw + j] = ((int64_t)r << 32) | (int64_t)(v.y * (W + 1) + v.x);
    }
}

// The keys of an image's rings are distinct: the place of a ring is the number of smaller keys.
__global__ __launch_bounds__(kTraceThreads) void k_trace_rank(const int64_t* __restrict__ ring_key,
                                                              const int32_t* __restrict__ ring_len, int hw, TraceFit fits,
                                                              int32_t* __restrict__ ring_place,
                                                              int32_t* __restrict__ placed_len,
                                                              int32_t* __restrict__ ring_region) {
    __shared__ int64_t keys[kTraceRankTile];
    const int b = blockIdx.y;
    if (!fits(b)) return;
    const int n = fits.num_rings[b];
    if (blockIdx.x * kTraceThreads >= n) return;
    const size_t rings = (size_t)b * hw;
    const int j = blockIdx.x * kTraceThreads + threadIdx.x;
    const int64_t mine = j < n ? ring_key[rings + j] : LLONG_MAX;
    int place = 0;
    for (int t = 0; t < n; t += kTraceRankTile) {
        __syncthreads();  // the tile before is consumed
        keys[threadIdx.x] = t + (int)threadIdx.x < n ? ring_key[rings + t + threadIdx.x] : LLONG_MAX;
        __syncthreads();
        const int count = min(kTraceRankTile, n - t);
        for (int k = 0; k < count; ++k) place += keys[k] < mine ? 1 : 0;  // one LDS address a wave: a broadcast
    }
    if (j >= n) return;
    ring_place[rings + j] = place;
    placed_len[rings + place] = ring_len[rings + j];
    ring_region[(size_t)b * (fits.N + 1) + place] = (int32_t)(mine >> 32);
}

// One workgroup an image.
__global__ __launch_bounds__(256) void k_trace_starts(const int32_t* __restrict__ placed_len, int hw, TraceFit fits, int B,
                                                      int32_t* __restrict__ ring_start, int32_t* __restrict__ ring_region,
                                                      int32_t* __restrict__ image_start, int64_t* __restrict__ ring_area2) {
    __shared__ int wave_sums[4];
    const int b = blockIdx.x, N = fits.N, V = fits.V;
    const int n = fits(b) ? fits.num_rings[b] : 0;
    const size_t row = (size_t)b * (N + 1);
    int running = b * V;
    for (int j0 = 0; j0 <= N; j0 += 256) {
        const int j = j0 + threadIdx.x;  // j0 is a multiple of 256 and at most N <= 2^31 - 2: j fits an int
        const int v = j < n ? placed_len[(size_t)b * hw + j] : 0;
        int total;
        const int before = isc_block_exclusive_scan(v, wave_sums, total);
        if (j <= N) {
            ring_start[row + j] = running + before;
            if (j >= n) ring_region[row + j] = -1;
            if (j < N && ring_area2) ring_area2[(size_t)b * N + j] = 0;
        }
        running += total;
        if (j0 > INT_MAX - 256) break;  // the last round of the largest N: the step would overflow
    }
    if (threadIdx.x == 0) {
        image_start[b] = (int)row;
        if (b == B - 1) {
            image_start[B] = B * (N + 1);
            ring_start[(size_t)B * (N + 1)] = B * V;
        }
    }
}

__global__ __launch_bounds__(kTraceThreads) void k_trace_write(int W, size_t image_nodes, int hw,
                                                               const int4* __restrict__ fin, const int4* __restrict__ idle,
                                                               const int32_t* __restrict__ node_key, TraceFit fits,
                                                               const int32_t* __restrict__ ring_place,
                                                               const int32_t* __restrict__ ring_len,
                                                               const int32_t* __restrict__ ring_start,
                                                               int2* __restrict__ vertices,
                                                               int64_t* __restrict__ ring_area2) {
    const int b = blockIdx.y;
    if (!fits(b)) return;
    const int n = fits.num_nodes[b];
    fin += (size_t)b * image_nodes;
    idle += (size_t)b * image_nodes;
    node_key += (size_t)b * image_nodes;
    const size_t rings = (size_t)b * hw;
    for (int i = blockIdx.x * kTraceThreads + threadIdx.x; i < n; i += gridDim.x * kTraceThreads) {
        const int4 a = fin[i];
        const int j = idle[a.y].x;
        const int place = ring_place[rings + j], len = ring_len[rings + j];
        const bool hole = (node_key[a.y] & 3) == 2;  // its leader ends at the start vertex: the ring starts one node on
        const int slot = hole ? (a.z == 0 ? len - 1 : a.z - 1) : a.z;
        const int key = node_key[i], p = key >> 2;
        const int2 v = start_vertex(p / W, p % W, key & 3);
        vertices[ring_start[(size_t)b * (fits.N + 1) + place] + slot] = make_int2(256 * v.x, 256 * v.y);
        if (ring_area2) {
            const int before = node_key[a.w], q = before >> 2;
            const int2 u = start_vertex(q / W, q % W, before & 3);
            const int64_t term = (int64_t)u.x * v.y - (int64_t)v.x * u.y;
            if (term != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(ring_area2 + (size_t)b * fits.N + place),
                          (unsigned long long)term);
        }
    }
}

struct TraceWorkspace {
    size_t pix_first_at, pix_chunks_at, node_chunks_at, node_key_at, state_at[2], ring_key_at, ring_len_at, ring_place_at,
        placed_len_at, bytes;
    int nchunks, node_chunks;
};

TraceWorkspace trace_workspace(int B, int H, int W) {
    const size_t hw = (size_t)H * W, pixels = (size_t)B * hw, nodes = 4 * pixels;
    TraceWorkspace ws;
    ws.nchunks = (int)isc_ceil_div(hw, (size_t)kTraceChunk);
    ws.node_chunks = (int)isc_ceil_div(4 * hw, (size_t)kTraceChunk);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += isc_align_up(bytes, 16);
        return here;
    };
    ws.state_at[0] = take(nodes * sizeof(int4));
    ws.state_at[1] = take(nodes * sizeof(int4));
    ws.ring_key_at = take(pixels * sizeof(int64_t));
    ws.node_key_at = take(nodes * sizeof(int32_t));
    ws.pix_first_at = take(pixels * sizeof(int32_t));
    ws.ring_len_at = take(pixels * sizeof(int32_t));
    ws.ring_place_at = take(pixels * sizeof(int32_t));
    ws.placed_len_at = take(pixels * sizeof(int32_t));
    ws.pix_chunks_at = take((size_t)B * ws.nchunks * sizeof(int32_t));
    ws.node_chunks_at = take((size_t)B * ws.node_chunks * sizeof(int32_t));
    ws.bytes = at;
    return ws;
}

int trace_shape_status(int B, int H, int W) {
    ISC_REQUIRE(B >= 0 && H >= 1 && W >= 1);
    if (H > kTraceMaxSide || W > kTraceMaxSide || B > 65535) return ISC_ERR_UNSUPPORTED;
    if ((int64_t)H * W >= (int64_t)1 << 29) return ISC_ERR_UNSUPPORTED;  // 4 H W corner edges must fit an int32 count
    return ISC_OK;
}

int trace_rounds(int H, int W) {  // the smallest K with 2^K >= 4 H W, the most nodes a ring can have
    int k = 2;
    while (((int64_t)1 << k) < 4 * (int64_t)H * W) ++k;
    return k;
}

}  // namespace

extern "C" int isc_trace_regions_geometry(int* pixel_chunk, int* node_chunk, int* ring_tile, int* node_pass) {
    ISC_REQUIRE(pixel_chunk && node_chunk && ring_tile && node_pass);
    *pixel_chunk = kTraceChunk;
    *node_chunk = kTraceChunk;
    *ring_tile = kTraceRankTile;
    *node_pass = kTraceNodeBlocks * kTraceThreads;
    return ISC_OK;
}

extern "C" int isc_trace_regions_workspace_bytes(int B, int H, int W, size_t* bytes) {
    ISC_REQUIRE(bytes);
    const int st = trace_shape_status(B, H, W);
    if (st != ISC_OK) return st;
    *bytes = trace_workspace(B > 0 ? B : 1, H, W).bytes;
    return ISC_OK;
}

extern "C" int isc_trace_regions(const int32_t* ids, int B, int H, int W, int R, int connectivity, int N, int V,
                                 int32_t* vertices, int32_t* ring_start, int32_t* ring_region, int32_t* image_start,
                                 int64_t* ring_area2, int32_t* num_rings, int32_t* num_vertices, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    ISC_REQUIRE(connectivity == 4 || connectivity == 8);
    ISC_REQUIRE(R >= 1 && N >= 1 && V >= 1);
    const int shape = trace_shape_status(B, H, W);
    if (shape != ISC_OK) return shape;
    const int64_t images = B > 0 ? B : 1;
    if (images * ((int64_t)N + 1) >= (int64_t)1 << 31 || images * (int64_t)V >= (int64_t)1 << 31) return ISC_ERR_UNSUPPORTED;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(ids && vertices && ring_start && ring_region && image_start && num_rings && num_vertices);
    const TraceWorkspace ws = trace_workspace(B, H, W);
    if (!workspace || workspace_bytes < ws.bytes) return ISC_ERR_WORKSPACE;
    if (!isc_aligned(workspace, 16) || !isc_aligned(vertices, 8) || !isc_aligned(ring_area2, 8) || !isc_aligned(ids, 4) ||
        !isc_aligned(ring_start, 4) || !isc_aligned(ring_region, 4) || !isc_aligned(image_start, 4) ||
        !isc_aligned(num_rings, 4) || !isc_aligned(num_vertices, 4))
        return ISC_ERR_ALIGNMENT;

    hipStream_t s = isc_stream(stream);
    char* wsp = static_cast<char*>(workspace);
    int4* state[2] = {reinterpret_cast<int4*>(wsp + ws.state_at[0]), reinterpret_cast<int4*>(wsp + ws.state_at[1])};
    int64_t* ring_key = reinterpret_cast<int64_t*>(wsp + ws.ring_key_at);
    int32_t* node_key = reinterpret_cast<int32_t*>(wsp + ws.node_key_at);
    int32_t* pix_first = reinterpret_cast<int32_t*>(wsp + ws.pix_first_at);
    int32_t* ring_len = reinterpret_cast<int32_t*>(wsp + ws.ring_len_at);
    int32_t* ring_place = reinterpret_cast<int32_t*>(wsp + ws.ring_place_at);
    int32_t* placed_len = reinterpret_cast<int32_t*>(wsp + ws.placed_len_at);
    int32_t* pix_chunks = reinterpret_cast<int32_t*>(wsp + ws.pix_chunks_at);
    int32_t* node_chunks = reinterpret_cast<int32_t*>(wsp + ws.node_chunks_at);
    const int hw = H * W, eight = connectivity == 8;
    const size_t image_nodes = 4 * (size_t)hw;
    const int node_blocks = (int)(isc_ceil_div(image_nodes, (size_t)kTraceThreads) < (size_t)kTraceNodeBlocks
                                      ? isc_ceil_div(image_nodes, (size_t)kTraceThreads)
                                      : (size_t)kTraceNodeBlocks);
    const dim3 pixel_grid(ws.nchunks, B), chunk_grid(ws.node_chunks, B), node_grid(node_blocks, B);
    const int held = N < hw ? N : hw;  // an image has at most H * W rings
    const TraceFit fits = {num_rings, num_vertices, N, V};

#define ISC_TRACE_LAUNCHED() \
    if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH
    hipLaunchKernelGGL(k_trace_count, pixel_grid, dim3(kTraceThreads), 0, s, ids, H, W, R, ws.nchunks, pix_chunks);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_offsets, dim3(B), dim3(256), 0, s, pix_chunks, ws.nchunks, num_vertices);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_number, pixel_grid, dim3(kTraceThreads), 0, s, ids, H, W, R, ws.nchunks, pix_chunks,
                       pix_first, node_key);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_link, node_grid, dim3(kTraceThreads), 0, s, ids, H, W, eight, num_vertices, pix_first,
                       node_key, state[0]);
    ISC_TRACE_LAUNCHED();
    const int rounds = trace_rounds(H, W);
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(k_trace_jump, node_grid, dim3(kTraceThreads), 0, s, state[k & 1], state[(k + 1) & 1],
                           image_nodes, num_vertices, 1 << k);
        ISC_TRACE_LAUNCHED();
    }
    const int4* fin = state[rounds & 1];
    int4* idle = state[(rounds + 1) & 1];
    hipLaunchKernelGGL(k_trace_leaders, chunk_grid, dim3(kTraceThreads), 0, s, fin, image_nodes, num_vertices,
                       ws.node_chunks, node_chunks);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_offsets, dim3(B), dim3(256), 0, s, node_chunks, ws.node_chunks, num_rings);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_rings, chunk_grid, dim3(kTraceThreads), 0, s, ids, H, W, eight, fin, idle, node_key, fits,
                       ws.node_chunks, node_chunks, ring_key, ring_len);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_rank, dim3(isc_ceil_div(held, kTraceThreads), B), dim3(kTraceThreads), 0, s, ring_key,
                       ring_len, hw, fits, ring_place, placed_len, ring_region);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_starts, dim3(B), dim3(256), 0, s, placed_len, hw, fits, B, ring_start, ring_region,
                       image_start, ring_area2);
    ISC_TRACE_LAUNCHED();
    hipLaunchKernelGGL(k_trace_write, node_grid, dim3(kTraceThreads), 0, s, W, image_nodes, hw, fin, idle, node_key, fits,
                       ring_place, ring_len, ring_start, reinterpret_cast<int2*>(vertices), ring_area2);
#undef ISC_TRACE_LAUNCHED
    return isc_launch_status();
}
