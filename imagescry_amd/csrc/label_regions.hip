// isc_label_regions: the connected regions of uint8 pixel label maps (include/imagescry_hip.h has the definition, which
// the tests hold these kernels to value for value).
//
// `region_ids` doubles as the parent array of a union-find forest over the pixels of one image; a parent is a linear
// index y * W + x inside the image, -1 for an unlabeled pixel.  THE invariant: every value ever stored in parent[x] is
// <= x and lies in x's region, and a stored value is only ever replaced by a smaller one.  So the root of a finished
// tree is the region's smallest index, its anchor, and a reader that sees an older value of parent[x] still sees a
// member of x's region that is <= x: nothing below needs a fresh read to be right, only an atomic's return value to
// decide who hooked.
//
//   k_regions_tile    a workgroup resolves its 64 x 16 tile in LDS and stores, per pixel, the tile's root of it
//   k_regions_border  a thread per pixel on the far side of a tile border joins it to its neighbours across the border
//   k_regions_area    counts per tile and slot (below), shortens every tile root's path to one hop, sums the areas on
//                     the roots
//   k_regions_count / k_regions_offsets / k_regions_number
//                     kept roots per chunk of 1024 pixels in raster order, their exclusive scan per image, the ranks
//   k_regions_final   region_ids, labels_out and the statistics, one set of atomics per tile and slot
//   k_regions_init / k_regions_finish   the tables' rows before and after the atomics
#include "isc_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kRegionTileW = 64;
constexpr int kRegionTileH = 16;
constexpr int kRegionPixels = kRegionTileW * kRegionTileH;
constexpr int kRegionThreads = 256;
constexpr int kRegionRounds = kRegionPixels / kRegionThreads;  // pixel `round * 256 + tid` of the tile: a wave = one row
constexpr int kRegionChunk = 1024;                             // pixels a numbering chunk, raster order
constexpr int kUnlabeledRegion = 255;
static_assert(kRegionTileW == ISC_WAVE && kRegionThreads == 4 * ISC_WAVE, "a wave owns one tile row a round");
static_assert(kRegionChunk == kRegionRounds * kRegionThreads, "the chunk kernels walk a chunk in the tile's rounds");

// The key slots of the peak: min(max_regions, H * W) an image, which the workspace holds up to this many.
__host__ __device__ inline int64_t peak_slots(int64_t hw) {
    const int64_t cap = hw / 8 > 1024 ? hw / 8 : 1024;
    return hw < cap ? hw : cap;
}

// ------------------------------------------------------------------------------------------------------- union-find
// find: follows parents until parent[x] == x.  Terminates: a parent that differs from x is smaller than x (the
// invariant), so x strictly decreases and is bounded below by 0.  Under a stale read it may return a node that has been
// hooked meanwhile; unite() lets the atomic decide.
template <int kScope>
__device__ __forceinline__ int find(const int32_t* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, kScope);
        if (p == x) return x;
        x = p;
    }
}

// unite: lock-free, waits for nobody.  Each turn finds two roots a > b and offers b to a with an atomic min; the value
// the atomic returns is the truth about a: it was a root (old == a) and now hangs under b, done; or it had already been
// hooked under old < a, parent[a] is now min(old, b), and what is left to join is old and b.  Terminates: in the next
// turn both candidates are < a (find(old) <= old < a, find(b) <= b < a), so max(a, b) strictly decreases every turn and
// is bounded below by 0.  The larger index always goes under the smaller, which keeps the invariant.
template <int kScope>
__device__ __forceinline__ void unite(int32_t* parent, int a, int b) {
    for (;;) {
        a = find<kScope>(parent, a);
        b = find<kScope>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, kScope);
        if (old == a) return;
        a = old;
    }
}

// ----------------------------------------------------------------------------------------------------------- tile pass
// lab / par are indexed by the tile-local pixel l = ly * 64 + lx.  A row's runs are linked by a ballot (every pixel
// straight to its run's first pixel); then a pixel joins the row above: N if it has the label (unless W and NW have it
// too: then W's own join with NW covers it), otherwise, at 8-connectivity, NW and NE (with N in the region they are
// joined to it inside their row).
__global__ __launch_bounds__(kRegionThreads) void k_regions_tile(const uint8_t* __restrict__ labels,
                                                                 int32_t* __restrict__ parent, int32_t* __restrict__ area,
                                                                 int H, int W, int eight) {
    __shared__ uint8_t lab[kRegionPixels];
    __shared__ int32_t par[kRegionPixels];
    const int tid = threadIdx.x, lx = tid & 63;
    const int X0 = blockIdx.x * kRegionTileW, Y0 = blockIdx.y * kRegionTileH;
    const size_t base = (size_t)blockIdx.z * H * W;
    const int x = X0 + lx;
    // a tile of full width whose rows start on a dword: 16 lanes load four labels each, a shuffle hands them out
    const bool wide = X0 + kRegionTileW <= W && (W & 3) == 0 && (reinterpret_cast<uintptr_t>(labels + base) & 3) == 0;
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid, y = Y0 + (l >> 6);
        int v;
        if (wide) {
            uint32_t quad = 0xffffffffu;  // four unlabeled pixels: a row below the image
            if (y < H && lx < 16) quad = *reinterpret_cast<const uint32_t*>(labels + base + (size_t)y * W + X0 + 4 * lx);
            quad = (uint32_t)__shfl((int)quad, lx >> 2, 64);
            v = (quad >> (8 * (lx & 3))) & 0xffu;
        } else {
            v = (y < H && x < W) ? labels[base + (size_t)y * W + x] : kUnlabeledRegion;
        }
        lab[l] = (uint8_t)v;
        const int left = __shfl_up(v, 1, 64);
        const unsigned long long starts = __ballot(lx == 0 || left != v);
        const int run = 63 - __builtin_clzll(starts & (~0ull >> (63 - lx)));  // bit 0 is set: never zero
        par[l] = (l & ~63) + run;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid;
        const int v = lab[l];
        if (v == kUnlabeledRegion || l < kRegionTileW) continue;
        const bool n = lab[l - 64] == v;
        const bool nw = lx > 0 && lab[l - 65] == v, ne = lx < 63 && lab[l - 63] == v;
        if (n) {
            if (!(nw && lab[l - 1] == v)) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l - 64);
        } else if (eight) {
            if (nw) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l - 65);
            if (ne) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l - 63);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid, y = Y0 + (l >> 6);
        if (y >= H || x >= W) continue;
        const size_t at = base + (size_t)y * W + x;
        if (lab[l] == kUnlabeledRegion) {
            parent[at] = -1;
            continue;
        }
        const int r = find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l);
        parent[at] = (Y0 + (r >> 6)) * W + X0 + (r & 63);
        if (r == l) area[at] = 0;  // only a tile's root can end as a region's root: k_regions_area sums there
    }
}

// --------------------------------------------------------------------------------------------------------- border pass
// Threads [0, nh): pixel (y, x) of the first row of a tile row, y = 16, 32, ..: joined to N, or at 8-connectivity, when
// N has another label, to NW and NE.  Threads [nh, nh + nv): pixel (y, x) of the first column of a tile column:
// joined to W, or, when W has another label, to NW and SW.  Every pair of neighbours that no tile holds whole is among
// these (a pair across a tile corner crosses both kinds of border and is seen by either), or is a diagonal whose two
// pixels share a neighbour of the region that is joined to both across an edge.  A pair across an edge is left out where
// the pair before it along the border (inside the same two tiles, whose passes joined each to its own neighbour) is of
// the region too: one join a run and border, not one a pixel.  Workgroups on other XCDs hook roots in this launch:
// find() reads through relaxed agent-scope atomic loads, and only the atomic min decides.
__global__ __launch_bounds__(256) void k_regions_border(const uint8_t* __restrict__ labels, int32_t* __restrict__ parent,
                                                        int H, int W, int eight, int nh, int nv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nh + nv) return;
    const size_t base = (size_t)blockIdx.y * H * W;
    const uint8_t* lab = labels + base;
    int32_t* par = parent + base;
    constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT;
    if (i < nh) {
        const int k = i / W, x = i - k * W, y = (k + 1) * kRegionTileH;
        const int p = y * W + x, n = p - W;
        const int v = lab[p];
        if (v == kUnlabeledRegion) return;
        if (lab[n] == v) {
            if (!((x & (kRegionTileW - 1)) != 0 && lab[p - 1] == v && lab[n - 1] == v)) unite<kAgent>(par, p, n);
        } else if (eight) {
            if (x > 0 && lab[n - 1] == v) unite<kAgent>(par, p, n - 1);
            if (x + 1 < W && lab[n + 1] == v) unite<kAgent>(par, p, n + 1);
        }
    } else {
        const int j = i - nh;
        const int k = j / H, y = j - k * H, x = (k + 1) * kRegionTileW;
        const int p = y * W + x, w = p - 1;
        const int v = lab[p];
        if (v == kUnlabeledRegion) return;
        if (lab[w] == v) {
            if (!((y & (kRegionTileH - 1)) != 0 && lab[p - W] == v && lab[w - W] == v)) unite<kAgent>(par, p, w);
        } else if (eight) {
            if (y > 0 && lab[w - W] == v) unite<kAgent>(par, p, w - W);
            if (y + 1 < H && lab[w + W] == v) unite<kAgent>(par, p, w + W);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- slots
// After the border pass a pixel that was no root of its tile still points at its tile's root, inside the tile; a tile's
// root points wherever it was hooked.  The pixels of a tile are grouped by SLOT: the tile-local index of parent[p] where
// that lies inside the tile, of p itself otherwise.  All pixels of a slot belong to one region (they point at the slot's
// own pixel or are it), so a tile sums per slot in LDS and then issues ONE set of global atomics a slot: a region that
// fills the image costs a set per tile, not per pixel.
struct TilePos {
    int X0, Y0, W;
    __device__ __forceinline__ int slot_of(int q) const {  // the tile-local index of pixel q, -1 outside the tile
        const int qy = q / W, qx = q - qy * W;
        const unsigned ly = (unsigned)(qy - Y0), lx = (unsigned)(qx - X0);
        return (ly < (unsigned)kRegionTileH && lx < (unsigned)kRegionTileW) ? (int)(ly * kRegionTileW + lx) : -1;
    }
    __device__ __forceinline__ int pixel_of(int l) const { return (Y0 + (l >> 6)) * W + X0 + (l & 63); }
};

// Area: the slot's owner walks to the region's root (the tree is final: the kernel boundary behind the border pass made
// it visible), stores the root as its own parent -- after this launch every pixel is at most two hops from its root, the
// first of them inside its tile -- and adds the slot's count on the root.  A walk through another tile may meet an
// owner's old parent or its new one; both are its ancestors.
__global__ __launch_bounds__(kRegionThreads) void k_regions_area(int32_t* __restrict__ parent, int32_t* __restrict__ area,
                                                                 int H, int W) {
    __shared__ int cnt[kRegionPixels];
    const int tid = threadIdx.x;
    const TilePos t = {(int)blockIdx.x * kRegionTileW, (int)blockIdx.y * kRegionTileH, W};
    const size_t base = (size_t)blockIdx.z * H * W;
    int32_t* par = parent + base;
    const int x = t.X0 + (tid & 63);
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) cnt[k * kRegionThreads + tid] = 0;
    __syncthreads();
    int first[kRegionRounds];
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid, y = t.Y0 + (l >> 6);
        first[k] = (y < H && x < W) ? par[y * W + x] : -1;
        if (first[k] < 0) continue;
        const int s = t.slot_of(first[k]);
        atomicAdd(&cnt[s >= 0 ? s : l], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid;
        const int c = cnt[l];
        if (c == 0) continue;
        const int root = find<__HIP_MEMORY_SCOPE_AGENT>(par, first[k]);
        if (root != first[k]) __hip_atomic_store(par + t.pixel_of(l), root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(area + base + root, c);
    }
}

// ------------------------------------------------------------------------------------------------------------ numbering
// A chunk is 1024 consecutive pixels of one image in raster order; pixel `round * 256 + tid` of it is the thread's.
__device__ __forceinline__ bool kept_root(const int32_t* par, const int32_t* area, int hw, int p, int min_area) {
    return p < hw && par[p] == p && area[p] >= min_area;
}

__global__ __launch_bounds__(kRegionThreads) void k_regions_count(const int32_t* __restrict__ parent,
                                                                  const int32_t* __restrict__ area, int hw, int min_area,
                                                                  int nchunks, int32_t* __restrict__ chunk_count) {
    __shared__ int wave_sums[4];
    const size_t base = (size_t)blockIdx.y * hw;
    const int p0 = blockIdx.x * kRegionChunk + threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k)
        mine += kept_root(parent + base, area + base, hw, p0 + k * kRegionThreads, min_area) ? 1 : 0;
    int total;
    isc_block_exclusive_scan(mine, wave_sums, total);
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * nchunks + blockIdx.x] = total;
}

// One workgroup an image: chunk_count -> the kept roots before each chunk, in place; num_regions = their total.
__global__ __launch_bounds__(256) void k_regions_offsets(int32_t* __restrict__ chunk_count, int nchunks,
                                                         int32_t* __restrict__ num_regions) {
    __shared__ int wave_sums[4];
    int32_t* c = chunk_count + (size_t)blockIdx.x * nchunks;
    int running = 0;
    for (int i0 = 0; i0 < nchunks; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const int v = i < nchunks ? c[i] : 0;
        int total;
        const int before = isc_block_exclusive_scan(v, wave_sums, total);
        if (i < nchunks) c[i] = running + before;
        running += total;
    }
    if (threadIdx.x == 0) num_regions[blockIdx.x] = running;
}

// The rank of every kept root: the chunk's offset + the kept roots before it inside the chunk (rounds ascending, inside
// a round threads ascending: raster order).  The root writes the rows it knows and leaves its rank where its area was;
// a dropped root leaves -1.
__global__ __launch_bounds__(kRegionThreads) void k_regions_number(
    const uint8_t* __restrict__ labels, const int32_t* __restrict__ parent, int32_t* __restrict__ area, int hw, int min_area,
    int nchunks, const int32_t* __restrict__ chunk_offset, int R, int32_t* __restrict__ region_label,
    int32_t* __restrict__ region_area, int32_t* __restrict__ region_anchor) {
    __shared__ int wave_sums[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * hw;
    int at = chunk_offset[(size_t)b * nchunks + blockIdx.x];
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int p = blockIdx.x * kRegionChunk + k * kRegionThreads + threadIdx.x;
        const bool root = p < hw && parent[base + p] == p;
        const int a = root ? area[base + p] : 0;
        const bool kept = root && a >= min_area;
        int total;
        const int r = at + isc_block_exclusive_scan(kept ? 1 : 0, wave_sums, total);
        at += total;
        if (!root) continue;
        area[base + p] = kept ? r : -1;
        if (kept && r < R) {
            const size_t row = (size_t)b * R + r;
            if (region_label) region_label[row] = labels[base + p];
            if (region_area) region_area[row] = a;
            if (region_anchor) region_anchor[row] = p;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- final pass
// The order of the searches as one unsigned key: value descending, NaN last, ties to the lower linear index.  High word:
// the float's order-preserving image (0 for a NaN, below -inf's 0x007fffff; -0.0 counts as +0.0: they are one value and
// tie); low word: the complement of the index.  Every key is > 0, the value the slots start from.
__device__ __forceinline__ unsigned peak_order(float v) {
    if (v != v) return 0;
    const unsigned bits = v == 0.f ? 0u : __float_as_uint(v);
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}

__device__ __forceinline__ unsigned long long peak_key(unsigned order, int p) {
    return ((unsigned long long)order << 32) | (unsigned)~p;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, 64));
    return v;
}

// The sum of the positions of the set bits.
__device__ __forceinline__ int bit_position_sum(unsigned long long m) {
    return __popcll(m & 0xaaaaaaaaaaaaaaaaull) + 2 * __popcll(m & 0xccccccccccccccccull) +
           4 * __popcll(m & 0xf0f0f0f0f0f0f0f0ull) + 8 * __popcll(m & 0xff00ff00ff00ff00ull) +
           16 * __popcll(m & 0xffff0000ffff0000ull) + 32 * __popcll(m & 0xffffffff00000000ull);
}

constexpr int kWaveRounds = 4;  // slots a row segment sums through ballots before its lanes turn to LDS atomics of their own

struct RegionTables {
    int32_t* box;
    unsigned long long* sum;
    unsigned long long* key;
    int R, key_stride;
};

// `rank` holds what k_regions_number left on the roots.  All reads of `ids` as parents (the pixel's own and, inside the
// tile, its tile root's) come before the barrier, all stores of ids after it, and no thread reads a parent outside its
// tile: a parent outside the tile is the root itself.
template <bool kStats>
__global__ __launch_bounds__(kRegionThreads) void k_regions_final(const uint8_t* __restrict__ labels,
                                                                  const float* __restrict__ best, int32_t* __restrict__ ids,
                                                                  const int32_t* __restrict__ rank, int H, int W,
                                                                  uint8_t* __restrict__ labels_out, RegionTables tb) {
    __shared__ int s_cnt[kStats ? kRegionPixels : 1], s_sy[kStats ? kRegionPixels : 1], s_sx[kStats ? kRegionPixels : 1];
    __shared__ int s_y0[kStats ? kRegionPixels : 1], s_x0[kStats ? kRegionPixels : 1];
    __shared__ int s_y1[kStats ? kRegionPixels : 1], s_x1[kStats ? kRegionPixels : 1];
    __shared__ unsigned long long s_key[kStats ? kRegionPixels : 1];
    const int tid = threadIdx.x, lx = tid & 63;
    const TilePos t = {(int)blockIdx.x * kRegionTileW, (int)blockIdx.y * kRegionTileH, W};
    const int b = blockIdx.z;
    const size_t base = (size_t)b * H * W;
    const int x = t.X0 + lx;
    int slot[kRegionRounds], id[kRegionRounds], lab[kRegionRounds];
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid, y = t.Y0 + (l >> 6);
        if (kStats) {
            s_cnt[l] = s_sy[l] = s_sx[l] = 0;
            s_y0[l] = s_x0[l] = INT_MAX;
            s_y1[l] = s_x1[l] = -1;
            s_key[l] = 0;
        }
        slot[k] = id[k] = -1;
        lab[k] = kUnlabeledRegion;
        if (y >= H || x >= W) continue;
        const int p = y * W + x;
        lab[k] = labels[base + p];
        if (lab[k] == kUnlabeledRegion) continue;
        const int q = ids[base + p];
        const int s = t.slot_of(q);
        slot[k] = s >= 0 ? s : l;
        const int root = s >= 0 ? ids[base + q] : q;
        id[k] = rank[base + root];
    }
    __syncthreads();
    // A wave holds one row segment of the tile, and the pixels of a slot in it are a set of lanes: count, sums and box of
    // the set follow from its ballot alone, the peak from one wave maximum (the first lane that holds it has the lowest
    // index).  The set's first lane adds them to the slot.  After kWaveRounds slots the lanes left add their own pixel.
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid, ly = l >> 6, y = t.Y0 + ly;
        const bool inside = y < H && x < W;
        const int p = y * W + x;
        if (inside) {
            ids[base + p] = id[k];
            if (labels_out) labels_out[base + p] = (uint8_t)(id[k] >= 0 ? lab[k] : kUnlabeledRegion);
        }
        if (!kStats) continue;
        const bool counts = inside && id[k] >= 0 && id[k] < tb.R;
        const unsigned order = (tb.key && counts) ? peak_order(best[base + p]) : 0u;
        unsigned long long todo = __ballot(counts);
        for (int round = 0; todo != 0 && round < kWaveRounds; ++round) {
            const int leader = __builtin_ctzll(todo);
            const int s = __shfl(slot[k], leader, 64);
            const bool member = counts && slot[k] == s;
            const unsigned long long set = __ballot(member);
            unsigned top = 0;
            int first = 0;
            if (tb.key) {
                top = wave_max(member ? order : 0u);
                first = __builtin_ctzll(__ballot(member && order == top));
            }
            if (lx == leader) {
                const int c = __popcll(set);
                atomicAdd(&s_cnt[s], c);
                atomicAdd(&s_sy[s], c * ly);
                atomicAdd(&s_sx[s], bit_position_sum(set));
                atomicMin(&s_y0[s], ly);
                atomicMax(&s_y1[s], ly);
                atomicMin(&s_x0[s], __builtin_ctzll(set));
                atomicMax(&s_x1[s], 63 - __builtin_clzll(set));
                if (tb.key) atomicMax(&s_key[s], peak_key(top, p - lx + first));
            }
            todo &= ~set;
        }
        if (counts && ((todo >> lx) & 1)) {
            const int s = slot[k];
            atomicAdd(&s_cnt[s], 1);
            atomicAdd(&s_sy[s], ly);
            atomicAdd(&s_sx[s], lx);
            atomicMin(&s_y0[s], ly);
            atomicMin(&s_x0[s], lx);
            atomicMax(&s_y1[s], ly);
            atomicMax(&s_x1[s], lx);
            if (tb.key) atomicMax(&s_key[s], peak_key(order, p));
        }
    }
    if (!kStats) return;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRegionRounds; ++k) {
        const int l = k * kRegionThreads + tid;
        const int c = s_cnt[l];
        if (c == 0) continue;  // a slot that has pixels belongs to a labeled pixel of a kept region below R: id[k] is it
        const size_t row = (size_t)b * tb.R + id[k];
        if (tb.box) {
            atomicMin(tb.box + row * 4 + 0, t.Y0 + s_y0[l]);
            atomicMin(tb.box + row * 4 + 1, t.X0 + s_x0[l]);
            atomicMax(tb.box + row * 4 + 2, t.Y0 + s_y1[l] + 1);
            atomicMax(tb.box + row * 4 + 3, t.X0 + s_x1[l] + 1);
        }
        if (tb.sum) {
            atomicAdd(tb.sum + row * 2 + 0, (unsigned long long)s_sy[l] + (unsigned long long)c * t.Y0);
            atomicAdd(tb.sum + row * 2 + 1, (unsigned long long)s_sx[l] + (unsigned long long)c * t.X0);
        }
        if (tb.key) atomicMax(tb.key + (size_t)b * tb.key_stride + id[k], s_key[l]);
    }
}

// ------------------------------------------------------------------------------------------------ the tables' rows
// Before the atomics: every row as an empty one, but the box's minima at INT_MAX, and the keys at 0.
__global__ __launch_bounds__(256) void k_regions_init(int B, int R, int key_stride, int32_t* __restrict__ region_label,
                                                      int32_t* __restrict__ region_area, int32_t* __restrict__ region_anchor,
                                                      int32_t* __restrict__ box, unsigned long long* __restrict__ sum,
                                                      unsigned long long* __restrict__ key) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * R) return;
    if (region_label) region_label[i] = -1;
    if (region_area) region_area[i] = 0;
    if (region_anchor) region_anchor[i] = -1;
    if (box) {
        box[i * 4 + 0] = box[i * 4 + 1] = INT_MAX;
        box[i * 4 + 2] = box[i * 4 + 3] = 0;
    }
    if (sum) sum[i * 2 + 0] = sum[i * 2 + 1] = 0;
    const int r = (int)(i % R);
    if (key && r < key_stride) key[i / R * key_stride + r] = 0;
}

// After them: the box of an empty row back to zeros; the peak out of its key.
__global__ __launch_bounds__(256) void k_regions_finish(int B, int R, int key_stride, size_t hw,
                                                        const int32_t* __restrict__ num_regions,
                                                        const float* __restrict__ best, int32_t* __restrict__ box,
                                                        const unsigned long long* __restrict__ key,
                                                        int32_t* __restrict__ peak, float* __restrict__ peak_score) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * R) return;
    const size_t b = i / R;
    const int r = (int)(i - b * R);
    const bool filled = r < num_regions[b];
    if (box && !filled) box[i * 4 + 0] = box[i * 4 + 1] = 0;
    if (!key) return;
    const int p = filled ? (int)~(unsigned)key[b * key_stride + r] : -1;
    if (peak) peak[i] = p;
    if (peak_score) peak_score[i] = filled ? best[b * hw + p] : -INFINITY;
}

struct RegionWorkspace {
    size_t rank_at, chunks_at, keys_at, bytes;
    int nchunks;
};

RegionWorkspace region_workspace(int B, int H, int W) {
    const size_t hw = (size_t)H * W;
    RegionWorkspace ws;
    ws.nchunks = (int)isc_ceil_div(hw, (size_t)kRegionChunk);
    ws.rank_at = 0;
    ws.chunks_at = isc_align_up((size_t)B * hw * sizeof(int32_t), 16);
    ws.keys_at = ws.chunks_at + isc_align_up((size_t)B * ws.nchunks * sizeof(int32_t), 16);
    ws.bytes = ws.keys_at + (size_t)B * peak_slots((int64_t)hw) * sizeof(unsigned long long);
    return ws;
}

int region_shape_status(int B, int H, int W) {
    ISC_REQUIRE(B >= 0 && H >= 1 && W >= 1);
    if ((int64_t)H * W >= (int64_t)1 << 31 || B > 65535) return ISC_ERR_UNSUPPORTED;
    if (isc_ceil_div(H, kRegionTileH) > 65535) return ISC_ERR_UNSUPPORTED;
    return ISC_OK;
}

}  // namespace

extern "C" int isc_label_regions_geometry(int* tile_w, int* tile_h) {
    ISC_REQUIRE(tile_w && tile_h);
    *tile_w = kRegionTileW;
    *tile_h = kRegionTileH;
    return ISC_OK;
}

extern "C" int isc_label_regions_workspace_bytes(int B, int H, int W, size_t* bytes) {
    ISC_REQUIRE(bytes);
    const int st = region_shape_status(B, H, W);
    if (st != ISC_OK) return st;
    *bytes = region_workspace(B > 0 ? B : 1, H, W).bytes;
    return ISC_OK;
}

extern "C" int isc_label_regions(const uint8_t* labels, const float* best, int B, int H, int W, int connectivity,
                                 int min_area, int max_regions, int32_t* region_ids, int32_t* num_regions,
                                 uint8_t* labels_out, int32_t* region_label, int32_t* region_area, int32_t* region_anchor,
                                 int32_t* region_box, int64_t* region_sum, int32_t* region_peak, float* region_peak_score,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    ISC_REQUIRE(connectivity == 4 || connectivity == 8);
    ISC_REQUIRE(min_area >= 1 && max_regions >= 1);
    ISC_REQUIRE(best || (!region_peak && !region_peak_score));
    const int shape = region_shape_status(B, H, W);
    if (shape != ISC_OK) return shape;
    const size_t hw = (size_t)H * W;
    const bool peaks = region_peak || region_peak_score;
    const int64_t rows = (int64_t)max_regions < (int64_t)hw ? max_regions : (int64_t)hw;  // rows that can ever fill
    if (peaks && rows > peak_slots((int64_t)hw)) return ISC_ERR_UNSUPPORTED;
    const size_t table_blocks = isc_ceil_div((size_t)(B > 0 ? B : 1) * max_regions, (size_t)256);
    if (table_blocks > (size_t)INT_MAX) return ISC_ERR_UNSUPPORTED;
    if (B == 0) return ISC_OK;
    ISC_REQUIRE(labels && region_ids && num_regions);
    if (labels_out) {  // the final pass reads a pixel's label after other tiles have stored theirs
        const uint8_t* lo = labels_out < labels ? labels_out : labels;
        const uint8_t* hi = labels_out < labels ? labels : labels_out;
        ISC_REQUIRE((size_t)(hi - lo) >= (size_t)B * hw);
    }
    const RegionWorkspace ws = region_workspace(B, H, W);
    if (!workspace || workspace_bytes < ws.bytes) return ISC_ERR_WORKSPACE;
    if (!isc_aligned(workspace, 16) || !isc_aligned(best, 4) || !isc_aligned(region_ids, 4) ||
        !isc_aligned(num_regions, 4) || !isc_aligned(region_label, 4) || !isc_aligned(region_area, 4) ||
        !isc_aligned(region_anchor, 4) || !isc_aligned(region_box, 4) || !isc_aligned(region_sum, 8) ||
        !isc_aligned(region_peak, 4) || !isc_aligned(region_peak_score, 4))
        return ISC_ERR_ALIGNMENT;

    hipStream_t s = isc_stream(stream);
    char* wsp = static_cast<char*>(workspace);
    int32_t* rank = reinterpret_cast<int32_t*>(wsp + ws.rank_at);  // areas on the roots until k_regions_number
    int32_t* chunks = reinterpret_cast<int32_t*>(wsp + ws.chunks_at);
    unsigned long long* keys = peaks ? reinterpret_cast<unsigned long long*>(wsp + ws.keys_at) : nullptr;
    const int R = max_regions, key_stride = (int)rows, eight = connectivity == 8;
    const bool tables = region_label || region_area || region_anchor || region_box || region_sum || peaks;
    const bool stats = region_box || region_sum || peaks;
    const int tiles_x = isc_ceil_div(W, kRegionTileW), tiles_y = isc_ceil_div(H, kRegionTileH);
    const dim3 tile_grid(tiles_x, tiles_y, B), chunk_grid(ws.nchunks, B);
    const int nh = (tiles_y - 1) * W, nv = (tiles_x - 1) * H;
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(region_sum);

#define ISC_REGION_LAUNCHED() \
    if (hipGetLastError() != hipSuccess) return ISC_ERR_LAUNCH
    if (tables) {
        hipLaunchKernelGGL(k_regions_init, dim3((unsigned)table_blocks), dim3(256), 0, s, B, R, key_stride, region_label,
                           region_area, region_anchor, region_box, sums, keys);
        ISC_REGION_LAUNCHED();
    }
    hipLaunchKernelGGL(k_regions_tile, tile_grid, dim3(kRegionThreads), 0, s, labels, region_ids, rank, H, W, eight);
    ISC_REGION_LAUNCHED();
    if (nh + nv > 0) {
        hipLaunchKernelGGL(k_regions_border, dim3(isc_ceil_div(nh + nv, 256), B), dim3(256), 0, s, labels, region_ids, H, W,
                           eight, nh, nv);
        ISC_REGION_LAUNCHED();
    }
    hipLaunchKernelGGL(k_regions_area, tile_grid, dim3(kRegionThreads), 0, s, region_ids, rank, H, W);
    ISC_REGION_LAUNCHED();
    hipLaunchKernelGGL(k_regions_count, chunk_grid, dim3(kRegionThreads), 0, s, region_ids, rank, (int)hw, min_area,
                       ws.nchunks, chunks);
    ISC_REGION_LAUNCHED();
    hipLaunchKernelGGL(k_regions_offsets, dim3(B), dim3(256), 0, s, chunks, ws.nchunks, num_regions);
    ISC_REGION_LAUNCHED();
    hipLaunchKernelGGL(k_regions_number, chunk_grid, dim3(kRegionThreads), 0, s, labels, region_ids, rank, (int)hw, min_area,
                       ws.nchunks, chunks, R, region_label, region_area, region_anchor);
    ISC_REGION_LAUNCHED();
    const RegionTables tb = {region_box, sums, keys, R, key_stride};
    if (stats)
        hipLaunchKernelGGL(k_regions_final<true>, tile_grid, dim3(kRegionThreads), 0, s, labels, best, region_ids, rank, H, W,
                           labels_out, tb);
    else
        hipLaunchKernelGGL(k_regions_final<false>, tile_grid, dim3(kRegionThreads), 0, s, labels, best, region_ids, rank, H,
                           W, labels_out, tb);
    if (region_box || peaks) {
        ISC_REGION_LAUNCHED();
        hipLaunchKernelGGL(k_regions_finish, dim3((unsigned)table_blocks), dim3(256), 0, s, B, R, key_stride, hw,
                           num_regions, best, region_box, keys, region_peak, region_peak_score);
    }
#undef ISC_REGION_LAUNCHED
    return isc_launch_status();
}
