// Packing of embedding rows into the tile-contiguous, row-permuted bank layout (include/imagescry_hip.h:
// isc_bank_pack, isc_bank_unpack, isc_bank_packed_bytes, isc_bank_permutation), and of a row filter into the same row
// order (isc_row_mask_words, isc_row_mask_pack), and of row group codes (isc_row_groups_pack); in-place append to a bank
// packed for a reserved capacity and its growth (isc_bank_append, isc_bank_repack); removal, replacement and compaction of
// such a bank (isc_bank_remove, isc_bank_replace, isc_bank_repack_map, isc_row_mask_unpack); the int8 shadow of an fp16
// bank (isc_bank_shadow_bytes, isc_bank_quantize).
#include "bank_layout.h"
#include "bank_pack_row.h"
#include "isc_common.h"

namespace {

template <typename TIN, typename TOUT>
__global__ __launch_bounds__(256) void k_bank_pack(const TIN* __restrict__ x, int64_t n_rows, int d, int64_t ldx,
                                                   int64_t first_row, IscPerm pm, int normalize, float eps,
                                                   unsigned char* __restrict__ packed, int ks,
                                                   unsigned* __restrict__ norm_bound) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    isc_pack_row<TIN, TOUT>(x + r * ldx, d, isc_perm_pos(pm, first_row + r), normalize, eps, packed, ks, norm_bound,
                            threadIdx.x & 63);
}

// In-place append to a bank laid out for `pm.n` = capacity rows (isc_bank_append): k_bank_pack's row, then the row's bit
// in the fill bitmap -- an atomic OR: 32 positions share a word and other waves of the launch set its other bits -- and
// its group code (negative -> -2, as k_row_groups_pack writes it).
template <typename TIN, typename TOUT>
__global__ __launch_bounds__(256) void k_bank_append(const TIN* __restrict__ x, int64_t n_rows, int d, int64_t ldx,
                                                     int64_t first_row, IscPerm pm, int normalize, float eps,
                                                     unsigned char* __restrict__ packed, int ks,
                                                     unsigned* __restrict__ norm_bound, uint32_t* __restrict__ fill_mask,
                                                     const int32_t* __restrict__ codes,
                                                     int32_t* __restrict__ packed_codes) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = isc_perm_pos(pm, first_row + r);
    isc_pack_row<TIN, TOUT>(x + r * ldx, d, row, normalize, eps, packed, ks, norm_bound, lane);
    if (lane == 0) {
        atomicOr(fill_mask + (row >> 5), 1u << (row & 31));
        if (packed_codes) {
            const int32_t c = codes[r];
            packed_codes[row] = c < 0 ? -2 : c;
        }
    }
}

// Growth of an appendable bank (isc_bank_repack): one wave per ORIGINAL row moves the row's K-step segments, 16 bytes a
// lane (8 lanes per 128-byte segment), from its position under the source permutation to its position under the
// destination's, byte for byte; its group code moves with it and its fill bit is set.
__global__ __launch_bounds__(256) void k_bank_repack(const unsigned char* __restrict__ src, IscPerm spm,
                                                     unsigned char* __restrict__ dst, IscPerm dpm, int ks,
                                                     int64_t first_row, int64_t n_rows,
                                                     const int32_t* __restrict__ src_codes,
                                                     int32_t* __restrict__ dst_codes, uint32_t* __restrict__ dst_fill) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t from = isc_perm_pos(spm, first_row + r), to = isc_perm_pos(dpm, first_row + r);
    for (int c = lane; c < ks * 8; c += 64)
        *reinterpret_cast<uint4*>(dst + isc_packed_offset(to, c >> 3, ks) + (c & 7) * 16) =
            *reinterpret_cast<const uint4*>(src + isc_packed_offset(from, c >> 3, ks) + (c & 7) * 16);
    if (lane == 0) {
        atomicOr(dst_fill + (to >> 5), 1u << (to & 31));
        if (dst_codes) dst_codes[to] = src_codes[from];
    }
}

// In-place removal (isc_bank_remove): one thread per index clears the row's bit in the fill bitmap -- an atomic AND: 32
// positions share a word, and the list may name a row twice.  Only the thread whose atomic saw the bit set owns the
// removal: it is counted (one atomic per wave), its group code becomes -2 and its group's count goes down by one.  An
// index outside [0, n_filled) is skipped; row bytes are not touched.
__global__ __launch_bounds__(256) void k_bank_remove(const int64_t* __restrict__ rows, int64_t n_rows, int64_t n_filled,
                                                     IscPerm pm, uint32_t* __restrict__ fill_mask,
                                                     int32_t* __restrict__ packed_codes,
                                                     unsigned long long* __restrict__ group_counts,
                                                     unsigned long long* __restrict__ removed_count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool won = false;
    if (i < n_rows) {
        const int64_t r = rows[i];
        if (r >= 0 && r < n_filled) {
            const int64_t pos = isc_perm_pos(pm, r);
            const uint32_t bit = 1u << (pos & 31);
            won = (atomicAnd(fill_mask + (pos >> 5), ~bit) & bit) != 0;
            if (won && packed_codes) {
                const int32_t c = packed_codes[pos];
                packed_codes[pos] = -2;
                if (group_counts && c >= 0) atomicAdd(group_counts + c, ~0ull);  // - 1 of the int64 count
            }
        }
    }
    const unsigned long long bits = __ballot(won);
    if (removed_count && won && (threadIdx.x & 63) == __ffsll(bits) - 1)
        atomicAdd(removed_count, (unsigned long long)__popcll(bits));
}

// In-place replacement (isc_bank_replace): k_bank_pack's row written at the position of ORIGINAL row row_index[r].  The
// wave reads the row's fill bit first: a removed (or never filled) row stays as it is.  An index outside [0, capacity) is
// skipped.
template <typename TIN, typename TOUT>
__global__ __launch_bounds__(256) void k_bank_replace(const TIN* __restrict__ x, int64_t n_rows, int d, int64_t ldx,
                                                      const int64_t* __restrict__ row_index, IscPerm pm, int normalize,
                                                      float eps, unsigned char* __restrict__ packed, int ks,
                                                      unsigned* __restrict__ norm_bound,
                                                      const uint32_t* __restrict__ fill_mask) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int64_t orig = row_index[r];
    if (orig < 0 || orig >= pm.n) return;
    const int64_t row = isc_perm_pos(pm, orig);
    if (fill_mask && !((fill_mask[row >> 5] >> (row & 31)) & 1u)) return;
    isc_pack_row<TIN, TOUT>(x + r * ldx, d, row, normalize, eps, packed, ks, norm_bound, threadIdx.x & 63);
}

// Compaction of an appendable bank (isc_bank_repack_map): k_bank_repack with the destination row taken from an index map:
// ORIGINAL row first_row + r of the source goes to ORIGINAL row new_index[first_row + r] of the destination; a negative
// entry (a removed row) or one past the destination's rows moves nothing.
__global__ __launch_bounds__(256) void k_bank_repack_map(const unsigned char* __restrict__ src, IscPerm spm,
                                                         unsigned char* __restrict__ dst, IscPerm dpm, int ks,
                                                         int64_t first_row, int64_t n_rows,
                                                         const int32_t* __restrict__ src_codes,
                                                         int32_t* __restrict__ dst_codes, uint32_t* __restrict__ dst_fill,
                                                         const int64_t* __restrict__ new_index) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int64_t ni = new_index[first_row + r];
    if (ni < 0 || ni >= dpm.n) return;
    const int lane = threadIdx.x & 63;
    const int64_t from = isc_perm_pos(spm, first_row + r), to = isc_perm_pos(dpm, ni);
    for (int c = lane; c < ks * 8; c += 64)
        *reinterpret_cast<uint4*>(dst + isc_packed_offset(to, c >> 3, ks) + (c & 7) * 16) =
            *reinterpret_cast<const uint4*>(src + isc_packed_offset(from, c >> 3, ks) + (c & 7) * 16);
    if (lane == 0) {
        atomicOr(dst_fill + (to >> 5), 1u << (to & 31));
        if (dst_codes) dst_codes[to] = src_codes[from];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bank_unpack(const unsigned char* __restrict__ packed, int d, int ks,
                                                     IscPerm pm, int64_t first_row, int64_t n_rows,
                                                     T* __restrict__ y, int64_t ldy) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = isc_perm_pos(pm, first_row + r);
    for (int e = lane; e < d; e += 64) y[r * ldy + e] = isc_packed_load<T>(packed, row, e, ks);
}

// Row filter of a masked search: one thread per PACKED position p of the padded bank, allowed iff p < n and
// allow[orig(p)] != 0; a wave's ballot is two bitmap words, written by lanes 0 and 32.  The allowed rows of the wave are
// added to `allowed_count` with one atomic.
__global__ __launch_bounds__(256) void k_row_mask_pack(const uint8_t* __restrict__ allow, IscPerm pm,
                                                       uint32_t* __restrict__ packed_mask,
                                                       unsigned long long* __restrict__ allowed_count) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool ok = p < pm.n && allow[isc_perm_orig(pm, p)] != 0;
    const unsigned long long bits = __ballot(ok);
    if (lane == 0) packed_mask[p >> 5] = (uint32_t)bits;
    if (lane == 32) packed_mask[p >> 5] = (uint32_t)(bits >> 32);
    if (allowed_count && lane == 0 && bits != 0ull) atomicAdd(allowed_count, (unsigned long long)__popcll(bits));
}

// Inverse of k_row_mask_pack for the first n_rows ORIGINAL rows: one thread per row reads the bit at its packed position.
__global__ __launch_bounds__(256) void k_row_mask_unpack(const uint32_t* __restrict__ packed_mask, IscPerm pm,
                                                         int64_t n_rows, uint8_t* __restrict__ allow) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = isc_perm_pos(pm, r);
    allow[r] = (uint8_t)((packed_mask[p >> 5] >> (p & 31)) & 1u);
}

// Row group codes of a grouped search: one thread per PACKED position p of the padded bank; code[orig(p)] for p < n, -2
// for the padding and for a negative code (a query code < 0 is read as -1: it matches neither).
__global__ __launch_bounds__(256) void k_row_groups_pack(const int32_t* __restrict__ codes, IscPerm pm,
                                                         int32_t* __restrict__ packed_codes) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t c = p < pm.n ? codes[isc_perm_orig(pm, p)] : -2;
    packed_codes[p] = c < 0 ? -2 : c;
}

// int8 shadow of a packed fp16 bank (bank_layout.h: IscShadowRec; isc_bank_quantize).  One workgroup per tile: a first
// sweep finds the tile's largest magnitude, a second one (the tile's 32 KiB blocks come from the L2 then) quantises with
// round to nearest and writes the int8 blocks; the per-row sums of the squared residuals and of the squared integers are
// taken in float64 -- (double)x * (double)c_t - X is exact there: 11 x 24 significant bits minus a small integer -- and
// their square roots go to the record rounded UP (x (1 + 1e-6) covers the float64 sum of <= 8192 terms, the sqrt and the
// conversion to float32).  Thread t covers 16-byte output chunk t & 7 of rows (t >> 3) + 32 i: the eight lanes of a row
// are neighbours, so a row's sums are three shuffles.
__global__ __launch_bounds__(256) void k_bank_quantize(const unsigned char* __restrict__ bank, int ks, int ks8,
                                                       unsigned char* __restrict__ shadow,
                                                       IscShadowRec* __restrict__ recs) {
    __shared__ float mx_sh[4];
    __shared__ double sum_sh[2][4];
    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char* src = bank + tile * ks * (int64_t)ISC_TILE_KSTEP_BYTES;
    float mx = 0.f;
    int bad = 0;
    for (int i = tid; i < ks * (ISC_TILE_KSTEP_BYTES / 16); i += 256) {
        const uint4 raw = *reinterpret_cast<const uint4*>(src + (size_t)i * 16);
        const _Float16* h = reinterpret_cast<const _Float16*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = fabsf((float)h[j]);
            bad |= !(v <= 65504.f) ? 1 : 0;  // inf or NaN
            mx = fmaxf(mx, v);
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) mx_sh[wave] = mx;
    bad = __syncthreads_or(bad);
    mx = fmaxf(fmaxf(mx_sh[0], mx_sh[1]), fmaxf(mx_sh[2], mx_sh[3]));
    const float c = mx > 0.f ? 127.f / mx : 1.f;  // <= 127 / 2^-24: finite
    const int row0 = tid >> 3, c8 = tid & 7;
    double rs[8], qs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rs[i] = qs[i] = 0.0;
    unsigned char* dst = shadow + tile * ks8 * (int64_t)ISC_TILE_KSTEP_BYTES;
    for (int s8 = 0; s8 < ks8; ++s8) {
        const int s = 2 * s8 + (c8 >> 2);  // the fp16 K step that holds dims 128 s8 + 16 c8 .. + 15
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = row0 + 32 * i;
            _Float16 h[16];
            if (s < ks) {
                const uint4* p = reinterpret_cast<const uint4*>(src + ((size_t)s * ISC_TILE_ROWS + row) * ISC_KSTEP_BYTES +
                                                                (c8 & 3) * 32);
                reinterpret_cast<uint4*>(h)[0] = p[0];
                reinterpret_cast<uint4*>(h)[1] = p[1];
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) h[j] = (_Float16)0.f;
            }
            signed char out[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float v = (float)h[j];
                float x = bad ? 0.f : rintf(v * c);
                x = fminf(fmaxf(x, -127.f), 127.f);
                const double r = bad ? 0.0 : (double)v * (double)c - (double)x;
                rs[i] = fma(r, r, rs[i]);
                qs[i] = fma((double)x, (double)x, qs[i]);
                out[j] = (signed char)(int)x;
            }
            *reinterpret_cast<uint4*>(dst + ((size_t)s8 * ISC_TILE_ROWS + row) * ISC_KSTEP_BYTES + c8 * 16) =
                *reinterpret_cast<const uint4*>(out);
        }
    }
    double rmax = 0.0, qmax = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            rs[i] += __shfl_xor(rs[i], off, 64);
            qs[i] += __shfl_xor(qs[i], off, 64);
        }
        rmax = fmax(rmax, rs[i]);
        qmax = fmax(qmax, qs[i]);
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
        rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
        qmax = fmax(qmax, __shfl_xor(qmax, off, 64));
    }
    if (lane == 0) {
        sum_sh[0][wave] = rmax;
        sum_sh[1][wave] = qmax;
    }
    __syncthreads();
    if (tid == 0) {
        rmax = fmax(fmax(sum_sh[0][0], sum_sh[0][1]), fmax(sum_sh[0][2], sum_sh[0][3]));
        qmax = fmax(fmax(sum_sh[1][0], sum_sh[1][1]), fmax(sum_sh[1][2], sum_sh[1][3]));
        IscShadowRec rec;
        rec.scale = mx > 0.f ? mx / 127.f : 1.f;
        rec.inv_scale = c;
        rec.resid = (float)sqrt(rmax) * (1.f + 1e-6f);
        rec.qnorm = bad ? INFINITY : (float)sqrt(qmax) * (1.f + 1e-6f);
        recs[tile] = rec;
    }
}

int check_dtype(int dtype) { return dtype == ISC_F16 || dtype == ISC_F32; }

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// x with (a * x) mod n == 1 (extended Euclid; a and n coprime, n >= 2)
int64_t mod_inverse(int64_t a, int64_t n) {
    int64_t t = 0, nt = 1, r = n, nr = a % n;
    while (nr) {
        const int64_t q = r / nr;
        int64_t tmp = t - q * nt;
        t = nt;
        nt = tmp;
        tmp = r - q * nr;
        r = nr;
        nr = tmp;
    }
    return t < 0 ? t + n : t;
}

}  // namespace

IscPerm isc_make_perm(int64_t n) {
    IscPerm pm;
    pm.n = n;
    if (n <= 2) {  // identity
        pm.mul = pm.mul_inv = 1;
        return pm;
    }
    int64_t m = (int64_t)((double)n * 0.6180339887498949);
    if (m < 1) m = 1;
    while (gcd64(m, n) != 1) ++m;  // terminates: n - 1 is coprime to n
    pm.mul = m % n;
    pm.mul_inv = mod_inverse(pm.mul, n);
    return pm;
}

extern "C" int isc_bank_permutation(int64_t N, int64_t* mul, int64_t* mul_inv) {
    ISC_REQUIRE(N > 0 && N <= 0x7fffffff && mul && mul_inv);
    const IscPerm pm = isc_make_perm(N);
    *mul = pm.mul;
    *mul_inv = pm.mul_inv;
    return ISC_OK;
}

extern "C" int isc_bank_packed_bytes(int dtype, int64_t N, int D, size_t* bytes) {
    ISC_REQUIRE(bytes && check_dtype(dtype) && N > 0 && D > 0);
    const int esz = dtype == ISC_F16 ? 2 : 4;
    const int64_t tiles = isc_ceil_div<int64_t>(N, ISC_TILE_ROWS);
    *bytes = (size_t)tiles * isc_ksteps(D, esz) * ISC_TILE_KSTEP_BYTES;
    return ISC_OK;
}

extern "C" int isc_bank_pack(const void* rows, int in_dtype, int64_t n_rows, int D, int64_t ldx, int64_t first_row,
                             int64_t n_total, int normalize, float eps, void* packed, int dtype, float* norm_bound,
                             void* stream) {
    ISC_REQUIRE(rows && packed && check_dtype(in_dtype) && check_dtype(dtype));
    ISC_REQUIRE(n_rows > 0 && D > 0 && ldx >= D && first_row >= 0);
    ISC_REQUIRE(n_total >= first_row + n_rows && n_total <= 0x7fffffff);
    if (!isc_aligned(packed, 16)) return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    const int ks = isc_ksteps(D, dtype == ISC_F16 ? 2 : 4);
    unsigned char* out = static_cast<unsigned char*>(packed);
    hipStream_t s = isc_stream(stream);
    const IscPerm pm = isc_make_perm(n_total);
    const dim3 grid((unsigned)blocks), block(256);
#define ISC_PACK(TIN, TOUT)                                                                                         \
    hipLaunchKernelGGL((k_bank_pack<TIN, TOUT>), grid, block, 0, s, static_cast<const TIN*>(rows), n_rows, D, ldx, \
                       first_row, pm, normalize, eps, out, ks, reinterpret_cast<unsigned*>(norm_bound))
    if (in_dtype == ISC_F32 && dtype == ISC_F16) ISC_PACK(float, _Float16);
    else if (in_dtype == ISC_F32 && dtype == ISC_F32) ISC_PACK(float, float);
    else if (in_dtype == ISC_F16 && dtype == ISC_F16) ISC_PACK(_Float16, _Float16);
    else ISC_PACK(_Float16, float);
#undef ISC_PACK
    return isc_launch_status();
}

extern "C" int isc_bank_append(const void* rows, int in_dtype, int64_t n_rows, int D, int64_t ldx, int64_t first_row,
                               int64_t capacity, int normalize, float eps, void* packed, int dtype, float* norm_bound,
                               uint32_t* fill_mask, const int32_t* codes, int32_t* packed_codes, void* stream) {
    ISC_REQUIRE(rows && packed && fill_mask && check_dtype(in_dtype) && check_dtype(dtype));
    ISC_REQUIRE(n_rows > 0 && D > 0 && ldx >= D && first_row >= 0);
    ISC_REQUIRE(capacity >= first_row + n_rows && capacity <= 0x7ffffffe);
    ISC_REQUIRE((codes == nullptr) == (packed_codes == nullptr));
    if (!isc_aligned(packed, 16) || !isc_aligned(fill_mask, 4) || !isc_aligned(codes, 4) || !isc_aligned(packed_codes, 16))
        return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    const int ks = isc_ksteps(D, dtype == ISC_F16 ? 2 : 4);
    unsigned char* out = static_cast<unsigned char*>(packed);
    hipStream_t s = isc_stream(stream);
    const IscPerm pm = isc_make_perm(capacity);
    const dim3 grid((unsigned)blocks), block(256);
#define ISC_APPEND(TIN, TOUT)                                                                                         \
    hipLaunchKernelGGL((k_bank_append<TIN, TOUT>), grid, block, 0, s, static_cast<const TIN*>(rows), n_rows, D, ldx, \
                       first_row, pm, normalize, eps, out, ks, reinterpret_cast<unsigned*>(norm_bound), fill_mask,    \
                       codes, packed_codes)
    if (in_dtype == ISC_F32 && dtype == ISC_F16) ISC_APPEND(float, _Float16);
    else if (in_dtype == ISC_F32 && dtype == ISC_F32) ISC_APPEND(float, float);
    else if (in_dtype == ISC_F16 && dtype == ISC_F16) ISC_APPEND(_Float16, _Float16);
    else ISC_APPEND(_Float16, float);
#undef ISC_APPEND
    return isc_launch_status();
}

extern "C" int isc_bank_repack(const void* src_packed, int64_t src_capacity, void* dst_packed, int64_t dst_capacity,
                               int dtype, int D, int64_t first_row, int64_t n_rows, const int32_t* src_codes,
                               int32_t* dst_codes, uint32_t* dst_fill_mask, void* stream) {
    ISC_REQUIRE(src_packed && dst_packed && dst_fill_mask && src_packed != dst_packed && check_dtype(dtype));
    ISC_REQUIRE(n_rows > 0 && D > 0 && first_row >= 0);
    ISC_REQUIRE(src_capacity >= first_row + n_rows && dst_capacity >= first_row + n_rows);
    ISC_REQUIRE(src_capacity <= 0x7ffffffe && dst_capacity <= 0x7ffffffe);
    ISC_REQUIRE((src_codes == nullptr) == (dst_codes == nullptr));
    if (!isc_aligned(src_packed, 16) || !isc_aligned(dst_packed, 16) || !isc_aligned(dst_fill_mask, 4) ||
        !isc_aligned(src_codes, 4) || !isc_aligned(dst_codes, 16))
        return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_bank_repack, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream),
                       static_cast<const unsigned char*>(src_packed), isc_make_perm(src_capacity),
                       static_cast<unsigned char*>(dst_packed), isc_make_perm(dst_capacity),
                       isc_ksteps(D, dtype == ISC_F16 ? 2 : 4), first_row, n_rows, src_codes, dst_codes, dst_fill_mask);
    return isc_launch_status();
}

extern "C" int isc_bank_remove(const int64_t* rows, int64_t n_rows, int64_t n_filled, int64_t capacity,
                               uint32_t* fill_mask, int32_t* packed_codes, int64_t* group_counts, int64_t* removed_count,
                               void* stream) {
    ISC_REQUIRE(rows && fill_mask && n_rows > 0 && n_filled >= 0);
    ISC_REQUIRE(capacity > 0 && capacity >= n_filled && capacity <= 0x7ffffffe);
    ISC_REQUIRE(!group_counts || packed_codes);
    if (!isc_aligned(rows, 8) || !isc_aligned(fill_mask, 4) || !isc_aligned(packed_codes, 16) ||
        !isc_aligned(group_counts, 8) || !isc_aligned(removed_count, 8))
        return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 256);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_bank_remove, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream), rows, n_rows, n_filled,
                       isc_make_perm(capacity), fill_mask, packed_codes,
                       reinterpret_cast<unsigned long long*>(group_counts),
                       reinterpret_cast<unsigned long long*>(removed_count));
    return isc_launch_status();
}

extern "C" int isc_bank_replace(const void* rows, int in_dtype, int64_t n_rows, int D, int64_t ldx,
                                const int64_t* row_index, int64_t capacity, int normalize, float eps, void* packed,
                                int dtype, float* norm_bound, const uint32_t* fill_mask, void* stream) {
    ISC_REQUIRE(rows && row_index && packed && check_dtype(in_dtype) && check_dtype(dtype));
    ISC_REQUIRE(n_rows > 0 && D > 0 && ldx >= D);
    ISC_REQUIRE(capacity > 0 && capacity <= 0x7ffffffe);
    if (!isc_aligned(packed, 16) || !isc_aligned(row_index, 8) || !isc_aligned(fill_mask, 4)) return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    const int ks = isc_ksteps(D, dtype == ISC_F16 ? 2 : 4);
    unsigned char* out = static_cast<unsigned char*>(packed);
    hipStream_t s = isc_stream(stream);
    const IscPerm pm = isc_make_perm(capacity);
    const dim3 grid((unsigned)blocks), block(256);
#define ISC_REPLACE(TIN, TOUT)                                                                                         \
    hipLaunchKernelGGL((k_bank_replace<TIN, TOUT>), grid, block, 0, s, static_cast<const TIN*>(rows), n_rows, D, ldx, \
                       row_index, pm, normalize, eps, out, ks, reinterpret_cast<unsigned*>(norm_bound), fill_mask)
    if (in_dtype == ISC_F32 && dtype == ISC_F16) ISC_REPLACE(float, _Float16);
    else if (in_dtype == ISC_F32 && dtype == ISC_F32) ISC_REPLACE(float, float);
    else if (in_dtype == ISC_F16 && dtype == ISC_F16) ISC_REPLACE(_Float16, _Float16);
    else ISC_REPLACE(_Float16, float);
#undef ISC_REPLACE
    return isc_launch_status();
}

extern "C" int isc_bank_repack_map(const void* src_packed, int64_t src_capacity, void* dst_packed, int64_t dst_capacity,
                                   int dtype, int D, int64_t first_row, int64_t n_rows, const int32_t* src_codes,
                                   int32_t* dst_codes, uint32_t* dst_fill_mask, const int64_t* new_index, void* stream) {
    ISC_REQUIRE(src_packed && dst_packed && dst_fill_mask && new_index && src_packed != dst_packed && check_dtype(dtype));
    ISC_REQUIRE(n_rows > 0 && D > 0 && first_row >= 0);
    ISC_REQUIRE(src_capacity >= first_row + n_rows && dst_capacity > 0);
    ISC_REQUIRE(src_capacity <= 0x7ffffffe && dst_capacity <= 0x7ffffffe);
    ISC_REQUIRE((src_codes == nullptr) == (dst_codes == nullptr));
    if (!isc_aligned(src_packed, 16) || !isc_aligned(dst_packed, 16) || !isc_aligned(dst_fill_mask, 4) ||
        !isc_aligned(src_codes, 4) || !isc_aligned(dst_codes, 16) || !isc_aligned(new_index, 8))
        return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_bank_repack_map, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream),
                       static_cast<const unsigned char*>(src_packed), isc_make_perm(src_capacity),
                       static_cast<unsigned char*>(dst_packed), isc_make_perm(dst_capacity),
                       isc_ksteps(D, dtype == ISC_F16 ? 2 : 4), first_row, n_rows, src_codes, dst_codes, dst_fill_mask,
                       new_index);
    return isc_launch_status();
}

extern "C" int isc_bank_unpack(const void* packed, int dtype, int D, int64_t n_total, int64_t first_row,
                               int64_t n_rows, void* rows, int64_t ldy, void* stream) {
    ISC_REQUIRE(packed && rows && check_dtype(dtype) && D > 0 && n_rows > 0 && first_row >= 0 && ldy >= D);
    ISC_REQUIRE(n_total >= first_row + n_rows && n_total <= 0x7fffffff);
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 4);
    if (blocks > 0x7fffffff) return ISC_ERR_UNSUPPORTED;
    const unsigned char* in = static_cast<const unsigned char*>(packed);
    const IscPerm pm = isc_make_perm(n_total);
    if (dtype == ISC_F16)
        hipLaunchKernelGGL(k_bank_unpack<_Float16>, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream), in, D,
                           isc_ksteps(D, 2), pm, first_row, n_rows, static_cast<_Float16*>(rows), ldy);
    else
        hipLaunchKernelGGL(k_bank_unpack<float>, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream), in, D,
                           isc_ksteps(D, 4), pm, first_row, n_rows, static_cast<float*>(rows), ldy);
    return isc_launch_status();
}

extern "C" int isc_row_mask_words(int64_t N, size_t* words) {
    ISC_REQUIRE(words && N > 0 && N <= 0x7ffffffe);
    *words = (size_t)isc_ceil_div<int64_t>(N, ISC_TILE_ROWS) * (ISC_TILE_ROWS / 32);
    return ISC_OK;
}

extern "C" int isc_row_mask_pack(const uint8_t* allow, int64_t N, uint32_t* packed_mask, int64_t* allowed_count,
                                 void* stream) {
    ISC_REQUIRE(allow && packed_mask && N > 0 && N <= 0x7ffffffe);
    if (!isc_aligned(packed_mask, 4) || !isc_aligned(allowed_count, 8)) return ISC_ERR_ALIGNMENT;
    const int64_t tiles = isc_ceil_div<int64_t>(N, ISC_TILE_ROWS);
    hipLaunchKernelGGL(k_row_mask_pack, dim3((unsigned)tiles), dim3(256), 0, isc_stream(stream), allow, isc_make_perm(N),
                       packed_mask, reinterpret_cast<unsigned long long*>(allowed_count));
    return isc_launch_status();
}

extern "C" int isc_row_mask_unpack(const uint32_t* packed_mask, int64_t N, int64_t n_rows, uint8_t* allow, void* stream) {
    ISC_REQUIRE(packed_mask && allow && N > 0 && N <= 0x7ffffffe && n_rows > 0 && n_rows <= N);
    if (!isc_aligned(packed_mask, 4)) return ISC_ERR_ALIGNMENT;
    const int64_t blocks = isc_ceil_div<int64_t>(n_rows, 256);
    hipLaunchKernelGGL(k_row_mask_unpack, dim3((unsigned)blocks), dim3(256), 0, isc_stream(stream), packed_mask,
                       isc_make_perm(N), n_rows, allow);
    return isc_launch_status();
}

extern "C" int isc_row_groups_pack(const int32_t* codes, int64_t N, int32_t* packed_codes, void* stream) {
    ISC_REQUIRE(codes && packed_codes && N > 0 && N <= 0x7ffffffe);
    if (!isc_aligned(codes, 4) || !isc_aligned(packed_codes, 16)) return ISC_ERR_ALIGNMENT;
    const int64_t tiles = isc_ceil_div<int64_t>(N, ISC_TILE_ROWS);
    hipLaunchKernelGGL(k_row_groups_pack, dim3((unsigned)tiles), dim3(256), 0, isc_stream(stream), codes,
                       isc_make_perm(N), packed_codes);
    return isc_launch_status();
}

extern "C" int isc_bank_shadow_bytes(int64_t N, int D, size_t* bytes) {
    ISC_REQUIRE(bytes && N > 0 && N <= 0x7ffffffe && D > 0);
    *bytes = isc_shadow_bytes(N, D);
    return ISC_OK;
}

extern "C" int isc_bank_quantize(const void* packed, int64_t N, int D, void* shadow, size_t shadow_bytes, void* stream) {
    ISC_REQUIRE(packed && shadow && N > 0 && N <= 0x7ffffffe && D > 0);
    if (!isc_aligned(packed, 16) || !isc_aligned(shadow, 256)) return ISC_ERR_ALIGNMENT;
    if (shadow_bytes < isc_shadow_bytes(N, D)) return ISC_ERR_WORKSPACE;
    const int64_t tiles = isc_ceil_div<int64_t>(N, ISC_TILE_ROWS);
    unsigned char* out = static_cast<unsigned char*>(shadow);
    hipLaunchKernelGGL(k_bank_quantize, dim3((unsigned)tiles), dim3(256), 0, isc_stream(stream),
                       static_cast<const unsigned char*>(packed), isc_ksteps(D, 2), isc_shadow_ksteps(D), out,
                       reinterpret_cast<IscShadowRec*>(out + isc_shadow_data_bytes(N, D)));
    return isc_launch_status();
}
