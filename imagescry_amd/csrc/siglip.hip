// The two kernels a SigLIP image tower adds to the ViT encoder (include/imagescry_hip.h: isc_attention_f16_probe,
// isc_vit_assemble_plain): the one-query attention of its pooling head and the token assembly without a class row.
#include "isc_common.h"
#include "packed_matrix.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------
// One query against the T keys of one (image, head): out = softmax(q . k_t / 8) v.
//
// A bandwidth kernel: 2 * T * 128 bytes per workgroup and ~130 flops per key, so the only thing that matters is that
// every load instruction of a wave covers whole 128-byte head segments.  Eight lanes hold the eight 16-byte parts of one
// key (or value) row, a wave eight consecutive tokens -- in the packed layout ONE contiguous KiB, row-major eight
// 128-byte lines --, the four waves of the workgroup 32 tokens per step.  Pass 1 leaves the scores in LDS, the maximum
// and the sum of the exponentials are block reductions over them, pass 2 streams the values.  Keys and values are read
// once each; nothing is atomic and every reduction has one fixed order (the header states it).
//
// A sequence of more than PROBE_CHUNK keys repeats the two passes per chunk under a running maximum.
constexpr int PROBE_THREADS = 256;
constexpr int PROBE_WAVES = PROBE_THREADS / 64;
constexpr int PROBE_SLOTS = PROBE_THREADS / 8;  // tokens per step
constexpr int PROBE_CHUNK = 4096;               // scores held in LDS: vit.MAX_PATCHES
constexpr float PROBE_LOG2E = 1.4426950408889634f;

template <bool PACKED>
__global__ __launch_bounds__(PROBE_THREADS) void k_attention_probe(const _Float16* __restrict__ kv,
                                                                   const _Float16* __restrict__ q, int T, int heads,
                                                                   _Float16* __restrict__ out) {
    __shared__ float score[PROBE_CHUNK];
    __shared__ float wred[2][PROBE_WAVES];
    __shared__ __attribute__((aligned(16))) float vred[PROBE_WAVES][64];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int c = tid & 7;   // 16-byte part of the head's 128-byte segment
    const int j = tid >> 3;  // token slot
    const int b = blockIdx.x / heads;
    const int h = blockIdx.x - b * heads;
    const int cols = 2 * heads * 64;
    const int kcol = h * 64 + 8 * c;
    const int vcol = (heads + h) * 64 + 8 * c;
    const long long row0 = (long long)b * T;

    auto load = [&](long long row, int col) {
        const size_t o = PACKED ? pk_offset(row, col, cols) : (size_t)row * cols + col;
        return *reinterpret_cast<const half8*>(kv + o);
    };

    float qf[8];
    {
        const half8 qh = *reinterpret_cast<const half8*>(q + h * 64 + 8 * c);
#pragma unroll
        for (int i = 0; i < 8; ++i) qf[i] = (float)qh[i] * 0.125f;
    }

    float run_max = -INFINITY;  // over the chunks so far
    float lsum = 0.f;           // this thread's share of the sum of the exponentials
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;

    for (int t0 = 0; t0 < T; t0 += PROBE_CHUNK) {
        const int n = min(PROBE_CHUNK, T - t0);
        // ---- pass 1: the scores of tokens t0 .. t0 + n - 1
        for (int t = j; t < n; t += PROBE_SLOTS) {
            const half8 k = load(row0 + t0 + t, kcol);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(qf[i], (float)k[i], s);
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            if (c == 0) score[t] = s;
        }
        __syncthreads();
        // ---- the maximum
        float m = -INFINITY;
        for (int t = tid; t < n; t += PROBE_THREADS) m = fmaxf(m, score[t]);
        m = isc_wave_max(m);
        if (lane == 0) wred[0][wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wred[0][0], wred[0][1]), fmaxf(wred[0][2], wred[0][3]));
        const float new_max = fmaxf(run_max, m);
        // what the earlier chunks left is brought to the new maximum (the first chunk: zeros times zero)
        const float rescale = __builtin_amdgcn_exp2f((run_max - new_max) * PROBE_LOG2E);
        run_max = new_max;
        lsum *= rescale;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] *= rescale;
        // ---- the exponentials, in place
        for (int t = tid; t < n; t += PROBE_THREADS) {
            const float p = __builtin_amdgcn_exp2f((score[t] - new_max) * PROBE_LOG2E);
            score[t] = p;
            lsum += p;
        }
        __syncthreads();
        // ---- pass 2: the values
        for (int t = j; t < n; t += PROBE_SLOTS) {
            const half8 v = load(row0 + t0 + t, vcol);
            const float p = score[t];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(p, (float)v[i], acc[i]);
        }
        __syncthreads();  // the next chunk overwrites score and wred
    }

    // ---- the sum: butterfly over the wave, then the four waves in order
    lsum = isc_wave_sum(lsum);
    if (lane == 0) wred[1][wave] = lsum;
    // ---- the accumulators: the eight token slots of a wave, then the four waves in order
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        acc[i] += __shfl_xor(acc[i], 8, 64);
        acc[i] += __shfl_xor(acc[i], 16, 64);
        acc[i] += __shfl_xor(acc[i], 32, 64);
    }
    if (lane < 8) {
        *reinterpret_cast<f32x4*>(&vred[wave][8 * c]) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(&vred[wave][8 * c + 4]) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
    if (tid < 8) {
        const float l = ((wred[1][0] + wred[1][1]) + wred[1][2]) + wred[1][3];
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int d = 8 * c + i;
            const float a = ((vred[0][d] + vred[1][d]) + vred[2][d]) + vred[3][d];
            o[i] = (_Float16)__fdiv_rn(a, l);
        }
        const int ocols = heads * 64;
        const size_t oo = PACKED ? pk_offset(b, h * 64 + 8 * c, ocols) : (size_t)b * ocols + h * 64 + 8 * c;
        *reinterpret_cast<half8*>(out + oo) = o;
    }
}

// tokens[b][j] = patch_embed[b * P + j] + pos[j]: k_vit_assemble without its class row
__global__ __launch_bounds__(256) void k_vit_assemble_plain(const float* __restrict__ pe, const float* __restrict__ pos,
                                                            size_t table4, size_t total4, float* __restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(pe + i * 4);
        v += *reinterpret_cast<const f32x4*>(pos + (i % table4) * 4);
        *reinterpret_cast<f32x4*>(y + i * 4) = v;
    }
}

}  // namespace

extern "C" int isc_attention_f16_probe(const void* kv, const void* q, int B, int T, int heads, int head_dim, void* out,
                                       int packed, void* stream) {
    ISC_REQUIRE(kv && q && out && B > 0 && T > 0 && heads > 0);
    if (head_dim != 64) return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(kv, 16) || !isc_aligned(q, 16) || !isc_aligned(out, 16)) return ISC_ERR_ALIGNMENT;
    if ((long long)B * T > 0x7fffffffLL || (long long)B * heads > 0x7fffffffLL || heads > (1 << 22))
        return ISC_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(B * heads));
    isc_timing_begin(ISC_KERNEL_ATTENTION_PROBE, isc_stream(stream));
    if (packed)
        hipLaunchKernelGGL(k_attention_probe<true>, grid, dim3(PROBE_THREADS), 0, isc_stream(stream),
                           reinterpret_cast<const _Float16*>(kv), reinterpret_cast<const _Float16*>(q), T, heads,
                           reinterpret_cast<_Float16*>(out));
    else
        hipLaunchKernelGGL(k_attention_probe<false>, grid, dim3(PROBE_THREADS), 0, isc_stream(stream),
                           reinterpret_cast<const _Float16*>(kv), reinterpret_cast<const _Float16*>(q), T, heads,
                           reinterpret_cast<_Float16*>(out));
    isc_timing_end(ISC_KERNEL_ATTENTION_PROBE, isc_stream(stream));
    return isc_launch_status();
}

extern "C" int isc_vit_assemble_plain(const float* patch_embed, const float* pos_embed, int B, int P, int D,
                                      float* tokens, void* stream) {
    ISC_REQUIRE(patch_embed && pos_embed && tokens && B > 0 && P > 0 && D > 0);
    if (D % 4 != 0) return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(patch_embed, 16) || !isc_aligned(pos_embed, 16) || !isc_aligned(tokens, 16)) return ISC_ERR_ALIGNMENT;
    const size_t table4 = (size_t)P * (D / 4);
    const size_t total4 = (size_t)B * table4;
    const size_t blocks = isc_ceil_div<size_t>(total4, 256);
    hipLaunchKernelGGL(k_vit_assemble_plain, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0,
                       isc_stream(stream), patch_embed, pos_embed, table4, total4, tokens);
    return isc_launch_status();
}
