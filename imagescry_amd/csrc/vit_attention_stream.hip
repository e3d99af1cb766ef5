// Multi-head self-attention for sequences of any length (head size 64): isc_attention_f16_stream.  The keys and values
// are STREAMED through LDS in chunks and the softmax is kept online (running maximum and sum per query, flash style),
// so neither a head's keys nor a query's score row has to fit anywhere.  isc_attention_f16 (vit.hip) holds both whole
// and stops at T = 224; this kernel is what vit._encode calls above that.  Operands, layouts and the result are
// those of isc_attention_f16.
//
// A workgroup of eight waves owns (image, head, block of AS_QB = 128 queries), a wave 16 of those queries, and all
// eight walk the keys in chunks of AS_KC = 64:
//   S^T[key][query] = K . Q^T / 8      4 key blocks x 2 MFMAs (mfma_f32_16x16x32_f16); a lane holds ONE query (lane & 15)
//                                       and 4 keys of every 16-key block (att_score_block, vit_attention.h, as every
//                                       piece shared with isc_attention_f16)
//   m' = max(m, chunk maximum), alpha = exp2((m - m') log2 e)          float32; the first chunk has no rescale, so
//   p  = exp2(fma(s, log2 e, -m' log2 e))                              -inf - (-inf) never occurs
//   l  = l alpha + sum p               per LANE (a query's four lanes see the same alpha); the lanes are added once, at
//                                       the end
//   O^T[d][query] = O^T alpha + V^T . P^T    the SAME alpha value as l; P rounded to fp16 stays in registers as the
//                                       P^T operand, V stays row-major in LDS and is read transposed (att_pv_step,
//                                       which has the slot mapping)
// The chunks are double-buffered and register-staged: the global loads of chunk c + 1 are issued before the arithmetic
// of chunk c and written to the other LDS buffer behind it, one barrier per chunk.  Key rows at or past T are staged
// as zeros (they may not exist -- row-major -- or hold anything -- packed padding) and their scores set to -inf behind
// the MFMA: 0 probability times 0 value.  Only the last chunk can hold such keys, and only it pays for the masks
// (as_chunk<true>), where it also skips the 16-key blocks that lie wholly past T.
//
// Workgroups of one (image, head) re-read the same keys and values, so they are placed on ONE XCD (workgroup i runs
// on XCD i % 8): the heads are dealt to the XCDs round robin and the query blocks of a head follow each other there.
#include "vit_attention.h"

namespace {

constexpr int AS_QB = 128;      // queries per workgroup (16 per wave)
constexpr int AS_KC = 64;       // keys per chunk; a multiple of 32 (att_pv_step pairs key blocks in 32s)
constexpr int AS_THREADS = 512;
constexpr int AS_NKB = AS_KC / 16;
constexpr int AS_XCDS = 8;
static_assert(AS_KC % 32 == 0 && AS_QB == AS_THREADS / 64 * 16 && AS_KC * 8 == AS_THREADS, "geometry");

// One chunk of AS_KC staged keys / values against a wave's 16 queries.  qf: the lane's two query fragments, scaled by
// 1/8; left = T - (first key of the chunk) > 0, only looked at when TAIL (left < AS_KC); first: chunk 0, no rescale.
template <bool TAIL>
__device__ __forceinline__ void as_chunk(const _Float16* __restrict__ Ks, const _Float16* __restrict__ Vs,
                                         const half8 (&qf)[2], int left, bool first, int qi, int g, float& m, float& l,
                                         f32x4 (&o)[4]) {
    constexpr float LOG2E = 1.4426950408889634f;
    f32x4 s[AS_NKB];
#pragma unroll
    for (int kb = 0; kb < AS_NKB; ++kb) {
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!TAIL || kb * 16 < left) a = att_score_block(Ks, kb, qf, qi, g);  // (wave-uniform) a block wholly past T is not computed
        if (TAIL) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kb * 16 + g * 4 + r >= left) a[r] = -INFINITY;
        }
        s[kb] = a;
    }
    float cm = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < AS_NKB; ++kb) cm = fmaxf(cm, fmaxf(fmaxf(s[kb][0], s[kb][1]), fmaxf(s[kb][2], s[kb][3])));
    cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
    cm = fmaxf(cm, __shfl_xor(cm, 32, 64));  // finite: every chunk holds at least one key below T
    if (first) {
        m = cm;
    } else {
        const float mn = fmaxf(m, cm);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);  // <= 1; ONE value for l and O
        m = mn;
        l *= alpha;
#pragma unroll
        for (int db = 0; db < 4; ++db) o[db] *= alpha;
    }
    const float mxl = -m * LOG2E;
#pragma unroll
    for (int kb = 0; kb < AS_NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s[kb][r], LOG2E, mxl));  // masked keys: exp2(-inf) = 0
            s[kb][r] = e;
            l += e;
        }
#pragma unroll
    for (int ks = 0; ks < AS_NKB / 2; ++ks) {
        if (TAIL && ks * 32 >= left) break;  // (wave-uniform) every probability of this step is 0
        att_pv_step(Vs, ks, s[2 * ks], s[2 * ks + 1], qi, g, o);
    }
}

// pairs = B * heads, nqb = query blocks per pair; the grid is ceil(pairs / 8) * 8 * nqb workgroups.  QPART / KPART: the
// parts of the row the query operand and the staged key rows come from (vit_attention.h).
template <bool PACKED, int QPART = ATT_PART_QUERY, int KPART = ATT_PART_KEY>
__global__ __launch_bounds__(AS_THREADS) void k_attention_f16_stream(const _Float16* __restrict__ qkv, int T, int heads,
                                                                       int pairs, int nqb, _Float16* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) _Float16 Kb[2][AS_KC * ATT_STRIDE];
    __shared__ __attribute__((aligned(16))) _Float16 Vb[2][AS_KC * ATT_STRIDE];
    // workgroup -> (pair, query block): XCD blockIdx.x % 8 takes the pairs xcd, xcd + 8, ..., a pair's blocks in a row
    const int xcd = blockIdx.x % AS_XCDS;
    const int slot = blockIdx.x / AS_XCDS;
    const int pair = (slot / nqb) * AS_XCDS + xcd;
    if (pair >= pairs) return;  // the whole workgroup: no barrier is left behind
    const int q0 = (slot % nqb) * AS_QB;
    const int b = pair / heads;
    const int h = pair - b * heads;
    const int D = heads * 64;
    const long long row0 = (long long)b * T;
    const int tid = threadIdx.x;

    // staging: thread tid holds 16 bytes of key row tid >> 3 of the chunk and the same of the value row
    const int st = tid >> 3, sc = tid & 7;
    half8 kreg, vreg;
    auto stage_load = [&](int k0) {
        kreg = half8{0, 0, 0, 0, 0, 0, 0, 0};
        vreg = kreg;
        if (k0 + st < T) {  // rows at or past T are never read: they are staged as zeros
            kreg = *reinterpret_cast<const half8*>(att_qkv_at<PACKED>(qkv, row0 + (k0 + st), D, h, KPART, sc));
            vreg = *reinterpret_cast<const half8*>(att_qkv_at<PACKED>(qkv, row0 + (k0 + st), D, h, ATT_PART_VALUE, sc));
        }
    };
    auto stage_store = [&](int buf) {
        *reinterpret_cast<half8*>(&Kb[buf][st * ATT_STRIDE + sc * 8]) = kreg;
        *reinterpret_cast<half8*>(&Vb[buf][st * ATT_STRIDE + sc * 8]) = vreg;
    };

    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int qi = lane & 15;
    const int g = lane >> 4;
    const int tq = q0 + wave * 16 + qi;
    const bool active = q0 + wave * 16 < T;  // (wave-uniform) a wave without queries only stages
    stage_load(0);
    half8 qf[2];
    att_load_query<PACKED, QPART>(qf, qkv, row0 + min(tq, T - 1), D, h, g);
    att_scale_query(qf, qf);
    stage_store(0);
    __syncthreads();

    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int chunks = (T + AS_KC - 1) / AS_KC;
    for (int c = 0; c < chunks; ++c) {
        const int k0 = c * AS_KC;
        const bool more = c + 1 < chunks;
        if (more) stage_load(k0 + AS_KC);  // in flight under this chunk's arithmetic
        if (active) {
            const int left = T - k0;
            if (left >= AS_KC) as_chunk<false>(Kb[c & 1], Vb[c & 1], qf, left, c == 0, qi, g, m, l, o);
            else as_chunk<true>(Kb[c & 1], Vb[c & 1], qf, left, c == 0, qi, g, m, l, o);
        }
        if (!more) break;
        stage_store((c + 1) & 1);  // the buffer chunk c - 1 was read from: every wave is past that chunk's barrier
        __syncthreads();
    }
    if (!active) return;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.f / l;
    // rows behind the output and packed padding rows are not written
    if (tq < T) att_store_row(att_out_row<PACKED>(out, row0 + tq, D, h), o, inv, g);
}

}  // namespace

extern "C" int isc_attention_stream_geometry(int* query_block, int* key_chunk) {
    ISC_REQUIRE(query_block && key_chunk);
    *query_block = AS_QB;
    *key_chunk = AS_KC;
    return ISC_OK;
}

namespace {

template <int QPART, int KPART>
int attention_stream_launch(const void* qkv, int B, int T, int heads, int head_dim, void* out, int packed, void* stream) {
    ISC_REQUIRE(qkv && out && B > 0 && T > 0 && heads > 0);
    if (head_dim != 64) return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(qkv, 16) || !isc_aligned(out, 16)) return ISC_ERR_ALIGNMENT;
    if ((long long)B * T > 0x7fffffffLL || heads > 0x7fffffff / 192) return ISC_ERR_UNSUPPORTED;
    const long long pairs = (long long)B * heads;
    const int nqb = (T + AS_QB - 1) / AS_QB;
    const long long grid = (pairs + AS_XCDS - 1) / AS_XCDS * AS_XCDS * nqb;
    if (pairs > 0x7fffffffLL || grid > 0x7fffffffLL) return ISC_ERR_UNSUPPORTED;
    if (packed)
        hipLaunchKernelGGL((k_attention_f16_stream<true, QPART, KPART>), dim3((unsigned)grid), dim3(AS_THREADS), 0,
                           isc_stream(stream), reinterpret_cast<const _Float16*>(qkv), T, heads, (int)pairs, nqb,
                           reinterpret_cast<_Float16*>(out));
    else
        hipLaunchKernelGGL((k_attention_f16_stream<false, QPART, KPART>), dim3((unsigned)grid), dim3(AS_THREADS), 0,
                           isc_stream(stream), reinterpret_cast<const _Float16*>(qkv), T, heads, (int)pairs, nqb,
                           reinterpret_cast<_Float16*>(out));
    return isc_launch_status();
}

}  // namespace

extern "C" int isc_attention_f16_stream(const void* qkv, int B, int T, int heads, int head_dim, void* out, int packed,
                                        void* stream) {
    return attention_stream_launch<ATT_PART_QUERY, ATT_PART_KEY>(qkv, B, T, heads, head_dim, out, packed, stream);
}

extern "C" int isc_attention_f16_self_stream(const void* qkv, int B, int T, int heads, int head_dim, int part, void* out,
                                             int packed, void* stream) {
    if (part == ATT_PART_QUERY)
        return attention_stream_launch<ATT_PART_QUERY, ATT_PART_QUERY>(qkv, B, T, heads, head_dim, out, packed, stream);
    if (part == ATT_PART_KEY)
        return attention_stream_launch<ATT_PART_KEY, ATT_PART_KEY>(qkv, B, T, heads, head_dim, out, packed, stream);
    return ISC_ERR_INVALID_ARG;
}
