// CAUSAL multi-head self-attention for short sequences (head size 64, T <= 128): isc_attention_f16_causal, the attention
// of the CLIP text tower (77 tokens).  Query i sees keys 0 .. i.  Operands, layouts and arithmetic are those of
// isc_attention_f16 (the pieces of vit_attention.h): the query scaled by 1/8 exactly, the exponent one fma feeding exp2,
// probabilities rounded to fp16 in registers as the P^T operand, values read through the transposed LDS reads.
//
// One workgroup per (sequence, head), ONE WAVE PER BLOCK OF 16 QUERIES: ceil(T / 16) waves, 5 at T = 77.  The workgroup
// stages the head's keys and values once -- rows T .. 32 ceil(T / 32) - 1 as zeros, whole MFMA k-steps of 32 -- and the
// wave of query block qb then computes key blocks 0 .. qb ONLY: blocks behind the diagonal hold nothing a query of the
// block may see.  Only the diagonal block qb is masked, element-wise, by assignment of -inf to key > query; that mask
// also covers the keys at or past T (for a query < T they are all > query).  At T = 77 the five waves compute
// 1 + 2 + 3 + 4 + 5 = 15 score blocks where the bidirectional kernel's generic form computes 5 x 14.
//
// One head per workgroup, no persistent form: a head needs 2 * 32 ceil(T / 32) * 72 * 2 bytes of LDS (27 KiB at T = 77,
// 36 KiB at 128) and five to eight waves, so five (four) workgroups share a CU and one head's staging runs under the
// others' arithmetic -- what k_attention_f16_p needs a second LDS image and sixteen waves for at 63 KiB a head.
//
// The row maximum is plain fmaxf: the hand-scheduled v_max3_f32 block of att_query_block rests on a wait-state invariant
// written for thirteen or fourteen key blocks behind one scheduling barrier, and is not copied here.
#include "vit_attention.h"

namespace {

constexpr int AC_TMAX = 128;
constexpr int AC_ROUNDS = 4;  // 16-byte chunks a thread stages per operand: ceil(32 ceil(T / 32) * 8 / (64 ceil(T / 16))) <= 4

// The query block whose NKB-th key block is the diagonal one (NKB = qb + 1).  qf: the lane's query fragments, scaled;
// tq = 16 qb + qi the lane's query (may be >= T in the last block: computed like any other, not stored).
template <int NKB>
__device__ __forceinline__ void ac_query_block(const _Float16* Ks, const _Float16* Vs, const half8 (&qf)[2], int T, int tq,
                                               int qi, int g, _Float16* orow) {
    constexpr float LOG2E = 1.4426950408889634f;
    f32x4 s[NKB + (NKB & 1)];  // odd NKB: one more block of zero probabilities, the upper half of the last P V step
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        f32x4 a = att_score_block(Ks, kb, qf, qi, g);
        if (kb == NKB - 1) {  // (compile-time) the diagonal block: keys behind the query
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kb * 16 + g * 4 + r > tq) a[r] = -INFINITY;
        }
        s[kb] = a;
        mx = fmaxf(mx, fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mxl = -mx * LOG2E;  // key 0 is never masked: every query has a finite maximum
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s[kb][r], LOG2E, mxl));  // masked keys: exp2(-inf) = 0
            s[kb][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    if constexpr (NKB & 1) s[NKB] = f32x4{0.f, 0.f, 0.f, 0.f};  // its value rows are staged (zeros past T)

    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < (NKB + 1) / 2; ++ks) att_pv_step(Vs, ks, s[2 * ks], s[2 * ks + 1], qi, g, o);
    if (tq < T) att_store_row(orow, o, inv, g);
}

template <bool PACKED>
__global__ __launch_bounds__(AC_TMAX / 16 * 64) void k_attention_f16_causal(const _Float16* __restrict__ qkv, int T, int heads,
                                                                           _Float16* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ac_lds[];
    const int trows = (T + 31) & ~31;  // key / value rows staged
    _Float16* const Ks = reinterpret_cast<_Float16*>(ac_lds);
    _Float16* const Vs = Ks + trows * ATT_STRIDE;
    const int b = blockIdx.x / heads;
    const int h = blockIdx.x - b * heads;
    const int D = heads * 64;
    const long long row0 = (long long)b * T;
    const int tid = threadIdx.x;
    const int threads = blockDim.x;  // 64 ceil(T / 16)

    // every chunk of the head is requested before the first one is waited for (AttStaged, vit.hip, has the reason)
    half8 k[AC_ROUNDS], v[AC_ROUNDS];
#pragma unroll
    for (int r = 0; r < AC_ROUNDS; ++r) {
        const int i = tid + r * threads;
        const int t = i >> 3, c = i & 7;
        k[r] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        v[r] = k[r];
        if (t < T) {  // rows T .. trows - 1 may not exist (row-major) or hold anything (packed padding): zeros
            k[r] = *reinterpret_cast<const half8*>(att_qkv_at<PACKED>(qkv, row0 + t, D, h, 1, c));
            v[r] = *reinterpret_cast<const half8*>(att_qkv_at<PACKED>(qkv, row0 + t, D, h, 2, c));
        }
    }
    const int lane = tid & 63;
    const int qb = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's query block
    const int qi = lane & 15;
    const int g = lane >> 4;
    const int tq = qb * 16 + qi;
    const long long row = row0 + min(tq, T - 1);
    half8 qf[2];
    att_load_query<PACKED>(qf, qkv, row, D, h, g);
#pragma unroll
    for (int r = 0; r < AC_ROUNDS; ++r) {
        const int i = tid + r * threads;
        const int t = i >> 3, c = i & 7;
        if (t < trows) {
            *reinterpret_cast<half8*>(&Ks[t * ATT_STRIDE + c * 8]) = k[r];
            *reinterpret_cast<half8*>(&Vs[t * ATT_STRIDE + c * 8]) = v[r];
        }
    }
    att_scale_query(qf, qf);
    __syncthreads();

    _Float16* const orow = att_out_row<PACKED>(out, row, D, h);
    switch (qb) {  // wave-uniform: EXEC stays all ones inside (att_pv_step)
        case 0: ac_query_block<1>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        case 1: ac_query_block<2>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        case 2: ac_query_block<3>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        case 3: ac_query_block<4>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        case 4: ac_query_block<5>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        case 5: ac_query_block<6>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        case 6: ac_query_block<7>(Ks, Vs, qf, T, tq, qi, g, orow); break;
        default: ac_query_block<8>(Ks, Vs, qf, T, tq, qi, g, orow); break;
    }
}

}  // namespace

extern "C" int isc_attention_f16_causal(const void* qkv, int B, int T, int heads, int head_dim, void* out, int packed,
                                        void* stream) {
    ISC_REQUIRE(qkv && out && B > 0 && T > 0 && heads > 0);
    if (head_dim != 64 || T > AC_TMAX) return ISC_ERR_UNSUPPORTED;
    if (!isc_aligned(qkv, 16) || !isc_aligned(out, 16)) return ISC_ERR_ALIGNMENT;
    if ((long long)B * heads > 0x7fffffffLL) return ISC_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(B * heads)), block((unsigned)((T + 15) / 16 * 64));
    const size_t lds = (size_t)2 * ((T + 31) & ~31) * ATT_STRIDE * sizeof(_Float16);
    if (packed)
        hipLaunchKernelGGL(k_attention_f16_causal<true>, grid, block, lds, isc_stream(stream),
                           reinterpret_cast<const _Float16*>(qkv), T, heads, reinterpret_cast<_Float16*>(out));
    else
        hipLaunchKernelGGL(k_attention_f16_causal<false>, grid, block, lds, isc_stream(stream),
                           reinterpret_cast<const _Float16*>(qkv), T, heads, reinterpret_cast<_Float16*>(out));
    return isc_launch_status();
}
