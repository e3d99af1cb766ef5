// Shared host/device helpers for the gfx950 kernels behind include/imagescry_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/imagescry_hip.h"

#define ISC_WAVE 64

#define ISC_REQUIRE(cond) \
    do {                  \
        if (!(cond)) return ISC_ERR_INVALID_ARG; \
    } while (0)

static inline int isc_launch_status() { return hipGetLastError() == hipSuccess ? ISC_OK : ISC_ERR_LAUNCH; }

static inline hipStream_t isc_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline bool isc_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Compute units of the CURRENT device, cached per device id (a process may drive several GPUs; thread-safe: the slots
// are written with the same value by whoever gets there first).  256 when the query fails.
static inline int isc_device_cus() {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64) {
        const int c = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
        if (c > 0) return c;
    }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (dev >= 0 && dev < 64) __atomic_store_n(&cached[dev], cus, __ATOMIC_RELAXED);
    return cus;
}

// device-time bracket around the launch(es) of one instrumented kernel (no-ops unless isc_timing_enable(1); defined in
// capi.hip).  `kernels` = how many launches of that kernel the bracket holds: isc_timing_read reports KERNEL launches, the
// unit a rocprofv3 kernel trace counts in.
void isc_timing_begin(int kernel_id, hipStream_t stream);
void isc_timing_end(int kernel_id, hipStream_t stream, int kernels = 1);

template <typename T>
static inline T isc_ceil_div(T a, T b) {
    return (a + b - 1) / b;
}

static inline size_t isc_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ISC_ACT_QUICK_GELU, v * sigmoid(1.702 v), in the form include/imagescry_hip.h states: one product, v_exp_f32, one
// addition, a reciprocal, one product.  exp2 saturates to +inf / 0 for large |v|, where the result is -0 / v.
__device__ __forceinline__ float isc_quick_gelu(float v) {
    const float e = __builtin_amdgcn_exp2f(v * -2.4554669595930157f);  // exp(-1.702 v)
    return v * __frcp_rn(1.f + e);
}

// ISC_ACT_GELU_TANH, 0.5 v (1 + tanh(u)) with u = sqrt(2 / pi) (v + 0.044715 v^3), as v * sigmoid(2 u) in the form
// include/imagescry_hip.h states: a square, one fma, two products, v_exp_f32, one addition, a reciprocal, one product.
// v^2 overflows to +inf for |v| > 1.8e19 and exp2 saturates long before that (|v| > 11): the result is -0 or v.
__device__ __forceinline__ float isc_gelu_tanh(float v) {
    const float w = v * fmaf(v * v, 0.044715f, 1.f);                   // v + 0.044715 v^3
    const float e = __builtin_amdgcn_exp2f(w * -2.3022081851959229f);  // exp(-2 u)
    return v * __frcp_rn(1.f + e);
}

// ---- wave-level reductions (64 lanes) ---------------------------------------------------------
__device__ __forceinline__ float isc_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double isc_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long isc_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float isc_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- workgroup-level scan (256 threads) ---------------------------------------------------------
// -> the sum of v over the threads before this one (256 threads); `total` = over all.  wave_sums: 4 ints of LDS.
__device__ __forceinline__ int isc_block_exclusive_scan(int v, int* wave_sums, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    __syncthreads();  // an earlier scan's sums are consumed
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_sums[w];
        total += wave_sums[w];
    }
    return before + incl - v;
}
