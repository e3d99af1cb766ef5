// The antialiased bicubic filter of torch (_upsample_bicubic2d_aa, align_corners = False), one axis: the single statement
// of it on the device.  isc_vit_pos_resample_aa (vit_tokens.hip) and isc_resize_aa (preprocess.hip) both take their taps
// and weights from here.
#pragma once

#include <hip/hip_runtime.h>

// A separable filter whose support grows with the downscaling factor.  Per axis, g input and n output samples, s = g / n:
// centre = s (dst + 0.5), support = 2 max(s, 1), taps
// [max(0, int(centre - support + 0.5)), min(g, int(centre + support + 0.5))), weight of tap j
// cubic((j - centre + 0.5) / max(s, 1)) with A = -0.5, divided by the sum over the taps that fall inside the input.
__device__ __forceinline__ float cubic_aa(float x) {
    constexpr float A = -0.5f;
    x = fabsf(x);
    if (x < 1.f) return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    if (x < 2.f) return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
    return 0.f;
}

struct AaTaps {
    int lo, n;
    float centre, inv, total;
    __device__ __forceinline__ AaTaps(int dst, float scale, int g) {
        centre = scale * ((float)dst + 0.5f);
        const float support = 2.f * fmaxf(scale, 1.f);
        inv = 1.f / fmaxf(scale, 1.f);
        lo = max((int)(centre - support + 0.5f), 0);
        n = min((int)(centre + support + 0.5f), g) - lo;
        total = 0.f;
        for (int j = 0; j < n; ++j) total += raw(j);
    }
    __device__ __forceinline__ float raw(int j) const { return cubic_aa(((float)(j + lo) - centre + 0.5f) * inv); }
    __device__ __forceinline__ float weight(int j) const { return raw(j) / total; }
};
