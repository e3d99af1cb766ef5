// The one copy of the bilinear source index (isc_resize_bilinear, isc_label_map).
#pragma once

#include <hip/hip_runtime.h>

// torch upsample_bilinear2d (align_corners=False): src = scale * (dst + 0.5) - 0.5, clamped at 0;
// i0 = min(int(src), in - 1); i1 = min(i0 + 1, in - 1); l1 = clamp(src - i0, 0, 1); l0 = 1 - l1.
__device__ __forceinline__ void bilinear_tap(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
    // one rounding, written out: the two-rounding form misses torch by 0.017 at 3001 -> 1000 (an ulp of 1500 in src), and which
    // of the two `scale * (dst + 0.5f) - 0.5f` compiles to is the contraction default's choice
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    i0 = min((int)src, in_size - 1);
    i1 = min(i0 + 1, in_size - 1);
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    l0 = 1.f - l1;
}
