// Stand-alone host program for a sanitizer run of the host side of csrc/bank_farthest.hip: workspace sizing and carving and
// every argument check of isc_bank_farthest.  No call below reaches a launch.  Build and run on a CPU:
//   hipcc -std=c++17 -O1 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/sanitize/farthest_host_main.cpp imagescry_amd/csrc/bank_farthest.hip imagescry_amd/csrc/bank_pack.hip \
//         -o farthest_host_check
//   ./farthest_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/imagescry_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                           \
    do {                                                                             \
        const int got_ = (call);                                                     \
        if (got_ != (want)) {                                                        \
            printf("line %d: %s = %d, expected %d\n", __LINE__, #call, got_, (want)); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

int main() {
    size_t need = 0, prev = 0;
    const int64_t ns[] = {0, 1, 255, 256, 257, 100000, 10000000, 0x7ffffffe};
    const int ds[] = {1, 31, 32, 33, 768, ISC_SEARCH_MAX_D};
    for (int dtype = ISC_F16; dtype <= ISC_F32; ++dtype)
        for (int d : ds) {
            prev = 0;
            for (int64_t n : ns) {
                EXPECT(isc_bank_farthest_workspace_bytes(dtype, n, d, &need), ISC_OK);
                if (need == 0 || need < prev) {
                    printf("workspace not positive and monotone in N: dtype %d d %d n %lld\n", dtype, d, (long long)n);
                    ++failures;
                }
                prev = need;
            }
        }
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_F16, 1000, ISC_SEARCH_MAX_D + 1, &need), ISC_ERR_UNSUPPORTED);
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_U8, 1000, 64, &need), ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_F16, -1, 64, &need), ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_F16, 0x7fffffff, 64, &need), ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_F16, 1000, 0, &need), ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_F16, 1000, 64, nullptr), ISC_ERR_INVALID_ARG);

    // argument checks: host buffers stand in for device memory, none is dereferenced
    void* buf = aligned_alloc(256, 4096);
    char* odd = static_cast<char*>(buf) + 2;
    int64_t* i64 = static_cast<int64_t*>(buf);
    float* f32 = static_cast<float*>(buf);
    uint32_t* u32 = static_cast<uint32_t*>(buf);
    EXPECT(isc_bank_farthest_workspace_bytes(ISC_F16, 1000, 64, &need), ISC_OK);
    auto call = [&](const void* bank, int dtype, int64_t n, int d, const int64_t* start, int64_t s, int64_t m,
                    const uint32_t* fill, const uint32_t* mask, int64_t* rows, float* cover, float* near, void* ws,
                    size_t wsb) {
        return isc_bank_farthest(bank, dtype, n, d, start, s, m, fill, mask, rows, cover, near, ws, wsb, nullptr);
    };
    EXPECT(call(nullptr, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 64, nullptr, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, nullptr, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, nullptr, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, f32, f32, nullptr, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_U8, 1000, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, -1, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 0, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 0x7fffffff, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 0, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, -1, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, -1, u32, u32, i64, f32, f32, buf, need), ISC_ERR_INVALID_ARG);
    EXPECT(call(buf, ISC_F16, 1000, ISC_SEARCH_MAX_D + 1, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_UNSUPPORTED);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, ISC_FARTHEST_MAX_PICKS + 1, u32, u32, i64, f32, f32, buf, need),
           ISC_ERR_UNSUPPORTED);
    EXPECT(call(odd, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, reinterpret_cast<int64_t*>(odd + 2), 2, 8, u32, u32, i64, f32, f32, buf, need),
           ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, reinterpret_cast<uint32_t*>(odd), u32, i64, f32, f32, buf, need),
           ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, reinterpret_cast<uint32_t*>(odd), i64, f32, f32, buf, need),
           ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, reinterpret_cast<int64_t*>(odd + 2), f32, f32, buf, need),
           ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, reinterpret_cast<float*>(odd), f32, buf, need),
           ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, f32, reinterpret_cast<float*>(odd), buf, need),
           ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, f32, f32, odd + 14, need), ISC_ERR_ALIGNMENT);
    EXPECT(call(buf, ISC_F16, 1000, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need - 1), ISC_ERR_WORKSPACE);
    EXPECT(call(buf, ISC_F16, 100000, 64, i64, 2, 8, u32, u32, i64, f32, f32, buf, need), ISC_ERR_WORKSPACE);
    EXPECT(call(nullptr, ISC_F16, 1000, 64, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ISC_OK);
    EXPECT(call(nullptr, ISC_F16, 0, 64, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ISC_OK);
    free(buf);
    printf(failures ? "farthest host checks: %d FAILED\n" : "farthest host checks: ok\n", failures);
    return failures ? 1 : 0;
}
