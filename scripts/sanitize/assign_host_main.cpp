// Stand-alone host program for a sanitizer run of the host side of csrc/bank_assign.hip: workspace sizing and carving and
// every argument check of the assign / group-sums entry points.  No call below reaches a launch.  Build and run on a CPU:
//   hipcc -std=c++17 -O1 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/sanitize/assign_host_main.cpp imagescry_amd/csrc/bank_assign.hip imagescry_amd/csrc/bank_pack.hip \
//         -o assign_host_check
//   ./assign_host_check
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
    const int cs[] = {0, 1, 16, 17, 64, 65, 1023, 1024, 1025, 1 << 24};
    const int ds[] = {1, 31, 32, 33, 768, ISC_SEARCH_MAX_D};
    for (int dtype = ISC_F16; dtype <= ISC_F32; ++dtype)
        for (int d : ds)
            for (int c : cs) {
                prev = 0;
                for (int64_t n : ns) {
                    EXPECT(isc_bank_assign_workspace_bytes(dtype, n, d, c, &need), ISC_OK);
                    if (need < prev) {
                        printf("workspace not monotone in N: dtype %d d %d c %d n %lld\n", dtype, d, c, (long long)n);
                        ++failures;
                    }
                    prev = need;
                }
            }
    size_t a = 0, b = 0;
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, 1000000, 768, 1024, &a), ISC_OK);
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, 1000000, 768, 1 << 24, &b), ISC_OK);
    if (a != b) ++failures;
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, 1000, ISC_SEARCH_MAX_D + 1, 4, &need), ISC_ERR_UNSUPPORTED);
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, 1000, 64, (1 << 24) + 1, &need), ISC_ERR_UNSUPPORTED);
    EXPECT(isc_bank_assign_workspace_bytes(ISC_U8, 1000, 64, 4, &need), ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, -1, 64, 4, &need), ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, 1000, 64, 4, nullptr), ISC_ERR_INVALID_ARG);
    for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)1024, (int64_t)1025, (int64_t)0x7ffffffe})
        for (int d : ds) EXPECT(isc_bank_group_sums_workspace_bytes(ISC_F32, m, d, &need), ISC_OK);
    EXPECT(isc_bank_group_sums_workspace_bytes(ISC_F32, 10, ISC_SEARCH_MAX_D + 1, &need), ISC_ERR_UNSUPPORTED);
    EXPECT(isc_bank_group_sums_workspace_bytes(ISC_F32, -1, 8, &need), ISC_ERR_INVALID_ARG);

    // argument checks: host buffers stand in for device memory, none is dereferenced
    void* buf = aligned_alloc(256, 4096);
    char* odd = static_cast<char*>(buf) + 2;
    EXPECT(isc_bank_assign_workspace_bytes(ISC_F16, 1000, 64, 8, &need), ISC_OK);
    int32_t* i32 = static_cast<int32_t*>(buf);
    float* f32 = static_cast<float*>(buf);
    for (int ex = 0; ex < 2; ++ex) {
        auto call = [&](const void* bank, int dtype, int64_t n, int d, const void* cent, int cd, int c, int64_t ldc,
                        const uint32_t* mask, int32_t* labels, float* scores, int32_t* status, void* ws, size_t wsb) {
            return ex ? isc_bank_assign_exhaustive(bank, dtype, n, d, cent, cd, c, ldc, mask, labels, scores, status, ws, wsb,
                                                   nullptr)
                      : isc_bank_assign(bank, dtype, n, d, cent, cd, c, ldc, f32, mask, labels, scores, status, ws, wsb,
                                        nullptr);
        };
        EXPECT(call(nullptr, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, 64, nullptr, ISC_F32, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, nullptr, nullptr, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, nullptr, i32, f32, nullptr, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_U8, 1000, 64, buf, ISC_F32, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, 64, buf, ISC_U8, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 63, nullptr, i32, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, 0, buf, ISC_F32, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_INVALID_ARG);
        EXPECT(call(buf, ISC_F16, 1000, ISC_SEARCH_MAX_D + 1, buf, ISC_F32, 8, 10000, nullptr, i32, f32, i32, buf, need),
               ISC_ERR_UNSUPPORTED);
        EXPECT(call(odd, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_ALIGNMENT);
        EXPECT(call(buf, ISC_F16, 1000, 64, odd, ISC_F32, 8, 64, nullptr, i32, f32, i32, buf, need), ISC_ERR_ALIGNMENT);
        EXPECT(call(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, reinterpret_cast<uint32_t*>(odd), i32, f32, i32, buf, need),
               ISC_ERR_ALIGNMENT);
        EXPECT(call(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, nullptr, reinterpret_cast<int32_t*>(odd), f32, i32, buf, need),
               ISC_ERR_ALIGNMENT);
        EXPECT(call(nullptr, ISC_F16, 1000, 64, nullptr, ISC_F32, 0, 64, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ISC_OK);
        EXPECT(call(nullptr, ISC_F16, 0, 64, nullptr, ISC_F32, 8, 64, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ISC_OK);
    }
    EXPECT(isc_bank_assign(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, f32, nullptr, i32, f32, i32, nullptr, need, nullptr),
           ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_assign(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, f32, nullptr, i32, f32, i32, odd + 14, need, nullptr),
           ISC_ERR_ALIGNMENT);
    EXPECT(isc_bank_assign(buf, ISC_F16, 1000, 64, buf, ISC_F32, 8, 64, f32, nullptr, i32, f32, i32, buf, need - 1, nullptr),
           ISC_ERR_WORKSPACE);
    EXPECT(isc_bank_assign(buf, ISC_F16, 1000, 64, buf, ISC_F32, 1024, 64, f32, nullptr, i32, f32, i32, buf, need, nullptr),
           ISC_ERR_WORKSPACE);

    int64_t* i64 = static_cast<int64_t*>(buf);
    double* f64 = static_cast<double*>(buf);
    EXPECT(isc_bank_group_sums_workspace_bytes(ISC_F16, 500, 64, &need), ISC_OK);
    EXPECT(isc_bank_group_sums(nullptr, ISC_F16, 1000, 64, i64, 500, i64, 4, nullptr, f64, 64, i64, buf, need, nullptr),
           ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_group_sums(buf, ISC_F16, 1000, 64, nullptr, 500, i64, 4, nullptr, f64, 64, i64, buf, need, nullptr),
           ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_group_sums(buf, ISC_F16, 0, 64, i64, 500, i64, 4, nullptr, f64, 64, i64, buf, need, nullptr),
           ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_group_sums(buf, ISC_F16, 1000, 64, i64, 500, i64, 4, nullptr, f64, 63, i64, buf, need, nullptr),
           ISC_ERR_INVALID_ARG);
    EXPECT(isc_bank_group_sums(buf, ISC_F16, 1000, 64, reinterpret_cast<int64_t*>(odd + 2), 500, i64, 4, nullptr, f64, 64,
                               i64, buf, need, nullptr),
           ISC_ERR_ALIGNMENT);
    EXPECT(isc_bank_group_sums(buf, ISC_F16, 1000, 64, i64, 500, i64, 4, nullptr, f64, 64, i64, buf, need - 1, nullptr),
           ISC_ERR_WORKSPACE);
    EXPECT(isc_bank_group_sums(buf, ISC_F16, 1000, 64, i64, 500, i64, (int64_t)1 << 31, nullptr, f64, 64, i64, buf, need,
                               nullptr),
           ISC_ERR_UNSUPPORTED);
    EXPECT(isc_bank_group_sums(nullptr, ISC_F16, 1000, 64, nullptr, 500, nullptr, 0, nullptr, nullptr, 64, nullptr, nullptr, 0,
                               nullptr),
           ISC_OK);
    free(buf);
    printf(failures ? "assign host checks: %d FAILED\n" : "assign host checks: ok\n", failures);
    return failures ? 1 : 0;
}
