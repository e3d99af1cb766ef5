// Stand-alone host check (no GPU, not loaded into Python): a straight-line form of isc_i8_threshold (cosine_topk.hip) -- clamp,
// one floor + convert, selects for the saturation and special cases -- returns the same int as the branching form the
// kernels use, for every input.  The straight-line form is NOT in the kernels: it cost the int8 filter 256 VGPRs and 12 B of
// scratch (LABLOG.md section 8); both forms stand side by side here so that the equality can be retaken.  README.md: the build.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include <cmath>

// ---- the straight-line form.  +-2e9 are floats and inside int32; fmaxf drops a NaN, which the !(lo <= 2e9) select answers.
static float isc_i8_threshold_bound(float thr_cq, float ct, float et, float nt, float qn, float eq) {
    const float t = thr_cq * ct;
    const float mg = fmaf(qn, et, eq * (nt + et));
    return (t - mg) - (fabsf(t) + mg) * 9.5367431640625e-7f - 1e-30f;
}
static int isc_i8_threshold_int(float lo, float thr_cq, float nt) {
    const float cl = fminf(fmaxf(lo, -2.0e9f), 2.0e9f);
    int r = (int)floorf(cl);
    r = lo < -2.0e9f ? INT32_MIN : r;
    r = !(lo <= 2.0e9f) ? INT32_MAX : r;
    const int tile_special = thr_cq < INFINITY ? INT32_MIN : INT32_MAX;
    return nt < INFINITY ? r : tile_special;
}
static int isc_i8_threshold(float thr_cq, float ct, float et, float nt, float qn, float eq) {
    return isc_i8_threshold_int(isc_i8_threshold_bound(thr_cq, ct, et, nt, qn, eq), thr_cq, nt);
}

// ---- the reference: the form of cosine_topk.hip (isc_i8_threshold there), verbatim
static int old_int(float lo, float thr_cq, float nt) {
    int r = !(lo <= 2.0e9f) ? INT32_MAX : lo < -2.0e9f ? INT32_MIN : (int)floorf(lo);
    if (!(nt < INFINITY)) r = thr_cq < INFINITY ? INT32_MIN : INT32_MAX;
    return r;
}
static int old_threshold(float thr_cq, float ct, float et, float nt, float qn, float eq) {
    const float t = thr_cq * ct;
    const float mg = fmaf(qn, et, eq * (nt + et));
    const float lo = (t - mg) - (fabsf(t) + mg) * 9.5367431640625e-7f - 1e-30f;
    return old_int(lo, thr_cq, nt);
}

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static long long failures = 0, checked = 0;
static void check_int(float lo, float thr_cq, float nt) {
    const int a = old_int(lo, thr_cq, nt), b = isc_i8_threshold_int(lo, thr_cq, nt);
    ++checked;
    if (a != b && failures++ < 20)
        std::printf("MISMATCH int: lo=%a (0x%08x) thr_cq=%a nt=%a old=%d new=%d\n", lo, bits_of(lo), thr_cq, nt, a, b);
}
static void check_full(float thr_cq, float ct, float et, float nt, float qn, float eq) {
    const int a = old_threshold(thr_cq, ct, et, nt, qn, eq), b = isc_i8_threshold(thr_cq, ct, et, nt, qn, eq);
    ++checked;
    if (a != b && failures++ < 20)
        std::printf("MISMATCH: thr_cq=%a ct=%a et=%a nt=%a qn=%a eq=%a old=%d new=%d\n", thr_cq, ct, et, nt, qn, eq, a, b);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // the special values and their neighbours (one and two ulps either side)
    std::vector<float> special;
    const float seeds[] = {0.f, -0.f, inf, -inf, nan, -nan, 1.4e-45f, -1.4e-45f, 1.17549435e-38f, -1.17549435e-38f,
                           5.87e-39f, -5.87e-39f, 2.0e9f, -2.0e9f, 2147483648.f, -2147483648.f, 4294967296.f, 1.f, -1.f,
                           0.5f, -0.5f, 1e-30f, -1e-30f, 16129.f * 768.f, -16129.f * 768.f, 3.4028235e38f, -3.4028235e38f,
                           8388608.f, -8388608.f, 16777216.f, -16777216.f, 123.5f, -123.5f, 7.f, -7.f};
    for (float s : seeds) {
        special.push_back(s);
        const uint32_t u = bits_of(s);
        for (int dlt = -2; dlt <= 2; ++dlt)
            if (dlt != 0) special.push_back(from_bits(u + (uint32_t)dlt));
    }
    const float nts[] = {0.f, 1.f, 1000.f, 3.4028235e38f, inf, nan, -inf};
    const float thrs[] = {0.f, -0.f, 1.f, -1.f, 127.f, inf, -inf, nan, 3.4028235e38f, -3.4028235e38f};

    // 1. bound -> int over the special bounds, every tile / threshold class
    for (float lo : special)
        for (float nt : nts)
            for (float th : thrs) check_int(lo, th, nt);
    // ... every float bit pattern of the exponents around the saturation points and around zero, and a stride over all
    for (uint32_t u = bits_of(1.9e9f); u <= bits_of(2.2e9f); ++u) {
        check_int(from_bits(u), 1.f, 1.f);
        check_int(from_bits(u | 0x80000000u), 1.f, 1.f);
    }
    for (uint64_t u = 0; u <= 0xffffffffull; u += 997) check_int(from_bits((uint32_t)u), 1.f, 1.f);

    // 2. the whole function: special values in every argument (thr_cq, ct, nt swept fully; the others over a subset)
    const float small[] = {0.f, -0.f, 1.4e-45f, 1e-3f, 1.f, 127.f, 2.0e9f, 3.4028235e38f, inf, nan};
    for (float th : special)
        for (float ct : special)
            for (float nt : nts)
                for (float et : small)
                    for (float qn : {0.f, 1.f, 1407.f, inf})
                        for (float eq : {0.f, 0.29f, inf, nan}) check_full(th, ct, et, nt, qn, eq);

    // 3. a few million random inputs: the ranges of real searches, then raw bit patterns
    std::mt19937 gen(12345);
    std::uniform_real_distribution<float> thr_d(-1.2f, 1.2f), cq_d(1.f, 4000.f), ct_d(1.f, 40000.f), et_d(0.f, 8.f),
        nt_d(0.f, 1500.f), qn_d(0.f, 1500.f), eq_d(0.f, 8.f);
    for (int i = 0; i < 4000000; ++i)
        check_full(thr_d(gen) * cq_d(gen), ct_d(gen), et_d(gen), nt_d(gen), qn_d(gen), eq_d(gen));
    for (int i = 0; i < 4000000; ++i)
        check_full(from_bits(gen()), from_bits(gen()), from_bits(gen()), from_bits(gen()), from_bits(gen()),
                   from_bits(gen()));

    std::printf("%lld inputs checked, %lld mismatches\n", checked, failures);
    return failures ? 1 : 0;
}
