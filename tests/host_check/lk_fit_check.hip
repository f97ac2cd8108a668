// lk_fit_check.hip -- TEST ONLY.  The vectors of lk_fit_cases.h through wave_sum2_fit_f32, wave_sum2_exact_f32 (where it applies) and
// wave_sum2_f32 ON gfx950 -- v_permlane32_swap, the DPP adds, v_cvt_f32_i32, v_readlane themselves --, one wavefront per vector,
// against (float)(int64 sum) computed here on the host.
//     lk_fit_check [out]    prints "OK <vectors> <vectors with a wrapping partial sum>", exit 0; a difference: the first vector, exit 1;
//                           HIP error: 3
// out: the device's FitOut records (tests/test_gpu_lk_fit_sums.py compares them with those of the g++ program over the emulator text).
#include <hip/hip_runtime.h>

#include "../../visual_odom_amd/csrc/vo_dev.h"

#include "lk_fit_cases.h"

#include <stdio.h>

__global__ __launch_bounds__(64) void fit_kernel(const FitCase *__restrict__ cases, int n, FitOut *__restrict__ out)
{
    const int i = (int)blockIdx.x, l = (int)threadIdx.x;
    if (i >= n)
        return;
    const FitCase &c = cases[i];
    const int a = c.a[l], b = c.b[l];
    const bool both = __builtin_amdgcn_readfirstlane(c.exact_ok) != 0;
    float f0, f1, e0 = 0.f, e1 = 0.f, g0, g1, h0 = 0.f, h1 = 0.f;
    vo::wave_sum2_fit_f32(a, b, f0, f1);
    vo::wave_sum2_f32(a, b, true, g0, g1);
    if (both) { // (wave-uniform)
        vo::wave_sum2_exact_f32(a, b, e0, e1);
        vo::wave_sum2_f32(a, b, false, h0, h1);
    }
    if (l == 0) {
        FitOut o;
        o.v[0] = __float_as_uint(f0);
        o.v[1] = __float_as_uint(f1);
        // (the two forms of the split sums are ONE record: they have to agree, and a difference shows as neither matching the host)
        o.v[2] = both ? (__float_as_uint(e0) == __float_as_uint(h0) ? __float_as_uint(e0) : 0xffffffffu) : 0u;
        o.v[3] = both ? (__float_as_uint(e1) == __float_as_uint(h1) ? __float_as_uint(e1) : 0xffffffffu) : 0u;
        o.v[4] = __float_as_uint(g0);
        o.v[5] = __float_as_uint(g1);
        out[i] = o;
    }
}

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        const hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                                   \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                                        \
            return 3;                                                                             \
        }                                                                                         \
    } while (0)

int main(int argc, char **argv)
{
    const std::vector<FitCase> cases = fit_cases();
    const int n = (int)cases.size();
    std::vector<FitOut> got((size_t)n);
    FitCase *d_cases = nullptr;
    FitOut *d_out = nullptr;
    CHECK(hipMalloc(&d_cases, sizeof(FitCase) * (size_t)n));
    CHECK(hipMalloc(&d_out, sizeof(FitOut) * (size_t)n));
    CHECK(hipMemcpy(d_cases, cases.data(), sizeof(FitCase) * (size_t)n, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, sizeof(FitOut) * (size_t)n));
    hipLaunchKernelGGL(fit_kernel, dim3((unsigned)n), dim3(64), 0, 0, d_cases, n, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(got.data(), d_out, sizeof(FitOut) * (size_t)n, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_cases));
    CHECK(hipFree(d_out));
    int n_wrap = 0;
    for (int i = 0; i < n; i++) {
        const FitCase &c = cases[(size_t)i];
        const uint32_t wa = fit_want_bits(c.a), wb = fit_want_bits(c.b);
        const FitOut &o = got[(size_t)i];
        const bool ok = o.v[0] == wa && o.v[1] == wb && o.v[4] == wa && o.v[5] == wb && o.v[2] == (c.exact_ok ? wa : 0u) && o.v[3] == (c.exact_ok ? wb : 0u);
        if (!ok) {
            printf("vector %d (exact_ok %d, wraps %d): totals %lld %lld want %08x %08x, the device: fit %08x %08x, split %08x %08x, wave_sum2_f32 %08x %08x\n",
                   i, c.exact_ok, c.wraps, (long long)fit_total(c.a), (long long)fit_total(c.b), wa, wb, o.v[0], o.v[1], o.v[2], o.v[3], o.v[4], o.v[5]);
            return 1;
        }
        n_wrap += c.wraps;
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (!f || fwrite(got.data(), sizeof(FitOut), got.size(), f) != got.size() || fclose(f) != 0)
            return 2;
    }
    printf("OK %d %d\n", n, n_wrap);
    return 0;
}
