// lk_cols_check.hip -- TEST ONLY.  The vectors of lk_cols_cases.h through lift8_cols + blend7_cols and bilinear7_deriv_cols ON
// gfx950 (v_perm_b32, v_dot2_u32_u16, v_dot2_i32_i16 behind the wrappers), one thread per case, against this program's host pass
// of the same composites, of the horizontal-pair ones and of the plain formula.
//     lk_cols_check [out]    prints "OK <cases> <cases with iw11 < 0>", exit 0; a difference: the first case, exit 1; HIP error: 3
// out: the device's ColsOut records (tests/test_gpu_lk_cols.py compares them with the g++ program's).
#include "lk_cols_cases.h"

#include <stdio.h>

__global__ void cols_kernel(const ColsCase *__restrict__ cases, int n, ColsOut *__restrict__ out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n)
        return;
    ColsOut o;
    cols_new(cases[i], o);
    out[i] = o;
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
    int n_neg = 0;
    const std::vector<ColsCase> cases = cols_cases(&n_neg);
    const int n = (int)cases.size();
    std::vector<ColsOut> got((size_t)n);
    ColsCase *d_cases = nullptr;
    ColsOut *d_out = nullptr;
    CHECK(hipMalloc(&d_cases, sizeof(ColsCase) * (size_t)n));
    CHECK(hipMalloc(&d_out, sizeof(ColsOut) * (size_t)n));
    CHECK(hipMemcpy(d_cases, cases.data(), sizeof(ColsCase) * (size_t)n, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, sizeof(ColsOut) * (size_t)n));
    hipLaunchKernelGGL(cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_cases, n, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(got.data(), d_out, sizeof(ColsOut) * (size_t)n, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_cases));
    CHECK(hipFree(d_out));
    for (int i = 0; i < n; i++) {
        ColsOut host, old, plain;
        cols_new(cases[(size_t)i], host);
        cols_old(cases[(size_t)i], old);
        cols_plain(cases[(size_t)i], plain);
        const bool a = cols_same(got[(size_t)i], host), b = cols_same(got[(size_t)i], old), c = cols_same(got[(size_t)i], plain);
        if (!(a && b && c)) {
            const ColsCase &k = cases[(size_t)i];
            printf("case %d: the device differs from %s: w = %d %d %d %d, pix = %08x %08x %08x %08x, val got %08x %08x %08x %08x want %08x %08x %08x %08x\n",
                   i, !a ? "the host pass of the same composites" : !b ? "the horizontal pairs" : "the plain formula", k.w[0], k.w[1], k.w[2],
                   k.w[3], k.pix[0], k.pix[1], k.pix[2], k.pix[3], got[(size_t)i].val[0], got[(size_t)i].val[1], got[(size_t)i].val[2],
                   got[(size_t)i].val[3], plain.val[0], plain.val[1], plain.val[2], plain.val[3]);
            return 1;
        }
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (!f || fwrite(got.data(), sizeof(ColsOut), got.size(), f) != got.size() || fclose(f) != 0)
            return 2;
    }
    if (n_neg == 0) {
        printf("the grid holds no weight pair with iw11 < 0\n");
        return 4;
    }
    printf("OK %d %d\n", n, n_neg);
    return 0;
}
