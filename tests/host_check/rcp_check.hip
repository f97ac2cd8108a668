// rcp_check.hip -- TEST ONLY.  rcp_normal_f32 (vo_isa.h: the reciprocal of the LK solve's determinant) ON gfx950 against the
// device's IEEE 1.0f / x, on EVERY float of the exponents 2^-23 .. 2^28 (rcp_cases.h: 52 * 2^23 operands, a fraction of a second).
//     rcp_check [out]   prints "OK <operands> 0", exit 0; differences: "MISMATCH <count> first x = <bits> got <bits> want <bits>",
//                       exit 1; HIP error: 3
// out: the device's 1.0f / x of the RCP_SAMPLES evenly spaced operands, raw bits (compared with rcp_host.cpp's by the test).
#include "rcp_cases.h"

#include "../../visual_odom_amd/csrc/vo_isa.h"

#include <stdio.h>
#include <vector>

#ifndef RCP_UNDER_TEST
#define RCP_UNDER_TEST(x) vo::rcp_normal_f32(x)
#endif

// thread t takes operands t, t + threads, ...: every operand exactly once, all of them inside [RCP_LO, RCP_LO + RCP_COUNT)
__global__ void rcp_all_kernel(unsigned long long *__restrict__ n_bad, unsigned int *__restrict__ first_bad)
{
    const uint32_t threads = gridDim.x * blockDim.x;
    uint32_t bad = 0, first = 0xffffffffu;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < RCP_COUNT; i += threads) {
        const float x = __uint_as_float(RCP_LO + i);
        const float got = RCP_UNDER_TEST(x), want = 1.0f / x;
        if (__float_as_uint(got) != __float_as_uint(want)) {
            bad++;
            first = first < RCP_LO + i ? first : RCP_LO + i;
        }
    }
    if (bad) {
        atomicAdd(n_bad, (unsigned long long)bad);
        atomicMin(first_bad, first);
    }
}

__global__ void rcp_samples_kernel(uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < RCP_SAMPLES)
        out[i] = __float_as_uint(1.0f / __uint_as_float(RCP_LO + i * RCP_STEP));
}

__global__ void rcp_one_kernel(uint32_t bits, uint32_t *__restrict__ out)
{
    const float x = __uint_as_float(bits);
    out[0] = __float_as_uint(RCP_UNDER_TEST(x));
    out[1] = __float_as_uint(1.0f / x);
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
    unsigned long long *d_bad = nullptr, n_bad = 0;
    unsigned int *d_first = nullptr, first = 0xffffffffu;
    uint32_t *d_out = nullptr;
    std::vector<uint32_t> q(RCP_SAMPLES);
    CHECK(hipMalloc(&d_bad, sizeof(n_bad)));
    CHECK(hipMalloc(&d_first, sizeof(first)));
    CHECK(hipMalloc(&d_out, 4 * (size_t)RCP_SAMPLES));
    CHECK(hipMemcpy(d_bad, &n_bad, sizeof(n_bad), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_first, &first, sizeof(first), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rcp_all_kernel, dim3(4096), dim3(256), 0, 0, d_bad, d_first);
    CHECK(hipGetLastError());
    hipLaunchKernelGGL(rcp_samples_kernel, dim3(RCP_SAMPLES / 256), dim3(256), 0, 0, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&n_bad, d_bad, sizeof(n_bad), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&first, d_first, sizeof(first), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(q.data(), d_out, 4 * (size_t)RCP_SAMPLES, hipMemcpyDeviceToHost));
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (!f || fwrite(q.data(), 4, q.size(), f) != q.size() || fclose(f) != 0)
            return 2;
    }
    if (n_bad != 0) {
        uint32_t two[2] = {0, 0};
        hipLaunchKernelGGL(rcp_one_kernel, dim3(1), dim3(1), 0, 0, first, d_out);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(two, d_out, sizeof(two), hipMemcpyDeviceToHost));
        printf("MISMATCH %llu first x = %08x got %08x want %08x\n", n_bad, first, two[0], two[1]);
        return 1;
    }
    CHECK(hipFree(d_bad));
    CHECK(hipFree(d_first));
    CHECK(hipFree(d_out));
    printf("OK %u 0\n", RCP_COUNT);
    return 0;
}
