// rcp_host.cpp -- TEST ONLY.  1.0f / x of the RCP_SAMPLES operands of rcp_cases.h as g++ computes it (IEEE division), written as
// raw bits: what tests/test_gpu_lk_level_setup.py compares the device's quotients with.
//     rcp_host out     prints "OK <samples>", exit 0
#include "rcp_cases.h"

#include <stdio.h>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    std::vector<uint32_t> q(RCP_SAMPLES);
    for (uint32_t i = 0; i < RCP_SAMPLES; i++) {
        volatile float x = rcp_operand(RCP_LO + i * RCP_STEP);
        q[i] = rcp_bits(1.0f / x);
    }
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(q.data(), 4, q.size(), f) != q.size() || fclose(f) != 0)
        return 2;
    printf("OK %u\n", RCP_SAMPLES);
    return 0;
}
