// rcp_cases.h -- TEST ONLY.  The operands of the reciprocal checks (rcp_check.hip on gfx950, rcp_host.cpp with g++): every float
// of the exponents 2^-23 .. 2^28 -- the determinant of the LK solve lies in [FLT_EPSILON, 2^29), lk.hip -- and 2^20 evenly spaced
// ones of them whose quotients both programs write.
#pragma once

#include <stdint.h>
#include <string.h>

constexpr uint32_t RCP_LO = 0x34000000u;                // 2^-23 = FLT_EPSILON / 2 ... the range starts one exponent below
constexpr uint32_t RCP_EXPONENTS = 52;                  // 2^-23 .. 2^28, the last one included
constexpr uint32_t RCP_COUNT = RCP_EXPONENTS << 23;     // 52 * 2^23 operands; RCP_LO + RCP_COUNT = 0x4e000000 = 2^29
constexpr uint32_t RCP_SAMPLES = 1u << 20, RCP_STEP = RCP_COUNT / RCP_SAMPLES;
static_assert(RCP_LO + RCP_COUNT == 0x4e000000u && RCP_STEP * RCP_SAMPLES == RCP_COUNT, "the range ends below 2^29, the samples divide it");

static inline float rcp_operand(uint32_t bits)
{
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static inline uint32_t rcp_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
