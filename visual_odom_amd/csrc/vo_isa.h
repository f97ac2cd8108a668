// vo_isa.h -- the CDNA4 instructions the kernels name directly, each wrapped ONCE: on the device the instruction (a builtin, or
// the vector expression the compiler selects it for), everywhere else its definition in plain C -- the host pass of hipcc, the
// CPU emulator of tests/host_check (VO_HOST_EMUL) and plain g++ (host_check.cpp) all compile the `#else` text.  Every user
// takes the wrappers from here (lk.hip / pyramid.hip / fast.hip through vo_lkmath.h, ingest_fmt.hip, vo_rectify.h), so the
// text the emulator suites run is the text tests/test_gpu_device_units.py compares with the instructions on gfx950, operand
// by operand (tests/host_check/unit_cases.h: LkRaw).  A wrapper is defined on the operands its comment names; the unit
// vectors stay inside them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#include <hip/hip_runtime.h>
#define VO_HD __host__ __device__ __forceinline__
#else
#define VO_HD static inline
#endif

namespace vo {

// v_perm_b32: result byte i = byte sel[i] of the 8-byte value {hi:lo} (0..3 -> lo, 4..7 -> hi), 0x0c -> 0
VO_HD uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) {
        uint32_t s = (sel >> (8 * i)) & 0xff;
        uint32_t b = s <= 7 ? (uint32_t)((v >> (8 * s)) & 0xff) : 0u; // only selectors 0..7 and 0x0c are used
        out |= b << (8 * i);
    }
    return out;
#endif
}

// v_dot2_u32_u16: a.lo*b.lo + a.hi*b.hi + c (unsigned 16-bit lanes)
VO_HD uint32_t udot2(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b), c, false);
#else
    return (a & 0xffff) * (b & 0xffff) + (a >> 16) * (b >> 16) + c;
#endif
}

// v_dot2_i32_i16: signed 16-bit lanes
VO_HD int32_t sdot2(uint32_t a, uint32_t b, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, a), __builtin_bit_cast(i16x2, b), c, false);
#else
    return (int32_t)(int16_t)(a & 0xffff) * (int16_t)(b & 0xffff) + (int32_t)(int16_t)(a >> 16) * (int16_t)(b >> 16) + c;
#endif
}

// The same dot product as the first link of an accumulation chain.  v_dot2c_i32_i16 (what the compiler picks for
// sdot2) accumulates in place, so a chain that starts from a constant or from a value that must survive costs a
// v_mov per chain; the clamped variant only exists in the three-address VOP3P form, which takes the start value
// from any operand.  No chain here gets anywhere near the int32 range, so the clamp never acts.
VO_HD int32_t sdot2_first(uint32_t a, uint32_t b, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, a), __builtin_bit_cast(i16x2, b), c, true);
#else
    return sdot2(a, b, c);
#endif
}

// v_pk_sub_i16 (wrapping) and v_pk_lshrrev_b16 by 1
VO_HD uint32_t pk_sub_i16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (i16x2)(__builtin_bit_cast(i16x2, a) - __builtin_bit_cast(i16x2, b)));
#else
    return (((a & 0xffff) - (b & 0xffff)) & 0xffff) | (((a >> 16) - (b >> 16)) << 16);
#endif
}

VO_HD uint32_t pk_lshr1_u16(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) >> (unsigned short)1));
#else
    return (a >> 1) & 0x7fff7fffu;
#endif
}

// v_dot4_u32_u8: sum of the four unsigned byte products + c
VO_HD uint32_t udot4(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    uint32_t r = c;
    for (int i = 0; i < 4; i++)
        r += ((a >> (8 * i)) & 0xff) * ((b >> (8 * i)) & 0xff);
    return r;
#endif
}

// packed 16-bit lanes, wrapping: v_pk_add_u16, v_pk_mul_lo_u16, v_pk_mad_u16 (the low 16 bits of a product or sum do
// not depend on signedness, so the same instructions serve int16 lanes)
VO_HD uint32_t pk_add_u16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
#else
    return (((a & 0xffff) + (b & 0xffff)) & 0xffff) | (((a >> 16) + (b >> 16)) << 16);
#endif
}

// v_pk_sub_u16 clamp (saturating at 0) and v_pk_min_u16
VO_HD uint32_t pk_subsat_u16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
#else
    const uint32_t al = a & 0xffff, bl = b & 0xffff, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al - bl : 0) | (ah > bh ? ah - bh : 0) << 16;
#endif
}

VO_HD uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
#else
    const uint32_t al = a & 0xffff, bl = b & 0xffff, ah = a >> 16, bh = b >> 16;
    return (al < bl ? al : bl) | (ah < bh ? ah : bh) << 16;
#endif
}

VO_HD uint32_t pk_mad_u16(uint32_t a, uint32_t k /* both lanes */, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 kk = {(unsigned short)k, (unsigned short)k};
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) * kk + __builtin_bit_cast(u16x2, c)));
#else
    return (((a & 0xffff) * k + (c & 0xffff)) & 0xffff) | ((((a >> 16) * k + (c >> 16)) & 0xffff) << 16);
#endif
}

// v_alignbyte_b32 / v_alignbit_b32: the 8-byte value {hi:lo} shifted right by `bytes` bytes, low dword
VO_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t bytes /* 0..3 */)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, bytes);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * bytes));
#endif
}

// |a - b| of the two int16 lanes (v_pk_sub_i16, v_pk_max_i16), for lanes whose difference fits int16: the residuals of the
// tracker's err epilogue, |Jp - Ip| <= 8160 (lk.hip)
VO_HD uint32_t pk_absdiff_i16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    const i16x2 d = __builtin_bit_cast(i16x2, a) - __builtin_bit_cast(i16x2, b);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(d, (i16x2)(-d)));
#else
    const int lo = (int16_t)(a & 0xffff) - (int16_t)(b & 0xffff), hi = (int16_t)(a >> 16) - (int16_t)(b >> 16);
    return (uint32_t)((lo < 0 ? -lo : lo) & 0xffff) | ((uint32_t)((hi < 0 ? -hi : hi) & 0xffff) << 16);
#endif
}

// v_cvt_i32_f32 on a VGPR: truncation towards zero, SATURATING, NaN -> 0 (vo_dev.h, vo_f2i, has what x86 does instead).  Named
// directly for a wave-uniform value that is broadcast next (lk.hip: the floors of the window corner): written as a cast the
// compiler moves the broadcast in front of the conversion and needs a second one behind it -- v_readfirstlane_b32,
// v_cvt_i32_f32 from the scalar, v_readfirstlane_b32 -- where convert + one broadcast do.
VO_HD int32_t cvt_i32_f32(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
#else
    if (v != v)
        return 0;
    if (v >= 2147483648.f)
        return 2147483647;
    if (v <= -2147483648.f)
        return -2147483647 - 1;
    return (int32_t)v;
#endif
}

// 1 / d, correctly rounded, for 2^-23 <= d < 2^29: v_rcp_f32 (1 ulp) and ONE Newton step, r + r * (1 - d * r), both halves fused.
// The compiler's own division is eleven instructions: it scales operands that need it (denormal or huge d, a denormal quotient:
// two v_div_scale_f32 and the scale inside v_div_fmas_f32), refines the reciprocal once and the quotient twice, and patches
// d = 0, +-inf, NaN (v_div_fixup_f32).  In this range nothing is scaled or patched, and on gfx950 the first step already lands on
// the correctly rounded quotient of EVERY operand: tests/host_check/rcp_check.hip compares this function with the device's
// 1.0f / d on all 52 * 2^23 floats of the range (tests/test_gpu_lk_level_setup.py; profiles/r09_lk_level_setup.md has the run,
// which the seven-instruction form -- the compiler's chain without scale and fix-up -- passes too).  Outside the range it is
// NOT the quotient: d = 0 and +-inf give NaN.
VO_HD float rcp_normal_f32(float d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.f), r, r);
#else
    return 1.f / d;
#endif
}

// (acc << 1) | (x < 0): one v_alignbit_b32 shifts a comparison's sign bit into a ring mask (a compare + select + or
// per bit cost 2.5 x as much issue time, profiles/r02_valu_issue_cost.txt; fast.hip)
VO_HD uint32_t shift_in_sign(uint32_t acc, int x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(acc, (uint32_t)x, 31);
#else
    return (acc << 1) | ((uint32_t)x >> 31);
#endif
}

} // namespace vo
