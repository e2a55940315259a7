/*
 * rt_vec.h — the device code's vector and short-form math helpers: the 16-byte load type, V3 and its operators, 1 / x and sqrt(x) in their
 * short forms, normalised(), the Box-Muller draw and the SGPR-mask select.  Used by every kernel that traces a ray.
 *
 * The arithmetic (types, order, the double-precision fragments) is the reference's; file:line
 * citations are on each piece.  -ffp-contract=off is assumed (see rt_kernel.hip).
 */
#ifndef RT_VEC_H
#define RT_VEC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_math.h"
#include "rt_rng.h"

#define RT_WAVE 64

/* 16-byte vector for LDS / global accesses: a single ds_read_b128 / global_load_dwordx4 each
 * (a struct of four floats gets split into narrower loads by the optimiser) */
typedef float v4f __attribute__((ext_vector_type(4)));

/* ---- 1 / x and sqrt(x), correctly rounded, in a third of the instructions (round 4) ---------------------------------
 * The compiler expands `1.0f / x` into 11 instructions (v_div_scale x 2, v_rcp, five fma, v_div_fmas, v_div_fixup) and sqrtf
 * into 17 + 5 s_nop, most of it for inputs a renderer never sees: denormals, results that underflow, zero, infinity.  On gfx950
 *   v_rcp_f32 + one Newton step (two fma)                is 1.0f / x bit for bit for every x with 2^-126 <= |x| <= 2^126,
 *   v_rsq_f32 + two multiplies + one residual step (2 fma) is sqrtf(x) bit for bit for every x with 2^-64 <= x < inf,
 * checked EXHAUSTIVELY - all 2^32 inputs against the compiler's expansions on the device, tests/test_gpu_math.py
 * (tools/ubench/exact_div_sqrt.hip, profiles/r04/experiments/exact_div_sqrt.txt: outside those ranges every single input fails,
 * inside none).  rt_sqrt / rt_rcp_sqrt take the short forms when EVERY active lane's operand is inside the range (one subtract,
 * one compare, a wave-uniform branch) and the compiler's otherwise: the value is the IEEE one for every input, always.  Used
 * where it pays: the normalisations (1 / sqrt: 41 -> 24 instructions), the sphere test's and Box-Muller's roots; same-box A/B:
 * three-sphere -8 %, cube -3.6 %, reference scene 0 -0.9 %, monkey -0.3 % (profiles/r04/experiments/exact_div_sqrt_ab.txt). */
__device__ __forceinline__ bool rt_rcp_in_range(float x) { return ((__float_as_uint(x) & 0x7fffffffu) - 0x00800000u) <= 0x7e000000u; }
__device__ __forceinline__ bool rt_sqrt_in_range(float x) { return (__float_as_uint(x) - 0x1f800000u) < 0x60000000u; }
__device__ __forceinline__ float rt_rcp_short(float x)
{
    const float y = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(y, __builtin_fmaf(-x, y, 1.0f), y);
}
/* sqrtf(x) for x in the range above, from the reciprocal square root: s0 = x * rsq(x) is the root to ~2 ulp, and one step
 * s0 + (x - s0^2) * (rsq / 2) with the residual as an fma lands on the correctly rounded value for EVERY binary32 from 2^-102 up
 * (tools/ubench/rsq_forms.hip on the device; tests/test_gpu_math.py's exhaustive test runs this very function against sqrtf over
 * all 2^32 patterns).  Five instructions - v_rsq_f32, two multiplies, two fma - where round 4's first form (v_sqrt_f32, then a
 * residual test of the neighbours one ulp down and up) took nine, four of them compares and selects
 * (profiles/r04/experiments/sqrt_from_rsq.txt). */
__device__ __forceinline__ float rt_sqrt_short(float x)
{
    const float y = __builtin_amdgcn_rsqf(x);
    const float s0 = x * y, h = 0.5f * y;
    return __builtin_fmaf(__builtin_fmaf(-s0, s0, x), h, s0);
}
__device__ __forceinline__ float rt_sqrt(float x)       /* == sqrtf(x) */
{
    if (__ballot(!rt_sqrt_in_range(x)) == 0ull) return rt_sqrt_short(x);
    return sqrtf(x);
}
/* 1.0f / sqrtf(m): sqrt of an in-range m lies in [2^-32, 2^64], inside the reciprocal's range - one check for both */
__device__ __forceinline__ float rt_rcp_sqrt(float m)
{
    if (__ballot(!rt_sqrt_in_range(m)) == 0ull) return rt_rcp_short(rt_sqrt_short(m));
    return 1.0f / sqrtf(m);
}

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
/* src/utils.cu:130-136: (x*x' + y*y') + z*z' */
__device__ __forceinline__ float dot(V3 a, V3 b) { float nx = a.x * b.x, ny = a.y * b.y, nz = a.z * b.z; return nx + ny + nz; }
/* src/utils.cu:146-153 */
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
/* src/utils.cu:118-128: one reciprocal of the magnitude, three multiplies */
__device__ __forceinline__ V3 normalised(V3 a)
{
    float m = a.x * a.x + a.y * a.y + a.z * a.z;
    float inv = rt_rcp_sqrt(m);
    return v3(a.x * inv, a.y * inv, a.z * inv);
}
__device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }

/* src/utils.cu:234-239 — Box-Muller cosine branch, theta drawn first.  rt_rng.h produces the
 * reference's (float)(r / 4294967295.0) and the binary64 products derived from it without the
 * binary64 divide, bit for bit (tests/test_rng_exhaustive.py covers all 2^32 inputs). */
template <bool SHORT_DIVIDE, bool GENERAL_FUNCTIONS>
__device__ __forceinline__ float normal_num(uint32_t &state)
{
    float theta = rt_theta(rt_pcg_next(&state));
    if (GENERAL_FUNCTIONS) {         /* (the hybrid kernels: see px_shade) */
        float rho_g = rt_sqrt(-2.0f * rt_logf(rt_u01(rt_pcg_next(&state))));
        return rho_g * rt_cosf(theta);
    }
    /* log on [0, 1] and cos on [0, 6.28318]: rt_logf / rt_cosf without the cases these arguments cannot be (rt_math.h; the
     * general-purpose pair everywhere was measured against it: profiles/r04/experiments/box_muller_on_its_domain.txt) */
    float rho = rt_sqrt(-2.0f * rt_logf_0_1(rt_u01(rt_pcg_next(&state)), SHORT_DIVIDE ? 1 : 0));
    return rho * rt_cosf_0_2pi(theta);
}

/* c ? a : b as a v_cndmask_b32 in its VOP3 form (mask from an SGPR pair).  The compiler prefers the VOP2 form, which reads
 * the mask from VCC - and two of THOSE back to back cost the issuing wave 16 cycles each instead of 4 on gfx950
 * (tools/ubench/valu_tput.hip K_CNDMASK / K_CC2 against K_CNDMASK_S / K_CC2S; profiles/r04/experiments/valu_tput.txt).
 * Used where the traversal loops select two values on one condition. */
__device__ __forceinline__ uint32_t rt_sel_u32(unsigned long long lanes, uint32_t a, uint32_t b)       /* lanes = __ballot(condition) */
{
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(lanes));
    return r;
}
__device__ __forceinline__ float rt_sel_f32(unsigned long long lanes, float a, float b) { return __uint_as_float(rt_sel_u32(lanes, __float_as_uint(a), __float_as_uint(b))); }

#endif
