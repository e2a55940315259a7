/*
 * rt_winding.h — winding-number queries (rt_winding_numbers[_device], rt_signed_distance[_device], include/rt_amd.h): what the kernel
 * (rt_winding_kernel.h), the entry points (rt_winding_capi.cpp) and the host tests (tests/sanitize/winding_host_check.cpp) share.  Host
 * code; self-contained.
 *
 *  - the arithmetic, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off):
 *    rt_wn_atan2, the term of a triangle record, the sphere and cuboid rules, an object's winding number, the sum over the solids;
 *  - the argument block (the launcher is rt_launch.h's rt_launch_winding).
 *
 * The definition - every formula in the order it is evaluated - is include/rt_amd.h's.  Nothing here depends on the point but the
 * arithmetic: every loop bound and every record address comes from the scene alone, so on the device all lanes of a wave are on the same
 * record at the same time and the records are read by wave-uniform addresses.
 */
#ifndef RT_WINDING_H
#define RT_WINDING_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"

#if defined(__HIPCC__)
#define RT_WN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT_WN_HD inline
#endif

#define RT_WINDING_MAX_POINTS (1 << 30)    /* points of one call (point ids and the chunk counter are 32-bit) */

/* the scene as the queries read it; F4 is a 16-byte unit with members x, y, z, w (rt_f4 on the host, the kernels' v4f on the device).  perm:
 * per triangle record of a mesh the commit index, within its mesh, of the one at that position; flip: one byte per triangle in commit
 * order at [the mesh's first record + commit index], four to a word */
template <class F4> struct rt_wn_scene {
    const F4 *tris, *objtab;
    const int32_t *perm;
    const uint32_t *flip;
    int32_t num_objects, num_tris;
};

RT_WN_HD uint32_t rt_wn_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_WN_HD float rt_wn_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
RT_WN_HD bool rt_wn_finite(float f) { return (rt_wn_bits(f) & 0x7f800000u) != 0x7f800000u; }
RT_WN_HD float rt_wn_abs(float f) { return rt_wn_float(rt_wn_bits(f) & 0x7fffffffu); }
RT_WN_HD float rt_wn_neg(float f) { return rt_wn_float(rt_wn_bits(f) ^ 0x80000000u); }

/* ---- the arithmetic ------------------------------------------------------------------------------------------------------------ */
RT_WN_HD float rt_wn_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* atan2(y, x) in binary32 without libm (include/rt_amd.h has the text): one division, the odd polynomial q * P(q * q) by Horner, the
 * quadrant fix-ups by compare and select.  Against binary64's atan2 the result is within 5.1 * 2^-24 absolute over 10^7 random arguments
 * of either sign and a magnitude ratio up to 2^20 either way (the polynomial itself within 1.72 * 2^-24 on [0, 1]; the rest is the spacing
 * of binary32 near pi and the rounding of pi); tests/winding_ref.py measures it. */
RT_WN_HD float rt_wn_atan2(float y, float x)
{
    const float ay = rt_wn_abs(y), ax = rt_wn_abs(x);
    const bool steep = ay > ax;
    const float mn = steep ? ax : ay, mx = steep ? ay : ax;
    const float q = mn / mx;
    const float s = q * q;
    float p = RT_WN_C8;
    p = p * s + RT_WN_C7;
    p = p * s + RT_WN_C6;
    p = p * s + RT_WN_C5;
    p = p * s + RT_WN_C4;
    p = p * s + RT_WN_C3;
    p = p * s + RT_WN_C2;
    p = p * s + RT_WN_C1;
    p = p * s + RT_WN_C0;
    float r = q * p;
    r = steep ? RT_WN_PI_2 - r : r;
    r = x < 0.0f ? RT_WN_PI - r : r;
    return y < 0.0f ? rt_wn_neg(r) : r;
}

/* the term of a triangle record q0 = (p0.xyz, s1.x), q1 = (s1.yz, s2.xy), q2 = (s2.z, ...) for the point p, before its sign: the angle
 * atan2(det, den) of Van Oosterom and Strackee, half the solid angle the triangle subtends */
template <class F4>
RT_WN_HD float rt_wn_term(const F4 q0, const F4 q1, const F4 q2, float px, float py, float pz)
{
    const float s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
    const float ax = q0.x - px, ay = q0.y - py, az = q0.z - pz;
    const float bx = ax + s1x, by = ay + s1y, bz = az + s1z;
    const float cx = ax + s2x, cy = ay + s2y, cz = az + s2z;
    const float la = sqrtf(rt_wn_dot(ax, ay, az, ax, ay, az));
    const float lb = sqrtf(rt_wn_dot(bx, by, bz, bx, by, bz));
    const float lc = sqrtf(rt_wn_dot(cx, cy, cz, cx, cy, cz));
    const float nx = s1y * s2z - s1z * s2y, ny = s1z * s2x - s1x * s2z, nz = s1x * s2y - s1y * s2x;
    const float det = rt_wn_dot(ax, ay, az, nx, ny, nz);
    const float den = ((la * lb) * lc + rt_wn_dot(ax, ay, az, bx, by, bz) * lc) + (rt_wn_dot(ax, ay, az, cx, cy, cz) * lb + rt_wn_dot(bx, by, bz, cx, cy, cz) * la);
    const float t = rt_wn_atan2(det, den);
    return det == 0.0f ? 0.0f : t;
}

/* a sphere (c, r) */
RT_WN_HD float rt_wn_sphere(float cx, float cy, float cz, float r, float px, float py, float pz)
{
    const float vx = px - cx, vy = py - cy, vz = pz - cz;
    return rt_wn_dot(vx, vy, vz, vx, vy, vz) < r * r ? 1.0f : 0.0f;
}

/* a mesh record's flip byte: the mesh's first record is `base`, the record's commit index within the mesh `commit` (its entry of perm) */
template <class F4>
RT_WN_HD uint32_t rt_wn_flip(const rt_wn_scene<F4> &S, int32_t base, int32_t commit)
{
    const uint32_t at = (uint32_t)(base + commit);
    return (S.flip[at >> 2] >> ((at & 3u) * 8u)) & 1u;
}

/* The winding number of object i (rt_object: type, prim_start, ..., v[0..3] = c, r of a sphere) for the point p.  The records are read
 * one ahead: the next one's loads are issued before the current one's term is formed. */
template <class F4>
RT_WN_HD float rt_wn_object(const rt_wn_scene<F4> &S, int32_t i, float px, float py, float pz)
{
    const F4 ob0 = S.objtab[3 * i];
    const int32_t type = (int32_t)rt_wn_bits(ob0.x), prim = (int32_t)rt_wn_bits(ob0.y);
    if (type == RT_OBJ_SPHERE) {
        const F4 ob1 = S.objtab[3 * i + 1];
        return rt_wn_sphere(ob1.x, ob1.y, ob1.z, ob1.w, px, py, pz);
    }
    if (type == RT_OBJ_CUBOID) {
        /* the box: componentwise min and max of p0 over the twelve records (every corner coordinate occurs among them) */
        const F4 first = S.tris[3 * (size_t)prim];
        float lox = first.x, loy = first.y, loz = first.z, hix = first.x, hiy = first.y, hiz = first.z;
        for (int32_t k = 1; k < 12; k++) {
            const F4 q0 = S.tris[3 * (size_t)(prim + k)];
            lox = q0.x < lox ? q0.x : lox; loy = q0.y < loy ? q0.y : loy; loz = q0.z < loz ? q0.z : loz;
            hix = q0.x > hix ? q0.x : hix; hiy = q0.y > hiy ? q0.y : hiy; hiz = q0.z > hiz ? q0.z : hiz;
        }
        return (lox < px && px < hix) && (loy < py && py < hiy) && (loz < pz && pz < hiz) ? 1.0f : 0.0f;
    }
    int32_t end = prim + (type == RT_OBJ_TRIANGLE ? 1 : 2);
    if (type == RT_OBJ_MESH) {
        end = S.num_tris;
        if (i + 1 < S.num_objects) end = (int32_t)rt_wn_bits(S.objtab[3 * (i + 1)].y);
    }
    float A = 0.0f;
    if (prim >= end) return A * RT_INV_2PI;
    const bool mesh = type == RT_OBJ_MESH;
    const F4 *t = S.tris + 3 * (size_t)prim;
    F4 n0 = t[0], n1 = t[1], n2 = t[2];
    uint32_t nflip = mesh ? rt_wn_flip(S, prim, S.perm[prim]) : 0u;
    int32_t ncommit = mesh && prim + 1 < end ? S.perm[prim + 1] : 0;       /* (the order list two ahead: the flip word's address then waits for nothing) */
    for (int32_t k = prim; k < end; k++) {
        const F4 q0 = n0, q1 = n1, q2 = n2;
        const uint32_t flip = nflip;
        if (k + 1 < end) {
            t += 3;
            n0 = t[0]; n1 = t[1]; n2 = t[2];
            nflip = mesh ? rt_wn_flip(S, prim, ncommit) : 1u;              /* a quad's second record turns the other way */
            if (mesh && k + 2 < end) ncommit = S.perm[k + 2];
        }
        const float term = rt_wn_term(q0, q1, q2, px, py, pz);
        A = A + (flip ? rt_wn_neg(term) : term);
    }
    return A * RT_INV_2PI;
}

/* what a query answers for the point p: object >= 0 that object's winding number; RT_WINDING_SOLIDS the sum over the spheres, cuboids
 * and meshes in list order.  A point that is not finite, and a NaN sum: the canonical quiet NaN */
template <class F4>
RT_WN_HD float rt_wn_point(const rt_wn_scene<F4> &S, int32_t object, float px, float py, float pz)
{
    const bool ok = rt_wn_finite(px) && rt_wn_finite(py) && rt_wn_finite(pz);
    const float x = ok ? px : 0.0f, y = ok ? py : 0.0f, z = ok ? pz : 0.0f;     /* (a stand-in: the loop stays the same for every lane) */
    float w = 0.0f;
    if (object >= 0) {
        w = rt_wn_object(S, object, x, y, z);
    } else {
        for (int32_t i = 0; i < S.num_objects; i++) {
            const int32_t type = (int32_t)rt_wn_bits(S.objtab[3 * i].x);
            if (type != RT_OBJ_SPHERE && type != RT_OBJ_CUBOID && type != RT_OBJ_MESH) continue;
            w = w + rt_wn_object(S, i, x, y, z);
        }
    }
    return ok && w == w ? w : rt_wn_float(0x7FC00000u);
}

RT_WN_HD bool rt_wn_inside(float w) { return rt_wn_abs(w) >= 0.5f; }      /* (false for a NaN) */
/* the signed distance from the point's nearest-surface record */
RT_WN_HD float rt_wn_sdf(float w, float distance) { return rt_wn_inside(w) ? rt_wn_neg(distance) : distance; }

/* ---- the argument block ------------------------------------------------------------------------------------------------------- */
typedef struct {
    const rt_f4 *blob;
    int32_t off_tris, off_objtab;
    int32_t num_objects, num_tris;
    const int32_t *perm;               /* num_tris entries (rt_scene::d_perm) */
    const uint32_t *flip;              /* num_tris bytes, padded to whole words (rt_scene::d_flip) */
    /* the work: points [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    const float *points;               /* n x 3 floats */
    int32_t object;                    /* an object's index, or RT_WINDING_SOLIDS */
    float *winding;                    /* n floats, or NULL */
    uint8_t *inside;                   /* n bytes, or NULL */
    const rt_nearest *nearest;         /* with sdf: the points' nearest-surface records */
    float *sdf;                        /* n floats, or NULL */
} rt_winding_args;

#endif
