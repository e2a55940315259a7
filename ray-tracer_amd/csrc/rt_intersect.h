/*
 * rt_intersect.h — the scene sections as a kernel sees them (Lds) and the primitive tests every traversal kernel shares: the slab test in its
 * three forms, Moller-Trumbore in its two, the quad, and the closest hit among the top-level objects (rt_closest_simple).
 *
 * The arithmetic is the reference's; file:line citations are on each piece.  -ffp-contract=off is assumed (see rt_kernel.hip).
 */
#ifndef RT_INTERSECT_H
#define RT_INTERSECT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_math.h"
#include "rt_vec.h"

/* the scene sections (LDS, or global memory for what of a large scene does not fit a CU's LDS) */
struct Lds {
    const v4f *nodes;
    const v4f *tris;
    const v4f *objs;
    const v4f *meshes;
    const v4f *objtab;   /* the object list (rt_object, 3 x 16 B each), read with wave-uniform addresses */
};

/* BoundingBox::ray_hits src/objects.cu:404-434.  fminf/fmaxf drop a NaN operand like CUDA's
 * min/max; the result only ever feeds comparisons, so the sign of a zero is irrelevant. */
__device__ __forceinline__ bool box_test(float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                         V3 o, V3 inv, float &tmin_out)
{
    float tmin = 0.0f, tmax = RT_INF_F;
    float t1 = (bx0 - o.x) * inv.x, t2 = (bx1 - o.x) * inv.x;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    t1 = (by0 - o.y) * inv.y; t2 = (by1 - o.y) * inv.y;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    t1 = (bz0 - o.z) * inv.z; t2 = (bz1 - o.z) * inv.z;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    tmin_out = tmin;
    return tmin < tmax && tmax > 0.0f;
}

/* The same slab test combined with the traversal's `entry distance < best` (src/objects.cu:509,
 * :517): enter = hit && tmin < best.  tmin >= 0 always (it starts from 0 and fmaxf drops NaNs), so
 * `tmin < tmax` already implies `tmax > 0`, and with neither tmax nor best ever NaN the two
 * remaining comparisons fold into one: tmin < min(tmax, best).  Same decisions, 3 compares and 2
 * mask operations fewer per box - measurable where a wave's serial instruction stream is the
 * critical path (tools/ubench/node_step.hip: 693 -> 633 cycles per node step). */
__device__ __forceinline__ bool box_enter(float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                          V3 o, V3 inv, float best, float &tmin_out)
{
    float tmin = 0.0f, tmax = RT_INF_F;
    float t1 = (bx0 - o.x) * inv.x, t2 = (bx1 - o.x) * inv.x;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    t1 = (by0 - o.y) * inv.y; t2 = (by1 - o.y) * inv.y;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    t1 = (bz0 - o.z) * inv.z; t2 = (bz1 - o.z) * inv.z;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    tmin_out = tmin;
    return tmin < fminf(tmax, best);
}

/* The same decision and, where the box is entered, the same entry distance from six v_med3_f32 instead of ten
 * min / max (round 4; the kernel is bound by instruction issue and min / max / med3 / compares cost twice an add or a
 * multiply there).  clamp(t; a, b) = med3(a, b, t) puts t into the slab's interval [min(a,b), max(a,b)].
 * phi = clamp_z o clamp_y o clamp_x is non-decreasing; the kernel enters iff phi(0) < phi(best):
 *  - if the reference enters (tmin < min(tmax, best), tmin = max(0, near_k), tmax = min(INF, far_k)): every near_k <= tmin <
 *    far_k, so clamping 0 from below only ever raises it to the next near_k: phi(0) = tmin, the SAME float (a maximum
 *    selects one of its operands); likewise phi(best) = min(best, far_k) > tmin: entered, with the reference's distance;
 *  - if it does not: the slabs' intervals are either disjoint somewhere (then phi is constant) or have a common
 *    intersection [N, F] onto which phi clamps, and max(0, N) >= min(best, F) gives phi(0) >= phi(best); with phi
 *    monotone that is equality: not entered.
 * best <= RT_INF_F always (w_best starts there and only falls), so min(INF, ...) needs no instruction.  The argument
 * needs every product to be a number: (b - o) * inv is NaN only for 0 * inf, i.e. a direction component of exactly 0
 * (NaN directions never traverse); rays with one take box_enter (the caller checks, wave-uniformly). */
__device__ __forceinline__ bool box_enter_med3(float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                               V3 o, V3 inv, float best, float &tmin_out)
{
    const float x0 = (bx0 - o.x) * inv.x, x1 = (bx1 - o.x) * inv.x;
    const float y0 = (by0 - o.y) * inv.y, y1 = (by1 - o.y) * inv.y;
    const float z0 = (bz0 - o.z) * inv.z, z1 = (bz1 - o.z) * inv.z;
    const float lo = __builtin_amdgcn_fmed3f(z0, z1, __builtin_amdgcn_fmed3f(y0, y1, __builtin_amdgcn_fmed3f(x0, x1, 0.0f)));
    const float hi = __builtin_amdgcn_fmed3f(z0, z1, __builtin_amdgcn_fmed3f(y0, y1, __builtin_amdgcn_fmed3f(x0, x1, best)));
    tmin_out = lo;
    return lo < hi;
}

/* Triangle::hit src/objects.cu:135-163 (Moller-Trumbore, two-sided, no early out) */
__device__ __forceinline__ bool tri_test(const v4f *tris, int idx, V3 o, V3 d, float &t_out, float &u_out, float &v_out)
{
    v4f q0 = tris[3 * idx], q1 = tris[3 * idx + 1], q2 = tris[3 * idx + 2];
    V3 p0 = v3(q0.x, q0.y, q0.z), s1 = v3(q0.w, q1.x, q1.y), s2 = v3(q1.z, q1.w, q2.x);
    V3 p_vec = cross(d, s2);
    float det = dot(s1, p_vec);
    float inv_det = 1.0f / det;
    V3 t_vec = o - p0;
    float u = dot(t_vec, p_vec) * inv_det;
    V3 q_vec = cross(t_vec, s1);
    float v = dot(d, q_vec) * inv_det;
    float w = 1.0f - u - v;
    float dist = dot(s2, q_vec) * inv_det;
    t_out = dist; u_out = u; v_out = v;
    return dist > RT_EPS_F && u >= 0.0f && v >= 0.0f && w >= 0.0f;
}

/* The same test for the traversal's leaf loop, with the outcome as a lane mask (compares written straight to SGPR pairs and
 * combined there): which lanes' rays hit AND are closer than `best`.  (__ballot of a bool built from several compares costs a
 * v_cndmask and a v_cmp to rebuild the mask.) */
#define RT_FCMP_OEQ 1
#define RT_FCMP_OGT 2
#define RT_FCMP_OGE 3
#define RT_FCMP_OLT 4
__device__ __forceinline__ unsigned long long tri_closer_lanes(const v4f *tris, int idx, V3 o, V3 d, float best, float &t_out)
{
    float t, u, v;
    v4f q0 = tris[3 * idx], q1 = tris[3 * idx + 1], q2 = tris[3 * idx + 2];
    V3 p0 = v3(q0.x, q0.y, q0.z), s1 = v3(q0.w, q1.x, q1.y), s2 = v3(q1.z, q1.w, q2.x);
    V3 p_vec = cross(d, s2);
    float det = dot(s1, p_vec);
    float inv_det = 1.0f / det;        /* (the short reciprocal behind a range check is SLOWER here - monkey +3 % early in round 4, +1.4 % on its final code, cube -0.9 %: the check and its branch sit in the leaf loop) */
    V3 t_vec = o - p0;
    u = dot(t_vec, p_vec) * inv_det;
    V3 q_vec = cross(t_vec, s1);
    v = dot(d, q_vec) * inv_det;
    float w = 1.0f - u - v;
    t = dot(s2, q_vec) * inv_det;
    t_out = t;
    /* u >= 0 && v >= 0 && w >= 0 is one compare of v_minimum3_f32 (gfx950; IEEE-754-2019 minimum: a NaN operand gives NaN,
     * which fails the compare exactly as it fails its own; -0 >= 0 holds either way) */
    const float m = __builtin_elementwise_minimum(__builtin_elementwise_minimum(u, v), w);
    return __builtin_amdgcn_fcmpf(t, RT_EPS_F, RT_FCMP_OGT) & __builtin_amdgcn_fcmpf(m, 0.0f, RT_FCMP_OGE) & __builtin_amdgcn_fcmpf(t, best, RT_FCMP_OLT);
}

/* Quad::hit src/objects.cu:223-236 — t1 if it hits, whatever t2's distance; else t2 */
__device__ __forceinline__ bool quad_test(const v4f *tris, int first, V3 o, V3 d, float &t_out, int &prim_out)
{
    float t1, t2, u, v;
    bool h1 = tri_test(tris, first, o, d, t1, u, v);
    bool h2 = tri_test(tris, first + 1, o, d, t2, u, v);
    t_out = h1 ? t1 : t2;
    prim_out = h1 ? first : first + 1;
    return h1 || h2;
}

/* The closest hit among the non-mesh objects: get_ray_collision src/raytracer.cu:24-46, shared by the render kernels (px_gen,
 * UNIT_DIR: the direction comes out of normalised()) and the query kernels (rt_query_kernel.h: any direction). */
/* TRAITS (RT_TRAIT_*, rt_device_scene.h; 0 everywhere but in rt_traits_kernel): what the scene's commit has fixed about the list.
 * SPHERES_ONLY: every entry is a sphere or a mesh, so the body is the sphere test alone, the same operations in the same order, from the one
 * record of the three that a sphere uses.  With ONE_MESH as well the mesh is the entry `skip` (a kernel argument, -1 without a mesh) and is
 * passed over by a scalar compare without reading anything of it; without, an entry's type is read and compared once. */
template <bool UNIT_DIR, int TRAITS = 0>
__device__ __forceinline__ void rt_closest_simple(V3 o, V3 d, int num_objects, const Lds &L, float &best_t_out, int &best_obj_out, int &best_prim_out, int skip = -1)
{
    if (TRAITS & RT_TRAIT_SPHERES_ONLY) {
        float best_t = RT_INF_F;
        int best_obj = -1;
        /* (kept rolled: the trip count is a launch argument, and copies of the body would only add to the scalar registers held across the round) */
#pragma unroll 1
        for (int i = 0; i < num_objects; i++) {
            if (TRAITS & RT_TRAIT_ONE_MESH) {
                if (i == skip) continue;
            } else if ((int32_t)__float_as_uint(L.objtab[3 * i].x) != RT_OBJ_SPHERE) {
                continue;
            }
            const v4f ob1 = L.objtab[3 * i + 1];
            /* Sphere::hit as below: see there for the division */
            V3 cq = v3(ob1.x, ob1.y, ob1.z) - o;
            float qa = dot(d, d);
            float qb = dot(d, cq) * (-2.0f);
            float qc = dot(cq, cq) - ob1.w * ob1.w;
            float disc = qb * qb - 4.0f * qa * qc;
            if (disc >= 0.0f) {
                float dist = UNIT_DIR ? rt__div_benign(-qb - rt_sqrt(disc), 2.0f * qa) : (-qb - rt_sqrt(disc)) / (2.0f * qa);
                if (dist > RT_EPS_F && dist <= best_t) { best_t = dist; best_obj = i; }
            }
        }
        best_t_out = best_t; best_obj_out = best_obj; best_prim_out = -1;
        return;
    }
    /* get_ray_collision src/raytracer.cu:24-46 over the non-mesh objects, in list order
     * (`<=`: the later object wins ties, :36; the precision_error term is a no-op for
     * accepted hits).  Meshes are merged afterwards with the same
     * rule made explicit: smaller distance, or equal distance and larger list index. */
    float best_t = RT_INF_F;
    int best_obj = -1, best_prim = -1;
    for (int i = 0; i < num_objects; i++) {
        /* rt_object from LDS: every lane reads the same address (broadcast) */
        const v4f ob0 = L.objtab[3 * i], ob1 = L.objtab[3 * i + 1], ob2 = L.objtab[3 * i + 2];
        rt_object ob;
        /* (the record is the same for every lane, but sending its type through an SGPR - scalar branches instead of exec-mask
         * regions - was slower: +1.2 % on reference scene 0, profiles/r04/experiments/small_instruction_savings.txt) */
        ob.type = (int32_t)__float_as_uint(ob0.x); ob.prim_start = (int32_t)__float_as_uint(ob0.y);
        ob.need_uv = (int32_t)__float_as_uint(ob0.z); ob.root_ref = __float_as_uint(ob0.w);
        ob.v[0] = ob1.x; ob.v[1] = ob1.y; ob.v[2] = ob1.z; ob.v[3] = ob1.w;
        ob.v[4] = ob2.x; ob.v[5] = ob2.y; ob.v[6] = ob2.z; ob.v[7] = ob2.w;
        bool hit = false;
        float t = RT_INF_F;
        int prim = -1;
        switch (ob.type) {
            case RT_OBJ_SPHERE: {   /* Sphere::hit src/objects.cu:40-79: near root, > 1e-6 */
                V3 cq = v3(ob.v[0], ob.v[1], ob.v[2]) - o;
                float qa = dot(d, d);
                float qb = dot(d, cq) * (-2.0f);
                float qc = dot(cq, cq) - ob.v[3] * ob.v[3];
                float disc = qb * qb - 4.0f * qa * qc;
                if (disc >= 0.0f) {
                    /* The near root's division in its short form (rt_math.h rt__div_benign).  d comes out of normalised(): a unit vector to a
                     * few ulp, so the divisor is 2 to a few ulp - or d has a NaN (divisor NaN: the quotient is NaN either way), or it is the
                     * zero vector (a vector whose squared length overflowed: then b and the dividend are zeros too and both forms give
                     * 0 / 0 = NaN).  For a dividend that form's precondition excludes - below 2^-100 in magnitude,
                     * or infinite - it may return another value than the operator, but never one that changes what follows: such a quotient is
                     * below RT_EPS_F (rejected), or - an infinite dividend: inf from the operator, NaN from the short form - fails
                     * `dist > RT_EPS_F` or `t <= best_t` (best_t <= 2^30) alike; every distance that IS accepted comes from a dividend between
                     * 2e-6 and 2^31, where the two agree bit for bit.  The operator's form, should parity ever need it, is
                     * `float dist = (-qb - rt_sqrt(disc)) / (2.0f * qa);` (profiles/r04/experiments/sphere_divide.txt) - which is what a caller
                     * whose direction is NOT a unit vector gets (!UNIT_DIR: the ray queries of rt_query_kernel.h take the ray as given). */
                    float dist = UNIT_DIR ? rt__div_benign(-qb - rt_sqrt(disc), 2.0f * qa) : (-qb - rt_sqrt(disc)) / (2.0f * qa);
                    if (dist > RT_EPS_F) { hit = true; t = dist; }
                }
                break;
            }
            case RT_OBJ_TRIANGLE: {
                float u, v;
                hit = tri_test(L.tris, ob.prim_start, o, d, t, u, v);
                prim = ob.prim_start;
                break;
            }
            case RT_OBJ_ONE_WAY_QUAD:   /* src/objects.cu:273-280 */
                if (dot(d, v3(ob.v[0], ob.v[1], ob.v[2])) < 0.0f) break;
                /* fall through */
            case RT_OBJ_QUAD:
                hit = quad_test(L.tris, ob.prim_start, o, d, t, prim);
                break;
            case RT_OBJ_CUBOID: {       /* src/objects.cu:305-322: strict <, first face wins ties */
                float cb = RT_INF_F;
                for (int fc = 0; fc < 6; fc++) {
                    float ft; int fp;
                    bool fh = quad_test(L.tris, ob.prim_start + 2 * fc, o, d, ft, fp);
                    if (fh && ft < cb) { cb = ft; prim = fp; hit = true; }
                }
                t = cb;
                break;
            }
            default: break;             /* RT_OBJ_MESH: traversed separately */
        }
        if (hit && t <= best_t) { best_t = t; best_obj = i; best_prim = prim; }
    }
    best_t_out = best_t; best_obj_out = best_obj; best_prim_out = best_prim;
}

#endif
