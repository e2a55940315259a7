/*
 * rt_tritri.h — triangle-overlap queries (rt_overlap_triangles[_device], include/rt_amd.h): what the kernel (rt_tritri_kernel.h), the entry
 * points (rt_tritri_capi.cpp) and the host tests (tests/sanitize/tritri_host_check.cpp) share.  Host code; self-contained.
 *
 *  - the tests, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off): a
 *    query's validity, bounding box and normal; a triangle record taken through the header's five steps (the query's box by compares, the
 *    two height tests, the in-plane axes of a coplanar pair, Moeller's intervals); a sphere by the nearest section's point-triangle
 *    distance; the segment of a pair that overlaps;
 *  - the traversal of one mesh as steps over rt_overlap.h's state (rt_ov_walk): rt_ov_step with another leaf test.  The path rule is
 *    rt_ov_boxes as it stands, on the query's bounding box; the ids are kept by rt_ov_insert in an rt_ov_buf.
 *
 *  - the argument block (the launcher is rt_launch.h's rt_launch_tritri).
 *
 * The definition - every formula in the order it is evaluated - is include/rt_amd.h's.
 */
#ifndef RT_TRITRI_H
#define RT_TRITRI_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"
#include "rt_multihit.h"        /* RT_MH_MAX_OBJECTS, RT_MH_NO_TRI, RT_MH_UNIFORM */
#include "rt_nearest.h"         /* rt_nr_tri: the point-triangle distance of the sphere test */
#include "rt_overlap.h"         /* rt_ov_box, rt_ov_boxes, rt_ov_buf, rt_ov_offer, rt_ov_walk */

#define RT_TRITRI_MAX_TRIANGLES (1 << 30)  /* query triangles of one call (ids and the chunk counter are 32-bit) */
#define RT_TT_NAN_BITS 0x7fc00000u         /* the floats of a kind-2 segment */

/* the query triangle: as given, its normal, and its bounding box in rt_overlap.h's form (lo and hi; the centre and half extents are not used) */
struct rt_tt_tri { float a0x, a0y, a0z, a1x, a1y, a1z, a2x, a2y, a2z, nx, ny, nz; rt_ov_box box; };
/* a 16-byte unit of the host side (the kernels have v4f) */
struct rt_tt_f4 { float x, y, z, w; };

RT_OV_HD float rt_tt_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
RT_OV_HD bool rt_tt_above(float a, float b, float c) { return (a > 0.0f) & (b > 0.0f) & (c > 0.0f); }
RT_OV_HD bool rt_tt_below(float a, float b, float c) { return (a < 0.0f) & (b < 0.0f) & (c < 0.0f); }
RT_OV_HD bool rt_tt_zero(float a, float b, float c) { return (a == 0.0f) & (b == 0.0f) & (c == 0.0f); }

/* ---- the query -------------------------------------------------------------------------------------------------------------------- */
/* the start of a query: false for a triangle that overlaps nothing (a float that is not finite).  lo / hi, e1, e2 and na */
RT_OV_HD bool rt_tt_begin(rt_tt_tri &t)
{
    if (!rt_ov_finite(t.a0x) || !rt_ov_finite(t.a0y) || !rt_ov_finite(t.a0z) || !rt_ov_finite(t.a1x) || !rt_ov_finite(t.a1y) || !rt_ov_finite(t.a1z) ||
        !rt_ov_finite(t.a2x) || !rt_ov_finite(t.a2y) || !rt_ov_finite(t.a2z)) return false;
    t.box.lox = fminf(fminf(t.a0x, t.a1x), t.a2x); t.box.loy = fminf(fminf(t.a0y, t.a1y), t.a2y); t.box.loz = fminf(fminf(t.a0z, t.a1z), t.a2z);
    t.box.hix = fmaxf(fmaxf(t.a0x, t.a1x), t.a2x); t.box.hiy = fmaxf(fmaxf(t.a0y, t.a1y), t.a2y); t.box.hiz = fmaxf(fmaxf(t.a0z, t.a1z), t.a2z);
    t.box.cx = t.box.cy = t.box.cz = t.box.hx = t.box.hy = t.box.hz = 0.0f;
    const float e1x = t.a1x - t.a0x, e1y = t.a1y - t.a0y, e1z = t.a1z - t.a0z, e2x = t.a2x - t.a0x, e2y = t.a2y - t.a0y, e2z = t.a2z - t.a0z;
    t.nx = e1y * e2z - e1z * e2y; t.ny = e1z * e2x - e1x * e2z; t.nz = e1x * e2y - e1y * e2x;
    return true;
}

/* ---- Moeller's intervals ---------------------------------------------------------------------------------------------------------- */
/* the lone vertex of heights (h0, h1, h2) that are neither all above, all below nor all zero, by Moeller's sign rule: exactly one of
 * l0, l1, l2 is set.  Selects, no branch */
RT_OV_HD void rt_tt_lone(float h0, float h1, float h2, bool &l0, bool &l1, bool &l2)
{
    const bool c1 = h0 * h1 > 0.0f, c2 = h0 * h2 > 0.0f, c3 = (h1 * h2 > 0.0f) | (h0 != 0.0f), c4 = h1 != 0.0f;
    l2 = c1 | (!c2 & !c3 & !c4);
    l1 = !c1 & (c2 | (!c3 & c4));
    l0 = !l1 & !l2;
}

/* where the edge from the lone vertex (value vl, height hl) to another (vo, ho) crosses the other plane: one IEEE division; vl where the
 * denominator is zero.  The value is a projection (the interval's end) or a coordinate (the segment's end): the same quotient */
RT_OV_HD float rt_tt_cross_at(float vl, float vo, float hl, float ho)
{
    const float den = hl - ho;
    const float x = vl + (vo - vl) * (hl / den);
    return den == 0.0f ? vl : x;
}

/* the two ends of a triangle's interval: values (v0, v1, v2) at heights (h0, h1, h2).  The lone vertex l and the others in index order:
 * l = 2: (0, 1); l = 1: (0, 2); l = 0: (1, 2) */
RT_OV_HD void rt_tt_ends(float v0, float v1, float v2, float h0, float h1, float h2, bool l0, bool l1, float &x1, float &x2)
{
    const float vl = l0 ? v0 : l1 ? v1 : v2, hl = l0 ? h0 : l1 ? h1 : h2;
    const float va = l0 ? v1 : v0, ha = l0 ? h1 : h0;
    const float vb = (l0 | l1) ? v2 : v1, hb = (l0 | l1) ? h2 : h1;
    x1 = rt_tt_cross_at(vl, va, hl, ha);
    x2 = rt_tt_cross_at(vl, vb, hl, hb);
}

/* one in-plane axis X of a coplanar pair: true when the query's three projections (u) lie strictly to one side of the record's three (w) */
RT_OV_HD bool rt_tt_axis(float u0, float u1, float u2, float w0, float w1, float w2)
{
    const bool lt = (u0 < w0) & (u0 < w1) & (u0 < w2) & (u1 < w0) & (u1 < w1) & (u1 < w2) & (u2 < w0) & (u2 < w1) & (u2 < w2);
    const bool gt = (u0 > w0) & (u0 > w1) & (u0 > w2) & (u1 > w0) & (u1 > w1) & (u1 > w2) & (u2 > w0) & (u2 > w1) & (u2 > w2);
    return lt | gt;
}

/* the axis cross(n, f) and the verdict on it: z, e1, e2 are the query's vertices taken from a0 (z the zero vector), d0..d2 the record's */
RT_OV_HD bool rt_tt_edge_axis(float nx, float ny, float nz, float fx, float fy, float fz, float zx, float zy, float zz, float e1x, float e1y, float e1z,
                              float e2x, float e2y, float e2z, float d0x, float d0y, float d0z, float d1x, float d1y, float d1z, float d2x, float d2y, float d2z)
{
    const float xx = ny * fz - nz * fy, xy = nz * fx - nx * fz, xz = nx * fy - ny * fx;
    return rt_tt_axis(rt_tt_dot(xx, xy, xz, zx, zy, zz), rt_tt_dot(xx, xy, xz, e1x, e1y, e1z), rt_tt_dot(xx, xy, xz, e2x, e2y, e2z),
                      rt_tt_dot(xx, xy, xz, d0x, d0y, d0z), rt_tt_dot(xx, xy, xz, d1x, d1y, d1z), rt_tt_dot(xx, xy, xz, d2x, d2y, d2z));
}

/* ---- a triangle record ------------------------------------------------------------------------------------------------------------- */
/* A record q0 = (p0.xyz, s1.x), q1 = (s1.yz, s2.xy), q2 = (s2.z, ...) against the query: the header's steps 1 to 5.  true: the pair
 * overlaps.  With SEGMENT (a pair that is known to overlap: the finish of a query) nothing leaves early and seg receives the pair's
 * segment; without it the three compare axes and the two height tests leave at once where they separate - most triangles a leaf holds -
 * and the interval part is formed without a branch between its verdicts (rt_ov_tri's comment has the reason: nested exits are lane masks
 * in scalar registers across the kernel's wave loop).  The coplanar pair is the one branch behind the height tests: it is rare. */
template <bool SEGMENT, class F4>
RT_OV_HD bool rt_tt_record(const F4 q0, const F4 q1, const F4 q2, const rt_tt_tri &t, rt_tri_segment *seg)
{
    const float px = q0.x, py = q0.y, pz = q0.z, s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
    const float bx = px + s1x, by = py + s1y, bz = pz + s1z, cx = px + s2x, cy = py + s2y, cz = pz + s2z;
    const rt_ov_box &b = t.box;
    /* 1. the query's bounding box: compares on lo and hi themselves */
    const bool sx = ((px > b.hix) & (bx > b.hix) & (cx > b.hix)) | ((px < b.lox) & (bx < b.lox) & (cx < b.lox));
    const bool sy = ((py > b.hiy) & (by > b.hiy) & (cy > b.hiy)) | ((py < b.loy) & (by < b.loy) & (cy < b.loy));
    const bool sz = ((pz > b.hiz) & (bz > b.hiz) & (cz > b.hiz)) | ((pz < b.loz) & (bz < b.loz) & (cz < b.loz));
    if (!SEGMENT && (sx | sy | sz)) return false;
    /* 2. the query over the record's plane */
    const float mx = s1y * s2z - s1z * s2y, my = s1z * s2x - s1x * s2z, mz = s1x * s2y - s1y * s2x;     /* nb */
    const float hA0 = rt_tt_dot(mx, my, mz, t.a0x - px, t.a0y - py, t.a0z - pz);
    const float hA1 = rt_tt_dot(mx, my, mz, t.a1x - px, t.a1y - py, t.a1z - pz);
    const float hA2 = rt_tt_dot(mx, my, mz, t.a2x - px, t.a2y - py, t.a2z - pz);
    const bool above_b = rt_tt_above(hA0, hA1, hA2), below_b = rt_tt_below(hA0, hA1, hA2);
    if (!SEGMENT && (above_b | below_b)) return false;
    /* 3. the record over the query's plane */
    const float d0x = px - t.a0x, d0y = py - t.a0y, d0z = pz - t.a0z;
    const float d1x = bx - t.a0x, d1y = by - t.a0y, d1z = bz - t.a0z;
    const float d2x = cx - t.a0x, d2y = cy - t.a0y, d2z = cz - t.a0z;
    const float hB0 = rt_tt_dot(t.nx, t.ny, t.nz, d0x, d0y, d0z);
    const float hB1 = rt_tt_dot(t.nx, t.ny, t.nz, d1x, d1y, d1z);
    const float hB2 = rt_tt_dot(t.nx, t.ny, t.nz, d2x, d2y, d2z);
    const bool above_a = rt_tt_above(hB0, hB1, hB2), below_a = rt_tt_below(hB0, hB1, hB2);
    if (!SEGMENT && (above_a | below_a)) return false;
    const float zx = t.a0x - t.a0x, zy = t.a0y - t.a0y, zz = t.a0z - t.a0z;
    const float e1x = t.a1x - t.a0x, e1y = t.a1y - t.a0y, e1z = t.a1z - t.a0z, e2x = t.a2x - t.a0x, e2y = t.a2y - t.a0y, e2z = t.a2z - t.a0z;
    /* 4. a coplanar pair, or a vanished normal: the six in-plane axes */
    const bool flat_a = rt_tt_zero(hA0, hA1, hA2), flat_b = rt_tt_zero(hB0, hB1, hB2);
    if (flat_a | flat_b) {
        if (SEGMENT) {
            uint32_t nan = RT_TT_NAN_BITS;
            float f;
            __builtin_memcpy(&f, &nan, 4);
            seg->p[0] = seg->p[1] = seg->p[2] = seg->q[0] = seg->q[1] = seg->q[2] = f;
            seg->kind = 2;
            seg->reserved = 0;
            return true;
        }
        bool sep = rt_tt_edge_axis(t.nx, t.ny, t.nz, e1x, e1y, e1z, zx, zy, zz, e1x, e1y, e1z, e2x, e2y, e2z, d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z);
        sep |= rt_tt_edge_axis(t.nx, t.ny, t.nz, t.a2x - t.a1x, t.a2y - t.a1y, t.a2z - t.a1z, zx, zy, zz, e1x, e1y, e1z, e2x, e2y, e2z, d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z);
        sep |= rt_tt_edge_axis(t.nx, t.ny, t.nz, t.a0x - t.a2x, t.a0y - t.a2y, t.a0z - t.a2z, zx, zy, zz, e1x, e1y, e1z, e2x, e2y, e2z, d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z);
        sep |= rt_tt_edge_axis(mx, my, mz, s1x, s1y, s1z, zx, zy, zz, e1x, e1y, e1z, e2x, e2y, e2z, d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z);
        sep |= rt_tt_edge_axis(mx, my, mz, s2x - s1x, s2y - s1y, s2z - s1z, zx, zy, zz, e1x, e1y, e1z, e2x, e2y, e2z, d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z);
        sep |= rt_tt_edge_axis(mx, my, mz, -s2x, -s2y, -s2z, zx, zy, zz, e1x, e1y, e1z, e2x, e2y, e2z, d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z);
        return !sep;
    }
    /* 5. the intervals on D = cross(na, nb) */
    const float Dx = t.ny * mz - t.nz * my, Dy = t.nz * mx - t.nx * mz, Dz = t.nx * my - t.ny * mx;
    const float pA0 = rt_tt_dot(Dx, Dy, Dz, zx, zy, zz), pA1 = rt_tt_dot(Dx, Dy, Dz, e1x, e1y, e1z), pA2 = rt_tt_dot(Dx, Dy, Dz, e2x, e2y, e2z);
    const float pB0 = rt_tt_dot(Dx, Dy, Dz, d0x, d0y, d0z), pB1 = rt_tt_dot(Dx, Dy, Dz, d1x, d1y, d1z), pB2 = rt_tt_dot(Dx, Dy, Dz, d2x, d2y, d2z);
    bool la0, la1, la2, lb0, lb1, lb2;
    rt_tt_lone(hA0, hA1, hA2, la0, la1, la2);
    rt_tt_lone(hB0, hB1, hB2, lb0, lb1, lb2);
    float xA1, xA2, xB1, xB2;
    rt_tt_ends(pA0, pA1, pA2, hA0, hA1, hA2, la0, la1, xA1, xA2);
    rt_tt_ends(pB0, pB1, pB2, hB0, hB1, hB2, lb0, lb1, xB1, xB2);
    if (!SEGMENT) {
        /* one interval's maximum below the other's minimum: all four compares of their ends.  A NaN holds in none */
        const bool a_below = (xA1 < xB1) & (xA1 < xB2) & (xA2 < xB1) & (xA2 < xB2);
        const bool b_below = (xB1 < xA1) & (xB1 < xA2) & (xB2 < xA1) & (xB2 < xA2);
        return !(a_below | b_below);
    }
    /* the segment: each interval's ends in order (end 1 is the minimum where x1 <= x2), the lower end from the interval whose minimum is
     * larger, the upper from the one whose maximum is smaller, a tie to the query; the point is the edge crossing with the same quotient */
    float a1[3], a2[3], b1[3], b2[3];
    rt_tt_ends(t.a0x, t.a1x, t.a2x, hA0, hA1, hA2, la0, la1, a1[0], a2[0]);
    rt_tt_ends(t.a0y, t.a1y, t.a2y, hA0, hA1, hA2, la0, la1, a1[1], a2[1]);
    rt_tt_ends(t.a0z, t.a1z, t.a2z, hA0, hA1, hA2, la0, la1, a1[2], a2[2]);
    rt_tt_ends(px, bx, cx, hB0, hB1, hB2, lb0, lb1, b1[0], b2[0]);
    rt_tt_ends(py, by, cy, hB0, hB1, hB2, lb0, lb1, b1[1], b2[1]);
    rt_tt_ends(pz, bz, cz, hB0, hB1, hB2, lb0, lb1, b1[2], b2[2]);
    const bool a_in_order = xA1 <= xA2, b_in_order = xB1 <= xB2;
    const float minA = a_in_order ? xA1 : xA2, maxA = a_in_order ? xA2 : xA1, minB = b_in_order ? xB1 : xB2, maxB = b_in_order ? xB2 : xB1;
    const bool lower_b = minB > minA, upper_b = maxB < maxA;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a_min = a_in_order ? a1[c] : a2[c], a_max = a_in_order ? a2[c] : a1[c];
        const float b_min = b_in_order ? b1[c] : b2[c], b_max = b_in_order ? b2[c] : b1[c];
        seg->p[c] = lower_b ? b_min : a_min;
        seg->q[c] = upper_b ? b_max : a_max;
    }
    seg->kind = 1;
    seg->reserved = 0;
    return true;
}

template <class F4>
RT_OV_HD bool rt_tt_test(const F4 q0, const F4 q1, const F4 q2, const rt_tt_tri &t) { return rt_tt_record<false>(q0, q1, q2, t, (rt_tri_segment *)nullptr); }

/* ---- a sphere ---------------------------------------------------------------------------------------------------------------------- */
/* a sphere (c, R) as a surface: the nearest section's squared distance from c to the record (a0, e1, e2) no larger than R * R, the
 * largest of the three squared vertex distances no smaller */
template <class F4>
RT_OV_HD bool rt_tt_sphere(float cx, float cy, float cz, float R, const rt_tt_tri &t)
{
    F4 q0, q1, q2;
    q0.x = t.a0x; q0.y = t.a0y; q0.z = t.a0z; q0.w = t.a1x - t.a0x;
    q1.x = t.a1y - t.a0y; q1.y = t.a1z - t.a0z; q1.z = t.a2x - t.a0x; q1.w = t.a2y - t.a0y;
    q2.x = t.a2z - t.a0z; q2.y = 0.0f; q2.z = 0.0f; q2.w = 0.0f;
    float pt[3];
    const float near2 = rt_nr_tri(q0, q1, q2, cx, cy, cz, pt);
    const float v0x = t.a0x - cx, v0y = t.a0y - cy, v0z = t.a0z - cz, v1x = t.a1x - cx, v1y = t.a1y - cy, v1z = t.a1z - cz;
    const float v2x = t.a2x - cx, v2y = t.a2y - cy, v2z = t.a2z - cz;
    const float far2 = fmaxf(fmaxf(rt_tt_dot(v0x, v0y, v0z, v0x, v0y, v0z), rt_tt_dot(v1x, v1y, v1z, v1x, v1y, v1z)), rt_tt_dot(v2x, v2y, v2z, v2x, v2y, v2z));
    const float rr = R * R;
    return near2 <= rr && far2 >= rr;
}

/* ---- the objects that are not meshes (rt_ov_simple with the tests above) ---------------------------------------------------------- */
template <class F4>
RT_OV_HD void rt_tt_simple(const rt_ov_scene<F4> &S, int32_t num_objects, const rt_tt_tri &t, int32_t k, bool any_only, rt_ov_buf &b)
{
#pragma unroll 1
    for (int32_t i = 0; i < num_objects; i++) {
        const F4 ob0 = S.objtab[3 * i], ob1 = S.objtab[3 * i + 1];
        const int32_t type = RT_MH_UNIFORM((int32_t)rt_ov_bits(ob0.x)), prim = RT_MH_UNIFORM((int32_t)rt_ov_bits(ob0.y));
        const int32_t faces = type == RT_OBJ_MESH ? 0 : type == RT_OBJ_SPHERE ? 1 : rt_ov_object_tris(type);
#pragma unroll 1
        for (int32_t fc = 0; fc < faces; fc++) {
            bool hit;
            uint32_t field = RT_MH_NO_TRI;
            if (type == RT_OBJ_SPHERE) {
                hit = rt_tt_sphere<F4>(ob1.x, ob1.y, ob1.z, ob1.w, t);
            } else {
                const F4 *q = S.tris + 3 * (size_t)(prim + fc);
                hit = rt_tt_test(q[0], q[1], q[2], t);
                field = (uint32_t)(prim + fc);
            }
            rt_ov_offer(b, k, hit, i, field);
        }
        if (any_only && b.total > 0u) return;
    }
}

/* ---- the traversal of one mesh: rt_ov_mesh_begin on t.box, and rt_ov_step with the triangle test as the leaf test ------------------- */
template <int STRIDE, class F4>
RT_OV_HD bool rt_tt_step(const rt_ov_scene<F4> &S, uint32_t *stack, int32_t object, const rt_tt_tri &t, int32_t k, rt_ov_buf &b, rt_ov_walk &w)
{
    if (!(w.cur & RT_REF_LEAF)) {
        const F4 *n = S.nodes + 4 * (size_t)(w.cur & RT_REF_NODE_MASK);
        const F4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
        const bool ol = rt_ov_boxes(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, t.box);
        const bool orr = rt_ov_boxes(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, t.box);
        const uint32_t lref = rt_ov_bits(q3.x) & ~RT_REF_CHAIN, rref = rt_ov_bits(q3.y) & ~RT_REF_CHAIN;
        if (ol && orr) {
            stack[(size_t)w.sp * (2 * STRIDE)] = rref;
            w.sp++;
        }
        w.at = 0;
        if (ol) { w.cur = lref; return true; }
        if (orr) { w.cur = rref; return true; }
    } else {
        const int32_t start = (int32_t)(w.cur & RT_REF_START_MASK), count = (int32_t)((w.cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        if (w.at < count) {
            const F4 *q = S.tris + 3 * (size_t)(start + w.at);
            rt_ov_offer(b, k, rt_tt_test(q[0], q[1], q[2], t), object, (uint32_t)(start + w.at));
            w.at++;
            if (w.at < count) return true;
        }
    }
    if (w.sp > 0) {
        w.sp--;
        w.cur = stack[(size_t)w.sp * (2 * STRIDE)];
        w.at = 0;
        return true;
    }
    return false;
}

/* ---- the finish -------------------------------------------------------------------------------------------------------------------- */
/* rank q's segment from its id word: an empty slot (kind 0, zeros), a sphere (kind 2, NaNs), or the pair's */
template <class F4>
RT_OV_HD rt_tri_segment rt_tt_segment(const rt_ov_scene<F4> &S, uint32_t word, bool held, const rt_tt_tri &t)
{
    rt_tri_segment seg;
    seg.p[0] = seg.p[1] = seg.p[2] = seg.q[0] = seg.q[1] = seg.q[2] = 0.0f;
    seg.kind = 0;
    seg.reserved = 0;
    if (held) {
        const uint32_t field = word & RT_MH_NO_TRI;
        if (field == RT_MH_NO_TRI) {
            uint32_t nan = RT_TT_NAN_BITS;
            float f;
            __builtin_memcpy(&f, &nan, 4);
            seg.p[0] = seg.p[1] = seg.p[2] = seg.q[0] = seg.q[1] = seg.q[2] = f;
            seg.kind = 2;
        } else {
            const F4 *q = S.tris + 3 * (size_t)field;
            rt_tt_record<true>(q[0], q[1], q[2], t, &seg);
        }
    }
    return seg;
}

/* ---- the argument block ------------------------------------------------------------------------------------------------------- */
/* The scene and work fields carry the names rt_query_args gives them: rt_internal.h's ray_args_scene fills them, rt_stage_scene reads them. */
typedef struct {
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;              /* (not read: the walk has no descend loop of its own) */
    /* the work: query triangles [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    const float *tris;                 /* n x 9 floats: a0, a1, a2 */
    rt_overlap_id *ids;                /* n * k records, [query][rank], 8-byte aligned (not read with k == 0) */
    int32_t *counts;                   /* n, or NULL */
    uint8_t *any;                      /* n, or NULL */
    rt_tri_segment *segments;          /* n * k records, 16-byte aligned, or NULL */
    int32_t k;                         /* ids per query, 0 .. RT_OVERLAP_MAX */
    int32_t any_only;                  /* 1: only `any` is asked for - a query stops at its first overlapping candidate */
} rt_tritri_args;

static_assert(sizeof(rt_tri_segment) == 32, "the kernel stores a segment as two 16-byte units");

#endif
