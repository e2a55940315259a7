/*
 * rt_sweep.h — sphere-cast queries (rt_sweep_spheres[_device], include/rt_amd.h): what the kernel (rt_sweep_kernel.h), the entry points
 * (rt_sweep_capi.cpp) and the host tests (tests/sanitize/sweep_host_check.cpp) share.  Host code; self-contained.
 *
 *  - the arithmetic, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off):
 *    the ball against a point, a scene sphere and the seven features of a triangle record, the winner's record formed again;
 *  - the traversal of one mesh as steps over a small state (rt_sw_walk): the boxes inflated by the ball's radius through rt_multihit.h's
 *    slab test, nearer child first by key, the other pushed with its key, a popped entry skipped when its key is greater than the best so
 *    far; one node or one triangle per step.  The kernel runs one step per lane and round of its wave loop, the host test runs the same
 *    steps in a plain loop;
 *  - nothing is restated: the closest point on a sphere and the candidate comparison are rt_nearest.h's, the slab test rt_multihit.h's.
 *
 *  - the argument block (the launcher is rt_launch.h's rt_launch_sweep).
 *
 * The definition - every formula in the order it is evaluated, and why the key makes pruning exact - is include/rt_amd.h's.
 */
#ifndef RT_SWEEP_H
#define RT_SWEEP_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"
#include "rt_multihit.h"
#include "rt_nearest.h"

#define RT_SW_HD RT_NR_HD

#define RT_SWEEP_MAX_QUERIES RT_NEAREST_MAX_POINTS
#define RT_SW_OVERLAP 0x7ffffffe           /* rt_sw_best.k.object of a ball that touches the scene at the start: its record is the nearest one's */

/* the best candidate so far: rt_nearest.h's (key, object, triangle) with the key K in place of dist2, and what K does not say */
struct rt_sw_best { rt_nr_best k; float t; int32_t feature; };
/* the walk of one mesh: the node or leaf a lane is on, its key (the largest entry distance on the path so far), the entries on its stack,
 * and on a leaf how many of its triangles are done */
struct rt_sw_walk { uint32_t cur; float key; int32_t sp, at; };

/* ---- the arithmetic ------------------------------------------------------------------------------------------------------------ */
RT_SW_HD float rt_sw_floor0(float t) { return t <= 0.0f ? 0.0f : t; }

/* ball(m, rad): a root of |m + t d| = rad - the near one, offered while approaching, or (far) the far one.  The root is taken from the point of
 * the path nearest the sphere's centre, t0 = -b / dd on: there m is about as long as the miss distance, and the discriminant's rounding error
 * scales with that length, not with the distance the ball has come */
RT_SW_HD bool rt_sw_ball(float mx, float my, float mz, const rt_mh_ray &q, float dd, float rad, bool far, float &t)
{
    const float b = rt_nr_dot(mx, my, mz, q.dx, q.dy, q.dz);
    const float t0 = -b / dd;
    const float nx = q.dx * t0 + mx, ny = q.dy * t0 + my, nz = q.dz * t0 + mz;
    const float b2 = rt_nr_dot(nx, ny, nz, q.dx, q.dy, q.dz);
    const float c2 = rt_nr_dot(nx, ny, nz, nx, ny, nz) - rad * rad;
    const float disc = b2 * b2 - dd * c2;
    const float root = sqrtf(disc);
    t = rt_sw_floor0(t0 + (far ? -b2 + root : -b2 - root) / dd);
    return disc >= 0.0f && (far || b < 0.0f);
}

/* a scene sphere (c, R): from outside the near root at R + r, from inside the far root at R - r */
RT_SW_HD bool rt_sw_sphere(float cx, float cy, float cz, float R, const rt_mh_ray &q, float dd, float r, float &t)
{
    const float mx = q.ox - cx, my = q.oy - cy, mz = q.oz - cz;
    const bool outside = rt_nr_dot(mx, my, mz, mx, my, mz) > R * R;
    const float rad = outside ? R + r : R - r;
    return rt_sw_ball(mx, my, mz, q, dd, rad, !outside, t) && (outside || rad > 0.0f);
}

/* an edge (A, e) with m = o - A: the near root of the infinite cylinder, the axial parameter into s.  The root is taken from the foot of the
 * common perpendicular: the path's point nearest the edge's line (t0 on), moved along the edge (by s0) to where it is perpendicular to it -
 * there m is about as long as the distance between the two lines */
RT_SW_HD bool rt_sw_edge(float ex, float ey, float ez, float mx, float my, float mz, const rt_mh_ray &q, float dd, float rr, float &t, float &s)
{
    const float ee = rt_nr_dot(ex, ey, ez, ex, ey, ez), de = rt_nr_dot(q.dx, q.dy, q.dz, ex, ey, ez), me = rt_nr_dot(mx, my, mz, ex, ey, ez);
    const float md = rt_nr_dot(mx, my, mz, q.dx, q.dy, q.dz);
    const float a = ee * dd - de * de, b = ee * md - de * me;
    const float t0 = -b / a;
    const float nx = q.dx * t0 + mx, ny = q.dy * t0 + my, nz = q.dz * t0 + mz;
    const float s0 = rt_nr_dot(nx, ny, nz, ex, ey, ez) / ee;
    const float px = nx - ex * s0, py = ny - ey * s0, pz = nz - ez * s0;
    const float me2 = rt_nr_dot(px, py, pz, ex, ey, ez), md2 = rt_nr_dot(px, py, pz, q.dx, q.dy, q.dz), mm2 = rt_nr_dot(px, py, pz, px, py, pz);
    const float b2 = ee * md2 - de * me2, c2 = ee * (mm2 - rr) - me2 * me2;
    const float disc = b2 * b2 - a * c2;
    const float t1 = (-b2 - sqrtf(disc)) / a;
    t = rt_sw_floor0(t0 + t1);
    s = s0 + (me2 + t1 * de) / ee;
    return a > 0.0f && disc >= 0.0f && b < 0.0f && s >= 0.0f && s <= 1.0f;
}

/* the face: t, the ball's centre then and the contact point; false: not offered, or the point is outside the triangle */
RT_SW_HD bool rt_sw_face(float p0x, float p0y, float p0z, float s1x, float s1y, float s1z, float s2x, float s2y, float s2z, float apx, float apy, float apz,
                         const rt_mh_ray &q, float r, float &t, float pt[3])
{
    const float nx = s1y * s2z - s1z * s2y, ny = s1z * s2x - s1x * s2z, nz = s1x * s2y - s1y * s2x;
    const float nn = rt_nr_dot(nx, ny, nz, nx, ny, nz);
    const float len = sqrtf(nn);
    const float h = rt_nr_dot(apx, apy, apz, nx, ny, nz), dn = rt_nr_dot(q.dx, q.dy, q.dz, nx, ny, nz);
    const bool neg = h < 0.0f;
    const float hs = neg ? -h : h, ds = neg ? -dn : dn;
    const float rl = r * len;
    t = rt_sw_floor0((rl - hs) / ds);
    const float cx = q.dx * t + q.ox, cy = q.dy * t + q.oy, cz = q.dz * t + q.oz;
    const float k = r / len;
    const float ks = neg ? -k : k;
    pt[0] = cx - nx * ks; pt[1] = cy - ny * ks; pt[2] = cz - nz * ks;
    const float wx = pt[0] - p0x, wy = pt[1] - p0y, wz = pt[2] - p0z;
    const float d00 = rt_nr_dot(s1x, s1y, s1z, s1x, s1y, s1z), d01 = rt_nr_dot(s1x, s1y, s1z, s2x, s2y, s2z), d11 = rt_nr_dot(s2x, s2y, s2z, s2x, s2y, s2z);
    const float d20 = rt_nr_dot(wx, wy, wz, s1x, s1y, s1z), d21 = rt_nr_dot(wx, wy, wz, s2x, s2y, s2z);
    const float vn = d11 * d20 - d01 * d21, wn = d00 * d21 - d01 * d20, den = d00 * d11 - d01 * d01;
    return nn > 0.0f && hs >= rl && ds < 0.0f && vn >= 0.0f && wn >= 0.0f && vn + wn <= den;
}

/* a triangle record q0 = (p0.xyz, s1.x), q1 = (s1.yz, s2.xy), q2 = (s2.z, ...): the smallest t over the seven features and which one gave it
 * (the lower index on equal t; a NaN is never smaller); +Inf and -1 when no feature offers one */
template <class F4>
RT_SW_HD float rt_sw_tri(const F4 q0, const F4 q1, const F4 q2, const rt_mh_ray &q, float dd, float r, int32_t &feature)
{
    const float p0x = q0.x, p0y = q0.y, p0z = q0.z, s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
    const float apx = q.ox - p0x, apy = q.oy - p0y, apz = q.oz - p0z;
    const float bpx = apx - s1x, bpy = apy - s1y, bpz = apz - s1z;
    const float cpx = apx - s2x, cpy = apy - s2y, cpz = apz - s2z;
    const float rr = r * r;
    float best = INFINITY, t, s, pt[3];
    int32_t f = -1;
    if (rt_sw_face(p0x, p0y, p0z, s1x, s1y, s1z, s2x, s2y, s2z, apx, apy, apz, q, r, t, pt) && t < best) { best = t; f = 0; }
    if (rt_sw_edge(s1x, s1y, s1z, apx, apy, apz, q, dd, rr, t, s) && t < best) { best = t; f = 1; }
    if (rt_sw_edge(s2x, s2y, s2z, apx, apy, apz, q, dd, rr, t, s) && t < best) { best = t; f = 2; }
    if (rt_sw_edge(s2x - s1x, s2y - s1y, s2z - s1z, bpx, bpy, bpz, q, dd, rr, t, s) && t < best) { best = t; f = 3; }
    if (rt_sw_ball(apx, apy, apz, q, dd, r, false, t) && t < best) { best = t; f = 4; }
    if (rt_sw_ball(bpx, bpy, bpz, q, dd, r, false, t) && t < best) { best = t; f = 5; }
    if (rt_sw_ball(cpx, cpy, cpz, q, dd, r, false, t) && t < best) { best = t; f = 6; }
    feature = f;
    return best;
}

/* the contact point of the winner (t, feature) on its record: the same operations on the same operands as when it was offered */
template <class F4>
RT_SW_HD void rt_sw_tri_point(const F4 q0, const F4 q1, const F4 q2, const rt_mh_ray &q, float dd, float r, int32_t feature, float pt[3])
{
    const float p0x = q0.x, p0y = q0.y, p0z = q0.z, s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
    const float apx = q.ox - p0x, apy = q.oy - p0y, apz = q.oz - p0z;
    float t, s;
    if (feature == 0) {
        (void)rt_sw_face(p0x, p0y, p0z, s1x, s1y, s1z, s2x, s2y, s2z, apx, apy, apz, q, r, t, pt);
    } else if (feature <= 3) {
        const bool third = feature == 3;
        const float ax = third ? p0x + s1x : p0x, ay = third ? p0y + s1y : p0y, az = third ? p0z + s1z : p0z;
        const float ex = feature == 1 ? s1x : third ? s2x - s1x : s2x, ey = feature == 1 ? s1y : third ? s2y - s1y : s2y, ez = feature == 1 ? s1z : third ? s2z - s1z : s2z;
        const float mx = third ? apx - s1x : apx, my = third ? apy - s1y : apy, mz = third ? apz - s1z : apz;
        (void)rt_sw_edge(ex, ey, ez, mx, my, mz, q, dd, r * r, t, s);
        pt[0] = ax + ex * s; pt[1] = ay + ey * s; pt[2] = az + ez * s;
    } else {
        pt[0] = feature == 4 ? p0x : feature == 5 ? p0x + s1x : p0x + s2x;
        pt[1] = feature == 4 ? p0y : feature == 5 ? p0y + s1y : p0y + s2y;
        pt[2] = feature == 4 ? p0z : feature == 5 ? p0z + s1z : p0z + s2z;
    }
}

RT_SW_HD void rt_sw_offer(float key, float t, int32_t feature, int32_t object, int32_t triangle, rt_sw_best &b)
{
    if (rt_nr_better(key, object, triangle, b.k)) { b.k.d2 = key; b.k.object = object; b.k.triangle = triangle; b.t = t; b.feature = feature; }
}

/* The start of a query: the reciprocal direction, sq(d) and the limit as the best key so far.  false: an input that gives a miss. */
RT_SW_HD bool rt_sw_begin(rt_mh_ray &q, float r, bool has_limit, float tmax, float &dd, rt_sw_best &best)
{
    q.ix = 1.0f / q.dx; q.iy = 1.0f / q.dy; q.iz = 1.0f / q.dz;
    dd = rt_nr_dot(q.dx, q.dy, q.dz, q.dx, q.dy, q.dz);
    best.k.d2 = RT_HIT_MISS_T; best.k.object = RT_NR_NONE; best.k.triangle = RT_NR_NONE;
    best.t = RT_HIT_MISS_T; best.feature = -1;
    if (!rt_nr_finite(q.ox) || !rt_nr_finite(q.oy) || !rt_nr_finite(q.oz) || !rt_nr_finite(q.dx) || !rt_nr_finite(q.dy) || !rt_nr_finite(q.dz)) return false;
    if (q.dx == 0.0f && q.dy == 0.0f && q.dz == 0.0f) return false;
    if (!rt_nr_finite(r) || !(r >= 0.0f)) return false;
    if (has_limit) {
        if (!(tmax > 0.0f)) return false;
        best.k.d2 = tmax < RT_HIT_MISS_T ? tmax : RT_HIT_MISS_T;
    }
    return true;
}

/* the objects that are not meshes, in list order, from the object table */
template <class F4>
RT_SW_HD void rt_sw_simple(const rt_nr_scene<F4> &S, int32_t num_objects, const rt_mh_ray &q, float dd, float r, rt_sw_best &best)
{
#pragma unroll 1
    for (int32_t i = 0; i < num_objects; i++) {
        const F4 ob0 = S.objtab[3 * i];
        const int32_t type = RT_MH_UNIFORM((int32_t)rt_nr_bits(ob0.x)), prim = RT_MH_UNIFORM((int32_t)rt_nr_bits(ob0.y));
        if (type == RT_OBJ_MESH) continue;
        if (type == RT_OBJ_SPHERE) {
            const F4 ob1 = S.objtab[3 * i + 1];
            float t;
            if (rt_sw_sphere(ob1.x, ob1.y, ob1.z, ob1.w, q, dd, r, t)) rt_sw_offer(t, t, -1, i, -1, best);
            continue;
        }
        const int32_t count = rt_nr_object_tris(type);
#pragma unroll 1
        for (int32_t k = 0; k < count; k++) {
            const F4 *tr = S.tris + 3 * (size_t)(prim + k);
            int32_t feature;
            const float t = rt_sw_tri(tr[0], tr[1], tr[2], q, dd, r, feature);
            rt_sw_offer(t, t, feature, i, prim + k, best);
        }
    }
}

/* ---- the traversal of one mesh --------------------------------------------------------------------------------------------------
 * CHAIN bits of a reference are masked off: they stand for a box tested twice, which changes nothing here. */
/* the box (lo, hi) inflated by r through the slab test */
RT_SW_HD bool rt_sw_box(float lox, float loy, float loz, float hix, float hiy, float hiz, float r, const rt_mh_ray &q, float &tmin)
{
    return rt_mh_box(lox - r, loy - r, loz - r, hix + r, hiy + r, hiz + r, q, tmin);
}

/* (m0, m1): the mesh's pair of the `meshes` section.  false: the ball's path misses the inflated root box, or enters it beyond the best key */
template <class F4>
RT_SW_HD bool rt_sw_mesh_begin(const F4 m0, const F4 m1, const rt_mh_ray &q, float r, const rt_sw_best &best, rt_sw_walk &w)
{
    float key;
    if (!rt_sw_box(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, r, q, key) || !(key <= best.k.d2)) return false;
    w.cur = rt_nr_bits(m1.z) & ~RT_REF_CHAIN;
    w.key = key;
    w.sp = 0;
    w.at = 0;
    return true;
}

/* One step: on an internal node, the two children's inflated boxes and keys, the child with the larger key pushed and the other entered (each
 * only if the path enters its box and its key is not greater than the best so far); on a leaf, its next triangle.  A lane with nowhere to go
 * on pops until it takes an entry.  false: the mesh is finished.  `stack` is the lane's own, entry s at stack[s * STRIDE] (the kernels'
 * [entry][thread] layout); it holds at most one entry per internal node on the path, the depth the scene's stack is sized for. */
template <int STRIDE, class F4>
RT_SW_HD bool rt_sw_step(const rt_nr_scene<F4> &S, rt_nr_entry *stack, int32_t object, const rt_mh_ray &q, float dd, float r, rt_sw_best &best, rt_sw_walk &w)
{
    if (!(w.cur & RT_REF_LEAF)) {
        const F4 *n = S.nodes + 4 * (size_t)(w.cur & RT_REF_NODE_MASK);
        const F4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
        float tl, tr;
        const bool hl = rt_sw_box(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r, q, tl);
        const bool hr = rt_sw_box(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r, q, tr);
        const float kl = tl < w.key ? w.key : tl, kr = tr < w.key ? w.key : tr;
        const bool el = hl && kl <= best.k.d2, er = hr && kr <= best.k.d2;
        const uint32_t lref = rt_nr_bits(q3.x) & ~RT_REF_CHAIN, rref = rt_nr_bits(q3.y) & ~RT_REF_CHAIN;
        const bool l_first = kl <= kr;
        const float near_key = l_first ? kl : kr, far_key = l_first ? kr : kl;
        const uint32_t near_ref = l_first ? lref : rref, far_ref = l_first ? rref : lref;
        const bool near_ok = l_first ? el : er, far_ok = l_first ? er : el;
        if (near_ok && far_ok) {
            rt_nr_entry e;
            e.key = far_key; e.ref = far_ref;
            stack[(size_t)w.sp * STRIDE] = e;
            w.sp++;
        }
        w.at = 0;
        if (near_ok) { w.cur = near_ref; w.key = near_key; return true; }
        if (far_ok) { w.cur = far_ref; w.key = far_key; return true; }
    } else {
        const int32_t start = (int32_t)(w.cur & RT_REF_START_MASK), count = (int32_t)((w.cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        if (w.at < count) {
            const F4 *tr = S.tris + 3 * (size_t)(start + w.at);
            int32_t feature;
            const float t = rt_sw_tri(tr[0], tr[1], tr[2], q, dd, r, feature);
            rt_sw_offer(t < w.key ? w.key : t, t, feature, object, start + w.at, best);
            w.at++;
            if (w.at < count) return true;
        }
    }
    while (w.sp > 0) {
        w.sp--;
        const rt_nr_entry e = stack[(size_t)w.sp * STRIDE];
        if (e.key <= best.k.d2) { w.cur = e.ref; w.key = e.key; w.at = 0; return true; }
    }
    return false;
}

/* the record of a finished query: a miss, the start overlap (`near`: the nearest-surface record of o under the limit r) or the winner, whose
 * contact point is formed again from its record */
template <class F4>
RT_SW_HD void rt_sw_record(const rt_nr_scene<F4> &S, const rt_mh_ray &q, float dd, float r, const rt_sw_best &best, const rt_nearest *near, rt_sweep &out)
{
    out.reserved = 0;
    out.overlap = 0;
    out.feature = -1;
    if (best.k.object == RT_NR_NONE) {
        out.t = RT_HIT_MISS_T;
        out.centre[0] = out.centre[1] = out.centre[2] = 0.0f;
        out.point[0] = out.point[1] = out.point[2] = 0.0f;
        out.object = out.triangle = -1;
        return;
    }
    if (best.k.object == RT_SW_OVERLAP) {
        out.t = 0.0f;
        out.centre[0] = q.ox; out.centre[1] = q.oy; out.centre[2] = q.oz;
        out.point[0] = near->point[0]; out.point[1] = near->point[1]; out.point[2] = near->point[2];
        out.object = near->object;
        out.triangle = near->triangle;
        out.overlap = 1;
        return;
    }
    out.t = best.t;
    out.centre[0] = q.dx * best.t + q.ox; out.centre[1] = q.dy * best.t + q.oy; out.centre[2] = q.dz * best.t + q.oz;
    if (best.k.triangle < 0) {
        const F4 ob1 = S.objtab[3 * best.k.object + 1];
        (void)rt_nr_sphere(ob1.x, ob1.y, ob1.z, ob1.w, out.centre[0], out.centre[1], out.centre[2], out.point);
    } else {
        const F4 *tr = S.tris + 3 * (size_t)best.k.triangle;
        rt_sw_tri_point(tr[0], tr[1], tr[2], q, dd, r, best.feature, out.point);
    }
    out.object = best.k.object;
    out.triangle = best.k.triangle;
    out.feature = best.feature;
}

/* ---- the argument block ------------------------------------------------------------------------------------------------------- */
/* The scene and work fields carry the names rt_query_args gives them: rt_internal.h's ray_args_scene fills them, rt_stage_scene reads them. */
typedef struct {
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;              /* (not read: the walk has no descend loop of its own) */
    /* the work: balls [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    const float *origins, *directions; /* n x 3 floats each */
    const float *radius;               /* n floats */
    const float *tmax;                 /* n floats, or NULL */
    const rt_nearest *nearest;         /* n records: the nearest-surface answers of the origins under the radii as limits */
    rt_sweep *out;                     /* n records, 16-byte aligned */
} rt_sweep_args;

static_assert(sizeof(rt_sweep) == 3 * sizeof(rt_f4) && sizeof(rt_nearest) == 2 * sizeof(rt_f4), "the kernel reads and stores the records in 16-byte units");

#endif
