/*
 * rt_nearest.h — nearest-surface queries (rt_nearest_points[_device], include/rt_amd.h): what the kernel (rt_nearest_kernel.h), the entry
 * points (rt_nearest_capi.cpp) and the host tests (tests/sanitize/nearest_host_check.cpp) share.  Host code; self-contained.
 *
 *  - the arithmetic, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off):
 *    the box distance, the sphere, the point-triangle test, the comparison of two candidates, the limit, the record;
 *  - the traversal of one mesh as steps over a small state (rt_nr_walk): nearest child first by path value, the farther child pushed
 *    with its path value, a popped entry skipped when its key is greater than the best so far.  The kernel runs one step per lane and
 *    round of its wave loop, the host test runs the same steps in a plain loop;
 *  - the argument block (the launcher is rt_launch.h's rt_launch_nearest).
 *
 * The definition - every formula in the order it is evaluated, and why the path value makes pruning exact - is include/rt_amd.h's.
 */
#ifndef RT_NEAREST_H
#define RT_NEAREST_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"

#if defined(__HIPCC__)
#define RT_NR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT_NR_HD inline
#endif

#define RT_NEAREST_MAX_POINTS (1 << 30)    /* points of one call (point ids and the chunk counter are 32-bit) */
#define RT_NR_NONE 0x7fffffff              /* the best so far before any candidate: loses every tie */

/* the best candidate so far: (dist2, object, triangle), compared in that order.  It starts as (limit^2, NONE, NONE), so a candidate at
 * exactly the limit wins and one beyond it does not */
struct rt_nr_best { float d2; int32_t object, triangle; };
/* one pending subtree of a lane's stack: 8 bytes, one LDS access */
struct __attribute__((aligned(8))) rt_nr_entry { float key; uint32_t ref; };
/* the walk of one mesh: the node or leaf a lane is on, its path value, the entries on its stack */
struct rt_nr_walk { uint32_t cur; float key; int32_t sp; };
/* the scene sections; F4 is a 16-byte unit with members x, y, z, w (rt_f4 on the host, the kernels' v4f on the device) */
template <class F4> struct rt_nr_scene { const F4 *nodes, *tris, *meshes, *objtab; };

RT_NR_HD uint32_t rt_nr_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_NR_HD bool rt_nr_finite(float f) { return (rt_nr_bits(f) & 0x7f800000u) != 0x7f800000u; }

/* ---- the arithmetic ------------------------------------------------------------------------------------------------------------ */
RT_NR_HD float rt_nr_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* the box distance: no operand is a NaN here (the point is finite, a box's planes are), and a zero's sign is squared away */
RT_NR_HD float rt_nr_box_d2(float lox, float loy, float loz, float hix, float hiy, float hiz, float px, float py, float pz)
{
    const float ex = fmaxf(fmaxf(lox - px, px - hix), 0.0f);
    const float ey = fmaxf(fmaxf(loy - py, py - hiy), 0.0f);
    const float ez = fmaxf(fmaxf(loz - pz, pz - hiz), 0.0f);
    return rt_nr_dot(ex, ey, ez, ex, ey, ez);
}

/* a sphere (c, r): dist2, and the closest point into pt */
RT_NR_HD float rt_nr_sphere(float cx, float cy, float cz, float r, float px, float py, float pz, float pt[3])
{
    const float vx = px - cx, vy = py - cy, vz = pz - cz;
    const float l = sqrtf(rt_nr_dot(vx, vy, vz, vx, vy, vz));
    const float s = l - r;
    const float k = r / l;
    const bool centre = l == 0.0f;
    pt[0] = centre ? cx + r : cx + vx * k;
    pt[1] = centre ? cy + 0.0f : cy + vy * k;
    pt[2] = centre ? cz + 0.0f : cz + vz * k;
    return s * s;
}

/* a triangle record q0 = (p0.xyz, s1.x), q1 = (s1.yz, s2.xy), q2 = (s2.z, ...): dist2, and the closest point into pt.  Every region's
 * barycentrics are formed and the first region that holds is selected (the later assignment overrides the earlier): no branch, the
 * same values as the chain of tests. */
template <class F4>
RT_NR_HD float rt_nr_tri(const F4 q0, const F4 q1, const F4 q2, float px, float py, float pz, float pt[3])
{
    const float ax = q0.x, ay = q0.y, az = q0.z, bx = q0.w, by = q1.x, bz = q1.y, cx = q1.z, cy = q1.w, cz = q2.x;   /* p0, s1, s2 */
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float bpx = apx - bx, bpy = apy - by, bpz = apz - bz;
    const float cpx = apx - cx, cpy = apy - cy, cpz = apz - cz;
    const float d1 = rt_nr_dot(bx, by, bz, apx, apy, apz), d2 = rt_nr_dot(cx, cy, cz, apx, apy, apz);
    const float d3 = rt_nr_dot(bx, by, bz, bpx, bpy, bpz), d4 = rt_nr_dot(cx, cy, cz, bpx, bpy, bpz);
    const float d5 = rt_nr_dot(bx, by, bz, cpx, cpy, cpz), d6 = rt_nr_dot(cx, cy, cz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float k = 1.0f / ((va + vb) + vc);
    float v = vb * k, w = vc * k;
    const float e = d4 - d3, f = d5 - d6;
    if (va <= 0.0f && e >= 0.0f && f >= 0.0f) { w = e / (e + f); v = 1.0f - w; }
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2 / (d2 - d6); }
    if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; }
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; }
    if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; }
    if (d1 <= 0.0f && d2 <= 0.0f) { v = 0.0f; w = 0.0f; }
    const float qx = bx * v + cx * w, qy = by * v + cy * w, qz = bz * v + cz * w;
    pt[0] = ax + qx; pt[1] = ay + qy; pt[2] = az + qz;
    const float rx = apx - qx, ry = apy - qy, rz = apz - qz;
    return rt_nr_dot(rx, ry, rz, rx, ry, rz);
}

/* a mesh triangle's dist2 under its path value: B where dist2 < B (a NaN stays a NaN) */
RT_NR_HD float rt_nr_clamp(float d2, float path) { return d2 < path ? path : d2; }
/* a child's path value: the larger of its parent's and its own box distance (neither is a NaN) */
RT_NR_HD float rt_nr_path(float parent, float box) { return box < parent ? parent : box; }

RT_NR_HD bool rt_nr_better(float d2, int32_t object, int32_t triangle, const rt_nr_best &b)
{
    return d2 < b.d2 || (d2 == b.d2 && (object < b.object || (object == b.object && triangle < b.triangle)));
}
RT_NR_HD void rt_nr_offer(float d2, int32_t object, int32_t triangle, rt_nr_best &b)
{
    if (rt_nr_better(d2, object, triangle, b)) { b.d2 = d2; b.object = object; b.triangle = triangle; }
}

/* the start of a point's query: false for a point or a limit that gives a miss.  has_limit == false, or +Inf: unbounded */
RT_NR_HD bool rt_nr_begin(float px, float py, float pz, bool has_limit, float max_dist, rt_nr_best &best)
{
    best.d2 = INFINITY; best.object = RT_NR_NONE; best.triangle = RT_NR_NONE;
    if (!rt_nr_finite(px) || !rt_nr_finite(py) || !rt_nr_finite(pz)) return false;
    if (has_limit) {
        if (!(max_dist >= 0.0f)) return false;
        best.d2 = max_dist * max_dist;
    }
    return true;
}

/* how many triangle records an object of the list that is neither a sphere nor a mesh holds from its prim_start on */
RT_NR_HD int32_t rt_nr_object_tris(int32_t type) { return type == RT_OBJ_TRIANGLE ? 1 : type == RT_OBJ_CUBOID ? 12 : 2; }

/* the objects that are not meshes, in list order, from the object table (rt_object: type, prim_start, ..., v[0..3] = c, r) */
template <class F4>
RT_NR_HD void rt_nr_simple(const rt_nr_scene<F4> &S, int32_t num_objects, float px, float py, float pz, rt_nr_best &best)
{
    float pt[3];
    for (int32_t i = 0; i < num_objects; i++) {
        const F4 ob0 = S.objtab[3 * i];
        const int32_t type = (int32_t)rt_nr_bits(ob0.x), prim = (int32_t)rt_nr_bits(ob0.y);
        if (type == RT_OBJ_MESH) continue;
        if (type == RT_OBJ_SPHERE) {
            const F4 ob1 = S.objtab[3 * i + 1];
            rt_nr_offer(rt_nr_sphere(ob1.x, ob1.y, ob1.z, ob1.w, px, py, pz, pt), i, -1, best);
            continue;
        }
        const int32_t count = rt_nr_object_tris(type);
        for (int32_t k = 0; k < count; k++) {
            const F4 *t = S.tris + 3 * (prim + k);
            rt_nr_offer(rt_nr_tri(t[0], t[1], t[2], px, py, pz, pt), i, prim + k, best);
        }
    }
}

/* ---- the traversal of one mesh --------------------------------------------------------------------------------------------------
 * CHAIN bits of a reference are masked off: they stand for a box tested twice, which changes nothing here. */
/* (m0, m1): the mesh's pair of the `meshes` section.  false: the whole mesh is farther than the best so far */
template <class F4>
RT_NR_HD bool rt_nr_mesh_begin(const F4 m0, const F4 m1, float px, float py, float pz, const rt_nr_best &best, rt_nr_walk &w)
{
    const float key = rt_nr_box_d2(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, px, py, pz);
    if (!(key <= best.d2)) return false;
    w.cur = rt_nr_bits(m1.z) & ~RT_REF_CHAIN;
    w.key = key;
    w.sp = 0;
    return true;
}

/* One step: on an internal node, the two children's path values, the farther one pushed and the nearer one entered (each only if its key
 * is not greater than the best so far); on a leaf, its triangles.  A lane with nowhere to go on pops until it takes an entry.  false:
 * the mesh is finished.  `stack` is the lane's own, entry s at stack[s * STRIDE] (the kernels' [entry][thread] layout); it holds at most
 * one entry per internal node on the path, the depth the scene's stack is sized for. */
template <int STRIDE, class F4>
RT_NR_HD bool rt_nr_step(const rt_nr_scene<F4> &S, rt_nr_entry *stack, int32_t object, float px, float py, float pz, rt_nr_best &best, rt_nr_walk &w)
{
    if (!(w.cur & RT_REF_LEAF)) {
        const F4 *n = S.nodes + 4 * (size_t)(w.cur & RT_REF_NODE_MASK);
        const F4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
        const float kl = rt_nr_path(w.key, rt_nr_box_d2(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, px, py, pz));
        const float kr = rt_nr_path(w.key, rt_nr_box_d2(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, px, py, pz));
        const uint32_t lref = rt_nr_bits(q3.x) & ~RT_REF_CHAIN, rref = rt_nr_bits(q3.y) & ~RT_REF_CHAIN;
        const bool l_first = kl <= kr;
        const float near_key = l_first ? kl : kr, far_key = l_first ? kr : kl;
        const uint32_t near_ref = l_first ? lref : rref, far_ref = l_first ? rref : lref;
        if (far_key <= best.d2) {
            rt_nr_entry e;
            e.key = far_key; e.ref = far_ref;
            stack[(size_t)w.sp * STRIDE] = e;
            w.sp++;
        }
        if (near_key <= best.d2) { w.cur = near_ref; w.key = near_key; return true; }
    } else {
        const int32_t start = (int32_t)(w.cur & RT_REF_START_MASK), count = (int32_t)((w.cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        float pt[3];
        for (int32_t k = 0; k < count; k++) {
            const F4 *t = S.tris + 3 * (size_t)(start + k);
            rt_nr_offer(rt_nr_clamp(rt_nr_tri(t[0], t[1], t[2], px, py, pz, pt), w.key), object, start + k, best);
        }
    }
    while (w.sp > 0) {
        w.sp--;
        const rt_nr_entry e = stack[(size_t)w.sp * STRIDE];
        if (e.key <= best.d2) { w.cur = e.ref; w.key = e.key; return true; }
    }
    return false;
}

/* the record of a finished query (words: distance, distance2, point, object, triangle, reserved): the winner's point is formed again from
 * its record - the same operations on the same operands as when it was offered */
template <class F4>
RT_NR_HD void rt_nr_record(const rt_nr_scene<F4> &S, float px, float py, float pz, const rt_nr_best &best, rt_nearest &out)
{
    out.reserved = 0;
    if (best.object == RT_NR_NONE) {
        out.distance = out.distance2 = RT_HIT_MISS_T;
        out.point[0] = out.point[1] = out.point[2] = 0.0f;
        out.object = out.triangle = -1;
        return;
    }
    if (best.triangle < 0) {
        const F4 ob1 = S.objtab[3 * best.object + 1];
        (void)rt_nr_sphere(ob1.x, ob1.y, ob1.z, ob1.w, px, py, pz, out.point);
    } else {
        const F4 *t = S.tris + 3 * (size_t)best.triangle;
        (void)rt_nr_tri(t[0], t[1], t[2], px, py, pz, out.point);
    }
    out.distance = sqrtf(best.d2);
    out.distance2 = best.d2;
    out.object = best.object;
    out.triangle = best.triangle;
}

/* ---- the argument block ------------------------------------------------------------------------------------------------------- */
/* The scene and work fields carry the names rt_query_args gives them: rt_internal.h's ray_args_scene fills them, rt_stage_scene reads them. */
typedef struct {
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;              /* (not read: the walk has no descend loop of its own) */
    /* the work: points [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    const float *points;               /* n x 3 floats */
    const float *max_dist;             /* n floats, or NULL: unbounded */
    rt_nearest *out;                   /* n records, 16-byte aligned */
} rt_nearest_args;

#endif
