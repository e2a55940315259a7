/*
 * rt_overlap.h — box-overlap queries (rt_overlap_boxes[_device], include/rt_amd.h): what the kernel (rt_overlap_kernel.h), the entry
 * points (rt_overlap_capi.cpp) and the host tests (tests/sanitize/overlap_host_check.cpp) share.  Host code; self-contained.
 *
 *  - the tests, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off): a
 *    box's validity, centre and half extents, the sphere's two distances, the thirteen separating axes of a triangle record, the compare
 *    of two boxes;
 *  - the per-box buffer of the k lowest ids (rt_ov_buf) and its insert: eight statically indexed 32-bit slots, compare and select;
 *  - the traversal of one mesh as steps over a small state (rt_ov_walk): an overlapping child entered, its sibling pushed only when it
 *    overlaps too, one node or ONE triangle per step.  The kernel runs one step per lane and round of its wave loop, the host test runs
 *    the same steps in a plain loop.
 *
 *  - the argument block (the launcher is rt_launch.h's rt_launch_overlap).
 *
 * The definition - every formula in the order it is evaluated, and why compares alone make pruning exact - is include/rt_amd.h's.
 */
#ifndef RT_OVERLAP_H
#define RT_OVERLAP_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"
#include "rt_multihit.h"        /* RT_MH_MAX_OBJECTS, RT_MH_NO_TRI, RT_MH_UNIFORM */

#if defined(__HIPCC__)
#define RT_OV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT_OV_HD inline
#endif

#define RT_OVERLAP_MAX_BOXES (1 << 30)     /* boxes of one call (box ids and the chunk counter are 32-bit) */
/* A candidate's identity in one word, ordered as the output asks (ascending word: lower object first, then lower triangle): bits 31..20
 * hold the object, bits 19..0 the flattened triangle index, or RT_MH_NO_TRI (all ones) for a sphere - an object offers a sphere or
 * triangles, never both, so the field's place in the order is never asked.  An empty slot is all ones: below no word, and the one word
 * it equals (a sphere that is object 4095) is the largest there is, so it lands where the empty slot already stands: the count, not the
 * slot's value, says how many slots hold an answer. */
#define RT_OV_EMPTY 0xffffffffu

/* the query box: as given, and its centre and half extents */
struct rt_ov_box { float lox, loy, loz, hix, hiy, hiz, cx, cy, cz, hx, hy, hz; };
/* One box's k lowest ids, ascending in all eight slots whatever k is (the first k are the answer), and `total`: every candidate that overlaps */
struct rt_ov_buf { uint32_t id[RT_OVERLAP_MAX]; uint32_t total; };
/* the walk of one mesh: the node or leaf a lane is on, the entries on its stack, and on a leaf how many of its triangles are done */
struct rt_ov_walk { uint32_t cur; int32_t sp, at; };
/* the scene sections; F4 is a 16-byte unit with members x, y, z, w (rt_f4 on the host, the kernels' v4f on the device) */
template <class F4> struct rt_ov_scene { const F4 *nodes, *tris, *meshes, *objtab; };

RT_OV_HD uint32_t rt_ov_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_OV_HD bool rt_ov_finite(float f) { return (rt_ov_bits(f) & 0x7f800000u) != 0x7f800000u; }

/* ---- the tests ----------------------------------------------------------------------------------------------------------------- */
/* the start of a box's query: false for a box that overlaps nothing (a component that is not finite, lo > hi on an axis) */
RT_OV_HD bool rt_ov_begin(rt_ov_box &b)
{
    if (!rt_ov_finite(b.lox) || !rt_ov_finite(b.loy) || !rt_ov_finite(b.loz) || !rt_ov_finite(b.hix) || !rt_ov_finite(b.hiy) || !rt_ov_finite(b.hiz)) return false;
    if (!(b.lox <= b.hix && b.loy <= b.hiy && b.loz <= b.hiz)) return false;
    b.cx = b.lox * 0.5f + b.hix * 0.5f; b.cy = b.loy * 0.5f + b.hiy * 0.5f; b.cz = b.loz * 0.5f + b.hiz * 0.5f;
    b.hx = b.hix * 0.5f - b.lox * 0.5f; b.hy = b.hiy * 0.5f - b.loy * 0.5f; b.hz = b.hiz * 0.5f - b.loz * 0.5f;
    return true;
}

/* two closed boxes by compares alone: the path rule of a mesh, the root box and every child box */
RT_OV_HD bool rt_ov_boxes(float nlox, float nloy, float nloz, float nhix, float nhiy, float nhiz, const rt_ov_box &b)
{
    return nlox <= b.hix && b.lox <= nhix && nloy <= b.hiy && b.loy <= nhiy && nloz <= b.hiz && b.loz <= nhiz;
}

/* a sphere (c, R) as a surface: the box's nearest point no farther than R, its farthest no nearer */
RT_OV_HD bool rt_ov_sphere(float cx, float cy, float cz, float R, const rt_ov_box &b)
{
    const float ex = fmaxf(fmaxf(b.lox - cx, cx - b.hix), 0.0f), ey = fmaxf(fmaxf(b.loy - cy, cy - b.hiy), 0.0f), ez = fmaxf(fmaxf(b.loz - cz, cz - b.hiz), 0.0f);
    const float gx = fmaxf(cx - b.lox, b.hix - cx), gy = fmaxf(cy - b.loy, b.hiy - cy), gz = fmaxf(cz - b.loz, b.hiz - cz);
    const float dmin2 = (ex * ex + ey * ey) + ez * ez;
    const float dmax2 = (gx * gx + gy * gy) + gz * gz;
    const float rr = R * R;
    return dmin2 <= rr && dmax2 >= rr;
}

/* one edge axis: the three projections against the radius.  true: the axis separates */
RT_OV_HD bool rt_ov_axis(float p0, float p1, float p2, float rad)
{
    const float neg = -rad;
    return ((p0 > rad) & (p1 > rad) & (p2 > rad)) | ((p0 < neg) & (p1 < neg) & (p2 < neg));
}

/* the nine edge axes' three of one edge f, on the vertices v0, v1, v2 taken from the centre.  true: one of them separates */
RT_OV_HD bool rt_ov_edge(float fx, float fy, float fz, float v0x, float v0y, float v0z, float v1x, float v1y, float v1z, float v2x, float v2y, float v2z,
                         const rt_ov_box &b)
{
    const float ax = fabsf(fx), ay = fabsf(fy), az = fabsf(fz);
    const bool sx = rt_ov_axis(v0z * fy - v0y * fz, v1z * fy - v1y * fz, v2z * fy - v2y * fz, b.hy * az + b.hz * ay);
    const bool sy = rt_ov_axis(v0x * fz - v0z * fx, v1x * fz - v1z * fx, v2x * fz - v2z * fx, b.hx * az + b.hz * ax);
    const bool sz = rt_ov_axis(v0y * fx - v0x * fy, v1y * fx - v1x * fy, v2y * fx - v2x * fy, b.hx * ay + b.hy * ax);
    return sx | sy | sz;
}

/* a triangle record q0 = (p0.xyz, s1.x), q1 = (s1.yz, s2.xy), q2 = (s2.z, ...): true when none of the thirteen axes separates.  The
 * verdicts have no side effects.  The box's own axes, compares alone, are taken first and leave at once where one separates (most
 * triangles a leaf holds for a small box); the other ten are formed without a branch between them: ten nested early exits are ten lane
 * masks in scalar registers across the kernel's wave loop, which then spills them. */
template <class F4>
RT_OV_HD bool rt_ov_tri(const F4 q0, const F4 q1, const F4 q2, const rt_ov_box &b)
{
    const float ax = q0.x, ay = q0.y, az = q0.z, s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
    const float bx = ax + s1x, by = ay + s1y, bz = az + s1z, cx = ax + s2x, cy = ay + s2y, cz = az + s2z;
    /* the box's own axes: compares on lo and hi themselves */
    const bool sx = ((ax > b.hix) & (bx > b.hix) & (cx > b.hix)) | ((ax < b.lox) & (bx < b.lox) & (cx < b.lox));
    const bool sy = ((ay > b.hiy) & (by > b.hiy) & (cy > b.hiy)) | ((ay < b.loy) & (by < b.loy) & (cy < b.loy));
    const bool sz = ((az > b.hiz) & (bz > b.hiz) & (cz > b.hiz)) | ((az < b.loz) & (bz < b.loz) & (cz < b.loz));
    if (sx | sy | sz) return false;
    const float v0x = ax - b.cx, v0y = ay - b.cy, v0z = az - b.cz;
    const float v1x = bx - b.cx, v1y = by - b.cy, v1z = bz - b.cz;
    const float v2x = cx - b.cx, v2y = cy - b.cy, v2z = cz - b.cz;
    /* the triangle's plane */
    const float nx = s1y * s2z - s1z * s2y, ny = s1z * s2x - s1x * s2z, nz = s1x * s2y - s1y * s2x;
    const float d = (nx * v0x + ny * v0y) + nz * v0z;
    const float r = (b.hx * fabsf(nx) + b.hy * fabsf(ny)) + b.hz * fabsf(nz);
    const bool sp = (d > r) | (d < -r);
    /* the nine cross products of an edge and a box axis */
    const bool s0 = rt_ov_edge(s1x, s1y, s1z, v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, b);
    const bool s1 = rt_ov_edge(s2x - s1x, s2y - s1y, s2z - s1z, v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, b);
    const bool s2 = rt_ov_edge(-s2x, -s2y, -s2z, v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, b);
    return !(sp | s0 | s1 | s2);
}

/* ---- the buffer ---------------------------------------------------------------------------------------------------------------- */
RT_OV_HD uint32_t rt_ov_word(int32_t object, uint32_t tri_field) { return ((uint32_t)object << 20) | tri_field; }
RT_OV_HD int32_t rt_ov_word_object(uint32_t w) { return (int32_t)(w >> 20); }
RT_OV_HD int32_t rt_ov_word_triangle(uint32_t w) { const uint32_t f = w & RT_MH_NO_TRI; return f == RT_MH_NO_TRI ? -1 : (int32_t)f; }

RT_OV_HD void rt_ov_clear(rt_ov_buf &b)
{
#pragma unroll
    for (int j = 0; j < RT_OVERLAP_MAX; j++) b.id[j] = RT_OV_EMPTY;
    b.total = 0u;
}

/* The insert (rt_mh_insert on 32-bit words): the word goes to its place among the ascending slots and the last one falls out.  Every slot
 * is a select between itself, its neighbour in front and the newcomer: no index is computed, the slots stay in registers. */
RT_OV_HD void rt_ov_insert(rt_ov_buf &b, uint32_t word)
{
    bool below = word < b.id[RT_OVERLAP_MAX - 1];
#pragma unroll
    for (int j = RT_OVERLAP_MAX - 1; j > 0; j--) {
        const bool below_prev = word < b.id[j - 1];
        b.id[j] = below_prev ? b.id[j - 1] : (below ? word : b.id[j]);
        below = below_prev;
    }
    b.id[0] = below ? word : b.id[0];
}

/* a tested candidate: counted, and kept among the lowest when anything is kept.  No branch around the insert: a candidate that does not
 * overlap is inserted as the all-ones word, which is below no slot.  k is the same for every box of a call */
RT_OV_HD void rt_ov_offer(rt_ov_buf &b, int32_t k, bool overlaps, int32_t object, uint32_t tri_field)
{
    b.total += overlaps ? 1u : 0u;
    if (k > 0) rt_ov_insert(b, overlaps ? rt_ov_word(object, tri_field) : RT_OV_EMPTY);
}

/* how many triangle records an object of the list that is neither a sphere nor a mesh holds from its prim_start on */
RT_OV_HD int32_t rt_ov_object_tris(int32_t type) { return type == RT_OBJ_TRIANGLE ? 1 : type == RT_OBJ_CUBOID ? 12 : 2; }

/* The objects that are not meshes, in list order, from the object table (rt_object: type, prim_start, ..., v[0..3] = c, r): one place
 * where a candidate is offered.  any_only: the walk over the list ends at the first candidate that overlaps. */
template <class F4>
RT_OV_HD void rt_ov_simple(const rt_ov_scene<F4> &S, int32_t num_objects, const rt_ov_box &box, int32_t k, bool any_only, rt_ov_buf &b)
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
                hit = rt_ov_sphere(ob1.x, ob1.y, ob1.z, ob1.w, box);
            } else {
                const F4 *q = S.tris + 3 * (size_t)(prim + fc);
                hit = rt_ov_tri(q[0], q[1], q[2], box);
                field = (uint32_t)(prim + fc);
            }
            rt_ov_offer(b, k, hit, i, field);
        }
        if (any_only && b.total > 0u) return;
    }
}

/* ---- the traversal of one mesh --------------------------------------------------------------------------------------------------
 * CHAIN bits of a reference are masked off: they stand for a box tested twice, which changes nothing here. */
/* (m0, m1): the mesh's pair of the `meshes` section.  false: the root box does not overlap the query box */
template <class F4>
RT_OV_HD bool rt_ov_mesh_begin(const F4 m0, const F4 m1, const rt_ov_box &box, rt_ov_walk &w)
{
    if (!rt_ov_boxes(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, box)) return false;
    w.cur = rt_ov_bits(m1.z) & ~RT_REF_CHAIN;
    w.sp = 0;
    w.at = 0;
    return true;
}

/* One step: on an internal node, the two children's boxes compared with the query box, the left one entered where it overlaps (else the
 * right), the right pushed only when both do; on a leaf, its next triangle (one per step: lanes in leaves and lanes at nodes keep each
 * other busy, and the slots are changed in straight-line code).  A lane with nowhere to go on pops.  false: the mesh is finished.
 * `stack` is the lane's own, entry s at stack[s * STRIDE] (the kernels' [entry][thread] layout, one 8-byte unit per entry of which the
 * first word is used); it holds at most one entry per internal node on the path, the depth the scene's stack is sized for. */
template <int STRIDE, class F4>
RT_OV_HD bool rt_ov_step(const rt_ov_scene<F4> &S, uint32_t *stack, int32_t object, const rt_ov_box &box, int32_t k, rt_ov_buf &b, rt_ov_walk &w)
{
    if (!(w.cur & RT_REF_LEAF)) {
        const F4 *n = S.nodes + 4 * (size_t)(w.cur & RT_REF_NODE_MASK);
        const F4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
        const bool ol = rt_ov_boxes(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, box);
        const bool orr = rt_ov_boxes(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, box);
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
            rt_ov_offer(b, k, rt_ov_tri(q[0], q[1], q[2], box), object, (uint32_t)(start + w.at));
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

/* rank q of a finished box (q is static where the caller unrolls): the id, or {-1, -1} past the count */
RT_OV_HD rt_overlap_id rt_ov_id(uint32_t word, bool held)
{
    rt_overlap_id r;
    r.object = held ? rt_ov_word_object(word) : -1;
    r.triangle = held ? rt_ov_word_triangle(word) : -1;
    return r;
}

/* ---- the argument block ------------------------------------------------------------------------------------------------------- */
/* The scene and work fields carry the names rt_query_args gives them: rt_internal.h's ray_args_scene fills them, rt_stage_scene reads them. */
typedef struct {
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;              /* (not read: the walk has no descend loop of its own) */
    /* the work: boxes [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    const float *lo, *hi;              /* n x 3 floats each */
    rt_overlap_id *ids;                /* n * k records, [box][rank], 8-byte aligned (not read with k == 0) */
    int32_t *counts;                   /* n, or NULL */
    uint8_t *any;                      /* n, or NULL */
    int32_t k;                         /* ids per box, 0 .. RT_OVERLAP_MAX */
    int32_t any_only;                  /* 1: only `any` is asked for - a box stops at its first overlapping candidate */
} rt_overlap_args;

static_assert(sizeof(rt_overlap_id) == 8, "the kernels store an id as one 8-byte unit");
static_assert(RT_OVERLAP_MAX == 8, "rt_ov_buf's slots and the kernels' stores are written for eight");

#endif
