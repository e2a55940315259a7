/*
 * rt_multihit.h — multi-hit ray queries (rt_trace_rays_multi[_device], include/rt_amd.h): what the kernel (rt_multihit_kernel.h), the entry
 * points (rt_multihit_capi.cpp) and the host tests (tests/sanitize/multihit_host_check.cpp) share.  Host code; self-contained.
 *
 *  - the candidate tests, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction
 *    off).  They restate rt_intersect.h's box_test, tri_test, quad_test and sphere test operation for operation on plain floats, so that
 *    the host tests run them too; tests/test_gpu_multihit.py holds record 0 to rt_trace_rays bit for bit;
 *  - the per-ray buffer of the first k candidates (rt_mh_buf) and its insert: eight statically indexed slots, compare and select;
 *  - the traversal of one mesh as steps over a small state (rt_mh_walk): nearer child first by key, the other pushed with its key when
 *    that is not greater than the threshold, a popped entry checked against the threshold of that moment.  The kernel runs one step per
 *    lane and round of its wave loop, the host test runs the same steps in a plain loop;
 *  - the argument blocks (the launchers are rt_launch.h's rt_launch_multihit and rt_launch_multihit_uv).
 *
 * The definition - candidates, key, limit, order, and why the key makes pruning exact - is include/rt_amd.h's.
 */
#ifndef RT_MULTIHIT_H
#define RT_MULTIHIT_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"

#if defined(__HIPCC__)
#define RT_MH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT_MH_HD inline
#endif

/* A value every lane of a wave holds alike (read from the object table at an address all lanes share), handed to the compiler as such:
 * what branches on it is then a scalar branch that saves no lane mask.  On the host it is the value. */
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_MH_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define RT_MH_UNIFORM(x) (x)
#endif

#define RT_MULTIHIT_MAX_RAYS (1 << 30)     /* rays of one call (ray ids and the chunk counter are 32-bit) */
/* A candidate's identity in one word, ordered as the tie rule asks (ascending word: higher object first, then lower triangle):
 * bits 31..20 hold RT_MH_MAX_OBJECTS - 1 - object, bits 19..0 the flattened triangle index (at most RT_REF_START_MASK - 1: rt_flatten
 * refuses more), or RT_MH_NO_TRI for a sphere.  A scene of more objects than that is refused by the entry points. */
#define RT_MH_MAX_OBJECTS 4096
#define RT_MH_NO_TRI 0x000fffffu
/* an empty slot: key +Inf, behind every candidate (a candidate's key is at most the limit, which is at most RT_HIT_MISS_T) */
#define RT_MH_EMPTY 0x7f800000ffffffffull

/* One ray's first candidates.  Slot s holds (key bits << 32 | identity word) and the candidate's raw t.  A key is a positive float, so
 * the 64-bit words order as (key, identity).  All eight slots are kept ascending whatever k is - the first k of them are the answer -
 * so that neither the insert nor an empty buffer depends on k (eight k-dependent start values would sit in scalar registers for the whole
 * kernel); only the threshold reads k: it is slot k - 1's key.
 * `total`: the candidates that counted, whether kept or not (exact while fewer than k are held, and always with k == 0). */
struct rt_mh_buf { uint64_t key[RT_MULTIHIT_MAX]; float t[RT_MULTIHIT_MAX]; uint32_t total; };
/* one pending subtree of a lane's stack: 8 bytes, one LDS access */
struct __attribute__((aligned(8))) rt_mh_entry { float key; uint32_t ref; };
/* the walk of one mesh: the node or leaf a lane is on, its key (the largest entry distance on the path so far), the entries on its stack, and
 * on a leaf how many of its triangles are done */
struct rt_mh_walk { uint32_t cur; float key; int32_t sp, at; };
/* the ray as given, and 1.0f / d per component */
struct rt_mh_ray { float ox, oy, oz, dx, dy, dz, ix, iy, iz; };
/* the scene sections; F4 is a 16-byte unit with members x, y, z, w (rt_f4 on the host, the kernels' v4f on the device) */
template <class F4> struct rt_mh_scene { const F4 *nodes, *tris, *meshes, *objtab; };

RT_MH_HD uint32_t rt_mh_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_MH_HD float rt_mh_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

/* ---- the candidate tests (rt_intersect.h's, on plain floats) ------------------------------------------------------------------ */
RT_MH_HD float rt_mh_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* box_test: the strict slab test, and the entry distance (starts from 0, drops NaNs: never a NaN) */
RT_MH_HD bool rt_mh_box(float bx0, float by0, float bz0, float bx1, float by1, float bz1, const rt_mh_ray &r, float &tmin_out)
{
    float tmin = 0.0f, tmax = RT_INF_F;
    float t1 = (bx0 - r.ox) * r.ix, t2 = (bx1 - r.ox) * r.ix;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    t1 = (by0 - r.oy) * r.iy; t2 = (by1 - r.oy) * r.iy;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    t1 = (bz0 - r.oz) * r.iz; t2 = (bz1 - r.oz) * r.iz;
    tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    tmin_out = tmin;
    return tmin < tmax && tmax > 0.0f;
}

/* tri_test on the record (q0, q1, q2) */
template <class F4>
RT_MH_HD bool rt_mh_tri(const F4 q0, const F4 q1, const F4 q2, const rt_mh_ray &r, float &t_out)
{
    const float p0x = q0.x, p0y = q0.y, p0z = q0.z, s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
    const float px = r.dy * s2z - r.dz * s2y, py = r.dz * s2x - r.dx * s2z, pz = r.dx * s2y - r.dy * s2x;     /* cross(d, s2) */
    const float det = rt_mh_dot(s1x, s1y, s1z, px, py, pz);
    const float inv_det = 1.0f / det;
    const float tx = r.ox - p0x, ty = r.oy - p0y, tz = r.oz - p0z;
    const float u = rt_mh_dot(tx, ty, tz, px, py, pz) * inv_det;
    const float qx = ty * s1z - tz * s1y, qy = tz * s1x - tx * s1z, qz = tx * s1y - ty * s1x;                 /* cross(t_vec, s1) */
    const float v = rt_mh_dot(r.dx, r.dy, r.dz, qx, qy, qz) * inv_det;
    const float w = 1.0f - u - v;
    const float dist = rt_mh_dot(s2x, s2y, s2z, qx, qy, qz) * inv_det;
    t_out = dist;
    return dist > RT_EPS_F && u >= 0.0f && v >= 0.0f && w >= 0.0f;
}

/* Sphere::hit's near root for the sphere (c, r) */
RT_MH_HD bool rt_mh_sphere(float cx, float cy, float cz, float rad, const rt_mh_ray &r, float &t_out)
{
    const float qx = cx - r.ox, qy = cy - r.oy, qz = cz - r.oz;
    const float qa = rt_mh_dot(r.dx, r.dy, r.dz, r.dx, r.dy, r.dz);
    const float qb = rt_mh_dot(r.dx, r.dy, r.dz, qx, qy, qz) * (-2.0f);
    const float qc = rt_mh_dot(qx, qy, qz, qx, qy, qz) - rad * rad;
    const float disc = qb * qb - 4.0f * qa * qc;
    if (!(disc >= 0.0f)) return false;
    const float dist = (-qb - sqrtf(disc)) / (2.0f * qa);
    t_out = dist;
    return dist > RT_EPS_F;
}

/* ---- the buffer ---------------------------------------------------------------------------------------------------------------- */
RT_MH_HD uint64_t rt_mh_word(float key, int32_t object, uint32_t tri_field)
{
    return ((uint64_t)rt_mh_bits(key) << 32) | (uint64_t)((((uint32_t)(RT_MH_MAX_OBJECTS - 1) - (uint32_t)object) << 20) | tri_field);
}
RT_MH_HD float rt_mh_word_key(uint64_t w) { return rt_mh_float((uint32_t)(w >> 32)); }
RT_MH_HD int32_t rt_mh_word_object(uint64_t w) { return (int32_t)((uint32_t)(RT_MH_MAX_OBJECTS - 1) - (((uint32_t)w) >> 20)); }
RT_MH_HD int32_t rt_mh_word_triangle(uint64_t w) { const uint32_t f = (uint32_t)w & RT_MH_NO_TRI; return f == RT_MH_NO_TRI ? -1 : (int32_t)f; }

RT_MH_HD void rt_mh_clear(rt_mh_buf &b)
{
#pragma unroll
    for (int j = 0; j < RT_MULTIHIT_MAX; j++) { b.key[j] = RT_MH_EMPTY; b.t[j] = 0.0f; }
    b.total = 0u;
}

/* The insert: the word goes to its place among the ascending slots and the last one falls out; a word not below the last slot changes nothing.
 * Every slot is a select between itself, its neighbour in front and the newcomer: no index is computed, the slots stay in registers. */
RT_MH_HD void rt_mh_insert(rt_mh_buf &b, uint64_t word, float t)
{
    /* from the last slot down: slot j takes slot j - 1 where the word goes in front of that, the word where it goes in front of slot j
     * only, and stays otherwise; slot j - 1 is read before its own turn overwrites it.  Two compares' outcomes are held at a time. */
    bool below = word < b.key[RT_MULTIHIT_MAX - 1];
#pragma unroll
    for (int j = RT_MULTIHIT_MAX - 1; j > 0; j--) {
        const bool below_prev = word < b.key[j - 1];
        b.key[j] = below_prev ? b.key[j - 1] : (below ? word : b.key[j]);
        b.t[j] = below_prev ? b.t[j - 1] : (below ? t : b.t[j]);
        below = below_prev;
    }
    b.key[0] = below ? word : b.key[0];
    b.t[0] = below ? t : b.t[0];
}

/* A tested record (accepted or not; t, object, triangle field) with path value B (0 for a candidate of no mesh): counted and kept when it
 * was accepted and its key is within the limit.  No branch: a record that does not count is inserted as the all-ones word, which is
 * below no slot and changes nothing (with a branch around the insert the compiler keeps the slots twice across a leaf's loop). */
RT_MH_HD void rt_mh_offer(rt_mh_buf &b, float lim, int32_t k, bool accepted, float t, float path, int32_t object, uint32_t tri_field)
{
    const float key = t < path ? path : t;
    const bool counts = accepted && key <= lim;
    b.total += counts ? 1u : 0u;
    if (k > 0) rt_mh_insert(b, counts ? rt_mh_word(key, object, tri_field) : ~0ull, t);
}

/* what a subtree's entry distance is compared with: the limit, or the k-th best key once there is one (an empty slot's key is +Inf).  A
 * subtree AT the threshold is still entered: a candidate in it may win the tie.  k is the same for every ray of a call: the switch is a
 * scalar branch, no slot is picked by a per-lane index */
RT_MH_HD float rt_mh_threshold(const rt_mh_buf &b, float lim, int32_t k)
{
    uint64_t kth;
    switch (k) {
        case 0: return lim;
        case 1: kth = b.key[0]; break;
        case 2: kth = b.key[1]; break;
        case 3: kth = b.key[2]; break;
        case 4: kth = b.key[3]; break;
        case 5: kth = b.key[4]; break;
        case 6: kth = b.key[5]; break;
        case 7: kth = b.key[6]; break;
        default: kth = b.key[7]; break;
    }
    return fminf(lim, rt_mh_word_key(kth));
}

/* how many records a finished ray has */
RT_MH_HD int32_t rt_mh_count(const rt_mh_buf &b, int32_t k)
{
    const uint32_t cap = k > 0 ? (uint32_t)k : 0xffffffffu;        /* (one scalar, not a lane mask kept for the whole kernel) */
    return (int32_t)(b.total < cap ? b.total : cap);
}

/* The start of a ray's query: the reciprocal direction and the limit.  false: nothing can count - a NaN in the direction (every test
 * fails), a NaN limit, or a limit that is not positive (an accepted t is above RT_EPS_F, and a key is no smaller than its t). */
RT_MH_HD bool rt_mh_begin(rt_mh_ray &r, bool has_limit, float tmax, float &lim)
{
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    lim = RT_HIT_MISS_T;
    if (r.dx != r.dx || r.dy != r.dy || r.dz != r.dz) return false;
    if (has_limit) {
        if (tmax != tmax) return false;
        lim = tmax < RT_HIT_MISS_T ? tmax : RT_HIT_MISS_T;
    }
    return lim > 0.0f;
}

/* The objects that are not meshes, in list order, from the object table (rt_object: type, prim_start, ..., v[0..7]).  Every object is a
 * number of FACES with one candidate each - a sphere, a loose triangle or a quad of either kind one, a cuboid its six quads - so that the
 * loop has one place where a candidate is offered: the insert is emitted once.  A quad face (records first, first + 1) is quad_test: the
 * first record if it hits, else the second; a one-way quad has no face when dot(d, normal) < 0. */
template <class F4>
RT_MH_HD void rt_mh_simple(const rt_mh_scene<F4> &S, int32_t num_objects, const rt_mh_ray &r, float lim, int32_t k, rt_mh_buf &b)
{
#pragma unroll 1
    for (int32_t i = 0; i < num_objects; i++) {
        const F4 ob0 = S.objtab[3 * i], ob1 = S.objtab[3 * i + 1];
        const int32_t type = RT_MH_UNIFORM((int32_t)rt_mh_bits(ob0.x)), prim = RT_MH_UNIFORM((int32_t)rt_mh_bits(ob0.y));
        int32_t faces = type == RT_OBJ_MESH ? 0 : type == RT_OBJ_CUBOID ? 6 : 1;
        if (type == RT_OBJ_ONE_WAY_QUAD && rt_mh_dot(r.dx, r.dy, r.dz, ob1.x, ob1.y, ob1.z) < 0.0f) faces = 0;
#pragma unroll 1
        for (int32_t fc = 0; fc < faces; fc++) {
            bool hit;
            float t = 0.0f;
            uint32_t field = RT_MH_NO_TRI;
            if (type == RT_OBJ_SPHERE) {
                hit = rt_mh_sphere(ob1.x, ob1.y, ob1.z, ob1.w, r, t);
            } else {
                const int32_t first = prim + 2 * fc;
                const F4 *q = S.tris + 3 * (size_t)first;
                hit = rt_mh_tri(q[0], q[1], q[2], r, t);
                field = (uint32_t)first;
                if (!hit && type != RT_OBJ_TRIANGLE) {      /* (the second record's own t is only ever reported when the first misses) */
                    hit = rt_mh_tri(q[3], q[4], q[5], r, t);
                    field = (uint32_t)(first + 1);
                }
            }
            rt_mh_offer(b, lim, k, hit, t, 0.0f, i, field);
        }
    }
}

/* ---- the traversal of one mesh --------------------------------------------------------------------------------------------------
 * CHAIN bits of a reference are masked off: they stand for a box tested twice, which changes nothing here. */
/* (m0, m1): the mesh's pair of the `meshes` section.  false: the ray misses the root box, or enters it beyond the threshold */
template <class F4>
RT_MH_HD bool rt_mh_mesh_begin(const F4 m0, const F4 m1, const rt_mh_ray &r, float threshold, rt_mh_walk &w)
{
    float key;
    if (!rt_mh_box(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, r, key) || !(key <= threshold)) return false;
    w.cur = rt_mh_bits(m1.z) & ~RT_REF_CHAIN;
    w.key = key;
    w.sp = 0;
    w.at = 0;
    return true;
}

/* One step: on an internal node, the two children's box tests and keys, the child with the larger key pushed and the other entered (each
 * only if the ray enters its box and its key is not greater than the threshold); on a leaf, its next triangle (one per step: the slots are
 * then changed in straight-line code, and a loop over a leaf that carries them made the compiler keep them twice).  A lane with nowhere
 * to go on pops until it takes an entry.  false: the mesh is finished.  `stack` is the lane's own, entry s at stack[s * STRIDE] (the
 * kernels' [entry][thread] layout); it holds at most one entry per internal node on the path, the depth the scene's stack is sized for. */
template <int STRIDE, class F4>
RT_MH_HD bool rt_mh_step(const rt_mh_scene<F4> &S, rt_mh_entry *stack, int32_t object, const rt_mh_ray &r, float lim, int32_t k, rt_mh_buf &b, rt_mh_walk &w)
{
    if (!(w.cur & RT_REF_LEAF)) {
        const F4 *n = S.nodes + 4 * (size_t)(w.cur & RT_REF_NODE_MASK);
        const F4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
        const float thr = rt_mh_threshold(b, lim, k);
        float tl, tr;
        const bool hl = rt_mh_box(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r, tl);
        const bool hr = rt_mh_box(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r, tr);
        const float kl = tl < w.key ? w.key : tl, kr = tr < w.key ? w.key : tr;
        const bool el = hl && kl <= thr, er = hr && kr <= thr;
        const uint32_t lref = rt_mh_bits(q3.x) & ~RT_REF_CHAIN, rref = rt_mh_bits(q3.y) & ~RT_REF_CHAIN;
        const bool l_first = kl <= kr;
        const float near_key = l_first ? kl : kr, far_key = l_first ? kr : kl;
        const uint32_t near_ref = l_first ? lref : rref, far_ref = l_first ? rref : lref;
        const bool near_ok = l_first ? el : er, far_ok = l_first ? er : el;
        if (near_ok && far_ok) {
            rt_mh_entry e;
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
            const F4 *q = S.tris + 3 * (size_t)(start + w.at);
            float t;
            const bool hit = rt_mh_tri(q[0], q[1], q[2], r, t);
            rt_mh_offer(b, lim, k, hit, t, w.key, object, (uint32_t)(start + w.at));
            w.at++;
            if (w.at < count) return true;
        }
    }
    while (w.sp > 0) {
        w.sp--;
        const rt_mh_entry e = stack[(size_t)w.sp * STRIDE];
        if (e.key <= rt_mh_threshold(b, lim, k)) { w.cur = e.ref; w.key = e.key; w.at = 0; return true; }
    }
    return false;
}

/* ---- the argument blocks ------------------------------------------------------------------------------------------------------ */
/* The scene and work fields carry the names rt_query_args gives them: rt_internal.h's ray_args_scene fills them, rt_stage_scene reads them. */
typedef struct {
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;              /* (not read: the walk has no descend loop of its own) */
    const float *tri_uv;
    /* the work: rays [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    const float *origins, *directions; /* n x 3 floats each */
    const float *tmax;                 /* n floats, or NULL: RT_HIT_MISS_T for every ray */
    int32_t k;                         /* records per ray, 0 .. RT_MULTIHIT_MAX; 0: count only */
    rt_hit *hits;                      /* n * k records, [ray][rank], 16-byte aligned (not read with k == 0) */
    int32_t *counts;                   /* n, or NULL */
} rt_multihit_args;

/* the second pass (rt_multihit_uv_kernel): the texture coordinates of the records that lie on a sphere whose material needs them */
typedef struct {
    const rt_f4 *objlds;               /* the scene's per-object shading records (blob + off_objlds) */
    rt_hit *hits;                      /* records of them */
    int64_t records;
} rt_multihit_uv_args;

#endif
