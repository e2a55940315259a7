/*
 * rt_winding.h — winding-number queries (rt_winding_numbers[_device], rt_signed_distance[_device], include/rt_amd.h): what the kernel
 * (rt_winding_kernel.h), the entry points (rt_winding_capi.cpp) and the host tests (tests/sanitize/winding_host_check.cpp) share.  Host
 * code; self-contained.
 *
 *  - the arithmetic, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off):
 *    rt_wn_atan2, the term of a triangle record, the sphere and cuboid rules, an object's winding number, the sum over the solids;
 *  - the fast queries (rt_winding_numbers_fast[_device], rt_signed_distance_fast[_device]): the gather into cluster order, the clusters'
 *    sums and moments and the stackless walk, again one text for the device, the host and the host tests; and, host only, the builder of
 *    the cluster trees' topology (rt_wn_tree) with the host's refit;
 *  - the argument block (the launcher is rt_launch.h's rt_launch_winding).
 *
 * The definition - every formula in the order it is evaluated - is include/rt_amd.h's.  Nothing here depends on the point but the
 * arithmetic: every loop bound and every record address comes from the scene alone, so on the device all lanes of a wave are on the same
 * record at the same time and the records are read by wave-uniform addresses.  (The exact query, that is: which clusters a fast query's
 * walk visits depends on the point.)
 */
#ifndef RT_WINDING_H
#define RT_WINDING_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

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

/* ---- the fast queries: a dipole cluster tree per mesh (include/rt_amd.h has the definition) ----------------------------------- */
/* What a walk reads.  topo: per cluster (skip, first, count, height) as bit patterns; moments: per cluster (c.xyz, r2) (M.xyz, 0); rec: the
 * meshes' records gathered in cluster order, three units each as in the blob but for the third, (s2.z, flip bit, 0, 0); object_range: per
 * object (c0, c1) */
template <class F4> struct rt_wn_fast {
    const F4 *topo, *moments, *rec;
    const int32_t *object_range;
    float beta2;
};

/* a record as the gather leaves it: position j of the mesh whose first record is `base` goes to where its commit index sits in the cluster order */
template <class F4>
RT_WN_HD void rt_wn_gather(const rt_wn_scene<F4> &S, const int32_t *inv, F4 *rec, int32_t base, int32_t count, int32_t j)
{
    const int32_t t = base + j, commit = S.perm[t];
    if ((uint32_t)commit >= (uint32_t)count) return;                        /* (a list entry outside its mesh: nothing is written) */
    const int32_t dst = inv[base + commit];
    if ((uint32_t)(dst - base) >= (uint32_t)count) return;
    F4 q2 = S.tris[3 * (size_t)t + 2];
    q2.y = rt_wn_float(rt_wn_flip(S, base, commit)); q2.z = 0.0f; q2.w = 0.0f;
    rec[3 * (size_t)dst] = S.tris[3 * (size_t)t];
    rec[3 * (size_t)dst + 1] = S.tris[3 * (size_t)t + 1];
    rec[3 * (size_t)dst + 2] = q2;
}

/* the sums of a cluster, four units: (Msum.xyz, Asum) (Gsum.xyz, 0) (lo.xyz, 0) (hi.xyz, 0).  A leaf's, over its gathered records: */
template <class F4>
RT_WN_HD void rt_wn_leaf_sums(const F4 *rec, int32_t first, int32_t count, F4 out[4])
{
    float mx = 0.0f, my = 0.0f, mz = 0.0f, as = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    const F4 f0 = rec[3 * (size_t)first];
    float lox = f0.x, loy = f0.y, loz = f0.z, hix = f0.x, hiy = f0.y, hiz = f0.z;
    for (int32_t k = first; k < first + count; k++) {
        const F4 q0 = rec[3 * (size_t)k], q1 = rec[3 * (size_t)k + 1], q2 = rec[3 * (size_t)k + 2];
        const float s1x = q0.w, s1y = q1.x, s1z = q1.y, s2x = q1.z, s2y = q1.w, s2z = q2.x;
        float nx = s1y * s2z - s1z * s2y, ny = s1z * s2x - s1x * s2z, nz = s1x * s2y - s1y * s2x;
        if (rt_wn_bits(q2.y) & 1u) { nx = rt_wn_neg(nx); ny = rt_wn_neg(ny); nz = rt_wn_neg(nz); }
        const float a = sqrtf(rt_wn_dot(nx, ny, nz, nx, ny, nz));
        const float cx = q0.x + (s1x + s2x) * RT_WN_THIRD, cy = q0.y + (s1y + s2y) * RT_WN_THIRD, cz = q0.z + (s1z + s2z) * RT_WN_THIRD;
        mx = mx + nx; my = my + ny; mz = mz + nz;
        as = as + a;
        gx = gx + a * cx; gy = gy + a * cy; gz = gz + a * cz;
        for (int corner = 0; corner < 3; corner++) {
            const float x = corner == 0 ? q0.x : corner == 1 ? q0.x + s1x : q0.x + s2x;
            const float y = corner == 0 ? q0.y : corner == 1 ? q0.y + s1y : q0.y + s2y;
            const float z = corner == 0 ? q0.z : corner == 1 ? q0.z + s1z : q0.z + s2z;
            lox = x < lox ? x : lox; loy = y < loy ? y : loy; loz = z < loz ? z : loz;
            hix = hix < x ? x : hix; hiy = hiy < y ? y : hiy; hiz = hiz < z ? z : hiz;
        }
    }
    out[0].x = mx; out[0].y = my; out[0].z = mz; out[0].w = as;
    out[1].x = gx; out[1].y = gy; out[1].z = gz; out[1].w = 0.0f;
    out[2].x = lox; out[2].y = loy; out[2].z = loz; out[2].w = 0.0f;
    out[3].x = hix; out[3].y = hiy; out[3].z = hiz; out[3].w = 0.0f;
}

/* an internal cluster's: the left child's plus the right child's, left operand first */
template <class F4>
RT_WN_HD void rt_wn_add_sums(const F4 L[4], const F4 R[4], F4 out[4])
{
    out[0].x = L[0].x + R[0].x; out[0].y = L[0].y + R[0].y; out[0].z = L[0].z + R[0].z; out[0].w = L[0].w + R[0].w;
    out[1].x = L[1].x + R[1].x; out[1].y = L[1].y + R[1].y; out[1].z = L[1].z + R[1].z; out[1].w = 0.0f;
    out[2].x = R[2].x < L[2].x ? R[2].x : L[2].x; out[2].y = R[2].y < L[2].y ? R[2].y : L[2].y; out[2].z = R[2].z < L[2].z ? R[2].z : L[2].z; out[2].w = 0.0f;
    out[3].x = L[3].x < R[3].x ? R[3].x : L[3].x; out[3].y = L[3].y < R[3].y ? R[3].y : L[3].y; out[3].z = L[3].z < R[3].z ? R[3].z : L[3].z; out[3].w = 0.0f;
}

/* the moments a walk reads, from the sums: (c.xyz, r2) (M.xyz, 0) */
template <class F4>
RT_WN_HD void rt_wn_moments(const F4 s[4], F4 out[2])
{
    const bool area = s[0].w > 0.0f;
    const float cx = area ? s[1].x / s[0].w : s[2].x, cy = area ? s[1].y / s[0].w : s[2].y, cz = area ? s[1].z / s[0].w : s[2].z;
    const float ax = cx - s[2].x, ay = cy - s[2].y, az = cz - s[2].z, bx = s[3].x - cx, by = s[3].y - cy, bz = s[3].z - cz;
    const float ex = ax > bx ? ax : bx, ey = ay > by ? ay : by, ez = az > bz ? az : bz;
    out[0].x = cx; out[0].y = cy; out[0].z = cz; out[0].w = rt_wn_dot(ex, ey, ez, ex, ey, ez);
    out[1].x = 0.25f * s[0].x; out[1].y = 0.25f * s[0].y; out[1].z = 0.25f * s[0].z; out[1].w = 0.0f;
}

/* The walk of a mesh's clusters [c0, c1) for the point p, stackless by the skip indices.  One step is either a cluster (far: its dipole; a
 * near leaf: its triangles are queued; a near internal one: on to its left child) or ONE triangle term of the queued leaf: on the device
 * the lanes of a wave are in different states, and a step that does one of each keeps both kinds busy.  The order of the additions into A
 * is the definition's whatever the interleaving: a lane finishes its leaf before its next cluster. */
template <class F4>
RT_WN_HD float rt_wn_mesh_fast(const rt_wn_fast<F4> &T, int32_t c0, int32_t c1, float px, float py, float pz)
{
    float A = 0.0f;
    int32_t i = c0, k = 0, kend = 0;
    while (k < kend || i < c1) {
        if (k < kend) {
            const F4 q0 = T.rec[3 * (size_t)k], q1 = T.rec[3 * (size_t)k + 1], q2 = T.rec[3 * (size_t)k + 2];
            const float term = rt_wn_term(q0, q1, q2, px, py, pz);
            A = A + ((rt_wn_bits(q2.y) & 1u) ? rt_wn_neg(term) : term);
            k++;
        } else {
            const F4 t = T.topo[i], m0 = T.moments[2 * (size_t)i], m1 = T.moments[2 * (size_t)i + 1];
            const float dx = m0.x - px, dy = m0.y - py, dz = m0.z - pz;
            const float d2 = rt_wn_dot(dx, dy, dz, dx, dy, dz);
            const int32_t skip = (int32_t)rt_wn_bits(t.x), first = (int32_t)rt_wn_bits(t.y), count = (int32_t)rt_wn_bits(t.z);
            if (d2 > T.beta2 * m0.w) {
                A = A + rt_wn_dot(m1.x, m1.y, m1.z, dx, dy, dz) / (d2 * sqrtf(d2));
                i = skip;
            } else if (count > 0) {
                k = first; kend = first + count;
                i = skip;
            } else {
                i = i + 1;
            }
        }
    }
    return A * RT_INV_2PI;
}

/* rt_wn_point with the meshes through their trees; everything else as there */
template <class F4>
RT_WN_HD float rt_wn_point_fast(const rt_wn_scene<F4> &S, const rt_wn_fast<F4> &T, int32_t object, float px, float py, float pz)
{
    const bool ok = rt_wn_finite(px) && rt_wn_finite(py) && rt_wn_finite(pz);
    const float x = ok ? px : 0.0f, y = ok ? py : 0.0f, z = ok ? pz : 0.0f;
    float w = 0.0f;
    for (int32_t i = object >= 0 ? object : 0; i < (object >= 0 ? object + 1 : S.num_objects); i++) {
        const int32_t type = (int32_t)rt_wn_bits(S.objtab[3 * i].x);
        if (object < 0 && type != RT_OBJ_SPHERE && type != RT_OBJ_CUBOID && type != RT_OBJ_MESH) continue;
        float wo;
        if (type == RT_OBJ_MESH) {
            const int32_t c0 = T.object_range[2 * i], c1 = T.object_range[2 * i + 1];
            wo = rt_wn_mesh_fast(T, c0, ok ? c1 : c0, x, y, z);                  /* (a point that is not finite walks nothing: its answer is the NaN) */
        } else {
            wo = rt_wn_object(S, i, x, y, z);
        }
        w = object >= 0 ? wo : w + wo;
    }
    return ok && w == w ? w : rt_wn_float(0x7FC00000u);
}

/* The trees of a scene on the host: the topology (never changed once built) and the lists the refit goes by */
struct rt_wn_tree {
    std::vector<int32_t> skip, first, count, height;       /* per cluster; height: 0 a leaf, else one more than the higher child */
    std::vector<int32_t> object_range;                     /* per object (c0, c1) */
    std::vector<int32_t> order, inv;                       /* per flattened triangle index: [base + cluster position] = commit index, and its inverse [base + commit index] = base + cluster position */
    std::vector<int32_t> levels, level_off;                /* the clusters sorted by height; level_off[h] .. level_off[h + 1]: those of height h */
};

inline void rt_wn_tree_init(rt_wn_tree &T, int32_t num_objects, int32_t num_tris)
{
    T = rt_wn_tree();
    T.object_range.assign(2 * (size_t)num_objects, 0);
    T.order.assign((size_t)num_tris, 0);
    T.inv.assign((size_t)num_tris, 0);
}

/* one subtree over the cluster positions [lo, hi) of the mesh at `base`, whose entries of T.order are commit indices already */
inline void rt_wn_build_range(rt_wn_tree &T, const float *centroids, int32_t base, int32_t lo, int32_t hi)
{
    const size_t me = T.skip.size();
    T.skip.push_back(0); T.first.push_back(0); T.count.push_back(0);
    const int32_t m = hi - lo;
    if (m <= RT_WINDING_LEAF_TRIS) {
        T.first[me] = base + lo;
        T.count[me] = m;
    } else {
        int32_t *o = T.order.data() + base;
        float mn[3], mx[3];
        for (int a = 0; a < 3; a++) mn[a] = mx[a] = centroids[3 * (size_t)o[lo] + a];
        for (int32_t k = lo + 1; k < hi; k++)
            for (int a = 0; a < 3; a++) {
                const float c = centroids[3 * (size_t)o[k] + a];
                if (c < mn[a]) mn[a] = c;
                if (c > mx[a]) mx[a] = c;
            }
        int axis = 0;
        for (int a = 1; a < 3; a++)
            if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
        std::stable_sort(o + lo, o + hi, [&](int32_t u, int32_t v) { return centroids[3 * (size_t)u + axis] < centroids[3 * (size_t)v + axis]; });
        const int32_t mid = lo + (m + 1) / 2;
        rt_wn_build_range(T, centroids, base, lo, mid);
        rt_wn_build_range(T, centroids, base, mid, hi);
    }
    T.skip[me] = (int32_t)T.skip.size();
}

/* the tree of object `object`, a mesh of n triangles whose first record is `base`; centroids: three floats per commit index (any NaN compares
 * false: the order is still a permutation) */
inline void rt_wn_build_mesh(rt_wn_tree &T, int32_t object, const float *centroids, int32_t n, int32_t base)
{
    T.object_range[2 * (size_t)object] = (int32_t)T.skip.size();
    for (int32_t k = 0; k < n; k++) T.order[(size_t)base + k] = k;
    if (n > 0) rt_wn_build_range(T, centroids, base, 0, n);
    T.object_range[2 * (size_t)object + 1] = (int32_t)T.skip.size();
    for (int32_t k = 0; k < n; k++) T.inv[(size_t)base + T.order[(size_t)base + k]] = base + k;
}

/* after the last mesh: the heights and the refit's lists */
inline void rt_wn_tree_finish(rt_wn_tree &T)
{
    const size_t n = T.skip.size();
    T.height.assign(n, 0);
    int32_t top = 0;
    for (size_t i = n; i-- > 0;) {
        if (T.count[i] > 0) continue;
        const int32_t l = T.height[i + 1], r = T.height[(size_t)T.skip[i + 1]];
        T.height[i] = 1 + (l > r ? l : r);
        if (T.height[i] > top) top = T.height[i];
    }
    T.level_off.assign((size_t)top + 2, 0);
    for (size_t i = 0; i < n; i++) T.level_off[(size_t)T.height[i] + 1]++;
    for (size_t h = 0; h + 1 < T.level_off.size(); h++) T.level_off[h + 1] += T.level_off[h];
    T.levels.assign(n, 0);
    std::vector<int32_t> at(T.level_off.begin(), T.level_off.end() - 1);
    for (size_t i = 0; i < n; i++) T.levels[(size_t)at[(size_t)T.height[i]]++] = (int32_t)i;
}

/* topo as a walk and the refit read it: four words per cluster */
inline std::vector<int32_t> rt_wn_tree_topo(const rt_wn_tree &T)
{
    std::vector<int32_t> topo(4 * T.skip.size());
    for (size_t i = 0; i < T.skip.size(); i++) { topo[4 * i] = T.skip[i]; topo[4 * i + 1] = T.first[i]; topo[4 * i + 2] = T.count[i]; topo[4 * i + 3] = T.height[i]; }
    return topo;
}

/* the refit on the host, as the device's kernels do it: the leaves' sums from the gathered records, the internal clusters' bottom-up (a
 * cluster's children come behind it), every cluster's moments.  sums: 4 units per cluster, moments: 2 */
template <class F4>
inline void rt_wn_host_refit(const rt_wn_tree &T, const F4 *rec, F4 *sums, F4 *moments)
{
    for (size_t i = T.skip.size(); i-- > 0;) {
        if (T.count[i] > 0) rt_wn_leaf_sums(rec, T.first[i], T.count[i], sums + 4 * i);
        else rt_wn_add_sums(sums + 4 * (i + 1), sums + 4 * (size_t)T.skip[i + 1], sums + 4 * i);
        rt_wn_moments(sums + 4 * i, moments + 2 * i);
    }
}

#define RT_WN_OP_EXACT 0                /* rt_winding_args::op: the exact query (a zeroed block's) */
#define RT_WN_OP_GATHER 1               /* the records of the mesh [mesh_base, mesh_base + mesh_count) into cluster order */
#define RT_WN_OP_LEAVES 2               /* sums and moments of the clusters levels[range_first .. + range_count), which are leaves */
#define RT_WN_OP_COMBINE 3              /* ... which are internal clusters of one height, their children's sums being there */
#define RT_WN_OP_FAST 4                 /* the fast query */

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
    /* the fast queries and their refit; all zero: the exact query, as before these fields were there */
    int32_t op;                        /* RT_WN_OP_* */
    float beta2;
    const rt_f4 *topo;                 /* per cluster (skip, first, count, height) as bit patterns (rt_scene::d_wn_topo) */
    const int32_t *object_range;       /* per object (c0, c1) */
    const int32_t *inv, *levels;       /* rt_wn_tree's */
    rt_f4 *rec, *sums, *moments;       /* 3 units per triangle, 4 and 2 per cluster: written by the refit, read by the query */
    int32_t mesh_base, mesh_count;     /* RT_WN_OP_GATHER */
    int32_t range_first, range_count;  /* RT_WN_OP_LEAVES, RT_WN_OP_COMBINE: entries of levels */
} rt_winding_args;

#endif
