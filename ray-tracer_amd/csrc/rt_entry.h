/*
 * rt_entry.h — the primary entry word: one word per pixel of a view, behind the cull plane's bits and gate words (rt_cull.h), that says where
 * the pixel's primary rays end: `triangle T` (every ray of the pixel's jitter cone ends its traversal of the one mesh with (w_prim, w_best) =
 * (T, t_T)), `nothing` (every ray ends it with w_prim == -1 although the cone reaches leaves), or 0 (not known: traverse).  Host and device
 * run the same function.  DESIGN.md section 24, "The primary entry word", has the figures.
 *
 * WHY THE FRAMES STAY BIT-IDENTICAL.  For a `triangle T` pixel (a)-(c) below hold for every sample: the ungated traversal reaches T's leaf,
 * accepts T there, and accepts no triangle at a distance <= t_T before or after it, whatever order it visits the leaves in: it ends with
 * (T, t_T).  The render kernel starts such a ray on the one-triangle leaf (T): the same triangle test on the same operands against
 * best = RT_INF_F gives the same t_T, the stack is empty, the merge with the simple objects follows unchanged.  A traversal draws no random
 * numbers.  `nothing` is the cull bit's argument one level down: every triangle of every leaf the cone can reach is certainly rejected, so
 * the traversal ends with w_prim == -1 and its merge is a no-op.  The gated traversal equals the ungated one (rt_cull.h).  Only the cost
 * counters move.
 *
 * THE SAMPLES OF A PIXEL.  As in rt_cull.h: v = fl(P + off), v_k in [fl(P_k - J), fl(P_k + J)] (the cone's box, the three axes independent),
 * d_k = fl(v_k * s) with ONE float s > 0 per sample, inv_k = fl(1 / d_k).  Write d_k = s * v'_k: v'_k = v_k (1 + e), |e| <= u = 2^-24.  Everything
 * the kernel computes from d is homogeneous in d, so it is bounded here in "v units" and s cancels wherever two quantities of ONE sample are
 * compared; only t > RT_EPS_F and t < RT_INF_F need s itself, bounded by 1 / (4 max|v_k|) .. 1 / max|v_k| up to roundings (below: vmin, vmax).
 * Every axis must keep its sign over the cone (a direction interval that touches zero answers 0), every input must be finite and inside
 * the guards of rt_cull.h, and a determinant is used only from 2^-60 up to 2^60: every float intermediate is then a normal number or
 * an underflow below 2^-110 in magnitude, which RT_ENTRY_ABS covers.
 *
 * THE TRIANGLE TEST (tri_closer_lanes, rt_intersect.h).  With t_vec = fl(o - p0), q_vec = fl(cross(t_vec, s1)) and NT = fl(dot(s2, q_vec)),
 * none of which depends on the direction and all of which are computed here as there, the kernel forms
 *     det = dot(s1, cross(d, s2))     nu = dot(t_vec, cross(d, s2))     nv = dot(d, q_vec)
 *     inv_det = 1 / det,  u = nu * inv_det,  v = nv * inv_det,  w = (1 - u) - v,  t = NT * inv_det
 * det, nu and nv are linear forms L . d of the direction whose coefficients are known exactly (products of two floats, exact in binary64).
 * Over the cone's box the real value of L . v has the range mid +- rad (mid = L . centre, rad = sum |L_k| radius_k: exact for a box, no
 * dependency problem), and the float evaluation is off by at most 6u times the sum of the magnitudes of its product terms (at most five
 * roundings on the way of each term), to which the rounding of d_k (u), of the coefficients' differences and of mid and rad in binary64
 * (2^-50) add: all inside RT_ENTRY_E = 2^-20 = 16u times that magnitude sum `mag`, plus RT_ENTRY_ABS.  So in v units
 *     det in [mid - rad - E mag - ABS, mid + rad + E mag + ABS]   and the same for nu, nv and for nu + nv (the form L_u + L_v).
 * With the sign of det fixed (multiply everything by it: D = |det| in [D_lo, D_hi], D_lo >= 2^-60):
 *   - u >= 0 for every sample if nu_lo >= 0 (a sign is never rounded; -0 >= 0 holds); u < 0 for every sample if nu_hi <= -2^-60 (no
 *     underflow to -0: |u| >= 2^-120).  The same for v.
 *   - u and v each carry two more roundings (1 / det and the product), so as real numbers u + v lies in hull((nu + nv) / D) widened by
 *     E (umax + vmax), umax = max|nu| / D_lo.  w >= 0 iff fl(1 - u) >= v (a float difference has the sign of the real one), which holds
 *     if 1 - (u + v)_hi >= E (1 + umax); w < 0 for every sample if (u + v)_lo - 1 > E (1 + umax).
 *   - t = (1 / s) t', t' = NT / D widened by E: [t_lo, t_hi] in v units.  NT of the wrong sign (or 0): t <= 0, rejected.  t > RT_EPS_F for
 *     every sample if t_lo * vmin * (1 - E) > RT_EPS_F; t <= RT_EPS_F for every sample if t_hi * vmax * (1 + E) < RT_EPS_F.
 * A triangle is CERTAINLY HIT (u, v, w >= 0, RT_EPS_F < t < RT_INF_F for every sample), CERTAINLY REJECTED (one of the four fails for
 * every sample; a NaN fails too), or MAYBE; a triangle whose det interval touches zero is MAYBE with t_lo = -infinity.
 *
 * THE BOXES ON THE WAY (the slab forms, rt_intersect.h).  As in rt_cull.h, the near and far product of axis k are fl(N_k |inv_k|) and
 * fl(F_k |inv_k|); with three roundings s * near_i <= N_i / min|v_i| (1 + E) for N_i >= 2^-40 (near_i <= 0 for N_i <= 0) and
 * s * far_j >= F_j / max|v_j| (1 - E) for F_j >= 2^-40.  A box is CERTAINLY ENTERED BEFORE x (in v units) if every F_j >= 2^-40, every
 * positive N_i >= 2^-40, N_i / min|v_i| (1 + E) < F_j / max|v_j| (1 - E) for every i != j, N_i (1 + E) < F_i (1 - E) for every i (the
 * same inv_i multiplies both; a flat box is entered by no ray), and its entry bound e = max(0, max_i N_i / min|v_i| (1 + E)) < x.  Then
 * tmin < tmax in every slab form (box_enter_med3 takes the same decisions for rays without a zero component, rt_intersect.h), and
 * tmin < best for every best >= x / s.
 *
 * THE WORD (rt_entry_word).  The walk is rt_cull_no_leaf's, over every leaf the cone may reach, with the entry bound of the path - the
 * maximum of e over the boxes from the root's child down, infinite as soon as one of them is not certainly entered - carried along.
 *   (a) T is certainly hit;
 *   (c) the path bound of T's leaf is below t_lo(T).  Until T is tested `best` is RT_INF_F or the distance of an accepted triangle, which by
 *       (b) exceeds t_hi(T) >= t_lo(T): every box of the path passes `entry < min(exit, best)` where its parent is visited, and its deferred
 *       entry is taken when popped - strictly below best, so the plain-edge and the chain-edge rule agree.  The root box is tested by the
 *       kernel as before.
 *   (b) every other triangle of every reachable leaf (T's own included) is certainly rejected or has t_lo > t_hi(T): tested before T it
 *       may lower best, but not to t_T or below; tested after T it fails t < best.  Strict, so no tie rule is involved.  A triangle in a
 *       leaf the cone cannot reach is never tested (rt_cull.h).
 * `nothing`: at least one leaf with triangles is reached and every triangle met is certainly rejected.  A pixel the bit plane flags has 0.
 * tests/sanitize/entry_soundness.cpp walks the kernel's float traversal from the root and from the word and compares the results.
 */
#ifndef RT_ENTRY_H
#define RT_ENTRY_H

#include "rt_cull.h"

#ifndef RT_ENTRY_E                       /* (tests/sanitize/entry_soundness.cpp is also built with the margins taken away, to show that it finds the loss) */
#define RT_ENTRY_E 9.5367431640625e-07           /* E = 2^-20 (binary64) */
#define RT_ENTRY_ABS 1e-30                       /* what underflowing float intermediates can add to a linear form */
#endif
#ifndef RT_ENTRY_ABS
#define RT_ENTRY_ABS 0.0
#endif
#define RT_ENTRY_DET_MIN 8.673617379884035e-19   /* 2^-60: the least |det|, |nu|, |nv| a sign is taken from */
#define RT_ENTRY_DET_MAX 1152921504606846976.0   /* 2^60 */
#define RT_ENTRY_BIG 1e300                       /* "not bounded" */

#define RT_ENTRY_NOTHING 2u              /* the entry word `nothing`; `triangle T` is T << 1 | 1: bit 0 tags it, and no gate word has bit 0 */
#define RT_ENTRY_TAG 1u
#define RT_CULL_WITH_ENTRY 4             /* rt_launch_cull's view_flags: compute the entry words (else every one is written as 0) ... */
#define RT_CULL_TRIS_SHIFT 4             /* ... of the triangles that start at 16-byte unit view_flags >> RT_CULL_TRIS_SHIFT of the blob */
RT_CULL_HD uint32_t rt_entry_triangle(uint32_t t) { return (t << 1) | RT_ENTRY_TAG; }
/* the render kernel's start for a tagged word: a leaf of the one triangle */
RT_CULL_HD uint32_t rt_entry_leaf(uint32_t word) { return RT_REF_LEAF | (1u << RT_REF_COUNT_SHIFT) | (word >> 1); }
/* the allocation with the entry words: the bits, a gate word and an entry word per thread of the pre-pass; pixel i's entry word is word
 * rt_cull_entry_base(plane_words) + i */
RT_CULL_HD size_t rt_cull_entry_base(size_t plane_words) { return rt_cull_alloc_words(plane_words); }
RT_CULL_HD size_t rt_cull_alloc_words_entry(size_t plane_words) { return rt_cull_alloc_words(plane_words) + plane_words * 32; }

/* the cone's box in v units, binary64: centre and radius per axis (signed), and the bounds on |v| */
struct rt_entry_box {
    double c[3], r[3], ahi[3], alo[3];
    double vmin, vmax;       /* max_k min|v_k| <= |v| <= 2 max_k max|v_k| */
    int32_t ok;              /* every axis keeps its sign, everything is inside the guards */
};

RT_CULL_HD rt_entry_box rt_entry_box_of(const rt_cull_cone &c)
{
    rt_entry_box b;
    b.ok = c.ok;
    b.vmin = 0.0; b.vmax = 0.0;
    for (int k = 0; k < 3; k++) {
        if (c.sgn[k] == 0) b.ok = 0;
        const double lo = c.sgn[k] > 0 ? (double)c.alo[k] : -(double)c.ahi[k], hi = c.sgn[k] > 0 ? (double)c.ahi[k] : -(double)c.alo[k];
        b.c[k] = 0.5 * (lo + hi);
        b.r[k] = 0.5 * (hi - lo);
        b.alo[k] = (double)c.alo[k]; b.ahi[k] = (double)c.ahi[k];
        b.vmin = b.alo[k] > b.vmin ? b.alo[k] : b.vmin;
        b.vmax = b.ahi[k] > b.vmax ? b.ahi[k] : b.vmax;
    }
    b.vmax *= 2.0;
    return b;
}

/* a float quantity of every sample, in v units: certainly inside [lo, hi] */
struct rt_entry_iv { double lo, hi; };

/* dot(a, cross(d, s2)) as a linear form of d: its coefficients, and the sum of the magnitudes of its six product terms over the box */
RT_CULL_HD void rt_entry_form_cross(const float a[3], const float s2[3], const rt_entry_box &b, double L[3], double &mag)
{
    const double ax = a[0], ay = a[1], az = a[2], sx = s2[0], sy = s2[1], sz = s2[2];
    L[0] = az * sy - ay * sz;
    L[1] = ax * sz - az * sx;
    L[2] = ay * sx - ax * sy;
    mag = b.ahi[0] * (fabs(az * sy) + fabs(ay * sz)) + b.ahi[1] * (fabs(ax * sz) + fabs(az * sx)) + b.ahi[2] * (fabs(ay * sx) + fabs(ax * sy));
}
RT_CULL_HD rt_entry_iv rt_entry_range(const double L[3], double mag, const rt_entry_box &b)
{
    const double mid = L[0] * b.c[0] + L[1] * b.c[1] + L[2] * b.c[2];
    const double rad = fabs(L[0]) * b.r[0] + fabs(L[1]) * b.r[1] + fabs(L[2]) * b.r[2];
    const double err = RT_ENTRY_E * mag + RT_ENTRY_ABS;
    rt_entry_iv v;
    v.lo = mid - rad - err; v.hi = mid + rad + err;
    return v;
}

enum { RT_ENTRY_REJECTED = 0, RT_ENTRY_MAYBE = 1, RT_ENTRY_HIT = 2 };
struct rt_entry_tri {
    int32_t cls;
    double t_lo, t_hi;       /* the accepted distance in v units (times s): meaningful unless REJECTED; -RT_ENTRY_BIG / RT_ENTRY_BIG: not bounded */
};

/* the triangle `q` (nine floats: p0, s1, s2) against every sample of the box from the origin `o` */
RT_CULL_HD rt_entry_tri rt_entry_classify(const rt_entry_box &b, const float o[3], const float *q)
{
    rt_entry_tri r;
    r.cls = RT_ENTRY_MAYBE; r.t_lo = -RT_ENTRY_BIG; r.t_hi = RT_ENTRY_BIG;
    if (!b.ok) return r;
    const float p0[3] = {q[0], q[1], q[2]}, s1[3] = {q[3], q[4], q[5]}, s2[3] = {q[6], q[7], q[8]};
    float tv[3];
    for (int k = 0; k < 3; k++) {
        if (!rt_cull_finite(p0[k]) || !rt_cull_finite(s1[k]) || !rt_cull_finite(s2[k])) return r;
        if (!(fabsf(p0[k]) <= RT_CULL_HUGE) || !(fabsf(s1[k]) <= RT_CULL_HUGE) || !(fabsf(s2[k]) <= RT_CULL_HUGE)) return r;
        tv[k] = o[k] - p0[k];
    }
    /* the kernel's q_vec = cross(t_vec, s1) and dot(s2, q_vec), operation for operation (rt_vec.h) */
    const float qv[3] = {tv[1] * s1[2] - tv[2] * s1[1], tv[2] * s1[0] - tv[0] * s1[2], tv[0] * s1[1] - tv[1] * s1[0]};
    const float ntx = s2[0] * qv[0], nty = s2[1] * qv[1], ntz = s2[2] * qv[2];
    const float nt = ntx + nty + ntz;
    if (!rt_cull_finite(nt) || !rt_cull_finite(qv[0]) || !rt_cull_finite(qv[1]) || !rt_cull_finite(qv[2])) return r;

    double Ld[3], Lu[3], Lv[3], Ls[3], mag_d, mag_u;
    rt_entry_form_cross(s1, s2, b, Ld, mag_d);
    rt_entry_form_cross(tv, s2, b, Lu, mag_u);
    for (int k = 0; k < 3; k++) { Lv[k] = (double)qv[k]; Ls[k] = Lu[k] + Lv[k]; }
    const double mag_v = b.ahi[0] * fabs(Lv[0]) + b.ahi[1] * fabs(Lv[1]) + b.ahi[2] * fabs(Lv[2]);
    rt_entry_iv det = rt_entry_range(Ld, mag_d, b), nu = rt_entry_range(Lu, mag_u, b), nv = rt_entry_range(Lv, mag_v, b);
    rt_entry_iv ns = rt_entry_range(Ls, mag_u + mag_v, b);
    ns.lo -= RT_ENTRY_ABS; ns.hi += RT_ENTRY_ABS;
    double ntd = (double)nt;
    if (det.hi <= -RT_ENTRY_DET_MIN) {
        /* a negative determinant: everything times -1 */
        rt_entry_iv x;
        x.lo = -det.hi; x.hi = -det.lo; det = x;
        x.lo = -nu.hi; x.hi = -nu.lo; nu = x;
        x.lo = -nv.hi; x.hi = -nv.lo; nv = x;
        x.lo = -ns.hi; x.hi = -ns.lo; ns = x;
        ntd = -ntd;
    } else if (!(det.lo >= RT_ENTRY_DET_MIN)) {
        return r;                                    /* the determinant may vanish: nothing is known, not even the distance */
    }
    if (!(det.hi <= RT_ENTRY_DET_MAX)) return r;
    if (!(ntd > 0.0)) { r.cls = RT_ENTRY_REJECTED; return r; }          /* t <= 0 (a sign is never rounded) */
    r.t_lo = ntd / det.hi * (1.0 - RT_ENTRY_E);
    r.t_hi = ntd / det.lo * (1.0 + RT_ENTRY_E);
    const double eps = (double)RT_EPS_F;
    if (r.t_hi * b.vmax * (1.0 + RT_ENTRY_E) < eps) { r.cls = RT_ENTRY_REJECTED; return r; }
    if (nu.hi <= -RT_ENTRY_DET_MIN || nv.hi <= -RT_ENTRY_DET_MIN) { r.cls = RT_ENTRY_REJECTED; return r; }
    const double umax = fmax(fabs(nu.lo), fabs(nu.hi)) / det.lo, vmax = fmax(fabs(nv.lo), fabs(nv.hi)) / det.lo;
    const double slack = RT_ENTRY_E * (umax + vmax), wmargin = RT_ENTRY_E * (1.0 + umax);
    const double s_lo = fmin(ns.lo / det.lo, ns.lo / det.hi) - slack, s_hi = fmax(ns.hi / det.lo, ns.hi / det.hi) + slack;
    if (s_lo - 1.0 > wmargin) { r.cls = RT_ENTRY_REJECTED; return r; }
    if (nu.lo >= 0.0 && nv.lo >= 0.0 && 1.0 - s_hi >= wmargin && r.t_lo * b.vmin * (1.0 - RT_ENTRY_E) > eps * (1.0 + RT_ENTRY_E) &&
        r.t_hi * b.vmax * (1.0 + RT_ENTRY_E) < 0.5 * (double)RT_INF_F)
        r.cls = RT_ENTRY_HIT;
    return r;
}

/* the entry bound e (v units) of a box that every sample certainly enters, RT_ENTRY_BIG if that is not certain */
RT_CULL_HD double rt_entry_box_bound(const rt_cull_cone &c, const rt_entry_box &eb, const float *bx)
{
    if (!eb.ok) return RT_ENTRY_BIG;
    double N[3], F[3];
    for (int k = 0; k < 3; k++) {
        const float b0 = bx[k], b1 = bx[3 + k];
        if (!rt_cull_finite(b0) || !rt_cull_finite(b1) || !(fabsf(b0) <= RT_CULL_HUGE) || !(fabsf(b1) <= RT_CULL_HUGE)) return RT_ENTRY_BIG;
        const float a0 = b0 - c.o[k], a1 = b1 - c.o[k];
        const float lo = a0 < a1 ? a0 : a1, hi = a0 < a1 ? a1 : a0;
        N[k] = c.sgn[k] > 0 ? (double)lo : -(double)hi;
        F[k] = c.sgn[k] > 0 ? (double)hi : -(double)lo;
        if (!(F[k] >= (double)RT_CULL_TINY)) return RT_ENTRY_BIG;
        if (N[k] > 0.0 && !(N[k] >= (double)RT_CULL_TINY)) return RT_ENTRY_BIG;
        if (!(N[k] * (1.0 + RT_ENTRY_E) < F[k] * (1.0 - RT_ENTRY_E))) return RT_ENTRY_BIG;
    }
    double e = 0.0;
    for (int i = 0; i < 3; i++) {
        if (!(N[i] > 0.0)) continue;
        const double near_i = N[i] / eb.alo[i] * (1.0 + RT_ENTRY_E);
        for (int j = 0; j < 3; j++)
            if (j != i && !(near_i < F[j] / eb.ahi[j] * (1.0 - RT_ENTRY_E))) return RT_ENTRY_BIG;
        e = near_i > e ? near_i : e;
    }
    return e;
}

/* a path bound as the float the walk's stack keeps: rounded up */
RT_CULL_HD float rt_entry_bound_f(double e)
{
    if (!(e < 1e30)) return RT_INF_F * 4.0f;
    return (float)(e * (1.0 + RT_ENTRY_E)) + 1e-37f;
}

/* what the walk learns of the triangles it meets */
struct rt_entry_state {
    int32_t cand;            /* the certainly hit triangle with the least t_hi whose path is certain, -1: none */
    double cand_hi;
    double lo1, lo2;         /* the two least t_lo among the triangles not certainly rejected, and whose the least is */
    int32_t id1;
    int32_t seen;            /* triangles not certainly rejected */
    int32_t leaves;          /* leaves with triangles reached */
};

/* The entry word of a cone for mesh `mesh` of a flattened scene whose triangles start at 16-byte unit off_tris.  `stack` holds the pending
 * references, `bounds` their path bounds (float bits).  Anything unexpected answers 0. */
template <class Stack>
RT_CULL_HD uint32_t rt_entry_word(const rt_cull_cone &c, const float *blob, int32_t off_nodes, int32_t num_nodes, int32_t off_meshes, int32_t mesh, int32_t off_tris,
                                  int32_t num_tris, Stack stack, Stack bounds, int64_t *tris_classified = nullptr)
{
    const rt_entry_box eb = rt_entry_box_of(c);
    if (!eb.ok) return 0u;
    const float *m0 = blob + 4 * ((size_t)off_meshes + 2 * (size_t)mesh);
    if (rt_cull_box_missed(c, m0[0], m0[1], m0[2], m0[3], m0[4], m0[5])) return 0u;
    rt_entry_state st;
    st.cand = -1; st.cand_hi = RT_ENTRY_BIG; st.lo1 = RT_ENTRY_BIG; st.lo2 = RT_ENTRY_BIG; st.id1 = -1; st.seen = 0; st.leaves = 0;
    int sp = 0;
    uint32_t cur = rt_cull_bits(m0[6]);
    float path = 0.0f;
    for (;;) {
        if (cur & RT_REF_LEAF) {
            const uint32_t count = (cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX, start = cur & RT_REF_START_MASK;
            if (count != 0u) st.leaves++;
            for (uint32_t k = 0; k < count; k++) {
                const uint32_t idx = start + k;
                if (idx >= (uint32_t)num_tris) return 0u;
                if (tris_classified) (*tris_classified)++;
                const rt_entry_tri t = rt_entry_classify(eb, c.o, blob + 4 * ((size_t)off_tris + 3 * (size_t)idx));
                if (t.cls == RT_ENTRY_REJECTED) continue;
                st.seen++;
                if (t.t_lo < st.lo1) { st.lo2 = st.lo1; st.lo1 = t.t_lo; st.id1 = (int32_t)idx; }
                else if (t.t_lo < st.lo2) st.lo2 = t.t_lo;
                if (t.cls == RT_ENTRY_HIT && (double)path < t.t_lo && t.t_hi < st.cand_hi) { st.cand = (int32_t)idx; st.cand_hi = t.t_hi; }
            }
            if (sp == 0) break;
            --sp;
            cur = stack[sp];
            { const uint32_t bits = bounds[sp]; __builtin_memcpy(&path, &bits, 4); }
            continue;
        }
        const uint32_t idx = cur & RT_REF_NODE_MASK;
        if (idx >= (uint32_t)num_nodes) return 0u;
        const float *n = blob + 4 * ((size_t)off_nodes + 4 * (size_t)idx);
        const bool l_missed = rt_cull_box_missed(c, n[0], n[1], n[2], n[3], n[4], n[5]);
        const bool r_missed = rt_cull_box_missed(c, n[6], n[7], n[8], n[9], n[10], n[11]);
        const uint32_t lref = rt_cull_bits(n[12]), rref = rt_cull_bits(n[13]);
        float l_path = path, r_path = path;
        if (!l_missed) { const float e = rt_entry_bound_f(rt_entry_box_bound(c, eb, n)); l_path = e > path ? e : path; }
        if (!r_missed) { const float e = rt_entry_bound_f(rt_entry_box_bound(c, eb, n + 6)); r_path = e > path ? e : path; }
        if (!l_missed && !r_missed) {
            if (sp >= RT_CULL_STACK) return 0u;
            stack[sp] = rref;
            bounds[sp] = rt_cull_bits(r_path);
            sp++;
            cur = lref; path = l_path;
        } else if (!l_missed) {
            cur = lref; path = l_path;
        } else if (!r_missed) {
            cur = rref; path = r_path;
        } else {
            if (sp == 0) break;
            --sp;
            cur = stack[sp];
            { const uint32_t bits = bounds[sp]; __builtin_memcpy(&path, &bits, 4); }
        }
    }
    if (st.leaves == 0) return 0u;                       /* the bit plane's pixel */
    if (st.seen == 0) return RT_ENTRY_NOTHING;
    if (st.cand < 0) return 0u;
    const double others = st.id1 == st.cand ? st.lo2 : st.lo1;
    return others > st.cand_hi ? rt_entry_triangle((uint32_t)st.cand) : 0u;
}

/* ================= THE SUB-ENTRY WORDS: the same word per sub-box of the jitter cube, for the pixels whose own word is 0 =================
 * A pixel whose cone straddles a triangle edge or a silhouette, or has a direction interval that touches zero, has the word 0 although most
 * of its samples are unambiguous.  The jitter cube [-J, J]^3 is split into RT_SUB_S^3 = 64 closed sub-boxes; sub-interval j of an axis is
 * [tau_j, tau_j+1] with tau = -J, -J/2, 0, J/2, J, five exact floats.  Rounding is monotone, so for a jitter off_k in sub-interval j
 * v_k = fl(P_k + off_k) lies in [fl(P_k + tau_j), fl(P_k + tau_j+1)] - rt_cull.h's own argument - and the SUB-CONE built from those two
 * floats per axis (rt_sub_cone_of) holds every sample whose jitter falls in the sub-box.  rt_entry_word runs on the sub-cone as it is: no
 * new predicate, no new error bound, and a sub-word `triangle T`, `nothing` or 0 has the meaning and the bit-identity argument above for
 * those samples.  A jitter on a threshold belongs to both neighbouring closed sub-boxes: either word is valid for it.
 *
 * THE INDEX of a sample (rt_sub_index) is computed from the very floats px_gen adds to the direction; this one definition serves the
 * render kernel, the host hooks and the tests.
 *
 * THE STORAGE.  Behind the entry words, in the same allocation (rt_sub_alloc_words): a header of RT_SUB_HEADER words whose first is the slot
 * counter, then `cap` words - the pixel of each slot - and then `cap` tables of 64 sub-words; cap = rt_sub_cap(plane words), an eighth of
 * the pre-pass's threads.  A pixel with a table carries its slot in its entry word as (slot + 1) << 2 | 2 (rt_sub_slot_word): bit 0 is
 * clear, so it is no `triangle`; bits 1..0 are 10 and the rest is not 0, so it is neither `nothing` (2) nor 0.  Only an unflagged pixel
 * whose word is 0 gets a slot; one that finds the tables full keeps 0.  Slot order is whatever the device's atomics make it: the image does
 * not depend on it.
 *
 * WHAT A TABLE STORES.  The render kernel has one register for a pixel's gate word, entry word or slot word (rt_pixel.h: a second one held
 * across the traversal loops costs it two VGPRs), so a table pixel's gate word rides in its table: a sub-word `triangle T` is stored as it
 * is, `nothing` as RT_SUB_NOTHING - all ones: T << 1 | 1 of a triangle no leaf can name, and no gate word, whose bit 0 is clear - and 0,
 * not known, as the pixel's gate word, which is what such a sample traverses with.  One load then brings whichever the sample needs
 * (rt_sub_stored).  rt_sub_word_of gives the sub-word back: that is what the debug hooks report. */
#define RT_SUB_NOTHING 0xffffffffu
RT_CULL_HD uint32_t rt_sub_stored(uint32_t sub_word, uint32_t gate_word) { return sub_word == 0u ? gate_word & ~RT_ENTRY_TAG : sub_word == RT_ENTRY_NOTHING ? RT_SUB_NOTHING : sub_word; }
RT_CULL_HD uint32_t rt_sub_word_of(uint32_t stored) { return stored == RT_SUB_NOTHING ? RT_ENTRY_NOTHING : (stored & RT_ENTRY_TAG) ? stored : 0u; }
static_assert((RT_SUB_NOTHING >> 1) > RT_REF_START_MASK, "no leaf names the triangle RT_SUB_NOTHING is tagged with");
#define RT_SUB_S 4
#define RT_SUB_WORDS 64                  /* RT_SUB_S^3 sub-words per table */
#define RT_SUB_HEADER 4                  /* words in front of the slots' pixels: the slot counter, three spare */
#define RT_CULL_WITH_SUBENTRY 8          /* rt_launch_cull's view_flags: queue the refinement; without RT_CULL_WITH_ENTRY the pre-pass itself is not run (the plane has this view's words already) */
/* The samples per pixel (spp x frames) from which a view's FIRST launch queues the refinement; below it the view's first reuse does
 * (rt_cull_host::Plan::refine; RT_AMD_SUBENTRY_SAMPLES overrides).  Set where the measured gain of one launch is twice the measured refinement
 * time: DESIGN.md section 24, "The sub-entry words", has the two figures. */
#define RT_SUB_THRESHOLD_SAMPLES 2200
static_assert(RT_CULL_WITH_SUBENTRY < (1 << RT_CULL_TRIS_SHIFT), "the flag sits below the triangles' offset");
RT_CULL_HD uint32_t rt_sub_slot_word(uint32_t slot) { return ((slot + 1u) << 2) | 2u; }
/* slot + 1 of a word that carries one, else 0 */
RT_CULL_HD uint32_t rt_sub_slot_plus1(uint32_t word) { return (word & 3u) == 2u ? word >> 2 : 0u; }
static_assert((((0u + 1u) << 2 | 2u) & RT_ENTRY_TAG) == 0u && ((0u + 1u) << 2 | 2u) != RT_ENTRY_NOTHING && (RT_ENTRY_NOTHING >> 2) == 0u && (RT_ENTRY_NOTHING & 3u) == 2u,
              "a slot word reads as neither `triangle` nor `nothing` nor 0, and `nothing` carries no slot");
RT_CULL_HD size_t rt_sub_cap(size_t plane_words) { return plane_words * 4; }
RT_CULL_HD size_t rt_sub_header_base(size_t plane_words) { return rt_cull_alloc_words_entry(plane_words); }
RT_CULL_HD size_t rt_sub_pixels_base(size_t plane_words) { return rt_sub_header_base(plane_words) + RT_SUB_HEADER; }
RT_CULL_HD size_t rt_sub_tables_base(size_t plane_words) { return rt_sub_pixels_base(plane_words) + rt_sub_cap(plane_words); }
RT_CULL_HD size_t rt_sub_alloc_words(size_t plane_words) { return rt_sub_tables_base(plane_words) + rt_sub_cap(plane_words) * RT_SUB_WORDS; }

/* tau_j, j = 0 .. RT_SUB_S */
RT_CULL_HD float rt_sub_tau(int j)
{
    return j <= 0 ? -RT_CULL_JITTER : j == 1 ? -0.5f * RT_CULL_JITTER : j == 2 ? 0.0f : j == 3 ? 0.5f * RT_CULL_JITTER : RT_CULL_JITTER;
}
/* the sub-interval of one jitter component, and the sub-box of a sample's three */
RT_CULL_HD uint32_t rt_sub_axis_index(float off)
{
    return (uint32_t)(off >= -0.5f * RT_CULL_JITTER) + (uint32_t)(off >= 0.0f) + (uint32_t)(off >= 0.5f * RT_CULL_JITTER);
}
RT_CULL_HD uint32_t rt_sub_index(float off_x, float off_y, float off_z)
{
    return rt_sub_axis_index(off_x) + 4u * rt_sub_axis_index(off_y) + 16u * rt_sub_axis_index(off_z);
}
/* the cone of the samples of primary direction P whose jitter falls in sub-box idx: rt_cull_cone_of with the sub-interval's ends for -J, J */
RT_CULL_HD rt_cull_cone rt_sub_cone_of(const float P[3], const float cam_pos[3], uint32_t idx)
{
    rt_cull_cone c;
    c.ok = 1;
    float largest = 0.0f;
    for (int k = 0; k < 3; k++) {
        const int j = (int)((idx >> (2 * k)) & 3u);
        const float lo = P[k] + rt_sub_tau(j), hi = P[k] + rt_sub_tau(j + 1);
        c.o[k] = cam_pos[k];
        if (!rt_cull_finite(lo) || !rt_cull_finite(hi) || !rt_cull_finite(cam_pos[k]) || !(fabsf(cam_pos[k]) <= RT_CULL_HUGE)) c.ok = 0;
        c.sgn[k] = lo >= RT_CULL_TINY ? 1 : (hi <= -RT_CULL_TINY ? -1 : 0);
        c.alo[k] = c.sgn[k] > 0 ? lo : -hi;
        c.ahi[k] = c.sgn[k] > 0 ? hi : -lo;
        const float a = fmaxf(fabsf(lo), fabsf(hi));
        largest = a > largest ? a : largest;
    }
    if (!(largest >= 0.25f && largest <= 4.0f)) c.ok = 0;
    return c;
}
/* does a pixel get a table?  An unflagged one whose own word is 0 (or a slot of an earlier refinement), in a jittered view */
RT_CULL_HD bool rt_sub_wants_table(bool flagged, uint32_t entry_word) { return !flagged && (entry_word == 0u || rt_sub_slot_plus1(entry_word) != 0u); }

/* ---- the kernel's triangle test (tri_closer_lanes, rt_intersect.h) restated for host code, operation for operation: accepted iff
 * t > RT_EPS_F, min(u, v, w) >= 0 (a NaN fails) and t < best.  What tests/sanitize/entry_soundness.cpp and the estimate walk. */
RT_CULL_HD bool rt_entry_tri_closer(const float *q, const float o[3], const float d[3], float best, float &t_out)
{
    const float p0[3] = {q[0], q[1], q[2]}, s1[3] = {q[3], q[4], q[5]}, s2[3] = {q[6], q[7], q[8]};
    const float pv[3] = {d[1] * s2[2] - d[2] * s2[1], d[2] * s2[0] - d[0] * s2[2], d[0] * s2[1] - d[1] * s2[0]};
    const float dx = s1[0] * pv[0], dy = s1[1] * pv[1], dz = s1[2] * pv[2];
    const float det = dx + dy + dz;
    const float inv_det = 1.0f / det;
    const float tv[3] = {o[0] - p0[0], o[1] - p0[1], o[2] - p0[2]};
    const float ux = tv[0] * pv[0], uy = tv[1] * pv[1], uz = tv[2] * pv[2];
    const float u = (ux + uy + uz) * inv_det;
    const float qv[3] = {tv[1] * s1[2] - tv[2] * s1[1], tv[2] * s1[0] - tv[0] * s1[2], tv[0] * s1[1] - tv[1] * s1[0]};
    const float vx = d[0] * qv[0], vy = d[1] * qv[1], vz = d[2] * qv[2];
    const float v = (vx + vy + vz) * inv_det;
    const float w = 1.0f - u - v;
    const float tx = s2[0] * qv[0], ty = s2[1] * qv[1], tz = s2[2] * qv[2];
    const float t = (tx + ty + tz) * inv_det;
    t_out = t;
    return t > RT_EPS_F && u >= 0.0f && v >= 0.0f && w >= 0.0f && t < best;
}

/* the leaf functor of rt_cull_walk that tests a leaf's triangles as the kernel's leaf loop does, counting the tests */
struct rt_entry_leaf_tests {
    const float *tris;       /* the blob's triangles */
    const float *o, *d;
    int64_t *tests;          /* (the walk takes the functor by value) */
    RT_CULL_HD_MEMBER void operator()(uint32_t ref, float &best, int32_t &prim) const
    {
        const uint32_t count = (ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX, start = ref & RT_REF_START_MASK;
        for (uint32_t k = 0; k < count; k++) {
            float t;
            (*tests)++;
            if (rt_entry_tri_closer(tris + 12 * (size_t)(start + k), o, d, best, t)) { best = t; prim = (int32_t)(start + k); }
        }
    }
};

#endif
