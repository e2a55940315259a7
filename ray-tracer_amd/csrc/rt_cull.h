/*
 * rt_cull.h — the primary-ray cull: one bit per pixel of a view, "no primary ray of this pixel can reach a leaf of any mesh".  Host and
 * device: the predicate (rt_cull_cone, rt_cull_box_missed), the walk over a flattened scene (rt_cull_no_leaf), the slab test's three forms
 * restated for the host (rt_cull_slab_*: rt_intersect.h is device code) and the host's bookkeeping of the plane (rt_cull_host); the
 * pre-pass kernel's launcher is rt_launch.h's rt_launch_cull (defined in rt_cull_kernel.h).  DESIGN.md section 24 has the argument and the figures.
 *
 * WHY THE FRAMES STAY BIT-IDENTICAL.  A primary ray of a flagged pixel fails the float slab test of at least one box on every root-to-leaf
 * path of every mesh, so the traversal that the render kernel would run for it tests no triangle and ends with w_prim == -1: its merge is
 * a no-op.  A traversal draws no random numbers.  Skipping it therefore changes only the cost counters and the "this pixel traverses" bit
 * of Px::frame_steps, which feed the tile schedule and not the image.
 *
 * THE DIRECTIONS OF A PIXEL.  px_fetch (rt_pixel.h) computes P = normalised((tl + (du * px + dv * py)) - cam_pos) and px_gen, for every
 * sample, d = normalised(P + off) with off_k = rt_jitter(...) in [-J, J], J = 0.001f (rt_rng.h: fmaf(u, 2J, -J), u in [0, 1]); without
 * antialias d = P.  With v = fl(P + off): rounding to nearest is monotone, so v_k lies in [fl(P_k - J), fl(P_k + J)], two float operations
 * the predicate repeats - no margin is needed for the jitter or the add.  d_k = fl(v_k * s) with s = fl(1 / fl(sqrt(m))) > 0 the SAME
 * number for the three components of one sample, and inv_k = fl(1 / d_k).
 *
 * THE ERROR BOUND.  Of a box [b0, b1] and the origin o the slab test forms t = fl(A * inv_k) with A = fl(b - o): the two A of an axis do
 * not depend on the direction and are computed here exactly as there.  Float multiplication is monotone, so the smaller (near) and larger
 * (far) product of an axis are fl(N * |inv_k|) and fl(F * |inv_k|) with (N, F) = (min A, max A) for v_k > 0 and (-max A, -min A) for
 * v_k < 0.  With u = 2^-24 and every intermediate a normal number (guarded below: |v_k| >= 2^-40, max |v| in [1/4, 4], |b|, |o| <= 2^39,
 * N and F used only from 2^-40 up - products then lie between 2^-46 and 2^85),
 *     near_i >= N_i / (|v_i| s) * (1 - u)^2 / (1 + u)          far_j <= F_j / (|v_j| s) * (1 + u)^2 / (1 - u)
 * (one rounding each in d, inv and the product).  s cancels: near_i >= far_j for EVERY sample of the pixel if
 *     N_i * min|v_j| * (1 - E) >= F_j * max|v_i| * (1 + E),      E = 2^-22 = 4u,
 * since (1 + E) / (1 - E) > 1 + 8u > ((1 + u) / (1 - u))^3 + 2^-40; both sides are evaluated in binary64, where a product of two floats is
 * exact and the two further roundings are below 2^-52 each.  Every slab form computes tmin >= near_i (a maximum over the axes, from 0;
 * fmaxf only ever drops a NaN of ANOTHER axis) and tmax <= far_j, and accepts only if tmin < tmax (box_test), tmin < min(tmax, best)
 * (box_enter) or the equivalent med3 chain (box_enter_med3, for rays without a zero component: rt_intersect.h has that proof).  So
 * near_i >= far_j for one pair of axes i != j, or F_j <= 0 for one axis (then far_j <= 0 exactly - a sign is never rounded - and
 * tmax > 0 / tmin < tmax with tmin >= 0 fail), means no form accepts the box for any sample and any `best`: "certainly missed".
 * An axis whose direction interval contains zero or comes closer to it than 2^-40 is not used (in either role); a NaN, an infinity or a
 * number outside the guards anywhere makes the answer "maybe".  "Maybe" is always safe.
 * tests/sanitize/cull_soundness.cpp looks for a counter-example among 10^6 (pixel, jitter, box) triples with adversarial boxes.
 */
#ifndef RT_CULL_H
#define RT_CULL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_device_scene.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
#define RT_CULL_HD __host__ __device__ static inline
#define RT_CULL_HD_MEMBER __host__ __device__
#else
#define RT_CULL_HD static inline
#define RT_CULL_HD_MEMBER
#endif
/* (the arithmetic below is px_fetch's and the slab test's, two roundings per a * b + c: every translation unit that includes this is built
 * with -ffp-contract=off, like the kernels) */

#define RT_CULL_JITTER 0.001f            /* rt_jitter's range (rt_rng.h) */
#define RT_CULL_TINY 9.094947017729282e-13f      /* 2^-40: the least |v_k|, N and F the bound is used from */
#define RT_CULL_HUGE 549755813888.0f             /* 2^39: the largest |b|, |o| */
#ifndef RT_CULL_E                        /* (tests/sanitize/gate_soundness.cpp is also built with the margin taken away, to show that it finds the loss) */
#define RT_CULL_E 2.384185791015625e-07          /* E = 2^-22 (binary64) */
#endif
#define RT_CULL_STACK 16                 /* pending siblings of the walk: at most one per level of a depth-RT_BVH_DEPTH tree */
static_assert(RT_CULL_STACK > RT_STACK_ENTRIES, "the walk's stack holds a pending sibling per tree level");

RT_CULL_HD uint32_t rt_cull_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_CULL_HD bool rt_cull_finite(float f) { return (rt_cull_bits(f) & 0x7f800000u) != 0x7f800000u; }

/* words of a W x H plane: 32 pixels to a word, pixel py * W + px; whole pairs of words (a wave of the pre-pass writes two) */
RT_CULL_HD size_t rt_cull_words(int32_t width, int32_t height) { return (((size_t)width * (size_t)height + 63) / 64) * 2; }

/* the primary direction of pixel (px, py): px_fetch's float operations in px_fetch's order (rt_pixel.h; rt_rcp_sqrt(m) == 1.0f / sqrtf(m)) */
RT_CULL_HD void rt_cull_primary(const float cam[12], int px, int py, float P[3])
{
    float w[3];
    for (int k = 0; k < 3; k++) {
        const float plane_point = cam[6 + k] * (float)px + cam[9 + k] * (float)py;
        w[k] = (cam[3 + k] + plane_point) - cam[k];
    }
    const float m = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const float inv = 1.0f / sqrtf(m);
    for (int k = 0; k < 3; k++) P[k] = w[k] * inv;
}

/* every direction px_gen can produce for one pixel, before the normalisation: per axis the sign and the range of |v_k| */
struct rt_cull_cone {
    float o[3];              /* the rays' origin: the camera position */
    float alo[3], ahi[3];    /* min |v_k| and max |v_k| */
    int32_t sgn[3];          /* +1 / -1: v_k keeps that sign and |v_k| >= RT_CULL_TINY; 0: the axis is not used */
    int32_t ok;              /* 0: something is not a number or outside the guards - every box is "maybe" */
};

RT_CULL_HD rt_cull_cone rt_cull_cone_of(const float P[3], const float cam_pos[3], int antialias)
{
    rt_cull_cone c;
    c.ok = 1;
    float largest = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float lo = antialias ? P[k] - RT_CULL_JITTER : P[k], hi = antialias ? P[k] + RT_CULL_JITTER : P[k];
        c.o[k] = cam_pos[k];
        if (!rt_cull_finite(lo) || !rt_cull_finite(hi) || !rt_cull_finite(cam_pos[k]) || !(fabsf(cam_pos[k]) <= RT_CULL_HUGE)) c.ok = 0;
        c.sgn[k] = lo >= RT_CULL_TINY ? 1 : (hi <= -RT_CULL_TINY ? -1 : 0);
        c.alo[k] = c.sgn[k] > 0 ? lo : -hi;
        c.ahi[k] = c.sgn[k] > 0 ? hi : -lo;
        const float a = fmaxf(fabsf(lo), fabsf(hi));
        largest = a > largest ? a : largest;
    }
    if (!(largest >= 0.25f && largest <= 4.0f)) c.ok = 0;      /* m, s = 1 / sqrt(m) and every d_k = v_k * s are normal numbers */
    return c;
}

/* "certainly missed": no slab form accepts the box (bx0 .. bz1 as the kernels are handed it) for any direction of the cone and any `best` */
RT_CULL_HD bool rt_cull_box_missed(const rt_cull_cone &c, float bx0, float by0, float bz0, float bx1, float by1, float bz1)
{
    if (!c.ok) return false;
    const float b0[3] = {bx0, by0, bz0}, b1[3] = {bx1, by1, bz1};
    float N[3], F[3];
    for (int k = 0; k < 3; k++) {
        if (!rt_cull_finite(b0[k]) || !rt_cull_finite(b1[k]) || !(fabsf(b0[k]) <= RT_CULL_HUGE) || !(fabsf(b1[k]) <= RT_CULL_HUGE)) return false;
        const float a0 = b0[k] - c.o[k], a1 = b1[k] - c.o[k];
        const float lo = a0 < a1 ? a0 : a1, hi = a0 < a1 ? a1 : a0;
        N[k] = c.sgn[k] > 0 ? lo : -hi;
        F[k] = c.sgn[k] > 0 ? hi : -lo;
    }
    for (int j = 0; j < 3; j++)
        if (c.sgn[j] != 0 && F[j] <= 0.0f) return true;                 /* the box is behind the origin along axis j */
    for (int i = 0; i < 3; i++) {
        if (c.sgn[i] == 0 || !(N[i] >= RT_CULL_TINY)) continue;
        for (int j = 0; j < 3; j++) {
            if (j == i || c.sgn[j] == 0 || !(F[j] >= RT_CULL_TINY)) continue;
            /* the ray leaves slab j before it enters slab i, whatever the sample */
            if ((double)N[i] * (double)c.alo[j] * (1.0 - RT_CULL_E) >= (double)F[j] * (double)c.ahi[i] * (1.0 + RT_CULL_E)) return true;
        }
    }
    return false;
}

/* Does the cone reach no leaf (with triangles) of any mesh of a flattened scene?  `blob` is the scene blob as floats (rt_device_scene.h),
 * the offsets in 16-byte units.  The walk is the traversal's with "maybe" for "entered": from each mesh's root box down, a node's two child
 * boxes from the node, a pending sibling on a small stack; it ends at the first leaf.  A reference outside the nodes or a stack that would
 * overflow (neither happens in a tree the flattener or the rebuild made) answers "a leaf may be reached".  *steps, if given, counts the
 * nodes visited. */
/* (Stack: RT_CULL_STACK words behind operator[] - an array on the host, a column of LDS in the kernel, which keeps no private memory) */
struct rt_cull_local_stack {
    uint32_t e[RT_CULL_STACK];
    RT_CULL_HD_MEMBER uint32_t &operator[](int i) { return e[i]; }
};
template <class Stack>
RT_CULL_HD bool rt_cull_no_leaf(const rt_cull_cone &c, const float *blob, int32_t off_nodes, int32_t num_nodes, int32_t off_meshes, int32_t num_meshes, Stack stack,
                                int32_t *steps = nullptr, bool stop_at_leaf = true)
{
    bool none = true;
    if (!c.ok) return false;
    for (int32_t m = 0; m < num_meshes; m++) {
        const float *m0 = blob + 4 * ((size_t)off_meshes + 2 * (size_t)m), *m1 = m0 + 4;
        if (rt_cull_box_missed(c, m0[0], m0[1], m0[2], m0[3], m1[0], m1[1])) continue;
        int sp = 0;
        uint32_t cur = rt_cull_bits(m1[2]);
        for (;;) {
            if (cur & RT_REF_LEAF) {
                if (((cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX) != 0u) {
                    none = false;
                    if (stop_at_leaf) return false;
                }
                if (sp == 0) break;
                cur = stack[--sp];
                continue;
            }
            const uint32_t idx = cur & RT_REF_NODE_MASK;
            if (idx >= (uint32_t)num_nodes) return false;
            if (steps) (*steps)++;
            const float *n = blob + 4 * ((size_t)off_nodes + 4 * (size_t)idx);
            const bool l_missed = rt_cull_box_missed(c, n[0], n[1], n[2], n[3], n[4], n[5]);
            const bool r_missed = rt_cull_box_missed(c, n[6], n[7], n[8], n[9], n[10], n[11]);
            const uint32_t lref = rt_cull_bits(n[12]), rref = rt_cull_bits(n[13]);
            if (!l_missed && !r_missed) {
                if (sp >= RT_CULL_STACK) return false;
                stack[sp++] = rref;
                cur = lref;
            } else if (!l_missed) {
                cur = lref;
            } else if (!r_missed) {
                cur = rref;
            } else {
                if (sp == 0) break;
                cur = stack[--sp];
            }
        }
    }
    return none;
}

/* ================= THE SUBTREE CULL: the same question one level down, per gate of the one mesh (rt_device_scene.h: rt_node, RT_GATE_COUNT) =====
 * Beside its bit a pixel gets a word: bit g is set iff gate g is DEAD for the pixel's cone.  A reference is dead when its box is certainly
 * missed (rt_cull_box_missed of the box its parent holds for it), or it is the empty leaf, or it is an internal node whose two references are
 * both dead - so no cone-live path leads from it to a leaf with triangles - or the reference above it is dead (which only spares the walk:
 * nothing below a dead reference is reached).  There is no new predicate and no new error bound.  The render kernel that reads the plane
 * (rt_descend_pop<.., GATES>, rt_traverse.h) does not enter a dead gate with a PRIMARY ray of the pixel; bounce rays are never gated.
 *
 * WHY THE FRAMES STAY BIT-IDENTICAL.  Below a dead reference every root-to-leaf path has a box that no slab form accepts for any sample of
 * the pixel and any `best` (the bound above, unchanged), or ends in the empty leaf.  So the ungated traversal of that subtree tests no
 * triangle: w_best and w_prim do not move, and whatever it pushes it pops or refuses before it returns to the entry below.  Not entering
 * the reference leaves the lane in the state the ungated traversal reaches after the subtree:
 *   - had the dead child been visited first and its sibling deferred, the sibling was pushed with dist < best and best has not changed when
 *     it is popped, so the pop is a take (dist < best takes through a chain edge too): going to the sibling directly is the same decision;
 *   - had the dead child been the deferred one, its later pop, taken or refused, changes nothing;
 *   - with both children dead the node is a dead end and pops, as the ungated traversal does after two fruitless subtrees.
 * A traversal draws no random numbers.  Only the cost counters change, which feed the tile schedule and not the image.
 * tests/sanitize/gate_soundness.cpp walks both traversals side by side and compares the triangles tested and the result.
 *
 * THE WORDS sit behind the bit plane in the same allocation: pixel i's word is word rt_cull_words(W, H) + i; the allocation is
 * rt_cull_alloc_words(rt_cull_words(W, H)) words, a word for every thread of the pre-pass. */
#define RT_CULL_ANTIALIAS 1              /* rt_launch_cull's view_flags: the view's rays are jittered ... */
#define RT_CULL_WITH_GATES 2             /* ... and the gate words are to be computed (else every one is written as 0) */
RT_CULL_HD size_t rt_cull_alloc_words(size_t plane_words) { return plane_words + plane_words * 32; }

/* no cone-live path from `ref` (whose own box is not missed) to a leaf with triangles?  rt_cull_no_leaf's walk from a reference, on the stack's
 * entries from `base` up; a reference outside the nodes or a full stack answers "a leaf may be reached" */
template <class Stack>
RT_CULL_HD bool rt_cull_ref_no_leaf(const rt_cull_cone &c, const float *blob, int32_t off_nodes, int32_t num_nodes, uint32_t ref, Stack &stack, int base)
{
    int sp = base;
    uint32_t cur = ref;
    for (;;) {
        if (cur & RT_REF_LEAF) {
            if (((cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX) != 0u) return false;
            if (sp == base) return true;
            cur = stack[--sp];
            continue;
        }
        const uint32_t idx = cur & RT_REF_NODE_MASK;
        if (idx >= (uint32_t)num_nodes) return false;
        const float *n = blob + 4 * ((size_t)off_nodes + 4 * (size_t)idx);
        const bool l_missed = rt_cull_box_missed(c, n[0], n[1], n[2], n[3], n[4], n[5]);
        const bool r_missed = rt_cull_box_missed(c, n[6], n[7], n[8], n[9], n[10], n[11]);
        const uint32_t lref = rt_cull_bits(n[12]), rref = rt_cull_bits(n[13]);
        if (!l_missed && !r_missed) {
            if (sp >= RT_CULL_STACK) return false;
            stack[sp++] = rref;
            cur = lref;
        } else if (!l_missed) {
            cur = lref;
        } else if (!r_missed) {
            cur = rref;
        } else {
            if (sp == base) return true;
            cur = stack[--sp];
        }
    }
}

/* The gate word of a cone for mesh `mesh` of a flattened scene: bit g set iff gate g is dead.  Walks the nodes that hold gates (a reference
 * without a gate has none below it: the numbering is breadth-first) with the pending ones on the stack, a dead parent marked in the entry's
 * chain bit, and asks rt_cull_ref_no_leaf about every gate that is neither below a dead one nor missed.  Anything unexpected (a cone that is
 * not ok, a reference outside the nodes, a full stack) leaves bits clear: "not dead" is always safe. */
#define RT_CULL_DEAD_ABOVE RT_REF_CHAIN
template <class Stack>
RT_CULL_HD uint32_t rt_cull_gate_word(const rt_cull_cone &c, const float *blob, int32_t off_nodes, int32_t num_nodes, int32_t off_meshes, int32_t mesh, Stack stack)
{
    if (!c.ok) return 0u;
    const uint32_t root = rt_cull_bits(blob[4 * ((size_t)off_meshes + 2 * (size_t)mesh + 1) + 2]);
    if (root & RT_REF_LEAF) return 0u;
    uint32_t word = 0u;
    int sp = 0;
    uint32_t cur = root & RT_REF_NODE_MASK;
    {
        /* (a cone that misses the root box: every gate is below a dead reference) */
        const float *m0 = blob + 4 * ((size_t)off_meshes + 2 * (size_t)mesh);
        if (rt_cull_box_missed(c, m0[0], m0[1], m0[2], m0[3], m0[4], m0[5])) cur |= RT_CULL_DEAD_ABOVE;
    }
    for (;;) {
        const uint32_t idx = cur & RT_REF_NODE_MASK;
        if (idx >= (uint32_t)num_nodes) return word;
        const float *n = blob + 4 * ((size_t)off_nodes + 4 * (size_t)idx);
        for (int side = 0; side < 2; side++) {
            const uint32_t gate = rt_cull_bits(n[14 + side]) & ~1u;
            if (gate == 0u) continue;
            const uint32_t ref = rt_cull_bits(n[12 + side]);
            const float *b = n + 6 * side;
            bool dead = (cur & RT_CULL_DEAD_ABOVE) != 0u || rt_cull_box_missed(c, b[0], b[1], b[2], b[3], b[4], b[5]);
            if (!dead) dead = rt_cull_ref_no_leaf(c, blob, off_nodes, num_nodes, ref, stack, sp);
            if (dead) word |= gate;
            if (!(ref & RT_REF_LEAF) && sp < RT_CULL_STACK) stack[sp++] = (ref & RT_REF_NODE_MASK) | (dead ? RT_CULL_DEAD_ABOVE : 0u);
        }
        if (sp == 0) return word;
        cur = stack[--sp];
    }
}

/* ---- the slab test's three forms (rt_intersect.h: box_test, box_enter, box_enter_med3) restated for host code, operation for operation:
 * what tests/sanitize/cull_soundness.cpp holds the predicate against.  fminf / fmaxf drop a NaN operand like the device's. */
RT_CULL_HD bool rt_cull_slab_test(const float b0[3], const float b1[3], const float o[3], const float inv[3])
{
    float tmin = 0.0f, tmax = RT_INF_F;
    for (int k = 0; k < 3; k++) {
        const float t1 = (b0[k] - o[k]) * inv[k], t2 = (b1[k] - o[k]) * inv[k];
        tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    }
    return tmin < tmax && tmax > 0.0f;
}
RT_CULL_HD bool rt_cull_slab_enter(const float b0[3], const float b1[3], const float o[3], const float inv[3], float best)
{
    float tmin = 0.0f, tmax = RT_INF_F;
    for (int k = 0; k < 3; k++) {
        const float t1 = (b0[k] - o[k]) * inv[k], t2 = (b1[k] - o[k]) * inv[k];
        tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
    }
    return tmin < fminf(tmax, best);
}
/* v_med3_f32 of three numbers (the kernel takes this form only for rays without a zero component: no NaN product) */
RT_CULL_HD float rt_cull_med3(float a, float b, float c) { return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c)); }
RT_CULL_HD bool rt_cull_slab_enter_med3(const float b0[3], const float b1[3], const float o[3], const float inv[3], float best)
{
    float lo = 0.0f, hi = best;
    for (int k = 0; k < 3; k++) {
        const float t1 = (b0[k] - o[k]) * inv[k], t2 = (b1[k] - o[k]) * inv[k];
        lo = rt_cull_med3(t1, t2, lo); hi = rt_cull_med3(t1, t2, hi);
    }
    return lo < hi;
}

/* ---- the render kernel's traversal of one mesh (rt_render_loop.inc: the ONE_MESH root test, rt_descend_pop's step, the leaf, rt_pop) restated
 * for host code with the slab forms above: far child first, strict <, the pop rule, the med3 form unless a direction component is exactly
 * zero.  `gates` is the lane's gate word (0: the ungated traversal).  leaf(ref, best, prim) tests a leaf's triangles and may lower best.
 * Returns the node steps, -1 for a tree the flattener did not make.  What tests/sanitize/gate_soundness.cpp and the estimate tool walk. */
RT_CULL_HD bool rt_cull_walk_enter(const float *b, const float o[3], const float inv[3], float best, bool med3, float &dist)
{
    const float b0[3] = {b[0], b[1], b[2]}, b1[3] = {b[3], b[4], b[5]};
    if (med3) {
        float lo = 0.0f;
        for (int k = 0; k < 3; k++) lo = rt_cull_med3((b0[k] - o[k]) * inv[k], (b1[k] - o[k]) * inv[k], lo);
        dist = lo;
        return rt_cull_slab_enter_med3(b0, b1, o, inv, best);
    }
    float tmin = 0.0f;
    for (int k = 0; k < 3; k++) tmin = fmaxf(tmin, fminf((b0[k] - o[k]) * inv[k], (b1[k] - o[k]) * inv[k]));
    dist = tmin;
    return rt_cull_slab_enter(b0, b1, o, inv, best);
}
template <class Leaf>
RT_CULL_HD int64_t rt_cull_walk(const float *blob, int32_t off_nodes, int32_t num_nodes, int32_t off_meshes, int32_t mesh, const float o[3], const float d[3],
                                const float inv[3], uint32_t gates, float &best, int32_t &prim, Leaf leaf)
{
    best = RT_INF_F; prim = -1;
    if (d[0] != d[0] || d[1] != d[1] || d[2] != d[2]) return 0;
    const float *m0 = blob + 4 * ((size_t)off_meshes + 2 * (size_t)mesh);
    const uint32_t root = rt_cull_bits(m0[6]);
    {
        const float b0[3] = {m0[0], m0[1], m0[2]}, b1[3] = {m0[3], m0[4], m0[5]};
        float rd = 0.0f;
        for (int k = 0; k < 3; k++) rd = fmaxf(rd, fminf((b0[k] - o[k]) * inv[k], (b1[k] - o[k]) * inv[k]));
        if (!rt_cull_slab_test(b0, b1, o, inv) || rd > RT_INF_F || ((root & RT_REF_CHAIN) && !(rd < RT_INF_F))) return 0;
    }
    const bool med3 = !(d[0] == 0.0f || d[1] == 0.0f || d[2] == 0.0f);
    struct { float dist; uint32_t ref; } stack[RT_STACK_ENTRIES + 2];
    int sp = 0;
    int64_t steps = 0;
    uint32_t cur = root;
    for (;;) {
        if (!(cur & RT_REF_LEAF)) {
            const uint32_t idx = cur & RT_REF_NODE_MASK;
            if (idx >= (uint32_t)num_nodes) return -1;
            steps++;
            const float *n = blob + 4 * ((size_t)off_nodes + 4 * (size_t)idx);
            float ld, rdist;
            bool l_push = rt_cull_walk_enter(n, o, inv, best, med3, ld), r_push = rt_cull_walk_enter(n + 6, o, inv, best, med3, rdist);
            const uint32_t lref = rt_cull_bits(n[12]), rref = rt_cull_bits(n[13]);
            l_push = l_push && (gates & rt_cull_bits(n[14])) == 0u;
            r_push = r_push && (gates & rt_cull_bits(n[15])) == 0u;
            const bool l_first = ld < rdist;
            if (l_push && r_push) {
                if (sp > RT_STACK_ENTRIES) return -1;
                stack[sp].dist = l_first ? ld : rdist;
                stack[sp].ref = l_first ? lref : rref;
                sp++;
                cur = l_first ? rref : lref;
                continue;
            }
            if (l_push || r_push) { cur = l_push ? lref : rref; continue; }
            cur = RT_REF_EMPTY_LEAF;
        }
        if (((cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX) != 0u) leaf(cur, best, prim);
        if (sp == 0) return steps;
        sp--;
        const bool take = stack[sp].dist < best || (stack[sp].dist == best && !(stack[sp].ref & RT_REF_CHAIN));
        cur = take ? stack[sp].ref : RT_REF_EMPTY_LEAF;
    }
}
struct rt_cull_no_triangles { RT_CULL_HD_MEMBER void operator()(uint32_t, float &, int32_t &) const {} };
RT_CULL_HD int64_t rt_cull_walk_steps(const float *blob, int32_t off_nodes, int32_t num_nodes, int32_t off_meshes, int32_t mesh, const float o[3], const float d[3],
                                      const float inv[3], uint32_t gates)
{
    float best; int32_t prim;
    return rt_cull_walk(blob, off_nodes, num_nodes, off_meshes, mesh, o, d, inv, gates, best, prim, rt_cull_no_triangles());
}

#include <cstring>
/* ---- what the context remembers about its plane (rt_capi.cpp), without a HIP call in it: tests/sanitize/cull_key_check.cpp drives it ---- */
namespace rt_cull_host {

/* what a plane was computed for: the scene (its uid changes with a commit and with every update of its geometry), the camera, the image
 * and the antialias flag */
struct Key {
    uint32_t scene_uid = 0;
    float cam[12] = {};
    int32_t width = 0, height = 0, antialias = 0;
    bool same(const Key &k) const
    {
        return scene_uid == k.scene_uid && std::memcmp(cam, k.cam, sizeof cam) == 0 && width == k.width && height == k.height && antialias == k.antialias;
    }
};

enum class Step { none, reuse, run };    /* none: render without a plane; reuse: the plane on the device is this view's; run: launch the pre-pass first */

struct Plan {
    Key key;
    bool valid = false;                  /* the plane on the device was computed for `key` */
    size_t cap_words = 0;                /* the allocation: grows with the image, never shrinks */
    bool used_last = false;              /* the last render launch was handed the plane */
    /* what the launch of view `k` does.  grow(words) allocates a plane of at least that many words and says whether it could; it is called
     * only when the image outgrows the allocation, and a refusal leaves the context without a plane (the launch renders without one). */
    /* The sub-entry tables (rt_entry.h) live behind the plane in the same allocation.  want_tables is the caller's switch, set before
     * next(); while next() calls grow(words), `tables` says which size the allocation is to have - with the tables (rt_sub_alloc_words) or
     * without (rt_cull_alloc_words_entry).  An allocation with tables that is refused is asked for again without them, once per size:
     * the plane then works as before and nothing is refined until the image outgrows it.  want_tables follows the scene (one mesh), `tables`
     * the allocation: once granted the larger allocation is kept - a launch that wants no tables uses its front part - and only growth of the
     * image allocates again, with the tables if the launch that grows it wants them.  So a one-mesh and a several-mesh scene alternating at
     * growing sizes allocate once per size, as before, and once more where the first launch of a size wanted no tables and a later one does;
     * each allocation frees the old plane, which waits for the launches that read it. */
    bool want_tables = false;
    bool tables = false;                 /* the allocation has room for the tables of cap_words */
    bool tables_refused = false;         /* ... it was refused with them: not asked for again at this size */
    bool refined = false;                /* the plane's view has its tables filled in (or queued to be) */
    template <class Grow> Step next(const Key &k, bool enabled, Grow grow)
    {
        used_last = false;
        if (!enabled) return Step::none;
        if (valid && key.same(k)) return Step::reuse;
        valid = false;
        refined = false;
        const size_t words = rt_cull_words(k.width, k.height);
        if (cap_words < words || (want_tables && !tables && !tables_refused)) {
            if (cap_words < words) tables_refused = false;
            cap_words = 0;
            tables = want_tables && !tables_refused;
            if (!grow(words)) {
                if (!tables) return Step::none;
                tables = false; tables_refused = true;
                if (!grow(words)) return Step::none;
            }
            cap_words = words;
        }
        return Step::run;
    }
    /* the pre-pass for `k` is queued (ok) or could not be (the launch then renders without the plane) */
    void ran(const Key &k, bool ok) { valid = ok; if (ok) key = k; else refined = false; }
    /* Does the launch that next() answered `step` for queue the refinement?  `samples` are the launch's own samples per pixel (spp x
     * frames).  A view's first launch refines at once if it reaches `threshold` - the refinement then pays for itself inside the launch -;
     * otherwise the first reuse of the view's plane does: a caller who never repeats a view with launches below the threshold never pays. */
    bool refine(Step step, const Key &k, int64_t samples, int64_t threshold)
    {
        /* (a view without jitter has one ray per pixel: no tables) */
        if (step == Step::none || !want_tables || !tables || refined || !k.antialias) return false;
        if (step == Step::run && samples < threshold) return false;
        refined = true;
        return true;
    }
    /* the refinement could not be queued: the words of the plane are as the pre-pass left them or half rewritten - compute the view again */
    void refine_failed() { valid = false; refined = false; }
};

}  // namespace rt_cull_host

#endif
