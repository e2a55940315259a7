/*
 * rt_traverse.h — the BVH traversal pieces of a lane state machine, shared by the render kernel (rt_render_kernel.h) and the ray kernels
 * (rt_query_kernel.h, rt_occlusion_kernel.h, rt_ao_kernel.h): the lane modes, the descend loop, the scene staging, mesh entry, a leaf's
 * triangles, the pop and the merge of a finished mesh.
 */
#ifndef RT_TRAVERSE_H
#define RT_TRAVERSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_instrument.h"
#include "rt_intersect.h"
#include "rt_vec.h"

/* lane states of the render loop and of the ray kernels' loops.  M_START (rt_occlusion_kernel.h, rt_ao_kernel.h): the lane holds a ray that
 * has not met the top-level objects yet */
enum { M_FETCH = 0, M_GEN = 1, M_MESH = 2, M_WAIT = 3, M_SHADE = 4, M_DONE = 5, M_START = 6 };

/* LLVM integer-compare predicates for __builtin_amdgcn_uicmp / sicmp (lane mask of a compare, straight into an SGPR pair) */
#define RT_ICMP_EQ 32
#define RT_ICMP_NE 33
#define RT_ICMP_SGT 38
#define RT_ICMP_SGE 39

/* The descend loop of a traversal macro step: from an internal node down to a leaf (or to "no child entered").
 * The body is branch-free: the deferred sibling is ALWAYS written to the slot above the top of the stack (one 8-byte
 * LDS store) and the stack pointer moves only when both children are entered, so the only divergent branch of the
 * loop is its exit.  The loop also ends, for everybody, once fewer than `descend_keep`/64 of the lanes that entered
 * it are still descending: those lanes just stay on their internal node and go on next step, instead of making the
 * others wait out the deepest descent of the wave.  MED3: box_enter_med3 (rays without a zero direction component). */
template <int NT, bool MED3>
__device__ __forceinline__ void rt_descend(uint32_t &cur, int &sp, uint2 *my_stack, const Lds &L, V3 o, V3 inv, float w_best, int descend_keep RT_STAT_PARAMS)
{
    const int n_enter = __popcll(__ballot(1));
    const int n_keep = (n_enter * descend_keep) >> 6;
    for (;;) {
        RT_STAT(ST_NODE);
        RT_COST(c_steps++);
        const v4f *n = L.nodes + 4 * (int)(cur & RT_REF_NODE_MASK);
        const v4f q0 = n[0], q1 = n[1], q2 = n[2];
        const uint2 refs = *(const uint2 *)(n + 3);          /* the two child references: 8 of the last 16 bytes */
        float ld, rdist;
        const bool l_push = MED3 ? box_enter_med3(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, w_best, ld)
                                 : box_enter(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, w_best, ld);
        const bool r_push = MED3 ? box_enter_med3(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, w_best, rdist)
                                 : box_enter(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, w_best, rdist);
        const uint32_t lref = refs.x, rref = refs.y;
        const bool l_first = ld < rdist;
        /* Of two entered children the one pushed first (left when l_first) is visited second: it is the deferred
         * sibling.  The other is popped immediately (its distance is still < best).  With one entered child that
         * child is next and nothing is deferred. */
        const bool both = l_push && r_push;
        const bool entered = l_push || r_push;
        const unsigned long long l_first_lanes = __builtin_amdgcn_fcmpf(ld, rdist, RT_FCMP_OLT);
        const uint32_t deferred_ref = rt_sel_u32(l_first_lanes, lref, rref);
        const float deferred_d = rt_sel_f32(l_first_lanes, ld, rdist);
        my_stack[sp * NT] = make_uint2(__float_as_uint(deferred_d), deferred_ref);
        sp += both ? 1 : 0;
        const uint32_t next = both ? (l_first ? rref : lref) : (l_push ? lref : rref);
        cur = entered ? next : RT_REF_EMPTY_LEAF;
        {
            /* One divergent exit: the lanes that leave - those that reached a leaf, or everybody once fewer than n_keep are
             * still on an internal node - are computed as a lane mask in five instructions (one compare, four scalar) and handed
             * to the compiler as the loop's exit condition (inverse ballot: no instruction).  The compiler's own rendering of
             * "leaf || count < n_keep" took 16 scalar instructions and 3 branches per node step (round 3), then, with the count
             * passed through a VGPR, 9 + 3 vector ones (-2 %, profiles/r04/experiments/keep_rule_single_exit.txt). */
            unsigned long long stop, internal;
            int cnt;
            asm volatile("v_cmp_gt_i32_e64 %0, 0, %3\n\t"
                         "s_andn2_b64 %1, exec, %0\n\t"
                         "s_bcnt1_i32_b64 %2, %1\n\t"
                         "s_cmp_lt_u32 %2, %4\n\t"
                         "s_cselect_b64 %0, exec, %0"
                         : "=&s"(stop), "=&s"(internal), "=&s"(cnt) : "v"(cur), "s"(n_keep) : "scc");
            if (__builtin_amdgcn_inverse_ballot_w64(stop)) break;
        }
    }
}

/* Pops one entry (sp > 0): it is taken iff !(dist > best) (src/objects.cu:501); through a collapsed chain iff dist < best (:517) - the distance is
 * never NaN, so that is dist < best, or dist == best on a plain edge.  A refused entry leaves the lane on the empty leaf: it pops again next step. */
template <int NT>
__device__ __forceinline__ uint32_t rt_pop(int &sp, const uint2 *my_stack, float w_best)
{
    sp--;
    const uint2 e = my_stack[sp * NT];
    const float dd = __uint_as_float(e.x);
    const bool take = dd < w_best || (dd == w_best && !(e.y & RT_REF_CHAIN));
    return take ? e.y : RT_REF_EMPTY_LEAF;
}

/* A lane of a macro step goes through rt_descend_pop (rather than straight to the leaf section): it is on an internal node, or on the empty
 * leaf with entries left on its stack (the post-leaf pop refused one) */
__device__ __forceinline__ bool rt_descend_pop_enters(uint32_t cur, int sp)
{
    return !(cur & RT_REF_LEAF) || (cur == RT_REF_EMPTY_LEAF && sp > 0);
}

/* rt_descend with the pop of a dead end inside the loop (the render kernels' form; while-while traversal).  A lane whose node entered no child
 * does not leave for the (empty) leaf section and the pop behind it: it pops its next deferred sibling here, with rt_pop's rule, and goes
 * on descending from a taken internal node in the following iterations.  A lane leaves once it is on a leaf: one with triangles, the empty
 * leaf with sp == 0 (the mesh is finished), or the empty leaf after a refused entry - that lane pops again in the leaf section and at the
 * head of its next call, as it does after rt_descend (rare: keeping it in the loop costs every iteration a select and a compare for
 * it, profiles/r12/experiments/).  The `descend_keep` rule and the single divergent exit are rt_descend's, on the lanes on an internal node;
 * which shapes run this loop, and the fraction they run it with by default, is rt_descend_pops / RT_DEF_DESCEND_KEEP_POP_LDS (rt_device_scene.h).
 * The body stays branch-free: the top of the stack is read with the node, every iteration, and the pop is selects on it.
 * Nothing a frame is made of changes: w_best does not change in here and no triangle is tested, so every take / refuse decision, every
 * box test, the push order and the visit order of a lane are those of rt_descend + rt_pop one macro step at a time - the frames are bit-identical. */
/* GATES (the subtree cull, rt_cull.h; only the kernel that reads the cull plane): `w_gates` is the lane's word of dead gates - its pixel's for a
 * primary ray, 0 for a bounce ray; bit 0 is not a gate and is ignored here (the caller keeps the ray's zero-direction flag in it).  The node's
 * last 16 bytes are then read whole, references and gate words, and a child whose gate is in the word is not entered, whatever its box says:
 * rt_cull.h has the argument for why the frames stay bit-identical. */
template <int NT, bool MED3, bool GATES = false>
__device__ __forceinline__ void rt_descend_pop(uint32_t &cur, int &sp, uint2 *my_stack, const Lds &L, V3 o, V3 inv, float w_best, int descend_keep, uint32_t w_gates RT_STAT_PARAMS)
{
    /* a lane that comes in on the empty leaf (the post-leaf pop refused its entry): pops until an entry is taken or the stack is empty (rare) */
    while (cur == RT_REF_EMPTY_LEAF && sp > 0) {
        RT_STAT(ST_POP_LOOP);
        cur = rt_pop<NT>(sp, my_stack, w_best);
    }
    if (cur & RT_REF_LEAF) return;
    const int n_enter = __popcll(__ballot(1));
    const int n_keep = (n_enter * descend_keep) >> 6;
    for (;;) {
        RT_STAT(ST_NODE);
        RT_COST(c_steps++);
        /* the top of the stack, asked for together with the node: a dead end below pops it without a second LDS round trip (nothing is
         * pushed in an iteration that enters no child, so it still is the top then; with sp == 0 slot 0 is read and not used) */
        const int top_slot = sp - (sp > 0 ? 1 : 0);
        const uint2 top = my_stack[top_slot * NT];
        const v4f *n = L.nodes + 4 * (int)(cur & RT_REF_NODE_MASK);
        const v4f q0 = n[0], q1 = n[1], q2 = n[2];
        uint32_t lref, rref, lgate = 0u, rgate = 0u;
        if (GATES) {
            const v4f q3 = n[3];                                 /* the references and their gate words: the last 16 bytes */
            lref = __float_as_uint(q3.x); rref = __float_as_uint(q3.y); lgate = __float_as_uint(q3.z); rgate = __float_as_uint(q3.w);
        } else {
            const uint2 refs = *(const uint2 *)(n + 3);          /* the two child references: 8 of the last 16 bytes */
            lref = refs.x; rref = refs.y;
        }
        /* (GATES: a dead child's box is tested against best = 0, which no box passes - both slab forms ask for an entry distance, never
         * negative, below min(exit distance, best) - so the gate costs a select in front of the test and no lane mask of its own to combine
         * behind it: with the masks combined the kernel spilled four more scalar registers and got a private segment) */
        const float l_best = GATES && (w_gates & lgate) != 0u ? 0.0f : w_best, r_best = GATES && (w_gates & rgate) != 0u ? 0.0f : w_best;
        float ld, rdist;
        const bool l_push = MED3 ? box_enter_med3(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, l_best, ld)
                                 : box_enter(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, l_best, ld);
        const bool r_push = MED3 ? box_enter_med3(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, r_best, rdist)
                                 : box_enter(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, r_best, rdist);
        const bool l_first = ld < rdist;
        /* (rt_descend's step: the deferred sibling always stored above the top, sp moves when both children are entered) */
        const bool both = l_push && r_push;
        const bool entered = l_push || r_push;
        const unsigned long long l_first_lanes = __builtin_amdgcn_fcmpf(ld, rdist, RT_FCMP_OLT);
        const uint32_t deferred_ref = rt_sel_u32(l_first_lanes, lref, rref);
        const float deferred_d = rt_sel_f32(l_first_lanes, ld, rdist);
        my_stack[sp * NT] = make_uint2(__float_as_uint(deferred_d), deferred_ref);
        const uint32_t next = both ? (l_first ? rref : lref) : (l_push ? lref : rref);
        /* a dead end with entries left pops the top by rt_pop's rule: taken, the lane goes on from it; refused, the lane is on the empty leaf */
        const float dd = __uint_as_float(top.x);
        const unsigned long long take = __builtin_amdgcn_sicmp(sp, 0, RT_ICMP_SGT) &
            (__builtin_amdgcn_fcmpf(dd, w_best, RT_FCMP_OLT) | (__builtin_amdgcn_fcmpf(dd, w_best, RT_FCMP_OEQ) & __builtin_amdgcn_uicmp(top.y & RT_REF_CHAIN, 0u, RT_ICMP_EQ)));
        if (!entered && sp > 0) RT_STAT(ST_POP_LOOP);      /* (development builds only) */
        /* what a lane that entered no child goes on with: the popped entry if it has one and takes it, else the empty leaf (finished with
         * sp == 0, refused otherwise); lane masks and selects, so that the body stays one block */
        const uint32_t popped = rt_sel_u32(take, top.y, RT_REF_EMPTY_LEAF);
        cur = entered ? next : popped;
        sp = entered ? sp + (both ? 1 : 0) : top_slot;
        {
            /* rt_descend's single divergent exit, same five instructions: the lanes on a leaf leave, or everybody once fewer than n_keep are on
             * an internal node */
            unsigned long long stop, internal;
            int cnt;
            asm volatile("v_cmp_gt_i32_e64 %0, 0, %3\n\t"
                         "s_andn2_b64 %1, exec, %0\n\t"
                         "s_bcnt1_i32_b64 %2, %1\n\t"
                         "s_cmp_lt_u32 %2, %4\n\t"
                         "s_cselect_b64 %0, exec, %0"
                         : "=&s"(stop), "=&s"(internal), "=&s"(cnt) : "v"(cur), "s"(n_keep) : "scc");
            if (__builtin_amdgcn_inverse_ballot_w64(stop)) break;
        }
    }
}

/* Where a workgroup of the query kernels (rt_query_kernel.h) reads the scene from (MODE: RT_SCENE_*, rt_device_scene.h): stages the blob, or its part before the triangles,
 * into LDS and points L's sections and the traversal stacks at their places.  The caller synchronises the workgroup.  This restates the first lines of
 * rt_render_kernel (rt_render_kernel.h), which keeps them in place: calling this function there changes 3 of its 13 instantiations (see below). */
template <int NT, int MODE, class Args>
__device__ __forceinline__ void rt_stage_scene(const Args &a, v4f *lds_raw, int tid, Lds &L, uint2 *&stack)
{
    if (MODE != RT_SCENE_GLOBAL) {
        /* stage the scene (or its part before the triangles) into LDS: coalesced 16-byte loads, one pass per workgroup */
        const int staged = MODE == RT_SCENE_LDS ? a.blob_f4 : a.off_tris;
        for (int i = tid; i < staged; i += NT) lds_raw[i] = ((const v4f *)a.blob)[i];
        L.nodes = lds_raw + a.off_nodes;
        L.objs = lds_raw + a.off_objlds;
        L.meshes = lds_raw + a.off_meshes;
        L.objtab = lds_raw + a.off_objtab;
        L.tris = MODE == RT_SCENE_LDS ? lds_raw + a.off_tris : (const v4f *)a.blob + a.off_tris;
        stack = (uint2 *)(lds_raw + staged);
    } else {
        const v4f *g = (const v4f *)a.blob;
        L.nodes = g + a.off_nodes;
        L.tris = g + a.off_tris;
        L.objs = g + a.off_objlds;
        L.meshes = g + a.off_meshes;
        L.objtab = g + a.off_objtab;
        stack = (uint2 *)lds_raw;
    }
}

/* rt_stage_scene above and rt_mesh_enter, rt_leaf_tris and rt_mesh_merge below serve the query kernels (rt_query_kernel.h) and restate what
 * rt_render_kernel's prologue, MESH and WORK sections do in place: with the render kernel calling them, some or all of its instantiations come out
 * with another register allocation or schedule (compared per function against the code object before the queries), and that kernel does not change
 * with the queries.  rt_descend, rt_pop, the box and triangle tests and rt_closest_simple (rt_intersect.h) ARE one statement for both: those calls leave
 * the render kernels byte-identical. */
/* Does a ray start traversing the mesh (m0, m1: its rt_f4 pair of the `meshes` section)?  If so `cur` is its root and `zero_dir` says whether the
 * direction has a component of exactly zero (box_enter_med3). */
__device__ __forceinline__ bool rt_mesh_enter(const v4f m0, const v4f m1, V3 o, V3 d, V3 inv, uint32_t &cur, uint32_t &zero_dir)
{
    /* a NaN direction (Box-Muller on a zero draw) fails every
     * triangle test: the mesh cannot be hit, no need to walk it */
    if (d.x != d.x || d.y != d.y || d.z != d.z) return false;
    /* the root is pushed unconditionally and tested when popped (src/objects.cu:494-501) */
    const uint32_t root_ref = __float_as_uint(m1.z);
    float rd;
    const bool rh = box_test(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, o, inv, rd);
    if (!rh || rd > RT_INF_F || ((root_ref & RT_REF_CHAIN) && !(rd < RT_INF_F))) return false;
    cur = root_ref;
    zero_dir = (d.x == 0.0f || d.y == 0.0f || d.z == 0.0f) ? 1u : 0u;
    return true;
}

/* The triangles of the leaf `cur`: strict <, first triangle wins ties (src/objects.cu:596) */
__device__ __forceinline__ void rt_leaf_tris(uint32_t cur, const Lds &L, V3 o, V3 d, float &w_best, int &w_prim)
{
    const int start = (int)(cur & RT_REF_START_MASK);
    const int count = (int)((cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
    for (int k = 0; k < count; k++) {
        float t;
        const unsigned long long closer = tri_closer_lanes(L.tris, start + k, o, d, w_best, t);
        w_best = rt_sel_f32(closer, t, w_best);
        w_prim = (int)rt_sel_u32(closer, (uint32_t)(start + k), (uint32_t)w_prim);
    }
}

/* A mesh is done: its closest triangle against the closest hit so far - smaller distance, or equal and later in the object list (the mesh's place in
 * the list is read again here rather than kept in a register) */
__device__ __forceinline__ void rt_mesh_merge(const Lds &L, int mesh, float w_best, int w_prim, float &best_t, int &best_obj, int &best_prim)
{
    const int w_obj = (int)__float_as_uint(L.meshes[2 * mesh + 1].w);
    if (w_prim >= 0 && (w_best < best_t || (w_best == best_t && w_obj > best_obj))) {
        best_t = w_best; best_obj = w_obj; best_prim = w_prim;
    }
}

#endif
