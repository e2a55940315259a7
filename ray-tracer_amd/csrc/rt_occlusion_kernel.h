/*
 * rt_occlusion_kernel.h — occlusion (any-hit) ray queries and the light-visibility plane of a view: "is anything in the way?", one byte
 * per ray.  The traversal pieces are rt_traverse.h's; the launcher at the end (rt_ray_kernel.h) is declared in rt_launch.h.
 *
 * occluded(o, d, tmax) := get_ray_collision (src/raytracer.cu:24-46; what rt_query_kernel answers) finds a hit AND its distance
 * t <= tmax.  The ray is taken as given (direction not normalised, t and tmax in units of its length, Ray::change_direction
 * src/ray.cu:198-202); a NaN direction hits nothing; a NaN tmax compares false.
 *
 * The early exits are exact.  The reference searches every object with a running best of its own that starts at "infinity"
 * (src/objects.cu:487-532) and answers the minimum over the objects; a running best only falls, so the final t is <= tmax iff some
 * running best is <= tmax at some moment.  A ray therefore stops
 *   - after rt_closest_simple, if a top-level object was hit at best_t <= tmax: no mesh is visited;
 *   - inside a mesh, right after a leaf's triangle tests, if w_best <= tmax (which also ends the walk over the meshes).
 * What is NOT done: starting a mesh's running best at tmax, or skipping a mesh whose root box is entered beyond tmax.  That changes
 * which boxes are entered (the slab distance and Moller-Trumbore's t round differently), and the tree's visit set is kept.
 *
 * One kernel, two fronts.  VIS == false reads n rays (and n limits, or none) and writes n bytes: 1 occluded, 0 not.  VIS == true is the
 * shadow mask of a point light, fused: per pixel the AOV pass's primary ray (px_fetch's expression, antialiasing off) and its closest
 * hit (no early exit: the limit of that segment is NaN, so no comparison with it holds), then from the hit's point P and shading normal
 * N as rt_hit reports them the segment o' = P + N * bias (two roundings per component), d' = light - o', limit 1; the byte is
 * RT_VIS_NO_SURFACE, RT_VIS_BLOCKED or RT_VIS_LIT.
 *
 * A lane is the query kernel's state machine: FETCH (take the next ray) -> START (reciprocal direction, the top-level objects, first
 * exit) -> MESH -> WAIT (traversal macro steps, second exit) -> SHADE (store the byte; or, for a pixel whose primary ray hit, form the
 * shadow segment and go to START again) -> FETCH.  In the visibility kernel START is a state of its own, so that the kernel holds
 * rt_closest_simple once, not once per segment; a ray query does it inside FETCH (as a state it kept the ray's registers live round the loop).  Both segments use the operator's division in the sphere test (!UNIT_DIR): on a
 * unit direction it gives the short form's bits for every accepted distance (rt_intersect.h, rt_closest_simple).
 */
#ifndef RT_OCCLUSION_KERNEL_H
#define RT_OCCLUSION_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_occlusion.h"
#include "rt_ray_kernel.h"
#include "rt_surface.h"
#include "rt_traverse.h"
#include "rt_vec.h"

/* lanes of a wave holding a finished ray before the traversal loop yields to store and refill them: swept over 8 / 16 / 24 / 32 with
 * tools/occlusion_probe.py (DESIGN.md §11 has the table) */
#ifndef RT_OCCLUSION_REFILL
#define RT_OCCLUSION_REFILL 16
#endif
#define RT_BELOW_INF_F 1073741760.0f      /* the largest binary32 below RT_INF_F (2^30 - 2^6) */

/* START: a lane's ray meets the top-level objects; first exit.  Leaves the lane in MESH (with the limit clamped for the mesh walks) or, answered, in SHADE.
 * (Args: rt_occlusion_args, or rt_ao_args of rt_ao_kernel.h) */
template <bool HAS_MESH, class Args>
__device__ __forceinline__ void rt_occlusion_start(const Args &a, const Lds &L, V3 o, V3 d, V3 &inv, float &tm, float &best_t, int &best_obj, int &best_prim,
                                                   uint32_t &occ, int &next_mesh, int &mode)
{
    if (HAS_MESH) inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);   /* src/ray.cu:198-202 */
    rt_closest_simple<false>(o, d, a.num_objects, L, best_t, best_obj, best_prim);
    /* (a top-level hit may lie AT RT_INF_F, `t <= best_t`: the index, not the distance, says whether there is one) */
    occ = (best_obj >= 0 && best_t <= tm) ? 1u : 0u;
    next_mesh = 0;
    mode = (HAS_MESH && a.num_meshes > 0 && !occ) ? M_MESH : M_SHADE;
    /* a mesh's running best starts at RT_INF_F and a triangle is taken below it only (strict <): "the mesh has a hit, and
     * within the limit" is one compare against the limit clamped below RT_INF_F.  A NaN limit stays NaN. */
    tm = tm >= RT_INF_F ? RT_BELOW_INF_F : tm;
}

template <int NT, bool HAS_MESH, int MODE, bool VIS>
__global__ __launch_bounds__(NT, 4) void rt_occlusion_kernel(const rt_occlusion_args a)
{
    extern __shared__ v4f lds_raw[];
    const int tid = threadIdx.x;
    const int lane = tid & (RT_WAVE - 1);

    Lds L;
    uint2 *stack;        /* [stack_entries + 1][NT], as in rt_render_kernel */
    rt_stage_scene<NT, MODE>(a, lds_raw, tid, L, stack);
    __syncthreads();
    uint2 *const my_stack = stack + tid;

    const V3 cam_pos = v3(a.cam[0], a.cam[1], a.cam[2]), tl = v3(a.cam[3], a.cam[4], a.cam[5]);
    const V3 du = v3(a.cam[6], a.cam[7], a.cam[8]), dv = v3(a.cam[9], a.cam[10], a.cam[11]);

    /* per-lane ray and traversal state */
    int mode = M_FETCH;
    uint32_t id = 0;
    V3 o = v3(0.f, 0.f, 0.f), d = o, inv = o;
    float tm = 0.f;                  /* the segment's limit; from MESH on clamped below RT_INF_F (see START) */
    uint32_t occ = 0u;               /* something is in the way within the limit */
    int shadow = 0;                  /* VIS: the lane is on its pixel's shadow segment */
    float best_t = RT_INF_F;         /* VIS: the primary ray's closest hit */
    int best_obj = -1, best_prim = -1, next_mesh = 0;
    uint32_t cur = 0, w_zero_dir = 0u;
    int sp = 0, w_prim = -1;
    float w_best = RT_INF_F;
    /* wave-uniform: ray ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the segment is answered ============================================== */
        if (mode == M_SHADE) {
            if (VIS && !shadow && best_obj >= 0) {
                /* the primary ray hit: the shadow segment from that surface to the light */
                const uint32_t packed = __float_as_uint(L.objs[RT_OBJLDS_F4 * best_obj + 1].w);
                V3 P, N;
                float tex_u, tex_v;
                rt_hit_surface(o, d, best_t, best_obj, best_prim, packed & ~16u, L, nullptr, P, N, tex_u, tex_v);     /* (no texture coordinates) */
                o = N * a.bias + P;
                d = v3(a.light[0], a.light[1], a.light[2]) - o;
                tm = 1.0f;
                shadow = 1;
                mode = M_START;
            } else {
                /* one byte per ray: an ordinary vector byte store */
                a.out[id] = (uint8_t)(VIS ? (shadow ? 1u - occ : (uint32_t)RT_VIS_NO_SURFACE) : occ);
                mode = M_FETCH;
            }
        }

        /* ================= FETCH: free lanes take the next ray ids (whole wave, as in rt_query_kernel) == */
        {
            const bool want = mode == M_FETCH;
            const unsigned long long mask = __ballot(want);
            if (mask) {
                const int need = __popcll(mask);
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                int taken = 0;
                long long my_id = -1;
                for (;;) {
                    const int avail = (int)(end - next);
                    const int take = avail < need - taken ? avail : need - taken;
                    if (want && rank >= taken && rank < taken + take) my_id = (long long)next + (rank - taken);
                    next += (uint32_t)take;
                    taken += take;
                    if (taken == need || exhausted) break;
                    uint32_t c = 0;
                    if (lane == 0) c = atomicAdd(a.counter, 1u);
                    c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
                    if (c >= a.num_chunks) { exhausted = true; break; }
                    next = c * 64u;
                    end = next + 64u < a.n ? next + 64u : a.n;
                }
                if (want) {
                    if (my_id < 0) {
                        mode = M_DONE;
                    } else if (VIS) {
                        /* a chunk is an 8x8 tile; a slot of a ragged edge tile outside the image is no ray: the lane stays in FETCH */
                        const uint32_t tile = (uint32_t)my_id >> 6, within = (uint32_t)my_id & 63u;
                        const uint32_t ty = tile / (uint32_t)a.tiles_x, tx = tile - ty * (uint32_t)a.tiles_x;
                        const int px = (int)(tx * 8u + (within & 7u)), py = (int)(ty * 8u + (within >> 3));
                        if (px < a.width && py < a.height) {
                            id = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
                            /* the renderer's primary ray with antialiasing off: px_fetch (src/raytracer.cu:123-127, src/camera.cu:24-29) */
                            const V3 plane_point = du * (float)px + dv * (float)py;
                            o = cam_pos;
                            d = normalised((tl + plane_point) - cam_pos);
                            tm = __uint_as_float(0x7fc00000u);          /* closest hit: no exit */
                            shadow = 0;
                            mode = M_START;
                        }
                    } else {
                        id = (uint32_t)my_id;
                        const float *qo = a.origins + 3 * (size_t)id, *qd = a.directions + 3 * (size_t)id;
                        o = v3(qo[0], qo[1], qo[2]);
                        d = v3(qd[0], qd[1], qd[2]);
                        tm = a.tmax ? a.tmax[id] : RT_INF_F;
                        rt_occlusion_start<HAS_MESH>(a, L, o, d, inv, tm, best_t, best_obj, best_prim, occ, next_mesh, mode);
                    }
                }
            }
        }

        /* ================= START (visibility kernel; a ray query starts in FETCH) ======================= */
        if (VIS && mode == M_START) rt_occlusion_start<HAS_MESH>(a, L, o, d, inv, tm, best_t, best_obj, best_prim, occ, next_mesh, mode);

        if (HAS_MESH) {
            /* ================= MESH: the next mesh whose root box the ray enters ============================= */
            while (mode == M_MESH) {
                if (next_mesh >= a.num_meshes) { mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * next_mesh], m1 = L.meshes[2 * next_mesh + 1];
                next_mesh++;
                if (!rt_mesh_enter(m0, m1, o, d, inv, cur, w_zero_dir)) continue;
                sp = 0; w_best = RT_INF_F; w_prim = -1;
                mode = M_WAIT;
            }

            /* ================= WORK: traversal macro steps (rt_query_kernel's, with the exit after the leaf) = */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); answered rays are stored, and their lanes refilled, in batches.  Once the
                 * last rays are handed out a ray query runs to its end; a pixel's answered primary ray still has its shadow segment to start */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if ((VIS || !exhausted) && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_OCCLUSION_REFILL) break;
                if (mode == M_WAIT) {
                    if (!(cur & RT_REF_LEAF)) {
                        if (__builtin_amdgcn_uicmp(w_zero_dir, 0u, RT_ICMP_NE) == 0ull) rt_descend<NT, true>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep);
                        else rt_descend<NT, false>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep);
                    }
                    if (cur & RT_REF_LEAF) {
                        rt_leaf_tris(cur, L, o, d, w_best, w_prim);
                        if (w_best <= tm) {
                            /* second exit: this mesh's running best is within the limit, and it can only fall */
                            occ = 1u;
                            mode = M_SHADE;
                        } else if (sp > 0) {
                            cur = rt_pop<NT>(sp, my_stack, w_best);
                        } else {
                            if (VIS) rt_mesh_merge(L, next_mesh - 1, w_best, w_prim, best_t, best_obj, best_prim);      /* (the primary ray's closest hit) */
                            mode = next_mesh >= a.num_meshes ? M_SHADE : M_MESH;
                        }
                    }
                }
            }
        }

        if (__ballot(mode != M_DONE) == 0ull) break;
    }
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
struct rt_occlusion_kernels {
    typedef rt_occlusion_args args;
    template <int NT, bool HAS_MESH, int MODE, bool VIS> static constexpr auto kernel = &rt_occlusion_kernel<NT, HAS_MESH, MODE, VIS>;
};

extern "C" hipError_t rt_launch_occlusion(const rt_occlusion_args *args, rt_shape shape, int vis, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_occlusion_kernels>(args, shape, vis, num_cus, lds_bytes, stream);
}

#endif
