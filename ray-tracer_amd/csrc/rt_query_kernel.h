/*
 * rt_query_kernel.h — closest-hit ray queries and the first-hit AOV pass: one ray per lane through the scene the render kernel
 * stages, stopped at the first hit, with the hit written out instead of shaded.  The traversal pieces are rt_traverse.h's, the hit's surface
 * is rt_surface.h's; the launcher at the end (rt_ray_kernel.h) is declared in rt_launch.h.
 *
 * What is found is get_ray_collision (src/raytracer.cu:24-46) under the render kernel's rules: the top-level objects in list order
 * with `t <= best_t` (rt_closest_simple, rt_intersect.h), then the meshes merged by "smaller distance, or equal distance and larger list
 * index", each walked with rt_descend / the leaf test / rt_pop of rt_traverse.h.  The ray is taken as given: the direction is NOT
 * normalised (Ray::change_direction, src/ray.cu:198-202), the distance is in units of its length, the reciprocal direction is
 * 1.0f / d per component.  A NaN direction hits nothing and is answered without traversing.
 *
 * One kernel, two fronts: AOV == false reads n rays (origins, directions: n x 3 floats) and writes n rt_hit records; AOV == true
 * generates the renderer's primary ray of every pixel with antialiasing off (px_fetch's expression) and writes the requested planes.
 *
 * A lane is a small state machine as in the render kernel: FETCH (take the next ray, test the top-level objects) -> MESH (next mesh
 * whose root box the ray enters) -> WAIT (traversal macro steps) -> SHADE (form the record, store it) -> FETCH.  A wave takes ray ids
 * 64 at a time from a global counter and hands them to whichever lanes are free, so no lane waits for the slowest ray of a wave: the
 * traversal loop yields once RT_QUERY_REFILL lanes hold a finished ray, and runs to its end once the last rays are handed out
 * (`exhausted`).  The grid is sized from the ray count by the launcher: one wave per 64 rays up to the persistent grid (every CU
 * filled), so a handful of rays stages the scene once, not once per CU.
 */
#ifndef RT_QUERY_KERNEL_H
#define RT_QUERY_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_query.h"
#include "rt_ray_kernel.h"
#include "rt_surface.h"
#include "rt_traverse.h"
#include "rt_vec.h"

#define RT_QUERY_REFILL 16      /* lanes of a wave holding a finished ray before the traversal loop yields to store and refill them (not tuned) */

template <int NT, bool HAS_MESH, int MODE, bool AOV>
__global__ __launch_bounds__(NT, 4) void rt_query_kernel(const rt_query_args a)
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
    float best_t = RT_INF_F;
    int best_obj = -1, best_prim = -1, next_mesh = 0;
    uint32_t cur = 0, w_zero_dir = 0u;
    int sp = 0, w_prim = -1;
    float w_best = RT_INF_F;
    /* wave-uniform: ray ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the closest hit is known; form the record and store it ================= */
        if (mode == M_SHADE) {
            V3 P = v3(0.f, 0.f, 0.f), N = P, albedo = v3(a.sky[0], a.sky[1], a.sky[2]);
            float tex_u = 0.f, tex_v = 0.f;
            if (best_obj >= 0) {
                const v4f mb = L.objs[RT_OBJLDS_F4 * best_obj + 1];
                const uint32_t packed = __float_as_uint(mb.w);
                rt_hit_surface(o, d, best_t, best_obj, best_prim, packed, L, a.tri_uv, P, N, tex_u, tex_v);
                if (AOV && a.albedo) {
                    /* what trace_ray (src/raytracer.cu:86-90) does with the first hit: an emissive object adds its light, any other
                     * multiplies the throughput by its texture colour */
                    const v4f ma = L.objs[RT_OBJLDS_F4 * best_obj];
                    albedo = (int)(packed & 3u) == RT_DEV_MAT_EMISSIVE ? v3(mb.x, mb.y, mb.z) : rt_texture_colour(ma, mb, packed, tex_u, tex_v, a.tex_data);
                }
            }
            if (AOV) {
                if (a.depth) a.depth[id] = best_t;
                if (a.normal) { float *q = a.normal + 3 * (size_t)id; q[0] = N.x; q[1] = N.y; q[2] = N.z; }
                if (a.albedo) { float *q = a.albedo + 3 * (size_t)id; q[0] = albedo.x; q[1] = albedo.y; q[2] = albedo.z; }
                if (a.object) a.object[id] = best_obj;
            } else {
                /* rt_hit: 48 bytes, three 16-byte stores; a miss is (RT_INF_F, 0..., -1, -1, 0, 0, 0) */
                v4f *h = (v4f *)a.hits + 3 * (size_t)id;
                const bool sphere_or_miss = best_prim < 0;
                v4f r0, r1, r2;
                r0.x = best_t; r0.y = P.x; r0.z = P.y; r0.w = P.z;
                r1.x = N.x; r1.y = N.y; r1.z = N.z; r1.w = __int_as_float(best_obj);
                r2.x = __int_as_float(sphere_or_miss ? -1 : best_prim); r2.y = tex_u; r2.z = tex_v; r2.w = 0.0f;
                h[0] = r0; h[1] = r1; h[2] = r2;
            }
            mode = M_FETCH;
        }

        /* ================= FETCH: free lanes take the next ray ids (whole wave, cf. px_fetch) ============= */
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
                    } else {
                        id = (uint32_t)my_id;
                        bool have_ray = true;
                        if (AOV) {
                            /* A chunk of the AOV pass is an 8x8 tile, as in the render kernel (64 pixels of one row make a wave's rays diverge sooner:
                             * measured 2.4 % behind the one-bounce render in raster order).  A slot of a ragged edge tile outside the image is
                             * no ray: the lane stays in FETCH.  From here on `id` is the pixel's index in the planes. */
                            const uint32_t tile = id >> 6, within = id & 63u;
                            const uint32_t ty = tile / (uint32_t)a.tiles_x, tx = tile - ty * (uint32_t)a.tiles_x;
                            const int px = (int)(tx * 8u + (within & 7u)), py = (int)(ty * 8u + (within >> 3));
                            have_ray = px < a.width && py < a.height;
                            id = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
                        }
                        if (!have_ray) {
                            /* stays M_FETCH */
                        } else {
                        if (AOV) {
                            /* the renderer's primary ray with antialiasing off: px_fetch (src/raytracer.cu:123-127, src/camera.cu:24-29) */
                            const int py = (int)(id / (uint32_t)a.width), px = (int)(id - (uint32_t)py * (uint32_t)a.width);
                            const V3 plane_point = du * (float)px + dv * (float)py;
                            o = cam_pos;
                            d = normalised((tl + plane_point) - cam_pos);
                            if (a.ray) { float *q = a.ray + 3 * (size_t)id; q[0] = d.x; q[1] = d.y; q[2] = d.z; }
                        } else {
                            const float *qo = a.origins + 3 * (size_t)id, *qd = a.directions + 3 * (size_t)id;
                            o = v3(qo[0], qo[1], qo[2]);
                            d = v3(qd[0], qd[1], qd[2]);
                        }
                        if (HAS_MESH) inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);   /* src/ray.cu:198-202 */
                        /* (the AOV pass's directions come out of normalised(), like the render kernel's: the sphere test's short division holds) */
                        rt_closest_simple<AOV>(o, d, a.num_objects, L, best_t, best_obj, best_prim);
                        next_mesh = 0;
                        mode = (HAS_MESH && a.num_meshes > 0) ? M_MESH : M_SHADE;
                        }
                    }
                }
            }
        }

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

            /* ================= WORK: traversal macro steps (the render kernel's, without its shading yields) = */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); finished rays are stored, and their lanes refilled, in batches */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (!exhausted && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_QUERY_REFILL) break;
                if (mode == M_WAIT) {
                    if (!(cur & RT_REF_LEAF)) {
                        if (__builtin_amdgcn_uicmp(w_zero_dir, 0u, RT_ICMP_NE) == 0ull) rt_descend<NT, true>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep);
                        else rt_descend<NT, false>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep);
                    }
                    if (cur & RT_REF_LEAF) {
                        rt_leaf_tris(cur, L, o, d, w_best, w_prim);
                        if (sp > 0) {
                            cur = rt_pop<NT>(sp, my_stack, w_best);
                        } else {
                            rt_mesh_merge(L, next_mesh - 1, w_best, w_prim, best_t, best_obj, best_prim);
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
struct rt_query_kernels {
    typedef rt_query_args args;
    template <int NT, bool HAS_MESH, int MODE, bool AOV> static constexpr auto kernel = &rt_query_kernel<NT, HAS_MESH, MODE, AOV>;
};

extern "C" hipError_t rt_launch_query(const rt_query_args *args, rt_shape shape, int aov, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_query_kernels>(args, shape, aov, num_cus, lds_bytes, stream);
}

#endif
