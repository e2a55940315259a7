/*
 * rt_ao_kernel.h — the ambient-occlusion plane of a view, fused: per pixel the AOV pass's primary ray and its closest hit, then from the
 * hit's point P and shading normal N `samples` cosine-weighted directions of the renderer's own sampler on the pixel's own random stream,
 * each an occlusion query (rt_occlusion_kernel.h) of the limit `radius` from o' = P + N * bias; the pixel is the number of free samples
 * and that number over `samples` (include/rt_amd.h has the definition to the bit).  It calls START and the early exits of
 * rt_occlusion_kernel.h; the launcher at the end (rt_ray_kernel.h) is declared in rt_launch.h.
 *
 * A lane is the occlusion kernel's state machine with a pixel held across segments: FETCH (take a tile slot, form the primary ray) ->
 * START -> MESH -> WAIT (the primary segment has a NaN limit: no exit, and its meshes are merged into the closest hit) -> SHADE.  SHADE
 * of a primary ray that hit forms o', seeds the stream and draws the first direction; SHADE of a sample adds 1 - occ and draws the next
 * direction, or stores the pixel and goes to FETCH.  Every sample takes six draws whatever its outcome, so a pixel's directions do not
 * depend on what the earlier ones met.  A sample's direction is px_shade's diffuse direction (rt_pixel.h; Ray::true_lambertian_reflect
 * src/ray.cu:157-178): three normal_num draws, flipped against N, normalised, added to N, normalised.
 *
 * What a lane keeps between segments: N, o' (in `o`: the primary ray's origin is not needed again), the stream's word, the sample index
 * and the count.  The primary ray's direction, distance and hit go when o' is formed.
 */
#ifndef RT_AO_KERNEL_H
#define RT_AO_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_ao.h"
#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_occlusion_kernel.h"
#include "rt_ray_kernel.h"
#include "rt_surface.h"
#include "rt_traverse.h"
#include "rt_vec.h"

/* lanes of a wave holding an answered segment before the traversal loop yields to count them and start their next one: swept over
 * 8 / 16 / 24 / 32 with tools/ao_probe.py (DESIGN.md §14 has the table) */
#ifndef RT_AO_REFILL
#define RT_AO_REFILL 16
#endif

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, 4) void rt_ao_kernel(const rt_ao_args a)
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

    /* per-lane pixel, segment and traversal state */
    int mode = M_FETCH;
    uint32_t id = 0;
    V3 o = v3(0.f, 0.f, 0.f), d = o, inv = o, N = o;
    float tm = 0.f;                  /* the segment's limit; from MESH on clamped below RT_INF_F (rt_occlusion_start) */
    uint32_t occ = 0u;               /* something is in the way within the limit */
    int k = -1;                      /* the sample the lane is on; -1: its pixel's primary ray */
    uint32_t free_samples = 0u, rng = 0u;
    float best_t = RT_INF_F;         /* the primary ray's closest hit */
    int best_obj = -1, best_prim = -1, next_mesh = 0;
    uint32_t cur = 0, w_zero_dir = 0u;
    int sp = 0, w_prim = -1;
    float w_best = RT_INF_F;
    /* wave-uniform: tile slots [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the segment is answered ============================================== */
        if (mode == M_SHADE) {
            bool more;
            if (k < 0) {
                more = best_obj >= 0;
                if (more) {
                    /* the primary ray hit: the samples start from that surface, on the renderer's stream for this pixel (px_fetch) */
                    const uint32_t packed = __float_as_uint(L.objs[RT_OBJLDS_F4 * best_obj + 1].w);
                    V3 P;
                    float tex_u, tex_v;
                    rt_hit_surface(o, d, best_t, best_obj, best_prim, packed & ~16u, L, nullptr, P, N, tex_u, tex_v);     /* (no texture coordinates) */
                    o = N * a.bias + P;
                    rng = (id * 3u) * 3145739u + a.seed;
                    free_samples = 0u;
                    k = 0;
                } else {
                    free_samples = (uint32_t)RT_AO_NO_SURFACE;
                }
            } else {
                free_samples += 1u - occ;
                k++;
                more = k < a.samples;
            }
            if (more) {
                /* px_shade's diffuse direction */
                const float gx = normal_num<true, false>(rng);
                const float gy = normal_num<true, false>(rng);
                const float gz = normal_num<true, false>(rng);
                V3 rv = v3(gx, gy, gz);
                if (dot(rv, N) < 0.0f) rv = neg(rv);
                rv = normalised(rv);
                d = normalised(N + rv);
                tm = a.radius;
                mode = M_START;
            } else {
                /* ordinary vector stores: two bytes and four per pixel */
                if (a.count) a.count[id] = (uint16_t)free_samples;
                if (a.ao) a.ao[id] = k < 0 ? 1.0f : (float)free_samples / (float)a.samples;
                mode = M_FETCH;
            }
        }

        /* ================= FETCH: free lanes take the next tile slots (whole wave, as in rt_occlusion_kernel) == */
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
                        /* a chunk is an 8x8 tile; a slot of a ragged edge tile outside the image is no pixel: the lane stays in FETCH */
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
                            k = -1;
                            mode = M_START;
                        }
                    }
                }
            }
        }

        /* ================= START: the segment meets the top-level objects; first exit =================== */
        if (mode == M_START) rt_occlusion_start<HAS_MESH>(a, L, o, d, inv, tm, best_t, best_obj, best_prim, occ, next_mesh, mode);

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

            /* ================= WORK: traversal macro steps (rt_occlusion_kernel's) ============================ */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); answered segments are counted, and their lanes' next ones started, in
                 * batches - also once the last tile is handed out: the lanes still have samples to start */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (__popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_AO_REFILL) break;
                if (mode == M_WAIT) {
                    if (!(cur & RT_REF_LEAF)) {
                        if (__builtin_amdgcn_uicmp(w_zero_dir, 0u, RT_ICMP_NE) == 0ull) rt_descend<NT, true>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep);
                        else rt_descend<NT, false>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep);
                    }
                    if (cur & RT_REF_LEAF) {
                        rt_leaf_tris(cur, L, o, d, w_best, w_prim);
                        if (w_best <= tm) {
                            /* second exit: this mesh's running best is within the limit, and it can only fall (never taken on a primary
                             * segment: its limit is NaN) */
                            occ = 1u;
                            mode = M_SHADE;
                        } else if (sp > 0) {
                            cur = rt_pop<NT>(sp, my_stack, w_best);
                        } else {
                            if (k < 0) rt_mesh_merge(L, next_mesh - 1, w_best, w_prim, best_t, best_obj, best_prim);      /* (the primary ray's closest hit) */
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
/* one front: both of rt_ray_launch's tables name the same thirteen kernels */
struct rt_ao_kernels {
    typedef rt_ao_args args;
    template <int NT, bool HAS_MESH, int MODE, bool> static constexpr auto kernel = &rt_ao_kernel<NT, HAS_MESH, MODE>;
};

extern "C" hipError_t rt_launch_ao(const rt_ao_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_ao_kernels>(args, shape, front, num_cus, lds_bytes, stream);
}

#endif
