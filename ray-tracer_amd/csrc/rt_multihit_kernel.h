/*
 * rt_multihit_kernel.h — multi-hit ray queries: one ray per lane through the scene the render kernel stages, the first k candidates along
 * it (or only their number) written out.  The candidate tests, the buffer and the walk of a mesh are rt_multihit.h's (one text for the
 * device and the host tests); the scene staging is rt_traverse.h's, a record's surface is rt_surface.h's, the launcher at the end
 * (rt_ray_kernel.h's table over RT_SHAPES) is declared in rt_launch.h.
 *
 * What is found is the first k of include/rt_amd.h's ordered candidates: the objects that are not meshes in list order from their LDS
 * records (rt_mh_simple), each accepted one offered to the buffer, then every mesh whose root box the ray enters no later than the
 * threshold, walked nearer child first (rt_mh_step).  The order changes nothing of the result - a subtree is skipped only when the ray
 * misses its box or enters it beyond the threshold, and no candidate in it has a smaller key than that by definition - so the lanes of a
 * wave are free to go different ways.
 *
 * A lane is a small state machine as in the query kernel: FETCH (take the next ray, test the objects that are not meshes) -> MESH (the
 * next mesh entered early enough) -> WAIT (one step of the walk per round) -> SHADE (form the records, store them) -> FETCH.  A wave
 * takes ray ids 64 at a time from a global counter and hands them to whichever lanes are free; the walk yields once RT_MULTIHIT_REFILL
 * lanes hold a finished ray, and runs to its end once the last rays are handed out.  The per-lane stack is the scene's ([entry][thread],
 * one pending sibling per level).  The buffer lives in registers: LDS is the scene's (blob plus stack, whatever the shape), and an
 * indexed array would be scratch.
 *
 * One part of a record is not formed here: the texture coordinates of a sphere whose material needs them are rt_multihit_uv_kernel's, a pass
 * over the records behind this kernel (below, with the reason).
 *
 * Not in the development builds (rt_ray_kernels.h decides; the launchers refuse there), like the other ray kernels.
 */
#ifndef RT_MULTIHIT_KERNEL_H
#define RT_MULTIHIT_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_multihit.h"
#include "rt_ray_kernels.h"     /* RT_RAY_KERNELS_BUILT */

#if RT_RAY_KERNELS_BUILT
#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_math.h"
#include "rt_ray_kernel.h"
#include "rt_surface.h"
#include "rt_traverse.h"
#include "rt_vec.h"

#define RT_MULTIHIT_REFILL 16   /* lanes of a wave holding a finished ray before the walk yields to store and refill them (the query kernel's value; not tuned) */

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, 4) void rt_multihit_kernel(const rt_multihit_args a)
{
    extern __shared__ v4f lds_raw[];
    const int tid = threadIdx.x;
    const int lane = tid & (RT_WAVE - 1);

    Lds L;
    uint2 *stack;        /* [stack_entries + 1][NT], as in rt_render_kernel */
    rt_stage_scene<NT, MODE>(a, lds_raw, tid, L, stack);
    __syncthreads();
    rt_mh_entry *const my_stack = (rt_mh_entry *)(stack + tid);
    rt_mh_scene<v4f> S;
    S.nodes = L.nodes; S.tris = L.tris; S.meshes = L.meshes; S.objtab = L.objtab;
    const int32_t k = a.k;

    /* per-lane ray, buffer and walk */
    int mode = M_FETCH;
    uint32_t id = 0;
    rt_mh_ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.f;
    float lim = 0.f;
    rt_mh_buf buf;
    rt_mh_clear(buf);
    rt_mh_walk w;
    w.cur = RT_REF_EMPTY_LEAF; w.key = 0.f; w.sp = 0; w.at = 0;
    int next_mesh = 0, w_obj = 0;
    /* wave-uniform: ray ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the ray is finished; its records (48 bytes, three 16-byte stores each) ====================== */
        if (mode == M_SHADE) {
            const int32_t count = rt_mh_count(buf, k);
            int32_t *const counts = a.counts;
            if (counts) counts[id] = count;
            v4f *const h = (v4f *)a.hits + 3 * ((size_t)id * (size_t)k);
            const float *const tri_uv = a.tri_uv;
            /* rank q is slot q: slot 0 is read and the slots move down by one, so that no slot is picked by an index */
#pragma unroll 1
            for (int32_t q = 0; q < k; q++) {
                const uint64_t word = buf.key[0];
                const float t = buf.t[0];
#pragma unroll
                for (int j = 0; j < RT_MULTIHIT_MAX - 1; j++) { buf.key[j] = buf.key[j + 1]; buf.t[j] = buf.t[j + 1]; }
                v4f r0, r1, r2;
                if (q < count) {
                    const int obj = rt_mh_word_object(word), prim = rt_mh_word_triangle(word);
                    const uint32_t packed = __float_as_uint(L.objs[RT_OBJLDS_F4 * obj + 1].w);
                    V3 P, N;
                    float tex_u, tex_v;
                    /* a sphere's texture coordinates are rt_multihit_uv_kernel's (below): here its record gets 0, 0 */
                    const V3 ro = v3(r.ox, r.oy, r.oz), rd = v3(r.dx, r.dy, r.dz);
                    if (packed & 32u) rt_hit_surface(ro, rd, t, obj, prim, 32u, L, tri_uv, P, N, tex_u, tex_v);
                    else rt_hit_surface(ro, rd, t, obj, prim, packed & 16u, L, tri_uv, P, N, tex_u, tex_v);
                    r0.x = t; r0.y = P.x; r0.z = P.y; r0.w = P.z;
                    r1.x = N.x; r1.y = N.y; r1.z = N.z; r1.w = __int_as_float(obj);
                    r2.x = __int_as_float(prim); r2.y = tex_u; r2.z = tex_v; r2.w = 0.0f;
                } else {
                    r0.x = RT_INF_F; r0.y = 0.f; r0.z = 0.f; r0.w = 0.f;
                    r1.x = 0.f; r1.y = 0.f; r1.z = 0.f; r1.w = __int_as_float(-1);
                    r2.x = __int_as_float(-1); r2.y = 0.f; r2.z = 0.f; r2.w = 0.0f;
                }
                h[3 * q] = r0; h[3 * q + 1] = r1; h[3 * q + 2] = r2;
            }
            mode = M_FETCH;
        }

        /* ================= FETCH: free lanes take the next ray ids (whole wave, as in rt_query_kernel) ================== */
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
                        const float *qo = a.origins + 3 * (size_t)id, *qd = a.directions + 3 * (size_t)id;
                        r.ox = qo[0]; r.oy = qo[1]; r.oz = qo[2];
                        r.dx = qd[0]; r.dy = qd[1]; r.dz = qd[2];
                        const float *const limits = a.tmax;
                        const bool has_limit = limits != nullptr;
                        const float tmax = has_limit ? limits[id] : 0.f;
                        rt_mh_clear(buf);
                        mode = M_SHADE;
                        if (rt_mh_begin(r, has_limit, tmax, lim)) {
                            rt_mh_simple(S, a.num_objects, r, lim, k, buf);
                            next_mesh = 0;
                            if (HAS_MESH) mode = M_MESH;        /* (a scene without a mesh on a mesh shape leaves MESH at once) */
                        }
                    }
                }
            }
        }

        if (HAS_MESH) {
            /* ================= MESH: the next mesh whose root box the ray enters no later than the threshold ================ */
            while (mode == M_MESH) {
                if (next_mesh >= a.num_meshes) { mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * next_mesh], m1 = L.meshes[2 * next_mesh + 1];
                next_mesh++;
                if (!rt_mh_mesh_begin(m0, m1, r, rt_mh_threshold(buf, lim, k), w)) continue;
                w_obj = (int)__float_as_uint(m1.w);
                mode = M_WAIT;
            }

            /* ================= WORK: steps of the walk ================================================================== */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); finished rays are stored, and their lanes refilled, in batches */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (!exhausted && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_MULTIHIT_REFILL) break;
                if (mode == M_WAIT) {
                    if (!rt_mh_step<NT>(S, my_stack, w_obj, r, lim, k, buf, w)) mode = next_mesh >= a.num_meshes ? M_SHADE : M_MESH;
                }
            }
        }

        if (__ballot(mode != M_DONE) == 0ull) break;
    }
}

/* The texture coordinates of the records that lie on a sphere whose material needs them: Sphere::assign_texture_coords (src/objects.cu:82-97)
 * from the record's own point, rt_surface.h's expressions stated once more.  A pass of its own over the n * k records, launched behind
 * rt_multihit_kernel only for a scene that has such a sphere: inside that kernel the binary64 constants of asin and acos, which the compiler
 * holds in scalar registers across the whole wave loop, do not fit beside the loop's own scalars, and it spills them. */
__global__ __launch_bounds__(256) void rt_multihit_uv_kernel(const rt_multihit_uv_args a)
{
    const v4f *const objs = (const v4f *)a.objlds;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.records; i += (int64_t)gridDim.x * 256) {
        v4f *const h = (v4f *)a.hits + 3 * (size_t)i;
        const v4f r0 = h[0];
        const int obj = __float_as_int(h[1].w);
        if (obj < 0) continue;
        const uint32_t packed = __float_as_uint(objs[RT_OBJLDS_F4 * obj + 1].w);
        if ((packed & 48u) != 48u) continue;                 /* not a sphere, or no texture coordinates wanted */
        const v4f sc = objs[RT_OBJLDS_F4 * obj + 2];
        const V3 P = v3(r0.y, r0.z, r0.w);
        const float PI = 3.141592653589793f;
        const float theta = rt_asinf((P.y - sc.y) / sc.w);
        const float phi = rt_acosf((P.x - sc.x) / sc.w);
        const float tex_u = (theta + PI / 2) / PI;
        const float v_ratio = (1 - phi / PI) / 2;
        const int behind = P.z > sc.z ? 1 : 0;
        const int mult = 1 - 2 * behind;
        const float tex_v = (float)(1 * behind) + (float)mult * v_ratio;
        v4f r2 = h[2];
        r2.y = tex_u; r2.z = tex_v;
        h[2] = r2;
    }
}

extern "C" hipError_t rt_launch_multihit_uv(const rt_multihit_uv_args *args, int num_cus, hipStream_t stream)
{
    if (args->records <= 0) return hipSuccess;
    long long blocks = (args->records + 255) / 256;
    const long long cap = (long long)(num_cus > 0 ? num_cus : 1) * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(rt_multihit_uv_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
/* one front: both of rt_ray_launch's tables name the same thirteen kernels */
struct rt_multihit_kernels {
    typedef rt_multihit_args args;
    template <int NT, bool HAS_MESH, int MODE, bool> static constexpr auto kernel = &rt_multihit_kernel<NT, HAS_MESH, MODE>;
};

extern "C" hipError_t rt_launch_multihit(const rt_multihit_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_multihit_kernels>(args, shape, front, num_cus, lds_bytes, stream);
}
#endif

#endif
