/*
 * rt_nearest_kernel.h — nearest-surface queries: one point per lane through the scene the render kernel stages, the closest surface point
 * and its distance written out.  The arithmetic and the walk of a mesh are rt_nearest.h's (one text for the device and the host tests);
 * the scene staging is rt_traverse.h's, the launcher at the end (rt_ray_kernel.h's table over RT_SHAPES) is declared in rt_launch.h.
 *
 * What is found is the minimum of include/rt_amd.h's definition over every candidate of the scene: the objects that are not meshes in
 * list order from their LDS records (rt_nr_simple), then every mesh whose root box is not farther than the best so far, walked nearest
 * child first (rt_nr_step).  The order changes nothing of the result - a subtree is skipped only when its path value is greater than
 * the best so far, and no candidate in it is nearer than that by definition - so the lanes of a wave are free to go different ways.
 *
 * A lane is a small state machine as in the query kernel: FETCH (take the next point, test the objects that are not meshes) -> MESH (the
 * next mesh near enough) -> WAIT (one step of the walk per round) -> SHADE (form the record, store it) -> FETCH.  A wave takes point ids
 * 64 at a time from a global counter and hands them to whichever lanes are free; the walk yields once RT_NEAREST_REFILL lanes hold a
 * finished point, and runs to its end once the last points are handed out.  The per-lane stack is the scene's ([entry][thread], one
 * pending sibling per level): the farther child is pushed only when it may still hold the winner.
 */
#ifndef RT_NEAREST_KERNEL_H
#define RT_NEAREST_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_nearest.h"
#include "rt_ray_kernel.h"
#include "rt_traverse.h"
#include "rt_vec.h"

#define RT_NEAREST_REFILL 16    /* lanes of a wave holding a finished point before the walk yields to store and refill them (the query kernel's value; not tuned) */

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, 4) void rt_nearest_kernel(const rt_nearest_args a)
{
    extern __shared__ v4f lds_raw[];
    const int tid = threadIdx.x;
    const int lane = tid & (RT_WAVE - 1);

    Lds L;
    uint2 *stack;        /* [stack_entries + 1][NT], as in rt_render_kernel */
    rt_stage_scene<NT, MODE>(a, lds_raw, tid, L, stack);
    __syncthreads();
    rt_nr_entry *const my_stack = (rt_nr_entry *)(stack + tid);
    rt_nr_scene<v4f> S;
    S.nodes = L.nodes; S.tris = L.tris; S.meshes = L.meshes; S.objtab = L.objtab;

    /* per-lane point and walk */
    int mode = M_FETCH;
    uint32_t id = 0;
    float px = 0.f, py = 0.f, pz = 0.f;
    rt_nr_best best;
    best.d2 = 0.f; best.object = RT_NR_NONE; best.triangle = RT_NR_NONE;
    rt_nr_walk w;
    w.cur = RT_REF_EMPTY_LEAF; w.key = 0.f; w.sp = 0;
    int next_mesh = 0, w_obj = 0;
    /* wave-uniform: point ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the winner is known; form the record and store it (32 bytes, two 16-byte stores) ===== */
        if (mode == M_SHADE) {
            rt_nearest r;
            rt_nr_record(S, px, py, pz, best, r);
            v4f *o = (v4f *)a.out + 2 * (size_t)id;
            v4f r0, r1;
            r0.x = r.distance; r0.y = r.distance2; r0.z = r.point[0]; r0.w = r.point[1];
            r1.x = r.point[2]; r1.y = __int_as_float(r.object); r1.z = __int_as_float(r.triangle); r1.w = __int_as_float(r.reserved);
            o[0] = r0; o[1] = r1;
            mode = M_FETCH;
        }

        /* ================= FETCH: free lanes take the next point ids (whole wave, as in rt_query_kernel) =============== */
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
                        const float *q = a.points + 3 * (size_t)id;
                        px = q[0]; py = q[1]; pz = q[2];
                        const bool has_limit = a.max_dist != nullptr;
                        const float max_dist = has_limit ? a.max_dist[id] : 0.f;
                        mode = M_SHADE;
                        if (rt_nr_begin(px, py, pz, has_limit, max_dist, best)) {
                            rt_nr_simple(S, a.num_objects, px, py, pz, best);
                            next_mesh = 0;
                            if (HAS_MESH && a.num_meshes > 0) mode = M_MESH;
                        }
                    }
                }
            }
        }

        if (HAS_MESH) {
            /* ================= MESH: the next mesh whose root box is not farther than the best so far ===================== */
            while (mode == M_MESH) {
                if (next_mesh >= a.num_meshes) { mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * next_mesh], m1 = L.meshes[2 * next_mesh + 1];
                next_mesh++;
                if (!rt_nr_mesh_begin(m0, m1, px, py, pz, best, w)) continue;
                w_obj = (int)__float_as_uint(m1.w);
                mode = M_WAIT;
            }

            /* ================= WORK: steps of the walk ================================================================ */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); finished points are stored, and their lanes refilled, in batches */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (!exhausted && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_NEAREST_REFILL) break;
                if (mode == M_WAIT) {
                    if (!rt_nr_step<NT>(S, my_stack, w_obj, px, py, pz, best, w)) mode = next_mesh >= a.num_meshes ? M_SHADE : M_MESH;
                }
            }
        }

        if (__ballot(mode != M_DONE) == 0ull) break;
    }
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
/* one front: both of rt_ray_launch's tables name the same thirteen kernels */
struct rt_nearest_kernels {
    typedef rt_nearest_args args;
    template <int NT, bool HAS_MESH, int MODE, bool> static constexpr auto kernel = &rt_nearest_kernel<NT, HAS_MESH, MODE>;
};

extern "C" hipError_t rt_launch_nearest(const rt_nearest_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_nearest_kernels>(args, shape, front, num_cus, lds_bytes, stream);
}

#endif
