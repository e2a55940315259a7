/*
 * rt_sweep_kernel.h — sphere-cast queries: one moving ball per lane through the scene the render kernel stages, the time and place of its
 * first contact written out.  The arithmetic and the walk of a mesh are rt_sweep.h's (one text for the device and the host tests); the
 * scene staging is rt_traverse.h's, the launcher at the end (rt_ray_kernel.h's table over RT_SHAPES) is declared in rt_launch.h.  The kernel
 * runs behind the nearest-surface launch whose records it reads (rt_sweep_capi.cpp queues the two).
 *
 * What is found is the minimum of include/rt_amd.h's definition over every candidate of the scene: the objects that are not meshes in
 * list order from their LDS records (rt_sw_simple), then every mesh whose inflated root box the ball's path enters no later than the best
 * key so far, walked nearer child first (rt_sw_step).  The order changes nothing of the result - a subtree is skipped only when its key
 * is greater than the best so far, and no candidate in it has a smaller one by definition - so the lanes of a wave are free to go
 * different ways.  A ball that touches the scene at the start (its nearest-surface record is a hit) walks nothing.
 *
 * A lane is the query kernel's small state machine: FETCH (take the next ball, test the objects that are not meshes) -> MESH (the next
 * mesh entered early enough) -> WAIT (one step of the walk per round: one node or one triangle, so that lanes at nodes and lanes in leaves
 * keep each other busy) -> SHADE (form the record, store it) -> FETCH.  A wave takes ball ids 64 at a time from a global counter and
 * hands them to whichever lanes are free; the walk yields once RT_SWEEP_REFILL lanes hold a finished ball, and runs to its end once the
 * last are handed out.  Through the walk a lane carries (K, t, object, triangle, feature) only: the contact point is formed again for the
 * winner in SHADE.
 */
#ifndef RT_SWEEP_KERNEL_H
#define RT_SWEEP_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_ray_kernel.h"
#include "rt_sweep.h"
#include "rt_traverse.h"
#include "rt_vec.h"

#define RT_SWEEP_REFILL 16      /* lanes of a wave holding a finished ball before the walk yields to store and refill them (the query kernel's value; not tuned) */

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, 4) void rt_sweep_kernel(const rt_sweep_args a)
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

    /* per-lane ball and walk */
    int mode = M_FETCH;
    uint32_t id = 0;
    rt_mh_ray q;
    q.ox = q.oy = q.oz = q.dx = q.dy = q.dz = q.ix = q.iy = q.iz = 0.f;
    float r = 0.f, dd = 0.f;
    rt_sw_best best;
    best.k.d2 = 0.f; best.k.object = RT_NR_NONE; best.k.triangle = RT_NR_NONE; best.t = 0.f; best.feature = -1;
    rt_sw_walk w;
    w.cur = RT_REF_EMPTY_LEAF; w.key = 0.f; w.sp = 0; w.at = 0;
    int next_mesh = 0, w_obj = 0;
    /* wave-uniform: ball ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the winner is known; form the record and store it (48 bytes, three 16-byte stores) === */
        if (mode == M_SHADE) {
            rt_sweep rec;
            rt_sw_record(S, q, dd, r, best, a.nearest + id, rec);
            v4f *o = (v4f *)a.out + 3 * (size_t)id;
            v4f r0, r1, r2;
            r0.x = rec.t; r0.y = rec.centre[0]; r0.z = rec.centre[1]; r0.w = rec.centre[2];
            r1.x = rec.point[0]; r1.y = rec.point[1]; r1.z = rec.point[2]; r1.w = __int_as_float(rec.object);
            r2.x = __int_as_float(rec.triangle); r2.y = __int_as_float(rec.feature); r2.z = __int_as_float(rec.overlap); r2.w = __int_as_float(rec.reserved);
            o[0] = r0; o[1] = r1; o[2] = r2;
            mode = M_FETCH;
        }

        /* ================= FETCH: free lanes take the next ball ids (whole wave, as in rt_query_kernel) ================= */
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
                        const float *po = a.origins + 3 * (size_t)id, *pd = a.directions + 3 * (size_t)id;
                        q.ox = po[0]; q.oy = po[1]; q.oz = po[2];
                        q.dx = pd[0]; q.dy = pd[1]; q.dz = pd[2];
                        r = a.radius[id];
                        const bool has_limit = a.tmax != nullptr;
                        const float tmax = has_limit ? a.tmax[id] : 0.f;
                        mode = M_SHADE;
                        if (rt_sw_begin(q, r, has_limit, tmax, dd, best)) {
                            if (a.nearest[id].object >= 0) {
                                best.k.object = RT_SW_OVERLAP;          /* touching at the start: the record is the nearest one's, nothing is walked */
                            } else {
                                rt_sw_simple(S, a.num_objects, q, dd, r, best);
                                next_mesh = 0;
                                if (HAS_MESH && a.num_meshes > 0) mode = M_MESH;
                            }
                        }
                    }
                }
            }
        }

        if (HAS_MESH) {
            /* ================= MESH: the next mesh whose inflated root box is entered no later than the best key so far ===== */
            while (mode == M_MESH) {
                if (next_mesh >= a.num_meshes) { mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * next_mesh], m1 = L.meshes[2 * next_mesh + 1];
                next_mesh++;
                if (!rt_sw_mesh_begin(m0, m1, q, r, best, w)) continue;
                w_obj = (int)__float_as_uint(m1.w);
                mode = M_WAIT;
            }

            /* ================= WORK: steps of the walk ================================================================ */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); finished balls are stored, and their lanes refilled, in batches */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (!exhausted && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_SWEEP_REFILL) break;
                if (mode == M_WAIT) {
                    if (!rt_sw_step<NT>(S, my_stack, w_obj, q, dd, r, best, w)) mode = next_mesh >= a.num_meshes ? M_SHADE : M_MESH;
                }
            }
        }

        if (__ballot(mode != M_DONE) == 0ull) break;
    }
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
/* one front: both of rt_ray_launch's tables name the same thirteen kernels */
struct rt_sweep_kernels {
    typedef rt_sweep_args args;
    template <int NT, bool HAS_MESH, int MODE, bool> static constexpr auto kernel = &rt_sweep_kernel<NT, HAS_MESH, MODE>;
};

extern "C" hipError_t rt_launch_sweep(const rt_sweep_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_sweep_kernels>(args, shape, front, num_cus, lds_bytes, stream);
}

#endif
