/*
 * rt_overlap_kernel.h — box-overlap queries: one box per lane against the scene the render kernel stages, the number of surfaces that
 * touch it, whether any does, and the k lowest of their ids written out.  The tests, the id buffer and the walk of a mesh are
 * rt_overlap.h's (one text for the device and the host tests); the scene staging is rt_traverse.h's, the launcher at the end
 * (rt_ray_kernel.h's table over RT_SHAPES) is declared in rt_launch.h.
 *
 * What is found is include/rt_amd.h's set: the objects that are not meshes in list order from their LDS records (rt_ov_simple), then
 * every mesh whose root box overlaps the box, walked by compares alone (rt_ov_step).  The order changes nothing of the result - a
 * subtree is skipped only when its box does not overlap the query box, and no candidate below it counts then by definition - so the
 * lanes of a wave are free to go different ways.
 *
 * A lane is the nearest kernel's state machine: FETCH (take the next box, test the objects that are not meshes) -> MESH (the next mesh
 * whose root box overlaps) -> WAIT (one step of the walk per round: one node or one triangle) -> SHADE (store the answers) -> FETCH.
 * A wave takes box ids 64 at a time from a global counter and hands them to whichever lanes are free; the walk yields once
 * RT_OVERLAP_REFILL lanes hold a finished box, and runs to its end once the last boxes are handed out.  The per-lane stack is the
 * scene's ([entry][thread], one pending sibling per level).  The ids live in registers: an indexed array would be scratch.  In any-only
 * mode (a wave-uniform flag of the argument block) a lane whose count is above zero goes to SHADE.
 *
 * Not in the development builds (rt_ray_kernels.h decides; the launcher refuses there), like the multi-hit kernel.
 */
#ifndef RT_OVERLAP_KERNEL_H
#define RT_OVERLAP_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_overlap.h"
#include "rt_ray_kernels.h"     /* RT_RAY_KERNELS_BUILT */

#if RT_RAY_KERNELS_BUILT
#include "rt_device_scene.h"
#include "rt_launch.h"
#include "rt_ray_kernel.h"
#include "rt_traverse.h"
#include "rt_vec.h"

#define RT_OVERLAP_REFILL 16    /* lanes of a wave holding a finished box before the walk yields to store and refill them (the query kernel's value; not tuned) */

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, 4) void rt_overlap_kernel(const rt_overlap_args a)
{
    extern __shared__ v4f lds_raw[];
    const int tid = threadIdx.x;
    const int lane = tid & (RT_WAVE - 1);

    Lds L;
    uint2 *stack;        /* [stack_entries + 1][NT], as in rt_render_kernel */
    rt_stage_scene<NT, MODE>(a, lds_raw, tid, L, stack);
    __syncthreads();
    uint32_t *const my_stack = (uint32_t *)(stack + tid);
    rt_ov_scene<v4f> S;
    S.nodes = L.nodes; S.tris = L.tris; S.meshes = L.meshes; S.objtab = L.objtab;
    const int32_t k = a.k;
    const bool any_only = a.any_only != 0;

    /* per-lane box, buffer and walk */
    int mode = M_FETCH;
    uint32_t id = 0;
    rt_ov_box box;
    box.lox = box.loy = box.loz = box.hix = box.hiy = box.hiz = box.cx = box.cy = box.cz = box.hx = box.hy = box.hz = 0.f;
    rt_ov_buf buf;
    rt_ov_clear(buf);
    rt_ov_walk w;
    w.cur = RT_REF_EMPTY_LEAF; w.sp = 0; w.at = 0;
    int next_mesh = 0, w_obj = 0;
    /* wave-uniform: box ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the box is finished; its count, its byte, its ids (whole 8-byte records) ============== */
        if (mode == M_SHADE) {
            const uint32_t total = buf.total;
            int32_t *const counts = a.counts;
            if (counts) counts[id] = (int32_t)total;
            uint8_t *const any = a.any;
            if (any) any[id] = total > 0u ? (uint8_t)1 : (uint8_t)0;
            if (k > 0) {
                int2 *const out = (int2 *)a.ids + (size_t)id * (size_t)k;
                /* rank q is slot q: slot 0 is read and the slots move down by one, so that no slot is picked by an index.  One 8-byte
                 * store per id: the paired 16-byte stores an even k allows were tried, and their second loop cost the global-placement
                 * mesh shape two spilled scalar registers */
#pragma unroll 1
                for (int32_t q = 0; q < k; q++) {
                    const rt_overlap_id r0 = rt_ov_id(buf.id[0], (uint32_t)q < total);
#pragma unroll
                    for (int j = 0; j < RT_OVERLAP_MAX - 1; j++) buf.id[j] = buf.id[j + 1];
                    int2 v;
                    v.x = r0.object; v.y = r0.triangle;
                    out[q] = v;
                }
            }
            mode = M_FETCH;
        }

        /* ================= FETCH: free lanes take the next box ids (whole wave, as in rt_query_kernel) ================== */
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
                        const float *ql = a.lo + 3 * (size_t)id, *qh = a.hi + 3 * (size_t)id;
                        box.lox = ql[0]; box.loy = ql[1]; box.loz = ql[2];
                        box.hix = qh[0]; box.hiy = qh[1]; box.hiz = qh[2];
                        rt_ov_clear(buf);
                        mode = M_SHADE;
                        if (rt_ov_begin(box)) {
                            rt_ov_simple(S, a.num_objects, box, k, any_only, buf);
                            next_mesh = 0;
                            if (HAS_MESH && !(any_only && buf.total > 0u)) mode = M_MESH;        /* (a scene without a mesh on a mesh shape leaves MESH at once) */
                        }
                    }
                }
            }
        }

        if (HAS_MESH) {
            /* ================= MESH: the next mesh whose root box overlaps the box ========================================== */
            while (mode == M_MESH) {
                if (next_mesh >= a.num_meshes) { mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * next_mesh], m1 = L.meshes[2 * next_mesh + 1];
                next_mesh++;
                if (!rt_ov_mesh_begin(m0, m1, box, w)) continue;
                w_obj = (int)__float_as_uint(m1.w);
                mode = M_WAIT;
            }

            /* ================= WORK: steps of the walk ================================================================== */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); finished boxes are stored, and their lanes refilled, in batches */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (!exhausted && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_OVERLAP_REFILL) break;
                if (mode == M_WAIT) {
                    const bool more = rt_ov_step<NT>(S, my_stack, w_obj, box, k, buf, w);
                    if (any_only && buf.total > 0u) mode = M_SHADE;
                    else if (!more) mode = next_mesh >= a.num_meshes ? M_SHADE : M_MESH;
                }
            }
        }

        if (__ballot(mode != M_DONE) == 0ull) break;
    }
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
/* one front: both of rt_ray_launch's tables name the same thirteen kernels */
struct rt_overlap_kernels {
    typedef rt_overlap_args args;
    template <int NT, bool HAS_MESH, int MODE, bool> static constexpr auto kernel = &rt_overlap_kernel<NT, HAS_MESH, MODE>;
};

extern "C" hipError_t rt_launch_overlap(const rt_overlap_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_overlap_kernels>(args, shape, front, num_cus, lds_bytes, stream);
}
#endif

#endif
