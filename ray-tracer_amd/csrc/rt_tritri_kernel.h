/*
 * rt_tritri_kernel.h — triangle-overlap queries: one query triangle per lane against the scene the render kernel stages, the number of
 * surfaces it cuts, whether it cuts any, the k lowest of their ids and, where asked, each pair's segment written out.  The tests and
 * the walk of a mesh are rt_tritri.h's, the id buffer rt_overlap.h's (one text for the device and the host tests); the scene staging is
 * rt_traverse.h's, the launcher at the end (rt_ray_kernel.h's table over RT_SHAPES) is declared in rt_launch.h.
 *
 * It is the box-overlap kernel's state machine (rt_overlap_kernel.h has the account: FETCH -> MESH -> WAIT -> SHADE, the chunked refill,
 * one node or ONE triangle per step) with another leaf test.  A lane keeps a0..a2, na, lo, hi, the count, eight ids and the walk.
 * The segments are formed in SHADE from the finished ids, rank by rank: the pair's record is read again and taken through the same
 * steps (rt_tt_record<true>), which costs the walk no register.
 *
 * Not in the development builds (rt_ray_kernels.h decides; the launcher refuses there), like the multi-hit kernel.
 */
#ifndef RT_TRITRI_KERNEL_H
#define RT_TRITRI_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_ray_kernels.h"     /* RT_RAY_KERNELS_BUILT */
#include "rt_tritri.h"

#if RT_RAY_KERNELS_BUILT
#include "rt_device_scene.h"
#include "rt_launch.h"
#include "rt_ray_kernel.h"
#include "rt_traverse.h"
#include "rt_vec.h"

#define RT_TRITRI_REFILL 16     /* lanes of a wave holding a finished query before the walk yields to store and refill them (the query kernel's value; not tuned) */

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, 4) void rt_tritri_kernel(const rt_tritri_args a)
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

    /* per-lane query, buffer and walk */
    int mode = M_FETCH;
    uint32_t id = 0;
    rt_tt_tri t;
    t.a0x = t.a0y = t.a0z = t.a1x = t.a1y = t.a1z = t.a2x = t.a2y = t.a2z = t.nx = t.ny = t.nz = 0.f;
    t.box.lox = t.box.loy = t.box.loz = t.box.hix = t.box.hiy = t.box.hiz = t.box.cx = t.box.cy = t.box.cz = t.box.hx = t.box.hy = t.box.hz = 0.f;
    rt_ov_buf buf;
    rt_ov_clear(buf);
    rt_ov_walk w;
    w.cur = RT_REF_EMPTY_LEAF; w.sp = 0; w.at = 0;
    int next_mesh = 0, w_obj = 0;
    /* wave-uniform: query ids [next, end) in hand */
    uint32_t next = 0, end = 0;
    bool exhausted = false;

    for (;;) {
        /* ================= SHADE: the query is finished; its count, its byte, its ids (8-byte records), its segments (two 16-byte stores) ==== */
        if (mode == M_SHADE) {
            const uint32_t total = buf.total;
            int32_t *const counts = a.counts;
            if (counts) counts[id] = (int32_t)total;
            uint8_t *const any = a.any;
            if (any) any[id] = total > 0u ? (uint8_t)1 : (uint8_t)0;
            if (k > 0) {
                int2 *const out = (int2 *)a.ids + (size_t)id * (size_t)k;
                v4f *const segs = a.segments ? (v4f *)a.segments + 2 * ((size_t)id * (size_t)k) : nullptr;
                /* rank q is slot q: slot 0 is read and the slots move down by one, so that no slot is picked by an index */
#pragma unroll 1
                for (int32_t q = 0; q < k; q++) {
                    const uint32_t word = buf.id[0];
                    const bool held = (uint32_t)q < total;
                    const rt_overlap_id r0 = rt_ov_id(word, held);
#pragma unroll
                    for (int j = 0; j < RT_OVERLAP_MAX - 1; j++) buf.id[j] = buf.id[j + 1];
                    int2 v;
                    v.x = r0.object; v.y = r0.triangle;
                    out[q] = v;
                    if (segs) {
                        const rt_tri_segment sg = rt_tt_segment(S, word, held, t);
                        v4f s0, s1;
                        s0.x = sg.p[0]; s0.y = sg.p[1]; s0.z = sg.p[2]; s0.w = sg.q[0];
                        s1.x = sg.q[1]; s1.y = sg.q[2]; s1.z = __int_as_float(sg.kind); s1.w = __int_as_float(sg.reserved);
                        segs[2 * q] = s0; segs[2 * q + 1] = s1;
                    }
                }
            }
            mode = M_FETCH;
        }

        /* ================= FETCH: free lanes take the next query ids (whole wave, as in rt_query_kernel) ================== */
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
                        const float *qt = a.tris + 9 * (size_t)id;
                        t.a0x = qt[0]; t.a0y = qt[1]; t.a0z = qt[2];
                        t.a1x = qt[3]; t.a1y = qt[4]; t.a1z = qt[5];
                        t.a2x = qt[6]; t.a2y = qt[7]; t.a2z = qt[8];
                        rt_ov_clear(buf);
                        mode = M_SHADE;
                        if (rt_tt_begin(t)) {
                            rt_tt_simple(S, a.num_objects, t, k, any_only, buf);
                            next_mesh = 0;
                            if (HAS_MESH && !(any_only && buf.total > 0u)) mode = M_MESH;        /* (a scene without a mesh on a mesh shape leaves MESH at once) */
                        }
                    }
                }
            }
        }

        if (HAS_MESH) {
            /* ================= MESH: the next mesh whose root box overlaps the query's bounding box ========================= */
            while (mode == M_MESH) {
                if (next_mesh >= a.num_meshes) { mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * next_mesh], m1 = L.meshes[2 * next_mesh + 1];
                next_mesh++;
                if (!rt_ov_mesh_begin(m0, m1, t.box, w)) continue;
                w_obj = (int)__float_as_uint(m1.w);
                mode = M_WAIT;
            }

            /* ================= WORK: steps of the walk ================================================================== */
            for (;;) {
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                if (m_wait == 0ull) break;
                /* a lane between two meshes goes round at once (cheap); finished queries are stored, and their lanes refilled, in batches */
                if (__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_MESH, RT_ICMP_EQ) != 0ull) break;
                if (!exhausted && __popcll(__builtin_amdgcn_uicmp((unsigned)mode, (unsigned)M_SHADE, RT_ICMP_EQ)) >= RT_TRITRI_REFILL) break;
                if (mode == M_WAIT) {
                    const bool more = rt_tt_step<NT>(S, my_stack, w_obj, t, k, buf, w);
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
struct rt_tritri_kernels {
    typedef rt_tritri_args args;
    template <int NT, bool HAS_MESH, int MODE, bool> static constexpr auto kernel = &rt_tritri_kernel<NT, HAS_MESH, MODE>;
};

extern "C" hipError_t rt_launch_tritri(const rt_tritri_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    return rt_ray_launch<rt_tritri_kernels>(args, shape, front, num_cus, lds_bytes, stream);
}
#endif

#endif
