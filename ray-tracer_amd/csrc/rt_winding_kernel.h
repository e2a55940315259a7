/*
 * rt_winding_kernel.h — winding-number queries: one point per lane, the generalized winding number of an object or of the scene's solids
 * written out, or the sign it gives a nearest-surface distance.  The arithmetic and the loops are rt_winding.h's (one text for the device
 * and the host tests); the launcher at the end is declared in rt_launch.h.
 *
 * A dense points x triangles reduction, unlike every other kernel here: no lane state machine, no stack, no LDS.  A wave takes point ids 64
 * at a time from a global counter, as the nearest-surface kernel does, and then every lane runs the SAME loop over objects and records -
 * the bounds and the addresses come from the scene alone - so the only divergence is the tail of the last chunk, whose idle lanes compute
 * on a stand-in point and store nothing.  The records, the object table, the order list and the flip words are read from global memory
 * through const __restrict__ kernel parameters by wave-uniform indices, which lets the compiler read them with scalar loads into SGPRs:
 * one load per wave and record instead of one per lane, and nothing staged.  The sum over a point's records is sequential per lane: that
 * order is part of the definition (include/rt_amd.h).
 */
#ifndef RT_WINDING_KERNEL_H
#define RT_WINDING_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_vec.h"
#include "rt_winding.h"

#define RT_WINDING_THREADS 256          /* four waves: nothing is shared between them */
#define RT_WINDING_BLOCKS_PER_CU 8      /* 32 waves per CU, eight per SIMD: the scalar loads' latency is other waves' arithmetic */

__global__ __launch_bounds__(RT_WINDING_THREADS) void rt_winding_kernel(const v4f *__restrict__ tris, const v4f *__restrict__ objtab,
                                                                        const int32_t *__restrict__ perm, const uint32_t *__restrict__ flip,
                                                                        const float *__restrict__ points, const rt_nearest *__restrict__ nearest,
                                                                        uint32_t *__restrict__ counter, float *__restrict__ winding,
                                                                        uint8_t *__restrict__ inside, float *__restrict__ sdf, int32_t num_objects,
                                                                        int32_t num_tris, int32_t object, uint32_t n, uint32_t num_chunks)
{
    const int lane = threadIdx.x & (RT_WAVE - 1);
    rt_wn_scene<v4f> S;
    S.tris = tris; S.objtab = objtab; S.perm = perm; S.flip = flip; S.num_objects = num_objects; S.num_tris = num_tris;
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(counter, 1u);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        if (c >= num_chunks) break;
        const uint32_t id = c * 64u + (uint32_t)lane;
        const bool live = id < n;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (live) {
            const float *q = points + 3 * (size_t)id;
            px = q[0]; py = q[1]; pz = q[2];
        }
        const float w = rt_wn_point(S, object, px, py, pz);
        if (live) {
            if (winding) winding[id] = w;
            if (inside) inside[id] = rt_wn_inside(w) ? 1 : 0;
            if (sdf) sdf[id] = rt_wn_sdf(w, nearest[id].distance);
        }
    }
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
extern "C" hipError_t rt_launch_winding(const rt_winding_args *a, int num_cus, hipStream_t stream)
{
    const uint32_t waves = RT_WINDING_THREADS / RT_WAVE;
    uint32_t blocks = (a->num_chunks + waves - 1) / waves;
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 1) * RT_WINDING_BLOCKS_PER_CU;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_winding_kernel, dim3(blocks), dim3(RT_WINDING_THREADS), 0, stream, (const v4f *)a->blob + a->off_tris,
                       (const v4f *)a->blob + a->off_objtab, a->perm, a->flip, a->points, a->nearest, a->counter, a->winding, a->inside, a->sdf,
                       a->num_objects, a->num_tris, a->object, a->n, a->num_chunks);
    return hipGetLastError();
}

#endif
