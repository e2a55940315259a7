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

/* ---- the fast queries (include/rt_amd.h, rt_winding.h) -----------------------------------------------------------------------------
 * rt_winding_fast_kernel: one point per lane, whole chunks of 64 from the same counter, and rt_wn_mesh_fast's stackless walk per lane: a lane
 * is either at a cluster or at one triangle of a leaf, and a loop step serves both kinds, so a lane in a leaf costs the others one term per
 * step and not eight.  Which clusters a lane visits depends on its point: the tree, the moments and the gathered records are read per lane
 * from global memory (48 bytes a step either way, from tables of a few hundred KB that stay in the caches).  No LDS, no stack, nothing
 * spilled.  Objects that are no meshes run rt_wn_object's wave-uniform loops as in the exact kernel.  Chunks are taken whole and not
 * refilled lane by lane: a walk is a few dozen steps, and a wave waits for its longest lane - see DESIGN.md section 28.
 *
 * The refit: rt_winding_gather_kernel (one thread per record of a mesh), rt_winding_leaves_kernel (one thread per leaf), and
 * rt_winding_combine_kernel once per height of the tree, bottom-up, one thread per cluster of that height.  Launches on one stream are the
 * only ordering: no kernel waits for another workgroup. */
#define RT_WINDING_REFIT_THREADS 256

__global__ __launch_bounds__(RT_WINDING_THREADS) void rt_winding_fast_kernel(const v4f *__restrict__ tris, const v4f *__restrict__ objtab,
                                                                             const int32_t *__restrict__ perm, const uint32_t *__restrict__ flip,
                                                                             const v4f *__restrict__ topo, const v4f *__restrict__ moments,
                                                                             const v4f *__restrict__ rec, const int32_t *__restrict__ object_range,
                                                                             const float *__restrict__ points, const rt_nearest *__restrict__ nearest,
                                                                             uint32_t *__restrict__ counter, float *__restrict__ winding,
                                                                             uint8_t *__restrict__ inside, float *__restrict__ sdf, int32_t num_objects,
                                                                             int32_t num_tris, int32_t object, float beta2, uint32_t n, uint32_t num_chunks)
{
    const int lane = threadIdx.x & (RT_WAVE - 1);
    rt_wn_scene<v4f> S;
    S.tris = tris; S.objtab = objtab; S.perm = perm; S.flip = flip; S.num_objects = num_objects; S.num_tris = num_tris;
    rt_wn_fast<v4f> T;
    T.topo = topo; T.moments = moments; T.rec = rec; T.object_range = object_range; T.beta2 = beta2;
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(counter, 1u);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        if (c >= num_chunks) break;
        const uint32_t id = c * 64u + (uint32_t)lane;
        const bool live = id < n;
        float px = rt_wn_float(0x7FC00000u), py = 0.f, pz = 0.f;       /* (an idle lane of the last chunk: not finite, so it walks nothing) */
        if (live) {
            const float *q = points + 3 * (size_t)id;
            px = q[0]; py = q[1]; pz = q[2];
        }
        const float w = rt_wn_point_fast(S, T, object, px, py, pz);
        if (live) {
            if (winding) winding[id] = w;
            if (inside) inside[id] = rt_wn_inside(w) ? 1 : 0;
            if (sdf) sdf[id] = rt_wn_sdf(w, nearest[id].distance);
        }
    }
}

__global__ __launch_bounds__(RT_WINDING_REFIT_THREADS) void rt_winding_gather_kernel(const v4f *__restrict__ tris, const int32_t *__restrict__ perm,
                                                                                     const uint32_t *__restrict__ flip, const int32_t *__restrict__ inv,
                                                                                     v4f *__restrict__ rec, int32_t base, int32_t count)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WINDING_REFIT_THREADS + threadIdx.x);
    if (j >= count) return;
    rt_wn_scene<v4f> S;
    S.tris = tris; S.objtab = nullptr; S.perm = perm; S.flip = flip; S.num_objects = 0; S.num_tris = 0;
    rt_wn_gather(S, inv, rec, base, count, j);
}

__global__ __launch_bounds__(RT_WINDING_REFIT_THREADS) void rt_winding_leaves_kernel(const v4f *__restrict__ topo, const int32_t *__restrict__ levels,
                                                                                     const v4f *__restrict__ rec, v4f *__restrict__ sums,
                                                                                     v4f *__restrict__ moments, int32_t first, int32_t count)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WINDING_REFIT_THREADS + threadIdx.x);
    if (j >= count) return;
    const int32_t i = levels[first + j];
    const v4f t = topo[i];
    int32_t tris = (int32_t)rt_wn_bits(t.z);
    if (tris > RT_WINDING_LEAF_TRIS) tris = RT_WINDING_LEAF_TRIS;
    if (tris <= 0) return;
    v4f s[4], m[2];
    rt_wn_leaf_sums(rec, (int32_t)rt_wn_bits(t.y), tris, s);
    rt_wn_moments(s, m);
    for (int k = 0; k < 4; k++) sums[4 * (size_t)i + k] = s[k];
    moments[2 * (size_t)i] = m[0];
    moments[2 * (size_t)i + 1] = m[1];
}

__global__ __launch_bounds__(RT_WINDING_REFIT_THREADS) void rt_winding_combine_kernel(const v4f *__restrict__ topo, const int32_t *__restrict__ levels,
                                                                                      v4f *sums, v4f *__restrict__ moments, int32_t first, int32_t count)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WINDING_REFIT_THREADS + threadIdx.x);
    if (j >= count) return;
    const int32_t i = levels[first + j];
    const int32_t left = i + 1, right = (int32_t)rt_wn_bits(topo[left].x);
    v4f L[4], R[4], s[4], m[2];
    for (int k = 0; k < 4; k++) { L[k] = sums[4 * (size_t)left + k]; R[k] = sums[4 * (size_t)right + k]; }
    rt_wn_add_sums(L, R, s);
    rt_wn_moments(s, m);
    for (int k = 0; k < 4; k++) sums[4 * (size_t)i + k] = s[k];
    moments[2 * (size_t)i] = m[0];
    moments[2 * (size_t)i + 1] = m[1];
}

/* ---- launcher (rt_launch.h) ----------------------------------------------------------------- */
static hipError_t winding_refit_launch(const rt_winding_args *a, hipStream_t stream)
{
    const int32_t items = a->op == RT_WN_OP_GATHER ? a->mesh_count : a->range_count;
    if (items <= 0) return hipSuccess;
    const dim3 grid((uint32_t)((items + RT_WINDING_REFIT_THREADS - 1) / RT_WINDING_REFIT_THREADS)), block(RT_WINDING_REFIT_THREADS);
    if (a->op == RT_WN_OP_GATHER)
        hipLaunchKernelGGL(rt_winding_gather_kernel, grid, block, 0, stream, (const v4f *)a->blob + a->off_tris, a->perm, a->flip, a->inv, (v4f *)a->rec,
                           a->mesh_base, a->mesh_count);
    else if (a->op == RT_WN_OP_LEAVES)
        hipLaunchKernelGGL(rt_winding_leaves_kernel, grid, block, 0, stream, (const v4f *)a->topo, a->levels, (const v4f *)a->rec, (v4f *)a->sums,
                           (v4f *)a->moments, a->range_first, a->range_count);
    else
        hipLaunchKernelGGL(rt_winding_combine_kernel, grid, block, 0, stream, (const v4f *)a->topo, a->levels, (v4f *)a->sums, (v4f *)a->moments,
                           a->range_first, a->range_count);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_winding(const rt_winding_args *a, int num_cus, hipStream_t stream)
{
    if (a->op == RT_WN_OP_GATHER || a->op == RT_WN_OP_LEAVES || a->op == RT_WN_OP_COMBINE) return winding_refit_launch(a, stream);
    if (a->op != RT_WN_OP_EXACT && a->op != RT_WN_OP_FAST) return hipErrorInvalidValue;
    const uint32_t waves = RT_WINDING_THREADS / RT_WAVE;
    uint32_t blocks = (a->num_chunks + waves - 1) / waves;
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 1) * RT_WINDING_BLOCKS_PER_CU;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) return hipSuccess;
    if (a->op == RT_WN_OP_FAST)
        hipLaunchKernelGGL(rt_winding_fast_kernel, dim3(blocks), dim3(RT_WINDING_THREADS), 0, stream, (const v4f *)a->blob + a->off_tris,
                           (const v4f *)a->blob + a->off_objtab, a->perm, a->flip, (const v4f *)a->topo, (const v4f *)a->moments, (const v4f *)a->rec,
                           a->object_range, a->points, a->nearest, a->counter, a->winding, a->inside, a->sdf, a->num_objects, a->num_tris, a->object,
                           a->beta2, a->n, a->num_chunks);
    else
        hipLaunchKernelGGL(rt_winding_kernel, dim3(blocks), dim3(RT_WINDING_THREADS), 0, stream, (const v4f *)a->blob + a->off_tris,
                           (const v4f *)a->blob + a->off_objtab, a->perm, a->flip, a->points, a->nearest, a->counter, a->winding, a->inside, a->sdf,
                           a->num_objects, a->num_tris, a->object, a->n, a->num_chunks);
    return hipGetLastError();
}

#endif
