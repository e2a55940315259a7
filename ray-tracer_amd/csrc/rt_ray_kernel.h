/*
 * rt_ray_kernel.h — the launch path the ray kernels (rt_query_kernel.h: closest hit; rt_occlusion_kernel.h: any hit; rt_ao_kernel.h: the
 * ambient-occlusion plane; rt_nearest_kernel.h, rt_sweep_kernel.h, rt_multihit_kernel.h, rt_overlap_kernel.h and rt_tritri_kernel.h: the
 * queries on points, balls, rays, boxes and triangles - like the ambient-occlusion kernel, one front under both values of `front`) share: one launcher over the
 * kernel (the LDS opt-in, the occupancy cache, the grid sized from the ray count) and one table of its instantiations over RT_SHAPES.  The
 * grid: one wave per 64 rays up to the persistent grid (every CU filled), so a handful of rays stages the scene once, not once per CU.
 *
 * The kernels' device code (the hand-out of ray ids, the tile slots and primary rays of a view, the MESH and WORK sections) is still stated in
 * each kernel: moved into functions here, or with the two argument blocks on a common base, the register allocation of the mesh shapes changes
 * (DESIGN.md §11), and the kernels' budgets (tests/test_occlusion_abi.py) are kept.
 */
#ifndef RT_RAY_KERNEL_H
#define RT_RAY_KERNEL_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <array>
#include <iterator>
#include <utility>

#include "rt_device_scene.h"

/* One launch of KERNEL (a ray kernel built for workgroups of NT threads) over args->num_chunks chunks. */
template <auto KERNEL, int NT, class Args>
static hipError_t rt_ray_launch_one(const Args *args, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    const void *fn = (const void *)KERNEL;
    /* the LDS opt-in and the resident workgroups per CU, asked once per kernel, device and LDS size (a scene's calls repeat them): two runtime
     * calls less on the path of a one-ray query.  A failed probe counts as one workgroup per CU and must not surface as a launch error. */
    static thread_local struct { int device; size_t lds; int per_cu; } seen = {-1, 0, 0};
    int device = 0;
    (void)hipGetDevice(&device);
    if (seen.device != device || seen.lds != lds_bytes) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, NT, lds_bytes) != hipSuccess || per_cu < 1) { per_cu = 1; (void)hipGetLastError(); }
        seen = {device, lds_bytes, per_cu};
    }
    /* few rays: few workgroups (a wave per 64 rays); many: the persistent grid */
    const long long waves_per_block = NT / 64;
    const long long needed = ((long long)args->num_chunks + waves_per_block - 1) / waves_per_block;
    long long blocks = (long long)num_cus * seen.per_cu;
    if (blocks > needed) blocks = needed;
    if (blocks < 1) return hipSuccess;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(NT), lds_bytes, stream, *args);
    return hipGetLastError();
}

/* The ray kernels are built for every shape of RT_SHAPES, the render kernel's list, each with either front: a committed scene's shape
 * (rt_sched::choose_shape) fixes a placement, a workgroup size and an LDS size that fit the blob plus the [entries + 1][threads] traversal
 * stack, which is all a ray kernel needs too, so a scene that renders answers queries.  K names a kernel: K::args is its argument block,
 * K::kernel<threads, has_mesh, mode, front> its instantiations. */
template <class K, bool FRONT, size_t... I>
static constexpr std::array<hipError_t (*)(const typename K::args *, int, size_t, hipStream_t), sizeof...(I)> rt_ray_fns_of(std::index_sequence<I...>)
{
    return {{rt_ray_launch_one<K::template kernel<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode, FRONT>, RT_SHAPES[I].threads, typename K::args>...}};
}

template <class K>
static hipError_t rt_ray_launch(const typename K::args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream)
{
    static constexpr auto plain = rt_ray_fns_of<K, false>(std::make_index_sequence<std::size(RT_SHAPES)>());
    static constexpr auto fronted = rt_ray_fns_of<K, true>(std::make_index_sequence<std::size(RT_SHAPES)>());
    const int i = rt_shape_index(shape);
    if (i < 0) return hipErrorInvalidValue;
    return (front ? fronted[i] : plain[i])(args, num_cus, lds_bytes, stream);
}

#endif
