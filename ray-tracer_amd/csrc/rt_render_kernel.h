/*
 * rt_render_kernel.h — the render kernel: the wave loop over the per-pixel sections of rt_pixel.h and the traversal pieces of rt_traverse.h,
 * its instantiations over RT_SHAPES and the launchers (declared in rt_launch.h).  rt_kernel.hip has the overview.
 *
 * The kernel's prologue and its MESH, leaf and merge steps are stated here in place, although rt_traverse.h has them as functions
 * (rt_stage_scene, rt_mesh_enter, rt_leaf_tris, rt_mesh_merge) for the ray kernels: calling those here changes the register allocation or
 * the schedule of 3 to 13 of the 13 instantiations (rt_traverse.h).  rt_descend and rt_pop are shared.
 */
#ifndef RT_RENDER_KERNEL_H
#define RT_RENDER_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <iterator>
#include <type_traits>
#include <utility>

#include "rt_device_scene.h"
#include "rt_instrument.h"
#include "rt_intersect.h"
#include "rt_launch.h"
#include "rt_pixel.h"
#include "rt_traverse.h"
#include "rt_vec.h"

/* MODE (RT_SCENE_*): where the scene is read from.  RT_SCENE_LDS: the whole blob is staged into LDS.  For scenes larger
 * than a CU's LDS the same code reads the triangles (RT_SCENE_HYBRID: the BVH nodes and the object records still fit) or
 * every section (RT_SCENE_GLOBAL) from global memory - they stay L2 / Infinity-Cache resident.  (Requesting a leaf's next
 * triangle before testing the current one, and testing two at a time, were measured on the 6,000- and 50,880-triangle
 * scenes: no difference - the compiler keeps the tests sequential and four waves per SIMD already cover the L2 latency.) */
/* Occupancy.  Built with -fno-slp-vectorize the kernel needs ~90 VGPRs (the SLP vectorizer's packed-f32 pairs cost
 * 128 and ~10 % of the time).  The 1024-thread workgroup of a large mesh scene is one per CU = four waves per SIMD,
 * whatever the registers (its LDS holds the scene and 1024 traversal stacks); the smaller workgroups - scenes without a
 * mesh, and mesh scenes small enough for several workgroups per CU - are register-bound, so they are compiled for
 * five waves per SIMD (<= 96 VGPRs; the allocator then lands on 79-80, which lets six be resident).  The launcher
 * asks the runtime how many workgroups of the chosen shape fit a CU (rt_kernel_blocks_per_cu). */
/* The loop itself is rt_render_loop.inc, included once per kernel.  BUDGET there: the budget variant (rt_budget_kernel below; `a` is an
 * rt_budget_args, handed to the sections as its base).  The wave loop is the same; what differs is in rt_pixel.h: px_fetch loads the pixel's budget n (0: the lane stays in M_FETCH), the end-of-sample test counts down from it, and
 * px_finish_budget divides by it and folds the mean into the frame by sample counts.  Progress with budgets of zero: see the FETCH step. */
template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, NT == 1024 ? 4 : (HAS_MESH ? RT_SMALL_WG_WAVES : RT_SMALL_WG_WAVES + 1)) void rt_render_kernel(const rt_kernel_args a)
#define RT_LOOP_BUDGET false
#define RT_LOOP_VIEWS false
#define RT_LOOP_SKY false
#define RT_LOOP_TRAITS 0
#define RT_LOOP_CULL rt_loop_culls(HAS_MESH, MODE, NT, RT_VARIANT_GENERIC)
#include "rt_render_loop.inc"
#undef RT_LOOP_CULL
#undef RT_LOOP_TRAITS
#undef RT_LOOP_SKY
#undef RT_LOOP_VIEWS
#undef RT_LOOP_BUDGET

/* The traits variant: the render kernel for a scene whose commit has fixed what the generic kernel decides again per lane, ray and hit
 * (RT_TRAIT_*, rt_device_scene.h): the same loop text with the traits of the shape's class switched on
 * (rt_variant_traits; instantiated for the shapes that have any), the same launch bounds, the same frames bit for bit.  Stated in the kernel like rt_render_kernel's, not as a function.  A name of its own, so that every kernel there was
 * keeps its symbol and its code (tools/compare_kernels.py). */
template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, NT == 1024 ? 4 : (HAS_MESH ? RT_SMALL_WG_WAVES : RT_SMALL_WG_WAVES + 1)) void rt_traits_kernel(const rt_traits_args a)
#define RT_LOOP_BUDGET false
#define RT_LOOP_VIEWS false
#define RT_LOOP_SKY false
#define RT_LOOP_TRAITS rt_variant_traits(HAS_MESH, MODE, NT)
#define RT_LOOP_CULL rt_loop_culls(HAS_MESH, MODE, NT, RT_VARIANT_TRAITS_KERNEL)
#include "rt_render_loop.inc"
#undef RT_LOOP_CULL
#undef RT_LOOP_TRAITS
#undef RT_LOOP_SKY
#undef RT_LOOP_VIEWS
#undef RT_LOOP_BUDGET

/* px_fetch under CULL reads rt_kernel_args::cull_lo / cull_hi at their offsets in the kernel's argument segment (rt_pixel.h): the block has to
 * start that segment.  Only rt_traits_kernel is compiled with CULL (rt_loop_culls is false for RT_VARIANT_GENERIC): its one parameter is an
 * rt_traits_args, whose first - and only - base is the block, in front of the members it adds. */
static_assert(!rt_loop_culls(1, RT_SCENE_LDS, 1024, RT_VARIANT_GENERIC), "rt_render_kernel is not compiled with CULL: its loop has no form of the cull");
static_assert(std::is_same<decltype(&rt_traits_kernel<1024, true, RT_SCENE_LDS>), void (*)(rt_traits_args)>::value,
              "the block is rt_traits_kernel's only parameter: px_fetch reads the cull plane's address at the block's offsets in the argument segment");
static_assert(std::is_base_of<rt_kernel_args, rt_traits_args>::value && !std::is_polymorphic<rt_traits_args>::value && std::is_standard_layout<rt_kernel_args>::value &&
                  sizeof(rt_traits_args) == sizeof(rt_kernel_args) + 8,
              "rt_traits_args is the block and, behind it, mesh_obj and its padding: nothing virtual, no second base in front of the block");

/* The budget variant: per-pixel sample counts (rt_render_budget_device), same shapes and launch bounds.  Its loop is a function taking the
 * argument block by reference: stated in the kernel like the render kernel's, the same text is allocated 101-113 registers in the
 * 1024-thread shapes and spills 12-49 registers in the smaller ones; as a function it takes 79-91 and spills none - as long as the sections see the block
 * through the base-class reference (profiles/r09/experiments/budget_loop_forms.txt: four forms, their figures). */
template <int NT, bool HAS_MESH, int MODE>
__device__ __forceinline__ void rt_budget_loop(const rt_budget_args &a)
#define RT_LOOP_BUDGET true
#define RT_LOOP_VIEWS false
#define RT_LOOP_SKY false
#define RT_LOOP_TRAITS 0
#define RT_LOOP_CULL false
#include "rt_render_loop.inc"
#undef RT_LOOP_CULL
#undef RT_LOOP_TRAITS
#undef RT_LOOP_SKY
#undef RT_LOOP_VIEWS
#undef RT_LOOP_BUDGET

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, NT == 1024 ? 4 : (HAS_MESH ? RT_SMALL_WG_WAVES : RT_SMALL_WG_WAVES + 1)) void rt_budget_kernel(const rt_budget_args a)
{
    rt_budget_loop<NT, HAS_MESH, MODE>(a);
}

/* The views variant: a camera per frame of the launch (rt_render_views_device), same shapes and launch bounds.  The wave loop is the
 * same; what differs is in rt_pixel.h: px_fetch takes the pixel's camera from rt_views_args::cams by the frame of its chunk, the end of a
 * sample restarts from that camera's position (read again from the table), and px_finish_pixel only stores the mean into the view's
 * plane.  A function taking the block by reference, like the budget loop and for its reason (DESIGN.md §17 has the registers per shape). */
template <int NT, bool HAS_MESH, int MODE>
__device__ __forceinline__ void rt_views_loop(const rt_views_args &a)
#define RT_LOOP_BUDGET false
#define RT_LOOP_VIEWS true
#define RT_LOOP_SKY false
#define RT_LOOP_TRAITS 0
#define RT_LOOP_CULL false
#include "rt_render_loop.inc"
#undef RT_LOOP_CULL
#undef RT_LOOP_TRAITS
#undef RT_LOOP_SKY
#undef RT_LOOP_VIEWS
#undef RT_LOOP_BUDGET

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, NT == 1024 ? 4 : (HAS_MESH ? RT_SMALL_WG_WAVES : RT_SMALL_WG_WAVES + 1)) void rt_views_kernel(const rt_views_args a)
{
    rt_views_loop<NT, HAS_MESH, MODE>(a);
}

/* The sky variant: the views variant whose rays that leave the scene look their light up in a cube map (rt_render_sky_device, rt_sky.h), same
 * shapes and launch bounds.  What differs is px_shade_miss under SKY (rt_pixel.h); the loop is a function taking the block by reference like
 * the other variants' (DESIGN.md section 22 has the registers per shape). */
template <int NT, bool HAS_MESH, int MODE>
__device__ __forceinline__ void rt_sky_loop(const rt_sky_args &a)
#define RT_LOOP_BUDGET false
#define RT_LOOP_VIEWS true
#define RT_LOOP_SKY true
#define RT_LOOP_TRAITS 0
#define RT_LOOP_CULL false
#include "rt_render_loop.inc"
#undef RT_LOOP_CULL
#undef RT_LOOP_TRAITS
#undef RT_LOOP_SKY
#undef RT_LOOP_VIEWS
#undef RT_LOOP_BUDGET

template <int NT, bool HAS_MESH, int MODE>
__global__ __launch_bounds__(NT, NT == 1024 ? 4 : (HAS_MESH ? RT_SMALL_WG_WAVES : RT_SMALL_WG_WAVES + 1)) void rt_sky_kernel(const rt_sky_args a)
{
    rt_sky_loop<NT, HAS_MESH, MODE>(a);
}

/* ---- launchers (rt_launch.h) ------------------------------------------------------------------------------------------- */
template <int NT, class Args, void (*KERNEL)(Args)>
static int rt_blocks_one(size_t lds_bytes)
{
    int n = 0;
    (void)hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)KERNEL, NT, lds_bytes) != hipSuccess) n = 0;
    return n;
}

/* one launch of KERNEL (rt_render_kernel, rt_budget_kernel, rt_views_kernel or rt_sky_kernel of one shape) with its argument block */
template <int NT, class Args, void (*KERNEL)(Args)>
static void rt_launch_one(const Args *args, int blocks, size_t lds_bytes, hipStream_t stream)
{
    (void)hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(NT), lds_bytes, stream, *args);
}

/* rt_traits_kernel's probe and launcher of a shape, or null where the shape has no traits kernel (and none is instantiated) */
template <int NT, bool HAS_MESH, int MODE, bool BUILT = rt_variant_traits(HAS_MESH, MODE, NT) != 0>
struct rt_traits_fns {
    static constexpr int (*blocks)(size_t) = rt_blocks_one<NT, rt_traits_args, rt_traits_kernel<NT, HAS_MESH, MODE>>;
    static constexpr void (*launch)(const rt_traits_args *, int, size_t, hipStream_t) = rt_launch_one<NT, rt_traits_args, rt_traits_kernel<NT, HAS_MESH, MODE>>;
};
template <int NT, bool HAS_MESH, int MODE>
struct rt_traits_fns<NT, HAS_MESH, MODE, false> {
    static constexpr int (*blocks)(size_t) = nullptr;
    static constexpr void (*launch)(const rt_traits_args *, int, size_t, hipStream_t) = nullptr;
};

/* the occupancy probe and the launcher of every built shape, in RT_SHAPES' order: the kernel is instantiated from that list alone */
struct rt_shape_fns {
    int (*blocks)(size_t lds_bytes);
    void (*launch)(const rt_kernel_args *args, int blocks, size_t lds_bytes, hipStream_t stream);
    int (*blocks_traits)(size_t lds_bytes);
    void (*launch_traits)(const rt_traits_args *args, int blocks, size_t lds_bytes, hipStream_t stream);
    void (*launch_budget)(const rt_budget_args *args, int blocks, size_t lds_bytes, hipStream_t stream);
    void (*launch_views)(const rt_views_args *args, int blocks, size_t lds_bytes, hipStream_t stream);
    void (*launch_sky)(const rt_sky_args *args, int blocks, size_t lds_bytes, hipStream_t stream);
};
template <size_t... I> static constexpr std::array<rt_shape_fns, sizeof...(I)> rt_shape_fns_of(std::index_sequence<I...>)
{
    return {{{rt_blocks_one<RT_SHAPES[I].threads, rt_kernel_args, rt_render_kernel<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>>,
              rt_launch_one<RT_SHAPES[I].threads, rt_kernel_args, rt_render_kernel<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>>,
              rt_traits_fns<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>::blocks,
              rt_traits_fns<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>::launch,
              rt_launch_one<RT_SHAPES[I].threads, rt_budget_args, rt_budget_kernel<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>>,
              rt_launch_one<RT_SHAPES[I].threads, rt_views_args, rt_views_kernel<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>>,
              rt_launch_one<RT_SHAPES[I].threads, rt_sky_args, rt_sky_kernel<RT_SHAPES[I].threads, RT_SHAPES[I].has_mesh != 0, RT_SHAPES[I].mode>>}...}};
}
static constexpr auto rt_shape_table = rt_shape_fns_of(std::make_index_sequence<std::size(RT_SHAPES)>());

/* workgroups of this shape of rt_render_kernel (shape.variant: of rt_traits_kernel) that are resident on one CU (registers, LDS, wave
 * slots), as the runtime reports it; 0 if the shape is not built */
extern "C" int rt_kernel_blocks_per_cu(rt_shape shape, size_t lds_bytes)
{
    const int i = rt_shape_index(shape);
    if (i < 0) return 0;
    return shape.variant == RT_VARIANT_TRAITS_KERNEL && rt_shape_table[i].blocks_traits ? rt_shape_table[i].blocks_traits(lds_bytes) : rt_shape_table[i].blocks(lds_bytes);
}

extern "C" hipError_t rt_launch_render(const rt_kernel_args *args, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream)
{
    const int i = rt_shape_index(shape);
    if (i < 0) return hipErrorInvalidValue;
    if (shape.variant == RT_VARIANT_TRAITS_KERNEL) {
        /* the scene has the traits and the shape a traits kernel (rt_sched::choose_variant decided at commit): every caller of this launcher
         * gets it through the shape it hands over.  A missing kernel is an error, not a reason to run the other one */
        if (!rt_shape_table[i].launch_traits) return hipErrorInvalidValue;
        rt_traits_args t;
        static_cast<rt_kernel_args &>(t) = *args;
        t.mesh_obj = shape.mesh_obj;
        rt_shape_table[i].launch_traits(&t, blocks, lds_bytes, stream);
        return hipGetLastError();
    }
    rt_shape_table[i].launch(args, blocks, lds_bytes, stream);
    return hipGetLastError();
}

/* the budget variant on the same shape; the caller sizes the grid as for the render kernel (the two have the same launch bounds and LDS) */
extern "C" hipError_t rt_launch_budget(const rt_kernel_args *args, const uint16_t *budget, uint32_t *count, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream)
{
    const int i = rt_shape_index(shape);
    if (i < 0) return hipErrorInvalidValue;
    rt_budget_args b;
    static_cast<rt_kernel_args &>(b) = *args;
    b.budget = budget;
    b.count = count;
    rt_shape_table[i].launch_budget(&b, blocks, lds_bytes, stream);
    return hipGetLastError();
}

/* the views variant on the same shape: cams is the device table of args->num_frames x 12 camera floats; the grid is sized as for the
 * render kernel */
extern "C" hipError_t rt_launch_views(const rt_kernel_args *args, const float *cams, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream)
{
    const int i = rt_shape_index(shape);
    if (i < 0) return hipErrorInvalidValue;
    rt_views_args v;
    static_cast<rt_kernel_args &>(v) = *args;
    v.cams = cams;
    rt_shape_table[i].launch_views(&v, blocks, lds_bytes, stream);
    return hipGetLastError();
}

/* the sky variant on the same shape (rt_launch.h): the views launch and the cube map's texels */
extern "C" hipError_t rt_launch_sky(const rt_kernel_args *args, const float *cams, const float *texels, int32_t face_size, rt_shape shape, int blocks, size_t lds_bytes,
                                    hipStream_t stream)
{
    const int i = rt_shape_index(shape);
    if (i < 0) return hipErrorInvalidValue;
    rt_sky_args s;
    static_cast<rt_kernel_args &>(s) = *args;
    s.cams = cams;
    s.sky_texels = texels;
    s.sky_n = face_size;
    rt_shape_table[i].launch_sky(&s, blocks, lds_bytes, stream);
    return hipGetLastError();
}

#endif
