/*
 * rt_kernel.hip — the per-pixel hot path as a hand-written HIP kernel for gfx950 (MI355X).
 *
 * What it computes is the reference's get_pixel_colour (src/raytracer.cu:116-136) and
 * everything below it: camera ray (src/camera.cu:24-29, src/ray.cu:147-155), per-bounce
 * direction jitter (src/ray.cu:130-142), closest hit over the object list
 * (src/raytracer.cu:24-46) with sphere / Moller-Trumbore triangle / quad / one-way quad /
 * cuboid / BVH mesh tests (src/objects.cu), Lambertian-metal-emissive scattering
 * (src/ray.cu:67-75,157-186), the PCG stream (src/utils.cu:220-239) and the progressive
 * average (src/raytracer.cu:97-113).  The arithmetic (types, order, the double-precision
 * fragments) is the reference's; the program structure is not:
 *
 *  - every lane is a small state machine (fetch pixel -> generate bounce -> mesh traversal ->
 *    shade -> ...).  Lanes take pixels one by one (tile-major ids handed out per wave from a
 *    global tile counter), so no lane waits for the slowest pixel of a tile; the spp loop and
 *    the bounce loop are one flat sequence per lane, so no lane waits for the longest path of
 *    the wave (the RNG stream stays per-pixel-sequential, SURVEY.md §7 hard part 3);
 *  - BVH traversal is decoupled from the bounce loop: lanes that need it park in a wait state
 *    and the wave runs traversal steps only while enough lanes (a ballot count) are
 *    traversing; lanes whose ray missed every mesh box, or finished early, go on shading and
 *    generating instead of idling behind the longest traversal;
 *  - the whole scene (BVH nodes with child boxes inline, 48-byte triangles, per-object
 *    shading record, the object list) is staged into LDS once per workgroup; the object list is
 *    read with wave-uniform addresses (one broadcast per quad) because every lane walks it in
 *    the same order;
 *  - BVH traversal keeps the current node in a register and only the deferred sibling (with
 *    its entry distance) on a per-lane LDS stack laid out [entry][thread], which is
 *    bank-conflict-free; a box is tested once, not twice as in the reference, by carrying the
 *    entry distance instead of re-testing on pop (same predicate, same outcome);
 *  - RNG state, ray, throughput and accumulators live in registers;
 *  - one launch can render several consecutive progressive frames (rt_render_device_batch): a
 *    ticket is one tile of one frame, the host lays the tickets out longest job first over ALL
 *    frames (rt_capi.cpp build_job_order), so every frame's expensive tiles start at once and the
 *    cheap ones fill in behind them; every frame stores its per-pixel mean in a plane of its own and
 *    rt_blend_kernel (rt_frame_kernels.h) folds the planes into the frame buffer in frame order.
 *
 * One translation unit, one concern per header.  rt_vec.h: vector and short-form math; rt_intersect.h: the primitive tests; rt_surface.h:
 * the surface at a hit; rt_instrument.h: the development counters; rt_traverse.h: the lane modes and the traversal pieces every kernel
 * shares; rt_pixel.h: the render kernel's per-pixel sections; then a header per kernel family, each with its launchers.  Every header
 * includes what it uses (tests/test_headers_compile.py); the order below only fixes the order in which the kernels are emitted - the
 * non-template kernels as they are defined, the templates as their launchers ask for them: ray kernels, denoiser, render kernel.
 *
 * No MFMA: there is no dense contraction anywhere in this workload.
 * Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize (the reference's a*b+c
 * are two roundings: contraction would change hit/miss decisions; the SLP vectorizer's packed f32
 * pairs cost 40 % more registers and 10 % of the time).
 */
#include "rt_ray_kernels.h"        /* closest-hit, any-hit and ambient-occlusion ray kernels (not in the development builds) */
#include "rt_denoise_kernel.h"     /* the edge-avoiding a-trous denoiser: image-space passes, nothing of the traversal (in every build) */
#include "rt_adaptive_kernel.h"    /* the adaptive sampling loop's image-space passes: plan, combine */
#include "rt_frame_kernels.h"      /* blend, tile copy, RGBA8 */
#include "rt_debug_kernels.h"      /* the math headers evaluated on the device, for the tests */
#include "rt_render_kernel.h"      /* the render kernel and its shape table */
#include "rt_rebuild_kernel.h"     /* a committed mesh's BVH rebuilt from new vertices: nothing of the traversal either (last: the kernels before it are emitted as they were) */
#include "rt_cull_kernel.h"        /* the primary-ray cull's pre-pass: one bit per pixel of a view (behind everything else, for the same reason) */
#include "rt_sweep_kernel.h"      /* sphere-cast queries: where a moving ball first touches the scene (in every build; last, for the same reason) */
#include "rt_nearest_kernel.h"     /* nearest-surface queries: closest point and distance (in every build; last, for the same reason) */
#include "rt_overlap_kernel.h"     /* box-overlap queries: which surfaces touch a box (not in the development builds; last, for the same reason) */
#include "rt_tritri_kernel.h"      /* triangle-overlap queries: which surfaces a triangle cuts, and where (not in the development builds; last, for the same reason) */
#include "rt_multihit_kernel.h"    /* multi-hit ray queries: the first k hits of a ray, and hit counts (not in the development builds; last, for the same reason) */
#include "rt_winding_kernel.h"     /* winding-number queries: containment and the sign of a distance; a dense reduction, no traversal (in every build; last, for the same reason) */
