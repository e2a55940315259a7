/*
 * rt_pixel.h — the render kernel's own per-pixel code (rt_render_kernel.h): the lane's pixel state (Px), the frame constants, the tile
 * hand-out, and the three per-pixel sections of the lane state machine (SHADE, FETCH, GEN).
 *
 * The arithmetic (types, order, the double-precision fragments) is the reference's; file:line
 * citations are on each piece.  -ffp-contract=off is assumed (see rt_kernel.hip).
 */
#ifndef RT_PIXEL_H
#define RT_PIXEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cull.h"
#include "rt_entry.h"
#include "rt_device_scene.h"
#include "rt_instrument.h"
#include "rt_intersect.h"
#include "rt_math.h"
#include "rt_rng.h"
#include "rt_sky.h"
#include "rt_traverse.h"
#include "rt_vec.h"

/* s_waitcnt vmcnt(0), expcnt and lgkmcnt at their maxima, as gfx9 encodes it (vmcnt in bits 3..0 and 15..14, expcnt in 6..4, lgkmcnt in
 * 11..8): right for gfx950 and the rest of the family, and wrong for gfx10 and later, whose fields lie elsewhere */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "RT_WAIT_VMCNT0 is the gfx9 encoding of s_waitcnt: give this target its own"
#endif
#define RT_WAIT_VMCNT0 0x0f70
#define PX_SUBTABLE 0x40000000u       /* ... and: the pixel has a sub-entry table (rt_entry.h), and the loop's gate-word register holds its slot word instead */
#define PX_NOCULL 0x80000000u         /* Px::id in the kernels that read the cull plane (rt_loop_culls): the pixel is NOT flagged by it */

/* per-lane pixel state (registers) */
struct Px {
    int mode;
    uint32_t rng;
    V3 colour, fin, thr, o, d, inv, primary;
    int sample, bounce;
    unsigned id;                 /* the pixel: 64 * (tile of this launch) + (row in tile * 8 + column in tile) */
    float cur_n;                 /* Ray::current_refractive_index src/ray.cu:56,144 */
    float best_t;
    int best_obj, best_prim, next_mesh;
    /* bits RT_FRAME_BITS-1..0: which frame of a multi-frame launch this pixel belongs to; bits 30..RT_FRAME_BITS: what it has
     * cost so far (RT_COST_* units), reported per tile when the launch collects costs (tile_cost); bit 31: one of its rays
     * has entered a mesh */
    unsigned frame_steps;
#ifdef RT_COSTMAP
    /* development build (tools/costmap.py): the frame holds, per pixel, (own traversal steps,
     * start tick, end tick) of the 100 MHz wall clock instead of the colour */
    unsigned c_steps, c_t0, c_wsteps;
#endif
};

/* wave-uniform frame constants */
struct Frame {
    V3 cam_pos, tl, du, dv, sky;
    int W, H, spp, limit, tiles_per_band;
};

/* The argument block of the budget variant of the render kernel (rt_budget_kernel, rt_render_kernel.h; rt_render_budget_device in
 * include/rt_amd.h): the render kernel's, and per pixel of the full frame how many samples it takes now and how many its value in `out`
 * already holds.  The sections below are handed the base and, where BUDGET is set, read the rest through px_budget. */
struct rt_budget_args : rt_kernel_args {
    const uint16_t *budget;      /* W*H: this launch's samples per pixel; 0: the pixel is neither read nor written */
    uint32_t *count;             /* W*H, or NULL (every pixel starts from nothing and no count is kept) */
};
/* (only under BUDGET, and the one user with BUDGET set is rt_budget_loop, whose parameter is an rt_budget_args: the render kernel's plain
 * block never gets here.  Carrying that in the sections' parameter type costs the budget kernels their registers:
 * profiles/r09/experiments/budget_loop_forms.txt) */
__device__ __forceinline__ const rt_budget_args &px_budget(const rt_kernel_args &a) { return static_cast<const rt_budget_args &>(a); }

/* The argument block of the views variant of the render kernel (rt_views_kernel, rt_render_kernel.h; rt_render_views_device in
 * include/rt_amd.h): the render kernel's, and one camera per frame of the launch.  `cam` of the base is not read: a lane takes the twelve
 * floats of its frame's camera from the table (the index differs across the lanes of a wave, which refill from different chunks, so the
 * table cannot be a kernel-argument array).  Only under VIEWS, and only rt_views_loop sets it: see px_budget. */
struct rt_views_args : rt_kernel_args {
    const float *cams;           /* num_frames x 12: cam_pos, tl_pixel_pos, delta_u, delta_v of frame k at cams + 12 * k */
};
__device__ __forceinline__ const rt_views_args &px_views(const rt_kernel_args &a) { return static_cast<const rt_views_args &>(a); }

/* The argument block of the sky variant (rt_sky_kernel, rt_render_kernel.h; rt_render_sky_device in include/rt_amd.h): the views variant's,
 * and the cube map a ray that leaves the scene looks its light up in (rt_sky.h).  Only under SKY, and only rt_sky_loop sets it: see
 * px_budget. */
struct rt_sky_args : rt_views_args {
    const float *sky_texels;     /* 6 x sky_n x sky_n texels of RT_SKY_TEXEL_FLOATS floats: faces +X, -X, +Y, -Y, +Z, -Z, rows, columns */
    int32_t sky_n;               /* texels on a face's side, 1 .. RT_SKY_MAX_FACE */
};
__device__ __forceinline__ const rt_sky_args &px_sky(const rt_kernel_args &a) { return static_cast<const rt_sky_args &>(a); }

/* The argument block of the traits variant (rt_traits_kernel, rt_render_kernel.h): the render kernel's, and the one mesh's place in the object
 * list, which rt_render_kernel reads from the mesh table in LDS whenever a traversal ends.  Only under RT_TRAIT_ONE_MESH, and only
 * rt_traits_kernel sets it: see px_budget. */
struct rt_traits_args : rt_kernel_args {
    int32_t mesh_obj;            /* -1: the scene has no mesh */
};
__device__ __forceinline__ const rt_traits_args &px_traits(const rt_kernel_args &a) { return static_cast<const rt_traits_args &>(a); }

/* wave-uniform pixel chunk: linear pixel ids [next, end) of one 8x8 tile */
struct Chunk {
    uint32_t next, end;
    int frame;                   /* the frame (of a multi-frame launch) the ids belong to */
    bool exhausted;
};

__device__ __forceinline__ void px_init(Px &p)
{
    const V3 z = v3(0.f, 0.f, 0.f);
    p.mode = M_FETCH; p.rng = 0;
    p.colour = z; p.fin = z; p.thr = z; p.o = z; p.d = z; p.inv = z; p.primary = z;
    p.sample = 0; p.bounce = 0; p.id = 0;
    p.cur_n = 1.0f; p.best_t = RT_INF_F;
    p.best_obj = -1; p.best_prim = -1; p.next_mesh = 0; p.frame_steps = 0;
    RT_COST(p.c_steps = 0; p.c_t0 = 0; p.c_wsteps = 0);
}

__device__ __forceinline__ void frame_init(Frame &f, const rt_kernel_args &a)
{
    f.cam_pos = v3(a.cam[0], a.cam[1], a.cam[2]);
    f.tl = v3(a.cam[3], a.cam[4], a.cam[5]);
    f.du = v3(a.cam[6], a.cam[7], a.cam[8]);
    f.dv = v3(a.cam[9], a.cam[10], a.cam[11]);
    f.sky = v3(a.sky[0], a.sky[1], a.sky[2]);
    f.W = a.width; f.H = a.height;
    f.spp = a.rays_per_pixel; f.limit = a.reflection_limit;
    f.tiles_per_band = a.tiles_x * (a.band_rows >> 3);
}

/* tile t of this launch -> its place in the image (tx, ty in tiles) and, for the compact band layout, the row of
 * the output buffer its first pixel row goes to */
__device__ __forceinline__ void tile_place(const rt_kernel_args &a, const Frame &f, int t, int &tx, int &ty, int &compact_row)
{
    if (a.tile_list) {
        const int g = (int)a.tile_list[t];
        ty = g / a.tiles_x; tx = g - ty * a.tiles_x;
        compact_row = 0;
    } else {
        const int band_local = t / f.tiles_per_band;
        const int in_band = t - band_local * f.tiles_per_band;
        const int tyb = in_band / a.tiles_x;
        tx = in_band - tyb * a.tiles_x;
        ty = (a.band_first + band_local * a.band_stride) * (a.band_rows >> 3) + tyb;
        compact_row = band_local * a.band_rows + tyb * 8;
    }
}

/* BUDGET: a pixel's n samples are done (n is read again here rather than kept in a register across the pixel: p.sample counts DOWN from
 * it, so the lane state is the render kernel's).  With m = the samples its value in the frame already holds, the frame becomes the mean
 * over all n + m: c if m == 0 (the frame is not read), else (c * n + frame * m) / (n + m), every operation rounded once; the count
 * becomes m + n.  Always a full frame (rt_render_budget_device refuses compact layouts). */
__device__ __forceinline__ void px_finish_budget(Px &p, const rt_kernel_args &a, const Frame &f)
{
    const rt_budget_args &b = px_budget(a);
    const int tile = (int)(p.id >> 6), within = (int)(p.id & 63u);
    int tx, ty, compact_row;
    tile_place(a, f, tile, tx, ty, compact_row);
    const int px = tx * 8 + (within & 7), py = ty * 8 + (within >> 3);
    const size_t pixel = (size_t)py * (size_t)f.W + (size_t)px;
    const uint32_t n = b.budget[pixel];
    const uint32_t m = b.count ? b.count[pixel] : 0u;
    const float fn = (float)n;
    V3 res = p.colour / fn;
    float *dst = a.out + pixel * 3;
    if (m != 0u) {
        const V3 previous = v3(dst[0], dst[1], dst[2]);
        res = (res * fn + previous * (float)m) / (float)(n + m);
    }
    dst[0] = rt_canon_nan(res.x); dst[1] = rt_canon_nan(res.y); dst[2] = rt_canon_nan(res.z);
    if (b.count) b.count[pixel] = m + n;
    p.mode = M_FETCH;
}

/* A pixel's samples are done: blend with the previous frame and store (src/raytracer.cu:107-112,
 * :133-135).
 *
 * Multi-frame launches (rt_kernel_args.partial != NULL) render consecutive progressive frames of one
 * view in ONE launch: every frame has its own seed, so frame k+1 of a pixel can be traced while
 * frame k of the same pixel is still being traced by another wave - the only thing that is
 * sequential is the blend, (c + prev * n) / (n + 1) with prev = the pixel's value after frame k.
 * So each frame only stores c, the mean of its own samples, into its plane of a scratch buffer
 * (plain stores, no ordering between frames needed), and a small kernel launched behind this one
 * (rt_blend_kernel) folds the planes into the frame buffer in frame order; NaN pixels are made the one
 * canonical quiet NaN there (any NaN plane value makes the blended value a NaN). */
/* CULL (rt_loop_culls): bit 31 of p.id is not part of the pixel's id (px_fetch keeps the pixel's cull bit there) */
template <bool BUDGET = false, bool VIEWS = false, bool CULL = false>
__device__ __forceinline__ void px_finish_pixel(Px &p, const rt_kernel_args &a, const Frame &f)
{
    if (BUDGET) { px_finish_budget(p, a, f); return; }
    if (VIEWS) {
        /* a views launch renders whole images into one plane per view and collects no costs: the mean goes to the pixel's place in its
         * view's plane, and what becomes of the planes (the fold, or the frame-0 arithmetic of separate frames) runs behind the kernel */
        const V3 c = p.colour / (float)f.spp;
        const int tile = (int)(p.id >> 6), within = (int)(p.id & 63u);
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int px = tx * 8 + (within & 7), py = ty * 8 + (within >> 3);
        const size_t pixel = (size_t)py * (size_t)f.W + (size_t)px;
        float *dst = a.partial + ((size_t)(p.frame_steps & (unsigned)(RT_MAX_BATCH_FRAMES - 1)) * a.partial_plane + pixel) * 3;
        dst[0] = c.x; dst[1] = c.y; dst[2] = c.z;
        p.mode = M_FETCH;
        return;
    }
    const V3 c = p.colour / (float)f.spp;
    const unsigned id = CULL ? p.id & ~(PX_NOCULL | PX_SUBTABLE) : p.id;
    const int tile = (int)(id >> 6), within = (int)(id & 63u);
    int tx, ty, compact_row;
    tile_place(a, f, tile, tx, ty, compact_row);
    const int px = tx * 8 + (within & 7), py = ty * 8 + (within >> 3);
    size_t pixel = (size_t)py * (size_t)f.W + (size_t)px;
    if (a.compact) pixel = a.tile_list ? (size_t)id : (size_t)(compact_row + (within >> 3)) * (size_t)f.W + (size_t)px;
    /* (first launch of a view) what this pixel cost, charged to its tile */
    if (a.tile_cost && (p.frame_steps & (unsigned)(RT_MAX_BATCH_FRAMES - 1)) == 0u) {
        /* (frame 0 of the launch only: the figures describe the view, not the launch, and a 32-frame sum could wrap)
         * cost units in bits 31..1 of the tile's sum; bit 0: some pixel of the tile traversed a mesh (those tiles are
         * the long jobs the schedule puts first, rt_capi.cpp build_job_order) */
        unsigned units = (p.frame_steps & 0x7fffffffu) >> RT_FRAME_BITS;
        units = units > RT_COST_PIXEL_CAP ? RT_COST_PIXEL_CAP : units;
        atomicAdd(a.tile_cost + tile, units << 1);
        /* ... and the tile's most expensive pixel: a tile-frame is one job, as long as its longest pixel (a pixel's samples
         * are one sequential stream), and the schedule starts the longest jobs first */
        atomicMax(a.tile_peak + tile, units);
        if (p.frame_steps >> 31) atomicOr(a.tile_cost + tile, 1u);
    }
    p.mode = M_FETCH;
    if (a.partial) {
        float *dst = a.partial + ((size_t)(p.frame_steps & (unsigned)(RT_MAX_BATCH_FRAMES - 1)) * a.partial_plane + pixel) * 3;
        dst[0] = c.x; dst[1] = c.y; dst[2] = c.z;
        return;
    }
    float *dst = a.out + pixel * 3;
    const int array_index = (py * f.W + px) * 3;
    V3 previous = v3(0.f, 0.f, 0.f);
    if (a.prev) previous = v3(a.prev[array_index], a.prev[array_index + 1], a.prev[array_index + 2]);
    V3 previous_sum = previous * (float)a.frame_num;
    V3 res = (c + previous_sum) / (float)(a.frame_num + 1);
#ifdef RT_COSTMAP
    res = v3(__uint_as_float(RT_COSTMAP == 2 ? p.c_wsteps : p.c_steps), __uint_as_float(p.c_t0), __uint_as_float((unsigned)wall_clock64()));
#endif
    dst[0] = rt_canon_nan(res.x); dst[1] = rt_canon_nan(res.y); dst[2] = rt_canon_nan(res.z);
}

/* the end of a sample (src/raytracer.cu:102-105): add it to the pixel, restart from a copy of the
 * primary ray; after the last sample the pixel is finished */
template <bool BUDGET = false, bool VIEWS = false, bool CULL = false>
__device__ __forceinline__ void px_end_sample(Px &p, const rt_kernel_args &a, const Frame &f)
{
    p.colour = p.colour + p.fin;
    if (VIEWS) {
        /* the render branch's restart below with the camera position of the pixel's own view, read again from the table by the frame index
         * in p.frame_steps rather than kept in three registers of Px (stated twice like the budget branch: a change goes into all copies) */
        p.sample++;
        p.fin = v3(0.f, 0.f, 0.f); p.thr = v3(1.f, 1.f, 1.f);
        const float *cam = px_views(a).cams + 12u * (p.frame_steps & (unsigned)(RT_MAX_BATCH_FRAMES - 1));
        p.o = v3(cam[0], cam[1], cam[2]); p.d = p.primary; p.bounce = 0; p.cur_n = 1.0f;
        if (p.sample >= f.spp) px_finish_pixel<false, true>(p, a, f);
        return;
    }
    if (BUDGET) {
        /* p.sample: the samples of the pixel's budget still to come.  (The restart lines are the render branch's below, stated twice so that
         * the render kernel's code stays byte for byte: a change to either copy goes into both.) */
        p.sample--;
        p.fin = v3(0.f, 0.f, 0.f); p.thr = v3(1.f, 1.f, 1.f);
        p.o = f.cam_pos; p.d = p.primary; p.bounce = 0; p.cur_n = 1.0f;
        if (p.sample <= 0) px_finish_pixel<true>(p, a, f);
        return;
    }
    p.sample++;
    p.fin = v3(0.f, 0.f, 0.f); p.thr = v3(1.f, 1.f, 1.f);
    p.o = f.cam_pos; p.d = p.primary; p.bounce = 0; p.cur_n = 1.0f;
    if (p.sample >= f.spp) px_finish_pixel<false, false, CULL>(p, a, f);
}

/* ================= SHADE, a ray that hit nothing (src/raytracer.cu:76-80): sky, end of sample == */
/* SKY: the sky is the texel of the cube map in the ray's direction (rt_sky_lookup: compares, two divisions, two conversions) times the
 * constant, which becomes the map's tint.  One load from global memory per sample, at an address that differs across the lanes; it is issued
 * at the end of a path, where nothing else of the lane is in flight, and the wave's other lanes wait for it with this one - the SIMD's other
 * waves cover it (DESIGN.md section 22 has what it costs).  The map is not staged into LDS: the scene's shape would change with it. */
template <bool BUDGET = false, bool VIEWS = false, bool SKY = false, bool CULL = false>
__device__ __forceinline__ void px_shade_miss(Px &p, const rt_kernel_args &a, const Frame &f)
{
    if (SKY) {
        const rt_sky_args &s = px_sky(a);
        const float *tx = s.sky_texels + (size_t)rt_sky_lookup(p.d.x, p.d.y, p.d.z, s.sky_n, nullptr, nullptr, nullptr) * RT_SKY_TEXEL_FLOATS;
#if RT_SKY_TEXEL_FLOATS == 4
        const v4f t = *(const v4f *)tx;
        const V3 light = v3(t.x, t.y, t.z) * f.sky;
#else
        const V3 light = v3(tx[0], tx[1], tx[2]) * f.sky;
#endif
        p.fin = p.fin + light * p.thr;
        p.mode = M_GEN;
        px_end_sample<BUDGET, VIEWS>(p, a, f);
        return;
    }
    p.fin = p.fin + f.sky * p.thr;
    p.mode = M_GEN;
    px_end_sample<BUDGET, VIEWS, CULL>(p, a, f);
}

/* ================= SHADE: the closest hit of this bounce is known (p.best_obj >= 0) ========= */
/* SHORT_DIVIDE: the logarithm's division in its short form (rt_math.h rt__div_benign; the same values): faster in every kernel but the
 * 1024-thread mesh kernel (three-sphere -4.2 %, cube -1.4 %, monkey +0.4 %), which keeps the division operator */
/* GENERAL_FUNCTIONS: Box-Muller through rt_logf / rt_cosf instead of their forms for a draw's arguments (again the same values): the hybrid
 * kernels (nodes in LDS, triangles from L2) are 2.8 % FASTER that way on the 6,000-triangle scene and indifferent on the 50,880-triangle one
 * (profiles/r04/experiments/box_muller_on_its_domain.txt) */
/* PLAIN (RT_TRAIT_PLAIN_MATERIALS; rt_traits_kernel alone): no material of the scene needs texture coordinates, refracts or carries a texture,
 * so the three regions that every hit would test for and skip are not compiled in; what is left is the same operations in the same order */
template <bool SHORT_DIVIDE, bool GENERAL_FUNCTIONS, bool BUDGET = false, bool VIEWS = false, bool PLAIN = false, bool CULL = false>
__device__ __forceinline__ void px_shade(Px &p, const rt_kernel_args &a, const Frame &f, const Lds &L)
{
    V3 &o = p.o, &d = p.d;
    {
        const int best_obj = p.best_obj, best_prim = p.best_prim;
        const v4f ma = L.objs[RT_OBJLDS_F4 * best_obj], mb = L.objs[RT_OBJLDS_F4 * best_obj + 1];
        const uint32_t packed = __float_as_uint(mb.w);
        const int mtype = (int)(packed & 3u);
        /* hit point and normal: Ray::get_pos src/ray.cu:63-65; Sphere :66; Triangle :158 */
        V3 P = d * p.best_t + o;
        V3 N;
        float tex_u = 0.f, tex_v = 0.f;
        if (packed & 32u) {
            const v4f sc = L.objs[RT_OBJLDS_F4 * best_obj + 2];
            N = normalised(P - v3(sc.x, sc.y, sc.z));
            if (!PLAIN && (packed & 16u)) {
                /* Sphere::assign_texture_coords src/objects.cu:82-97 (latitude / longitude) */
                const float PI = 3.141592653589793f;
                const float theta = rt_asinf((P.y - sc.y) / sc.w);
                const float phi = rt_acosf((P.x - sc.x) / sc.w);
                tex_u = (theta + PI / 2) / PI;
                const float v_ratio = (1 - phi / PI) / 2;
                const int behind = P.z > sc.z ? 1 : 0;
                const int mult = 1 - 2 * behind;
                tex_v = (float)(1 * behind) + (float)mult * v_ratio;
            }
        } else {
            const v4f q2 = L.tris[3 * best_prim + 2];
            V3 n = v3(q2.y, q2.z, q2.w);
            N = (dot(n, d) > 0.0f) ? neg(n) : n;
            if (!PLAIN && (packed & 16u)) {
                /* Triangle::assign_texture_coords src/objects.cu:160,196-199, called as (w,u,v) */
                float t, u, v;
                tri_test(L.tris, best_prim, o, d, t, u, v);
                float w = 1.0f - u - v;
                const float *uv = a.tri_uv + 6 * best_prim;
                tex_u = uv[0] * w + uv[2] * u + uv[4] * v;
                tex_v = uv[1] * w + uv[3] * u + uv[5] * v;
            }
        }
        /* update_ray src/raytracer.cu:49-64: REFRACTIVE goes through Ray::refract
         * (src/ray.cu:77-128, Snell + Schlick + total internal reflection), which falls
         * back to reflect(); everything else reflects */
        bool do_reflect = true;
        V3 refr_dir = v3(0.f, 0.f, 0.f);
        if (!PLAIN && mtype == RT_DEV_MAT_REFRACTIVE) {
            const float mat_n = L.objs[RT_OBJLDS_F4 * best_obj + 3].x;
            float n1, n2;
            V3 rn;
            if (dot(N, d) > 0.0f) { n1 = mat_n; n2 = p.cur_n; rn = N; }        /* leaving the object */
            else                  { n1 = p.cur_n; n2 = mat_n; rn = neg(N); }   /* entering */
            p.cur_n = n2;
            /* min(float, double) is CUDA's double overload; acos / asin of doubles */
            const float theta1 = (float)rt_acos(fmin((double)dot(d, rn), 1.0));
            const float theta2 = (float)rt_asin(fmin((double)(n1 * rt_sinf(theta1) / n2), 1.0));
            const float critical_angle = rt_asinf(n2 / n1);
            /* get_reflection_coeff :188-196: pow(float, int) is the double pow */
            const float sqrt_r0 = (n1 - n2) / (n1 + n2);
            const float r0 = sqrt_r0 * sqrt_r0;
            const float cos_theta = rt_cosf(theta1);
            const float reflection_coeff = (float)((double)r0 + (double)(1.0f - r0) * rt_pow5((double)(1.0f - cos_theta)));
            do_reflect = theta1 > critical_angle;
            if (!do_reflect) do_reflect = reflection_coeff > rt_u01(rt_pcg_next(&p.rng));   /* `||` short-circuits */
            if (!do_reflect) {
                V3 perp = v3(0.f, 0.f, 0.f);
                if (theta1 != 0.0f) perp = (d - rn * rt_cosf(theta1)) / rt_sinf(theta1);
                refr_dir = normalised(rn * rt_cosf(theta2) + perp * rt_sinf(theta2));
            }
        }
        if (do_reflect) {
            /* Ray::reflect src/ray.cu:67-75 with diffuse_reflect :157-170,
             * true_lambertian_reflect :172-178, perfect_reflect :180-186, lerp :32-34 */
            float gx = normal_num<SHORT_DIVIDE, GENERAL_FUNCTIONS>(p.rng);
            float gy = normal_num<SHORT_DIVIDE, GENERAL_FUNCTIONS>(p.rng);
            float gz = normal_num<SHORT_DIVIDE, GENERAL_FUNCTIONS>(p.rng);
            V3 rv = v3(gx, gy, gz);
            if (dot(rv, N) < 0.0f) rv = neg(rv);
            rv = normalised(rv);
            V3 diffuse_dir = normalised(N + rv);
            float dn = dot(d, N);
            V3 specular_dir = normalised(d - (N * 2.0f) * dn);
            d = normalised(diffuse_dir + (specular_dir - diffuse_dir) * ma.w);
        } else {
            d = refr_dir;
        }
        o = P;

        /* src/raytracer.cu:86-90 */
        if (mtype == RT_DEV_MAT_EMISSIVE) {
            p.fin = p.fin + v3(mb.x, mb.y, mb.z) * p.thr;
        } else {
            V3 tc;
            const int tex = (int)((packed >> 2) & 3u);
            if (PLAIN || tex == 0) {
                tc = v3(ma.x, ma.y, ma.z);
            } else if (tex == 1) {
                tc = v3(tex_u, tex_v, 0.f);                              /* gradient src/material.cu:80-82 */
            } else if (tex == 3) {
                /* image src/material.cu:119-124: nearest texel; an out-of-range index is clamped */
                const int iw = (int)__float_as_uint(ma.x), ih = (int)__float_as_uint(ma.y);
                const int uc = rt_f2i((float)(iw - 1) * tex_u), vc = rt_f2i((float)(ih - 1) * tex_v);
                int idx = (int)((uint32_t)vc * (uint32_t)iw + (uint32_t)uc);       /* wraps like the 32-bit machine arithmetic */
                idx = idx < 0 ? 0 : (idx > iw * ih - 1 ? iw * ih - 1 : idx);
                const float *tx = a.tex_data + (size_t)__float_as_uint(ma.z) + 3 * (size_t)idx;
                tc = v3(tx[0], tx[1], tx[2]);
            } else {
                const int nsq = (int)(packed >> 8);                      /* checkerboard :90-99 */
                const int uc = rt_f2i(tex_u * (float)nsq), vc = rt_f2i(tex_v * (float)nsq);
                tc = ((int)((uint32_t)uc + (uint32_t)vc) % 2 == 0) ? v3(ma.x, ma.y, ma.z) : v3(mb.x, mb.y, mb.z);
            }
            p.thr = p.thr * tc;
        }
        p.bounce++;
        p.frame_steps += (unsigned)(RT_COST_HIT * RT_MAX_BATCH_FRAMES);
    }
    p.mode = M_GEN;
    if (p.bounce >= f.limit) px_end_sample<BUDGET, VIEWS, CULL>(p, a, f);
}

/* ================= FETCH: lanes without a pixel take the next ones =========================
 * Linear pixel ids are tile-major (64 per 8x8 tile), tiles come from a global counter; a wave
 * asks for one tile at a time and hands its ids out to whichever lanes are free.  Must be called
 * by the whole wave.  Every call with a lane in M_FETCH either hands that lane a slot it has not been handed before or, once the tiles
 * are out, ends it (M_DONE): a lane that stays in M_FETCH (a slot outside the image; BUDGET: a pixel of budget 0) has used a slot up, so
 * calling again until no lane is in M_FETCH ends after at most (tiles * 64) slots, whatever the budgets are. */
/* CULL: the pixel's bit of the view's cull plane is read here, once per pixel and frame (a null plane, tested wave-uniformly: no bit), into
 * bit 31 of p.id, which no id reaches (at most 2^28 pixels: check_image_size) - PX_NOCULL is set unless the plane says that no primary ray
 * of this pixel reaches a leaf of any mesh.  A spare bit, not a member of Px: a member, even a dead one, changes the register numbering of
 * every kernel built from Px, and a register of its own held across the traversal loops changed their schedule (monkey +1.6 %).
 * CULL also loads the pixel's gate word (the subtree cull, rt_cull.h) into *px_gates, a register of the caller's loop.  Such a register is
 * what cost the bit 1.6 %; the word has no spare bits to go to, and it pays for itself: with it the kernel keeps its 97 VGPRs and the
 * descend loop its four waits, and the launch is 4 % shorter than the parent's ("The subtree cull"). */
template <bool BUDGET = false, bool VIEWS = false, bool CULL = false>
__device__ __forceinline__ void px_fetch(Px &p, Chunk &ch, const rt_kernel_args &a, const Frame &f, int lane, uint32_t *px_gates = nullptr)
{
    const bool want = p.mode == M_FETCH;
    const unsigned long long mask = __ballot(want);
    if (!mask) return;
    const int need = __popcll(mask);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    int taken = 0;
    int my_id = -1, my_frame = 0;
    for (;;) {
        const int avail = (int)(ch.end - ch.next);
        const int take = avail < need - taken ? avail : need - taken;
        if (want && rank >= taken && rank < taken + take) { my_id = (int)ch.next + (rank - taken); my_frame = ch.frame; }
        ch.next += (uint32_t)take;
        taken += take;
        if (taken == need || ch.exhausted) break;
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.tile_counter, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        /* Tickets of a multi-frame launch: first the `num_heavy_tiles` most expensive tiles (the
         * head of tile_order) of frame 0, of frame 1, ... of the last frame, then the other tiles
         * frame by frame.  Frames only meet in the blend of a pixel, so the longest jobs of EVERY
         * frame can start at once and everything else fills in behind them: the launch is then as
         * long as its work, not as its last frame's tail.  (num_heavy_tiles == 0, or one frame:
         * plainly frame by frame.) */
        if (t >= (uint32_t)a.num_tiles * (uint32_t)a.num_frames) { ch.exhausted = true; break; }
        if (a.job_order) {
            /* the host has laid out the whole schedule (rt_capi.cpp: longest job first over all frames) */
            const uint32_t job = a.job_order[t];
            ch.frame = (int)(job >> RT_JOB_FRAME_SHIFT);
            t = job & RT_JOB_TILE_MASK;
            ch.next = t * 64u;
            ch.end = t * 64u + 64u;
            continue;
        }
        uint32_t fr;
        const uint32_t nh = (uint32_t)a.num_heavy_tiles;
        if (t < nh * (uint32_t)a.num_frames) {
            fr = t / nh;
            t -= fr * nh;
        } else {
            const uint32_t nl = (uint32_t)a.num_tiles - nh;
            t -= nh * (uint32_t)a.num_frames;
            fr = t / nl;
            t = nh + (t - fr * nl);
        }
        ch.frame = (int)fr;
        /* ticket -> tile through a permutation.  A pixel's samples are sequential, so the frame
         * cannot finish before its most expensive tile does; the host therefore lists the tiles
         * whose centre ray enters a mesh box first (longest-job-first), each class scattered by a
         * stride coprime to the tile count so that neighbouring (equally expensive) tiles do not
         * land on the waves of one CU.  Any order gives the same image. */
        t = a.tile_order ? a.tile_order[t]
                         : (uint32_t)(((unsigned long long)t * (unsigned long long)a.tile_stride) % (unsigned long long)a.num_tiles);
        ch.next = t * 64u;
        ch.end = t * 64u + 64u;
    }
    if (!want) return;
    if (my_id < 0) { p.mode = M_DONE; return; }
    const int tile = my_id >> 6, within = my_id & 63;
    int tx, ty, compact_row;
    if (VIEWS) { ty = tile / a.tiles_x; tx = tile - ty * a.tiles_x; compact_row = 0; }    /* whole images only: tile t is the image's tile t */
    else tile_place(a, f, tile, tx, ty, compact_row);
    const int px = tx * 8 + (within & 7);
    const int py = ty * 8 + (within >> 3);
    p.id = (unsigned)my_id;
    if (BUDGET) {
        /* the pixel's budget n; 0 (or a slot outside the image): the lane stays in M_FETCH and nothing of the pixel is touched.  The
         * stream (the seed), the primary ray (the camera) and the restart state are the render branch's below, stated twice so that the
         * render kernel's code stays byte for byte: a change to either copy goes into both.  p.sample counts down from n */
        if (px >= f.W || py >= f.H) return;
        const int n = (int)px_budget(a).budget[(size_t)py * (size_t)f.W + (size_t)px];
        if (n == 0) return;
        const int array_index = (py * f.W + px) * 3;
        p.frame_steps = 0u;
        p.rng = (uint32_t)array_index * 3145739u + a.seeds[0];
        V3 plane_point = f.du * (float)px + f.dv * (float)py;
        p.primary = normalised((f.tl + plane_point) - f.cam_pos);
        p.colour = v3(0.f, 0.f, 0.f);
        p.fin = v3(0.f, 0.f, 0.f); p.thr = v3(1.f, 1.f, 1.f);
        p.o = f.cam_pos; p.d = p.primary;
        p.bounce = 0; p.cur_n = 1.0f;
        p.sample = n;
        if (f.limit > 0) p.mode = M_GEN;
        else px_finish_pixel<true>(p, a, f);                  /* a zero bounce limit traces nothing: (0,0,0) / n */
        return;
    }
    if (VIEWS) {
        /* the render branch below with the camera of the pixel's own view (my_frame) from the table, stated twice like the budget branch.
         * The table is at most 1.5 KB and every lane of the launch reads it: it stays in the L1 / L2. */
        if (px >= f.W || py >= f.H) return;
        const float *cam = px_views(a).cams + 12 * my_frame;
        const int array_index = (py * f.W + px) * 3;
        p.frame_steps = (unsigned)my_frame;
        p.rng = (uint32_t)array_index * 3145739u + a.seeds[my_frame];
        V3 plane_point = v3(cam[6], cam[7], cam[8]) * (float)px + v3(cam[9], cam[10], cam[11]) * (float)py;
        const V3 cam_pos = v3(cam[0], cam[1], cam[2]);
        p.primary = normalised((v3(cam[3], cam[4], cam[5]) + plane_point) - cam_pos);
        p.colour = v3(0.f, 0.f, 0.f);
        p.fin = v3(0.f, 0.f, 0.f); p.thr = v3(1.f, 1.f, 1.f);
        p.o = cam_pos; p.d = p.primary;
        p.bounce = 0; p.cur_n = 1.0f;
        p.sample = f.limit > 0 ? 0 : f.spp;
        if (p.sample >= f.spp) {
            const float q = 0.0f / (float)f.spp;
            p.colour = v3(q, q, q) * (float)f.spp;
            px_finish_pixel<false, true>(p, a, f);
        } else {
            p.mode = M_GEN;
        }
        return;
    }
    if (px < f.W && py < f.H) {
        /* src/raytracer.cu:123-127; Ray::set_direction_origin src/ray.cu:147-155,
         * cam_pixel_to_world src/camera.cu:24-29 */
        const int array_index = (py * f.W + px) * 3;
        p.frame_steps = (unsigned)my_frame;
        p.rng = (uint32_t)array_index * 3145739u + a.seeds[my_frame];
        RT_COST(p.c_steps = 0; p.c_wsteps = 0; p.c_t0 = (unsigned)wall_clock64());
        V3 plane_point = f.du * (float)px + f.dv * (float)py;
        p.primary = normalised((f.tl + plane_point) - f.cam_pos);
        if (CULL) {
            /* (the address is put together from two words of the block, so the compiler is told where it points: global memory) */
            typedef const __attribute__((address_space(1))) uint32_t *cull_words;
            /* the two words are read here, from the kernel's argument segment and by two volatile scalar loads of their own: as ordinary reads
             * of a.cull_lo / a.cull_hi they join the block's other argument loads into wider ones, and the compiler then keeps the whole block
             * in spilled scalar registers instead of loading an argument again where it is used (monkey +5 %).  The offsets are the block's,
             * so the block has to be the kernel's first parameter: rt_render_kernel.h asserts it for every kernel compiled with CULL */
            typedef const volatile __attribute__((address_space(4))) uint32_t *arg_words;
            const arg_words args = (arg_words)__builtin_amdgcn_kernarg_segment_ptr();
            const uint32_t plane_lo = args[offsetof(rt_kernel_args, cull_lo) / 4], plane_hi = args[offsetof(rt_kernel_args, cull_hi) / 4];
            const cull_words plane = (cull_words)(uintptr_t)(((uint64_t)plane_hi << 32) | (uint64_t)plane_lo);
            unsigned nocull = PX_NOCULL;
            uint32_t gates = 0u;     /* the pixel's dead gates (the subtree cull, rt_cull.h): the word behind the bit plane */
            if (plane) {
                const unsigned pixel = (unsigned)(py * f.W + px);
                nocull = (~(plane[pixel >> 5] >> (pixel & 31u))) << 31;
                gates = plane[rt_cull_words(f.W, f.H) + pixel];
                /* the pixel's entry word (rt_entry.h), behind the gate words: `nothing` makes the pixel a flagged one - its primary rays
                 * test no triangle that they hit - and `triangle T`, tagged by bit 0, which no gate word has, takes the gate word's place:
                 * the mesh start reads it there (rt_render_loop.inc) */
                const uint32_t entry = plane[rt_cull_entry_base(rt_cull_words(f.W, f.H)) + pixel];
                if (entry == RT_ENTRY_NOTHING) nocull = 0u;
                if (entry & RT_ENTRY_TAG) gates = entry;
                /* ... and a pixel whose own word is 0 may carry the slot of its sub-entry table there.  The slot word then takes the gate
                 * word's place too, marked by PX_SUBTABLE in p.id (bit 30, which no id reaches either): the table's words for the sub-boxes
                 * that are not known are the pixel's gate word itself, so px_gen's one load brings whichever the sample needs.  No register
                 * of its own: one more held across the traversal loops puts the kernel above the generic kernel's 97 VGPRs */
                if (rt_sub_slot_plus1(entry) != 0u) { gates = entry; nocull |= PX_SUBTABLE; }
            }
            p.id |= nocull;
            *px_gates = gates;
        }
        p.colour = v3(0.f, 0.f, 0.f);
        p.fin = v3(0.f, 0.f, 0.f); p.thr = v3(1.f, 1.f, 1.f);
        p.o = f.cam_pos; p.d = p.primary;
        p.bounce = 0; p.cur_n = 1.0f;
        /* a zero bounce limit traces nothing: every sample is (0,0,0) */
        p.sample = f.limit > 0 ? 0 : f.spp;
        if (p.sample >= f.spp) {
            const float q = 0.0f / (float)f.spp;               /* NaN for spp == 0, like the reference */
            p.colour = v3(q, q, q) * (float)f.spp;             /* px_finish_pixel divides by spp again: q either way */
            px_finish_pixel<false, false, CULL>(p, a, f);      /* M_FETCH: takes another pixel next time round */
        } else {
            p.mode = M_GEN;
        }
    }
    /* a pixel outside the image (ragged edge tile): stay in M_FETCH */
}

/* ================= GEN: jitter the direction, test the simple objects ====================== */
/* TRAITS: see rt_closest_simple (rt_intersect.h).  With RT_TRAIT_ONE_MESH a ray leaves as M_SHADE and the caller tests the one mesh's root box
 * at once (rt_render_loop.inc): there is no M_MESH and no mesh counter */
/* SUB (the kernel that reads the cull plane): *sub becomes the word the mesh start acts on (rt_render_loop.inc) - px_gates, the pixel's gate
 * word or tagged entry word, or, for a primary ray of a pixel with a sub-entry table (PX_SUBTABLE: px_gates is then its slot word, rt_entry.h),
 * the table's word for the sub-box of the very jitter added to the direction here.  The load is issued as soon as the jitter is known; the
 * mesh start uses it behind the simple objects' tests. */
template <bool HAS_MESH, int TRAITS = 0, bool SUB = false>
__device__ __forceinline__ void px_gen(Px &p, const rt_kernel_args &a, const Lds &L, const Frame *f = nullptr, uint32_t px_gates = 0u, uint32_t *sub = nullptr)
{
    V3 &o = p.o, &d = p.d;
    p.frame_steps += (unsigned)(RT_COST_GEN * RT_MAX_BATCH_FRAMES);
    /* Ray::apply_antialias src/ray.cu:130-142 */
    if (a.antialias) {
        V3 off;
        off.x = rt_jitter(rt_pcg_next(&p.rng));
        off.y = rt_jitter(rt_pcg_next(&p.rng));
        off.z = rt_jitter(rt_pcg_next(&p.rng));
        if (SUB) {
            uint32_t word = px_gates;
            if (((unsigned)p.bounce | (~p.id & PX_SUBTABLE)) == 0u) {
                /* (the plane's address as px_fetch reads it: two volatile scalar loads from the argument segment) */
                typedef const __attribute__((address_space(1))) uint32_t *cull_words;
                typedef const volatile __attribute__((address_space(4))) uint32_t *arg_words;
                const arg_words args = (arg_words)__builtin_amdgcn_kernarg_segment_ptr();
                const uint32_t plane_lo = args[offsetof(rt_kernel_args, cull_lo) / 4], plane_hi = args[offsetof(rt_kernel_args, cull_hi) / 4];
                const cull_words plane = (cull_words)(uintptr_t)(((uint64_t)plane_hi << 32) | (uint64_t)plane_lo);
                word = plane[rt_sub_tables_base(rt_cull_words(f->W, f->H)) + (size_t)(rt_sub_slot_plus1(px_gates) - 1u) * RT_SUB_WORDS + rt_sub_index(off.x, off.y, off.z)];
            }
            *sub = word;
        }
        d = normalised(d + off);
    } else if (SUB) {
        *sub = px_gates;
    }
    if (HAS_MESH) p.inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);   /* src/ray.cu:198-202 (three short reciprocals behind one range check: -0.3 % cube, +0.5 % monkey - not taken) */

    float best_t;
    int best_obj, best_prim;
    if (TRAITS & RT_TRAIT_SPHERES_ONLY) rt_closest_simple<true, TRAITS>(o, d, a.num_objects, L, best_t, best_obj, best_prim, (TRAITS & RT_TRAIT_ONE_MESH) ? px_traits(a).mesh_obj : -1);
    else rt_closest_simple<true>(o, d, a.num_objects, L, best_t, best_obj, best_prim);
    p.best_t = best_t; p.best_obj = best_obj; p.best_prim = best_prim;
    if (HAS_MESH && (TRAITS & RT_TRAIT_ONE_MESH)) { p.mode = M_SHADE; return; }
    p.next_mesh = 0;
    p.mode = (HAS_MESH && a.num_meshes > 0) ? M_MESH : M_SHADE;
}

#endif
