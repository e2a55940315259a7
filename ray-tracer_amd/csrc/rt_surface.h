/*
 * rt_surface.h — the surface at a closest hit, for the ray kernels (rt_query_kernel.h, rt_occlusion_kernel.h, rt_ao_kernel.h): hit point,
 * shading normal, texture coordinates, texture colour.  The render kernel keeps its own statement of these expressions in px_shade
 * (rt_pixel.h); the comments below say why.
 */
#ifndef RT_SURFACE_H
#define RT_SURFACE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_scene.h"
#include "rt_intersect.h"
#include "rt_math.h"
#include "rt_vec.h"

/* The surface at a closest hit for the query kernels (rt_query_kernel.h): the hit point, the shading normal and, when the object's material
 * needs them (`packed` bit 4), the texture coordinates - else 0.  These are px_shade's expressions, stated a second time: px_shade calling
 * this function (and rt_texture_colour below) compiles to render kernels with another register allocation, and the render kernels' code is
 * not to change with the queries.  tests/test_gpu_query.py holds this copy to the oracle bit for bit, as test_gpu_parity.py holds px_shade. */
__device__ __forceinline__ void rt_hit_surface(V3 o, V3 d, float best_t, int best_obj, int best_prim, uint32_t packed, const Lds &L, const float *tri_uv,
                                               V3 &P, V3 &N, float &tex_u, float &tex_v)
{
    /* hit point and normal: Ray::get_pos src/ray.cu:63-65; Sphere :66; Triangle :158 */
    P = d * best_t + o;
    tex_u = 0.f; tex_v = 0.f;
    if (packed & 32u) {
        const v4f sc = L.objs[RT_OBJLDS_F4 * best_obj + 2];
        N = normalised(P - v3(sc.x, sc.y, sc.z));
        if (packed & 16u) {
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
        if (packed & 16u) {
            /* Triangle::assign_texture_coords src/objects.cu:160,196-199, called as (w,u,v) */
            float t, u, v;
            tri_test(L.tris, best_prim, o, d, t, u, v);
            float w = 1.0f - u - v;
            const float *uv = tri_uv + 6 * best_prim;
            tex_u = uv[0] * w + uv[2] * u + uv[4] * v;
            tex_v = uv[1] * w + uv[3] * u + uv[5] * v;
        }
    }
}

/* Texture::get_texture_colour src/material.cu:53-69 for the object record (ma, mb) at (tex_u, tex_v): what trace_ray multiplies the
 * throughput by, for the albedo plane of rt_query_kernel.h (px_shade's lookup, restated for the same reason) */
__device__ __forceinline__ V3 rt_texture_colour(const v4f ma, const v4f mb, uint32_t packed, float tex_u, float tex_v, const float *tex_data)
{
    V3 tc;
    const int tex = (int)((packed >> 2) & 3u);
    if (tex == 0) {
        tc = v3(ma.x, ma.y, ma.z);
    } else if (tex == 1) {
        tc = v3(tex_u, tex_v, 0.f);                              /* gradient src/material.cu:80-82 */
    } else if (tex == 3) {
        /* image src/material.cu:119-124: nearest texel; an out-of-range index is clamped */
        const int iw = (int)__float_as_uint(ma.x), ih = (int)__float_as_uint(ma.y);
        const int uc = rt_f2i((float)(iw - 1) * tex_u), vc = rt_f2i((float)(ih - 1) * tex_v);
        int idx = (int)((uint32_t)vc * (uint32_t)iw + (uint32_t)uc);       /* wraps like the 32-bit machine arithmetic */
        idx = idx < 0 ? 0 : (idx > iw * ih - 1 ? iw * ih - 1 : idx);
        const float *tx = tex_data + (size_t)__float_as_uint(ma.z) + 3 * (size_t)idx;
        tc = v3(tx[0], tx[1], tx[2]);
    } else {
        const int nsq = (int)(packed >> 8);                      /* checkerboard :90-99 */
        const int uc = rt_f2i(tex_u * (float)nsq), vc = rt_f2i(tex_v * (float)nsq);
        tc = ((int)((uint32_t)uc + (uint32_t)vc) % 2 == 0) ? v3(ma.x, ma.y, ma.z) : v3(mb.x, mb.y, mb.z);
    }
    return tc;
}

#endif
