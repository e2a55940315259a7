/*
 * rt_sky.h — the cube-map sky (include/rt_amd.h: rt_sky_create, rt_sky_texel_direction, rt_render_sky[_device]): what the kernel
 * (rt_pixel.h, px_shade_miss under SKY), the entry points (rt_sky_capi.cpp) and the host-only sanitizer program
 * (tests/sanitize/sky_host_fuzz.cpp) share.  The lookup and its inverse as the one text every side compiles (binary32, nothing fused: the
 * library and the tests build with contraction off) and the argument checks; the sky kernel's launcher is rt_launch.h's rt_launch_sky.
 * Host code; self-contained.
 */
#ifndef RT_SKY_H
#define RT_SKY_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_amd.h"     /* RT_SKY_MAX_FACE */
#include "rt_device_scene.h"
#include "rt_math.h"

/* floats per texel on the device: 4 (r, g, b and a pad: one aligned 16-byte load per sample) or 3 (the caller's layout: 12 bytes).  The
 * shipped value is what tools/sky_probe.py measured no slower; the other is a development build. */
#ifndef RT_SKY_TEXEL_FLOATS
#define RT_SKY_TEXEL_FLOATS 4
#endif

/* ---- the lookup (include/rt_amd.h has the definition) -------------------------------------------------------------------------- */
/* a face coordinate in [-1, 1] -> its texel column or row: (s * 0.5f + 0.5f) * (float)n, three roundings, converted towards zero and
 * clamped (a NaN is texel 0) */
RT_HD int rt_sky_coord(float s, int n)
{
    const float h = s * 0.5f;
    const float u = h + 0.5f;
    const int i = rt_f2i(u * (float)n);
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

/* direction (x, y, z) -> the texel's index face * n * n + row * n + col, always inside 6 * n * n; face, row, col: optional */
RT_HD uint32_t rt_sky_lookup(float x, float y, float z, int n, int *face_out, int *row_out, int *col_out)
{
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y), az = __builtin_fabsf(z);
    int axis;
    float c, a, b;
    if (ax >= ay && ax >= az) { axis = 0; c = x; a = y; b = z; }
    else if (ay >= az)        { axis = 1; c = y; a = z; b = x; }
    else                      { axis = 2; c = z; a = x; b = y; }
    const float m = __builtin_fabsf(c);
    const int face = 2 * axis + (c < 0.0f ? 1 : 0);
    const float s = a / m, t = b / m;
    const int col = rt_sky_coord(s, n), row = rt_sky_coord(t, n);
    if (face_out) *face_out = face;
    if (row_out) *row_out = row;
    if (col_out) *col_out = col;
    return ((uint32_t)face * (uint32_t)n + (uint32_t)row) * (uint32_t)n + (uint32_t)col;
}

/* the inverse: the direction through the centre of texel (face, row, col); the arguments are in range */
RT_HD float rt_sky_centre(int i, int n)
{
    const float q = ((float)i + 0.5f) / (float)n;
    const float d = q * 2.0f;
    return d - 1.0f;
}

RT_HD void rt_sky_direction(int n, int face, int row, int col, float out[3])
{
    const int axis = face >> 1;
    const float major = (face & 1) ? -1.0f : 1.0f;
    const float s = rt_sky_centre(col, n), t = rt_sky_centre(row, n);
    out[axis] = major;
    out[(axis + 1) % 3] = s;
    out[(axis + 2) % 3] = t;
}

namespace rt_sky_host {

inline bool face_size_ok(int32_t n) { return n >= 1 && n <= RT_SKY_MAX_FACE; }

/* what is wrong with rt_sky_texel_direction's arguments (nullptr: nothing) */
inline const char *texel_error(int32_t n, int32_t face, int32_t row, int32_t col, const float *out)
{
    if (!out) return "null argument";
    if (!face_size_ok(n)) return "bad face size (1 .. RT_SKY_MAX_FACE)";
    if (face < 0 || face > 5) return "bad face (0 .. 5)";
    if (row < 0 || row >= n || col < 0 || col >= n) return "bad texel (0 .. face_size - 1)";
    return nullptr;
}

/* the device copy of a map, from the caller's faces[6][n][n][3]: RT_SKY_TEXEL_FLOATS per texel, the pad zero */
inline size_t device_floats(int32_t n) { return (size_t)6 * (size_t)n * (size_t)n * RT_SKY_TEXEL_FLOATS; }
inline void pack(const float *faces_rgb, int32_t n, float *out)
{
    const size_t texels = (size_t)6 * (size_t)n * (size_t)n;
    for (size_t i = 0; i < texels; i++) {
        __builtin_memcpy(out + i * RT_SKY_TEXEL_FLOATS, faces_rgb + i * 3, 12);      /* (bytes: a NaN keeps its payload) */
        for (int k = 3; k < RT_SKY_TEXEL_FLOATS; k++) out[i * RT_SKY_TEXEL_FLOATS + k] = 0.0f;
    }
}

}  // namespace rt_sky_host

#endif
