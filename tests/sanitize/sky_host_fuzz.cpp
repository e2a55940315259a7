// The host side of the cube-map sky (rt_sky.h, rt_sky_capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; test
// infrastructure): the lookup as the host compiles it on seeded random and special directions - NaN, Inf, zeros, subnormals, ties between
// the axes - always inside the map and on the face the definition names; the round trip texel -> direction -> texel, as given, normalised and
// scaled; the packing of a map for the device; and every refusal of the entry points through the C ABI on a context built in host memory
// (no GPU is opened: nothing here gets as far as a HIP call), each with the message rt_render_views[_device] gives for the same arguments,
// whose checks they share.  Kernel launchers are stubs that fail the run if they are reached.
//   sky_host_fuzz <seed> <iterations>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "rt_sky.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                      \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "sky fuzz: %s (iteration %d)\n", what, it); return 1; } \
    } while (0)

static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

static float uniform(std::mt19937 &rng, float lo, float hi) { return lo + (hi - lo) * (float)(rng() % 100001) / 100000.0f; }

// the definition's face, restated: the first axis that is at least as large as the others (a NaN compares false), its sign (-0 positive)
static int face_of(float x, float y, float z)
{
    const float ax = std::fabs(x), ay = std::fabs(y), az = std::fabs(z);
    if (ax >= ay && ax >= az) return x < 0.0f ? 1 : 0;
    if (ay >= az) return y < 0.0f ? 3 : 2;
    return z < 0.0f ? 5 : 4;
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int iterations = argc > 2 ? std::atoi(argv[2]) : 1000;
    std::mt19937 rng(seed);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), tiny = std::numeric_limits<float>::denorm_min();
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, inf, -inf, nan, tiny, -tiny, 1e-39f, std::numeric_limits<float>::min(), std::numeric_limits<float>::max(),
                             -std::numeric_limits<float>::max(), 0.5f, 1e-3f};
    const int n_special = (int)(sizeof special / sizeof special[0]);
    rt_ctx ctx, other;
    rt_scene scene, foreign_scene;
    scene.ctx = &ctx;
    foreign_scene.ctx = &other;
    rt_sky sky, foreign_sky;                       // no texels: nothing reads them before a launch, and no launch is reached
    sky.ctx = &ctx;
    sky.face_size = 4;
    foreign_sky.ctx = &other;
    foreign_sky.face_size = 4;
    rt_render_settings rs{4, 8, 1, {1.0f, 1.0f, 1.0f}};
    std::vector<float> frames(RT_VIEWS_MAX * 16 * 16 * 3, 7.0f);
    rt_camera cam;
    rt_camera_default(16, 16, &cam);
    for (int it = 0; it < iterations; it++) {
        const int n = it % 7 == 0 ? 1 + (int)(rng() % RT_SKY_MAX_FACE) : 1 + (int)(rng() % 70);
        // ---- the lookup: always inside the map, on the definition's face ----------------------------------------------------------
        {
            float d[3];
            const int kind = (int)(rng() % 4);
            for (int k = 0; k < 3; k++) d[k] = kind == 0 ? special[rng() % n_special] : uniform(rng, -2.0f, 2.0f);
            if (kind == 1) d[rng() % 3] = special[rng() % n_special];                    // one special component among ordinary ones
            if (kind == 2) { const float v = d[0]; d[rng() % 3] = rng() & 1 ? v : -v; }   // a tie between two axes
            int face = -1, row = -1, col = -1;
            const uint32_t index = rt_sky_lookup(d[0], d[1], d[2], n, &face, &row, &col);
            CHECK(face >= 0 && face < 6 && row >= 0 && row < n && col >= 0 && col < n, "the lookup stays inside the map");
            CHECK(index == ((uint32_t)face * (uint32_t)n + (uint32_t)row) * (uint32_t)n + (uint32_t)col && index < 6u * (uint32_t)n * (uint32_t)n, "the texel's index");
            CHECK(face == face_of(d[0], d[1], d[2]), "the face the definition names");
            CHECK(rt_sky_lookup(d[0], d[1], d[2], n, nullptr, nullptr, nullptr) == index, "the outputs are optional");
        }
        // ---- the round trip ---------------------------------------------------------------------------------------------------------
        {
            const int face = (int)(rng() % 6), row = it % 3 == 0 ? (rng() & 1 ? 0 : n - 1) : (int)(rng() % (unsigned)n), col = it % 5 == 0 ? (rng() & 1 ? 0 : n - 1) : (int)(rng() % (unsigned)n);
            float d[3] = {9.0f, 9.0f, 9.0f};
            CHECK(rt_sky_texel_direction(n, face, row, col, d) == RT_OK, "a texel's direction");
            CHECK(std::fabs(d[face >> 1]) == 1.0f && (d[face >> 1] < 0.0f) == ((face & 1) != 0), "the major component is +1 or -1");
            const volatile float q = ((float)col + 0.5f) / (float)n, twice = q * 2.0f, s = twice - 1.0f;
            CHECK(d[((face >> 1) + 1) % 3] == s, "the column's coordinate, operation by operation");
            const float inv = 1.0f / std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            const float forms[3][3] = {{d[0], d[1], d[2]}, {d[0] * inv, d[1] * inv, d[2] * inv}, {d[0] * 1e-3f, d[1] * 1e-3f, d[2] * 1e-3f}};
            for (const float *v : forms) {
                int f = -1, r = -1, c = -1;
                rt_sky_lookup(v[0], v[1], v[2], n, &f, &r, &c);
                CHECK(f == face && r == row && c == col, "the lookup of a texel's direction is the texel (as given, normalised, scaled)");
            }
            // refusals leave `out` alone
            float keep[3] = {7.0f, 7.0f, 7.0f};
            const int32_t bad_n[] = {0, -1 - (int32_t)(rng() % 100), RT_SKY_MAX_FACE + 1 + (int32_t)(rng() % 100)};
            CHECK(rt_sky_texel_direction(bad_n[rng() % 3], face, 0, 0, keep) == RT_ERR_INVALID, "texel direction: face size");
            CHECK(rt_sky_texel_direction(n, rng() & 1 ? -1 : 6, row, col, keep) == RT_ERR_INVALID, "texel direction: face");
            CHECK(rt_sky_texel_direction(n, face, rng() & 1 ? -1 : n, col, keep) == RT_ERR_INVALID && rt_sky_texel_direction(n, face, row, rng() & 1 ? -1 : n, keep) == RT_ERR_INVALID, "texel direction: row / col");
            CHECK(rt_sky_texel_direction(n, face, row, col, nullptr) == RT_ERR_INVALID, "texel direction: null out");
            CHECK(keep[0] == 7.0f && keep[1] == 7.0f && keep[2] == 7.0f, "a refused call leaves out untouched");
        }
        // ---- packing a map for the device -----------------------------------------------------------------------------------------------
        if (n <= 70) {
            std::vector<float> faces((size_t)6 * n * n * 3);
            for (float &f : faces) f = rng() % 9 == 0 ? special[rng() % n_special] : uniform(rng, 0.0f, 50.0f);
            std::vector<float> packed(rt_sky_host::device_floats(n), 9.0f);
            CHECK(packed.size() == (size_t)6 * n * n * RT_SKY_TEXEL_FLOATS, "the device copy's size");
            rt_sky_host::pack(faces.data(), n, packed.data());
            for (size_t i = 0; i < (size_t)6 * n * n; i++) {
                CHECK(!std::memcmp(&packed[i * RT_SKY_TEXEL_FLOATS], &faces[i * 3], 12), "a texel's three values, bit for bit");
                for (int k = 3; k < RT_SKY_TEXEL_FLOATS; k++) CHECK(packed[i * RT_SKY_TEXEL_FLOATS + k] == 0.0f, "the pad is zero");
            }
        }
        // ---- the entry points' refusals, through the C ABI ------------------------------------------------------------------------------
        {
            const int32_t nv = 1 + (int32_t)(rng() % RT_VIEWS_MAX);
            std::vector<rt_camera> cams((size_t)nv, cam);
            std::vector<int32_t> times((size_t)nv, 5);
            int32_t fn = 0;
            const int32_t acc = (int32_t)(rng() & 1);
            ctx.err.clear();
            rt_sky *made = (rt_sky *)&sky;
            const float one_texel[18] = {0};
            CHECK(rt_sky_create(nullptr, 1, one_texel, &made) == RT_ERR_INVALID && rt_sky_create(&ctx, 1, nullptr, &made) == RT_ERR_INVALID && said(ctx, "null argument"), "create: null");
            CHECK(rt_sky_create(&ctx, 1, one_texel, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "create: null out");
            CHECK(rt_sky_create(&ctx, rng() & 1 ? 0 : RT_SKY_MAX_FACE + 1, one_texel, &made) == RT_ERR_INVALID && said(ctx, "face size") && made == &sky, "create: face size");
            rt_sky_destroy(nullptr);
            // a null context first, whatever else is wrong
            CHECK(rt_render_sky_device(nullptr, &scene, &sky, cams.data(), times.data(), nv, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID, "null context, device form");
            CHECK(rt_render_sky(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == RT_ERR_INVALID, "null context, host form");
            // the sky
            CHECK(rt_render_sky_device(&ctx, &scene, nullptr, cams.data(), times.data(), nv, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null sky, device form");
            CHECK(rt_render_sky(&ctx, &scene, nullptr, cams.data(), times.data(), nv, &rs, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "null argument"), "null sky, host form");
            CHECK(rt_render_sky_device(&ctx, &scene, &foreign_sky, cams.data(), times.data(), nv, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "sky belongs to another context"), "foreign sky, device form");
            CHECK(rt_render_sky(&ctx, &scene, &foreign_sky, cams.data(), times.data(), nv, &rs, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "sky belongs to another context"), "foreign sky, host form");
            CHECK(rt_render_sky(&ctx, &scene, &sky, cams.data(), times.data(), nv, &rs, acc, nullptr, frames.data()) == RT_ERR_INVALID && said(ctx, "null argument"), "null frame_num, host form");
            // everything the camera sequences refuse, with their message: one bad argument per round
            rt_render_settings r = rs;
            std::vector<rt_camera> c = cams;
            const rt_scene *sc = &scene;
            const rt_camera *cp = c.data();
            const int32_t *tp = times.data();
            const rt_render_settings *rp = &r;
            float *fp = frames.data();
            int32_t views = nv, a = acc, frame_num = 0;
            const char *msg = "";
            switch (rng() % 12) {
                case 0: sc = nullptr; msg = "null argument"; break;
                case 1: sc = &foreign_scene; msg = "another context"; break;
                case 2: cp = nullptr; msg = "null argument"; break;
                case 3: tp = nullptr; msg = "null argument"; break;
                case 4: rp = nullptr; msg = "null argument"; break;
                case 5: fp = nullptr; msg = "null argument"; break;
                case 6: views = rng() & 1 ? -(int32_t)(rng() % 3) : RT_VIEWS_MAX + 1 + (int32_t)(rng() % 100); msg = "number of views"; break;
                case 7: frame_num = -1 - (int32_t)(rng() % 100); msg = "frame number"; break;
                case 8: a = 0; frame_num = 1 + (int32_t)(rng() % 100); msg = "frame number"; break;
                case 9: (rng() & 1 ? r.reflection_limit : r.rays_per_pixel) = -1 - (int32_t)(rng() % 100); msg = "render settings"; break;
                case 10: (rng() & 1 ? c[0].width : c[0].height) = rng() & 1 ? -(int32_t)(rng() % 100) : 32769 + (int32_t)(rng() % 1000); msg = "image size"; break;
                default:
                    if (nv > 1) { c[1 + rng() % (size_t)(nv - 1)].width += 1; msg = "share one image size"; }
                    else { views = 0; msg = "number of views"; }
                    break;
            }
            CHECK(rt_render_views_device(&ctx, sc, cp, tp, views, rp, a, frame_num, fp, nullptr) == RT_ERR_INVALID && said(ctx, msg), "the camera sequences refuse it");
            const std::string theirs = ctx.err;
            ctx.err.clear();
            CHECK(rt_render_sky_device(&ctx, sc, &sky, cp, tp, views, rp, a, frame_num, fp, nullptr) == RT_ERR_INVALID && ctx.err == theirs, "the sky's device form refuses it in the same words");
            if (views <= RT_VIEWS_MAX) {                  // (the host form takes any number of views from 1)
                int32_t fnb = frame_num;
                ctx.err.clear();
                CHECK(rt_render_sky(&ctx, sc, &sky, cp, tp, views, rp, a, &fnb, fp) == RT_ERR_INVALID && ctx.err == theirs && fnb == frame_num, "the sky's host form refuses it in the same words");
            }
            CHECK(g_launches == 0 && fn == 0, "a refused call reached a launcher or moved the frame number");
        }
    }
    for (float f : frames)
        if (f != 7.0f) { std::fprintf(stderr, "sky fuzz: a refused call wrote the frames\n"); return 1; }
    std::printf("sky host side: %d iterations, sanitizers silent\n", iterations);
    return 0;
}
