// The argument checks of the ray-query / AOV entry points (rt_query_capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; test
// infrastructure): a context and two scenes built in host memory (no GPU is opened: nothing here gets as far as a HIP call), every
// refusal of include/rt_amd.h with random counts, sizes and pointers.  Kernel launchers are stubs that fail the run if they are reached.
//   query_host_fuzz <seed> <iterations>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "rt_internal.h"
#include "rt_query.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                        \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "query fuzz: %s (iteration %d)\n", what, it); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int iterations = argc > 2 ? std::atoi(argv[2]) : 1000;
    std::mt19937 rng(seed);
    rt_ctx ctx, other;
    rt_scene mine, foreign;
    mine.ctx = &ctx;
    foreign.ctx = &other;
    float rays[64 * 3] = {0};
    rt_hit hits[64];
    float sky[3] = {0, 0, 0}, plane[16];
    int32_t iplane[16];
    for (int it = 0; it < iterations; it++) {
        const int64_t bad_n = -(int64_t)(rng() % 1000000) - 1, big_n = (int64_t)RT_QUERY_MAX_RAYS + 1 + (int64_t)(rng() % 1000), n = 1 + (int64_t)(rng() % 64);
        ctx.err.clear();
        CHECK(rt_trace_rays(&ctx, &mine, rays, rays, bad_n, hits) == RT_ERR_INVALID && std::string(rt_last_error(&ctx)).find("ray count") != std::string::npos, "n < 0");
        CHECK(rt_trace_rays_device(&ctx, &mine, rays, rays, big_n, hits, nullptr) == RT_ERR_INVALID, "n too large");
        const int which = (int)(rng() % 3);
        CHECK(rt_trace_rays(&ctx, &mine, which == 0 ? nullptr : rays, which == 1 ? nullptr : rays, n, which == 2 ? nullptr : hits) == RT_ERR_INVALID, "null pointer, host form");
        CHECK(rt_trace_rays_device(&ctx, &mine, which == 0 ? nullptr : rays, which == 1 ? nullptr : rays, n, which == 2 ? nullptr : hits, nullptr) == RT_ERR_INVALID, "null pointer, device form");
        CHECK(rt_trace_rays_device(&ctx, &mine, rays, rays, n, (rt_hit *)((char *)hits + 4 * (1 + rng() % 3)), nullptr) == RT_ERR_INVALID, "misaligned records");
        CHECK(rt_trace_rays(&ctx, &foreign, rays, rays, n, hits) == RT_ERR_INVALID && std::string(rt_last_error(&ctx)).find("another context") != std::string::npos, "foreign scene");
        CHECK(rt_trace_rays(&ctx, nullptr, rays, rays, n, hits) == RT_ERR_INVALID && rt_trace_rays(nullptr, &mine, rays, rays, n, hits) == RT_ERR_INVALID, "null scene / context");
        CHECK(rt_trace_rays(&ctx, &mine, nullptr, nullptr, 0, nullptr) == RT_OK && rt_trace_rays_device(&ctx, &mine, nullptr, nullptr, 0, nullptr, nullptr) == RT_OK, "n == 0");
        rt_camera cam;
        std::memset(&cam, 0, sizeof cam);
        cam.width = 4; cam.height = 4;
        CHECK(rt_render_aov(&ctx, &mine, &cam, sky, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "no plane, host form");
        CHECK(rt_render_aov_device(&ctx, &mine, &cam, sky, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "no plane, device form");
        CHECK(rt_render_aov(&ctx, &foreign, &cam, sky, plane, nullptr, nullptr, iplane, nullptr) == RT_ERR_INVALID, "foreign scene, planes");
        CHECK(rt_render_aov(&ctx, &mine, nullptr, sky, plane, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "null camera");
        CHECK(rt_render_aov(&ctx, &mine, &cam, nullptr, plane, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "null sky");
        switch (rng() % 4) {
            case 0: cam.width = -(int32_t)(rng() % 100); break;
            case 1: cam.height = 0; break;
            case 2: cam.width = 32769 + (int32_t)(rng() % 1000); break;
            default: cam.width = 32768; cam.height = 8193 + (int32_t)(rng() % 1000); break;
        }
        CHECK(rt_render_aov_device(&ctx, &mine, &cam, sky, plane, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "bad image size");
        CHECK(g_launches == 0, "a refused call reached a launcher");
    }
    std::printf("query entry points: %d iterations, sanitizers silent\n", iterations);
    return 0;
}
