// The argument checks of the denoiser's entry points (rt_denoise_capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; test
// infrastructure): a context built in host memory (no GPU is opened: nothing here gets as far as a HIP call), every refusal of
// include/rt_amd.h with random sizes, parameters and pointers.  Kernel launchers are stubs that fail the run if they are reached.
//   denoise_host_fuzz <seed> <iterations>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>

#include "rt_denoise.h"
#include "rt_internal.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                          \
    do {                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "denoise fuzz: %s (iteration %d)\n", what, it); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int iterations = argc > 2 ? std::atoi(argv[2]) : 1000;
    std::mt19937 rng(seed);
    rt_ctx ctx;
    float plane[4 * 4 * 3] = {0};
    int32_t ids[4 * 4] = {0};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int it = 0; it < iterations; it++) {
        rt_denoise_params good;
        std::memset(&good, 0xAB, sizeof good);
        rt_denoise_params_default(&good);
        CHECK(good.iterations >= 1 && good.iterations <= 8 && good.sigma_colour > 0 && good.sigma_depth > 0 && good.normal_power_log2 >= 0 &&
              good.normal_power_log2 <= 8 && good.albedo_floor > 0 && !good.reserved[0] && !good.reserved[1] && !good.reserved[2], "defaults in range");
        ctx.err.clear();
        // null context first, whatever else is wrong
        CHECK(rt_denoise(nullptr, 4, 4, plane, plane, plane, ids, plane, &good, plane) == RT_ERR_INVALID, "null context, host form");
        CHECK(rt_denoise_device(nullptr, -1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "null context, device form");
        // a null required pointer (object and albedo are optional)
        const int which = (int)(rng() % 5);
        const float *c = which == 0 ? nullptr : plane, *n = which == 1 ? nullptr : plane, *z = which == 2 ? nullptr : plane;
        float *out = which == 3 ? nullptr : plane;
        const rt_denoise_params *pp = which == 4 ? nullptr : &good;
        CHECK(rt_denoise(&ctx, 4, 4, c, n, z, ids, plane, pp, out) == RT_ERR_INVALID && std::string(rt_last_error(&ctx)).find("null argument") != std::string::npos, "null pointer, host form");
        CHECK(rt_denoise_device(&ctx, 4, 4, c, n, z, nullptr, nullptr, pp, out, nullptr) == RT_ERR_INVALID, "null pointer, device form");
        // sizes
        int32_t w = 4, h = 4;
        switch (rng() % 4) {
            case 0: w = -(int32_t)(rng() % 100); break;
            case 1: h = 0; break;
            case 2: w = 32769 + (int32_t)(rng() % 1000); break;
            default: w = 32768; h = 8193 + (int32_t)(rng() % 1000); break;
        }
        CHECK(rt_denoise(&ctx, w, h, plane, plane, plane, ids, plane, &good, plane) == RT_ERR_INVALID && std::string(rt_last_error(&ctx)).find("image size") != std::string::npos, "bad image size, host form");
        CHECK(rt_denoise_device(&ctx, w, h, plane, plane, plane, ids, plane, &good, plane, nullptr) == RT_ERR_INVALID, "bad image size, device form");
        // parameters
        rt_denoise_params bad = good;
        const float *albedo = plane;
        switch (rng() % 9) {
            case 0: bad.iterations = 0 - (int32_t)(rng() % 1000); break;
            case 1: bad.iterations = 9 + (int32_t)(rng() % 1000); break;
            case 2: bad.sigma_colour = (rng() & 1) ? 0.0f : -1.0f / (float)(1 + rng() % 100); break;
            case 3: bad.sigma_colour = (rng() & 1) ? nan : inf; break;
            case 4: bad.sigma_depth = (rng() & 1) ? nan : -(float)(rng() % 100); break;
            case 5: bad.normal_power_log2 = (rng() & 1) ? -1 - (int32_t)(rng() % 100) : 9 + (int32_t)(rng() % 100); break;
            case 6: bad.albedo_floor = (rng() & 1) ? 0.0f : nan; break;
            case 7: bad.reserved[rng() % 3] = 1 + (int32_t)(rng() % 1000); break;
            default: bad.sigma_depth = inf; albedo = nullptr; break;
        }
        CHECK(rt_denoise(&ctx, 4, 4, plane, plane, plane, ids, albedo, &bad, plane) == RT_ERR_INVALID && std::string(rt_last_error(&ctx)).find("denoise parameters") != std::string::npos, "bad parameters, host form");
        CHECK(rt_denoise_device(&ctx, 4, 4, plane, plane, plane, nullptr, albedo, &bad, plane, nullptr) == RT_ERR_INVALID, "bad parameters, device form");
        CHECK(g_launches == 0, "a refused call reached a launcher");
    }
    std::printf("denoise entry points: %d iterations, sanitizers silent\n", iterations);
    return 0;
}
