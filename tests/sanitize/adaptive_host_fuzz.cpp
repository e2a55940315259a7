// The host side of the budget render and the adaptive driver (rt_adaptive_capi.cpp, rt_adaptive.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer (CPU only; test infrastructure): a pass's tile list from random tile_active / tile_error planes (order, ties,
// an empty list, NaN and infinite errors, ragged image sizes) against a plain restatement, the parameter validation on every range's both
// sides, and every refusal of include/rt_amd.h through the C ABI on a context built in host memory (no GPU is opened: nothing here gets as
// far as a HIP call).  Kernel launchers are stubs that fail the run if they are reached.
//   adaptive_host_fuzz <seed> <iterations>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rt_adaptive.h"
#include "rt_internal.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                           \
    do {                                                                                            \
        if (!(cond)) { std::fprintf(stderr, "adaptive fuzz: %s (iteration %d)\n", what, it); return 1; } \
    } while (0)

static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int iterations = argc > 2 ? std::atoi(argv[2]) : 1000;
    std::mt19937 rng(seed);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    rt_ctx ctx, other;
    rt_scene scene, foreign;
    scene.ctx = &ctx;
    foreign.ctx = &other;
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    rt_render_settings rs{4, 8, 1, {1.0f, 1.0f, 1.0f}};
    uint16_t budget[16 * 16] = {0};
    uint32_t count[16 * 16] = {0};
    float frame[16 * 16 * 3] = {0};
    float tile_plane[4] = {0};
    for (int it = 0; it < iterations; it++) {
        // ---- the tile list of a pass ---------------------------------------------------------------------------------------------
        {
            const int W = 1 + (int)(rng() % 70), H = 1 + (int)(rng() % 50);       // ragged edges in most draws
            const int n = ((W + 7) / 8) * ((H + 7) / 8);
            std::vector<float> err((size_t)n);
            std::vector<uint32_t> act((size_t)n);
            const int kind = (int)(rng() % 4);
            for (int t = 0; t < n; t++) {
                // few distinct errors, so that ties are the rule; now and then an infinity or a NaN
                const unsigned r = rng() % 16;
                err[(size_t)t] = r == 0 ? inf : (r == 1 && kind == 3 ? nan : (float)(rng() % 5) * 0.25f);
                act[(size_t)t] = kind == 0 ? 0u : (kind == 1 ? 1u + rng() % 64 : (rng() % 3 ? 0u : 1u + rng() % 64));
            }
            std::vector<uint32_t> list(3, 77u);                                   // (old content goes)
            rt_adaptive::build_tile_list(err.data(), act.data(), n, list);
            size_t want = 0;
            for (int t = 0; t < n; t++) want += act[(size_t)t] != 0u;
            CHECK(list.size() == want, "the list holds the tiles with an active pixel");
            CHECK(kind != 0 || list.empty(), "no active pixel: an empty list");
            std::vector<char> seen((size_t)n, 0);
            for (size_t i = 0; i < list.size(); i++) {
                const uint32_t t = list[i];
                CHECK(t < (uint32_t)n && act[t] != 0u && !seen[t], "a listed tile is in the image, active and listed once");
                seen[t] = 1;
                if (i == 0) continue;
                const uint32_t p = list[i - 1];
                const float ep = err[p], et = err[t];
                const bool np_ = ep != ep, nt = et != et;
                // by decreasing error (a NaN ahead of everything), ties by the lower index
                CHECK((np_ && !nt) || (np_ == nt && (np_ || ep > et || (ep == et && p < t))), "order: decreasing error, ties by the lower index");
            }
        }
        // ---- the parameters ------------------------------------------------------------------------------------------------------
        rt_adaptive_params good;
        std::memset(&good, 0xAB, sizeof good);
        rt_adaptive_params_default(&good);
        CHECK(rt_adaptive::params_error(good) == nullptr && good.reserved[0] == 0, "defaults in range");
        {
            // both ends of every range are accepted
            rt_adaptive_params p = good;
            p.pilot_spp = 1; p.step_spp = 65535; p.max_spp = 1; p.max_passes = 0; p.pixel_threshold = inf;
            CHECK(rt_adaptive::params_error(p) == nullptr, "low ends accepted");
            p.pilot_spp = 65535; p.step_spp = 1; p.max_spp = 1 << 24; p.max_passes = 64; p.pixel_threshold = 1e-30f; p.threshold = 3e38f; p.floor = 1e-38f;
            CHECK(rt_adaptive::params_error(p) == nullptr, "high ends accepted");
        }
        rt_adaptive_params bad = good;
        switch (rng() % 14) {
            case 0: bad.pilot_spp = 0 - (int32_t)(rng() % 1000); break;
            case 1: bad.pilot_spp = 65536 + (int32_t)(rng() % 1000); bad.max_spp = 1 << 24; break;
            case 2: bad.step_spp = 0 - (int32_t)(rng() % 1000); break;
            case 3: bad.step_spp = 65536 + (int32_t)(rng() % 1000); break;
            case 4: bad.max_spp = bad.pilot_spp - 1 - (int32_t)(rng() % 10); break;
            case 5: bad.max_spp = (1 << 24) + 1 + (int32_t)(rng() % 1000); break;
            case 6: bad.max_passes = -1 - (int32_t)(rng() % 100); break;
            case 7: bad.max_passes = 65 + (int32_t)(rng() % 100); break;
            case 8: bad.threshold = (rng() & 1) ? 0.0f : ((rng() & 1) ? nan : inf); break;
            case 9: bad.threshold = -1.0f / (float)(1 + rng() % 100); break;
            case 10: bad.pixel_threshold = (rng() & 1) ? 0.0f : ((rng() & 1) ? nan : -inf); break;
            case 11: bad.floor = (rng() & 1) ? 0.0f : ((rng() & 1) ? nan : inf); break;
            case 12: bad.floor = -(float)(1 + rng() % 100); break;
            default: bad.reserved[0] = 1 + (int32_t)(rng() % 1000); break;
        }
        CHECK(rt_adaptive::params_error(bad) != nullptr, "a parameter outside its range is refused");
        // ---- the entry points' refusals, through the C ABI -----------------------------------------------------------------------
        cam.width = 16; cam.height = 16;
        ctx.err.clear();
        rt_adaptive_stats stats;
        std::memset(&stats, 0, sizeof stats);
        // a null context first, whatever else is wrong
        CHECK(rt_render_budget_device(nullptr, &scene, &cam, &rs, 0, nullptr, budget, count, frame, nullptr) == RT_ERR_INVALID, "null context, budget device form");
        CHECK(rt_render_budget(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "null context, budget host form");
        CHECK(rt_adaptive_plan_device(nullptr, 16, 16, frame, frame, count, &good, budget, tile_plane, count, nullptr) == RT_ERR_INVALID, "null context, plan");
        CHECK(rt_render_adaptive(nullptr, &scene, &cam, &rs, 0, &good, frame, count, &stats, nullptr) == RT_ERR_INVALID, "null context, driver");
        CHECK(rt_render_adaptive_host(nullptr, &scene, &cam, &rs, 0, &good, frame, count, &stats) == RT_ERR_INVALID, "null context, driver host form");
        // a scene of another context, a null required pointer (the count plane is optional)
        CHECK(rt_render_budget_device(&ctx, &foreign, &cam, &rs, 0, nullptr, budget, count, frame, nullptr) == RT_ERR_INVALID && said(ctx, "another context"), "foreign scene, budget");
        CHECK(rt_render_adaptive(&ctx, &foreign, &cam, &rs, 0, &good, frame, count, &stats, nullptr) == RT_ERR_INVALID && said(ctx, "another context"), "foreign scene, driver");
        {
            const int which = (int)(rng() % 5);
            CHECK(rt_render_budget_device(&ctx, which == 0 ? nullptr : &scene, which == 1 ? nullptr : &cam, which == 2 ? nullptr : &rs, 0, nullptr, which == 3 ? nullptr : budget,
                                          nullptr, which == 4 ? nullptr : frame, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, budget device form");
            CHECK(rt_render_budget(&ctx, which == 0 ? nullptr : &scene, which == 1 ? nullptr : &cam, which == 2 ? nullptr : &rs, 0, nullptr, which == 3 ? nullptr : budget,
                                   nullptr, which == 4 ? nullptr : frame) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, budget host form");
            CHECK(rt_render_adaptive(&ctx, which == 0 ? nullptr : &scene, which == 1 ? nullptr : &cam, which == 2 ? nullptr : &rs, 0, which == 3 ? nullptr : &good,
                                     which == 4 ? nullptr : frame, nullptr, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, driver");
            CHECK(rt_render_adaptive_host(&ctx, which == 0 ? nullptr : &scene, which == 1 ? nullptr : &cam, which == 2 ? nullptr : &rs, 0, which == 3 ? nullptr : &good,
                                          which == 4 ? nullptr : frame, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, driver host form");
            const int w7 = (int)(rng() % 7);
            CHECK(rt_adaptive_plan_device(&ctx, 16, 16, w7 == 0 ? nullptr : frame, w7 == 1 ? nullptr : frame, w7 == 2 ? nullptr : count, w7 == 3 ? nullptr : &good,
                                          w7 == 4 ? nullptr : budget, w7 == 5 ? nullptr : tile_plane, w7 == 6 ? nullptr : count, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, plan");
        }
        // sizes
        {
            rt_camera c = cam;
            switch (rng() % 4) {
                case 0: c.width = -(int32_t)(rng() % 100); break;
                case 1: c.height = 0; break;
                case 2: c.width = 32769 + (int32_t)(rng() % 1000); break;
                default: c.width = 32768; c.height = 8193 + (int32_t)(rng() % 1000); break;
            }
            CHECK(rt_render_budget_device(&ctx, &scene, &c, &rs, 0, nullptr, budget, count, frame, nullptr) == RT_ERR_INVALID && said(ctx, "image size"), "bad image size, budget");
            CHECK(rt_render_adaptive(&ctx, &scene, &c, &rs, 0, &good, frame, count, &stats, nullptr) == RT_ERR_INVALID && said(ctx, "image size"), "bad image size, driver");
            CHECK(rt_adaptive_plan_device(&ctx, c.width, c.height, frame, frame, count, &good, budget, tile_plane, count, nullptr) == RT_ERR_INVALID && said(ctx, "image size"), "bad image size, plan");
        }
        // render settings
        {
            rt_render_settings r = rs;
            r.reflection_limit = -1 - (int32_t)(rng() % 100);
            CHECK(rt_render_budget_device(&ctx, &scene, &cam, &r, 0, nullptr, budget, count, frame, nullptr) == RT_ERR_INVALID && said(ctx, "render settings"), "negative bounce limit");
        }
        // tile specs: bands, compact, costs, a bad count, an index outside the image, a tile listed twice (the image is 2 x 2 tiles)
        {
            uint32_t list[4] = {0, 1, 2, 3}, cost[4] = {1, 1, 1, 1};
            std::shuffle(list, list + 4, rng);
            rt_tile_spec t;
            std::memset(&t, 0, sizeof t);
            t.band_rows = 8; t.band_stride = 1; t.tile_list = list; t.num_tiles = (int32_t)(rng() % 5);
            const char *msg = "";
            switch (rng() % 7) {
                case 0: t.tile_list = nullptr; msg = "not bands"; break;
                case 1: t.compact = 1; msg = "compact"; break;
                case 2: t.tile_cost = cost; msg = "tile_cost"; break;
                case 3: t.tile_peak = cost; msg = "tile_cost"; break;
                case 4: t.num_tiles = (rng() & 1) ? -1 - (int32_t)(rng() % 10) : 5 + (int32_t)(rng() % 10); msg = "num_tiles"; break;
                case 5: t.num_tiles = 4; list[rng() % 4] = 4 + rng() % 1000; msg = "outside the image"; break;
                default: t.num_tiles = 4; list[0] = list[3]; msg = "listed twice"; break;
            }
            CHECK(rt_render_budget_device(&ctx, &scene, &cam, &rs, 0, &t, budget, count, frame, nullptr) == RT_ERR_INVALID && said(ctx, msg), "bad tile spec, device form");
            CHECK(rt_render_budget(&ctx, &scene, &cam, &rs, 0, &t, budget, count, frame) == RT_ERR_INVALID && said(ctx, msg), "bad tile spec, host form");
        }
        // parameters, through the plan and the driver
        CHECK(rt_adaptive_plan_device(&ctx, 16, 16, frame, frame, count, &bad, budget, tile_plane, count, nullptr) == RT_ERR_INVALID && said(ctx, "adaptive parameters"), "bad parameters, plan");
        CHECK(rt_render_adaptive(&ctx, &scene, &cam, &rs, 0, &bad, frame, count, &stats, nullptr) == RT_ERR_INVALID && said(ctx, "adaptive parameters"), "bad parameters, driver");
        CHECK(rt_render_adaptive_host(&ctx, &scene, &cam, &rs, 0, &bad, frame, count, &stats) == RT_ERR_INVALID && said(ctx, "adaptive parameters"), "bad parameters, driver host form");
        CHECK(g_launches == 0 && stats.passes == 0 && stats.total_samples == 0, "a refused call reached a launcher or wrote its stats");
    }
    std::printf("adaptive host side: %d iterations, sanitizers silent\n", iterations);
    return 0;
}
