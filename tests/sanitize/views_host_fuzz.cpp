// The host side of the camera sequences (rt_views_capi.cpp, rt_views.h, rt_sched::views_job_order) under AddressSanitizer +
// UndefinedBehaviorSanitizer (CPU only; test infrastructure): the launch schedule on randomised scenes and cameras - a permutation of all
// (tile, view) jobs, heavy jobs round-robin over the views ahead of the light ones; one tile, one view, no mesh -, the chunking of the host
// form, rt_camera_lens against a plain restatement and its refusals, and every refusal of the entry points through the C ABI on a context
// built in host memory (no GPU is opened: nothing here gets as far as a HIP call).  Kernel launchers are stubs that fail the run if they
// are reached.
//   views_host_fuzz <seed> <iterations>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "rt_views.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                        \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "views fuzz: %s (iteration %d)\n", what, it); return 1; } \
    } while (0)

static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

static float uniform(std::mt19937 &rng, float lo, float hi) { return lo + (hi - lo) * (float)(rng() % 100001) / 100000.0f; }

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
    rt_render_settings rs{4, 8, 1, {1.0f, 1.0f, 1.0f}};
    std::vector<float> frames(40 * 16 * 16 * 3, 7.0f);
    for (int it = 0; it < iterations; it++) {
        // ---- the schedule of a launch --------------------------------------------------------------------------------------------
        {
            const int kind = (int)(rng() % 6);
            const int W = kind == 0 ? 1 + (int)(rng() % 8) : 1 + (int)(rng() % 90), H = kind == 0 ? 1 + (int)(rng() % 8) : 1 + (int)(rng() % 60);   // kind 0: one tile
            const int tiles_x = (W + 7) / 8, n_tiles = tiles_x * ((H + 7) / 8);
            const uint32_t n_views = kind == 1 ? 1u : 1u + rng() % RT_VIEWS_MAX;
            std::vector<rt_object> objects(rng() % 4);
            for (rt_object &ob : objects) {
                std::memset(&ob, 0, sizeof ob);
                ob.type = kind == 2 ? RT_OBJ_SPHERE : (rng() % 3 ? RT_OBJ_MESH : RT_OBJ_SPHERE);       // kind 2: no mesh
                for (int k = 0; k < 3; k++) { ob.v[k] = uniform(rng, -2.0f, 1.0f); ob.v[3 + k] = ob.v[k] + uniform(rng, 0.0f, 2.0f); }
                if (rng() % 8 == 0) ob.v[3] = ob.v[0];                                                 // a flat box
            }
            std::vector<float> cams(12 * (size_t)n_views);
            for (uint32_t v = 0; v < n_views; v++) {
                float *c = cams.data() + 12 * (size_t)v;
                for (int k = 0; k < 3; k++) c[k] = uniform(rng, -3.0f, 3.0f);
                for (int k = 0; k < 3; k++) c[3 + k] = c[k] + uniform(rng, -0.2f, 0.2f);
                for (int k = 0; k < 6; k++) c[6 + k] = rng() % 5 ? uniform(rng, -0.01f, 0.01f) : 0.0f;   // (zero components: a division by zero in the slab test)
                if (rng() % 50 == 0) c[rng() % 12] = rng() & 1 ? nan : inf;
            }
            std::vector<uint32_t> jobs(5, 99u);                                                        // (old content goes)
            rt_sched::views_job_order((uint32_t)n_tiles, tiles_x, cams.data(), n_views, objects, jobs);
            CHECK(jobs.size() == (size_t)n_tiles * n_views, "one job per (tile, view) pair");
            std::vector<char> seen(jobs.size(), 0);
            bool light_begun = false;
            uint32_t last_light_view = 0;
            std::vector<uint32_t> heavy_seen(n_views, 0u);
            for (uint32_t job : jobs) {
                const uint32_t t = job & RT_JOB_TILE_MASK, v = job >> RT_JOB_FRAME_SHIFT;
                CHECK(t < (uint32_t)n_tiles && v < n_views, "a job names a tile of the image and a view of the launch");
                CHECK(!seen[(size_t)v * n_tiles + t], "a (tile, view) pair appears once");
                seen[(size_t)v * n_tiles + t] = 1;
                const bool heavy = rt_sched::centre_ray_enters_mesh(t, tiles_x, cams.data() + 12 * (size_t)v, objects);
                CHECK(kind != 2 || !heavy, "without a mesh every job is light");
                if (heavy) {
                    CHECK(!light_begun, "every heavy job precedes the light ones");
                    heavy_seen[v]++;
                    // round-robin: a view is never more than one heavy job ahead of a lower-numbered view that still has some
                } else {
                    CHECK(!light_begun || v >= last_light_view, "the light jobs come view by view");
                    light_begun = true;
                    last_light_view = v;
                }
            }
            // the guessed one-view order classes by the same test: its heavy class is the schedule's for that view
            std::vector<uint32_t> tiles((size_t)n_tiles);
            for (int t = 0; t < n_tiles; t++) tiles[(size_t)t] = (uint32_t)t;
            const uint32_t v0 = rng() % n_views;
            const std::vector<uint32_t> order = rt_sched::guessed_order(tiles, tiles_x, cams.data() + 12 * (size_t)v0, objects);
            std::vector<uint32_t> mine;
            for (uint32_t job : jobs) if ((job >> RT_JOB_FRAME_SHIFT) == v0) mine.push_back(job & RT_JOB_TILE_MASK);
            CHECK(mine == order, "a view's jobs, in the schedule's order, are its guessed one-view order");
            // round-robin over the views: among the first k * n_views heavy jobs no view has more than k
            size_t total_heavy = 0;
            for (uint32_t h : heavy_seen) total_heavy += h;
            std::vector<uint32_t> upto(n_views, 0u);
            for (size_t i = 0; i < total_heavy; i++) {
                const uint32_t v = jobs[i] >> RT_JOB_FRAME_SHIFT;
                upto[v]++;
                uint32_t least_open = ~0u;
                for (uint32_t u = 0; u < n_views; u++) if (upto[u] < heavy_seen[u]) least_open = std::min(least_open, upto[u]);
                CHECK(least_open == ~0u || upto[v] <= least_open + 1u, "heavy jobs go round-robin over the views");
            }
        }
        // ---- the host form's chunks ----------------------------------------------------------------------------------------------
        {
            const int32_t n = 1 + (int32_t)(rng() % 200), accumulate = (int32_t)(rng() & 1), batch = (int32_t)(rng() % 40) - 2;
            const int32_t cap = rt_views::launch_cap(accumulate, batch);
            CHECK(cap >= 1 && cap <= RT_VIEWS_MAX && (accumulate ? cap == std::max(1, std::min(batch, RT_VIEWS_MAX)) : cap == RT_VIEWS_MAX), "the launch's limit");
            int32_t done = 0, launches = 0;
            while (done < n) {
                const int32_t k = rt_views::next_chunk(n, done, cap);
                CHECK(k >= 1 && k <= cap && done + k <= n && (k == cap || done + k == n), "a chunk is full or the last");
                done += k;
                launches++;
            }
            CHECK(done == n && launches == (n + cap - 1) / cap, "the chunks cover the views in the fewest launches");
        }
        // ---- rt_camera_lens --------------------------------------------------------------------------------------------------------
        rt_camera cam;
        {
            const float pos[3] = {uniform(rng, -3.0f, 3.0f), uniform(rng, -3.0f, 3.0f), uniform(rng, -3.0f, 3.0f)};
            const float focal = uniform(rng, 0.05f, 2.0f), dist = uniform(rng, 0.05f, 50.0f), lu = uniform(rng, -0.5f, 0.5f), lv = uniform(rng, -0.5f, 0.5f);
            rt_camera_make(16, 16, pos, uniform(rng, 0.3f, 2.0f), focal, uniform(rng, -3.0f, 3.0f), uniform(rng, -3.0f, 3.0f), uniform(rng, -3.0f, 3.0f), &cam);
            rt_camera out, centre;
            std::memset(&out, 0x5A, sizeof out);
            CHECK(rt_camera_lens(&cam, focal, dist, lu, lv, &out) == RT_OK && rt_camera_lens(&cam, focal, dist, 0.0f, 0.0f, &centre) == RT_OK, "a lens sample");
            CHECK(out.width == 16 && out.height == 16, "the image size is copied");
            CHECK(!std::memcmp(out.tl_pixel_pos, centre.tl_pixel_pos, 12) && !std::memcmp(out.delta_u, centre.delta_u, 12) && !std::memcmp(out.delta_v, centre.delta_v, 12),
                  "the image plane does not depend on the offset");
            const volatile float s = dist / focal;
            for (int k = 0; k < 3; k++) {
                const volatile float du = cam.delta_u[k] * s, arm = (cam.tl_pixel_pos[k] - cam.cam_pos[k]) * s, tl = arm + cam.cam_pos[k];
                CHECK(out.delta_u[k] == du && out.tl_pixel_pos[k] == tl, "the scaled image plane, operation by operation");
            }
            rt_camera alias = cam;
            CHECK(rt_camera_lens(&alias, focal, dist, lu, lv, &alias) == RT_OK && !std::memcmp(&alias, &out, sizeof out), "out may be cam");
            // refusals leave `out` alone
            rt_camera keep = out, flat = cam;
            std::memset(rng() & 1 ? flat.delta_u : flat.delta_v, 0, 12);
            const float bad_pos[] = {0.0f, -focal, inf, nan}, bad_off[] = {inf, -inf, nan};
            const float b = bad_pos[rng() % 4], o = bad_off[rng() % 3];
            CHECK(rt_camera_lens(nullptr, focal, dist, lu, lv, &out) == RT_ERR_INVALID && rt_camera_lens(&cam, focal, dist, lu, lv, nullptr) == RT_ERR_INVALID, "lens: null pointer");
            CHECK(rt_camera_lens(&cam, b, dist, lu, lv, &out) == RT_ERR_INVALID && rt_camera_lens(&cam, focal, b, lu, lv, &out) == RT_ERR_INVALID, "lens: focal_len / focus_dist");
            CHECK(rt_camera_lens(&cam, focal, dist, o, lv, &out) == RT_ERR_INVALID && rt_camera_lens(&cam, focal, dist, lu, o, &out) == RT_ERR_INVALID, "lens: offset");
            CHECK(rt_camera_lens(&flat, focal, dist, lu, lv, &out) == RT_ERR_INVALID, "lens: a pixel step of length 0");
            CHECK(!std::memcmp(&keep, &out, sizeof out), "a refused lens call leaves out untouched");
        }
        // ---- the entry points' refusals, through the C ABI -----------------------------------------------------------------------
        {
            const int32_t n = 1 + (int32_t)(rng() % RT_VIEWS_MAX);
            std::vector<rt_camera> cams((size_t)n, cam);
            std::vector<int32_t> times((size_t)n, 5);
            int32_t fn = 0;
            const int32_t acc = (int32_t)(rng() & 1);
            ctx.err.clear();
            // a null context first, whatever else is wrong
            CHECK(rt_render_views_device(nullptr, &scene, cams.data(), times.data(), n, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID, "null context, device form");
            CHECK(rt_render_views(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == RT_ERR_INVALID, "null context, host form");
            CHECK(rt_render_views_device(&ctx, &foreign, cams.data(), times.data(), n, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "another context"), "foreign scene, device form");
            CHECK(rt_render_views(&ctx, &foreign, cams.data(), times.data(), n, &rs, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "another context"), "foreign scene, host form");
            const int which = (int)(rng() % 5);
            CHECK(rt_render_views_device(&ctx, which == 0 ? nullptr : &scene, which == 1 ? nullptr : cams.data(), which == 2 ? nullptr : times.data(), n, which == 3 ? nullptr : &rs, acc, 0,
                                         which == 4 ? nullptr : frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, device form");
            CHECK(rt_render_views(&ctx, which == 0 ? nullptr : &scene, which == 1 ? nullptr : cams.data(), which == 2 ? nullptr : times.data(), n, which == 3 ? nullptr : &rs, acc, &fn,
                                  which == 4 ? nullptr : frames.data()) == RT_ERR_INVALID && said(ctx, "null argument"), "null pointer, host form");
            CHECK(rt_render_views(&ctx, &scene, cams.data(), times.data(), n, &rs, acc, nullptr, frames.data()) == RT_ERR_INVALID && said(ctx, "null argument"), "null frame_num, host form");
            // the number of views
            const int32_t few = -(int32_t)(rng() % 3), many = RT_VIEWS_MAX + 1 + (int32_t)(rng() % 100);
            CHECK(rt_render_views_device(&ctx, &scene, cams.data(), times.data(), few, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "number of views"), "too few views");
            CHECK(rt_render_views_device(&ctx, &scene, cams.data(), times.data(), many, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "number of views"), "too many views");
            CHECK(rt_render_views(&ctx, &scene, cams.data(), times.data(), few, &rs, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "number of views"), "too few views, host form");
            // frame numbers
            const int32_t negative = -1 - (int32_t)(rng() % 100), positive = 1 + (int32_t)(rng() % 100);
            CHECK(rt_render_views_device(&ctx, &scene, cams.data(), times.data(), n, &rs, acc, negative, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "frame number"), "negative frame number");
            CHECK(rt_render_views_device(&ctx, &scene, cams.data(), times.data(), n, &rs, 0, positive, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "frame number"), "a frame number without accumulate");
            CHECK(rt_render_views_device(&ctx, &scene, cams.data(), times.data(), n, &rs, 1, std::numeric_limits<int32_t>::max() - n + 1, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "frame number"),
                  "a frame number that would overflow");
            int32_t fnb = rng() & 1 ? negative : positive;
            const int32_t fnb0 = fnb;
            CHECK(rt_render_views(&ctx, &scene, cams.data(), times.data(), n, &rs, fnb < 0 ? acc : 0, &fnb, frames.data()) == RT_ERR_INVALID && said(ctx, "frame number") && fnb == fnb0, "bad frame number, host form");
            // render settings, image sizes, cameras that differ in size
            rt_render_settings r = rs;
            (rng() & 1 ? r.reflection_limit : r.rays_per_pixel) = -1 - (int32_t)(rng() % 100);
            CHECK(rt_render_views_device(&ctx, &scene, cams.data(), times.data(), n, &r, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "render settings"), "negative settings");
            CHECK(rt_render_views(&ctx, &scene, cams.data(), times.data(), n, &r, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "render settings"), "negative settings, host form");
            std::vector<rt_camera> sized = cams;
            switch (rng() % 4) {
                case 0: sized[0].width = -(int32_t)(rng() % 100); break;
                case 1: sized[0].height = 0; break;
                case 2: sized[0].width = 32769 + (int32_t)(rng() % 1000); break;
                default: sized[0].width = 32768; sized[0].height = 8193 + (int32_t)(rng() % 1000); break;
            }
            CHECK(rt_render_views_device(&ctx, &scene, sized.data(), times.data(), n, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "image size"), "bad image size");
            CHECK(rt_render_views(&ctx, &scene, sized.data(), times.data(), n, &rs, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "image size"), "bad image size, host form");
            if (n > 1) {
                std::vector<rt_camera> mixed = cams;
                rt_camera &m = mixed[1 + rng() % (size_t)(n - 1)];
                (rng() & 1 ? m.width : m.height) += rng() & 1 ? 1 : -1;
                CHECK(rt_render_views_device(&ctx, &scene, mixed.data(), times.data(), n, &rs, acc, 0, frames.data(), nullptr) == RT_ERR_INVALID && said(ctx, "share one image size"), "cameras of two sizes");
                CHECK(rt_render_views(&ctx, &scene, mixed.data(), times.data(), n, &rs, acc, &fn, frames.data()) == RT_ERR_INVALID && said(ctx, "share one image size"), "cameras of two sizes, host form");
            }
            CHECK(g_launches == 0 && fn == 0, "a refused call reached a launcher or moved the frame number");
        }
    }
    for (float f : frames)
        if (f != 7.0f) { std::fprintf(stderr, "views fuzz: a refused call wrote the frames\n"); return 1; }
    std::printf("views host side: %d iterations, sanitizers silent\n", iterations);
    return 0;
}
