/*
 * example_adaptive.cpp — per-pixel sample budgets and the adaptive loop of raytracer.hpp: the reference's monkey_test_scene (scene 0: the
 * monkey and a sphere in a Cornell box, no sky; src/main.cu:150-170) sampled to a noise target, written as two pictures: the frame, and
 * the map of where the samples went (white: the most any pixel got).
 *
 *   example_adaptive <models_dir> <width> <height> <out prefix>      ->  <prefix>.png, <prefix>_samples.png
 *
 * It first checks the budget render against the renderer itself - a uniform budget of 3 from nothing is render() at 3 samples per pixel,
 * bit for bit, and a second call doubles every count - then runs the loop and prints
 *   adaptive ok: <W> x <H>, <passes> passes, <total> samples (<mean> per pixel, <min> .. <max>), tiles per pass: ...
 *
 * Build:  g++ -std=c++17 -O2 example_adaptive.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <out prefix>\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const size_t px = (size_t)W * (size_t)H;
    try {
        SceneObjects mesh_data(0, argv[1]);
        const Vec3 sky = mesh_data.use_sky ? Vec3(0.8f, 1, 1) : Vec3(0, 0, 0);
        Camera camera(W, H);
        Renderer renderer(0);
        renderer.set_scene(mesh_data);
        /* the budget render against render() */
        RenderData three(3, 5, true, sky);
        VariableRenderData data{0, std::vector<float>(px * 3, 0.0f)};
        renderer.render(camera, three, &data, 12345);
        Renderer::Accumulation acc(camera);
        const std::vector<uint16_t> budget(px, 3);
        renderer.render_budget(camera, three, budget, &acc, 12345);
        if (std::memcmp(acc.frame.data(), data.previous_render.data(), px * 12) != 0) throw std::runtime_error("a uniform budget differs from render()");
        renderer.render_budget(camera, three, budget, &acc, 12346);
        if (std::count(acc.count.begin(), acc.count.end(), 6u) != (long)px) throw std::runtime_error("the counts are not the budgets' sum");
        /* the loop */
        rt_adaptive_params params = Renderer::adaptive_defaults();
        params.max_spp = 128;
        const Renderer::Adaptive a = renderer.render_adaptive(camera, three, 12345, params);
        unsigned long long total = 0;
        uint32_t lo = ~0u, hi = 0;
        for (uint32_t c : a.count) { total += c; lo = std::min(lo, c); hi = std::max(hi, c); }
        if (total != a.stats.total_samples || lo < 2u * (uint32_t)params.pilot_spp || hi > 2u * (uint32_t)params.max_spp) throw std::runtime_error("the counts and the statistics disagree");
        std::printf("adaptive ok: %d x %d, %d passes, %llu samples (%.1f per pixel, %u .. %u), tiles per pass:", W, H, a.stats.passes, total, (double)total / (double)px, lo, hi);
        for (int k = 0; k < a.stats.passes; k++) std::printf(" %d", a.stats.active_tiles[k]);
        std::printf("\n");
        const std::string prefix = argv[4];
        write_png(prefix + ".png", parse_pixel_colours(a.frame, W, H), W, H);
        std::vector<float> map(px * 3);
        for (size_t i = 0; i < px; i++) map[3 * i] = map[3 * i + 1] = map[3 * i + 2] = (float)a.count[i] / (float)hi;
        write_png(prefix + "_samples.png", parse_pixel_colours(map, W, H), W, H);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
