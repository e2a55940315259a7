/*
 * example_denoise.cpp — the denoiser of raytracer.hpp: the reference's monkey_test_scene (scene 0: the monkey and a sphere in a Cornell
 * box, no sky; src/main.cu:150-170) rendered at a few samples per pixel, filtered
 * with the view's first-hit planes, and written as ONE picture, the noisy frame on the left and the denoised one on the right.
 *
 *   example_denoise <models_dir> <width> <height> <samples per pixel> <out.png> [out.f32]
 *
 * Prints  denoised <W> x <H>: <n> pixels changed, filter <ms> ms.  The optional last argument takes the two frames as raw binary32
 * (noisy, then denoised; W*H*3 floats each).
 *
 * Build:  g++ -std=c++17 -O2 example_denoise.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <samples per pixel> <out.png> [out.f32]\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), spp = std::atoi(argv[4]);
    try {
        SceneObjects mesh_data(0, argv[1]);
        const Vec3 sky = mesh_data.use_sky ? Vec3(0.8f, 1, 1) : Vec3(0, 0, 0);
        RenderData render_data(spp, 5, true, sky);
        Camera camera(W, H);
        Renderer renderer(0);
        renderer.set_scene(mesh_data);
        VariableRenderData data{0, std::vector<float>((size_t)W * (size_t)H * 3, 0.0f)};
        renderer.render(camera, render_data, &data, 12345);
        const Renderer::Aov aov = renderer.render_aov(camera, sky);
        const std::vector<float> clean = renderer.denoise(camera, data.previous_render, aov);
        const float ms = renderer.last_kernel_ms();
        size_t changed = 0;
        for (size_t i = 0; i < (size_t)W * (size_t)H; i++) changed += std::memcmp(&clean[3 * i], &data.previous_render[3 * i], 12) != 0;
        std::printf("denoised %d x %d: %zu pixels changed, filter %.3f ms\n", W, H, changed, ms);
        /* side by side */
        std::vector<float> pair((size_t)2 * W * H * 3);
        for (int y = 0; y < H; y++) {
            std::memcpy(&pair[((size_t)y * 2 * W) * 3], &data.previous_render[(size_t)y * W * 3], (size_t)W * 12);
            std::memcpy(&pair[((size_t)y * 2 * W + W) * 3], &clean[(size_t)y * W * 3], (size_t)W * 12);
        }
        write_png(argv[5], parse_pixel_colours(pair, 2 * W, H), 2 * W, H);
        if (argc > 6) {
            FILE *fp = std::fopen(argv[6], "wb");
            if (!fp) throw std::runtime_error("cannot open output file");
            std::fwrite(data.previous_render.data(), 4, data.previous_render.size(), fp);
            std::fwrite(clean.data(), 4, clean.size(), fp);
            std::fclose(fp);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
