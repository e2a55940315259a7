/*
 * example_views.cpp — camera sequences of raytracer.hpp: the monkey scene (the monkey, a light and a ground sphere; the metric scene of
 * bench.py) seen from an orbit of cameras, all views rendered by ONE launch and written as numbered pictures, and one depth-of-field frame
 * accumulated from lens samples of the first camera.
 *
 *   example_views <models_dir> <width> <height> <views> <out prefix>      ->  <prefix>_000.png ..., <prefix>_dof.png
 *
 * It first checks the sequence against the renderer itself - every view is render() of its camera from frame 0, bit for bit, and the
 * accumulated frame is that many chained render() calls - and prints
 *   views ok: <n> views of <W> x <H> in one launch, <ms> ms; depth of field from <k> lens samples
 *
 * Build:  g++ -std=c++17 -O2 example_views.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cmath>
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
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <views> <out prefix>\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n = std::atoi(argv[4]);
    const size_t frame = (size_t)W * (size_t)H * 3;
    try {
        if (n < 1 || n > RT_VIEWS_MAX) throw std::invalid_argument("1 .. 32 views");
        /* the monkey scene of the benchmark: src/main.cu:157-160's mesh transform, a light above, a slightly glossy ground */
        SceneObjects objs;
        ObjFileMesh monkey(std::string(argv[1]) + "/low_poly_monkey.obj");
        monkey.enlarge(0.3f);
        monkey.rotate(0, 2.3f, 0);
        monkey.translate(0.1f, -0.1f, 1.6f);
        objs.create_mesh(monkey, Material::create_standard(Texture::create_const_colour(Vec3(1, 1, 1)), 0));
        objs.create_sphere(Vec3(0, 1.2f, 1.2f), 0.5f, Material::create_emissive(Vec3(1, 1, 1), 6));
        objs.create_sphere(Vec3(0, -100.5f, 1.5f), 100, Material::create_standard(Texture::create_const_colour(Vec3(0.5f, 0.5f, 0.5f)), 0.3f));
        Renderer renderer(0);
        renderer.set_scene(objs);
        /* an orbit about the monkey (at z = 1.6), the camera turned to keep facing it */
        const float fov = 60.0f * 3.14159265f / 180.0f, radius = 1.6f;
        std::vector<Camera> orbit;
        std::vector<int> times;
        for (int i = 0; i < n; i++) {
            const float a = (float)i / (float)n * 0.8f - 0.4f;                       /* -0.4 .. 0.4 rad about the vertical axis */
            orbit.push_back(Camera(W, H, Vec3(radius * std::sin(a), 0, 1.6f - radius * std::cos(a)), fov, 0.1f, 0, a, 0));
            times.push_back(12345 + i);
        }
        RenderData rd(16, 5, true, Vec3(0, 0, 0));
        const std::vector<float> frames = renderer.render_views(orbit, rd, times);
        const float ms = renderer.last_kernel_ms();
        for (int i = 0; i < n; i++) {
            VariableRenderData one{0, std::vector<float>(frame, 0.0f)};
            renderer.render(orbit[i], rd, &one, times[i]);
            if (std::memcmp(one.previous_render.data(), frames.data() + (size_t)i * frame, frame * 4) != 0) throw std::runtime_error("a view differs from render() of its camera");
            char name[32];
            std::snprintf(name, sizeof name, "_%03d.png", i);
            write_png(std::string(argv[5]) + name, parse_pixel_colours(one.previous_render, W, H), W, H);
        }
        /* depth of field: lens samples of the first camera focused on the monkey, one progressive frame each, folded in one launch */
        const int k = n < 16 ? n : 16;
        const std::vector<Camera> lens = lens_cameras(orbit[0], 0.1f, radius, 0.03f, k);
        const std::vector<int> lens_times(times.begin(), times.begin() + k);
        VariableRenderData dof{0, std::vector<float>(frame, 0.0f)}, chained{0, std::vector<float>(frame, 0.0f)};
        renderer.render_views(lens, rd, lens_times, true, &dof);
        for (int i = 0; i < k; i++) renderer.render(lens[i], rd, &chained, lens_times[i]);
        if (dof.frame_num != k || std::memcmp(dof.previous_render.data(), chained.previous_render.data(), frame * 4) != 0) throw std::runtime_error("the accumulated frame differs from chained render() calls");
        write_png(std::string(argv[5]) + "_dof.png", parse_pixel_colours(dof.previous_render, W, H), W, H);
        std::printf("views ok: %d views of %d x %d in one launch, %.3f ms; depth of field from %d lens samples\n", n, W, H, ms, k);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
