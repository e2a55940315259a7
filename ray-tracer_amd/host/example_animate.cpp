/*
 * example_animate.cpp — time-varying geometry of raytracer.hpp: the monkey scene (the monkey, a light and a ground sphere; the metric scene of
 * bench.py) with the monkey bent a little further at every time step.  The scene is committed once; each step hands the mesh's new vertices to
 * Renderer::update_mesh, which rebuilds its BVH on the GPU, and renders a picture.
 *
 *   example_animate <models_dir> <width> <height> <steps> <out prefix>      ->  <prefix>_000.png ...
 *
 * It first checks the update against the renderer itself - the last step's picture is, bit for bit, the picture of a scene committed with that
 * step's triangles - and prints
 *   animate ok: <steps> steps of <n> triangles, <W> x <H>
 *
 * Build:  g++ -std=c++17 -O2 example_animate.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

/* the monkey bent about the z axis: a point's turn grows with its height above the chin */
static std::vector<float> bent(const std::vector<float> &base, float amount)
{
    std::vector<float> out = base;
    for (size_t i = 0; i + 2 < out.size(); i += 3) {
        const float x = base[i] - 0.1f, y = base[i + 1] + 0.1f, a = amount * (y + 0.3f);
        out[i] = 0.1f + x * std::cos(a) - y * std::sin(a);
        out[i + 1] = -0.1f + x * std::sin(a) + y * std::cos(a);
    }
    return out;
}

static void add_surroundings(SceneObjects &objs)
{
    objs.create_sphere(Vec3(0, 1.2f, 1.2f), 0.5f, Material::create_emissive(Vec3(1, 1, 1), 6));
    objs.create_sphere(Vec3(0, -100.5f, 1.5f), 100, Material::create_standard(Texture::create_const_colour(Vec3(0.5f, 0.5f, 0.5f)), 0.3f));
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <steps> <out prefix>\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), steps = std::atoi(argv[4]);
    const size_t frame = (size_t)W * (size_t)H * 3;
    try {
        if (steps < 1 || steps > 999) throw std::invalid_argument("1 .. 999 steps");
        ObjFileMesh monkey(std::string(argv[1]) + "/low_poly_monkey.obj");
        monkey.enlarge(0.3f);
        monkey.rotate(0, 2.3f, 0);
        monkey.translate(0.1f, -0.1f, 1.6f);
        const std::vector<float> base = monkey.triangles();
        const Material white = Material::create_standard(Texture::create_const_colour(Vec3(1, 1, 1)), 0);
        SceneObjects objs;
        objs.create_mesh(monkey, white);                 /* object 0 */
        add_surroundings(objs);
        Renderer renderer(0);
        renderer.set_scene(objs);
        const Camera cam(W, H);
        const RenderData rd(16, 5, true, Vec3(0, 0, 0));
        std::vector<float> last, now;
        for (int step = 0; step < steps; step++) {
            now = bent(base, 0.6f * std::sin(0.5f * (float)step));
            renderer.update_mesh(0, now);
            VariableRenderData data{0, std::vector<float>(frame, 0.0f)};
            renderer.render(cam, rd, &data, 12345 + step);
            char name[32];
            std::snprintf(name, sizeof name, "_%03d.png", step);
            write_png(std::string(argv[5]) + name, parse_pixel_colours(data.previous_render, W, H), W, H);
            last = data.previous_render;
        }
        /* the last step, committed afresh */
        SceneObjects fresh;
        fresh.create_mesh(now, white);
        add_surroundings(fresh);
        Renderer second(0);
        second.set_scene(fresh);
        VariableRenderData data{0, std::vector<float>(frame, 0.0f)};
        second.render(cam, rd, &data, 12345 + steps - 1);
        if (std::memcmp(data.previous_render.data(), last.data(), frame * 4) != 0) throw std::runtime_error("the updated scene's picture differs from a fresh commit's");
        std::printf("animate ok: %d steps of %d triangles, %d x %d\n", steps, (int)(base.size() / 9), W, H);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
