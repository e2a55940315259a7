/*
 * example_sky.cpp — environment lighting of raytracer.hpp: the monkey on its ground sphere with no lamp in the scene, lit by a cube-map sky
 * filled from a procedural function of direction - a gradient from a warm horizon to a blue zenith, a dim ground half, a small HDR sun -
 * through Sky::texel_direction.
 *
 *   example_sky <models_dir> <width> <height> <face size> <out prefix>   ->  <prefix>.png, <prefix>_frame.f32, <prefix>_sky.f32
 *
 * The two raw files hold the frame (W*H*3 floats) and the map (6*n*n*3 floats) as they are in memory, for whoever wants to render the same
 * picture through another binding.  It first checks the sky against the renderer itself - a map of all 1.0f renders, bit for bit, what
 * render_views renders under the constant sky - and prints
 *   sky ok: <W> x <H> under a <n>-texel cube map, <ms> ms
 *
 * Build:  g++ -std=c++17 -O2 example_sky.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

/* the light arriving from direction d (any length) */
static Vec3 sky_light(Vec3 d)
{
    const float len = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    const float x = d.x / len, y = d.y / len, z = d.z / len;
    if (y < 0.0f) return Vec3(0.08f, 0.07f, 0.06f);                                    /* below the horizon */
    const float up = std::sqrt(y);                                                     /* 0 at the horizon, 1 at the zenith */
    Vec3 c(1.0f + (0.25f - 1.0f) * up, 0.85f + (0.45f - 0.85f) * up, 0.7f + (1.0f - 0.7f) * up);
    const float sx = 0.45f, sy = 0.65f, sz = -0.6124f;                                 /* the sun: behind the camera, up and to the right */
    if (x * sx + y * sy + z * sz > 0.995f) c = Vec3(60.0f, 55.0f, 45.0f);
    return c;
}

static void write_raw(const std::string &path, const std::vector<float> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) throw std::runtime_error("cannot write " + path);
    std::fclose(f);
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <face size> <out prefix>\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n = std::atoi(argv[4]);
    const std::string prefix = argv[5];
    try {
        if (n < 1 || n > RT_SKY_MAX_FACE) throw std::invalid_argument("a face size of 1 .. 2048");
        SceneObjects objs;
        ObjFileMesh monkey(std::string(argv[1]) + "/low_poly_monkey.obj");
        monkey.enlarge(0.3f);
        monkey.rotate(0, 2.3f, 0);
        monkey.translate(0.1f, -0.1f, 1.6f);
        objs.create_mesh(monkey, Material::create_standard(Texture::create_const_colour(Vec3(0.9f, 0.9f, 0.9f)), 0.2f));
        objs.create_sphere(Vec3(0, -100.5f, 1.5f), 100, Material::create_standard(Texture::create_const_colour(Vec3(0.5f, 0.5f, 0.5f)), 0.3f));
        Renderer renderer(0);
        renderer.set_scene(objs);

        std::vector<float> faces((size_t)6 * n * n * 3);
        for (int face = 0; face < 6; face++)
            for (int row = 0; row < n; row++)
                for (int col = 0; col < n; col++) {
                    const Vec3 c = sky_light(Sky::texel_direction(n, face, row, col));
                    float *texel = faces.data() + (((size_t)face * n + row) * n + col) * 3;
                    texel[0] = c.x; texel[1] = c.y; texel[2] = c.z;
                }
        const std::vector<Camera> cams{Camera(W, H)};
        const std::vector<int> times{12345};
        {
            /* the identity: a white map under a tint is the constant sky of that colour */
            const Sky white = renderer.create_sky(1, std::vector<float>(18, 1.0f));
            const RenderData tinted(4, 5, true, Vec3(0.8f, 1.0f, 1.0f));
            const std::vector<float> a = renderer.render_sky(white, cams, tinted, times), b = renderer.render_views(cams, tinted, times);
            if (a.size() != b.size() || std::memcmp(a.data(), b.data(), a.size() * 4) != 0) throw std::runtime_error("a white map differs from the constant sky");
        }
        const Sky sky = renderer.create_sky(n, faces);
        const RenderData rd(32, 5, true, Vec3(1, 1, 1));
        const std::vector<float> frame = renderer.render_sky(sky, cams, rd, times);
        const float ms = renderer.last_kernel_ms();
        write_png(prefix + ".png", parse_pixel_colours(frame, W, H), W, H);
        write_raw(prefix + "_frame.f32", frame);
        write_raw(prefix + "_sky.f32", faces);
        std::printf("sky ok: %d x %d under a %d-texel cube map, %.3f ms\n", W, H, n, ms);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
