/*
 * example_nearest.cpp — the nearest-surface queries of raytracer.hpp: a slice of the monkey's unsigned distance field written as a binary
 * PGM (8-bit, on the surface = white, `reach` away or farther = black), and one point probed on its own.
 *
 *   example_nearest <models_dir> <width> <height> <out.pgm>
 *
 * The scene is the monkey alone (low_poly_monkey.obj as monkey_test_scene places it); the slice is the plane z = 1.6 through it, x and y
 * from -0.6 to 0.6.  Prints, each on a line of its own:
 *   probe: object <index> triangle <index> distance <%.9g> point <x y z>       (the point (0.1, 0.4, 1.6), above the monkey)
 *   slice: <pixels> points, nearest <distance> farthest <distance>, <n> within <reach>
 *
 * Build:  g++ -std=c++17 -O2 example_nearest.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <out.pgm>\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const float reach = 0.3f;
    try {
        if (W < 2 || H < 2) throw std::invalid_argument("the slice needs at least 2 x 2 points");
        SceneObjects objs;
        ObjFileMesh m(std::string(argv[1]) + "/low_poly_monkey.obj");
        m.enlarge(0.3f);
        m.rotate(0, 2.3f, 0);
        m.translate(0.1f, -0.1f, 1.6f);
        objs.create_mesh(m, Material::create_standard(Texture::create_const_colour(Vec3(1, 1, 1)), 0));
        Renderer renderer(0);
        renderer.set_scene(objs);
        const rt_nearest probe = renderer.nearest_point(Vec3(0.1f, 0.4f, 1.6f));
        std::printf("probe: object %d triangle %d distance %.9g point %.9g %.9g %.9g\n", probe.object, probe.triangle, probe.distance, probe.point[0], probe.point[1],
                    probe.point[2]);
        std::vector<float> points((size_t)W * (size_t)H * 3);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                float *p = &points[((size_t)y * (size_t)W + (size_t)x) * 3];
                p[0] = -0.6f + 1.2f * (float)x / (float)(W - 1);
                p[1] = 0.6f - 1.2f * (float)y / (float)(H - 1);
                p[2] = 1.6f;
            }
        const std::vector<rt_nearest> field = renderer.nearest_points(points);
        float nearest = RT_HIT_MISS_T, farthest = 0;
        size_t within = 0;
        for (const rt_nearest &r : field) {
            if (r.object < 0) throw std::runtime_error("an unbounded query of a scene with a mesh missed");
            if (r.distance < nearest) nearest = r.distance;
            if (r.distance > farthest) farthest = r.distance;
            within += r.distance <= reach;
        }
        std::printf("slice: %zu points, nearest %.9g farthest %.9g, %zu within %.9g\n", field.size(), nearest, farthest, within, reach);
        /* the same points under a limit: beyond it a miss, within it the same record */
        const std::vector<rt_nearest> limited = renderer.nearest_points(points, std::vector<float>(field.size(), reach));
        for (size_t i = 0; i < field.size(); i++)
            if ((limited[i].object >= 0) != (field[i].distance2 <= reach * reach) || (limited[i].object >= 0 && limited[i].distance != field[i].distance))
                throw std::runtime_error("the limited and the unbounded query disagree");
        FILE *fp = std::fopen(argv[4], "wb");
        if (!fp) throw std::runtime_error("cannot open output file");
        std::fprintf(fp, "P5\n%d %d\n255\n", W, H);
        for (const rt_nearest &r : field) {
            const int g = (int)(255.0f * (1.0f - r.distance / reach));
            std::fputc(g < 0 ? 0 : (g > 255 ? 255 : g), fp);
        }
        std::fclose(fp);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
