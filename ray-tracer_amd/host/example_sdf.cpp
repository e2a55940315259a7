/*
 * example_sdf.cpp — the winding-number queries of raytracer.hpp: a slice of the monkey's SIGNED distance field written as a binary PGM
 * (8-bit: mid grey on the surface, darker inside, lighter outside, saturating `reach` away), and one point probed on its own.
 *
 *   example_sdf <models_dir> <width> <height> <out.pgm> [beta]
 *
 * With a beta the slice is answered a second time by the fast winding numbers (Renderer::signed_distance_fast, the dipole cluster tree) and
 * a third line says how many of its signs differ from the exact ones; without it nothing of that runs and the output is as it always was.
 *
 * The scene is the monkey alone (low_poly_monkey.obj as monkey_test_scene places it); the slice is the plane z = 1.6 through it, x and y
 * from -0.6 to 0.6.  Prints, each on a line of its own:
 *   probe: winding <%.9g> inside <0|1> sdf <%.9g>                     (the point (0.1, -0.1, 1.6), the middle of the head)
 *   slice: <pixels> points, <n> inside, sdf from <lowest> to <highest>
 *
 * Build:  g++ -std=c++17 -O2 example_sdf.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
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
        std::fprintf(stderr, "usage: %s <models_dir> <width> <height> <out.pgm> [beta]\n", argv[0]);
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
        const std::vector<float> probe = {0.1f, -0.1f, 1.6f};
        std::printf("probe: winding %.9g inside %d sdf %.9g\n", renderer.winding_numbers(probe)[0], (int)renderer.contains(probe)[0], renderer.signed_distance(probe)[0]);
        std::vector<float> points((size_t)W * (size_t)H * 3);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                float *p = &points[((size_t)y * (size_t)W + (size_t)x) * 3];
                p[0] = -0.6f + 1.2f * (float)x / (float)(W - 1);
                p[1] = 0.6f - 1.2f * (float)y / (float)(H - 1);
                p[2] = 1.6f;
            }
        std::vector<rt_nearest> records;
        const std::vector<float> field = renderer.signed_distance(points, {}, &records);
        const std::vector<uint8_t> in = renderer.contains(points);
        float lowest = RT_HIT_MISS_T, highest = -RT_HIT_MISS_T;
        size_t inside = 0;
        for (size_t i = 0; i < field.size(); i++) {
            if ((field[i] < 0) != (in[i] != 0) || (field[i] < 0 ? -field[i] : field[i]) != records[i].distance)
                throw std::runtime_error("the signed distance, the containment byte and the nearest-surface record disagree");
            if (field[i] < lowest) lowest = field[i];
            if (field[i] > highest) highest = field[i];
            inside += field[i] < 0;
        }
        std::printf("slice: %zu points, %zu inside, sdf from %.9g to %.9g\n", field.size(), inside, lowest, highest);
        if (argc > 5) {
            const float beta = (float)std::atof(argv[5]);
            const std::vector<float> fast = renderer.signed_distance_fast(points, beta);
            size_t differ = 0;
            for (size_t i = 0; i < field.size(); i++) differ += (fast[i] < 0) != (field[i] < 0);
            std::printf("fast: beta %.9g, %zu of %zu signs differ from the exact ones\n", beta, differ, field.size());
        }
        FILE *fp = std::fopen(argv[4], "wb");
        if (!fp) throw std::runtime_error("cannot open output file");
        std::fprintf(fp, "P5\n%d %d\n255\n", W, H);
        for (float d : field) {
            const int g = (int)(127.5f * (1.0f + d / reach));
            std::fputc(g < 0 ? 0 : (g > 255 ? 255 : g), fp);
        }
        std::fclose(fp);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
