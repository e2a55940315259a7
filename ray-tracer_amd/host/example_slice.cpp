/*
 * example_slice.cpp — the triangle-overlap queries of raytracer.hpp: a cross-section of the monkey.  A horizontal cutting plane is tiled into
 * 2 * m * m small triangles, every tile is asked which of the monkey's triangles it cuts and along which segment
 * (Renderer::overlap_triangles with k = 8 and segments), and the segments - together the cross-section's outline - are rasterised into a
 * binary PGM (8-bit: the outline white on black).  A tile that cuts more than eight triangles reports its eight lowest: such tiles are
 * counted and printed, and a finer tiling (a larger m) brings their number down.
 *
 *   example_slice <models_dir> <height> <m> <out.pgm>
 *
 * The scene is the monkey alone (low_poly_monkey.obj as monkey_test_scene places it); the plane y = height spans the square of side 1.3
 * centred at x = 0.1, z = 1.6, cut into m x m cells of two triangles each (corners computed in double and rounded once, so that neighbours
 * share their edges exactly).  The image is 256 x 256 over the same square, x to the right, z upwards.  Prints, each on a line of its own:
 *   slice: y = <height>, <n> tiles, <n> cut the mesh, <n> segments, <n> truncated
 *   probe: the triangle (a0, a1, a2) touches: <0 or 1>                                        (Renderer::touches on the first tile)
 *
 * Build:  g++ -std=c++17 -O2 example_slice.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <models_dir> <height> <m> <out.pgm>\n", argv[0]);
        return 2;
    }
    const float height = (float)std::atof(argv[2]);
    const int M = std::atoi(argv[3]), W = 256;
    const double side = 1.3, x0 = 0.1 - side / 2, z0 = 1.6 - side / 2;
    try {
        if (M < 1 || M > 1024) throw std::invalid_argument("m must be 1 .. 1024 cells along an axis");
        SceneObjects objs;
        ObjFileMesh mesh(std::string(argv[1]) + "/low_poly_monkey.obj");
        mesh.enlarge(0.3f);
        mesh.rotate(0, 2.3f, 0);
        mesh.translate(0.1f, -0.1f, 1.6f);
        objs.create_mesh(mesh, Material::create_standard(Texture::create_const_colour(Vec3(1, 1, 1)), 0));
        Renderer renderer(0);
        renderer.set_scene(objs);
        std::vector<float> ex, ez;
        for (int i = 0; i <= M; i++) {
            ex.push_back((float)(x0 + side * (double)i / (double)M));
            ez.push_back((float)(z0 + side * (double)i / (double)M));
        }
        std::vector<float> tiles;
        tiles.reserve((size_t)M * (size_t)M * 18);
        for (int i = 0; i < M; i++)
            for (int j = 0; j < M; j++) {
                const float xa = ex[(size_t)i], xb = ex[(size_t)i + 1], za = ez[(size_t)j], zb = ez[(size_t)j + 1];
                const float two[18] = {xa, height, za, xb, height, za, xb, height, zb, xa, height, za, xb, height, zb, xa, height, zb};
                tiles.insert(tiles.end(), two, two + 18);
            }
        const size_t n = tiles.size() / 9;
        const Renderer::TriangleOverlaps o = renderer.overlap_triangles(tiles, RT_OVERLAP_MAX, true);
        std::vector<unsigned char> image((size_t)W * (size_t)W, 0);
        size_t cutting = 0, segments = 0, truncated = 0;
        for (size_t i = 0; i < n; i++) {
            cutting += o.counts[i] > 0 ? 1 : 0;
            truncated += o.counts[i] > RT_OVERLAP_MAX ? 1 : 0;
            for (int r = 0; r < RT_OVERLAP_MAX; r++) {
                const rt_tri_segment &s = o.segments[i * RT_OVERLAP_MAX + (size_t)r];
                if (s.kind != 1) continue;
                segments++;
                /* the segment, sampled finer than a pixel */
                const double px = (s.p[0] - x0) / side * W, pz = (s.p[2] - z0) / side * W, qx = (s.q[0] - x0) / side * W, qz = (s.q[2] - z0) / side * W;
                const int steps = 1 + (int)(2.0 * std::fmax(std::fabs(qx - px), std::fabs(qz - pz)));
                for (int t = 0; t <= steps; t++) {
                    const int u = (int)std::floor(px + (qx - px) * t / steps), v = (int)std::floor(pz + (qz - pz) * t / steps);
                    if (u >= 0 && u < W && v >= 0 && v < W) image[(size_t)(W - 1 - v) * (size_t)W + (size_t)u] = 255;
                }
            }
        }
        std::printf("slice: y = %g, %zu tiles, %zu cut the mesh, %zu segments, %zu truncated\n", (double)height, n, cutting, segments, truncated);
        const bool first = renderer.touches(Vec3(tiles[0], tiles[1], tiles[2]), Vec3(tiles[3], tiles[4], tiles[5]), Vec3(tiles[6], tiles[7], tiles[8]));
        std::printf("probe: the triangle (%g %g %g, %g %g %g, %g %g %g) touches: %d\n", (double)tiles[0], (double)tiles[1], (double)tiles[2], (double)tiles[3],
                    (double)tiles[4], (double)tiles[5], (double)tiles[6], (double)tiles[7], (double)tiles[8], first ? 1 : 0);
        FILE *fp = std::fopen(argv[4], "wb");
        if (!fp) throw std::runtime_error("cannot open output file");
        std::fprintf(fp, "P5\n%d %d\n255\n", W, W);
        std::fwrite(image.data(), 1, image.size(), fp);
        std::fclose(fp);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
