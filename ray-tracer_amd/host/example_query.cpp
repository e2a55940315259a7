/*
 * example_query.cpp — the two query capabilities of raytracer.hpp: what does the centre pixel of a view see, and the view's
 * first-hit depth plane written as a binary PGM (8-bit, nearest = white, a miss = black).
 *
 *   example_query <models_dir> <scene 0..3> <width> <height> <out.pgm>
 *
 * Prints, each on a line of its own:
 *   centre ray: object <index> triangle <index> t <distance, %.9g> point <x y z> normal <x y z>
 *   probe: object <index> t <distance>          (one ray traced on its own, straight ahead from the origin; the same hit)
 *   planes: <hits> of <pixels> pixels hit, nearest <t> farthest <t>
 *   line of sight: whole <0|1> half <0|1>       (is the segment from the origin to (0, 0, 2), and its first half, blocked?)
 *   shadow mask: blocked <n> lit <n> no surface <n>      (the view's visibility plane for a point light at (0, 0.3, 1.7))
 *
 * Build:  g++ -std=c++17 -O2 example_query.cpp -L.. -lraytracer_amd -Wl,-rpath,'$ORIGIN/..'
 */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace rtamd;

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <models_dir> <scene 0..3> <width> <height> <out.pgm>\n", argv[0]);
        return 2;
    }
    const int scene_num = std::atoi(argv[2]), W = std::atoi(argv[3]), H = std::atoi(argv[4]);
    try {
        SceneObjects mesh_data(scene_num, argv[1]);
        Camera camera(W, H);
        Renderer renderer(0);
        renderer.set_scene(mesh_data);
        Renderer::Aov aov = renderer.render_aov(camera, mesh_data.use_sky ? Vec3(0.8f, 1, 1) : Vec3(0, 0, 0));
        /* the centre pixel's primary ray, traced again as a query */
        const size_t c = (size_t)(H / 2) * (size_t)W + (size_t)(W / 2);
        const Vec3 o(camera.c.cam_pos[0], camera.c.cam_pos[1], camera.c.cam_pos[2]), d(aov.ray[3 * c], aov.ray[3 * c + 1], aov.ray[3 * c + 2]);
        const rt_hit h = renderer.trace_ray(o, d);
        std::printf("centre ray: object %d triangle %d t %.9g point %.9g %.9g %.9g normal %.9g %.9g %.9g\n", h.object, h.triangle, h.t, h.point[0], h.point[1],
                    h.point[2], h.normal[0], h.normal[1], h.normal[2]);
        if (h.object != aov.object[c] || h.t != aov.depth[c]) throw std::runtime_error("the query and the planes disagree on the centre pixel");
        const rt_hit probe = renderer.trace_rays({0, 0, 0}, {0, 0, 2})[0];       /* (length 2: t comes out halved) */
        std::printf("probe: object %d t %.9g\n", probe.object, probe.t);
        size_t hits = 0;
        float nearest = RT_HIT_MISS_T, farthest = 0;
        for (size_t i = 0; i < aov.depth.size(); i++) {
            if (aov.object[i] < 0) continue;
            hits++;
            if (aov.depth[i] < nearest) nearest = aov.depth[i];
            if (aov.depth[i] > farthest) farthest = aov.depth[i];
        }
        std::printf("planes: %zu of %zu pixels hit, nearest %.9g farthest %.9g\n", hits, aov.depth.size(), nearest, farthest);
        /* occlusion queries: the direction is the segment itself, so the limit is a fraction of it */
        std::printf("line of sight: whole %d half %d\n", (int)renderer.occluded(Vec3(0, 0, 0), Vec3(0, 0, 2), 1.0f), (int)renderer.occluded(Vec3(0, 0, 0), Vec3(0, 0, 2), 0.5f));
        const std::vector<uint8_t> mask = renderer.render_visibility(camera, Vec3(0.0f, 0.3f, 1.7f), 1e-3f);
        size_t codes[3] = {0, 0, 0};
        for (uint8_t b : mask) codes[b]++;
        std::printf("shadow mask: blocked %zu lit %zu no surface %zu\n", codes[RT_VIS_BLOCKED], codes[RT_VIS_LIT], codes[RT_VIS_NO_SURFACE]);
        FILE *fp = std::fopen(argv[5], "wb");
        if (!fp) throw std::runtime_error("cannot open output file");
        std::fprintf(fp, "P5\n%d %d\n255\n", W, H);
        for (size_t i = 0; i < aov.depth.size(); i++) {
            int g = 0;
            if (aov.object[i] >= 0 && farthest > nearest) g = (int)(255.0f * (farthest - aov.depth[i]) / (farthest - nearest));
            else if (aov.object[i] >= 0) g = 255;
            std::fputc(g < 0 ? 0 : (g > 255 ? 255 : g), fp);
        }
        std::fclose(fp);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
