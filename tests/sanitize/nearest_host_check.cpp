// The nearest-surface queries (rt_nearest_points[_device]: rt_nearest.h, rt_nearest_capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer
// (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. the kernel's traversal as plain host code - the steps of rt_nearest.h (rt_nr_simple, rt_nr_mesh_begin, rt_nr_step, rt_nr_record), the
//      text the kernel compiles, on a stack of exactly the scene's stack_entries - against the EXHAUSTIVE minimum over every candidate (every
//      sphere, every triangle record, a mesh's triangles under the path values of a plain recursion over its whole tree), byte for byte: seeded
//      random and adversarial inputs - points on surfaces, coordinates up to 2^20, coplanar fans, identical triangles, meshes of 1 to 9
//      triangles (every chain shape) and of 1,023 to 1,025, limits around the answer;
//   2. every refusal of both entry points, on a context and scenes built in host memory (nothing gets as far as a HIP call or the launcher).
//   nearest_host_check <seed> <points per scene>
// A second form answers a scene from a file, for tests/test_nearest_host.py to set against the NumPy yardstick:
//   nearest_host_check file <in> <out>   in: int32 blob_f4, off_nodes, off_tris, off_meshes, num_meshes, num_objects, stack_entries, n, has_limit;
//                                            the blob; n x 3 floats; n floats if has_limit.   out: n records
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "rt_nearest.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                             \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "nearest check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_steps = 0, g_skipped_meshes = 0, g_points = 0;

struct Flat {
    const rt_f4 *blob;
    int off_nodes, off_tris, off_meshes, off_objtab, num_meshes, num_objects, stack_entries;
    rt_nr_scene<rt_f4> S() const
    {
        rt_nr_scene<rt_f4> s;
        s.nodes = blob + off_nodes; s.tris = blob + off_tris; s.meshes = blob + off_meshes; s.objtab = blob + off_objtab;
        return s;
    }
};

static Flat flat_of(const rt_flat_view &v)
{
    return Flat{(const rt_f4 *)v.blob, v.off_nodes, v.off_tris, v.off_meshes, v.off_meshes + 2 * v.num_meshes, v.num_meshes, v.num_objects, v.stack_entries};
}

// ---- the kernel's path: one lane, the steps in a plain loop -------------------------------------------------------------------------------
static rt_nearest walk(const Flat &f, const float p[3], bool has_limit, float max_dist)
{
    const rt_nr_scene<rt_f4> S = f.S();
    rt_nearest out;
    rt_nr_best best;
    if (rt_nr_begin(p[0], p[1], p[2], has_limit, max_dist, best)) {
        rt_nr_simple(S, f.num_objects, p[0], p[1], p[2], best);
        std::vector<rt_nr_entry> stack((size_t)f.stack_entries);          // exactly what the scene sizes: one entry more is the sanitizer's to find
        for (int m = 0; m < f.num_meshes; m++) {
            rt_nr_walk w;
            if (!rt_nr_mesh_begin(S.meshes[2 * m], S.meshes[2 * m + 1], p[0], p[1], p[2], best, w)) { g_skipped_meshes++; continue; }
            const int32_t object = (int32_t)rt_nr_bits(S.meshes[2 * m + 1].w);
            while (rt_nr_step<1>(S, stack.data(), object, p[0], p[1], p[2], best, w)) g_steps++;
        }
    }
    rt_nr_record(S, p[0], p[1], p[2], best, out);
    return out;
}

// ---- the definition: every candidate ------------------------------------------------------------------------------------------------------
static void every_triangle(const Flat &f, uint32_t ref, float path, int32_t object, const float p[3], rt_nr_best &best)
{
    const rt_nr_scene<rt_f4> S = f.S();
    float pt[3];
    if (ref & RT_REF_LEAF) {
        const int start = (int)(ref & RT_REF_START_MASK), count = (int)((ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        for (int k = 0; k < count; k++) {
            const rt_f4 *t = S.tris + 3 * (size_t)(start + k);
            rt_nr_offer(rt_nr_clamp(rt_nr_tri(t[0], t[1], t[2], p[0], p[1], p[2], pt), path), object, start + k, best);
        }
        return;
    }
    const rt_f4 *n = S.nodes + 4 * (size_t)(ref & RT_REF_NODE_MASK);
    const float dl = rt_nr_box_d2(n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, p[0], p[1], p[2]);
    const float dr = rt_nr_box_d2(n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w, p[0], p[1], p[2]);
    every_triangle(f, rt_nr_bits(n[3].y), rt_nr_path(path, dr), object, p, best);     // (right first: not the walk's order)
    every_triangle(f, rt_nr_bits(n[3].x), rt_nr_path(path, dl), object, p, best);
}

static rt_nearest exhaustive(const Flat &f, const float p[3], bool has_limit, float max_dist)
{
    const rt_nr_scene<rt_f4> S = f.S();
    rt_nearest out;
    rt_nr_best best;
    if (rt_nr_begin(p[0], p[1], p[2], has_limit, max_dist, best)) {
        for (int m = f.num_meshes - 1; m >= 0; m--) {                   // (meshes first and backwards: not the walk's order)
            const rt_f4 m0 = S.meshes[2 * m], m1 = S.meshes[2 * m + 1];
            every_triangle(f, rt_nr_bits(m1.z), rt_nr_box_d2(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, p[0], p[1], p[2]), (int32_t)rt_nr_bits(m1.w), p, best);
        }
        float pt[3];
        for (int i = f.num_objects - 1; i >= 0; i--) {
            rt_object ob;
            std::memcpy(&ob, S.objtab + 3 * i, sizeof ob);
            if (ob.type == RT_OBJ_MESH) continue;
            if (ob.type == RT_OBJ_SPHERE) { rt_nr_offer(rt_nr_sphere(ob.v[0], ob.v[1], ob.v[2], ob.v[3], p[0], p[1], p[2], pt), i, -1, best); continue; }
            const int count = ob.type == RT_OBJ_TRIANGLE ? 1 : ob.type == RT_OBJ_CUBOID ? 12 : 2;
            for (int k = count - 1; k >= 0; k--) {
                const rt_f4 *t = S.tris + 3 * (size_t)(ob.prim_start + k);
                rt_nr_offer(rt_nr_tri(t[0], t[1], t[2], p[0], p[1], p[2], pt), i, ob.prim_start + k, best);
            }
        }
    }
    rt_nr_record(S, p[0], p[1], p[2], best, out);
    return out;
}

// ---- scenes --------------------------------------------------------------------------------------------------------------------------------
static float uniform(std::mt19937 &rng, float lo, float hi) { return lo + (hi - lo) * (float)(rng() % 1000001) / 1000000.0f; }

static std::vector<float> soup(std::mt19937 &rng, int n, float spread, float size)
{
    std::vector<float> t((size_t)n * 9);
    for (int i = 0; i < n; i++) {
        const float c[3] = {uniform(rng, -spread, spread), uniform(rng, -spread, spread), uniform(rng, 2.0f - spread, 2.0f + spread)};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) t[(size_t)i * 9 + v * 3 + k] = c[k] + uniform(rng, -size, size);
    }
    return t;
}

struct Scene {
    rt_scene_builder *b = nullptr;
    rt_flat_view v{};
    Scene() = default;
    Scene(const Scene &) = delete;
    ~Scene() { rt_scene_builder_destroy(b); }
};

// [sphere, mesh, quad, cuboid, second mesh, triangle, one-way quad, sphere] - or the mesh alone
static bool make_scene(Scene &s, const std::vector<float> &tris, const std::vector<float> &second, bool mesh_alone)
{
    if (rt_scene_builder_create(&s.b) != RT_OK) return false;
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    rt_material plain;
    rt_material_standard(&plain, grey, 0.2f);
    const float c0[3] = {0.4f, 0.1f, 1.5f}, c1[3] = {-0.9f, 0.6f, 2.5f}, cc[3] = {0.8f, -0.4f, 2.6f};
    const float q[4][3] = {{-3, -1, -1}, {3, -1, -1}, {3, -1, 7}, {-3, -1, 7}}, o[4][3] = {{-1, 1, 3}, {0, 1, 3}, {0, 2, 3}, {-1, 2, 3}};
    const float t[3][3] = {{1.0f, 1.0f, 1.0f}, {1.5f, 1.0f, 1.2f}, {1.2f, 1.6f, 0.9f}};
    bool ok = true;
    if (!mesh_alone) ok = ok && rt_scene_add_sphere(s.b, c0, 0.3f, &plain) == RT_OK;
    ok = ok && rt_scene_add_mesh(s.b, tris.data(), (int32_t)(tris.size() / 9), &plain) == RT_OK;
    if (!mesh_alone) {
        ok = ok && rt_scene_add_quad(s.b, q[0], q[1], q[2], q[3], &plain) == RT_OK && rt_scene_add_cuboid(s.b, cc, 0.3f, 0.2f, 0.4f, &plain) == RT_OK;
        ok = ok && rt_scene_add_mesh(s.b, second.data(), (int32_t)(second.size() / 9), &plain) == RT_OK;
        ok = ok && rt_scene_add_triangle(s.b, t[0], t[1], t[2], &plain) == RT_OK && rt_scene_add_one_way_quad(s.b, o[0], o[1], o[2], o[3], 1, &plain) == RT_OK;
        ok = ok && rt_scene_add_sphere(s.b, c1, 0.25f, &plain) == RT_OK;
    }
    return ok && rt_debug_flatten(s.b, &s.v) == RT_OK;
}

static int same(const rt_nearest &a, const rt_nearest &b) { return !std::memcmp(&a, &b, sizeof a); }

static int check_scene(const std::vector<float> &tris, const std::vector<float> &second, bool mesh_alone, int points, std::mt19937 &rng)
{
    Scene s;
    CHECK(make_scene(s, tris, second, mesh_alone), "building the scene");
    const Flat f = flat_of(s.v);
    const int n_tris = s.v.num_triangles;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < points; i++) {
        float p[3];
        const unsigned kind = rng() % 8;
        if (kind < 3) {
            for (int k = 0; k < 3; k++) p[k] = uniform(rng, -2.5f, 2.5f) + (k == 2 ? 2.0f : 0.0f);
        } else if (kind < 6 && n_tris > 0) {                        // on a surface: a vertex, an edge midpoint or the centroid of some triangle record
            const rt_f4 *t = f.blob + f.off_tris + 3 * (size_t)(rng() % (unsigned)n_tris);
            const float a[3] = {t[0].x, t[0].y, t[0].z}, s1[3] = {t[0].w, t[1].x, t[1].y}, s2[3] = {t[1].z, t[1].w, t[2].x};
            const unsigned where = rng() % 5;
            for (int k = 0; k < 3; k++)
                p[k] = where == 0 ? a[k] : where == 1 ? a[k] + s1[k] : where == 2 ? a[k] + s1[k] / 2 : where == 3 ? (a[k] + s1[k]) + (s2[k] - s1[k]) / 2 : a[k] + (s1[k] + s2[k]) / 3;
        } else if (kind == 6) {                                     // large coordinates, signed zeros
            for (int k = 0; k < 3; k++) { const unsigned r = rng() % 4; p[k] = r == 0 ? 1048576.0f : r == 1 ? -1048576.0f : r == 2 ? -0.0f : uniform(rng, -1000.0f, 1000.0f); }
        } else {                                                    // a sphere's centre, or the scene's first point again
            p[0] = 0.4f; p[1] = 0.1f; p[2] = 1.5f;
        }
        const rt_nearest free_walk = walk(f, p, false, 0.0f), free_all = exhaustive(f, p, false, 0.0f);
        g_points++;
        CHECK(same(free_walk, free_all), "the walk differs from the exhaustive minimum");
        CHECK(free_all.object >= 0 && free_all.reserved == 0 && free_all.distance == std::sqrt(free_all.distance2), "an unbounded query of a scene with objects has an answer");
        // limits: the answer's own distance, one step down and up, 0, a random one, and the ones that miss
        const float d = free_all.distance;
        const float lims[] = {d, std::nextafter(d, 0.0f), std::nextafter(d, inf), 0.0f, -0.0f, uniform(rng, 0.0f, 3.0f), inf, -1.0f, nan, -inf};
        for (float l : lims) {
            const rt_nearest a = walk(f, p, true, l), b = exhaustive(f, p, true, l);
            CHECK(same(a, b), "the walk differs from the exhaustive minimum under a limit");
            if (l == inf) CHECK(same(a, free_all), "+Inf is unbounded");
            if (!(l >= 0.0f)) CHECK(a.object == -1 && a.triangle == -1 && a.distance == RT_HIT_MISS_T && a.distance2 == RT_HIT_MISS_T && a.point[0] == 0.0f, "a NaN or negative limit misses");
            if (a.object >= 0) CHECK(a.distance2 <= l * l, "a winner beyond the limit");
        }
    }
    const float bad[3][3] = {{nan, 0, 0}, {0, inf, 0}, {0, 0, -inf}};
    for (const float *p : {bad[0], bad[1], bad[2]}) {
        const rt_nearest a = walk(f, p, false, 0.0f);
        CHECK(same(a, exhaustive(f, p, false, 0.0f)) && a.object == -1 && a.distance == RT_HIT_MISS_T, "a point that is not finite misses");
    }
    return 0;
}

// ---- the refusals --------------------------------------------------------------------------------------------------------------------------
static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

static int refusals()
{
    g_case = "refusals";
    rt_ctx ctx, other;
    rt_scene scene, foreign;
    scene.ctx = &ctx; foreign.ctx = &other;
    alignas(16) static rt_nearest out[2];
    const float pts[6] = {0, 0, 0, 1, 1, 1}, lim[2] = {1, 1};
    rt_nearest *const misaligned = (rt_nearest *)((char *)out + 4);
    for (int form = 0; form < 2; form++) {
        auto call = [&](rt_ctx *c, const rt_scene *s, const float *p, const float *l, int64_t n, rt_nearest *o) {
            return form ? rt_nearest_points(c, s, p, l, n, o) : rt_nearest_points_device(c, s, p, l, n, o, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(call(nullptr, &scene, pts, lim, 2, out) == RT_ERR_INVALID, "null context");
        CHECK(call(nullptr, nullptr, nullptr, nullptr, 0, nullptr) == RT_ERR_INVALID, "null context, no points");
        CHECK(call(&ctx, nullptr, pts, lim, 2, out) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(call(&ctx, &foreign, pts, lim, 2, out) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(call(&ctx, &scene, pts, lim, -1, out) == RT_ERR_INVALID && said(ctx, "point count"), "a negative count");
        CHECK(call(&ctx, &scene, pts, lim, ((int64_t)1 << 30) + 1, out) == RT_ERR_INVALID && said(ctx, "point count"), "more than 2^30 points");
        CHECK(call(&ctx, &scene, nullptr, lim, 2, out) == RT_ERR_INVALID && said(ctx, "null argument"), "null points");
        CHECK(call(&ctx, &scene, pts, lim, 2, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null records");
        CHECK(call(&ctx, &scene, nullptr, nullptr, 0, nullptr) == RT_OK && call(&ctx, &scene, pts, lim, 0, out) == RT_OK, "no points: nothing to do");
    }
    CHECK(rt_nearest_points_device(&ctx, &scene, pts, nullptr, 2, misaligned, nullptr) == RT_ERR_INVALID && said(ctx, "16-byte aligned"), "misaligned records");
    CHECK(g_launches == 0, "a refused call reached a launcher");
    CHECK(!ctx.launched && !ctx.have_timing && ctx.last_stream == nullptr, "a refused call touched the launch order");
    return 0;
}

// ---- a scene from a file -------------------------------------------------------------------------------------------------------------------
static int from_file(const char *in, const char *outp)
{
    FILE *fi = std::fopen(in, "rb");
    if (!fi) return 2;
    int32_t h[9];
    if (std::fread(h, 4, 9, fi) != 9 || h[0] < 0 || h[7] < 0) { std::fclose(fi); return 2; }
    std::vector<rt_f4> blob((size_t)h[0] + 1);
    std::vector<float> pts((size_t)h[7] * 3 + 1), lim((size_t)h[7] + 1);
    bool ok = std::fread(blob.data(), 16, (size_t)h[0], fi) == (size_t)h[0] && std::fread(pts.data(), 12, (size_t)h[7], fi) == (size_t)h[7];
    if (h[8]) ok = ok && std::fread(lim.data(), 4, (size_t)h[7], fi) == (size_t)h[7];
    std::fclose(fi);
    if (!ok) return 2;
    const Flat f{blob.data(), h[1], h[2], h[3], h[3] + 2 * h[4], h[4], h[5], h[6]};
    std::vector<rt_nearest> out((size_t)h[7]);
    for (int i = 0; i < h[7]; i++) out[(size_t)i] = walk(f, &pts[(size_t)i * 3], h[8] != 0, lim[(size_t)i]);
    FILE *fo = std::fopen(outp, "wb");
    if (!fo) return 2;
    ok = std::fwrite(out.data(), sizeof(rt_nearest), out.size(), fo) == out.size();
    std::fclose(fo);
    std::printf("nearest host side: %d points from a file, %ld steps, sanitizers silent\n", h[7], g_steps);
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(rt_nearest) == 32 && alignof(rt_nearest) == 16 && sizeof(rt_nr_entry) == 8, "the record and the stack entry");
    if (argc == 4 && !std::strcmp(argv[1], "file")) return from_file(argv[2], argv[3]);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int points = argc > 2 ? std::atoi(argv[2]) : 200;
    std::mt19937 rng(seed);
    const std::vector<float> second = soup(rng, 37, 0.8f, 0.15f);
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 100, 1023, 1024, 1025, 3000};
    for (int n : sizes) {
        g_n = n;
        const int pts = n > 1000 ? points / 4 + 1 : points;
        g_case = "random";
        if (check_scene(soup(rng, n, 0.8f, 0.12f), second, false, pts, rng)) return 1;
        g_case = "the mesh alone";
        if (check_scene(soup(rng, n, 0.8f, 0.12f), second, true, pts, rng)) return 1;
        // ties: a coplanar fan around one vertex (z = 2: neighbours share edges, points above an edge are equally far from two triangles), every
        // triangle the same, every triangle four times
        std::vector<float> fan((size_t)n * 9), ident = soup(rng, n, 0.8f, 0.12f), dup = soup(rng, n, 0.8f, 0.12f);
        for (int i = 0; i < n; i++) {
            const float a0 = 6.2831853f * (float)i / (float)n, a1 = 6.2831853f * (float)(i + 1) / (float)n;
            const float t[9] = {0.0f, 0.0f, 2.0f, std::cos(a0), std::sin(a0), 2.0f, std::cos(a1), std::sin(a1), 2.0f};
            std::memcpy(&fan[(size_t)i * 9], t, 36);
            std::memcpy(&ident[(size_t)i * 9], &ident[0], 36);
            std::memcpy(&dup[(size_t)i * 9], &dup[(size_t)(i / 4) * 9], 36);
        }
        g_case = "a coplanar fan";
        if (check_scene(fan, second, true, pts, rng) || check_scene(fan, second, false, pts / 2 + 1, rng)) return 1;
        g_case = "identical triangles";
        if (check_scene(ident, second, true, pts / 2 + 1, rng)) return 1;
        g_case = "every triangle four times";
        if (check_scene(dup, second, false, pts / 2 + 1, rng)) return 1;
    }
    if (refusals()) return 1;
    std::printf("nearest host side: %ld points on %d sizes of meshes, %ld steps, %ld meshes skipped at their root box, sanitizers silent\n", g_points,
                (int)(sizeof sizes / sizeof sizes[0]), g_steps, g_skipped_meshes);
    return 0;
}
