// The sphere-cast queries (rt_sweep_spheres[_device]: rt_sweep.h, rt_sweep_capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer
// (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. the kernel's traversal as plain host code - the steps of rt_sweep.h (rt_sw_begin, rt_sw_simple, rt_sw_mesh_begin, rt_sw_step,
//      rt_sw_record), the text the kernel compiles, on a stack of exactly the scene's stack_entries, behind the nearest-surface walk of
//      rt_nearest.h that decides the start overlap - against the EXHAUSTIVE minimum over every candidate (every sphere, every triangle
//      record, a mesh's triangles under the path flags and values of a plain recursion over its whole tree), byte for byte: seeded random
//      and adversarial inputs - balls aimed at vertices and edges, radius 0 and radii larger than the scene, signed zeros, tied keys
//      (coplanar fans, identical triangles), zero-area triangles, meshes of 1 to 9 triangles (every chain shape) and of about 1,024,
//      limits around the answer;
//   2. every refusal of both entry points, on a context and scenes built in host memory (nothing gets as far as a HIP call or the launcher).
//   sweep_host_check <seed> <balls per scene>
// A second form answers a scene from a file, for tests/test_sweep_host.py to set against the NumPy yardstick:
//   sweep_host_check file <in> <out>   in: int32 blob_f4, off_nodes, off_tris, off_meshes, num_meshes, num_objects, stack_entries, n, has_limit;
//                                          the blob; n x 3 origins; n x 3 directions; n radii; n limits if has_limit.   out: n records
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
#include "rt_sweep.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                             \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "sweep check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_steps = 0, g_skipped_meshes = 0, g_balls = 0, g_overlaps = 0, g_hits = 0, g_feature[8] = {0, 0, 0, 0, 0, 0, 0, 0};

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

struct Ball { float o[3], d[3], r; bool has_limit; float tmax; };

static rt_mh_ray ray_of(const Ball &b)
{
    rt_mh_ray q;
    q.ox = b.o[0]; q.oy = b.o[1]; q.oz = b.o[2]; q.dx = b.d[0]; q.dy = b.d[1]; q.dz = b.d[2];
    q.ix = q.iy = q.iz = 0.0f;
    return q;
}

// ---- the first launch: the nearest-surface walk of the origin under the radius (rt_nearest.h's steps, as nearest_host_check.cpp runs them)
static rt_nearest nearest_walk(const Flat &f, const float p[3], float max_dist)
{
    const rt_nr_scene<rt_f4> S = f.S();
    rt_nearest out;
    rt_nr_best best;
    if (rt_nr_begin(p[0], p[1], p[2], true, max_dist, best)) {
        rt_nr_simple(S, f.num_objects, p[0], p[1], p[2], best);
        std::vector<rt_nr_entry> stack((size_t)f.stack_entries);
        for (int m = 0; m < f.num_meshes; m++) {
            rt_nr_walk w;
            if (!rt_nr_mesh_begin(S.meshes[2 * m], S.meshes[2 * m + 1], p[0], p[1], p[2], best, w)) continue;
            const int32_t object = (int32_t)rt_nr_bits(S.meshes[2 * m + 1].w);
            while (rt_nr_step<1>(S, stack.data(), object, p[0], p[1], p[2], best, w)) {}
        }
    }
    rt_nr_record(S, p[0], p[1], p[2], best, out);
    return out;
}

// ---- the kernel's path: one lane, the steps in a plain loop -------------------------------------------------------------------------------
static rt_sweep walk(const Flat &f, const Ball &b)
{
    const rt_nr_scene<rt_f4> S = f.S();
    const rt_nearest near = nearest_walk(f, b.o, b.r);
    rt_mh_ray q = ray_of(b);
    float dd;
    rt_sw_best best;
    rt_sweep out;
    if (rt_sw_begin(q, b.r, b.has_limit, b.tmax, dd, best)) {
        if (near.object >= 0) {
            best.k.object = RT_SW_OVERLAP;
        } else {
            rt_sw_simple(S, f.num_objects, q, dd, b.r, best);
            std::vector<rt_nr_entry> stack((size_t)f.stack_entries);          // exactly what the scene sizes: one entry more is the sanitizer's to find
            for (int m = 0; m < f.num_meshes; m++) {
                rt_sw_walk w;
                if (!rt_sw_mesh_begin(S.meshes[2 * m], S.meshes[2 * m + 1], q, b.r, best, w)) { g_skipped_meshes++; continue; }
                const int32_t object = (int32_t)rt_nr_bits(S.meshes[2 * m + 1].w);
                while (rt_sw_step<1>(S, stack.data(), object, q, dd, b.r, best, w)) g_steps++;
            }
        }
    }
    rt_sw_record(S, q, dd, b.r, best, &near, out);
    return out;
}

// ---- the definition: every candidate ------------------------------------------------------------------------------------------------------
static void every_triangle(const Flat &f, uint32_t ref, float path, int32_t object, const rt_mh_ray &q, float dd, float r, rt_sw_best &best)
{
    const rt_nr_scene<rt_f4> S = f.S();
    if (ref & RT_REF_LEAF) {
        const int start = (int)(ref & RT_REF_START_MASK), count = (int)((ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        for (int k = count - 1; k >= 0; k--) {                              // (backwards: not the walk's order)
            const rt_f4 *t = S.tris + 3 * (size_t)(start + k);
            int32_t feature;
            const float tt = rt_sw_tri(t[0], t[1], t[2], q, dd, r, feature);
            rt_sw_offer(tt < path ? path : tt, tt, feature, object, start + k, best);
        }
        return;
    }
    const rt_f4 *n = S.nodes + 4 * (size_t)(ref & RT_REF_NODE_MASK);
    float tl, tr;
    const bool hl = rt_sw_box(n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, r, q, tl);
    const bool hr = rt_sw_box(n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w, r, q, tr);
    if (hr) every_triangle(f, rt_nr_bits(n[3].y), tr < path ? path : tr, object, q, dd, r, best);     // (right first: not the walk's order)
    if (hl) every_triangle(f, rt_nr_bits(n[3].x), tl < path ? path : tl, object, q, dd, r, best);
}

static rt_sweep exhaustive(const Flat &f, const Ball &b)
{
    const rt_nr_scene<rt_f4> S = f.S();
    const rt_nearest near = nearest_walk(f, b.o, b.r);
    rt_mh_ray q = ray_of(b);
    float dd;
    rt_sw_best best;
    rt_sweep out;
    if (rt_sw_begin(q, b.r, b.has_limit, b.tmax, dd, best)) {
        if (near.object >= 0) {
            best.k.object = RT_SW_OVERLAP;
        } else {
            for (int m = f.num_meshes - 1; m >= 0; m--) {                   // (meshes first and backwards: not the walk's order)
                const rt_f4 m0 = S.meshes[2 * m], m1 = S.meshes[2 * m + 1];
                float key;
                if (rt_sw_box(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, b.r, q, key)) every_triangle(f, rt_nr_bits(m1.z), key, (int32_t)rt_nr_bits(m1.w), q, dd, b.r, best);
            }
            for (int i = f.num_objects - 1; i >= 0; i--) {
                rt_object ob;
                std::memcpy(&ob, S.objtab + 3 * i, sizeof ob);
                if (ob.type == RT_OBJ_MESH) continue;
                float t;
                if (ob.type == RT_OBJ_SPHERE) {
                    if (rt_sw_sphere(ob.v[0], ob.v[1], ob.v[2], ob.v[3], q, dd, b.r, t)) rt_sw_offer(t, t, -1, i, -1, best);
                    continue;
                }
                const int count = ob.type == RT_OBJ_TRIANGLE ? 1 : ob.type == RT_OBJ_CUBOID ? 12 : 2;
                for (int k = count - 1; k >= 0; k--) {
                    const rt_f4 *tr = S.tris + 3 * (size_t)(ob.prim_start + k);
                    int32_t feature;
                    t = rt_sw_tri(tr[0], tr[1], tr[2], q, dd, b.r, feature);
                    rt_sw_offer(t, t, feature, i, ob.prim_start + k, best);
                }
            }
        }
    }
    rt_sw_record(S, q, dd, b.r, best, &near, out);
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

static int same(const rt_sweep &a, const rt_sweep &b) { return !std::memcmp(&a, &b, sizeof a); }

static bool is_miss(const rt_sweep &a)
{
    return a.t == RT_HIT_MISS_T && a.object == -1 && a.triangle == -1 && a.feature == -1 && a.overlap == 0 && a.reserved == 0 && a.centre[0] == 0.0f &&
           a.centre[1] == 0.0f && a.centre[2] == 0.0f && a.point[0] == 0.0f && a.point[1] == 0.0f && a.point[2] == 0.0f;
}

static int check_scene(const std::vector<float> &tris, const std::vector<float> &second, bool mesh_alone, int balls, std::mt19937 &rng)
{
    Scene s;
    CHECK(make_scene(s, tris, second, mesh_alone), "building the scene");
    const Flat f = flat_of(s.v);
    const int n_tris = s.v.num_triangles;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < balls; i++) {
        Ball b;
        b.has_limit = false; b.tmax = 0.0f;
        float target[3];
        const unsigned kind = rng() % 8;
        for (int k = 0; k < 3; k++) b.o[k] = uniform(rng, -3.5f, 3.5f) + (k == 2 ? 2.0f : 0.0f);
        for (int k = 0; k < 3; k++) target[k] = uniform(rng, -1.0f, 1.0f) + (k == 2 ? 2.0f : 0.0f);
        if (kind < 5 && n_tris > 0) {                               // aimed at a vertex, a point of an edge or the inside of some triangle record
            const rt_f4 *t = f.blob + f.off_tris + 3 * (size_t)(rng() % (unsigned)n_tris);
            const float a[3] = {t[0].x, t[0].y, t[0].z}, s1[3] = {t[0].w, t[1].x, t[1].y}, s2[3] = {t[1].z, t[1].w, t[2].x};
            const unsigned where = rng() % 7;
            const float u = uniform(rng, 0.05f, 0.95f);
            for (int k = 0; k < 3; k++)
                target[k] = where == 0 ? a[k] : where == 1 ? a[k] + s1[k] : where == 2 ? a[k] + s2[k] : where == 3 ? a[k] + s1[k] * u : where == 4 ? a[k] + s2[k] * u
                          : where == 5 ? (a[k] + s1[k]) + (s2[k] - s1[k]) * u : a[k] + (s1[k] + s2[k]) / 3;
        } else if (kind == 5) {                                     // a sphere's centre
            target[0] = 0.4f; target[1] = 0.1f; target[2] = 1.5f;
        } else if (kind == 6) {                                     // signed zeros and axis-parallel paths
            for (int k = 0; k < 3; k++) { const unsigned z = rng() % 3; if (z == 0) b.o[k] = target[k] = -0.0f; else if (z == 1) target[k] = b.o[k]; }
        }
        for (int k = 0; k < 3; k++) b.d[k] = target[k] - b.o[k];
        if (b.d[0] == 0.0f && b.d[1] == 0.0f && b.d[2] == 0.0f) b.d[2] = -0.0f, b.d[1] = 1.0f;
        if (rng() % 3 == 0) { const float l = std::sqrt(b.d[0] * b.d[0] + b.d[1] * b.d[1] + b.d[2] * b.d[2]); for (int k = 0; k < 3; k++) b.d[k] /= l; }
        const unsigned rk = rng() % 8;
        b.r = rk == 0 ? 0.0f : rk == 1 ? -0.0f : rk < 4 ? uniform(rng, 0.001f, 0.02f) : rk < 7 ? uniform(rng, 0.05f, 0.4f) : uniform(rng, 3.0f, 30.0f);
        if (rng() % 10 == 0) for (int k = 0; k < 3; k++) b.o[k] = target[k] - b.d[k] * 0.01f;      // next to the target: overlaps, and contacts at the start
        const rt_sweep free_walk = walk(f, b), free_all = exhaustive(f, b);
        g_balls++;
        CHECK(same(free_walk, free_all), "the walk differs from the exhaustive minimum");
        CHECK(free_all.reserved == 0 && (free_all.overlap == 0 || (free_all.t == 0.0f && free_all.feature == -1 && free_all.object >= 0)), "a start overlap is reported at t = 0");
        if (free_all.overlap) g_overlaps++;
        if (free_all.object < 0) { CHECK(is_miss(free_all), "the miss pattern"); }
        else if (!free_all.overlap) { g_hits++; g_feature[free_all.feature + 1]++; CHECK(free_all.t >= 0.0f && free_all.feature >= -1 && free_all.feature <= 6, "a contact has a time and a feature"); }
        // limits: the answer's own time, one step down and up, a random one, and the ones that miss
        const float t = free_all.object >= 0 ? free_all.t : 1.0f;
        const float lims[] = {t, std::nextafter(t, 0.0f), std::nextafter(t, inf), uniform(rng, 0.0f, 3.0f), inf, 0.0f, -0.0f, -1.0f, nan, -inf};
        for (float l : lims) {
            Ball c = b;
            c.has_limit = true; c.tmax = l;
            const rt_sweep a = walk(f, c), e = exhaustive(f, c);
            CHECK(same(a, e), "the walk differs from the exhaustive minimum under a limit");
            if (l == inf) CHECK(same(a, free_all), "+Inf is unbounded");
            if (!(l > 0.0f)) CHECK(is_miss(a), "a NaN limit or one that is not positive misses");
            if (a.object >= 0 && !a.overlap && a.triangle < 0) CHECK(a.t <= l, "a winner beyond the limit");
        }
    }
    Ball ok_ball;
    ok_ball.o[0] = 0.1f; ok_ball.o[1] = 3.0f; ok_ball.o[2] = 2.0f; ok_ball.d[0] = 0.0f; ok_ball.d[1] = -1.0f; ok_ball.d[2] = 0.0f; ok_ball.r = 0.1f; ok_ball.has_limit = false; ok_ball.tmax = 0.0f;
    for (int k = 0; k < 3; k++)
        for (float bad : {nan, inf, -inf}) {
            Ball b = ok_ball;
            b.o[k] = bad;
            CHECK(is_miss(walk(f, b)) && is_miss(exhaustive(f, b)), "an origin that is not finite misses");
            b = ok_ball;
            b.d[k] = bad;
            CHECK(is_miss(walk(f, b)) && is_miss(exhaustive(f, b)), "a direction that is not finite misses");
        }
    for (float bad : {nan, inf, -inf, -1.0f, -1e-30f}) {
        Ball b = ok_ball;
        b.r = bad;
        CHECK(is_miss(walk(f, b)) && is_miss(exhaustive(f, b)), "a radius that is NaN, negative or infinite misses");
    }
    Ball still = ok_ball;
    still.d[1] = -0.0f;
    CHECK(is_miss(walk(f, still)) && is_miss(exhaustive(f, still)), "a zero direction misses");
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
    alignas(16) static rt_sweep out[2];
    const float o[6] = {0, 0, 0, 1, 1, 1}, d[6] = {0, 0, 1, 0, 1, 0}, r[2] = {0.1f, 0.2f}, lim[2] = {1, 1};
    rt_sweep *const misaligned = (rt_sweep *)((char *)out + 4);
    for (int form = 0; form < 2; form++) {
        auto call = [&](rt_ctx *c, const rt_scene *s, const float *po, const float *pd, const float *pr, const float *l, int64_t n, rt_sweep *res) {
            return form ? rt_sweep_spheres(c, s, po, pd, pr, l, n, res) : rt_sweep_spheres_device(c, s, po, pd, pr, l, n, res, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(call(nullptr, &scene, o, d, r, lim, 2, out) == RT_ERR_INVALID, "null context");
        CHECK(call(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == RT_ERR_INVALID, "null context, no balls");
        CHECK(call(&ctx, nullptr, o, d, r, lim, 2, out) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(call(&ctx, &foreign, o, d, r, lim, 2, out) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(call(&ctx, &scene, o, d, r, lim, -1, out) == RT_ERR_INVALID && said(ctx, "point count"), "a negative count");
        CHECK(call(&ctx, &scene, o, d, r, lim, ((int64_t)1 << 30) + 1, out) == RT_ERR_INVALID && said(ctx, "point count"), "more than 2^30 balls");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, nullptr, d, r, lim, 2, out) == RT_ERR_INVALID && said(ctx, "null argument"), "null origins");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, o, nullptr, r, lim, 2, out) == RT_ERR_INVALID && said(ctx, "null argument"), "null directions");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, o, d, nullptr, lim, 2, out) == RT_ERR_INVALID && said(ctx, "null argument"), "null radii");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, o, d, r, lim, 2, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null records");
        CHECK(call(&ctx, &scene, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == RT_OK && call(&ctx, &scene, o, d, r, lim, 0, out) == RT_OK, "no balls: nothing to do");
    }
    CHECK(rt_sweep_spheres_device(&ctx, &scene, o, d, r, nullptr, 2, misaligned, nullptr) == RT_ERR_INVALID && said(ctx, "16-byte aligned"), "misaligned records");
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
    const size_t n = (size_t)h[7];
    std::vector<rt_f4> blob((size_t)h[0] + 1);
    std::vector<float> org(n * 3 + 1), dir(n * 3 + 1), rad(n + 1), lim(n + 1);
    bool ok = std::fread(blob.data(), 16, (size_t)h[0], fi) == (size_t)h[0] && std::fread(org.data(), 12, n, fi) == n && std::fread(dir.data(), 12, n, fi) == n &&
              std::fread(rad.data(), 4, n, fi) == n;
    if (h[8]) ok = ok && std::fread(lim.data(), 4, n, fi) == n;
    std::fclose(fi);
    if (!ok) return 2;
    const Flat f{blob.data(), h[1], h[2], h[3], h[3] + 2 * h[4], h[4], h[5], h[6]};
    std::vector<rt_sweep> out(n);
    for (size_t i = 0; i < n; i++) {
        Ball b;
        for (int k = 0; k < 3; k++) { b.o[k] = org[i * 3 + k]; b.d[k] = dir[i * 3 + k]; }
        b.r = rad[i]; b.has_limit = h[8] != 0; b.tmax = lim[i];
        out[i] = walk(f, b);
    }
    FILE *fo = std::fopen(outp, "wb");
    if (!fo) return 2;
    ok = std::fwrite(out.data(), sizeof(rt_sweep), out.size(), fo) == out.size();
    std::fclose(fo);
    std::printf("sweep host side: %d balls from a file, %ld steps, sanitizers silent\n", h[7], g_steps);
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(rt_sweep) == 48 && alignof(rt_sweep) == 16 && sizeof(rt_nr_entry) == 8, "the record and the stack entry");
    if (argc == 4 && !std::strcmp(argv[1], "file")) return from_file(argv[2], argv[3]);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int balls = argc > 2 ? std::atoi(argv[2]) : 200;
    std::mt19937 rng(seed);
    const std::vector<float> second = soup(rng, 37, 0.8f, 0.15f);
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 100, 1023, 1025};
    for (int n : sizes) {
        g_n = n;
        const int count = n > 1000 ? balls / 4 + 1 : balls;
        g_case = "random";
        if (check_scene(soup(rng, n, 0.8f, 0.12f), second, false, count, rng)) return 1;
        g_case = "the mesh alone";
        if (check_scene(soup(rng, n, 0.8f, 0.12f), second, true, count, rng)) return 1;
        // ties: a coplanar fan around one vertex (neighbours share edges and the hub: equal times on several records), every triangle the same,
        // every triangle four times; and zero-area triangles (two vertices the same, all three the same) among ordinary ones
        std::vector<float> fan((size_t)n * 9), ident = soup(rng, n, 0.8f, 0.12f), dup = soup(rng, n, 0.8f, 0.12f), thin = soup(rng, n, 0.8f, 0.12f);
        for (int i = 0; i < n; i++) {
            const float a0 = 6.2831853f * (float)i / (float)n, a1 = 6.2831853f * (float)(i + 1) / (float)n;
            const float t[9] = {0.0f, 0.0f, 2.0f, std::cos(a0), std::sin(a0), 2.0f, std::cos(a1), std::sin(a1), 2.0f};
            std::memcpy(&fan[(size_t)i * 9], t, 36);
            std::memcpy(&ident[(size_t)i * 9], &ident[0], 36);
            std::memcpy(&dup[(size_t)i * 9], &dup[(size_t)(i / 4) * 9], 36);
            if (i % 3 == 0) std::memcpy(&thin[(size_t)i * 9 + 3], &thin[(size_t)i * 9], 12);
            if (i % 6 == 0) std::memcpy(&thin[(size_t)i * 9 + 6], &thin[(size_t)i * 9], 12);
        }
        g_case = "a coplanar fan";
        if (check_scene(fan, second, true, count, rng) || check_scene(fan, second, false, count / 2 + 1, rng)) return 1;
        g_case = "identical triangles";
        if (check_scene(ident, second, true, count / 2 + 1, rng)) return 1;
        g_case = "every triangle four times";
        if (check_scene(dup, second, false, count / 2 + 1, rng)) return 1;
        g_case = "zero-area triangles";
        if (check_scene(thin, second, true, count / 2 + 1, rng)) return 1;
    }
    if (refusals()) return 1;
    for (int k = 0; k < 8; k++)
        if (g_feature[k] == 0) { std::fprintf(stderr, "sweep check: no contact with feature %d in the whole run\n", k - 1); return 1; }
    std::printf("sweep host side: %ld balls on %d sizes of meshes (%ld contacts: sphere %ld, face %ld, edges %ld %ld %ld, vertices %ld %ld %ld; %ld start overlaps), "
                "%ld steps, %ld meshes skipped at their root box, sanitizers silent\n", g_balls, (int)(sizeof sizes / sizeof sizes[0]), g_hits, g_feature[0], g_feature[1],
                g_feature[2], g_feature[3], g_feature[4], g_feature[5], g_feature[6], g_feature[7], g_overlaps, g_steps, g_skipped_meshes);
    return 0;
}
