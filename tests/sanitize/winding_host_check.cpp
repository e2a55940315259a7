// The winding-number queries (rt_winding_numbers[_device], rt_signed_distance[_device]: rt_winding.h, rt_winding_capi.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. rt_winding.h's text - what the kernel compiles: the term, rt_wn_atan2, the record loop with its loads one ahead, the order list and the
//      flip words exactly as large as the scene makes them - as plain host code against a straightforward binary64 sum of solid angles, on seeded
//      random meshes (points well away from the triangles, where the angle is determined), on closed shapes (a tetrahedron given as triangles in
//      either orientation, a box given as quad faces of a file: |w| = 1 inside, 0 outside), and on the objects that are not meshes;
//   2. the flip bytes of every rt_scene_add_* path against the construction;
//   3. every refusal of the four entry points, on a context and scenes built in host memory (nothing gets as far as the launchers);
//   4. the scene's order list under an allocation that fails (the program hides every device from itself, so it is refused on any machine):
//      the scene is left as it was.
//   winding_host_check <seed> <points per scene>
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
#include "rt_winding.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                             \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "winding check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_points = 0, g_terms = 0;

// ---- a scene as the kernel reads it: the flattened blob, the order list and the flip words ---------------------------------------------
struct Scene {
    rt_scene_builder *b = nullptr;
    FlatScene flat;
    std::vector<uint32_t> words;
    Scene() = default;
    Scene(const Scene &) = delete;
    ~Scene() { rt_scene_builder_destroy(b); }
    bool finish()
    {
        if (!rt_flatten(*b, flat).empty()) return false;
        words.assign((flat.tri_flip_commit.size() + 3) / 4, 0u);                   // exactly what rt_winding_capi.cpp uploads: a byte more is the sanitizer's to find
        if (!flat.tri_flip_commit.empty()) std::memcpy(words.data(), flat.tri_flip_commit.data(), flat.tri_flip_commit.size());
        return true;
    }
    rt_wn_scene<rt_f4> S() const
    {
        rt_wn_scene<rt_f4> s;
        s.tris = flat.blob.data() + flat.off_tris; s.objtab = flat.blob.data() + flat.off_objtab;
        s.perm = flat.tri_order.data(); s.flip = words.data();
        s.num_objects = (int32_t)flat.objects.size(); s.num_tris = flat.num_tris;
        return s;
    }
};

static rt_material plain()
{
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    rt_material m;
    rt_material_standard(&m, grey, 0.2f);
    return m;
}

// ---- the definition, straightforwardly, in binary64 ----------------------------------------------------------------------------------------
static double angle64(const rt_f4 *t, const double p[3])
{
    const double p0[3] = {t[0].x, t[0].y, t[0].z}, s1[3] = {t[0].w, t[1].x, t[1].y}, s2[3] = {t[1].z, t[1].w, t[2].x};
    double a[3], b[3], c[3];
    for (int k = 0; k < 3; k++) { a[k] = p0[k] - p[k]; b[k] = a[k] + s1[k]; c[k] = a[k] + s2[k]; }
    auto dot = [](const double *u, const double *v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; };
    const double la = std::sqrt(dot(a, a)), lb = std::sqrt(dot(b, b)), lc = std::sqrt(dot(c, c));
    const double n[3] = {s1[1] * s2[2] - s1[2] * s2[1], s1[2] * s2[0] - s1[0] * s2[2], s1[0] * s2[1] - s1[1] * s2[0]};
    const double det = dot(a, n), den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la;
    return det == 0.0 ? 0.0 : std::atan2(det, den);
}

// object i's winding number from the flattened view alone (tri_flip in flattened order: not the order list, not the words)
static double object64(const Scene &s, int i, const float pf[3])
{
    const FlatScene &f = s.flat;
    const rt_object &o = f.objects[(size_t)i];
    const double p[3] = {pf[0], pf[1], pf[2]};
    const rt_f4 *tris = f.blob.data() + f.off_tris;
    if (o.type == RT_OBJ_SPHERE) {
        const double v[3] = {p[0] - o.v[0], p[1] - o.v[1], p[2] - o.v[2]};
        return v[0] * v[0] + v[1] * v[1] + v[2] * v[2] < (double)o.v[3] * o.v[3] ? 1.0 : 0.0;
    }
    if (o.type == RT_OBJ_CUBOID) {
        double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
        for (int k = 0; k < 12; k++) {
            const rt_f4 q = tris[3 * (size_t)(o.prim_start + k)];
            const double c[3] = {q.x, q.y, q.z};
            for (int d = 0; d < 3; d++) { lo[d] = std::fmin(lo[d], c[d]); hi[d] = std::fmax(hi[d], c[d]); }
        }
        return lo[0] < p[0] && p[0] < hi[0] && lo[1] < p[1] && p[1] < hi[1] && lo[2] < p[2] && p[2] < hi[2] ? 1.0 : 0.0;
    }
    const int end = o.type == RT_OBJ_MESH ? ((size_t)i + 1 < f.objects.size() ? f.objects[(size_t)i + 1].prim_start : f.num_tris)
                                          : o.prim_start + (o.type == RT_OBJ_TRIANGLE ? 1 : 2);
    double A = 0.0;
    for (int k = o.prim_start; k < end; k++) {
        const bool negate = o.type == RT_OBJ_MESH ? f.tri_flip[(size_t)k] != 0 : k > o.prim_start;
        const double t = angle64(tris + 3 * (size_t)k, p);
        A += negate ? -t : t;
        g_terms++;
    }
    return A / (2.0 * 3.14159265358979323846);
}

static double solids64(const Scene &s, const float p[3])
{
    double w = 0.0;
    for (size_t i = 0; i < s.flat.objects.size(); i++) {
        const int t = s.flat.objects[i].type;
        if (t == RT_OBJ_SPHERE || t == RT_OBJ_CUBOID || t == RT_OBJ_MESH) w += object64(s, (int)i, p);
    }
    return w;
}

// ---- scenes --------------------------------------------------------------------------------------------------------------------------------
static float uniform(std::mt19937 &rng, float lo, float hi) { return lo + (hi - lo) * (float)(rng() % 1000001) / 1000000.0f; }

static std::vector<float> soup(std::mt19937 &rng, int n)
{
    std::vector<float> t((size_t)n * 9);
    for (int i = 0; i < n; i++) {
        const float c[3] = {uniform(rng, -0.7f, 0.7f), uniform(rng, -0.7f, 0.7f), uniform(rng, 1.3f, 2.7f)};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) t[(size_t)i * 9 + v * 3 + k] = c[k] + uniform(rng, -0.15f, 0.15f);
    }
    return t;
}

// a box of quad faces as a file gives them (every face counter-clockwise from outside), rotated a little so that no face is axis-aligned
static bool add_quad_box(rt_scene_builder *b, const float centre[3], float half, const rt_material *m)
{
    float v[8][3];
    for (int i = 0; i < 8; i++) {
        const float x = (i & 1 ? half : -half), y = (i & 2 ? half : -half), z = (i & 4 ? half : -half);
        v[i][0] = centre[0] + 0.96f * x - 0.28f * y; v[i][1] = centre[1] + 0.28f * x + 0.96f * y; v[i][2] = centre[2] + z;
    }
    const int32_t idx[24] = {0, 2, 3, 1, 4, 5, 7, 6, 0, 1, 5, 4, 2, 6, 7, 3, 0, 4, 6, 2, 1, 3, 7, 5}, arity[6] = {4, 4, 4, 4, 4, 4};
    rt_obj *o = nullptr;
    if (rt_obj_from_arrays(&v[0][0], 8, idx, arity, 6, &o) != RT_OK) return false;
    const bool ok = rt_scene_add_obj_mesh(b, o, m) == RT_OK;
    rt_obj_destroy(o);
    return ok;
}

static void far_point(std::mt19937 &rng, float p[3])
{
    // on a shell of radius 3 to 6 around the soups' middle: every triangle is at least two units away
    for (;;) {
        const float d[3] = {uniform(rng, -1, 1), uniform(rng, -1, 1), uniform(rng, -1, 1)};
        const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (l < 0.2f || l > 1.0f) continue;
        const float r = uniform(rng, 3.0f, 6.0f) / l;
        p[0] = d[0] * r; p[1] = d[1] * r; p[2] = 2.0f + d[2] * r;
        return;
    }
}

static int check_soups(std::mt19937 &rng, int n, int points)
{
    g_case = "random meshes";
    g_n = n;
    Scene s;
    const rt_material m = plain();
    const float c0[3] = {0.3f, 0.2f, 1.8f}, cc[3] = {-0.5f, 0.4f, 2.2f}, box_at[3] = {0.4f, -0.3f, 2.1f};
    const float q[4][3] = {{-3, -1, -1}, {3, -1, -1}, {3, -1, 7}, {-3, -1, 7}}, t[3][3] = {{1.0f, 1.0f, 1.0f}, {1.5f, 1.0f, 1.2f}, {1.2f, 1.6f, 0.9f}};
    const std::vector<float> first = soup(rng, n), second = soup(rng, 37);
    CHECK(rt_scene_builder_create(&s.b) == RT_OK, "a builder");
    bool ok = rt_scene_add_sphere(s.b, c0, 0.3f, &m) == RT_OK && rt_scene_add_mesh(s.b, first.data(), n, &m) == RT_OK;
    ok = ok && rt_scene_add_quad(s.b, q[0], q[1], q[2], q[3], &m) == RT_OK && rt_scene_add_cuboid(s.b, cc, 0.3f, 0.2f, 0.4f, &m) == RT_OK;
    ok = ok && add_quad_box(s.b, box_at, 0.25f, &m) && rt_scene_add_mesh(s.b, second.data(), 37, &m) == RT_OK;
    ok = ok && rt_scene_add_triangle(s.b, t[0], t[1], t[2], &m) == RT_OK && rt_scene_add_one_way_quad(s.b, q[3], q[2], q[1], q[0], 1, &m) == RT_OK;
    CHECK(ok && s.finish(), "building the scene");
    const rt_wn_scene<rt_f4> S = s.S();
    const double tol = (double)(s.flat.num_tris + 8) * 8.0 * std::ldexp(1.0, -24);     // a term away from its triangle is good to a few 2^-24; the sum adds them up
    for (int i = 0; i < points; i++) {
        float p[3];
        far_point(rng, p);
        g_points++;
        const float w = rt_wn_point(S, RT_WINDING_SOLIDS, p[0], p[1], p[2]);
        CHECK(std::fabs((double)w - solids64(s, p)) <= tol, "the solids' sum differs from binary64");
        for (int o = 0; o < S.num_objects; o++) {
            const float wo = rt_wn_point(S, o, p[0], p[1], p[2]);
            CHECK(std::fabs((double)wo - object64(s, o, p)) <= tol, "an object's winding number differs from binary64");
        }
    }
    // inside the things that enclose: the sphere, the cuboid, the box of quad faces
    const float in_sphere[3] = {0.35f, 0.25f, 1.85f}, in_cuboid[3] = {-0.35f, 0.3f, 2.4f}, in_box[3] = {0.45f, -0.25f, 2.15f};
    CHECK(rt_wn_point(S, 0, in_sphere[0], in_sphere[1], in_sphere[2]) == 1.0f, "inside the sphere");
    CHECK(rt_wn_point(S, 3, in_cuboid[0], in_cuboid[1], in_cuboid[2]) == 1.0f && rt_wn_point(S, 3, in_sphere[0], in_sphere[1], in_sphere[2]) == 0.0f, "the cuboid");
    const float wb = rt_wn_point(S, 4, in_box[0], in_box[1], in_box[2]);
    CHECK(std::fabs(std::fabs(wb) - 1.0f) < 1e-5f && rt_wn_inside(wb), "inside the box of quad faces: its six flip bits make it whole");
    CHECK(std::fabs((double)wb - object64(s, 4, in_box)) < 1e-5, "the box against binary64");
    // points that are not finite, and the derived values
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[3][3] = {{nan, 0, 0}, {0, inf, 0}, {0, 0, -inf}};
    for (const float *p : {bad[0], bad[1], bad[2]}) {
        const float w = rt_wn_point(S, RT_WINDING_SOLIDS, p[0], p[1], p[2]);
        CHECK(rt_wn_bits(w) == 0x7FC00000u && !rt_wn_inside(w) && rt_wn_sdf(w, RT_HIT_MISS_T) == RT_HIT_MISS_T, "a point that is not finite");
    }
    CHECK(rt_wn_sdf(1.0f, 0.25f) == -0.25f && rt_wn_sdf(-0.75f, 0.25f) == -0.25f && rt_wn_sdf(0.49f, 0.25f) == 0.25f && rt_wn_sdf(0.5f, RT_HIT_MISS_T) == -RT_HIT_MISS_T, "the sign rule");
    return 0;
}

static int check_tetrahedron()
{
    g_case = "a tetrahedron";
    const float v[4][3] = {{0, 0, 2}, {1, 0, 2}, {0, 1, 2}, {0, 0, 3}};
    const int faces[4][3] = {{0, 2, 1}, {0, 1, 3}, {1, 2, 3}, {2, 0, 3}};        // counter-clockwise from outside
    for (int turned = 0; turned < 2; turned++) {
        g_n = turned;
        Scene s;
        const rt_material m = plain();
        std::vector<float> tris;
        for (const int *f : {faces[0], faces[1], faces[2], faces[3]})
            for (int k = 0; k < 3; k++) { const float *p = v[f[turned ? 2 - k : k]]; tris.insert(tris.end(), p, p + 3); }
        CHECK(rt_scene_builder_create(&s.b) == RT_OK && rt_scene_add_mesh(s.b, tris.data(), 4, &m) == RT_OK && s.finish(), "building the scene");
        const rt_wn_scene<rt_f4> S = s.S();
        const float w_in = rt_wn_point(S, 0, 0.2f, 0.2f, 2.2f), w_out = rt_wn_point(S, RT_WINDING_SOLIDS, 2.0f, 2.0f, 2.0f);
        CHECK(std::fabs(w_in - (turned ? -1.0f : 1.0f)) < 1e-5f && rt_wn_inside(w_in), "inside: 1, or -1 for the mesh turned inside out, and enclosed either way");
        CHECK(std::fabs(w_out) < 1e-5f && !rt_wn_inside(w_out), "outside");
        // in a face's plane beside the face, on a vertex, on an edge: the term of that face is 0 by definition, the answer is finite
        const float edge[3][3] = {{5.0f, 5.0f, 2.0f}, {0, 0, 2}, {0.5f, 0, 2}};
        for (const float *p : {edge[0], edge[1], edge[2]}) CHECK(std::isfinite(rt_wn_point(S, 0, p[0], p[1], p[2])), "a point in a face's plane");
    }
    return 0;
}

// ---- the flip bytes of every way to add an object -----------------------------------------------------------------------------------------------
static int check_flip_bytes(std::mt19937 &rng)
{
    g_case = "flip bytes";
    Scene s;
    const rt_material m = plain();
    const float c[3] = {0, 0, 2}, q[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
    const std::vector<float> tris = soup(rng, 50);
    // a file's mesh of quads and triangles in turn: vertices 4 per quad, 3 per triangle
    std::vector<float> verts;
    std::vector<int32_t> idx, arity;
    std::vector<uint8_t> want_commit;
    for (int f = 0; f < 30; f++) {
        const int n = f % 3 == 1 ? 3 : 4;
        arity.push_back(n);
        for (int k = 0; k < n; k++) {
            idx.push_back((int32_t)(verts.size() / 3));
            for (int d = 0; d < 3; d++) verts.push_back(uniform(rng, -1, 1) + (d == 2 ? 2.0f : 0.0f) + 0.01f * (float)f);
        }
        want_commit.push_back(0);
        if (n == 4) want_commit.push_back(1);
    }
    CHECK(rt_scene_builder_create(&s.b) == RT_OK, "a builder");
    rt_obj *o = nullptr;
    bool ok = rt_scene_add_sphere(s.b, c, 0.3f, &m) == RT_OK && rt_scene_add_triangle(s.b, q[0], q[1], q[2], &m) == RT_OK;
    const float nine[9] = {0, 0, 0, 1, 0, 0, 1, 1, 0}, uv[6] = {0, 0, 1, 0, 1, 1};
    ok = ok && rt_scene_add_triangle_uv(s.b, nine, uv, &m) == RT_OK && rt_scene_add_quad(s.b, q[0], q[1], q[2], q[3], &m) == RT_OK;
    ok = ok && rt_scene_add_one_way_quad(s.b, q[0], q[1], q[2], q[3], 0, &m) == RT_OK && rt_scene_add_cuboid(s.b, c, 1, 1, 1, &m) == RT_OK;
    ok = ok && rt_scene_add_mesh(s.b, tris.data(), 50, &m) == RT_OK;
    ok = ok && rt_obj_from_arrays(verts.data(), (int32_t)(verts.size() / 3), idx.data(), arity.data(), 30, &o) == RT_OK && rt_scene_add_obj_mesh(s.b, o, &m) == RT_OK;
    rt_obj_destroy(o);
    CHECK(ok && s.finish(), "building the scene");
    const FlatScene &f = s.flat;
    const int before = 1 + 1 + 2 + 2 + 12 + 50;                                  // records ahead of the file's mesh
    CHECK(f.num_tris == before + (int)want_commit.size() && (int)f.tri_flip.size() == f.num_tris && (int)f.tri_flip_commit.size() == f.num_tris, "one byte per record");
    for (int k = 0; k < before; k++) CHECK(f.tri_flip[(size_t)k] == 0 && f.tri_flip_commit[(size_t)k] == 0, "a record of no file's mesh has no flip");
    int flips = 0;
    for (size_t k = 0; k < want_commit.size(); k++) {
        CHECK(f.tri_flip_commit[(size_t)before + k] == want_commit[k], "the commit-order byte is the construction's");
        const int32_t from = f.tri_order[(size_t)before + k];
        CHECK(from >= 0 && (size_t)from < want_commit.size() && f.tri_flip[(size_t)before + k] == want_commit[(size_t)from], "the flattened byte follows its triangle through the tree build");
        CHECK(rt_wn_flip(s.S(), before, from) == want_commit[(size_t)from], "... and the words give the same bit");
        flips += f.tri_flip[(size_t)before + k];
    }
    CHECK(flips == 20, "twenty quad faces, twenty flips");
    rt_flat_view v{};
    CHECK(rt_debug_flatten(s.b, &v) == RT_OK && v.tri_flip && !std::memcmp(v.tri_flip, f.tri_flip.data(), f.tri_flip.size()), "rt_debug_flatten reports the flattened bytes");
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
    scene.flat.objects.resize(3);
    alignas(16) static rt_nearest rec[2];
    const float pts[6] = {0, 0, 0, 1, 1, 1}, lim[2] = {1, 1};
    float w[2], sdf[2];
    uint8_t in[2];
    for (int form = 0; form < 2; form++) {
        auto wn = [&](rt_ctx *c, rt_scene *s, const float *p, int64_t n, int32_t object, float *ow, uint8_t *oi) {
            return form ? rt_winding_numbers(c, s, p, n, object, ow, oi) : rt_winding_numbers_device(c, s, p, n, object, ow, oi, nullptr);
        };
        auto sd = [&](rt_ctx *c, rt_scene *s, const float *p, const float *l, int64_t n, rt_nearest *r, float *o) {
            return form ? rt_signed_distance(c, s, p, l, n, r, o) : rt_signed_distance_device(c, s, p, l, n, r, o, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(wn(nullptr, &scene, pts, 2, -1, w, in) == RT_ERR_INVALID && wn(nullptr, nullptr, nullptr, 0, -1, nullptr, nullptr) == RT_ERR_INVALID, "null context");
        CHECK(wn(&ctx, nullptr, pts, 2, -1, w, in) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(wn(&ctx, &foreign, pts, 2, -1, w, in) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(wn(&ctx, &scene, pts, -1, -1, w, in) == RT_ERR_INVALID && said(ctx, "point count"), "a negative count");
        CHECK(wn(&ctx, &scene, pts, ((int64_t)1 << 30) + 1, -1, w, in) == RT_ERR_INVALID && said(ctx, "point count"), "more than 2^30 points");
        CHECK(wn(&ctx, &scene, nullptr, 2, -1, w, in) == RT_ERR_INVALID && said(ctx, "null argument"), "null points");
        CHECK(wn(&ctx, &scene, pts, 2, -1, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "both outputs null");
        CHECK(wn(&ctx, &scene, pts, 2, 3, w, in) == RT_ERR_INVALID && said(ctx, "object"), "an object index past the list");
        CHECK(wn(&ctx, &scene, pts, 2, -2, w, in) == RT_ERR_INVALID && said(ctx, "object"), "an object index below RT_WINDING_SOLIDS");
        CHECK(wn(&ctx, &scene, pts, 0, 3, nullptr, nullptr) == RT_ERR_INVALID, "an object index out of range, no points");
        CHECK(wn(&ctx, &scene, nullptr, 0, -1, nullptr, nullptr) == RT_OK && wn(&ctx, &scene, pts, 0, 2, w, in) == RT_OK, "no points: nothing to do");
        CHECK(sd(nullptr, &scene, pts, lim, 2, rec, sdf) == RT_ERR_INVALID, "null context");
        CHECK(sd(&ctx, nullptr, pts, lim, 2, rec, sdf) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(sd(&ctx, &foreign, pts, lim, 2, rec, sdf) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(sd(&ctx, &scene, pts, lim, -1, rec, sdf) == RT_ERR_INVALID && said(ctx, "point count"), "a negative count");
        CHECK(sd(&ctx, &scene, pts, lim, ((int64_t)1 << 30) + 1, rec, sdf) == RT_ERR_INVALID && said(ctx, "point count"), "more than 2^30 points");
        CHECK(sd(&ctx, &scene, nullptr, lim, 2, rec, sdf) == RT_ERR_INVALID && said(ctx, "null argument"), "null points");
        CHECK(sd(&ctx, &scene, pts, lim, 2, rec, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null sdf");
        CHECK(sd(&ctx, &scene, nullptr, nullptr, 0, nullptr, nullptr) == RT_OK, "no points: nothing to do");
    }
    CHECK(rt_signed_distance_device(&ctx, &scene, pts, nullptr, 2, (rt_nearest *)((char *)rec + 4), sdf, nullptr) == RT_ERR_INVALID && said(ctx, "16-byte aligned"), "misaligned records");
    CHECK(g_launches == 0, "a refused call reached a launcher");
    CHECK(!ctx.launched && !ctx.have_timing && ctx.last_stream == nullptr, "a refused call touched the launch order");
    CHECK(!scene.d_perm.p && !scene.d_flip.p, "a refused call prepared the scene");
    return 0;
}

// ---- the order list when the device gives no memory ----------------------------------------------------------------------------------------
static int perm_helper()
{
    g_case = "the order list";
    rt_ctx ctx;
    rt_scene scene;
    scene.ctx = &ctx;
    scene.flat.tri_order = {0, 2, 1, 0};
    const rt_status st = ensure_scene_perm(&ctx, &scene);
    if (st != RT_OK) {                     // no device, or no memory: the scene is as it was and says why
        CHECK(st == RT_ERR_HIP && !scene.d_perm.p && scene.d_perm.cap == 0 && said(ctx, "triangle order"), "a failed allocation leaves the scene without the list");
        CHECK(ensure_scene_perm(&ctx, &scene) == RT_ERR_HIP && !scene.d_perm.p, "... and the next call tries again");
    } else {
        CHECK(scene.d_perm.p && scene.d_perm.cap == 4, "the list is there");
        int32_t *const made = scene.d_perm.p;
        CHECK(ensure_scene_perm(&ctx, &scene) == RT_OK && scene.d_perm.p == made, "made once");
    }
    return 0;
}

int main(int argc, char **argv)
{
    // no device for this process, wherever it runs: the one HIP call it makes (the order list's allocation) is meant to be refused
    setenv("HIP_VISIBLE_DEVICES", "-1", 1);
    setenv("ROCR_VISIBLE_DEVICES", "-1", 1);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int points = argc > 2 ? std::atoi(argv[2]) : 100;
    std::mt19937 rng(seed);
    for (int n : {1, 2, 3, 7, 64, 500, 1025})
        if (check_soups(rng, n, n > 400 ? points / 4 + 1 : points)) return 1;
    if (check_tetrahedron() || check_flip_bytes(rng) || refusals() || perm_helper()) return 1;
    std::printf("winding host side: %ld points, %ld binary64 terms, sanitizers silent\n", g_points, g_terms);
    return 0;
}
