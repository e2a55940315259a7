// The fast winding numbers (rt_winding_numbers_fast[_device], rt_signed_distance_fast[_device]: rt_winding.h, rt_winding_capi.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. the builder of rt_winding.h on meshes of 0 to 1025 triangles - around the leaf size above all - with random centroids, ties and NaNs: every
//      triangle in exactly one leaf, leaves of 1 .. RT_WINDING_LEAF_TRIS, preorder with consistent skip, the lists of the refit;
//   2. the builder, the gather, the moments and the walk - rt_winding.h's text, what the kernels compile - as plain host code through
//      rt_debug_winding_tree on seeded random meshes, against a straightforward binary64 sum of solid angles: with beta = inf within the exact
//      query's tolerance (the same terms in cluster order); with beta = 2 within the bound the triangle inequality gives for points from which the
//      whole mesh is far, sum(area) * (1 / dmin^2 + 1 / dc^2) / (4 pi) - crude, but a wrong sign, a wrong scale or a wrong centre breaks it;
//      objects that are no meshes answer with rt_wn_point's bits; a degenerate mesh of zero area answers 0;
//   3. every refusal of the four entry points, on a context and scenes built in host memory (nothing gets as far as the launchers);
//   4. the scene's trees under an allocation that fails (the program hides every device from itself): the scene is left as it was.
//   winding_fast_host_check <seed> <points per scene>
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

#define CHECK(cond, what)                                                                                  \
    do {                                                                                                   \
        if (!(cond)) { std::fprintf(stderr, "fast winding check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_points = 0, g_clusters = 0;

static float uniform(std::mt19937 &rng, float lo, float hi) { return lo + (hi - lo) * (float)(rng() % 1000001) / 1000000.0f; }

static rt_material plain()
{
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    rt_material m;
    rt_material_standard(&m, grey, 0.2f);
    return m;
}

// ---- 1. the builder alone ------------------------------------------------------------------------------------------------------------------
static int subtree(const rt_wn_tree &T, int32_t c, int32_t end, int32_t base, std::vector<int> &seen, int &tris)
{
    CHECK(c >= 0 && (size_t)c < T.skip.size() && T.skip[(size_t)c] == end, "a skip index does not close its subtree");
    if (T.count[(size_t)c] > 0) {
        const int32_t first = T.first[(size_t)c], count = T.count[(size_t)c];
        CHECK(count <= RT_WINDING_LEAF_TRIS && end == c + 1 && first >= base && (size_t)(first - base + count) <= seen.size(), "a leaf's range");
        for (int32_t k = 0; k < count; k++) seen[(size_t)(first - base + k)]++;
        tris = count;
        return 0;
    }
    CHECK(c + 1 < end, "an internal cluster without children");
    const int32_t right = T.skip[(size_t)c + 1];
    CHECK(right > c + 1 && right < end, "an internal cluster without a right child");
    int l = 0, r = 0;
    if (subtree(T, c + 1, right, base, seen, l) || subtree(T, right, end, base, seen, r)) return 1;
    CHECK(l == (l + r + 1) / 2 && l + r > RT_WINDING_LEAF_TRIS, "the split is not the median's");
    CHECK(T.height[(size_t)c] == 1 + std::max(T.height[(size_t)c + 1], T.height[(size_t)right]), "a height");
    tris = l + r;
    return 0;
}

static int check_builder(std::mt19937 &rng, int n)
{
    g_case = "the builder";
    g_n = n;
    const int32_t base = 5;                                            // the mesh is the second object: five records of others ahead of it
    std::vector<float> centroids((size_t)n * 3);
    for (float &c : centroids) c = rng() % 7 == 0 ? 0.5f : uniform(rng, -1, 1);      // ties
    if (n > 3) centroids[4] = std::numeric_limits<float>::quiet_NaN();
    rt_wn_tree T;
    rt_wn_tree_init(T, 3, base + n + 2);
    rt_wn_build_mesh(T, 1, centroids.data(), n, base);
    rt_wn_tree_finish(T);
    const int32_t c0 = T.object_range[2], c1 = T.object_range[3];
    CHECK(c0 == 0 && c1 == (int32_t)T.skip.size() && (n > 0) == (c1 > 0) && T.object_range[0] == 0 && T.object_range[1] == 0 && T.object_range[5] == 0, "the objects' ranges");
    std::vector<int> seen((size_t)n, 0), commit((size_t)n, 0);
    int tris = 0;
    if (n > 0 && subtree(T, 0, c1, base, seen, tris)) return 1;
    CHECK(tris == n, "the root holds every triangle");
    for (int k = 0; k < n; k++) {
        CHECK(seen[(size_t)k] == 1, "a cluster position is in no leaf, or in two");
        const int32_t from = T.order[(size_t)base + k];
        CHECK(from >= 0 && from < n && T.inv[(size_t)base + from] == base + k, "order and its inverse");
        commit[(size_t)from]++;
    }
    for (int k = 0; k < n; k++) CHECK(commit[(size_t)k] == 1, "order is no permutation");
    CHECK(T.levels.size() == T.skip.size() && T.level_off.front() == 0 && (size_t)T.level_off.back() == T.skip.size(), "the refit's lists");
    for (size_t h = 0; h + 1 < T.level_off.size(); h++)
        for (int32_t k = T.level_off[h]; k < T.level_off[h + 1]; k++) CHECK(T.height[(size_t)T.levels[(size_t)k]] == (int32_t)h, "a cluster listed under another height");
    g_clusters += (long)T.skip.size();
    return 0;
}

// ---- 2. the whole host text against binary64 -----------------------------------------------------------------------------------------------
struct Scene {
    rt_scene_builder *b = nullptr;
    rt_flat_view flat{};
    rt_winding_tree_view tree{};
    std::vector<rt_f4> topo, moments, rec;
    Scene() = default;
    Scene(const Scene &) = delete;
    ~Scene() { rt_scene_builder_destroy(b); }
    const rt_f4 *tris() const { return reinterpret_cast<const rt_f4 *>(flat.blob) + flat.off_tris; }
    const rt_object &object(int i) const { return static_cast<const rt_object *>(flat.objects)[i]; }
    int end_of(int i) const { return i + 1 < flat.num_objects ? object(i + 1).prim_start : flat.num_triangles; }
    // the views, and from them alone what a walk reads: the records gathered by `position`, the flip bit from the flattened bytes
    bool finish()
    {
        if (rt_debug_winding_tree(b, &tree) != RT_OK || rt_debug_flatten(b, &flat) != RT_OK) return false;
        if (tree.num_objects != flat.num_objects || tree.num_triangles != flat.num_triangles) return false;
        const size_t nc = (size_t)tree.num_clusters, nt = (size_t)flat.num_triangles;
        topo.assign(nc + 1, rt_f4{0, 0, 0, 0});
        moments.assign(2 * nc + 1, rt_f4{0, 0, 0, 0});
        rec.assign(3 * nt + 1, rt_f4{0, 0, 0, 0});
        for (size_t i = 0; i < nc; i++) {
            topo[i] = rt_f4{rt_wn_float((uint32_t)tree.skip[i]), rt_wn_float((uint32_t)tree.first[i]), rt_wn_float((uint32_t)tree.count[i]), 0.0f};
            std::memcpy(&moments[2 * i], tree.moments + 8 * i, 32);
        }
        for (int o = 0; o < flat.num_objects; o++) {
            if (object(o).type != RT_OBJ_MESH) continue;
            for (int k = object(o).prim_start; k < end_of(o); k++) {
                const int32_t at = tree.position[k];
                if (at < object(o).prim_start || at >= end_of(o)) return false;
                rec[3 * (size_t)k] = tris()[3 * (size_t)at];
                rec[3 * (size_t)k + 1] = tris()[3 * (size_t)at + 1];
                rec[3 * (size_t)k + 2] = rt_f4{tris()[3 * (size_t)at + 2].x, rt_wn_float(flat.tri_flip[at]), 0.0f, 0.0f};
            }
        }
        return true;
    }
    rt_wn_fast<rt_f4> T(float beta) const
    {
        rt_wn_fast<rt_f4> t;
        t.topo = topo.data(); t.moments = moments.data(); t.rec = rec.data(); t.object_range = tree.object_range; t.beta2 = beta * beta;
        return t;
    }
};

static double angle64(const rt_f4 *t, const double p[3], double *area, double *dmin)
{
    const double p0[3] = {t[0].x, t[0].y, t[0].z}, s1[3] = {t[0].w, t[1].x, t[1].y}, s2[3] = {t[1].z, t[1].w, t[2].x};
    double a[3], b[3], c[3];
    for (int k = 0; k < 3; k++) { a[k] = p0[k] - p[k]; b[k] = a[k] + s1[k]; c[k] = a[k] + s2[k]; }
    auto dot = [](const double *u, const double *v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; };
    const double la = std::sqrt(dot(a, a)), lb = std::sqrt(dot(b, b)), lc = std::sqrt(dot(c, c));
    const double n[3] = {s1[1] * s2[2] - s1[2] * s2[1], s1[2] * s2[0] - s1[0] * s2[2], s1[0] * s2[1] - s1[1] * s2[0]};
    const double det = dot(a, n), den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la;
    *area += 0.5 * std::sqrt(dot(n, n));
    // (the nearest point of a triangle is no farther than its nearest corner less its longest edge: a lower bound is all the check needs)
    const double edge = std::fmax(std::sqrt(dot(s1, s1)), std::sqrt(dot(s2, s2)));
    *dmin = std::fmin(*dmin, std::fmin(la, std::fmin(lb, lc)) - edge);
    return det == 0.0 ? 0.0 : std::atan2(det, den);
}

// mesh object i in binary64 from the flattened view alone; area and dmin: the mesh's area and a lower bound of its distance from p
static double mesh64(const Scene &s, int i, const float pf[3], double *area, double *dmin)
{
    const double p[3] = {pf[0], pf[1], pf[2]};
    double A = 0.0;
    for (int k = s.object(i).prim_start; k < s.end_of(i); k++) {
        const double t = angle64(s.tris() + 3 * (size_t)k, p, area, dmin);
        A += s.flat.tri_flip[k] ? -t : t;
    }
    return A / (2.0 * 3.14159265358979323846);
}

static std::vector<float> soup(std::mt19937 &rng, int n, bool degenerate)
{
    std::vector<float> t((size_t)n * 9);
    for (int i = 0; i < n; i++) {
        const float c[3] = {uniform(rng, -0.7f, 0.7f), uniform(rng, -0.7f, 0.7f), uniform(rng, 1.3f, 2.7f)};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) t[(size_t)i * 9 + v * 3 + k] = c[k] + (degenerate ? 0.0f : uniform(rng, -0.15f, 0.15f));
    }
    return t;
}

static void far_point(std::mt19937 &rng, float p[3])
{
    for (;;) {                             // on a shell of radius 4 to 7 around the soups' middle: the whole mesh (radius below 1.3) is far at beta = 2
        const float d[3] = {uniform(rng, -1, 1), uniform(rng, -1, 1), uniform(rng, -1, 1)};
        const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (l < 0.2f || l > 1.0f) continue;
        const float r = uniform(rng, 4.0f, 7.0f) / l;
        p[0] = d[0] * r; p[1] = d[1] * r; p[2] = 2.0f + d[2] * r;
        return;
    }
}

static int check_soups(std::mt19937 &rng, int n, int points, bool degenerate)
{
    g_case = degenerate ? "a mesh of zero area" : "random meshes";
    g_n = n;
    Scene s;
    const rt_material m = plain();
    const float c0[3] = {0.3f, 0.2f, 1.8f}, cc[3] = {-0.5f, 0.4f, 2.2f};
    const float q[4][3] = {{-3, -1, -1}, {3, -1, -1}, {3, -1, 7}, {-3, -1, 7}};
    const std::vector<float> first = soup(rng, n, degenerate), second = soup(rng, 37, false);
    CHECK(rt_scene_builder_create(&s.b) == RT_OK, "a builder");
    bool ok = rt_scene_add_sphere(s.b, c0, 0.3f, &m) == RT_OK && rt_scene_add_mesh(s.b, first.data(), n, &m) == RT_OK;
    ok = ok && rt_scene_add_quad(s.b, q[0], q[1], q[2], q[3], &m) == RT_OK && rt_scene_add_cuboid(s.b, cc, 0.3f, 0.2f, 0.4f, &m) == RT_OK;
    ok = ok && rt_scene_add_mesh(s.b, second.data(), 37, &m) == RT_OK;
    CHECK(ok && s.finish(), "building the scene and its views");
    rt_wn_scene<rt_f4> S;
    S.tris = s.tris(); S.objtab = reinterpret_cast<const rt_f4 *>(s.flat.blob) + (s.flat.off_tris - 3 * s.flat.num_objects);
    S.perm = nullptr; S.flip = nullptr; S.num_objects = s.flat.num_objects; S.num_tris = s.flat.num_triangles;    // (the fast path reads neither list for a mesh)
    const float inf = std::numeric_limits<float>::infinity();
    const rt_wn_fast<rt_f4> Tinf = s.T(inf), T2 = s.T(2.0f);
    const double tol = (double)(s.flat.num_triangles + 8) * 8.0 * std::ldexp(1.0, -24);
    for (int i = 0; i < points; i++) {
        float p[3];
        far_point(rng, p);
        g_points++;
        for (int o : {1, 4}) {
            double area = 0.0, dmin = 1e30;
            const double want = mesh64(s, o, p, &area, &dmin);
            const float w_inf = rt_wn_point_fast(S, Tinf, o, p[0], p[1], p[2]), w2 = rt_wn_point_fast(S, T2, o, p[0], p[1], p[2]);
            CHECK(std::fabs((double)w_inf - want) <= tol, "beta = inf differs from binary64's exact sum");
            if (degenerate && o == 1) {
                CHECK(w2 == 0.0f && w_inf == 0.0f && want == 0.0, "a mesh of zero area subtends nothing");
                continue;
            }
            const rt_f4 c = s.moments[2 * (size_t)s.tree.object_range[2 * o]];
            const double dc2 = ((double)c.x - p[0]) * ((double)c.x - p[0]) + ((double)c.y - p[1]) * ((double)c.y - p[1]) + ((double)c.z - p[2]) * ((double)c.z - p[2]);
            CHECK(dmin > 1.0 && dc2 > 4.0 * (double)c.w, "the point is not far from the whole mesh");
            CHECK(std::fabs((double)w2 - want) <= area * (1.0 / (dmin * dmin) + 1.0 / dc2) / (4.0 * 3.14159265358979323846) + tol, "beta = 2 is farther from binary64 than the far field allows");
        }
        for (int o : {0, 2, 3}) {
            const float a = rt_wn_point_fast(S, T2, o, p[0], p[1], p[2]), b = rt_wn_point(S, o, p[0], p[1], p[2]);
            CHECK(rt_wn_bits(a) == rt_wn_bits(b), "an object that is no mesh answers with the exact query's bits");
        }
    }
    // points near and inside the soup, where the walk goes down to the leaves: beta = inf still is the exact sum, beta = 2 is finite
    for (int i = 0; i < points; i++) {
        const float p[3] = {uniform(rng, -1, 1), uniform(rng, -1, 1), uniform(rng, 1, 3)};
        CHECK(std::isfinite(rt_wn_point_fast(S, T2, RT_WINDING_SOLIDS, p[0], p[1], p[2])) && std::isfinite(rt_wn_point_fast(S, Tinf, 1, p[0], p[1], p[2])), "a point near the mesh");
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(rt_wn_bits(rt_wn_point_fast(S, T2, 1, nan, 0, 0)) == 0x7FC00000u && rt_wn_bits(rt_wn_point_fast(S, Tinf, 4, 0, inf, 0)) == 0x7FC00000u, "a point that is not finite");
    return 0;
}

// ---- 3. the refusals -----------------------------------------------------------------------------------------------------------------------
static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

static int refusals()
{
    g_case = "refusals";
    rt_ctx ctx, other;
    rt_scene scene, foreign;
    scene.ctx = &ctx; foreign.ctx = &other;
    scene.flat.objects.resize(3);
    alignas(16) static rt_nearest rec[2];
    const float pts[6] = {0, 0, 0, 1, 1, 1}, lim[2] = {1, 1}, B = RT_WINDING_BETA_DEFAULT;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    float w[2], sdf[2];
    uint8_t in[2];
    for (int form = 0; form < 2; form++) {
        auto wn = [&](rt_ctx *c, rt_scene *s, const float *p, int64_t n, int32_t object, float beta, float *ow, uint8_t *oi) {
            return form ? rt_winding_numbers_fast(c, s, p, n, object, beta, ow, oi) : rt_winding_numbers_fast_device(c, s, p, n, object, beta, ow, oi, nullptr);
        };
        auto sd = [&](rt_ctx *c, rt_scene *s, const float *p, const float *l, int64_t n, float beta, rt_nearest *r, float *o) {
            return form ? rt_signed_distance_fast(c, s, p, l, n, beta, r, o) : rt_signed_distance_fast_device(c, s, p, l, n, beta, r, o, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(wn(nullptr, &scene, pts, 2, -1, B, w, in) == RT_ERR_INVALID, "null context");
        CHECK(wn(&ctx, nullptr, pts, 2, -1, B, w, in) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(wn(&ctx, &foreign, pts, 2, -1, B, w, in) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(wn(&ctx, &scene, pts, -1, -1, B, w, in) == RT_ERR_INVALID && said(ctx, "point count"), "a negative count");
        CHECK(wn(&ctx, &scene, pts, ((int64_t)1 << 30) + 1, -1, B, w, in) == RT_ERR_INVALID && said(ctx, "point count"), "more than 2^30 points");
        CHECK(wn(&ctx, &scene, nullptr, 2, -1, B, w, in) == RT_ERR_INVALID && said(ctx, "null argument"), "null points");
        CHECK(wn(&ctx, &scene, pts, 2, -1, B, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "both outputs null");
        CHECK(wn(&ctx, &scene, pts, 2, 3, B, w, in) == RT_ERR_INVALID && said(ctx, "object"), "an object index past the list");
        CHECK(wn(&ctx, &scene, pts, 2, -2, B, w, in) == RT_ERR_INVALID && said(ctx, "object"), "an object index below RT_WINDING_SOLIDS");
        for (float beta : {0.0f, -0.0f, -1.0f, nan, -inf}) {
            CHECK(wn(&ctx, &scene, pts, 2, -1, beta, w, in) == RT_ERR_INVALID && said(ctx, "beta"), "a beta that is not above zero");
            CHECK(wn(&ctx, &scene, pts, 0, -1, beta, w, in) == RT_ERR_INVALID, "a bad beta, no points");
            CHECK(sd(&ctx, &scene, pts, lim, 2, beta, rec, sdf) == RT_ERR_INVALID && said(ctx, "beta"), "a beta that is not above zero");
        }
        CHECK(wn(&ctx, &scene, nullptr, 0, -1, B, nullptr, nullptr) == RT_OK && wn(&ctx, &scene, pts, 0, 2, inf, w, in) == RT_OK, "no points: nothing to do");
        CHECK(sd(nullptr, &scene, pts, lim, 2, B, rec, sdf) == RT_ERR_INVALID, "null context");
        CHECK(sd(&ctx, nullptr, pts, lim, 2, B, rec, sdf) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(sd(&ctx, &foreign, pts, lim, 2, B, rec, sdf) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(sd(&ctx, &scene, pts, lim, -1, B, rec, sdf) == RT_ERR_INVALID && said(ctx, "point count"), "a negative count");
        CHECK(sd(&ctx, &scene, nullptr, lim, 2, B, rec, sdf) == RT_ERR_INVALID && said(ctx, "null argument"), "null points");
        CHECK(sd(&ctx, &scene, pts, lim, 2, B, rec, nullptr) == RT_ERR_INVALID && said(ctx, "null argument"), "null sdf");
        CHECK(sd(&ctx, &scene, nullptr, nullptr, 0, B, nullptr, nullptr) == RT_OK, "no points: nothing to do");
    }
    CHECK(rt_signed_distance_fast_device(&ctx, &scene, pts, nullptr, 2, B, (rt_nearest *)((char *)rec + 4), sdf, nullptr) == RT_ERR_INVALID && said(ctx, "16-byte aligned"), "misaligned records");
    CHECK(g_launches == 0, "a refused call reached a launcher");
    CHECK(!ctx.launched && !ctx.have_timing && ctx.last_stream == nullptr, "a refused call touched the launch order");
    CHECK(!scene.d_perm.p && !scene.d_flip.p && !scene.wn_built && !scene.d_wn_topo.p && scene.wn_tree.skip.empty(), "a refused call prepared the scene");
    return 0;
}

// ---- 4. the trees when the device gives nothing ----------------------------------------------------------------------------------------------
static int no_device()
{
    g_case = "the trees without a device";
    rt_ctx ctx;
    rt_scene scene;
    scene.ctx = &ctx;
    scene.flat.objects.resize(1);
    scene.flat.objects[0].type = RT_OBJ_SPHERE;
    const float pts[3] = {0, 0, 0};
    float w[1];
    rt_winding_tree_view v{};
    for (int round = 0; round < 2; round++) {          // (the second call tries again, and fails the same way)
        const rt_status st = rt_winding_numbers_fast_device(&ctx, &scene, pts, 1, RT_WINDING_SOLIDS, 2.0f, w, nullptr, nullptr);
        CHECK(st == RT_ERR_HIP && !ctx.err.empty(), "a valid call without a device is a HIP error");
        CHECK(!scene.wn_built && scene.wn_stale && !scene.d_wn_topo.p && !scene.d_wn_ints.p && !scene.d_wn_rec.p && !scene.d_wn_sums.p && !scene.d_wn_moments.p && scene.wn_tree.skip.empty(),
              "a failed preparation leaves the scene as it was: no trees, no buffers");
        CHECK(rt_debug_scene_winding_tree(&ctx, &scene, &v) == RT_ERR_HIP && !scene.wn_built, "the debug view fails the same way");
    }
    CHECK(g_launches == 0 && !ctx.launched, "nothing was launched");
    return 0;
}

int main(int argc, char **argv)
{
    // no device for this process, wherever it runs: the HIP calls it makes are meant to be refused
    setenv("HIP_VISIBLE_DEVICES", "-1", 1);
    setenv("ROCR_VISIBLE_DEVICES", "-1", 1);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int points = argc > 2 ? std::atoi(argv[2]) : 100;
    std::mt19937 rng(seed);
    for (int n : {0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65, 500, 1025})
        if (check_builder(rng, n)) return 1;
    for (int n : {1, 7, 8, 9, 16, 17, 64, 500})
        if (check_soups(rng, n, n > 400 ? points / 4 + 1 : points, false)) return 1;
    for (int n : {1, 9, 40})
        if (check_soups(rng, n, points / 4 + 1, true)) return 1;
    if (refusals() || no_device()) return 1;
    std::printf("fast winding host side: %ld points, %ld clusters built, sanitizers silent\n", g_points, g_clusters);
    return 0;
}
