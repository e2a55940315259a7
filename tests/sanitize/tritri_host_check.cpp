// The triangle-overlap queries (rt_overlap_triangles[_device]: rt_tritri.h, rt_tritri_capi.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. the kernel's traversal as plain host code - the steps of rt_tritri.h and rt_overlap.h (rt_tt_begin, rt_tt_simple, rt_ov_mesh_begin,
//      rt_tt_step, rt_ov_insert, rt_tt_segment), the text the kernel compiles, on a stack of exactly the scene's stack_entries - against
//      the EXHAUSTIVE loop over every candidate (every sphere, every triangle record, a mesh's triangles under the path flags of a plain
//      recursion over its whole tree; the ids sorted, not inserted), as bytes: seeded random and adversarial queries - a query vertex on
//      a mesh vertex, a mesh triangle itself as the query (the coplanar path), zero-area queries, queries that hold the scene, identical
//      triangles and every triangle four times, zero-area triangles, meshes of 1 to 9 triangles and of about 1,024, queries that are not
//      finite, k from 0 to 8, and the any-only walk;
//   2. every refusal of both entry points, on a context and scenes built in host memory (nothing gets as far as a HIP call or the launcher).
//   tritri_host_check <seed> <queries per scene>
// A second form answers a scene from a file, for tests/test_tritri_host.py to set against the NumPy yardstick:
//   tritri_host_check file <in> <out>   in: int32 blob_f4, off_nodes, off_tris, off_meshes, num_meshes, num_objects, stack_entries, n, k;
//                                           the blob; n x 9 floats.   out: n int32 counts; n bytes; n * k ids; n * k segments
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "rt_tritri.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                               \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "tritri check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_steps = 0, g_skipped_meshes = 0, g_queries = 0, g_touching = 0, g_overflowed = 0, g_path_bites = 0, g_coplanar = 0, g_segments = 0;

struct Flat {
    const rt_f4 *blob;
    int off_nodes, off_tris, off_meshes, off_objtab, num_meshes, num_objects, stack_entries;
    rt_ov_scene<rt_f4> S() const
    {
        rt_ov_scene<rt_f4> s;
        s.nodes = blob + off_nodes; s.tris = blob + off_tris; s.meshes = blob + off_meshes; s.objtab = blob + off_objtab;
        return s;
    }
};

static Flat flat_of(const rt_flat_view &v)
{
    return Flat{(const rt_f4 *)v.blob, v.off_nodes, v.off_tris, v.off_meshes, v.off_meshes + 2 * v.num_meshes, v.num_meshes, v.num_objects, v.stack_entries};
}

struct Answer {
    int32_t count;
    uint8_t any;
    rt_overlap_id ids[RT_OVERLAP_MAX];
    rt_tri_segment segs[RT_OVERLAP_MAX];
};

static rt_tt_tri tri_of(const float q[9])
{
    rt_tt_tri t;
    std::memset(&t, 0, sizeof t);
    t.a0x = q[0]; t.a0y = q[1]; t.a0z = q[2]; t.a1x = q[3]; t.a1y = q[4]; t.a1z = q[5]; t.a2x = q[6]; t.a2y = q[7]; t.a2z = q[8];
    return t;
}

// ---- the kernel's path: one lane, the steps in a plain loop -------------------------------------------------------------------------------
static Answer walk(const Flat &f, const float q[9], int32_t k, bool any_only)
{
    const rt_ov_scene<rt_f4> S = f.S();
    rt_tt_tri t = tri_of(q);
    rt_ov_buf buf;
    rt_ov_clear(buf);
    if (rt_tt_begin(t)) {
        rt_tt_simple(S, f.num_objects, t, k, any_only, buf);
        std::vector<uint32_t> stack((size_t)f.stack_entries * 2);          // exactly what the scene sizes, in 8-byte units: one entry more is the sanitizer's to find
        for (int m = 0; m < f.num_meshes && !(any_only && buf.total > 0u); m++) {
            rt_ov_walk w;
            if (!rt_ov_mesh_begin(S.meshes[2 * m], S.meshes[2 * m + 1], t.box, w)) { g_skipped_meshes++; continue; }
            const int32_t object = (int32_t)rt_ov_bits(S.meshes[2 * m + 1].w);
            while (rt_tt_step<1>(S, stack.data(), object, t, k, buf, w)) {
                g_steps++;
                if (any_only && buf.total > 0u) break;
            }
        }
    }
    Answer a;
    std::memset(&a, 0, sizeof a);
    a.count = (int32_t)buf.total;
    a.any = buf.total > 0u ? 1 : 0;
    for (int r = 0; r < RT_OVERLAP_MAX; r++) {
        const bool held = r < k && (uint32_t)r < buf.total;
        a.ids[r] = rt_ov_id(buf.id[r], held);
        a.segs[r] = rt_tt_segment(S, buf.id[r], held, t);
    }
    return a;
}

// ---- the definition: every candidate ------------------------------------------------------------------------------------------------------
static void every_triangle(const Flat &f, uint32_t ref, bool path, int32_t object, const rt_tt_tri &t, std::vector<uint32_t> &found)
{
    const rt_ov_scene<rt_f4> S = f.S();
    if (ref & RT_REF_LEAF) {
        const int start = (int)(ref & RT_REF_START_MASK), count = (int)((ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        for (int j = count - 1; j >= 0; j--) {                              // (backwards: not the walk's order)
            const rt_f4 *r = S.tris + 3 * (size_t)(start + j);
            const bool bare = rt_tt_test(r[0], r[1], r[2], t);
            if (bare && !path) g_path_bites++;
            if (bare && path) found.push_back(rt_ov_word(object, (uint32_t)(start + j)));
        }
        return;
    }
    const rt_f4 *n = S.nodes + 4 * (size_t)(ref & RT_REF_NODE_MASK);
    const bool ol = rt_ov_boxes(n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, t.box);
    const bool orr = rt_ov_boxes(n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w, t.box);
    every_triangle(f, rt_ov_bits(n[3].y), path && orr, object, t, found);         // (right first, and into subtrees off the path: the whole tree)
    every_triangle(f, rt_ov_bits(n[3].x), path && ol, object, t, found);
}

static Answer exhaustive(const Flat &f, const float q[9], int32_t k)
{
    const rt_ov_scene<rt_f4> S = f.S();
    rt_tt_tri t = tri_of(q);
    std::vector<uint32_t> found;
    if (rt_tt_begin(t)) {
        for (int i = f.num_objects - 1; i >= 0; i--) {                      // (backwards: not the walk's order)
            const int32_t type = (int32_t)rt_ov_bits(S.objtab[3 * i].x), prim = (int32_t)rt_ov_bits(S.objtab[3 * i].y);
            if (type == RT_OBJ_MESH) continue;
            if (type == RT_OBJ_SPHERE) {
                const rt_f4 ob1 = S.objtab[3 * i + 1];
                if (rt_tt_sphere<rt_f4>(ob1.x, ob1.y, ob1.z, ob1.w, t)) found.push_back(rt_ov_word(i, RT_MH_NO_TRI));
                continue;
            }
            for (int j = 0; j < rt_ov_object_tris(type); j++) {
                const rt_f4 *r = S.tris + 3 * (size_t)(prim + j);
                if (rt_tt_test(r[0], r[1], r[2], t)) found.push_back(rt_ov_word(i, (uint32_t)(prim + j)));
            }
        }
        for (int m = 0; m < f.num_meshes; m++) {
            const rt_f4 m0 = S.meshes[2 * m], m1 = S.meshes[2 * m + 1];
            every_triangle(f, rt_ov_bits(m1.z), rt_ov_boxes(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, t.box), (int32_t)rt_ov_bits(m1.w), t, found);
        }
    }
    std::sort(found.begin(), found.end());
    Answer a;
    std::memset(&a, 0, sizeof a);
    a.count = (int32_t)found.size();
    a.any = found.empty() ? 0 : 1;
    for (int r = 0; r < RT_OVERLAP_MAX; r++) {
        const bool held = r < k && (size_t)r < found.size();
        const uint32_t word = held ? found[(size_t)r] : RT_OV_EMPTY;
        a.ids[r].object = held ? (int32_t)(word >> 20) : -1;
        a.ids[r].triangle = held ? ((word & RT_MH_NO_TRI) == RT_MH_NO_TRI ? -1 : (int32_t)(word & RT_MH_NO_TRI)) : -1;
        a.segs[r] = rt_tt_segment(S, word, held, t);
    }
    return a;
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

static bool same(const Answer &a, const Answer &b)
{
    return a.count == b.count && a.any == b.any && !std::memcmp(a.ids, b.ids, sizeof a.ids) && !std::memcmp(a.segs, b.segs, sizeof a.segs);
}

static void record_vertices(const rt_f4 *r, float v[9])
{
    v[0] = r[0].x; v[1] = r[0].y; v[2] = r[0].z;
    v[3] = r[0].x + r[0].w; v[4] = r[0].y + r[1].x; v[5] = r[0].z + r[1].y;
    v[6] = r[0].x + r[1].z; v[7] = r[0].y + r[1].w; v[8] = r[0].z + r[2].x;
}

static int check_query(const Flat &f, const float q[9], std::mt19937 &rng)
{
    const Answer all = exhaustive(f, q, RT_OVERLAP_MAX);
    g_queries++;
    if (all.count > 0) g_touching++;
    if (all.count > RT_OVERLAP_MAX) g_overflowed++;
    const int32_t k_some = (int32_t)(rng() % (RT_OVERLAP_MAX + 1));
    for (int32_t k = 0; k <= RT_OVERLAP_MAX; k++) {
        if (k != 0 && k != RT_OVERLAP_MAX && k != k_some && g_queries % 16 != 0) continue;        // (every k on every sixteenth query, three of them on the others)
        const Answer w = walk(f, q, k, false), e = exhaustive(f, q, k);
        CHECK(same(w, e), "the walk differs from the exhaustive loop");
        CHECK(e.count == all.count && !std::memcmp(e.ids, all.ids, (size_t)k * sizeof(rt_overlap_id)), "the ids under a smaller k are a prefix");
        for (int r = 1; r < k && r < e.count; r++)
            CHECK(e.ids[r - 1].object < e.ids[r].object || (e.ids[r - 1].object == e.ids[r].object && e.ids[r - 1].triangle < e.ids[r].triangle), "ids ascend");
        for (int r = 0; r < RT_OVERLAP_MAX; r++) {
            const bool held = r < k && r < e.count;
            CHECK(held || (e.ids[r].object == -1 && e.ids[r].triangle == -1 && e.segs[r].kind == 0), "slots past the count");
            CHECK(!held || e.segs[r].kind == 1 || e.segs[r].kind == 2, "a held slot's kind");
            CHECK(!held || e.segs[r].kind != 2 || (e.segs[r].p[0] != e.segs[r].p[0] && e.segs[r].q[2] != e.segs[r].q[2]), "a kind-2 segment's floats are NaN");
            CHECK(!held || e.ids[r].triangle >= 0 || e.segs[r].kind == 2, "a sphere has no segment");
            if (held && e.segs[r].kind == 1) g_segments++;
            if (held && e.segs[r].kind == 2 && e.ids[r].triangle >= 0) g_coplanar++;
        }
    }
    CHECK(walk(f, q, 0, true).any == all.any, "the any-only walk's byte");
    return 0;
}

static int check_scene(const std::vector<float> &tris, const std::vector<float> &second, bool mesh_alone, int queries, std::mt19937 &rng)
{
    Scene s;
    CHECK(make_scene(s, tris, second, mesh_alone), "building the scene");
    const Flat f = flat_of(s.v);
    const int n_tris = s.v.num_triangles;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < queries; i++) {
        float q[9];
        const unsigned kind = rng() % 10;
        const float scale = kind < 3 ? 0.05f : kind < 6 ? 0.3f : 1.0f;
        const float c[3] = {uniform(rng, -1.5f, 1.5f), uniform(rng, -1.5f, 1.5f), uniform(rng, 0.5f, 3.5f)};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) q[v * 3 + k] = c[k] + uniform(rng, -scale, scale);
        if (kind >= 6 && n_tris > 0) {
            float rv[9];
            record_vertices(f.blob + f.off_tris + 3 * (size_t)(rng() % (unsigned)n_tris), rv);
            if (kind == 6) std::memcpy(q, rv + 3 * (rng() % 3), 12);                              // a query vertex on a scene vertex
            else if (kind == 7) std::memcpy(q, rv, 36);                                           // a scene triangle itself: coplanar
            else if (kind == 8) { std::memcpy(q, rv, 24); for (int k = 0; k < 3; k++) q[6 + k] = rv[k] + 0.5f * (rv[3 + k] - rv[k]); }   // zero area, along a scene edge
            else { for (int k = 0; k < 3; k++) { q[k] = rv[k] + (rv[k] - q[3 + k]); } }            // an edge of the query through a scene vertex (up to rounding)
        }
        if (check_query(f, q, rng)) return 1;
    }
    // the whole scene in one triangle's bounding box: the walk enters every leaf
    const float huge[9] = {-60, -60, -60, 60, 60, -60, 0, 0, 80};
    CHECK(same(walk(f, huge, RT_OVERLAP_MAX, false), exhaustive(f, huge, RT_OVERLAP_MAX)), "a query whose box holds the scene");
    const float point[9] = {0.4f, 0.1f, 1.5f, 0.4f, 0.1f, 1.5f, 0.4f, 0.1f, 1.5f};               // the first sphere's centre: inside the ball, not on its surface
    const Answer inner = exhaustive(f, point, RT_OVERLAP_MAX);
    for (int r = 0; r < RT_OVERLAP_MAX; r++) CHECK(!(inner.ids[r].object == 0 && inner.ids[r].triangle == -1 && !mesh_alone), "a triangle wholly inside a ball touches its surface");
    // queries that are not finite overlap nothing
    for (int k = 0; k < 9; k++)
        for (float bad : {nan, inf, -inf}) {
            float q[9];
            std::memcpy(q, huge, sizeof q);
            q[k] = bad;
            CHECK(walk(f, q, 8, false).count == 0 && exhaustive(f, q, 8).count == 0 && walk(f, q, 0, true).any == 0, "a query that is not finite");
        }
    return 0;
}

// ---- the refusals --------------------------------------------------------------------------------------------------------------------------
static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

static int refusals()
{
    g_case = "refusals";
    rt_ctx ctx, other;
    rt_scene scene, foreign, crowded;
    scene.ctx = &ctx; foreign.ctx = &other; crowded.ctx = &ctx;
    crowded.flat.objects.resize(RT_MH_MAX_OBJECTS + 1);
    alignas(16) static rt_overlap_id ids[2 * RT_OVERLAP_MAX + 1];
    alignas(16) static rt_tri_segment segs[2 * RT_OVERLAP_MAX + 1];
    int32_t counts[2] = {-3, -3};
    uint8_t any[2] = {7, 7};
    const float tris[18] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1};
    rt_overlap_id *const misaligned = (rt_overlap_id *)((char *)ids + 4);
    rt_tri_segment *const misaligned_segs = (rt_tri_segment *)((char *)segs + 8);
    for (int form = 0; form < 2; form++) {
        auto call = [&](rt_ctx *c, const rt_scene *s, const float *t, int64_t n, int32_t k, rt_overlap_id *pi, int32_t *pc, uint8_t *pa, rt_tri_segment *ps) {
            return form ? rt_overlap_triangles(c, s, t, n, k, pi, pc, pa, ps) : rt_overlap_triangles_device(c, s, t, n, k, pi, pc, pa, ps, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(call(nullptr, &scene, tris, 2, 2, ids, counts, any, segs) == RT_ERR_INVALID, "null context");
        CHECK(call(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "null context, no triangles");
        CHECK(call(&ctx, nullptr, tris, 2, 2, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(call(&ctx, &foreign, tris, 2, 2, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(call(&ctx, &scene, tris, -1, 2, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "triangle count"), "a negative count");
        CHECK(call(&ctx, &scene, tris, ((int64_t)1 << 30) + 1, 2, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "triangle count"), "more than 2^30 triangles");
        CHECK(call(&ctx, &scene, tris, 2, -1, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "id count"), "k below 0");
        CHECK(call(&ctx, &scene, tris, 2, RT_OVERLAP_MAX + 1, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "id count"), "k above RT_OVERLAP_MAX");
        CHECK(call(&ctx, &scene, tris, 0, RT_OVERLAP_MAX + 1, ids, counts, any, segs) == RT_ERR_INVALID, "k above RT_OVERLAP_MAX without triangles");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, nullptr, 2, 2, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "null argument"), "null triangles");
        CHECK(call(&ctx, &scene, tris, 2, 2, nullptr, counts, any, nullptr) == RT_ERR_INVALID && said(ctx, "null ids"), "null ids while k > 0");
        CHECK(call(&ctx, &scene, tris, 2, 0, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "no output"), "all outputs null");
        CHECK(call(&ctx, &scene, tris, 2, 0, ids, nullptr, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "no output"), "ids alone with k == 0 is no output");
        CHECK(call(&ctx, &scene, tris, 2, 0, nullptr, counts, nullptr, segs) == RT_ERR_INVALID && said(ctx, "segments asked for"), "segments with k == 0");
        CHECK(call(&ctx, &crowded, tris, 2, 2, ids, counts, any, segs) == RT_ERR_INVALID && said(ctx, "too many objects"), "more than 4,096 objects");
        CHECK(call(&ctx, &scene, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr) == RT_OK && call(&ctx, &scene, tris, 0, 2, ids, counts, any, segs) == RT_OK, "no triangles: nothing to do");
    }
    CHECK(rt_overlap_triangles_device(&ctx, &scene, tris, 2, 2, misaligned, counts, any, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "8-byte aligned"), "misaligned d_ids");
    CHECK(rt_overlap_triangles_device(&ctx, &scene, tris, 2, 2, ids, counts, any, misaligned_segs, nullptr) == RT_ERR_INVALID && said(ctx, "16-byte aligned"), "misaligned d_segments");
    CHECK(counts[0] == -3 && counts[1] == -3 && any[0] == 7 && any[1] == 7, "a refused call wrote");
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
    if (std::fread(h, 4, 9, fi) != 9 || h[0] < 0 || h[7] < 0 || h[8] < 0 || h[8] > RT_OVERLAP_MAX) { std::fclose(fi); return 2; }
    const size_t n = (size_t)h[7];
    const int32_t k = h[8];
    std::vector<rt_f4> blob((size_t)h[0] + 1);
    std::vector<float> q(n * 9 + 1);
    const bool read = std::fread(blob.data(), 16, (size_t)h[0], fi) == (size_t)h[0] && std::fread(q.data(), 36, n, fi) == n;
    std::fclose(fi);
    if (!read) return 2;
    const Flat f{blob.data(), h[1], h[2], h[3], h[3] + 2 * h[4], h[4], h[5], h[6]};
    std::vector<int32_t> counts(n + 1);
    std::vector<uint8_t> any(n + 1);
    std::vector<rt_overlap_id> ids(n * (size_t)k + 1);
    std::vector<rt_tri_segment> segs(n * (size_t)k + 1);
    for (size_t i = 0; i < n; i++) {
        const Answer a = walk(f, &q[i * 9], k, false);
        counts[i] = a.count;
        any[i] = walk(f, &q[i * 9], 0, true).any;
        for (int r = 0; r < k; r++) { ids[i * (size_t)k + (size_t)r] = a.ids[r]; segs[i * (size_t)k + (size_t)r] = a.segs[r]; }
    }
    FILE *fo = std::fopen(outp, "wb");
    if (!fo) return 2;
    const size_t records = n * (size_t)k;
    const bool ok = std::fwrite(counts.data(), 4, n, fo) == n && std::fwrite(any.data(), 1, n, fo) == n && std::fwrite(ids.data(), 8, records, fo) == records &&
                    std::fwrite(segs.data(), 32, records, fo) == records;
    std::fclose(fo);
    std::printf("tritri host side: %d queries from a file, %ld steps, sanitizers silent\n", h[7], g_steps);
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(rt_tri_segment) == 32, "the segment");
    if (argc == 4 && !std::strcmp(argv[1], "file")) return from_file(argv[2], argv[3]);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int queries = argc > 2 ? std::atoi(argv[2]) : 200;
    std::mt19937 rng(seed);
    const std::vector<float> second = soup(rng, 37, 0.8f, 0.15f);
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 100, 1023, 1025};
    for (int n : sizes) {
        g_n = n;
        const int count = n > 1000 ? queries / 4 + 1 : queries;
        g_case = "random";
        if (check_scene(soup(rng, n, 0.8f, 0.12f), second, false, count, rng)) return 1;
        g_case = "the mesh alone";
        if (check_scene(soup(rng, n, 0.8f, 0.12f), second, true, count, rng)) return 1;
        // equal geometry under different ids (every triangle the same; every triangle four times), and zero-area triangles among ordinary ones
        std::vector<float> ident = soup(rng, n, 0.8f, 0.12f), dup = soup(rng, n, 0.8f, 0.12f), thin = soup(rng, n, 0.8f, 0.12f);
        for (int i = 0; i < n; i++) {
            std::memcpy(&ident[(size_t)i * 9], &ident[0], 36);
            std::memcpy(&dup[(size_t)i * 9], &dup[(size_t)(i / 4) * 9], 36);
            if (i % 3 == 0) std::memcpy(&thin[(size_t)i * 9 + 3], &thin[(size_t)i * 9], 12);
            if (i % 6 == 0) std::memcpy(&thin[(size_t)i * 9 + 6], &thin[(size_t)i * 9], 12);
        }
        g_case = "identical triangles";
        if (check_scene(ident, second, true, count / 2 + 1, rng)) return 1;
        g_case = "every triangle four times";
        if (check_scene(dup, second, false, count / 2 + 1, rng)) return 1;
        g_case = "zero-area triangles";
        if (check_scene(thin, second, true, count / 2 + 1, rng)) return 1;
    }
    if (refusals()) return 1;
    if (g_touching == 0 || g_overflowed == 0 || g_coplanar == 0 || g_segments == 0) {
        std::fprintf(stderr, "tritri check: no query touched anything, none met more than %d candidates, no coplanar pair or no segment\n", RT_OVERLAP_MAX);
        return 1;
    }
    std::printf("tritri host side: %ld queries on %d sizes of meshes (%ld touch a surface, %ld meet more than %d; %ld segments, %ld coplanar pairs; the path rule alone "
                "decided %ld pairs), %ld steps, %ld meshes skipped at their root box, sanitizers silent\n", g_queries, (int)(sizeof sizes / sizeof sizes[0]), g_touching,
                g_overflowed, RT_OVERLAP_MAX, g_segments, g_coplanar, g_path_bites, g_steps, g_skipped_meshes);
    return 0;
}
