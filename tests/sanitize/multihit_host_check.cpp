// The multi-hit ray queries (rt_trace_rays_multi[_device]: rt_multihit.h, rt_multihit_capi.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. the kernel's walk and insert as plain host code - the steps of rt_multihit.h (rt_mh_begin, rt_mh_simple, rt_mh_mesh_begin, rt_mh_step,
//      rt_mh_insert), the text the kernel compiles, on a stack of exactly the scene's stack_entries - against the EXHAUSTIVE sort over every
//      candidate (every sphere, every face, a mesh's triangles under the path flags and values of a plain recursion over its whole tree, all
//      of them collected, sorted with std::sort by the header's order and cut at k), byte for byte: seeded random and adversarial inputs -
//      identical triangles and every triangle four times (tied keys), rays that start in a box face and run along it, zero direction
//      components, more than 8 candidates along a ray, k from 0 to 8, limits one ulp either side of a key;
//   2. every refusal of both entry points, on a context and scenes built in host memory (nothing gets as far as a HIP call or the launcher).
//   multihit_host_check <seed> <rays per scene>
// A second form answers a scene from a file, for tests/test_multihit_host.py to set against the NumPy yardstick:
//   multihit_host_check file <in> <out>   in: int32 blob_f4, off_nodes, off_tris, off_meshes, num_meshes, num_objects, stack_entries, n, has_limit, k;
//                                             the blob; n x 3 origins; n x 3 directions; n limits if has_limit.
//                                         out: n int32 counts, then n * k records of (float t, int32 object, int32 triangle)
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
#include "rt_multihit.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                             \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "multihit check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_steps = 0, g_skipped_meshes = 0, g_rays = 0, g_overflows = 0, g_ties = 0;

struct Rec { float t; int32_t object, triangle; };
struct Answer { int32_t count; Rec rec[RT_MULTIHIT_MAX]; };

struct Flat {
    const rt_f4 *blob;
    int off_nodes, off_tris, off_meshes, off_objtab, num_meshes, num_objects, stack_entries;
    rt_mh_scene<rt_f4> S() const
    {
        rt_mh_scene<rt_f4> s;
        s.nodes = blob + off_nodes; s.tris = blob + off_tris; s.meshes = blob + off_meshes; s.objtab = blob + off_objtab;
        return s;
    }
};

static Flat flat_of(const rt_flat_view &v)
{
    return Flat{(const rt_f4 *)v.blob, v.off_nodes, v.off_tris, v.off_meshes, v.off_meshes + 2 * v.num_meshes, v.num_meshes, v.num_objects, v.stack_entries};
}

static Answer blank()
{
    Answer a;
    std::memset(&a, 0, sizeof a);
    for (Rec &r : a.rec) { r.t = RT_HIT_MISS_T; r.object = -1; r.triangle = -1; }
    return a;
}

// ---- the kernel's path: one lane, the steps in a plain loop -------------------------------------------------------------------------------
static Answer walk(const Flat &f, const float o[3], const float d[3], bool has_limit, float tmax, int32_t k)
{
    const rt_mh_scene<rt_f4> S = f.S();
    rt_mh_ray r;
    r.ox = o[0]; r.oy = o[1]; r.oz = o[2]; r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
    rt_mh_buf buf;
    rt_mh_clear(buf);
    float lim;
    if (rt_mh_begin(r, has_limit, tmax, lim)) {
        rt_mh_simple(S, f.num_objects, r, lim, k, buf);
        std::vector<rt_mh_entry> stack((size_t)f.stack_entries);          // exactly what the scene sizes: one entry more is the sanitizer's to find
        for (int m = 0; m < f.num_meshes; m++) {
            rt_mh_walk w;
            if (!rt_mh_mesh_begin(S.meshes[2 * m], S.meshes[2 * m + 1], r, rt_mh_threshold(buf, lim, k), w)) { g_skipped_meshes++; continue; }
            const int32_t object = (int32_t)rt_mh_bits(S.meshes[2 * m + 1].w);
            while (rt_mh_step<1>(S, stack.data(), object, r, lim, k, buf, w)) g_steps++;
        }
    }
    Answer a = blank();
    a.count = rt_mh_count(buf, k);
    for (int q = 0; q < k && q < a.count; q++) {
        const int slot = q;
        a.rec[q].t = buf.t[slot];
        a.rec[q].object = rt_mh_word_object(buf.key[slot]);
        a.rec[q].triangle = rt_mh_word_triangle(buf.key[slot]);
    }
    return a;
}

// ---- the definition: every candidate, collected and sorted ----------------------------------------------------------------------------------
struct Cand { float key, t; int32_t object, triangle; };

static void every_triangle(const Flat &f, uint32_t ref, bool ok, float path, int32_t object, const rt_mh_ray &r, std::vector<Cand> &all)
{
    const rt_mh_scene<rt_f4> S = f.S();
    if (ref & RT_REF_LEAF) {
        const int start = (int)(ref & RT_REF_START_MASK), count = (int)((ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        for (int i = count - 1; i >= 0; i--) {
            const rt_f4 *q = S.tris + 3 * (size_t)(start + i);
            float t;
            if (rt_mh_tri(q[0], q[1], q[2], r, t) && ok) all.push_back(Cand{t < path ? path : t, t, object, start + i});
        }
        return;
    }
    const rt_f4 *n = S.nodes + 4 * (size_t)(ref & RT_REF_NODE_MASK);
    float tl, tr;
    const bool hl = rt_mh_box(n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, r, tl);
    const bool hr = rt_mh_box(n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w, r, tr);
    every_triangle(f, rt_mh_bits(n[3].y), ok && hr, tr < path ? path : tr, object, r, all);     // (right first: not the walk's order)
    every_triangle(f, rt_mh_bits(n[3].x), ok && hl, tl < path ? path : tl, object, r, all);
}

static Answer exhaustive(const Flat &f, const float o[3], const float d[3], bool has_limit, float tmax, int32_t k, std::vector<Cand> *keep = nullptr)
{
    const rt_mh_scene<rt_f4> S = f.S();
    rt_mh_ray r;
    r.ox = o[0]; r.oy = o[1]; r.oz = o[2]; r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    float lim = RT_HIT_MISS_T;
    if (has_limit) lim = tmax < RT_HIT_MISS_T ? tmax : RT_HIT_MISS_T;
    std::vector<Cand> all;
    const bool nan_dir = std::isnan(d[0]) || std::isnan(d[1]) || std::isnan(d[2]);
    if (!nan_dir && !(has_limit && std::isnan(tmax))) {
        for (int m = f.num_meshes - 1; m >= 0; m--) {                   // (meshes first and backwards: not the walk's order)
            const rt_f4 m0 = S.meshes[2 * m], m1 = S.meshes[2 * m + 1];
            float t0;
            const bool h = rt_mh_box(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, r, t0);
            every_triangle(f, rt_mh_bits(m1.z), h, t0, (int32_t)rt_mh_bits(m1.w), r, all);
        }
        for (int i = f.num_objects - 1; i >= 0; i--) {
            rt_object ob;
            std::memcpy(&ob, S.objtab + 3 * i, sizeof ob);
            float t;
            if (ob.type == RT_OBJ_MESH) continue;
            if (ob.type == RT_OBJ_SPHERE) {
                if (rt_mh_sphere(ob.v[0], ob.v[1], ob.v[2], ob.v[3], r, t)) all.push_back(Cand{t, t, i, -1});
                continue;
            }
            if (ob.type == RT_OBJ_TRIANGLE) {
                const rt_f4 *q = S.tris + 3 * (size_t)ob.prim_start;
                if (rt_mh_tri(q[0], q[1], q[2], r, t)) all.push_back(Cand{t, t, i, ob.prim_start});
                continue;
            }
            if (ob.type == RT_OBJ_ONE_WAY_QUAD && rt_mh_dot(r.dx, r.dy, r.dz, ob.v[0], ob.v[1], ob.v[2]) < 0.0f) continue;
            const int faces = ob.type == RT_OBJ_CUBOID ? 6 : 1;
            for (int fc = 0; fc < faces; fc++) {
                const int first = ob.prim_start + 2 * fc;
                const rt_f4 *q = S.tris + 3 * (size_t)first;
                float t1, t2;
                const bool h1 = rt_mh_tri(q[0], q[1], q[2], r, t1), h2 = rt_mh_tri(q[3], q[4], q[5], r, t2);
                if (h1) all.push_back(Cand{t1, t1, i, first});
                else if (h2) all.push_back(Cand{t2, t2, i, first + 1});
            }
        }
    }
    std::vector<Cand> counted;
    for (const Cand &c : all)
        if (c.key <= lim) counted.push_back(c);
    std::sort(counted.begin(), counted.end(), [](const Cand &a, const Cand &b) {
        if (a.key != b.key) return a.key < b.key;
        if (a.object != b.object) return a.object > b.object;
        return a.triangle < b.triangle;
    });
    Answer a = blank();
    a.count = k > 0 ? (int32_t)std::min<size_t>(counted.size(), (size_t)k) : (int32_t)counted.size();
    for (int q = 0; q < k && q < a.count; q++) a.rec[q] = Rec{counted[(size_t)q].t, counted[(size_t)q].object, counted[(size_t)q].triangle};
    if (keep) *keep = counted;
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

static int same(const Answer &a, const Answer &b) { return !std::memcmp(&a, &b, sizeof a); }

static int check_scene(const std::vector<float> &tris, const std::vector<float> &second, bool mesh_alone, int rays, std::mt19937 &rng)
{
    Scene s;
    CHECK(make_scene(s, tris, second, mesh_alone), "building the scene");
    const Flat f = flat_of(s.v);
    const int n_tris = s.v.num_triangles, n_nodes = s.v.num_nodes;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < rays; i++) {
        float o[3], d[3];
        const unsigned kind = rng() % 8;
        // from outside towards a point of the scene, by default
        float target[3] = {uniform(rng, -0.8f, 0.8f), uniform(rng, -0.8f, 0.8f), uniform(rng, 1.2f, 2.8f)};
        if (kind < 3 && n_tris > 0) {                                   // through the centroid of some triangle record
            const rt_f4 *t = f.blob + f.off_tris + 3 * (size_t)(rng() % (unsigned)n_tris);
            target[0] = t[0].x + (t[0].w + t[1].z) / 3; target[1] = t[0].y + (t[1].x + t[1].w) / 3; target[2] = t[0].z + (t[1].y + t[2].x) / 3;
        }
        for (int a = 0; a < 3; a++) o[a] = uniform(rng, -3.0f, 3.0f) + (a == 2 ? 2.0f : 0.0f);
        for (int a = 0; a < 3; a++) d[a] = (target[a] - o[a]) * (kind == 3 ? 0.25f : 1.0f);
        if (kind == 4) {                                                // along an axis or in an axis plane: zero direction components
            const unsigned z = rng() % 3;
            d[z] = rng() % 2 ? 0.0f : -0.0f;
            if (rng() % 2) d[(z + 1) % 3] = 0.0f;
            for (int a = 0; a < 3; a++) o[a] = target[a] - d[a] * 2.0f;
        } else if (kind == 5 && n_nodes > 0) {                          // in a face of a child box of some node, running along it: 0 * inf in the slab test
            const rt_f4 *nd = f.blob + f.off_nodes + 4 * (size_t)(rng() % (unsigned)n_nodes);
            const float lo[3] = {nd[0].x, nd[0].y, nd[0].z}, hi[3] = {nd[0].w, nd[1].x, nd[1].y};
            const unsigned z = rng() % 3;
            for (int a = 0; a < 3; a++) o[a] = lo[a] + (hi[a] - lo[a]) * uniform(rng, -0.5f, 0.5f);
            o[z] = rng() % 2 ? lo[z] : hi[z];
            for (int a = 0; a < 3; a++) d[a] = uniform(rng, -1.0f, 1.0f);
            d[z] = 0.0f;
        } else if (kind == 6 && n_tris > 0) {                           // from a vertex of some triangle record: t at the acceptance threshold
            const rt_f4 *t = f.blob + f.off_tris + 3 * (size_t)(rng() % (unsigned)n_tris);
            o[0] = t[0].x; o[1] = t[0].y; o[2] = t[0].z;
            for (int a = 0; a < 3; a++) d[a] = target[a] - o[a];
        }
        g_rays++;
        std::vector<Cand> all;
        const Answer count_all = exhaustive(f, o, d, false, 0.0f, 0, &all);
        if (all.size() > RT_MULTIHIT_MAX) g_overflows++;
        for (size_t c = 1; c < all.size(); c++) g_ties += all[c].key == all[c - 1].key;
        for (int k = 0; k <= RT_MULTIHIT_MAX; k++) {
            const Answer a = walk(f, o, d, false, 0.0f, k), b = exhaustive(f, o, d, false, 0.0f, k);
            CHECK(same(a, b), "the walk differs from the exhaustive sort");
            if (k == 0) CHECK(same(a, count_all) && a.count == (int32_t)all.size(), "count-only mode counts every candidate");
        }
        // limits: the key of some candidate, one step down and up, 0, a negative one, NaN, the infinities, a random one
        const float key = all.empty() ? 1.0f : all[rng() % all.size()].key;
        const float lims[] = {key, std::nextafter(key, 0.0f), std::nextafter(key, inf), 0.0f, -0.0f, -1.0f, nan, inf, -inf, RT_HIT_MISS_T, uniform(rng, 0.0f, 6.0f)};
        for (float l : lims) {
            const int32_t k = (int32_t)(rng() % (RT_MULTIHIT_MAX + 1));
            for (int32_t kk : {k, (int32_t)0}) {
                const Answer a = walk(f, o, d, true, l, kk), b = exhaustive(f, o, d, true, l, kk);
                CHECK(same(a, b), "the walk differs from the exhaustive sort under a limit");
                if (!(l > 0.0f)) CHECK(a.count == 0 && a.rec[0].object == -1 && a.rec[0].t == RT_HIT_MISS_T, "a NaN limit, or one that is not positive, counts nothing");
                if (l == inf) CHECK(same(a, walk(f, o, d, false, 0.0f, kk)), "+Inf is no limit");
            }
        }
    }
    const float bad[3][3] = {{nan, 0, 1}, {0, nan, 1}, {1, 0, nan}};
    const float org[3] = {0, 0, -1};
    for (const float *d : {bad[0], bad[1], bad[2]})
        for (int32_t k : {0, 1, 8}) {
            const Answer a = walk(f, org, d, false, 0.0f, k);
            CHECK(same(a, exhaustive(f, org, d, false, 0.0f, k)) && a.count == 0, "a direction with a NaN component has no candidate");
        }
    return 0;
}

// ---- the insert alone: every order of arrival gives the sorted prefix ------------------------------------------------------------------------
static int check_insert(std::mt19937 &rng)
{
    g_case = "the insert";
    for (int round = 0; round < 2000; round++) {
        const int32_t k = RT_MULTIHIT_MAX;
        const int n = (int)(rng() % 24);
        std::vector<uint64_t> words;
        rt_mh_buf buf;
        rt_mh_clear(buf);
        for (int i = 0; i < n; i++) {
            const float key = (float)(1 + rng() % 6) * 0.5f;                      // few distinct keys: many ties
            const uint64_t w = rt_mh_word(key, (int32_t)(rng() % 5), rng() % 4 ? (uint32_t)(rng() % 7) : RT_MH_NO_TRI);
            if (std::find(words.begin(), words.end(), w) != words.end()) continue;      // a candidate is offered once
            words.push_back(w);
            rt_mh_insert(buf, w, key + 100.0f);
        }
        std::sort(words.begin(), words.end());
        g_n = round;
        for (int q = 0; q < k; q++) {
            const int slot = q;
            if (q < (int)words.size()) CHECK(buf.key[slot] == words[(size_t)q] && buf.t[slot] == rt_mh_word_key(words[(size_t)q]) + 100.0f, "a slot is not the sorted prefix's");
            else CHECK(buf.key[slot] == RT_MH_EMPTY, "a slot behind the last candidate is not empty");
        }
        for (int32_t kk = 0; kk <= RT_MULTIHIT_MAX; kk++) {
            const float want = kk == 0 || kk > (int)words.size() ? 7.0f : rt_mh_word_key(words[(size_t)kk - 1]);
            CHECK(rt_mh_threshold(buf, 7.0f, kk) == want, "the threshold is not the k-th best key");
        }
    }
    const uint64_t w = rt_mh_word(1.5f, 4095, RT_MH_NO_TRI), w0 = rt_mh_word(1.5f, 0, 1048574u);
    CHECK(rt_mh_word_object(w) == 4095 && rt_mh_word_triangle(w) == -1 && rt_mh_word_key(w) == 1.5f && w < w0, "the word of the last object, a sphere");
    CHECK(rt_mh_word_object(w0) == 0 && rt_mh_word_triangle(w0) == 1048574 && w0 < RT_MH_EMPTY, "the word of the first object's last triangle");
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
    alignas(16) static rt_hit hits[2 * RT_MULTIHIT_MAX + 1];
    int32_t counts[2] = {0, 0};
    const float o[6] = {0, 0, 0, 1, 1, 1}, d[6] = {0, 0, 1, 0, 0, 1}, lim[2] = {1, 1};
    rt_hit *const misaligned = (rt_hit *)((char *)hits + 4);
    for (int form = 0; form < 2; form++) {
        auto call = [&](rt_ctx *c, const rt_scene *s, const float *po, const float *pd, const float *l, int64_t n, int32_t k, rt_hit *h, int32_t *cn) {
            return form ? rt_trace_rays_multi(c, s, po, pd, l, n, k, h, cn) : rt_trace_rays_multi_device(c, s, po, pd, l, n, k, h, cn, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(call(nullptr, &scene, o, d, lim, 2, 2, hits, counts) == RT_ERR_INVALID, "null context");
        CHECK(call(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr) == RT_ERR_INVALID, "null context, no rays");
        CHECK(call(&ctx, nullptr, o, d, lim, 2, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(call(&ctx, &foreign, o, d, lim, 2, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(call(&ctx, &scene, o, d, lim, -1, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "ray count"), "a negative count");
        CHECK(call(&ctx, &scene, o, d, lim, ((int64_t)1 << 30) + 1, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "ray count"), "more than 2^30 rays");
        CHECK(call(&ctx, &scene, o, d, lim, 2, -1, hits, counts) == RT_ERR_INVALID && said(ctx, "record count"), "a negative k");
        CHECK(call(&ctx, &scene, o, d, lim, 2, RT_MULTIHIT_MAX + 1, hits, counts) == RT_ERR_INVALID && said(ctx, "record count"), "k beyond RT_MULTIHIT_MAX");
        CHECK(call(&ctx, &scene, o, d, lim, 0, RT_MULTIHIT_MAX + 1, hits, counts) == RT_ERR_INVALID, "k beyond RT_MULTIHIT_MAX, no rays");
        CHECK(call(&ctx, &scene, nullptr, d, lim, 2, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "null argument"), "null origins");
        CHECK(call(&ctx, &scene, o, nullptr, lim, 2, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "null argument"), "null directions");
        CHECK(call(&ctx, &scene, o, d, lim, 2, 2, nullptr, counts) == RT_ERR_INVALID && said(ctx, "null argument"), "null records with k > 0");
        CHECK(call(&ctx, &scene, o, d, lim, 2, 0, hits, nullptr) == RT_ERR_INVALID && said(ctx, "null counts"), "null counts with k == 0");
        CHECK(call(&ctx, &crowded, o, d, lim, 2, 2, hits, counts) == RT_ERR_INVALID && said(ctx, "too many objects"), "a scene of more than 4096 objects");
        CHECK(call(&ctx, &scene, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr) == RT_OK && call(&ctx, &scene, o, d, lim, 0, 3, hits, counts) == RT_OK, "no rays: nothing to do");
    }
    CHECK(rt_trace_rays_multi_device(&ctx, &scene, o, d, nullptr, 2, 2, misaligned, counts, nullptr) == RT_ERR_INVALID && said(ctx, "16-byte aligned"), "misaligned records");
    CHECK(g_launches == 0, "a refused call reached a launcher");
    CHECK(!ctx.launched && !ctx.have_timing && ctx.last_stream == nullptr, "a refused call touched the launch order");
    return 0;
}

// ---- a scene from a file -------------------------------------------------------------------------------------------------------------------
static int from_file(const char *in, const char *outp)
{
    FILE *fi = std::fopen(in, "rb");
    if (!fi) return 2;
    int32_t h[10];
    if (std::fread(h, 4, 10, fi) != 10 || h[0] < 0 || h[7] < 0 || h[9] < 0 || h[9] > RT_MULTIHIT_MAX) { std::fclose(fi); return 2; }
    const size_t n = (size_t)h[7];
    const int32_t k = h[9];
    std::vector<rt_f4> blob((size_t)h[0] + 1);
    std::vector<float> org(n * 3 + 1), dir(n * 3 + 1), lim(n + 1);
    bool ok = std::fread(blob.data(), 16, (size_t)h[0], fi) == (size_t)h[0] && std::fread(org.data(), 12, n, fi) == n && std::fread(dir.data(), 12, n, fi) == n;
    if (h[8]) ok = ok && std::fread(lim.data(), 4, n, fi) == n;
    std::fclose(fi);
    if (!ok) return 2;
    const Flat f{blob.data(), h[1], h[2], h[3], h[3] + 2 * h[4], h[4], h[5], h[6]};
    std::vector<int32_t> counts(n + 1);
    std::vector<Rec> recs(n * (size_t)k + 1);        // (one more: no null pointer to fwrite with k == 0)
    for (size_t i = 0; i < n; i++) {
        const Answer a = walk(f, &org[i * 3], &dir[i * 3], h[8] != 0, lim[i], k);
        counts[i] = a.count;
        for (int q = 0; q < k; q++) recs[i * (size_t)k + (size_t)q] = a.rec[q];
    }
    FILE *fo = std::fopen(outp, "wb");
    if (!fo) return 2;
    ok = std::fwrite(counts.data(), 4, n, fo) == n && std::fwrite(recs.data(), sizeof(Rec), n * (size_t)k, fo) == n * (size_t)k;
    std::fclose(fo);
    std::printf("multihit host side: %zu rays from a file, %ld steps, sanitizers silent\n", n, g_steps);
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(rt_hit) == 48 && sizeof(rt_mh_entry) == 8 && sizeof(Rec) == 12 && RT_MULTIHIT_MAX == 8, "the record, the stack entry and the slots");
    if (argc == 4 && !std::strcmp(argv[1], "file")) return from_file(argv[2], argv[3]);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int rays = argc > 2 ? std::atoi(argv[2]) : 100;
    std::mt19937 rng(seed);
    if (check_insert(rng)) return 1;
    const std::vector<float> second = soup(rng, 37, 0.8f, 0.15f);
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 100, 1023, 1024, 1025, 3000};
    for (int n : sizes) {
        g_n = n;
        const int cnt = n > 1000 ? rays / 4 + 1 : rays;
        g_case = "random";
        if (check_scene(soup(rng, n, 0.8f, 0.3f), second, false, cnt, rng)) return 1;
        g_case = "the mesh alone";
        if (check_scene(soup(rng, n, 0.8f, 0.3f), second, true, cnt, rng)) return 1;
        // ties: every triangle the same, every triangle four times
        std::vector<float> ident = soup(rng, n, 0.8f, 0.3f), dup = soup(rng, n, 0.8f, 0.3f);
        for (int i = 0; i < n; i++) {
            std::memcpy(&ident[(size_t)i * 9], &ident[0], 36);
            std::memcpy(&dup[(size_t)i * 9], &dup[(size_t)(i / 4) * 9], 36);
        }
        g_case = "identical triangles";
        if (check_scene(ident, second, true, cnt / 2 + 1, rng)) return 1;
        g_case = "every triangle four times";
        if (check_scene(dup, second, false, cnt / 2 + 1, rng)) return 1;
    }
    if (refusals()) return 1;
    if (rays >= 40 && (g_overflows == 0 || g_ties == 0)) { std::fprintf(stderr, "multihit check: no ray had more than 8 candidates, or none a tied key\n"); return 1; }
    std::printf("multihit host side: %ld rays on %d sizes of meshes, %ld steps, %ld meshes skipped at their root box, %ld rays of more than 8 candidates, %ld tied keys, sanitizers silent\n",
                g_rays, (int)(sizeof sizes / sizeof sizes[0]), g_steps, g_skipped_meshes, g_overflows, g_ties);
    return 0;
}
