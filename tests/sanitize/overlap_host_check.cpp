// The box-overlap queries (rt_overlap_boxes[_device]: rt_overlap.h, rt_overlap_capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer
// (CPU only; test infrastructure), and the part of their proof that needs no GPU:
//   1. the kernel's traversal as plain host code - the steps of rt_overlap.h (rt_ov_begin, rt_ov_simple, rt_ov_mesh_begin, rt_ov_step,
//      rt_ov_insert), the text the kernel compiles, on a stack of exactly the scene's stack_entries - against the EXHAUSTIVE loop over
//      every candidate (every sphere, every triangle record, a mesh's triangles under the path flags of a plain recursion over its whole
//      tree; the ids sorted, not inserted), as bytes: seeded random and adversarial inputs - boxes equal to node boxes and to a mesh's root
//      box, boxes with a face on a vertex, zero-extent boxes on vertices, boxes that hold the scene, identical triangles and every
//      triangle four times (tied ids are impossible: equal geometry under different ids), zero-area triangles, meshes of 1 to 9
//      triangles (every chain shape) and of about 1,024, boxes that are not valid, k from 0 to 8, and the any-only walk;
//   2. every refusal of both entry points, on a context and scenes built in host memory (nothing gets as far as a HIP call or the launcher).
//   overlap_host_check <seed> <boxes per scene>
// A second form answers a scene from a file, for tests/test_overlap_host.py to set against the NumPy yardstick:
//   overlap_host_check file <in> <out>   in: int32 blob_f4, off_nodes, off_tris, off_meshes, num_meshes, num_objects, stack_entries, n, k;
//                                            the blob; n x 3 lo; n x 3 hi.   out: n int32 counts; n bytes; n * k ids
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
#include "rt_overlap.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                               \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "overlap check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;
static long g_steps = 0, g_skipped_meshes = 0, g_boxes = 0, g_touching = 0, g_overflowed = 0, g_path_bites = 0;

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
};

static rt_ov_box box_of(const float lo[3], const float hi[3])
{
    rt_ov_box b;
    std::memset(&b, 0, sizeof b);
    b.lox = lo[0]; b.loy = lo[1]; b.loz = lo[2]; b.hix = hi[0]; b.hiy = hi[1]; b.hiz = hi[2];
    return b;
}

// ---- the kernel's path: one lane, the steps in a plain loop -------------------------------------------------------------------------------
static Answer walk(const Flat &f, const float lo[3], const float hi[3], int32_t k, bool any_only)
{
    const rt_ov_scene<rt_f4> S = f.S();
    rt_ov_box box = box_of(lo, hi);
    rt_ov_buf buf;
    rt_ov_clear(buf);
    if (rt_ov_begin(box)) {
        rt_ov_simple(S, f.num_objects, box, k, any_only, buf);
        std::vector<uint32_t> stack((size_t)f.stack_entries * 2);          // exactly what the scene sizes, in 8-byte units: one entry more is the sanitizer's to find
        for (int m = 0; m < f.num_meshes && !(any_only && buf.total > 0u); m++) {
            rt_ov_walk w;
            if (!rt_ov_mesh_begin(S.meshes[2 * m], S.meshes[2 * m + 1], box, w)) { g_skipped_meshes++; continue; }
            const int32_t object = (int32_t)rt_ov_bits(S.meshes[2 * m + 1].w);
            while (rt_ov_step<1>(S, stack.data(), object, box, k, buf, w)) {
                g_steps++;
                if (any_only && buf.total > 0u) break;
            }
        }
    }
    Answer a;
    a.count = (int32_t)buf.total;
    a.any = buf.total > 0u ? 1 : 0;
    for (int q = 0; q < RT_OVERLAP_MAX; q++) a.ids[q] = rt_ov_id(buf.id[q], q < k && (uint32_t)q < buf.total);
    return a;
}

// ---- the definition: every candidate ------------------------------------------------------------------------------------------------------
static void every_triangle(const Flat &f, uint32_t ref, bool path, int32_t object, const rt_ov_box &box, std::vector<uint32_t> &found)
{
    const rt_ov_scene<rt_f4> S = f.S();
    if (ref & RT_REF_LEAF) {
        const int start = (int)(ref & RT_REF_START_MASK), count = (int)((ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
        for (int j = count - 1; j >= 0; j--) {                              // (backwards: not the walk's order)
            const rt_f4 *t = S.tris + 3 * (size_t)(start + j);
            const bool bare = rt_ov_tri(t[0], t[1], t[2], box);
            if (bare && !path) g_path_bites++;
            if (bare && path) found.push_back(rt_ov_word(object, (uint32_t)(start + j)));
        }
        return;
    }
    const rt_f4 *n = S.nodes + 4 * (size_t)(ref & RT_REF_NODE_MASK);
    const bool ol = rt_ov_boxes(n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, box);
    const bool orr = rt_ov_boxes(n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w, box);
    every_triangle(f, rt_ov_bits(n[3].y), path && orr, object, box, found);         // (right first, and into subtrees off the path: the whole tree)
    every_triangle(f, rt_ov_bits(n[3].x), path && ol, object, box, found);
}

static Answer exhaustive(const Flat &f, const float lo[3], const float hi[3], int32_t k)
{
    const rt_ov_scene<rt_f4> S = f.S();
    rt_ov_box box = box_of(lo, hi);
    std::vector<uint32_t> found;
    if (rt_ov_begin(box)) {
        for (int i = f.num_objects - 1; i >= 0; i--) {                      // (backwards: not the walk's order)
            const int32_t type = (int32_t)rt_ov_bits(S.objtab[3 * i].x), prim = (int32_t)rt_ov_bits(S.objtab[3 * i].y);
            if (type == RT_OBJ_MESH) continue;
            if (type == RT_OBJ_SPHERE) {
                const rt_f4 ob1 = S.objtab[3 * i + 1];
                if (rt_ov_sphere(ob1.x, ob1.y, ob1.z, ob1.w, box)) found.push_back(rt_ov_word(i, RT_MH_NO_TRI));
                continue;
            }
            for (int j = 0; j < rt_ov_object_tris(type); j++) {
                const rt_f4 *t = S.tris + 3 * (size_t)(prim + j);
                if (rt_ov_tri(t[0], t[1], t[2], box)) found.push_back(rt_ov_word(i, (uint32_t)(prim + j)));
            }
        }
        for (int m = 0; m < f.num_meshes; m++) {
            const rt_f4 m0 = S.meshes[2 * m], m1 = S.meshes[2 * m + 1];
            every_triangle(f, rt_ov_bits(m1.z), rt_ov_boxes(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, box), (int32_t)rt_ov_bits(m1.w), box, found);
        }
    }
    std::sort(found.begin(), found.end());
    Answer a;
    a.count = (int32_t)found.size();
    a.any = found.empty() ? 0 : 1;
    for (int q = 0; q < RT_OVERLAP_MAX; q++) {
        const bool held = q < k && (size_t)q < found.size();
        a.ids[q].object = held ? (int32_t)(found[(size_t)q] >> 20) : -1;
        a.ids[q].triangle = held ? ((found[(size_t)q] & RT_MH_NO_TRI) == RT_MH_NO_TRI ? -1 : (int32_t)(found[(size_t)q] & RT_MH_NO_TRI)) : -1;
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

static bool same(const Answer &a, const Answer &b) { return a.count == b.count && a.any == b.any && !std::memcmp(a.ids, b.ids, sizeof a.ids); }

static int check_box(const Flat &f, const float lo[3], const float hi[3], std::mt19937 &rng)
{
    const Answer all = exhaustive(f, lo, hi, RT_OVERLAP_MAX);
    g_boxes++;
    if (all.count > 0) g_touching++;
    if (all.count > RT_OVERLAP_MAX) g_overflowed++;
    const int32_t k_some = (int32_t)(rng() % (RT_OVERLAP_MAX + 1));
    for (int32_t k = 0; k <= RT_OVERLAP_MAX; k++) {
        if (k != 0 && k != RT_OVERLAP_MAX && k != k_some && g_boxes % 16 != 0) continue;        // (every k on every sixteenth box, three of them on the others)
        const Answer w = walk(f, lo, hi, k, false), e = exhaustive(f, lo, hi, k);
        CHECK(same(w, e), "the walk differs from the exhaustive loop");
        CHECK(e.count == all.count && !std::memcmp(e.ids, all.ids, (size_t)k * sizeof(rt_overlap_id)), "the ids under a smaller k are a prefix");
        for (int q = 1; q < k && q < e.count; q++)
            CHECK(e.ids[q - 1].object < e.ids[q].object || (e.ids[q - 1].object == e.ids[q].object && e.ids[q - 1].triangle < e.ids[q].triangle), "ids ascend");
        for (int q = (e.count < k ? e.count : k); q < RT_OVERLAP_MAX; q++) CHECK(e.ids[q].object == -1 && e.ids[q].triangle == -1, "slots past the count");
    }
    CHECK(walk(f, lo, hi, 0, true).any == all.any, "the any-only walk's byte");
    return 0;
}

static int check_scene(const std::vector<float> &tris, const std::vector<float> &second, bool mesh_alone, int boxes, std::mt19937 &rng)
{
    Scene s;
    CHECK(make_scene(s, tris, second, mesh_alone), "building the scene");
    const Flat f = flat_of(s.v);
    const int n_tris = s.v.num_triangles, n_nodes = s.v.num_nodes;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < boxes; i++) {
        float lo[3], hi[3];
        const unsigned kind = rng() % 10;
        const float scale = kind < 3 ? 0.01f : kind < 6 ? 0.1f : 1.0f;
        for (int k = 0; k < 3; k++) {
            const float c = uniform(rng, -1.5f, 1.5f) + (k == 2 ? 2.0f : 0.0f), e = uniform(rng, 0.0f, scale);
            lo[k] = c - e; hi[k] = c + e;
        }
        if (kind == 6 && n_nodes > 0) {                               // a node's child box itself, or that box one step in or out on one face
            const rt_f4 *n = f.blob + f.off_nodes + 4 * (size_t)(rng() % (unsigned)n_nodes);
            const float l[6] = {n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y}, r[6] = {n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w};
            const float *b = rng() % 2 ? l : r;
            for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; }
            const unsigned tweak = rng() % 5, a = rng() % 3;
            if (tweak == 1) lo[a] = std::nextafter(lo[a], inf); else if (tweak == 2) hi[a] = std::nextafter(hi[a], -inf);
            else if (tweak == 3) { hi[a] = lo[a]; } else if (tweak == 4) { lo[a] = hi[a]; }        // a face of the node box: touching
            if (!(lo[a] <= hi[a])) hi[a] = lo[a];
        } else if (kind == 7 && f.num_meshes > 0) {                   // a mesh's root box, and the box beside it that shares a face
            const rt_f4 *m = f.blob + f.off_meshes + 2 * (size_t)(rng() % (unsigned)f.num_meshes);
            const float b[6] = {m[0].x, m[0].y, m[0].z, m[0].w, m[1].x, m[1].y};
            for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; }
            if (rng() % 2) { const unsigned a = rng() % 3; const float e = hi[a] - lo[a]; lo[a] = hi[a]; hi[a] = lo[a] + e; }
        } else if ((kind == 8 || kind == 9) && n_tris > 0) {           // a vertex: a zero-extent box on it, or a box with a face through it
            const rt_f4 *t = f.blob + f.off_tris + 3 * (size_t)(rng() % (unsigned)n_tris);
            const unsigned which = rng() % 3;
            const float v[3] = {which == 0 ? t[0].x : which == 1 ? t[0].x + t[0].w : t[0].x + t[1].z, which == 0 ? t[0].y : which == 1 ? t[0].y + t[1].x : t[0].y + t[1].w,
                                which == 0 ? t[0].z : which == 1 ? t[0].z + t[1].y : t[0].z + t[2].x};
            if (kind == 8) { for (int k = 0; k < 3; k++) lo[k] = hi[k] = v[k]; }
            else { const unsigned a = rng() % 3; for (int k = 0; k < 3; k++) { lo[k] = v[k] - 0.05f; hi[k] = v[k] + 0.05f; } if (rng() % 2) lo[a] = v[a]; else hi[a] = v[a]; }
        }
        if (check_box(f, lo, hi, rng)) return 1;
    }
    // the whole scene: every candidate (a sphere inside the box touches it: only a box inside the ball does not)
    const float all_lo[3] = {-50, -50, -50}, all_hi[3] = {50, 50, 50};
    const Answer whole = exhaustive(f, all_lo, all_hi, RT_OVERLAP_MAX);
    CHECK(whole.count == n_tris + (mesh_alone ? 0 : 2) && same(walk(f, all_lo, all_hi, RT_OVERLAP_MAX, false), whole), "a box that holds the scene meets every candidate");
    const float in_lo[3] = {0.35f, 0.05f, 1.45f}, in_hi[3] = {0.45f, 0.15f, 1.55f};            // inside the first sphere (0.4, 0.1, 1.5; 0.3): a sphere is a surface
    const Answer inner = exhaustive(f, in_lo, in_hi, RT_OVERLAP_MAX);
    for (int q = 0; q < RT_OVERLAP_MAX; q++) CHECK(!(inner.ids[q].object == 0 && inner.ids[q].triangle == -1 && !mesh_alone), "a box wholly inside a ball touches its surface");
    // boxes that are not valid overlap nothing
    for (int k = 0; k < 3; k++)
        for (float bad : {nan, inf, -inf}) {
            float lo[3] = {-50, -50, -50}, hi[3] = {50, 50, 50};
            lo[k] = bad;
            if (bad != -inf) CHECK(walk(f, lo, hi, 8, false).count == 0 && exhaustive(f, lo, hi, 8).count == 0, "lo > hi or not a number");
            else CHECK(walk(f, lo, hi, 8, false).count == 0 && exhaustive(f, lo, hi, 8).count == 0 && walk(f, lo, hi, 0, true).any == 0, "an infinite box");
            lo[k] = -50; hi[k] = bad;
            CHECK(walk(f, lo, hi, 8, false).count == 0 && exhaustive(f, lo, hi, 8).count == 0, "hi that is not finite or below lo");
        }
    const float swapped_lo[3] = {1, 0, 0}, swapped_hi[3] = {0.5f, 3, 3};
    CHECK(walk(f, swapped_lo, swapped_hi, 8, false).count == 0 && exhaustive(f, swapped_lo, swapped_hi, 8).count == 0, "lo > hi on one axis");
    return 0;
}

// ---- the insert on its own: every order of arrival gives the sorted prefix ---------------------------------------------------------------
static int inserts(std::mt19937 &rng)
{
    g_case = "the insert";
    for (int round = 0; round < 2000; round++) {
        const int n = (int)(rng() % 20);
        std::vector<uint32_t> words((size_t)n);
        for (auto &w : words) w = rng() % 4 == 0 ? rt_ov_word((int32_t)(rng() % 4096), RT_MH_NO_TRI) : rt_ov_word((int32_t)(rng() % 4096), rng() % 0xfffffu);
        if (n > 0 && round % 7 == 0) words[0] = 0xffffffffu;           // object 4095, a sphere: the word an empty slot holds
        if (n > 1 && round % 5 == 0) words[1] = 0u;
        rt_ov_buf b;
        rt_ov_clear(b);
        for (uint32_t w : words) rt_ov_offer(b, 8, true, rt_ov_word_object(w), w & RT_MH_NO_TRI);
        rt_ov_offer(b, 8, false, 0, 0u);                               // one that does not overlap changes nothing
        std::vector<uint32_t> sorted = words;
        std::sort(sorted.begin(), sorted.end());
        sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
        if (sorted.size() != words.size()) continue;                   // (a candidate is offered once: equal words do not occur)
        CHECK(b.total == (uint32_t)n, "the total");
        for (int q = 0; q < RT_OVERLAP_MAX; q++) CHECK(b.id[q] == (q < n ? sorted[(size_t)q] : RT_OV_EMPTY), "the slots are the sorted prefix");
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
    int32_t counts[2] = {-3, -3};
    uint8_t any[2] = {7, 7};
    const float lo[6] = {0, 0, 0, 1, 1, 1}, hi[6] = {1, 1, 1, 2, 2, 2};
    rt_overlap_id *const misaligned = (rt_overlap_id *)((char *)ids + 4);
    for (int form = 0; form < 2; form++) {
        auto call = [&](rt_ctx *c, const rt_scene *s, const float *l, const float *h, int64_t n, int32_t k, rt_overlap_id *pi, int32_t *pc, uint8_t *pa) {
            return form ? rt_overlap_boxes(c, s, l, h, n, k, pi, pc, pa) : rt_overlap_boxes_device(c, s, l, h, n, k, pi, pc, pa, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(call(nullptr, &scene, lo, hi, 2, 2, ids, counts, any) == RT_ERR_INVALID, "null context");
        CHECK(call(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == RT_ERR_INVALID, "null context, no boxes");
        CHECK(call(&ctx, nullptr, lo, hi, 2, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(call(&ctx, &foreign, lo, hi, 2, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(call(&ctx, &scene, lo, hi, -1, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "box count"), "a negative count");
        CHECK(call(&ctx, &scene, lo, hi, ((int64_t)1 << 30) + 1, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "box count"), "more than 2^30 boxes");
        CHECK(call(&ctx, &scene, lo, hi, 2, -1, ids, counts, any) == RT_ERR_INVALID && said(ctx, "id count"), "k below 0");
        CHECK(call(&ctx, &scene, lo, hi, 2, RT_OVERLAP_MAX + 1, ids, counts, any) == RT_ERR_INVALID && said(ctx, "id count"), "k above RT_OVERLAP_MAX");
        CHECK(call(&ctx, &scene, lo, hi, 0, RT_OVERLAP_MAX + 1, ids, counts, any) == RT_ERR_INVALID, "k above RT_OVERLAP_MAX without boxes");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, nullptr, hi, 2, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "null argument"), "null lo");
        ctx.err.clear();
        CHECK(call(&ctx, &scene, lo, nullptr, 2, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "null argument"), "null hi");
        CHECK(call(&ctx, &scene, lo, hi, 2, 2, nullptr, counts, any) == RT_ERR_INVALID && said(ctx, "null ids"), "null ids while k > 0");
        CHECK(call(&ctx, &scene, lo, hi, 2, 0, nullptr, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "no output"), "all three outputs null");
        CHECK(call(&ctx, &scene, lo, hi, 2, 0, ids, nullptr, nullptr) == RT_ERR_INVALID && said(ctx, "no output"), "ids alone with k == 0 is no output");
        CHECK(call(&ctx, &crowded, lo, hi, 2, 2, ids, counts, any) == RT_ERR_INVALID && said(ctx, "too many objects"), "more than 4,096 objects");
        CHECK(call(&ctx, &scene, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == RT_OK && call(&ctx, &scene, lo, hi, 0, 2, ids, counts, any) == RT_OK, "no boxes: nothing to do");
    }
    CHECK(rt_overlap_boxes_device(&ctx, &scene, lo, hi, 2, 2, misaligned, counts, any, nullptr) == RT_ERR_INVALID && said(ctx, "8-byte aligned"), "misaligned d_ids");
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
    std::vector<float> lo(n * 3 + 1), hi(n * 3 + 1);
    const bool read = std::fread(blob.data(), 16, (size_t)h[0], fi) == (size_t)h[0] && std::fread(lo.data(), 12, n, fi) == n && std::fread(hi.data(), 12, n, fi) == n;
    std::fclose(fi);
    if (!read) return 2;
    const Flat f{blob.data(), h[1], h[2], h[3], h[3] + 2 * h[4], h[4], h[5], h[6]};
    std::vector<int32_t> counts(n + 1);
    std::vector<uint8_t> any(n + 1);
    std::vector<rt_overlap_id> ids(n * (size_t)k + 1);
    for (size_t i = 0; i < n; i++) {
        const Answer a = walk(f, &lo[i * 3], &hi[i * 3], k, false);
        counts[i] = a.count;
        any[i] = walk(f, &lo[i * 3], &hi[i * 3], 0, true).any;
        for (int q = 0; q < k; q++) ids[i * (size_t)k + (size_t)q] = a.ids[q];
    }
    FILE *fo = std::fopen(outp, "wb");
    if (!fo) return 2;
    const bool ok = std::fwrite(counts.data(), 4, n, fo) == n && std::fwrite(any.data(), 1, n, fo) == n && std::fwrite(ids.data(), 8, n * (size_t)k, fo) == n * (size_t)k;
    std::fclose(fo);
    std::printf("overlap host side: %d boxes from a file, %ld steps, sanitizers silent\n", h[7], g_steps);
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    static_assert(sizeof(rt_overlap_id) == 8, "the id");
    if (argc == 4 && !std::strcmp(argv[1], "file")) return from_file(argv[2], argv[3]);
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int boxes = argc > 2 ? std::atoi(argv[2]) : 200;
    std::mt19937 rng(seed);
    const std::vector<float> second = soup(rng, 37, 0.8f, 0.15f);
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 100, 1023, 1025};
    for (int n : sizes) {
        g_n = n;
        const int count = n > 1000 ? boxes / 4 + 1 : boxes;
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
    if (inserts(rng) || refusals()) return 1;
    if (g_touching == 0 || g_overflowed == 0) { std::fprintf(stderr, "overlap check: no box touched anything, or none met more than %d candidates\n", RT_OVERLAP_MAX); return 1; }
    std::printf("overlap host side: %ld boxes on %d sizes of meshes (%ld touch a surface, %ld meet more than %d; the path rule alone decided %ld pairs), "
                "%ld steps, %ld meshes skipped at their root box, sanitizers silent\n", g_boxes, (int)(sizeof sizes / sizeof sizes[0]), g_touching, g_overflowed,
                RT_OVERLAP_MAX, g_path_bites, g_steps, g_skipped_meshes);
    return 0;
}
