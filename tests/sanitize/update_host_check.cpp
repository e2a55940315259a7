// The host side of rt_scene_update_mesh[_device] (rt_update_capi.cpp, rt_rebuild.h) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only;
// test infrastructure), and the part of the rebuild's proof that needs no GPU:
//   1. the plan (rt_rb_make_plan: a mesh's tree from its triangle count alone) against the tree BvhBuilder makes of n random triangles, for every
//      n the caller asks for: the levels tile [0, n), the child and root references, the stack depth - and a count the builder refuses has no plan;
//   2. a plain host executor of the device algorithm - the plan, the __host__ __device__ arithmetic of rt_rebuild.h, a std::sort of the composite
//      words per segment, boxes folded in pieces and joined in list order - run on a scene flattened with OLD triangles, against the flattened
//      scene of a builder with the NEW ones, byte for byte (blob, object table, texture coordinates): random, tied and signed-zero meshes, meshes
//      with texture coordinates, several meshes in a scene;
//   3. every refusal of both entry points, on a context and scenes built in host memory (nothing gets as far as a HIP call).
//   update_host_check <seed> <every n up to> [larger n ...]
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
#include "rt_math.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                                             \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "update check: %s (%s, n = %d)\n", what, g_case, g_n); return 1; } \
    } while (0)

static const char *g_case = "";
static int g_n = 0;

static float uniform(std::mt19937 &rng, float lo, float hi) { return lo + (hi - lo) * (float)(rng() % 1000001) / 1000000.0f; }

static std::vector<float> random_soup(std::mt19937 &rng, int n)
{
    std::vector<float> t((size_t)n * 9);
    for (int i = 0; i < n; i++) {
        float c[3] = {uniform(rng, -1.0f, 1.0f), uniform(rng, -1.0f, 1.0f), uniform(rng, -4.0f, -2.0f)};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) t[(size_t)i * 9 + v * 3 + k] = c[k] + uniform(rng, -0.1f, 0.1f);
    }
    return t;
}

// ---- a scene of the shape [sphere, MAIN MESH, textured quad, sphere, second mesh]: object 1 is the mesh that changes ------------------------
struct Scene {
    rt_scene_builder *b = nullptr;
    rt_flat_view v{};
    Scene() = default;
    Scene(const Scene &) = delete;
    ~Scene() { rt_scene_builder_destroy(b); }
};
static const int MAIN = 1;

// main mesh: `tris` (9 n floats), or, with quads != 0, an .obj of n / 2 quads over the vertices `tris` holds (12 floats per quad) with a material that
// needs texture coordinates; commit_tris receives the mesh's triangles in commit order
static bool make_scene(Scene &s, const std::vector<float> &tris, int n, bool quads, const std::vector<float> &second, std::vector<float> *commit_tris)
{
    if (rt_scene_builder_create(&s.b) != RT_OK) return false;
    const float grey[3] = {0.5f, 0.5f, 0.5f}, dark[3] = {0.1f, 0.1f, 0.1f};
    rt_material plain, checker;
    rt_material_standard(&plain, grey, 0.2f);
    rt_material_checkerboard(&checker, grey, dark, 4, 0.0f);
    const float c0[3] = {0.0f, 0.0f, -5.0f}, c1[3] = {2.0f, 0.0f, -5.0f};
    const float q[4][3] = {{-3, -1, -1}, {3, -1, -1}, {3, -1, -7}, {-3, -1, -7}};
    bool ok = rt_scene_add_sphere(s.b, c0, 0.5f, &plain) == RT_OK;
    if (quads) {
        std::vector<int32_t> idx, arity;
        for (int f = 0; f < n / 2; f++) { arity.push_back(4); for (int k = 0; k < 4; k++) idx.push_back(4 * f + k); }
        rt_obj *o = nullptr;
        ok = ok && rt_obj_from_arrays(tris.data(), 4 * (n / 2), idx.data(), arity.data(), n / 2, &o) == RT_OK;
        if (ok && commit_tris) { commit_tris->resize((size_t)n * 9); ok = rt_obj_get_triangles(o, commit_tris->data()) == RT_OK; }
        ok = ok && rt_scene_add_obj_mesh(s.b, o, &checker) == RT_OK;
        rt_obj_destroy(o);
    } else {
        ok = ok && rt_scene_add_mesh(s.b, tris.data(), n, &plain) == RT_OK;
        if (commit_tris) *commit_tris = tris;
    }
    ok = ok && rt_scene_add_quad(s.b, q[0], q[1], q[2], q[3], &checker) == RT_OK && rt_scene_add_sphere(s.b, c1, 0.25f, &checker) == RT_OK;
    ok = ok && rt_scene_add_mesh(s.b, second.data(), (int32_t)(second.size() / 9), &plain) == RT_OK;
    return ok && rt_debug_flatten(s.b, &s.v) == RT_OK;
}

// ---- the executor: the device algorithm in plain host code -------------------------------------------------------------------------------
static rt_rb_box fold_in_pieces(const float *pts, const std::vector<int> &list, int start, int count, std::mt19937 &rng)
{
    // pieces of random length, each folded point by point; then neighbours joined pairwise, in list order, until one is left
    std::vector<rt_rb_box> part;
    for (int j = 0; j < count;) {
        const int len = 1 + (int)(rng() % (unsigned)(count < 7 ? count : 7));
        rt_rb_box b;
        b.valid = 0;
        if (rng() % 5 == 0) part.push_back(b);           // (a thread whose piece is empty)
        for (int e = j; e < j + len && e < count; e++)
            for (int v = 0; v < 3; v++) rt_rb_box_add(&b, pts + (size_t)list[(size_t)(start + e)] * 9 + 3 * v);
        part.push_back(b);
        j += len;
    }
    while (part.size() > 1) {
        std::vector<rt_rb_box> next;
        for (size_t i = 0; i < part.size(); i += 2) next.push_back(i + 1 < part.size() ? rt_rb_box_join(part[i], part[i + 1]) : part[i]);
        part.swap(next);
    }
    return part[0];
}

struct Target {
    std::vector<rt_f4> blob;
    std::vector<rt_object> objects;
    std::vector<float> tri_uv;
};

static void box6(const std::vector<rt_rb_box> &boxes, int heap, float v[6])
{
    for (int k = 0; k < 3; k++) { v[k] = heap >= 0 ? boxes[(size_t)heap].lo[k] : 0.0f; v[3 + k] = heap >= 0 ? boxes[(size_t)heap].hi[k] : 0.0f; }
}

static void execute(const rt_rb_plan &p, const float *pts, const std::vector<float> &uv0, const rt_flat_view &f, int oi, int tri_base, int node_base, int mesh_index,
                    Target &t, std::mt19937 &rng)
{
    const int n = p.n;
    std::vector<int> list((size_t)n), next((size_t)n);
    for (int i = 0; i < n; i++) list[(size_t)i] = i;
    std::vector<rt_rb_box> boxes(RT_REBUILD_SEGS);
    for (int level = 0; level <= RT_BVH_DEPTH; level++) {
        for (int i = 0; i < (1 << level); i++) {
            const rt_rb_seg seg = p.segs[(size_t)rt_rb_heap(level, i)];
            if (seg.count == 0) continue;
            const rt_rb_box box = fold_in_pieces(pts, list, seg.start, seg.count, rng);
            boxes[(size_t)rt_rb_heap(level, i)] = box;
            if (level == RT_BVH_DEPTH) continue;
            float ref[3];
            rt_rb_ref_point(box, ref);
            std::vector<uint64_t> words((size_t)seg.count);
            for (int j = 0; j < seg.count; j++) words[(size_t)j] = rt_rb_word((uint32_t)i, rt_rb_key(pts + (size_t)list[(size_t)(seg.start + j)] * 9, ref), (uint32_t)j);
            std::sort(words.begin(), words.end());
            for (int j = 0; j < seg.count; j++) next[(size_t)(seg.start + j)] = list[(size_t)seg.start + rt_rb_word_pos(words[(size_t)j])];
        }
        if (level < RT_BVH_DEPTH) list = next;
    }
    for (int k = 0; k < n; k++) {
        rt_rb_tri(pts + (size_t)list[(size_t)k] * 9, &t.blob[(size_t)f.off_tris + (size_t)(tri_base + k) * 3]);
        if (!t.tri_uv.empty()) std::memcpy(&t.tri_uv[(size_t)(tri_base + k) * 6], &uv0[(size_t)list[(size_t)k] * 6], 24);
    }
    for (size_t k = 0; k < p.slots.size(); k++) {
        float l[6], r[6];
        box6(boxes, p.slots[k].left, l);
        box6(boxes, p.slots[k].right, r);
        rt_f4 *q = &t.blob[(size_t)f.off_nodes + ((size_t)node_base + k) * 4];
        q[0] = rt_f4{l[0], l[1], l[2], l[3]};
        q[1] = rt_f4{l[4], l[5], r[0], r[1]};
        q[2] = rt_f4{r[2], r[3], r[4], r[5]};
    }
    float v[6];
    box6(boxes, p.root_seg, v);
    rt_f4 *mt = &t.blob[(size_t)f.off_meshes + (size_t)mesh_index * 2];
    mt[0] = rt_f4{v[0], v[1], v[2], v[3]};
    mt[1].x = v[4];
    mt[1].y = v[5];
    const int off_objtab = f.off_meshes + f.num_meshes * 2;
    rt_object in_blob;
    std::memcpy(&in_blob, &t.blob[(size_t)off_objtab + (size_t)oi * 3], sizeof in_blob);
    for (int k = 0; k < 6; k++) { in_blob.v[k] = v[k]; t.objects[(size_t)oi].v[k] = v[k]; }
    std::memcpy(&t.blob[(size_t)off_objtab + (size_t)oi * 3], &in_blob, sizeof in_blob);
    t.blob[(size_t)f.off_objlds + (size_t)oi * RT_OBJLDS_F4 + 2] = rt_f4{v[0], v[1], v[2], v[3]};
}

// old -> new through the executor == a fresh flatten of new
static int update_equals_commit(const std::vector<float> &old_tris, const std::vector<float> &new_tris, int n, bool quads, const std::vector<float> &second, std::mt19937 &rng)
{
    Scene a, b;
    std::vector<float> commit_new;
    CHECK(make_scene(a, old_tris, n, quads, second, nullptr) && make_scene(b, new_tris, n, quads, second, &commit_new), "building the two scenes");
    const rt_flat_view &f = a.v;
    CHECK(f.blob_f4 == b.v.blob_f4 && f.off_tris == b.v.off_tris && f.num_nodes == b.v.num_nodes && f.stack_entries == b.v.stack_entries, "the layout follows from the counts");
    const rt_object *objs = (const rt_object *)f.objects;
    CHECK(objs[MAIN].type == RT_OBJ_MESH && objs[MAIN + 1].prim_start - objs[MAIN].prim_start == n, "the main mesh");
    rt_rb_plan p;
    CHECK(rt_rb_make_plan(n, p), "a plan");
    Target t;
    t.blob.assign((const rt_f4 *)f.blob, (const rt_f4 *)f.blob + f.blob_f4);
    t.objects.assign(objs, objs + f.num_objects);
    if (f.tri_uv) t.tri_uv.assign(f.tri_uv, f.tri_uv + (size_t)f.num_triangles * 6);
    std::vector<float> uv0((size_t)n * 6, 0.0f);
    const std::vector<int> &order = a.b->objs[MAIN].order;
    CHECK((int)order.size() == n, "the builder keeps the commit order");
    if (f.tri_uv)
        for (int k = 0; k < n; k++) std::memcpy(&uv0[(size_t)order[(size_t)k] * 6], f.tri_uv + (size_t)(objs[MAIN].prim_start + k) * 6, 24);
    execute(p, commit_new.data(), uv0, f, MAIN, objs[MAIN].prim_start, 0, 0, t, rng);
    CHECK(!std::memcmp(t.blob.data(), b.v.blob, (size_t)f.blob_f4 * 16), "the blob after the update is the fresh commit's");
    CHECK(!std::memcmp(t.objects.data(), b.v.objects, (size_t)f.num_objects * sizeof(rt_object)), "the object table after the update is the fresh commit's");
    CHECK(!f.tri_uv == !b.v.tri_uv && (!f.tri_uv || !std::memcmp(t.tri_uv.data(), b.v.tri_uv, t.tri_uv.size() * 4)), "the texture coordinates after the update are the fresh commit's");
    return 0;
}

// ---- 1: the plan against the builder -------------------------------------------------------------------------------------------------------
static int plan_equals_builder(int n, std::mt19937 &rng)
{
    g_n = n;
    const std::vector<float> tris = random_soup(rng, n);
    rt_scene_builder *b = nullptr;
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    rt_material plain;
    rt_material_standard(&plain, grey, 0.2f);
    CHECK(rt_scene_builder_create(&b) == RT_OK, "a builder");
    const rt_status st = rt_scene_add_mesh(b, tris.data(), n, &plain);
    rt_rb_plan p;
    const bool planned = rt_rb_make_plan(n, p);
    int bad = 0;
    if (st != RT_OK || !planned) {
        bad = !(st == RT_ERR_UNSUPPORTED && !planned);   // a count the builder refuses has no plan, and the other way round
    } else {
        const HostObject &o = b->objs[0];
        bad |= o.root_ref != p.root_ref || o.stack_need != p.stack_need || o.nodes.size() != p.slots.size() || (int)o.order.size() != n;
        for (size_t k = 0; k < o.nodes.size() && !bad; k++) bad |= rt_f2u(o.nodes[k].q[3].x) != p.lref[k] || rt_f2u(o.nodes[k].q[3].y) != p.rref[k];
        for (int level = 0; level <= RT_BVH_DEPTH && !bad; level++) {
            int at = 0;
            for (int i = 0; i < (1 << level); i++) {
                const rt_rb_seg seg = p.segs[(size_t)rt_rb_heap(level, i)];
                bad |= seg.count < 0 || (seg.count > 0 && seg.start != at);
                at += seg.count;
            }
            bad |= at != n;
        }
        const int top = p.segs[(size_t)rt_rb_heap(p.local_level, 0)].count;
        bad |= top > RT_REBUILD_LDS_TRIS || (p.local_level > 0 && p.segs[(size_t)rt_rb_heap(p.local_level - 1, 0)].count <= RT_REBUILD_LDS_TRIS);
    }
    rt_scene_builder_destroy(b);
    CHECK(!bad, "the plan is the builder's tree");
    return 0;
}

// ---- 3: the refusals ------------------------------------------------------------------------------------------------------------------------
static bool said(const rt_ctx &ctx, const char *what) { return ctx.err.find(what) != std::string::npos; }

static int refusals()
{
    g_case = "refusals";
    rt_ctx ctx, other;
    rt_scene scene, foreign, empty;
    scene.ctx = &ctx; foreign.ctx = &other; empty.ctx = &ctx;
    scene.uid = 41; empty.uid = 42;
    auto object = [](int type, int prim_start) { rt_object o; std::memset(&o, 0, sizeof o); o.type = type; o.prim_start = prim_start; return o; };
    scene.flat.objects = {object(RT_OBJ_SPHERE, 0), object(RT_OBJ_MESH, 0), object(RT_OBJ_QUAD, 5)};
    scene.flat.num_tris = 7;
    foreign.flat = scene.flat;
    empty.flat.objects = {object(RT_OBJ_MESH, 0), object(RT_OBJ_SPHERE, 0)};
    std::vector<float> tris(5 * 9, 0.25f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int form = 0; form < 2; form++) {
        auto call = [&](rt_ctx *c, rt_scene *s, int32_t oi, const float *t, int32_t n) {
            return form ? rt_scene_update_mesh(c, s, oi, t, n) : rt_scene_update_mesh_device(c, s, oi, t, n, nullptr);
        };
        g_n = form;
        ctx.err.clear();
        CHECK(call(nullptr, &scene, 1, tris.data(), 5) == RT_ERR_INVALID, "null context");
        CHECK(call(&ctx, nullptr, 1, tris.data(), 5) == RT_ERR_INVALID && said(ctx, "null argument"), "null scene");
        CHECK(call(&ctx, &foreign, 1, tris.data(), 5) == RT_ERR_INVALID && said(ctx, "another context"), "a scene of another context");
        CHECK(call(&ctx, &scene, -1, tris.data(), 5) == RT_ERR_INVALID && said(ctx, "out of range"), "a negative index");
        CHECK(call(&ctx, &scene, 3, tris.data(), 5) == RT_ERR_INVALID && said(ctx, "out of range"), "an index past the objects");
        CHECK(call(&ctx, &scene, 0, tris.data(), 5) == RT_ERR_INVALID && said(ctx, "not a mesh"), "a sphere");
        CHECK(call(&ctx, &scene, 2, tris.data(), 2) == RT_ERR_INVALID && said(ctx, "not a mesh"), "a quad");
        CHECK(call(&ctx, &scene, 1, tris.data(), 4) == RT_ERR_INVALID && said(ctx, "triangle count"), "fewer triangles");
        CHECK(call(&ctx, &scene, 1, tris.data(), 6) == RT_ERR_INVALID && said(ctx, "triangle count"), "more triangles");
        CHECK(call(&ctx, &scene, 1, tris.data(), 0) == RT_ERR_INVALID && said(ctx, "triangle count"), "no triangles for a mesh that has some");
        CHECK(call(&ctx, &scene, 1, nullptr, 5) == RT_ERR_INVALID && said(ctx, "null argument"), "null triangles");
        CHECK(call(&ctx, &empty, 0, nullptr, 0) == RT_OK && call(&ctx, &empty, 0, tris.data(), 0) == RT_OK, "an empty mesh: nothing to do");
        CHECK(call(&ctx, &empty, 0, tris.data(), 1) == RT_ERR_INVALID && said(ctx, "triangle count"), "a triangle for an empty mesh");
    }
    const float bad[] = {nan, inf, -inf, 2.0f * RT_REBUILD_MAX_COORD, -1e30f};
    for (float v : bad)
        for (size_t at : {(size_t)0, (size_t)22, tris.size() - 1}) {
            std::vector<float> t = tris;
            t[at] = v;
            CHECK(rt_scene_update_mesh(&ctx, &scene, 1, t.data(), 5) == RT_ERR_INVALID && said(ctx, "not finite"), "a vertex that is not finite, or too large");
        }
    CHECK(g_launches == 0, "a refused call reached a launcher");
    CHECK(!ctx.launched && !ctx.have_timing && ctx.last_stream == nullptr, "a refused call touched the launch order");
    CHECK(scene.uid == 41 && empty.uid == 42 && scene.updates.empty() && empty.updates.empty(), "a refused call touched the scene");
    return 0;
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int every = argc > 2 ? std::atoi(argv[2]) : 3000;
    std::mt19937 rng(seed);
    // 1
    g_case = "plan";
    for (int n = 0; n <= every; n++)
        if (plan_equals_builder(n, rng)) return 1;
    // larger ones: the first count with a global level, the 50,880-triangle surface's, a mesh near 200,000, one near the limit (the reference's leaves hold
    // at most 1,023 triangles) and 2^20 - 1, which the builder refuses
    std::vector<int> larger;
    for (int k = 3; k < argc; k++) larger.push_back(std::atoi(argv[k]));
    if (argc <= 3) larger = {RT_REBUILD_LDS_TRIS + 1, 50880, 200000 + (int)(rng() % 1000), 1040000 + (int)(rng() % 1000), (1 << 20) - 1};
    for (int n : larger)
        if (plan_equals_builder(n, rng)) return 1;
    // 2
    const std::vector<float> second = random_soup(rng, 37);
    const int sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 100, 1023, 1024, 1025, 2047, 2049, RT_REBUILD_LDS_TRIS + 1, 2 * RT_REBUILD_LDS_TRIS + 3, 6000};
    for (int n : sizes) {
        g_n = n;
        g_case = "random";
        if (update_equals_commit(random_soup(rng, n), random_soup(rng, n), n, false, second, rng)) return 1;
        // ties: every triangle four times; a fan around one p0; all triangles the same
        std::vector<float> dup = random_soup(rng, n), fan = random_soup(rng, n), same = random_soup(rng, n);
        for (int i = 0; i < n; i++) {
            std::memcpy(&dup[(size_t)i * 9], &dup[(size_t)(i / 4) * 9], 36);
            std::memcpy(&fan[(size_t)i * 9], &fan[0], 12);
            std::memcpy(&same[(size_t)i * 9], &same[0], 36);
        }
        g_case = "every triangle four times";
        if (update_equals_commit(random_soup(rng, n), dup, n, false, second, rng)) return 1;
        g_case = "a fan";
        if (update_equals_commit(random_soup(rng, n), fan, n, false, second, rng)) return 1;
        g_case = "identical triangles";
        if (update_equals_commit(random_soup(rng, n), same, n, false, second, rng)) return 1;
        // signed zeros: a triangle's coordinates are -0, +0 or of one sign, so a box of triangles of the positive kind has its low planes at a
        // zero and one of the negative kind its high planes, at whichever zero its list meets first (a.x, b.y, c.z are not zero: no zero area)
        std::vector<float> zeros((size_t)n * 9);
        for (int i = 0; i < n; i++) {
            const float sign = rng() & 1 ? 1.0f : -1.0f;
            for (int e = 0; e < 9; e++) {
                const unsigned r = rng() % 3;
                zeros[(size_t)i * 9 + e] = (r == 0 && e != 0 && e != 4 && e != 8) ? -0.0f : (r == 1 && e != 0 && e != 4 && e != 8) ? 0.0f : sign * uniform(rng, 0.5f, 1.5f);
            }
        }
        g_case = "signed zeros";
        if (update_equals_commit(random_soup(rng, n), zeros, n, false, second, rng)) return 1;
        if (n % 2 == 0) {                // texture coordinates: an .obj of quads under a material that needs them
            std::vector<float> va((size_t)(n / 2) * 12), vb(va.size());
            for (float &x : va) x = uniform(rng, -1.0f, 1.0f);
            for (float &x : vb) x = uniform(rng, -1.0f, 1.0f);
            g_case = "texture coordinates";
            if (update_equals_commit(va, vb, n, true, second, rng)) return 1;
        }
    }
    // 3
    if (refusals()) return 1;
    std::printf("update host side: plans up to %d and %d larger, %d sizes of meshes, sanitizers silent\n", every, (int)larger.size(), (int)(sizeof sizes / sizeof sizes[0]));
    return 0;
}
