/*
 * rt_winding_capi.cpp — the winding-number queries of the C ABI (include/rt_amd.h): argument checks, the scene's flip bytes on the device,
 * the host-buffer forms.  The kernel is rt_winding_kernel.h, the arithmetic rt_winding.h; rt_signed_distance_device also runs the
 * nearest-surface kernel (as rt_nearest_capi.cpp runs it).  The context, the scene, the launch bracket and the ray kernels' enqueue are
 * rt_internal.h's.  The fast forms (rt_winding_numbers_fast[_device], rt_signed_distance_fast[_device]) are here too: the scene's cluster
 * trees built on the host and uploaded at its first fast query, their refit queued ahead of a query when the moments are stale, and the
 * two debug views of the trees (rt_debug_winding_tree, rt_debug_scene_winding_tree).
 */
#include <cstdint>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "rt_internal.h"
#include "rt_nearest.h"
#include "rt_winding.h"

namespace {

rt_status check_winding(rt_ctx *ctx, const rt_scene *scene, const void *points, int64_t n, int32_t object, const void *winding, const void *inside)
{
    rt_status st = check_points(ctx, scene, points, n);
    if (st != RT_OK) return st;
    if (object != RT_WINDING_SOLIDS && (object < 0 || (size_t)object >= scene->flat.objects.size()))
        return set_err(ctx, RT_ERR_INVALID, "object is neither RT_WINDING_SOLIDS nor an index of the scene's object list");
    if (n > 0 && !winding && !inside) return set_err(ctx, RT_ERR_INVALID, "null argument (one of the two outputs is needed)");
    return RT_OK;
}

/* what the kernel reads beside the blob, made at the scene's first query: the triangle order (unless an update already made it) and the
 * flip bytes in commit order, four to a word */
rt_status prepare_scene(rt_ctx *ctx, rt_scene *scene)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const rt_status st = ensure_scene_perm(ctx, scene);
    if (st != RT_OK) return st;
    if (scene->d_flip.p) return RT_OK;
    const std::vector<uint8_t> &bytes = scene->flat.tri_flip_commit;
    std::vector<uint32_t> words((bytes.size() + 3) / 4, 0u);
    if (!bytes.empty()) std::memcpy(words.data(), bytes.data(), bytes.size());
    RT_HIP(ctx, scene->d_flip.grow(words.size()), "allocating the scene's flip bytes");
    const hipError_t e = words.empty() ? hipSuccess : hipMemcpy(scene->d_flip.p, words.data(), words.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        scene->d_flip.release();
        return hip_fail(ctx, e, "uploading the scene's flip bytes");
    }
    return RT_OK;
}

rt_winding_args winding_args(const rt_ctx *ctx, const rt_scene *scene, const float *d_points, uint32_t n, int32_t object)
{
    rt_winding_args a;
    std::memset(&a, 0, sizeof a);
    a.blob = scene->d_blob.p;
    a.off_tris = scene->flat.off_tris;
    a.off_objtab = scene->flat.off_objtab;
    a.num_objects = (int32_t)scene->flat.objects.size();
    a.num_tris = scene->flat.num_tris;
    a.perm = scene->d_perm.p;
    a.flip = scene->d_flip.p;
    a.n = n;
    a.num_chunks = (n + 63u) / 64u;
    a.counter = ctx->tile_counter.p;
    a.points = d_points;
    a.object = object;
    return a;
}

rt_status enqueue_winding(rt_ctx *ctx, const rt_winding_args &a, hipStream_t stream)
{
    RT_HIP(ctx, hipMemsetAsync(a.counter, 0, 512, stream), "clearing the point counter");
    RT_HIP(ctx, rt_launch_winding(&a, ctx->num_cus, stream), "launching winding-number kernel");
    return RT_OK;
}

/* ---- the fast queries: the scene's cluster trees ------------------------------------------------------------------------------------ */
int32_t mesh_tris(const FlatScene &f, size_t oi)
{
    const int32_t end = oi + 1 < f.objects.size() ? f.objects[oi + 1].prim_start : f.num_tris;
    return end - f.objects[oi].prim_start;
}

/* the topology of every mesh of a flattened scene, from its commit-time records in commit order (rt_winding.h's builder) */
void build_trees(const FlatScene &f, rt_wn_tree &T)
{
    rt_wn_tree_init(T, (int32_t)f.objects.size(), f.num_tris);
    std::vector<float> centroids;
    for (size_t oi = 0; oi < f.objects.size(); oi++) {
        if (f.objects[oi].type != RT_OBJ_MESH) continue;
        const int32_t base = f.objects[oi].prim_start, n = mesh_tris(f, oi);
        centroids.assign((size_t)n * 3, 0.0f);
        for (int32_t k = 0; k < n; k++) {
            const rt_f4 *q = &f.blob[(size_t)f.off_tris + 3 * ((size_t)base + k)];
            const int32_t commit = f.tri_order[(size_t)base + k];
            if (commit < 0 || commit >= n) continue;
            float *c = &centroids[3 * (size_t)commit];
            c[0] = q[0].x + (q[0].w + q[1].z) * RT_WN_THIRD;
            c[1] = q[0].y + (q[1].x + q[1].w) * RT_WN_THIRD;
            c[2] = q[0].z + (q[1].y + q[2].x) * RT_WN_THIRD;
        }
        rt_wn_build_mesh(T, (int32_t)oi, centroids.data(), n, base);
    }
    rt_wn_tree_finish(T);
}

std::vector<uint32_t> flip_words(const FlatScene &f)
{
    std::vector<uint32_t> words((f.tri_flip_commit.size() + 3) / 4, 0u);
    if (!f.tri_flip_commit.empty()) std::memcpy(words.data(), f.tri_flip_commit.data(), f.tri_flip_commit.size());
    return words;
}

template <class T> void take(DevBuf<T> &into, DevBuf<T> &from)
{
    into.release();
    into.p = from.p; into.cap = from.cap;
    from.p = nullptr; from.cap = 0;
}

/* prepare_scene's fast counterpart: at the scene's first fast query the trees are built on the host and their tables uploaded.  Everything is
 * allocated and copied into buffers of this function first: a failure leaves the scene as it was, without trees. */
rt_status prepare_scene_fast(rt_ctx *ctx, rt_scene *scene)
{
    const rt_status st = prepare_scene(ctx, scene);
    if (st != RT_OK || scene->wn_built) return st;
    rt_wn_tree T;
    build_trees(scene->flat, T);
    const std::vector<int32_t> topo = rt_wn_tree_topo(T);
    std::vector<int32_t> ints(T.object_range);
    ints.insert(ints.end(), T.inv.begin(), T.inv.end());
    ints.insert(ints.end(), T.levels.begin(), T.levels.end());
    const size_t clusters = T.skip.size();
    DevBuf<rt_f4> d_topo, d_rec, d_sums, d_moments;
    DevBuf<int32_t> d_ints;
    RT_HIP(ctx, d_topo.grow(clusters), "allocating the scene's cluster trees");
    RT_HIP(ctx, d_ints.grow(ints.size()), "allocating the scene's cluster trees");
    RT_HIP(ctx, d_rec.grow(3 * (size_t)scene->flat.num_tris), "allocating the scene's gathered records");
    RT_HIP(ctx, d_sums.grow(4 * clusters), "allocating the scene's cluster sums");
    RT_HIP(ctx, d_moments.grow(2 * clusters), "allocating the scene's cluster moments");
    if (clusters) RT_HIP(ctx, hipMemcpy(d_topo.p, topo.data(), topo.size() * 4, hipMemcpyHostToDevice), "uploading the scene's cluster trees");
    if (!ints.empty()) RT_HIP(ctx, hipMemcpy(d_ints.p, ints.data(), ints.size() * 4, hipMemcpyHostToDevice), "uploading the scene's cluster trees");
    take(scene->d_wn_topo, d_topo);
    take(scene->d_wn_ints, d_ints);
    take(scene->d_wn_rec, d_rec);
    take(scene->d_wn_sums, d_sums);
    take(scene->d_wn_moments, d_moments);
    scene->wn_tree = std::move(T);
    scene->wn_built = true;
    scene->wn_stale = true;
    return RT_OK;
}

rt_winding_args fast_args(const rt_ctx *ctx, const rt_scene *scene, const float *d_points, uint32_t n, int32_t object, float beta)
{
    rt_winding_args a = winding_args(ctx, scene, d_points, n, object);
    const rt_wn_tree &T = scene->wn_tree;
    a.op = RT_WN_OP_FAST;
    a.beta2 = beta * beta;
    a.topo = scene->d_wn_topo.p;
    a.object_range = scene->d_wn_ints.p;
    a.inv = a.object_range + T.object_range.size();
    a.levels = a.inv + T.inv.size();
    a.rec = scene->d_wn_rec.p;
    a.sums = scene->d_wn_sums.p;
    a.moments = scene->d_wn_moments.p;
    return a;
}

/* the refit on `stream`: every mesh's records into cluster order, the leaves, then the internal clusters one height at a time.  For a caller
 * inside the launch bracket. */
rt_status enqueue_refit(rt_ctx *ctx, const rt_scene *scene, hipStream_t stream)
{
    const FlatScene &f = scene->flat;
    const rt_wn_tree &T = scene->wn_tree;
    rt_winding_args a = fast_args(ctx, scene, nullptr, 0, RT_WINDING_SOLIDS, 1.0f);
    a.op = RT_WN_OP_GATHER;
    for (size_t oi = 0; oi < f.objects.size(); oi++) {
        if (f.objects[oi].type != RT_OBJ_MESH) continue;
        a.mesh_base = f.objects[oi].prim_start;
        a.mesh_count = mesh_tris(f, oi);
        RT_HIP(ctx, rt_launch_winding(&a, ctx->num_cus, stream), "launching the cluster trees' gather kernel");
    }
    for (size_t h = 0; h + 1 < T.level_off.size(); h++) {
        a.op = h == 0 ? RT_WN_OP_LEAVES : RT_WN_OP_COMBINE;
        a.range_first = T.level_off[h];
        a.range_count = T.level_off[h + 1] - T.level_off[h];
        RT_HIP(ctx, rt_launch_winding(&a, ctx->num_cus, stream), "launching the cluster trees' moment kernels");
    }
    return RT_OK;
}

/* the fast query's work inside the bracket: the refit first where the moments are stale */
rt_status enqueue_fast(rt_ctx *ctx, rt_scene *scene, const rt_winding_args &a, hipStream_t stream)
{
    if (scene->wn_stale) {
        const rt_status st = enqueue_refit(ctx, scene, stream);
        if (st != RT_OK) return st;
    }
    return enqueue_winding(ctx, a, stream);
}

rt_status check_beta(rt_ctx *ctx, float beta)
{
    if (!(beta > 0.0f)) return set_err(ctx, RT_ERR_INVALID, "beta must be greater than zero (+inf is allowed)");
    return RT_OK;
}

/* rt_debug_winding_tree's copy, owned by the builder */
struct WindingDebug {
    rt_wn_tree tree;
    std::vector<int32_t> position;
    std::vector<rt_f4> rec, sums, moments;
};

/* per [base + cluster position] the flattened index of the record that holds that triangle, from a triangle list (position -> commit index) */
std::vector<int32_t> positions(const rt_wn_tree &T, const FlatScene &f, const int32_t *perm)
{
    std::vector<int32_t> at(T.order.size() + 1, 0);
    for (size_t oi = 0; oi < f.objects.size(); oi++) {
        if (f.objects[oi].type != RT_OBJ_MESH) continue;
        const int32_t base = f.objects[oi].prim_start, n = mesh_tris(f, oi);
        for (int32_t k = 0; k < n; k++) {
            const int32_t commit = perm[(size_t)base + k];
            if (commit >= 0 && commit < n) at[(size_t)T.inv[(size_t)base + commit]] = base + k;
        }
    }
    return at;
}

void fill_view(const rt_wn_tree &T, const std::vector<int32_t> &position, const float *moments, rt_winding_tree_view *out)
{
    out->position = position.data();
    out->skip = T.skip.data(); out->first = T.first.data(); out->count = T.count.data();
    out->num_clusters = (int32_t)T.skip.size();
    out->object_range = T.object_range.data();
    out->num_objects = (int32_t)(T.object_range.size() / 2);
    out->order = T.order.data();
    out->num_triangles = (int32_t)T.order.size();
    out->moments = moments;
}

}  // namespace

extern "C" rt_status rt_debug_winding_tree(rt_scene_builder *b, rt_winding_tree_view *out)
{
    if (!b || !out) return RT_ERR_INVALID;
    rt_flat_view flat;
    const rt_status st = rt_debug_flatten(b, &flat);
    if (st != RT_OK) return st;
    const FlatScene &f = *b->debug_flat;
    WindingDebug *d = new (std::nothrow) WindingDebug();
    if (!d) return RT_ERR_NOMEM;
    if (b->debug_winding) b->debug_winding_free(b->debug_winding);
    b->debug_winding = d;
    b->debug_winding_free = [](void *p) { delete static_cast<WindingDebug *>(p); };
    build_trees(f, d->tree);
    /* the host's gather and refit, through the text the device compiles */
    const std::vector<uint32_t> words = flip_words(f);
    rt_wn_scene<rt_f4> S;
    S.tris = f.blob.data() + f.off_tris; S.objtab = f.blob.data() + f.off_objtab; S.perm = f.tri_order.data(); S.flip = words.data();
    S.num_objects = (int32_t)f.objects.size(); S.num_tris = f.num_tris;
    const size_t clusters = d->tree.skip.size();
    d->rec.assign(3 * (size_t)f.num_tris + 1, rt_f4{0, 0, 0, 0});
    d->sums.assign(4 * clusters + 1, rt_f4{0, 0, 0, 0});
    d->moments.assign(2 * clusters + 1, rt_f4{0, 0, 0, 0});
    for (size_t oi = 0; oi < f.objects.size(); oi++) {
        if (f.objects[oi].type != RT_OBJ_MESH) continue;
        const int32_t base = f.objects[oi].prim_start, n = mesh_tris(f, oi);
        for (int32_t j = 0; j < n; j++) rt_wn_gather(S, d->tree.inv.data(), d->rec.data(), base, n, j);
    }
    rt_wn_host_refit(d->tree, d->rec.data(), d->sums.data(), d->moments.data());
    d->position = positions(d->tree, f, f.tri_order.data());
    fill_view(d->tree, d->position, reinterpret_cast<const float *>(d->moments.data()), out);
    return RT_OK;
}

extern "C" rt_status rt_debug_scene_winding_tree(rt_ctx *ctx, rt_scene *scene, rt_winding_tree_view *out)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!out) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if ((st = prepare_scene_fast(ctx, scene)) != RT_OK) return st;
    if (scene->wn_stale) {
        st = launch_bracket(ctx, nullptr, [&]() -> rt_status { return enqueue_refit(ctx, scene, nullptr); });
        if (st != RT_OK) return st;
        scene->wn_stale = false;
    }
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for the device");
    const size_t clusters = scene->wn_tree.skip.size();
    scene->wn_read.assign(8 * clusters + 1, 0.0f);
    if (clusters) RT_HIP(ctx, hipMemcpy(scene->wn_read.data(), scene->d_wn_moments.p, clusters * 32, hipMemcpyDeviceToHost), "reading the cluster moments");
    std::vector<int32_t> perm(scene->flat.tri_order.size() + 1, 0);
    if (!scene->flat.tri_order.empty()) RT_HIP(ctx, hipMemcpy(perm.data(), scene->d_perm.p, scene->flat.tri_order.size() * 4, hipMemcpyDeviceToHost), "reading the triangle list");
    scene->wn_position = positions(scene->wn_tree, scene->flat, perm.data());
    fill_view(scene->wn_tree, scene->wn_position, scene->wn_read.data(), out);
    return RT_OK;
}

extern "C" rt_status rt_winding_numbers_fast_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, int64_t n, int32_t object, float beta,
                                                    float *d_winding, uint8_t *d_inside, void *hip_stream)
{
    rt_status st = check_winding(ctx, scene, d_points, n, object, d_winding, d_inside);
    if (st != RT_OK) return st;
    if ((st = check_beta(ctx, beta)) != RT_OK) return st;
    if (n == 0) return RT_OK;
    if ((st = prepare_scene_fast(ctx, scene)) != RT_OK) return st;
    rt_winding_args a = fast_args(ctx, scene, d_points, (uint32_t)n, object, beta);
    a.winding = d_winding;
    a.inside = d_inside;
    hipStream_t stream = (hipStream_t)hip_stream;
    st = launch_bracket(ctx, stream, [&]() -> rt_status { return enqueue_fast(ctx, scene, a, stream); });
    if (st == RT_OK) scene->wn_stale = false;
    return st;
}

extern "C" rt_status rt_winding_numbers_fast(rt_ctx *ctx, rt_scene *scene, const float *points, int64_t n, int32_t object, float beta, float *winding,
                                             uint8_t *inside)
{
    rt_status st = check_winding(ctx, scene, points, n, object, winding, inside);
    if (st != RT_OK) return st;
    if ((st = check_beta(ctx, beta)) != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(floats + 2 * (size_t)n), "allocating the points");
    float *d_w = ctx->d_query_in.p + floats;
    uint8_t *d_in = (uint8_t *)(d_w + (size_t)n);
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    st = rt_winding_numbers_fast_device(ctx, scene, ctx->d_query_in.p, n, object, beta, winding ? d_w : nullptr, inside ? d_in : nullptr, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "winding-number kernel");
    if (winding) RT_HIP(ctx, hipMemcpy(winding, d_w, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the winding numbers to host");
    if (inside) RT_HIP(ctx, hipMemcpy(inside, d_in, (size_t)n, hipMemcpyDeviceToHost), "copying the containment bytes to host");
    return RT_OK;
}

extern "C" rt_status rt_signed_distance_fast_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n, float beta,
                                                    rt_nearest *d_nearest, float *d_sdf, void *hip_stream)
{
    rt_status st = check_points(ctx, scene, d_points, n);
    if (st != RT_OK) return st;
    if ((st = check_beta(ctx, beta)) != RT_OK) return st;
    if (n > 0 && !d_sdf) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if ((uintptr_t)d_nearest & 15u) return set_err(ctx, RT_ERR_INVALID, "d_nearest must be 16-byte aligned");
    if (n == 0) return RT_OK;
    if ((st = prepare_scene_fast(ctx, scene)) != RT_OK) return st;
    if (!d_nearest) {
        if (ctx->d_query_out.cap < (size_t)n * 2 || !ctx->d_query_out.p) {
            if (ctx->launched) RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for the launch that uses the records");
            RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
        }
        d_nearest = (rt_nearest *)ctx->d_query_out.p;
    }
    rt_nearest_args na = ray_args_scene<rt_nearest_args>(ctx, scene, (uint32_t)n);
    na.points = d_points;
    na.max_dist = d_max_dist;
    na.out = d_nearest;
    rt_winding_args wa = fast_args(ctx, scene, d_points, (uint32_t)n, RT_WINDING_SOLIDS, beta);
    wa.nearest = d_nearest;
    wa.sdf = d_sdf;
    hipStream_t stream = (hipStream_t)hip_stream;
    st = launch_bracket(ctx, stream, [&]() -> rt_status {
        const rt_status queued = enqueue_rays(ctx, scene, na, rt_launch_nearest, false, "clearing the point counter", "launching nearest-surface kernel", stream);
        return queued != RT_OK ? queued : enqueue_fast(ctx, scene, wa, stream);
    });
    if (st == RT_OK) scene->wn_stale = false;
    return st;
}

extern "C" rt_status rt_signed_distance_fast(rt_ctx *ctx, rt_scene *scene, const float *points, const float *max_dist, int64_t n, float beta,
                                             rt_nearest *nearest, float *sdf)
{
    rt_status st = check_points(ctx, scene, points, n);
    if (st != RT_OK) return st;
    if ((st = check_beta(ctx, beta)) != RT_OK) return st;
    if (n > 0 && !sdf) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(floats + 2 * (size_t)n), "allocating the points");
    RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
    float *d_lim = ctx->d_query_in.p + floats, *d_sdf = d_lim + (size_t)n;
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    if (max_dist) RT_HIP(ctx, hipMemcpy(d_lim, max_dist, (size_t)n * 4, hipMemcpyHostToDevice), "copying the limits");
    st = rt_signed_distance_fast_device(ctx, scene, ctx->d_query_in.p, max_dist ? d_lim : nullptr, n, beta, (rt_nearest *)ctx->d_query_out.p, d_sdf, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "signed-distance kernels");
    RT_HIP(ctx, hipMemcpy(sdf, d_sdf, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the signed distances to host");
    if (nearest) RT_HIP(ctx, hipMemcpy(nearest, ctx->d_query_out.p, (size_t)n * sizeof(rt_nearest), hipMemcpyDeviceToHost), "copying the records to host");
    return RT_OK;
}

extern "C" rt_status rt_winding_numbers_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, int64_t n, int32_t object, float *d_winding,
                                               uint8_t *d_inside, void *hip_stream)
{
    rt_status st = check_winding(ctx, scene, d_points, n, object, d_winding, d_inside);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if ((st = prepare_scene(ctx, scene)) != RT_OK) return st;
    rt_winding_args a = winding_args(ctx, scene, d_points, (uint32_t)n, object);
    a.winding = d_winding;
    a.inside = d_inside;
    hipStream_t stream = (hipStream_t)hip_stream;
    return launch_bracket(ctx, stream, [&]() -> rt_status { return enqueue_winding(ctx, a, stream); });
}

extern "C" rt_status rt_winding_numbers(rt_ctx *ctx, rt_scene *scene, const float *points, int64_t n, int32_t object, float *winding, uint8_t *inside)
{
    rt_status st = check_winding(ctx, scene, points, n, object, winding, inside);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the points, the winding numbers and the bytes (a float's room each), one after the other */
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(floats + 2 * (size_t)n), "allocating the points");
    float *d_w = ctx->d_query_in.p + floats;
    uint8_t *d_in = (uint8_t *)(d_w + (size_t)n);
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    st = rt_winding_numbers_device(ctx, scene, ctx->d_query_in.p, n, object, winding ? d_w : nullptr, inside ? d_in : nullptr, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "winding-number kernel");
    if (winding) RT_HIP(ctx, hipMemcpy(winding, d_w, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the winding numbers to host");
    if (inside) RT_HIP(ctx, hipMemcpy(inside, d_in, (size_t)n, hipMemcpyDeviceToHost), "copying the containment bytes to host");
    return RT_OK;
}

extern "C" rt_status rt_signed_distance_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n,
                                               rt_nearest *d_nearest, float *d_sdf, void *hip_stream)
{
    rt_status st = check_points(ctx, scene, d_points, n);
    if (st != RT_OK) return st;
    if (n > 0 && !d_sdf) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if ((uintptr_t)d_nearest & 15u) return set_err(ctx, RT_ERR_INVALID, "d_nearest must be 16-byte aligned");
    if (n == 0) return RT_OK;
    if ((st = prepare_scene(ctx, scene)) != RT_OK) return st;
    if (!d_nearest) {
        /* the context's record buffer: grown once what may still read the old one has run */
        static_assert(sizeof(rt_nearest) == 2 * sizeof(rt_f4), "rt_nearest is two 16-byte units");
        if (ctx->d_query_out.cap < (size_t)n * 2 || !ctx->d_query_out.p) {
            if (ctx->launched) RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for the launch that uses the records");
            RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
        }
        d_nearest = (rt_nearest *)ctx->d_query_out.p;
    }
    rt_nearest_args na = ray_args_scene<rt_nearest_args>(ctx, scene, (uint32_t)n);
    na.points = d_points;
    na.max_dist = d_max_dist;
    na.out = d_nearest;
    rt_winding_args wa = winding_args(ctx, scene, d_points, (uint32_t)n, RT_WINDING_SOLIDS);
    wa.nearest = d_nearest;
    wa.sdf = d_sdf;
    hipStream_t stream = (hipStream_t)hip_stream;
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        const rt_status queued = enqueue_rays(ctx, scene, na, rt_launch_nearest, false, "clearing the point counter", "launching nearest-surface kernel", stream);
        return queued != RT_OK ? queued : enqueue_winding(ctx, wa, stream);
    });
}

extern "C" rt_status rt_signed_distance(rt_ctx *ctx, rt_scene *scene, const float *points, const float *max_dist, int64_t n, rt_nearest *nearest,
                                        float *sdf)
{
    rt_status st = check_points(ctx, scene, points, n);
    if (st != RT_OK) return st;
    if (n > 0 && !sdf) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the points, the limits and the signed distances, one after the other; the records in the context's record buffer */
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(floats + 2 * (size_t)n), "allocating the points");
    RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
    float *d_lim = ctx->d_query_in.p + floats, *d_sdf = d_lim + (size_t)n;
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    if (max_dist) RT_HIP(ctx, hipMemcpy(d_lim, max_dist, (size_t)n * 4, hipMemcpyHostToDevice), "copying the limits");
    st = rt_signed_distance_device(ctx, scene, ctx->d_query_in.p, max_dist ? d_lim : nullptr, n, (rt_nearest *)ctx->d_query_out.p, d_sdf, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "signed-distance kernels");
    RT_HIP(ctx, hipMemcpy(sdf, d_sdf, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the signed distances to host");
    if (nearest) RT_HIP(ctx, hipMemcpy(nearest, ctx->d_query_out.p, (size_t)n * sizeof(rt_nearest), hipMemcpyDeviceToHost), "copying the records to host");
    return RT_OK;
}
