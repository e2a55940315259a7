/*
 * rt_update_capi.cpp — time-varying geometry of the C ABI (include/rt_amd.h): rt_scene_update_mesh[_device] rebuild one committed mesh's BVH
 * from new vertices on the device, and rt_debug_scene_read shows the tests what is there afterwards.  The kernels are rt_rebuild_kernel.h's, the
 * plan and the arithmetic rt_rebuild.h's; the context, the scene and the launch bracket are rt_internal.h's.
 *
 * What the host keeps of a committed scene (rt_scene::flat) is not rewritten by an update: its sizes, offsets, references and the commit-time
 * texture coordinates and triangle order never change, and the one geometric thing read from it after commit - the meshes' root boxes in
 * flat.objects, by rt_sched::guessed_order and views_job_order - only orders a schedule.
 */
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_math.h"

namespace {

int32_t mesh_count(const FlatScene &f, size_t oi)
{
    const int32_t end = oi + 1 < f.objects.size() ? f.objects[oi + 1].prim_start : f.num_tris;
    return end - f.objects[oi].prim_start;
}

/* every refusal the two entry points share: none needs the device */
rt_status check_update(rt_ctx *ctx, const rt_scene *scene, int32_t object_index, const float *triangles, int32_t n)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    const FlatScene &f = scene->flat;
    if (object_index < 0 || (size_t)object_index >= f.objects.size()) return set_err(ctx, RT_ERR_INVALID, "object index out of range");
    if (f.objects[(size_t)object_index].type != RT_OBJ_MESH) return set_err(ctx, RT_ERR_INVALID, "the object is not a mesh");
    if (n != mesh_count(f, (size_t)object_index)) return set_err(ctx, RT_ERR_INVALID, "the triangle count differs from the mesh's (a mesh that grows or shrinks is rt_scene_commit's)");
    if (n > 0 && !triangles) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return RT_OK;
}

/* a child or root reference relative to its mesh -> as the flattener stores it (rt_flatten's rebase) */
uint32_t rebase(uint32_t ref, uint32_t tri_base, uint32_t node_base)
{
    const uint32_t chain = ref & RT_REF_CHAIN;
    if (ref & RT_REF_LEAF) {
        const uint32_t count = (ref >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX;
        if (count == 0) return RT_REF_EMPTY_LEAF;
        return RT_REF_LEAF | chain | (count << RT_REF_COUNT_SHIFT) | ((ref & RT_REF_START_MASK) + tri_base);
    }
    return ((ref & RT_REF_NODE_MASK) + node_base) | chain;
}

/* the plan's topology is the committed tree's: every stored node's two references, the root's, the stack depth */
bool plan_matches(const FlatScene &f, const MeshUpdate &m, size_t oi)
{
    const rt_rb_plan &p = m.plan;
    if ((size_t)m.node_base + p.slots.size() > (size_t)f.num_nodes || p.stack_need > f.stack_entries) return false;
    if (f.objects[oi].root_ref != rebase(p.root_ref, (uint32_t)m.tri_base, (uint32_t)m.node_base)) return false;
    for (size_t k = 0; k < p.slots.size(); k++) {
        const rt_f4 &q3 = f.blob[(size_t)f.off_nodes + ((size_t)m.node_base + k) * 4 + 3];
        if (rt_f2u(q3.x) != rebase(p.lref[k], (uint32_t)m.tri_base, (uint32_t)m.node_base) || rt_f2u(q3.y) != rebase(p.rref[k], (uint32_t)m.tri_base, (uint32_t)m.node_base)) return false;
    }
    return true;
}

/* a scratch buffer of the context, grown behind the launches that may still use the old one */
template <class T> rt_status grow_scratch(rt_ctx *ctx, DevBuf<T> &buf, size_t need, const char *what)
{
    if (buf.p && buf.cap >= need) return RT_OK;
    if (buf.p && ctx->launched) RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for the update that uses the scratch");
    RT_HIP(ctx, buf.grow(need), what);
    return RT_OK;
}

/* the mesh's plan and what goes with it on the device */
rt_status fill_mesh(rt_ctx *ctx, rt_scene *scene, int32_t object_index, MeshUpdate &m)
{
    const FlatScene &f = scene->flat;
    m.n = mesh_count(f, (size_t)object_index);
    m.tri_base = f.objects[(size_t)object_index].prim_start;
    for (size_t oi = 0; oi < (size_t)object_index; oi++) {
        if (f.objects[oi].type != RT_OBJ_MESH) continue;
        rt_rb_plan before;
        if (!rt_rb_make_plan(mesh_count(f, oi), before)) return set_err(ctx, RT_ERR_UNSUPPORTED, "a mesh of the scene has no plan");
        m.node_base += (int32_t)before.slots.size();
        m.mesh_index++;
    }
    if (!rt_rb_make_plan(m.n, m.plan) || !plan_matches(f, m, (size_t)object_index))
        return set_err(ctx, RT_ERR_UNSUPPORTED, "the mesh's tree is not the one its triangle count implies");
    RT_HIP(ctx, m.d_segs.grow(m.plan.segs.size()), "allocating the update plan");
    RT_HIP(ctx, hipMemcpy(m.d_segs.p, m.plan.segs.data(), m.plan.segs.size() * sizeof(rt_rb_seg), hipMemcpyHostToDevice), "uploading the update plan");
    RT_HIP(ctx, m.d_slots.grow(m.plan.slots.size()), "allocating the update plan");
    if (!m.plan.slots.empty())
        RT_HIP(ctx, hipMemcpy(m.d_slots.p, m.plan.slots.data(), m.plan.slots.size() * sizeof(rt_rb_slot), hipMemcpyHostToDevice), "uploading the update plan");
    if (!f.tri_uv.empty()) {
        std::vector<float> uv0((size_t)m.n * 6);
        for (size_t k = 0; k < (size_t)m.n; k++) std::memcpy(&uv0[(size_t)f.tri_order[(size_t)m.tri_base + k] * 6], &f.tri_uv[((size_t)m.tri_base + k) * 6], 24);
        RT_HIP(ctx, m.d_uv0.grow(uv0.size()), "allocating the mesh's texture coordinates");
        RT_HIP(ctx, hipMemcpy(m.d_uv0.p, uv0.data(), uv0.size() * 4, hipMemcpyHostToDevice), "uploading the mesh's texture coordinates");
    }
    return ensure_scene_perm(ctx, scene);
}

/* ... made at the mesh's first update and kept with the scene */
rt_status prepare_mesh(rt_ctx *ctx, rt_scene *scene, int32_t object_index, MeshUpdate **out)
{
    auto found = scene->updates.find(object_index);
    if (found == scene->updates.end()) {
        found = scene->updates.try_emplace(object_index).first;
        const rt_status st = fill_mesh(ctx, scene, object_index, found->second);
        if (st != RT_OK) { scene->updates.erase(found); return st; }
    }
    *out = &found->second;
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_scene_update_mesh_device(rt_ctx *ctx, rt_scene *scene, int32_t object_index, const float *d_triangles, int32_t n, void *hip_stream)
{
    rt_status st = check_update(ctx, scene, object_index, d_triangles, n);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    MeshUpdate *m = nullptr;
    if ((st = prepare_mesh(ctx, scene, object_index, &m)) != RT_OK) return st;
    const FlatScene &f = scene->flat;
    rt_rebuild_args a;
    std::memset(&a, 0, sizeof a);
    a.pts = d_triangles;
    a.n = n;
    a.local_level = m->plan.local_level;
    a.root_seg = m->plan.root_seg;
    a.num_nodes = (int32_t)m->plan.slots.size();
    a.segs = m->d_segs.p;
    a.slots = m->d_slots.p;
    if ((st = grow_scratch(ctx, ctx->d_update_boxes, (size_t)RT_REBUILD_SEGS * RT_REBUILD_BOX_FLOATS, "allocating the update's boxes")) != RT_OK) return st;
    a.boxes = ctx->d_update_boxes.p;
    if (a.local_level > 0) {             /* levels above the workgroup-local ones: the whole mesh's words, padded to the sort's power of two, and two lists */
        a.pad_n = 1;
        while (a.pad_n < n) a.pad_n <<= 1;
        if ((st = grow_scratch(ctx, ctx->d_update_words, (size_t)a.pad_n, "allocating the update's sort words")) != RT_OK) return st;
        if ((st = grow_scratch(ctx, ctx->d_update_perm, 2 * (size_t)n, "allocating the update's triangle lists")) != RT_OK) return st;
        a.words = ctx->d_update_words.p;
        a.perm_a = ctx->d_update_perm.p;
        a.perm_b = ctx->d_update_perm.p + n;
    }
    a.blob = scene->d_blob.p;
    a.objects = scene->d_objects.p;
    a.tri_uv = scene->d_tri_uv.p;
    a.uv0 = m->d_uv0.p;
    a.perm = scene->d_perm.p + m->tri_base;
    a.off_nodes = f.off_nodes; a.off_tris = f.off_tris; a.off_objlds = f.off_objlds; a.off_meshes = f.off_meshes; a.off_objtab = f.off_objtab;
    a.tri_base = m->tri_base;
    a.node_base = m->node_base;
    a.mesh_index = m->mesh_index;
    a.object_index = object_index;
    hipStream_t stream = (hipStream_t)hip_stream;
    st = launch_bracket(ctx, stream, [&]() -> rt_status {
        RT_HIP(ctx, rt_launch_rebuild(&a, stream), "launching the rebuild kernels");
        return RT_OK;
    });
    if (st != RT_OK) return st;
    scene->wn_stale = true;              /* the fast winding numbers' moments are refitted ahead of the next fast query (rt_winding_capi.cpp) */
    scene->uid = next_scene_uid();       /* the view cached for the old geometry, its tile order and costs, is not found again */
    return RT_OK;
}

extern "C" rt_status rt_scene_update_mesh(rt_ctx *ctx, rt_scene *scene, int32_t object_index, const float *triangles, int32_t n)
{
    rt_status st = check_update(ctx, scene, object_index, triangles, n);
    if (st != RT_OK) return st;
    for (size_t i = 0; i < (size_t)n * 9; i++)
        if (!(std::fabs(triangles[i]) <= RT_REBUILD_MAX_COORD)) return set_err(ctx, RT_ERR_INVALID, "a vertex is not finite, or larger than 2^28");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the vertices go into the context's buffer once no earlier update reads it any more */
    if (ctx->launched) RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for the previous launch");
    RT_HIP(ctx, ctx->d_update_pts.grow((size_t)n * 9), "allocating the update's vertices");
    RT_HIP(ctx, hipMemcpy(ctx->d_update_pts.p, triangles, (size_t)n * 36, hipMemcpyHostToDevice), "copying the vertices to the device");
    if ((st = rt_scene_update_mesh_device(ctx, scene, object_index, ctx->d_update_pts.p, n, nullptr)) != RT_OK) return st;
    RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "rebuild kernels");
    return RT_OK;
}

extern "C" rt_status rt_debug_scene_read(rt_ctx *ctx, rt_scene *scene, rt_flat_view *out)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!out) return set_err(ctx, RT_ERR_INVALID, "null argument");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for the device");
    const FlatScene &f = scene->flat;
    FlatScene &r = scene->debug_read;
    r.blob.resize(f.blob.size());
    r.objects.resize(f.objects.size());
    r.tri_uv.resize(f.tri_uv.size());
    if (!r.blob.empty()) RT_HIP(ctx, hipMemcpy(r.blob.data(), scene->d_blob.p, r.blob.size() * sizeof(rt_f4), hipMemcpyDeviceToHost), "reading the scene");
    if (!r.objects.empty()) RT_HIP(ctx, hipMemcpy(r.objects.data(), scene->d_objects.p, r.objects.size() * sizeof(rt_object), hipMemcpyDeviceToHost), "reading the scene");
    if (!r.tri_uv.empty()) RT_HIP(ctx, hipMemcpy(r.tri_uv.data(), scene->d_tri_uv.p, r.tri_uv.size() * 4, hipMemcpyDeviceToHost), "reading the scene");
    /* the flip bytes as a winding-number query finds them: the commit-order bytes through the device's list of who sits where */
    r.tri_flip = f.tri_flip;
    if (scene->d_perm.p && !f.tri_order.empty()) {
        std::vector<int32_t> perm(f.tri_order.size());
        RT_HIP(ctx, hipMemcpy(perm.data(), scene->d_perm.p, perm.size() * 4, hipMemcpyDeviceToHost), "reading the scene");
        for (size_t oi = 0; oi < f.objects.size(); oi++) {
            if (f.objects[oi].type != RT_OBJ_MESH) continue;
            const size_t base = (size_t)f.objects[oi].prim_start, n = (size_t)mesh_count(f, oi);
            for (size_t k = 0; k < n; k++) {
                const size_t from = (size_t)perm[base + k];
                r.tri_flip[base + k] = from < n ? f.tri_flip_commit[base + from] : 0xFF;    /* (0xFF: a list entry outside its mesh) */
            }
        }
    }
    out->tri_flip = r.tri_flip.empty() ? nullptr : r.tri_flip.data();
    out->blob = reinterpret_cast<const float *>(r.blob.data());
    out->blob_f4 = (int32_t)r.blob.size();
    out->off_nodes = f.off_nodes;
    out->off_tris = f.off_tris;
    out->off_objlds = f.off_objlds;
    out->off_meshes = f.off_meshes;
    out->num_meshes = f.num_meshes;
    out->stack_entries = f.stack_entries;
    out->objects = r.objects.data();
    out->num_objects = (int32_t)r.objects.size();
    out->object_stride = (int32_t)sizeof(rt_object);
    out->tri_uv = r.tri_uv.empty() ? nullptr : r.tri_uv.data();
    out->num_triangles = f.num_tris;
    out->num_nodes = f.num_nodes;
    out->has_mesh = f.has_mesh ? 1 : 0;
    out->traits = (int32_t)f.traits;
    out->kernel_variant = scene->kernel.shape.variant;      /* (what the committed scene runs, as rt_scene_get_info reports it) */
    return RT_OK;
}
