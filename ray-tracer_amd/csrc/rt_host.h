/*
 * rt_host.h — host-side scene model shared by rt_host.cpp (builders, loaders, flattening) and
 * rt_capi.cpp (upload + launch).  Internal to libraytracer_amd.so.
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include <string>
#include <vector>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"

struct HostTri {
    float p0[3], s1[3], s2[3], n[3];
    float uv[6];
};

struct HostObject {
    int type = 0;
    rt_material mat{};
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};   /* see rt_object */
    std::vector<HostTri> tris;           /* top-level shapes: 1 / 2 / 12; meshes: leaf order */
    std::vector<rt_node> nodes;          /* meshes: child refs relative to this object */
    std::vector<int> order;              /* meshes: order[k] = the index, in the order the triangles were given, of the one at leaf position k */
    std::vector<uint8_t> flip;           /* meshes, in the order the triangles were given: 1 where the record's orientation is opposite to its face's (make_quad's second triangle) */
    std::vector<float> texels;           /* IMAGE texture: a copy of the caller's rgb data */
    uint32_t root_ref = RT_REF_EMPTY_LEAF;
    int stack_need = 0;
};

struct FlatScene;

struct rt_scene_builder {
    std::vector<HostObject> objs;
    std::string err;
    FlatScene *debug_flat = nullptr;     /* owned; rt_debug_flatten */
    void *debug_winding = nullptr;       /* owned, with how to free it; rt_debug_winding_tree (rt_winding_capi.cpp) */
    void (*debug_winding_free)(void *) = nullptr;
    ~rt_scene_builder();
};

struct rt_obj {
    std::vector<float> vx, vy, vz;               /* vertex_mat rows (reference src/obj_read.cu:49) */
    std::vector<std::vector<int>> faces;         /* 0-based vertex indices per face */
};

/* flattened scene, ready to upload */
struct FlatScene {
    std::vector<rt_f4> blob;
    int off_nodes = 0, off_tris = 0, off_objlds = 0, off_meshes = 0, off_objtab = 0;
    int num_meshes = 0;
    int stack_entries = 1;                       /* per-lane traversal stack depth this scene needs */
    std::vector<rt_object> objects;
    std::vector<float> tri_uv;                   /* empty unless some material needs UVs */
    std::vector<int32_t> tri_order;              /* per triangle of a mesh: its index in the mesh's commit order (HostObject::order); others: 0 */
    std::vector<uint8_t> tri_flip;               /* per triangle record: HostObject::flip of the one at that position (a mesh's), others: 0 */
    std::vector<uint8_t> tri_flip_commit;        /* the same bytes with every mesh's range in its commit order: [prim_start + commit index] (what the device is handed, rt_winding_capi.cpp) */
    std::vector<float> tex_data;                 /* IMAGE texels of all objects, back to back */
    int num_tris = 0, num_nodes = 0;
    bool has_mesh = false;
    uint32_t traits = 0;                         /* RT_TRAIT_* (rt_device_scene.h): what of the scene lets the render kernel leave control flow out */
    int mesh_obj = -1;                           /* the first mesh's place in the object list (with RT_TRAIT_ONE_MESH: the only one's), or -1 */
};

/* the traits of a flattened object list: from the object types and the materials alone, so rt_scene_update_mesh never changes them */
uint32_t rt_scene_traits(const rt_scene_builder &b);

/* returns "" or an error message */
std::string rt_flatten(const rt_scene_builder &b, FlatScene &out);

#endif
