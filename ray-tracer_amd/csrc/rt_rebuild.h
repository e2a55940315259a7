/*
 * rt_rebuild.h — rebuilding one committed mesh's BVH from new vertices (rt_scene_update_mesh[_device], include/rt_amd.h): what the kernels
 * (rt_rebuild_kernel.h), the entry points (rt_update_capi.cpp) and the host tests (tests/sanitize/update_host_check.cpp) share.  Host code;
 * self-contained.
 *
 * The reference's builder (BvhBuilder::build, rt_host.cpp) sends the first m / 2 + 1 triangles of a node's sorted list left and the rest
 * right, for RT_BVH_DEPTH levels, emits leaves left to right and nodes in post-order.  So everything about a mesh's tree but the order of
 * its triangles and the boxes follows from its triangle count: the PLAN below.  A rebuild is then, level by level and for every segment of
 * the level, "box in list order, reference point, keys, sort", and at the end boxes written into slots the plan names.
 *
 *  - the segments: level L (0 the root .. RT_BVH_DEPTH the leaves) has 2^L of them, entry i at heap index 2^L - 1 + i, its children
 *    2 i and 2 i + 1 one level down; (start, count) in the mesh's leaf-order range, count 0 for a subtree that does not exist;
 *  - the arithmetic, as the one text both sides compile (binary32, nothing fused: the library and the tests build with contraction off):
 *    the triangle record, the ordered min / max, the reference point, the key, the composite sort word.
 */
#ifndef RT_REBUILD_H
#define RT_REBUILD_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/rt_amd.h"     /* RT_REBUILD_LDS_TRIS */
#include "rt_device_scene.h"

#if defined(__HIPCC__)
#define RT_RB_HD __host__ __device__ inline
#else
#define RT_RB_HD inline
#endif

/* The largest segment the workgroup-local path takes: one workgroup keeps, per triangle, its nine coordinates (36 B), its sort word (8 B), two
 * generations of its list position (8 B) and its commit index (4 B) in LDS, and 28 KB of partial boxes beside them: 56 B x 2,048 + 28 KB = 140 KB
 * of the CU's 160 KB.  The bitonic network wants a power of two, and 4,096 triangles would need 252 KB.  (The value is include/rt_amd.h's.) */
static_assert(RT_REBUILD_LDS_TRIS == 2048, "the LDS budget above is worked out for 2,048 triangles");
#define RT_REBUILD_THREADS 1024
#define RT_REBUILD_LEVELS (RT_BVH_DEPTH + 1)
#define RT_REBUILD_SEGS ((1 << RT_REBUILD_LEVELS) - 1)
#define RT_REBUILD_BOX_FLOATS 8                     /* a segment's box in the scratch: lo.xyz, hi.xyz, two unused */
#define RT_REBUILD_MAX_COORD 268435456.0f           /* 2^28: the host form refuses larger coordinates (3 (8 m^2)^2, the normal's squared length, stays finite) */

typedef struct { int32_t start, count; } rt_rb_seg;
typedef struct { int32_t left, right; } rt_rb_slot;  /* a stored node: the heap indices of the segments whose boxes are its q[0..2]; -1: the (0,0,0) box */
typedef struct { float lo[3], hi[3]; int32_t valid; } rt_rb_box;   /* valid == 0: of no point yet */

RT_RB_HD int rt_rb_heap(int level, int i) { return (1 << level) - 1 + i; }

/* ---- the arithmetic ------------------------------------------------------------------------------------------------------------ */
/* std::min(lo, p) and std::max(hi, p) of BvhBuilder::bounds as the comparisons they are: the earlier operand stays on equality, so with +0 and
 * -0 among the coordinates a box keeps the zero met first.  (fminf / v_min_f32 do not promise that.)  As a reduction the operation is
 * associative as long as the left operand is the earlier part of the list. */
RT_RB_HD float rt_rb_min(float earlier, float later) { return (later < earlier) ? later : earlier; }
RT_RB_HD float rt_rb_max(float earlier, float later) { return (earlier < later) ? later : earlier; }

RT_RB_HD void rt_rb_box_add(rt_rb_box *b, const float p[3])
{
    if (!b->valid) {
        for (int k = 0; k < 3; k++) b->lo[k] = b->hi[k] = p[k];
        b->valid = 1;
        return;
    }
    for (int k = 0; k < 3; k++) { b->lo[k] = rt_rb_min(b->lo[k], p[k]); b->hi[k] = rt_rb_max(b->hi[k], p[k]); }
}

/* the box of a list = join(box of its earlier part, box of its later part) */
RT_RB_HD rt_rb_box rt_rb_box_join(const rt_rb_box &earlier, const rt_rb_box &later)
{
    if (!earlier.valid) return later;
    if (!later.valid) return earlier;
    rt_rb_box b;
    b.valid = 1;
    for (int k = 0; k < 3; k++) { b.lo[k] = rt_rb_min(earlier.lo[k], later.lo[k]); b.hi[k] = rt_rb_max(earlier.hi[k], later.hi[k]); }
    return b;
}

/* BvhBuilder::ref_point */
RT_RB_HD void rt_rb_ref_point(const rt_rb_box &b, float ref[3])
{
    const float width = b.hi[0] - b.lo[0], height = b.hi[1] - b.lo[1], depth = b.hi[2] - b.lo[2];
    if (width >= height && width >= depth) { ref[0] = b.lo[0] + width / 2; ref[1] = b.lo[1]; ref[2] = b.lo[2] + depth / 2; return; }
    if (height >= width && height >= depth) { ref[0] = b.lo[0]; ref[1] = b.lo[1] + height / 2; ref[2] = b.lo[2] + depth / 2; return; }
    ref[0] = b.lo[0] + width / 2; ref[1] = b.lo[1] + height / 2; ref[2] = b.lo[2];
}

/* magnitude(p0 - ref): sqrt((dx dx + dy dy) + dz dz).  sqrtf and the division below are the compilers' correctly rounded ones on both sides. */
RT_RB_HD float rt_rb_key(const float p0[3], const float ref[3])
{
    const float dx = p0[0] - ref[0], dy = p0[1] - ref[1], dz = p0[2] - ref[2];
    const float m = dx * dx + dy * dy + dz * dz;
    return sqrtf(m);
}

/* Ascending key, equal keys in DESCENDING position in the parent's list (the reference's merge sort emits the right run first), as one total
 * order on 64-bit words: keys are not negative, so their bit patterns order like the floats; `segment` (the segment's index among those sorted
 * together, < 2^12) keeps every segment's words in its own range; pos < 2^20 (RT_REF_START_MASK).  The words of one pass are all different. */
RT_RB_HD uint64_t rt_rb_word(uint32_t segment, float key, uint32_t pos)
{
    uint32_t bits;
    memcpy(&bits, &key, 4);
    return ((uint64_t)segment << 52) | ((uint64_t)bits << 20) | (uint64_t)(0xFFFFFu - pos);
}
RT_RB_HD uint32_t rt_rb_word_segment(uint64_t w) { return (uint32_t)(w >> 52); }
RT_RB_HD uint32_t rt_rb_word_pos(uint64_t w) { return 0xFFFFFu - (uint32_t)(w & 0xFFFFFu); }

/* make_tri (Triangle::precompute): p0, s1 = b - a, s2 = c - a, normalised(cross(s1, s2)) with one reciprocal of the magnitude */
RT_RB_HD void rt_rb_tri(const float p[9], rt_f4 q[3])
{
    const float s1x = p[3] - p[0], s1y = p[4] - p[1], s1z = p[5] - p[2];
    const float s2x = p[6] - p[0], s2y = p[7] - p[1], s2z = p[8] - p[2];
    const float cx = s1y * s2z - s1z * s2y, cy = s1z * s2x - s1x * s2z, cz = s1x * s2y - s1y * s2x;
    const float m = cx * cx + cy * cy + cz * cz;
    const float inv = 1 / sqrtf(m);
    q[0].x = p[0]; q[0].y = p[1]; q[0].z = p[2]; q[0].w = s1x;
    q[1].x = s1y; q[1].y = s1z; q[1].z = s2x; q[1].w = s2y;
    q[2].x = s2z; q[2].y = cx * inv; q[2].z = cy * inv; q[2].w = cz * inv;
}

/* ---- the plan ------------------------------------------------------------------------------------------------------------------ */
struct rt_rb_plan {
    int32_t n = -1;
    std::vector<rt_rb_seg> segs;         /* RT_REBUILD_SEGS, heap order */
    std::vector<rt_rb_slot> slots;       /* per stored node, in the builder's (post-)order */
    std::vector<uint32_t> lref, rref;    /* per stored node: its child references, relative to the mesh (as HostObject::nodes has them) */
    int32_t root_seg = -1;               /* the segment whose box is the mesh's root box (-1: no triangle, the (0,0,0) box) */
    uint32_t root_ref = RT_REF_EMPTY_LEAF;
    int32_t stack_need = 0;
    int32_t local_level = 0;             /* the first level whose segments all hold at most RT_REBUILD_LDS_TRIS triangles */
};

namespace rt_rb_detail {
struct Sub { uint32_t ref; int32_t seg, need; };
/* the subtree over `count` triangles starting at leaf position `start`: what BvhBuilder::build returns for it, from the counts alone */
inline Sub derive(rt_rb_plan &p, int level, int i, int32_t start, int32_t count, bool *ok)
{
    p.segs[(size_t)rt_rb_heap(level, i)] = rt_rb_seg{start, count};
    if (count == 0) return Sub{RT_REF_EMPTY_LEAF, -1, 0};
    if (level == RT_BVH_DEPTH) {
        if ((uint32_t)count > RT_REF_COUNT_MAX || (uint32_t)(start + count) > RT_REF_START_MASK) *ok = false;
        return Sub{RT_REF_LEAF | ((uint32_t)count << RT_REF_COUNT_SHIFT) | (uint32_t)start, rt_rb_heap(level, i), 0};
    }
    const int32_t n_left = count / 2 + 1 < count ? count / 2 + 1 : count;       /* list positions 0 .. count / 2 */
    Sub l = derive(p, level + 1, 2 * i, start, n_left, ok);
    const Sub r = derive(p, level + 1, 2 * i + 1, start + n_left, count - n_left, ok);
    if (count == n_left) {               /* a single-child node is not stored: the edge into it stands for its child, box and all */
        l.ref |= RT_REF_CHAIN;
        return l;
    }
    p.slots.push_back(rt_rb_slot{l.seg, r.seg});
    p.lref.push_back(l.ref);
    p.rref.push_back(r.ref);
    return Sub{(uint32_t)p.slots.size() - 1u, rt_rb_heap(level, i), 1 + (l.need > r.need ? l.need : r.need)};
}
}  // namespace rt_rb_detail

/* the plan of a mesh of n triangles; false: such a mesh cannot have been committed (a leaf of more than 1,023 triangles, more than 2^20 - 1 in all) */
inline bool rt_rb_make_plan(int32_t n, rt_rb_plan &p)
{
    p = rt_rb_plan();
    if (n < 0 || (uint32_t)n > RT_REF_START_MASK) return false;
    p.n = n;
    p.segs.assign(RT_REBUILD_SEGS, rt_rb_seg{0, 0});
    bool ok = true;
    const rt_rb_detail::Sub root = rt_rb_detail::derive(p, 0, 0, 0, n, &ok);
    p.root_seg = root.seg;
    p.root_ref = root.ref;
    p.stack_need = root.need;
    p.local_level = 0;                   /* (a level's first segment is its largest) */
    while (p.local_level < RT_BVH_DEPTH && p.segs[(size_t)rt_rb_heap(p.local_level, 0)].count > RT_REBUILD_LDS_TRIS) p.local_level++;
    return ok;
}

/* ---- the argument block (the launcher is rt_launch.h's rt_launch_rebuild) -------------------------------------------------------- */
typedef struct {
    const float *pts;              /* n x 9: the mesh's new triangles in commit order */
    int32_t n;
    int32_t pad_n;                 /* the words the global passes sort: a power of two >= n (unused when local_level == 0) */
    int32_t local_level, root_seg, num_nodes;
    const rt_rb_seg *segs;         /* the plan on the device */
    const rt_rb_slot *slots;
    /* the context's scratch */
    float *boxes;                  /* RT_REBUILD_SEGS x RT_REBUILD_BOX_FLOATS */
    unsigned long long *words;     /* pad_n */
    int32_t *perm_a, *perm_b;      /* n each: the list of a global level (position -> commit index) and of the next */
    /* the scene */
    rt_f4 *blob;
    rt_object *objects;
    float *tri_uv;                 /* or NULL */
    const float *uv0;              /* with tri_uv: the mesh's texture coordinates in commit order, 6 floats per triangle */
    int32_t *perm;                 /* the mesh's range of the scene's current permutation: leaf position -> commit index */
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t tri_base, node_base;   /* the mesh's first triangle and first node in the scene */
    int32_t mesh_index, object_index;
} rt_rebuild_args;

#endif
