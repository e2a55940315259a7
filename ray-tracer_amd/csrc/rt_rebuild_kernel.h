/*
 * rt_rebuild_kernel.h — the kernels that rebuild one mesh's BVH on the device (rt_scene_update_mesh_device) and their launcher (declared in
 * rt_launch.h).  The arithmetic is rt_rebuild.h's, the same text the host tests run.
 *
 * Shape.  A level of the tree is "per segment: box in list order, reference point, keys, sort".  Levels whose segments fit a workgroup's LDS
 * (RT_REBUILD_LDS_TRIS) are all done by rt_rb_local_kernel, one workgroup per segment of the first such level, without leaving the CU: a mesh
 * of up to 2,048 triangles is one workgroup and one launch.  The levels above run over global memory, per level: rt_rb_level_kernel (one
 * workgroup per segment: its box, then its words), a bitonic sort of the whole mesh's words - the segment index is their top field, so one sort
 * serves every segment of the level -, and rt_rb_apply_kernel (the new list).  rt_rb_finish_kernel writes the boxes into the nodes and the
 * root box into its places.
 *
 * Why a bitonic network and not a radix sort: the words are unique, so any correct sort gives the reference's order; the network needs no
 * histogram, no scan and no look-back between workgroups - no kernel here waits for another workgroup, spins or is launched cooperatively -
 * and its LDS form is what the local path needs anyway.  Its cost is launches: strides of 2,048 words and more are one launch each, the rest
 * of a size is one launch over LDS tiles (50,880 triangles: 21 launches per global level, five such levels).
 * Boxes are ordered reductions (rt_rb_box_join): a thread folds a contiguous piece of the list, pieces are joined in list order.
 * Memory safety does not depend on the vertices: lists are only ever permuted inside a segment, and segments come from the plan.
 */
#ifndef RT_REBUILD_KERNEL_H
#define RT_REBUILD_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_rebuild.h"

#define RT_RB_TILE RT_REBUILD_LDS_TRIS      /* words of one LDS tile of the sort */
#define RT_RB_PAD_WORD 0xFFFFFFFFFFFFFFFFull /* sorts behind every word of a triangle (their segment field is below 2^12 - 1) */

/* The stages of a bitonic sort that stay inside a tile of `tile_n` words in LDS (a power of two, at most RT_RB_TILE), whose first word is word
 * `base` of the whole array: for every size k = k_first, 2 k_first, .., k_last the strides min(k, tile_n) / 2 .. 1.  Ascending overall.  All
 * threads of the workgroup call it; it ends behind a barrier. */
__device__ __forceinline__ void rt_rb_bitonic_lds(unsigned long long *w, int tile_n, unsigned base, unsigned k_first, unsigned k_last)
{
    for (unsigned k = k_first; k <= k_last && k != 0; k <<= 1) {
        for (unsigned j = (k >> 1) < (unsigned)(tile_n >> 1) ? (k >> 1) : (unsigned)(tile_n >> 1); j > 0; j >>= 1) {
            for (unsigned p = threadIdx.x; p < (unsigned)(tile_n >> 1); p += blockDim.x) {
                const unsigned i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
                const unsigned long long a = w[i], b = w[q];
                const bool ascending = ((base + i) & k) == 0;
                if ((a > b) == ascending) { w[i] = b; w[q] = a; }
            }
            __syncthreads();
        }
    }
}

/* the partial boxes of a workgroup's threads, one array per component (no bank conflicts), and their ordered fold */
struct rt_rb_partials {
    float lo[3][RT_REBUILD_THREADS], hi[3][RT_REBUILD_THREADS];
    int32_t valid[RT_REBUILD_THREADS];
};
__device__ __forceinline__ void rt_rb_partial_put(rt_rb_partials *s, int t, const rt_rb_box &b)
{
    for (int k = 0; k < 3; k++) { s->lo[k][t] = b.lo[k]; s->hi[k][t] = b.hi[k]; }
    s->valid[t] = b.valid;
}
__device__ __forceinline__ rt_rb_box rt_rb_partial_get(const rt_rb_partials *s, int t)
{
    rt_rb_box b;
    for (int k = 0; k < 3; k++) { b.lo[k] = s->lo[k][t]; b.hi[k] = s->hi[k][t]; }
    b.valid = s->valid[t];
    return b;
}
/* Threads come in groups of `group` consecutive ones (a power of two), thread r of a group holding the box of the r-th piece of the group's list:
 * afterwards the group's first thread's entry is the box of the whole list, joined in list order.  Ends behind a barrier. */
__device__ __forceinline__ void rt_rb_partial_fold(rt_rb_partials *s, int group)
{
    const int t = (int)threadIdx.x, r = t & (group - 1);
    __syncthreads();
    for (int step = 1; step < group; step <<= 1) {
        if ((r & (2 * step - 1)) == 0) rt_rb_partial_put(s, t, rt_rb_box_join(rt_rb_partial_get(s, t), rt_rb_partial_get(s, t + step)));
        __syncthreads();
    }
}
__device__ __forceinline__ void rt_rb_store_box(float *boxes, int heap, const rt_rb_box &b)
{
    float *o = boxes + (size_t)heap * RT_REBUILD_BOX_FLOATS;
    for (int k = 0; k < 3; k++) { o[k] = b.lo[k]; o[3 + k] = b.hi[k]; }
}

/* ---- a global level: per segment, its box and then its triangles' words ------------------------------------------------------------- */
/* grid: the 2^level segments; list: position -> commit index (NULL: the identity, level 0) */
__global__ void __launch_bounds__(RT_REBUILD_THREADS) rt_rb_level_kernel(rt_rebuild_args a, int level, const int32_t *list)
{
    __shared__ rt_rb_partials part;
    const int t = (int)threadIdx.x;
    const rt_rb_seg seg = a.segs[rt_rb_heap(level, (int)blockIdx.x)];
    /* the words behind the last triangle, once per level */
    if (blockIdx.x == 0)
        for (int i = a.n + t; i < a.pad_n; i += RT_REBUILD_THREADS) a.words[i] = RT_RB_PAD_WORD;
    if (seg.count <= 0) return;          /* (the whole workgroup) */
    const int piece = (seg.count + RT_REBUILD_THREADS - 1) / RT_REBUILD_THREADS;
    const int first = t * piece < seg.count ? t * piece : seg.count, last = first + piece < seg.count ? first + piece : seg.count;
    rt_rb_box b;
    b.valid = 0;
    for (int j = first; j < last; j++) {
        const int tri = list ? list[seg.start + j] : seg.start + j;
        const float *p = a.pts + (size_t)tri * 9;
        for (int v = 0; v < 3; v++) { const float q[3] = {p[3 * v], p[3 * v + 1], p[3 * v + 2]}; rt_rb_box_add(&b, q); }
    }
    rt_rb_partial_put(&part, t, b);
    rt_rb_partial_fold(&part, RT_REBUILD_THREADS);
    const rt_rb_box box = rt_rb_partial_get(&part, 0);
    if (t == 0) rt_rb_store_box(a.boxes, rt_rb_heap(level, (int)blockIdx.x), box);
    float ref[3];
    rt_rb_ref_point(box, ref);
    for (int j = t; j < seg.count; j += RT_REBUILD_THREADS) {
        const int tri = list ? list[seg.start + j] : seg.start + j;
        const float *p = a.pts + (size_t)tri * 9;
        const float p0[3] = {p[0], p[1], p[2]};
        a.words[seg.start + j] = rt_rb_word(blockIdx.x, rt_rb_key(p0, ref), (uint32_t)j);
    }
}

/* one tile of the global sort in LDS: sizes k_first .. k_last (see rt_rb_bitonic_lds).  grid: pad_n / RT_RB_TILE */
__global__ void __launch_bounds__(RT_REBUILD_THREADS) rt_rb_sort_tile_kernel(unsigned long long *words, unsigned k_first, unsigned k_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rt_rb_lds[];
    unsigned long long *w = (unsigned long long *)rt_rb_lds;
    const unsigned base = blockIdx.x * RT_RB_TILE;
    for (int i = (int)threadIdx.x; i < RT_RB_TILE; i += RT_REBUILD_THREADS) w[i] = words[base + i];
    __syncthreads();
    rt_rb_bitonic_lds(w, RT_RB_TILE, base, k_first, k_last);
    for (int i = (int)threadIdx.x; i < RT_RB_TILE; i += RT_REBUILD_THREADS) words[base + i] = w[i];
}

/* one stage of the global sort whose stride j does not fit a tile: a thread per pair.  grid: pad_n / 2 / 256 */
__global__ void __launch_bounds__(256) rt_rb_sort_step_kernel(unsigned long long *words, unsigned k, unsigned j)
{
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    const unsigned i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
    const unsigned long long x = words[i], y = words[q];
    if ((x > y) == ((i & k) == 0)) { words[i] = y; words[q] = x; }
}

/* the level's sorted words -> the next level's list: the triangle now at position i was at `pos` of its segment.  grid: ceil(n / 256) */
__global__ void __launch_bounds__(256) rt_rb_apply_kernel(rt_rebuild_args a, int level, const int32_t *list, int32_t *next)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.n) return;
    const unsigned long long w = a.words[i];
    unsigned s = rt_rb_word_segment(w);
    if (s >= (1u << level)) s = (1u << level) - 1u;       /* (cannot happen: the words are a permutation of what rt_rb_level_kernel wrote) */
    const rt_rb_seg seg = a.segs[rt_rb_heap(level, (int)s)];
    int src = seg.start + (int)rt_rb_word_pos(w);
    if (src >= a.n) src = a.n - 1;
    next[i] = list ? list[src] : src;
}

/* ---- the workgroup-local levels ------------------------------------------------------------------------------------------------------ */
struct rt_rb_local_lds {
    float pts[RT_REBUILD_LDS_TRIS * 9];                  /* by slot: the order the segment's triangles were loaded in */
    unsigned long long words[RT_REBUILD_LDS_TRIS];
    int32_t slot_a[RT_REBUILD_LDS_TRIS], slot_b[RT_REBUILD_LDS_TRIS];   /* list position -> slot, this level's and the next's */
    int32_t commit[RT_REBUILD_LDS_TRIS];                 /* slot -> commit index */
    rt_rb_partials part;
};

/* grid: the 2^local_level segments of that level; list: as above.  From its segment's list a workgroup runs every remaining level: at relative
 * depth d its subtree has 2^d segments, each folded, keyed and written by a group of 1024 >> d consecutive threads, and sorted together.  Then it
 * writes the triangle records, the texture coordinates and the permutation of its range. */
__global__ void __launch_bounds__(RT_REBUILD_THREADS) rt_rb_local_kernel(rt_rebuild_args a, const int32_t *list)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rt_rb_lds[];
    rt_rb_local_lds *s = (rt_rb_local_lds *)rt_rb_lds;
    const int t = (int)threadIdx.x;
    const rt_rb_seg top = a.segs[rt_rb_heap(a.local_level, (int)blockIdx.x)];
    const int c = top.count;
    if (c <= 0 || c > RT_REBUILD_LDS_TRIS) return;       /* (the whole workgroup; the second cannot happen: the plan chose the level) */
    int sort_n = 2;
    while (sort_n < c) sort_n <<= 1;
    for (int i = t; i < c; i += RT_REBUILD_THREADS) {
        s->commit[i] = list ? list[top.start + i] : top.start + i;
        s->slot_a[i] = i;
    }
    __syncthreads();
    for (int e = t; e < 9 * c; e += RT_REBUILD_THREADS) s->pts[e] = a.pts[(size_t)s->commit[e / 9] * 9 + (e % 9)];
    int32_t *cur = s->slot_a, *nxt = s->slot_b;
    for (int level = a.local_level; level <= RT_BVH_DEPTH; level++) {
        const int d = level - a.local_level, group = RT_REBUILD_THREADS >> d;
        const int g = t / group, r = t & (group - 1);
        const int first_seg = (int)blockIdx.x << d;
        const rt_rb_seg seg = a.segs[rt_rb_heap(level, first_seg + g)];
        const int at = seg.start - top.start;            /* the segment's first position in the workgroup's list */
        const int piece = (seg.count + group - 1) / group;
        const int first = r * piece < seg.count ? r * piece : seg.count, last = first + piece < seg.count ? first + piece : seg.count;
        __syncthreads();                                 /* the list of this level, and (first level) the points, are in LDS */
        rt_rb_box b;
        b.valid = 0;
        for (int j = first; j < last; j++) {
            const float *p = s->pts + 9 * cur[at + j];
            for (int v = 0; v < 3; v++) { const float q[3] = {p[3 * v], p[3 * v + 1], p[3 * v + 2]}; rt_rb_box_add(&b, q); }
        }
        rt_rb_partial_put(&s->part, t, b);
        rt_rb_partial_fold(&s->part, group);
        const rt_rb_box box = rt_rb_partial_get(&s->part, t - r);
        if (r == 0 && seg.count > 0) rt_rb_store_box(a.boxes, rt_rb_heap(level, first_seg + g), box);
        if (level == RT_BVH_DEPTH) break;
        float ref[3];
        rt_rb_ref_point(box, ref);
        for (int j = r; j < seg.count; j += group) {
            const float *p = s->pts + 9 * cur[at + j];
            const float p0[3] = {p[0], p[1], p[2]};
            s->words[at + j] = rt_rb_word((uint32_t)g, rt_rb_key(p0, ref), (uint32_t)j);
        }
        for (int i = c + t; i < sort_n; i += RT_REBUILD_THREADS) s->words[i] = RT_RB_PAD_WORD;
        __syncthreads();
        rt_rb_bitonic_lds(s->words, sort_n, 0u, 2u, (unsigned)sort_n);
        for (int i = t; i < c; i += RT_REBUILD_THREADS) {
            const unsigned long long w = s->words[i];
            unsigned from = rt_rb_word_segment(w);
            if (from >= (1u << d)) from = (1u << d) - 1u; /* (cannot happen, as in rt_rb_apply_kernel) */
            int src = a.segs[rt_rb_heap(level, first_seg + (int)from)].start - top.start + (int)rt_rb_word_pos(w);
            if (src < 0 || src >= c) src = 0;
            nxt[i] = cur[src];
        }
        int32_t *swap = cur; cur = nxt; nxt = swap;      /* (the loop's first barrier orders the next level behind these writes) */
    }
    /* the range's triangle records, texture coordinates and permutation */
    for (int i = t; i < c; i += RT_REBUILD_THREADS) {
        const int slot = cur[i], tri = a.tri_base + top.start + i, commit = s->commit[slot];
        rt_f4 q[3];
        rt_rb_tri(s->pts + 9 * slot, q);
        rt_f4 *out = a.blob + a.off_tris + (size_t)tri * 3;
        out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
        a.perm[top.start + i] = commit;
        if (a.tri_uv)
            for (int k = 0; k < 6; k++) a.tri_uv[(size_t)tri * 6 + k] = a.uv0[(size_t)commit * 6 + k];
    }
}

/* ---- the boxes into their places ------------------------------------------------------------------------------------------------------ */
__device__ __forceinline__ void rt_rb_load_box(const float *boxes, int heap, float v[6])
{
    for (int k = 0; k < 6; k++) v[k] = heap >= 0 ? boxes[(size_t)heap * RT_REBUILD_BOX_FLOATS + k] : 0.0f;
}

/* grid: ceil((num_nodes + 1) / 256): a thread per stored node (q[0..2]; q[3], the references, is topology and stays), and one for the root box:
 * the mesh table's entry, the object's v[0..5] in the object table and in the objtab section, rec[2] of its shading record */
__global__ void __launch_bounds__(256) rt_rb_finish_kernel(rt_rebuild_args a)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < a.num_nodes) {
        const rt_rb_slot slot = a.slots[i];
        float l[6], r[6];
        rt_rb_load_box(a.boxes, slot.left, l);
        rt_rb_load_box(a.boxes, slot.right, r);
        rt_f4 *q = a.blob + a.off_nodes + (size_t)(a.node_base + i) * 4;
        q[0] = rt_f4{l[0], l[1], l[2], l[3]};
        q[1] = rt_f4{l[4], l[5], r[0], r[1]};
        q[2] = rt_f4{r[2], r[3], r[4], r[5]};
    } else if (i == a.num_nodes) {
        float v[6];
        rt_rb_load_box(a.boxes, a.root_seg, v);
        rt_f4 *mt = a.blob + a.off_meshes + (size_t)a.mesh_index * 2;
        mt[0] = rt_f4{v[0], v[1], v[2], v[3]};
        mt[1].x = v[4];
        mt[1].y = v[5];
        rt_object *in_blob = (rt_object *)(a.blob + a.off_objtab + (size_t)a.object_index * 3);
        for (int k = 0; k < 6; k++) { in_blob->v[k] = v[k]; a.objects[a.object_index].v[k] = v[k]; }
        a.blob[a.off_objlds + (size_t)a.object_index * RT_OBJLDS_F4 + 2] = rt_f4{v[0], v[1], v[2], v[3]};
    }
}

extern "C" hipError_t rt_launch_rebuild(const rt_rebuild_args *args, hipStream_t stream)
{
    const rt_rebuild_args &a = *args;
    if (a.n <= 0 || a.local_level < 0 || a.local_level > RT_BVH_DEPTH) return hipErrorInvalidValue;
    const int32_t *list = nullptr;
    int32_t *next = a.perm_a;
    if (a.local_level > 0 && (a.pad_n < a.n || a.pad_n < 2 * RT_RB_TILE || (a.pad_n & (a.pad_n - 1)))) return hipErrorInvalidValue;
    const size_t tile_bytes = (size_t)RT_RB_TILE * sizeof(unsigned long long);
    for (int level = 0; level < a.local_level; level++) {
        hipLaunchKernelGGL(rt_rb_level_kernel, dim3(1u << level), dim3(RT_REBUILD_THREADS), 0, stream, a, level, list);
        const unsigned pad = (unsigned)a.pad_n, tiles = pad / RT_RB_TILE;
        hipLaunchKernelGGL(rt_rb_sort_tile_kernel, dim3(tiles), dim3(RT_REBUILD_THREADS), tile_bytes, stream, a.words, 2u, (unsigned)RT_RB_TILE);
        for (unsigned k = 2u * RT_RB_TILE; k <= pad; k <<= 1) {
            for (unsigned j = k >> 1; j >= (unsigned)RT_RB_TILE; j >>= 1)
                hipLaunchKernelGGL(rt_rb_sort_step_kernel, dim3(pad / 2 / 256), dim3(256), 0, stream, a.words, k, j);
            hipLaunchKernelGGL(rt_rb_sort_tile_kernel, dim3(tiles), dim3(RT_REBUILD_THREADS), tile_bytes, stream, a.words, k, k);
        }
        hipLaunchKernelGGL(rt_rb_apply_kernel, dim3(((unsigned)a.n + 255u) / 256u), dim3(256), 0, stream, a, level, list, next);
        list = next;
        next = next == a.perm_a ? a.perm_b : a.perm_a;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipFuncSetAttribute((const void *)rt_rb_local_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(rt_rb_local_lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rt_rb_local_kernel, dim3(1u << a.local_level), dim3(RT_REBUILD_THREADS), sizeof(rt_rb_local_lds), stream, a, list);
    hipLaunchKernelGGL(rt_rb_finish_kernel, dim3(((unsigned)a.num_nodes + 1u + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

#endif
