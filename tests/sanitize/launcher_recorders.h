// Every kernel launcher of rt_launch.h as a RECORDER, for tests/sanitize/order_host_check.cpp: where the stubs of launcher_stubs.h fail,
// these succeed and log the launch - its stream and every buffer its argument block names, with the bytes the kernel may touch and
// whether it writes them - into the program's happens-before checker (rec::launch, defined by the program).  A launcher missing here is
// a link error and one whose signature differs from rt_launch.h does not compile, as with the stubs; tests/test_launch_order.py checks
// that this file defines every launcher once.  The sizes restate what the kernels index (rt_render_kernel.h, rt_frame_kernels.h,
// rt_query_kernel.h, rt_occlusion_kernel.h, rt_ao_kernel.h, rt_multihit_kernel.h, rt_denoise_kernel.h, rt_adaptive_kernel.h,
// rt_rebuild_kernel.h, rt_cull_kernel.h, rt_nearest_kernel.h, rt_sweep_kernel.h, rt_overlap_kernel.h, rt_tritri_kernel.h, rt_winding_kernel.h); the checker also refuses a range that leaves its
// allocation.  Included by one translation unit.
#pragma once

#include <initializer_list>

#include "rt_cull.h"       // rt_cull_words
#include "rt_launch.h"
#include "rt_sky.h"        // RT_SKY_TEXEL_FLOATS

namespace rec {
struct Use {
    const void *p;            // null: not used by this launch
    size_t bytes;
    bool write;
    const char *what;
};
// one kernel launch on `stream` touching `uses`; hipSuccess
hipError_t launch(const char *kernel, hipStream_t stream, std::initializer_list<Use> uses);
// the plan kernel's per-tile outputs, made up: which tiles the adaptive loop's next pass renders
void fill_plan(float *tile_error, uint32_t *tile_active, int num_tiles);
// the bytes from `p` to the end of its allocation (0: not a known allocation): for a section whose length the argument block does not carry
size_t extent(const void *p);
}  // namespace rec

namespace rec_detail {
constexpr bool R = false, W = true;
constexpr size_t COUNTER_BYTES = 64;      // the ticket word(s) at the head of the 1 KB counter buffer

inline size_t px(int w, int h) { return (size_t)w * (size_t)h; }
inline const rt_f4 *f4(const rt_f4 *blob, int32_t off) { return blob ? blob + off : nullptr; }

// what a render launch writes through `out` (a plain frame) in the output layout of its tile spec
inline size_t out_bytes(const rt_kernel_args *a)
{
    if (!a->compact) return px(a->width, a->height) * 12;
    if (a->tile_list) return (size_t)a->num_tiles * 192 * 4;
    const int bands = (a->height + a->band_rows - 1) / a->band_rows;
    int owned = 0;
    for (int b = 0; b < bands; b++) owned += b % a->band_stride == a->band_first;
    return (size_t)owned * a->band_rows * a->width * 12;
}

inline hipError_t render_like(const char *kernel, const rt_kernel_args *a, hipStream_t stream, rec::Use x, rec::Use y, rec::Use z, bool out_is_frame)
{
    const size_t nt = (size_t)a->num_tiles, nf = (size_t)a->num_frames;
    return rec::launch(kernel, stream, {
        {a->tile_counter, COUNTER_BYTES, W, "ticket counter"},
        {a->partial, (size_t)a->partial_plane * 12 * nf, W, "per-frame planes"},
        {a->partial ? nullptr : a->out, out_is_frame ? px(a->width, a->height) * 12 : out_bytes(a), W, "out"},
        {a->prev, px(a->width, a->height) * 12, R, "prev"},
        {a->tile_list, nt * 4, R, "tile list"},
        {a->tile_order, nt * 4, R, "tile order"},
        {a->job_order, nt * nf * 4, R, "job order"},
        {a->tile_cost, nt * 4, W, "tile costs"},
        {a->tile_peak, nt * 4, W, "tile peaks"},
        {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
        {a->objects, (size_t)a->num_objects * sizeof(rt_object), R, "scene objects"},
        x, y, z});
}
}  // namespace rec_detail

extern "C" {
int rt_kernel_blocks_per_cu(rt_shape, size_t) { return 1; }
hipError_t rt_launch_render(const rt_kernel_args *a, rt_shape, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    return render_like("render", a, stream, {}, {}, {}, false);
}
hipError_t rt_launch_budget(const rt_kernel_args *a, const uint16_t *budget, uint32_t *count, rt_shape, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    return render_like("budget render", a, stream, {budget, px(a->width, a->height) * 2, R, "budget plane"}, {count, px(a->width, a->height) * 4, W, "count plane"}, {}, true);
}
hipError_t rt_launch_views(const rt_kernel_args *a, const float *cams, rt_shape, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    return render_like("views", a, stream, {cams, (size_t)a->num_frames * 48, R, "camera table"}, {}, {}, true);
}
hipError_t rt_launch_sky(const rt_kernel_args *a, const float *cams, const float *texels, int32_t face_size, rt_shape, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    return render_like("sky", a, stream, {cams, (size_t)a->num_frames * 48, R, "camera table"},
                       {texels, (size_t)6 * (size_t)face_size * (size_t)face_size * RT_SKY_TEXEL_FLOATS * 4, R, "sky texels"}, {}, true);
}
hipError_t rt_launch_blend(const float *partial, long long plane_floats, int num_frames, int, float *frame, long long n_floats, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("blend", stream, {{partial, ((size_t)(num_frames - 1) * (size_t)plane_floats + (size_t)n_floats) * 4, R, "per-frame planes"},
                                         {frame, (size_t)n_floats * 4, W, "frame"}});
}
hipError_t rt_launch_blend_tiles(const float *partial, long long plane_floats, int num_frames, int, float *frame, const uint32_t *tile_list, int n_tiles, int, int w, int h,
                                 hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("blend tiles", stream, {{partial, (size_t)num_frames * (size_t)plane_floats * 4, R, "per-frame planes"}, {frame, px(w, h) * 12, W, "frame"},
                                               {tile_list, (size_t)n_tiles * 4, R, "tile list"}});
}
hipError_t rt_launch_tiles_copy(float *compact, float *frame, const uint32_t *tile_list, int n_tiles, int, int w, int h, int to_frame, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("tiles copy", stream, {{compact, (size_t)n_tiles * 192 * 4, !to_frame, "compact image"}, {frame, px(w, h) * 12, to_frame != 0, "frame"},
                                              {tile_list, (size_t)n_tiles * 4, R, "tile list"}});
}
hipError_t rt_launch_rgba8(const float *rgb, int n_pixels, uint8_t *out, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("rgba8", stream, {{rgb, (size_t)n_pixels * 12, R, "rgb"}, {out, (size_t)n_pixels * 4, W, "rgba"}});
}
hipError_t rt_launch_query(const rt_query_args *a, rt_shape, int aov, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n, p = aov ? px(a->width, a->height) : 0;
    return rec::launch("query", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
                                         {aov ? nullptr : a->origins, n * 12, R, "origins"}, {aov ? nullptr : a->directions, n * 12, R, "directions"},
                                         {aov ? nullptr : a->hits, n * sizeof(rt_hit), W, "hits"}, {a->depth, p * 4, W, "depth"}, {a->normal, p * 12, W, "normal"},
                                         {a->albedo, p * 12, W, "albedo"}, {a->object, p * 4, W, "object"}, {a->ray, p * 12, W, "ray"}});
}
hipError_t rt_launch_occlusion(const rt_occlusion_args *a, rt_shape, int vis, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n;
    return rec::launch("occlusion", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
                                             {vis ? nullptr : a->origins, n * 12, R, "origins"}, {vis ? nullptr : a->directions, n * 12, R, "directions"},
                                             {vis ? nullptr : a->tmax, n * 4, R, "limits"}, {a->out, vis ? px(a->width, a->height) : n, W, "answers"}});
}
hipError_t rt_launch_ao(const rt_ao_args *a, rt_shape, int, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t p = px(a->width, a->height);
    return rec::launch("ambient occlusion", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
                                                     {a->count, p * 2, W, "ao counts"}, {a->ao, p * 4, W, "ao plane"}});
}
hipError_t rt_launch_multihit(const rt_multihit_args *a, rt_shape, int, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n, k = (size_t)a->k;
    const size_t tris = (size_t)(a->blob_f4 - a->off_tris) / 3;       // the triangle records are the blob's last section: one uv record per triangle
    return rec::launch("multi-hit", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
                                             {a->tri_uv, tris * 24, R, "triangle uvs"}, {a->origins, n * 12, R, "origins"}, {a->directions, n * 12, R, "directions"},
                                             {a->tmax, n * 4, R, "limits"}, {a->hits, n * k * sizeof(rt_hit), W, "multi-hit records"}, {a->counts, n * 4, W, "hit counts"}});
}
hipError_t rt_launch_multihit_uv(const rt_multihit_uv_args *a, int, hipStream_t stream)
{
    using namespace rec_detail;
    if (a->records <= 0) return hipSuccess;
    // (a record names its object: the shading records are read up to the scene's last, which is as far as the blob goes for this block)
    return rec::launch("multi-hit uv", stream, {{a->objlds, rec::extent(a->objlds), R, "scene blob"}, {a->hits, (size_t)a->records * sizeof(rt_hit), W, "multi-hit records"}});
}
hipError_t rt_launch_overlap(const rt_overlap_args *a, rt_shape, int, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n, k = (size_t)a->k;
    return rec::launch("box overlap", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
                                               {a->lo, n * 12, R, "lower corners"}, {a->hi, n * 12, R, "upper corners"},
                                               {k > 0 ? a->ids : nullptr, n * k * sizeof(rt_overlap_id), W, "overlap ids"}, {a->counts, n * 4, W, "overlap counts"},
                                               {a->any, n, W, "overlap bytes"}});
}
hipError_t rt_launch_tritri(const rt_tritri_args *a, rt_shape, int, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n, k = (size_t)a->k;
    return rec::launch("triangle overlap", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"},
                                                    {a->tris, n * 36, R, "query triangles"}, {k > 0 ? a->ids : nullptr, n * k * sizeof(rt_overlap_id), W, "overlap ids"},
                                                    {a->counts, n * 4, W, "overlap counts"}, {a->any, n, W, "overlap bytes"},
                                                    {k > 0 ? a->segments : nullptr, n * k * sizeof(rt_tri_segment), W, "overlap segments"}});
}
hipError_t rt_launch_denoise_pack(const rt_denoise_args *a, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t p = px(a->width, a->height);
    return rec::launch("denoise pack", stream, {{a->colour, p * 12, R, "colour"}, {a->normal, p * 12, R, "normal"}, {a->depth, p * 4, R, "depth"}, {a->object, p * 4, R, "object"},
                                                {a->albedo, p * 12, R, "albedo"}, {a->guide, p * 16, W, "denoise guide records"}, {a->dst, p * 16, W, "denoise colour records"}});
}
hipError_t rt_launch_denoise_level(const rt_denoise_args *a, int last, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t p = px(a->width, a->height);
    return rec::launch("denoise level", stream, {{a->guide, p * 16, R, "denoise guide records"}, {a->src, p * 16, R, "denoise colour records"},
                                                 {last ? nullptr : a->dst, p * 16, W, "denoise colour records"}, {last ? a->out : nullptr, p * 12, W, "denoised frame"},
                                                 {last ? a->albedo : nullptr, p * 12, R, "albedo"}});
}
hipError_t rt_launch_adaptive_plan(const rt_plan_args *a, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t p = px(a->width, a->height), nt = (size_t)a->num_tiles;
    const hipError_t e = rec::launch("adaptive plan", stream, {{a->a, p * 12, R, "half buffer A"}, {a->b, p * 12, R, "half buffer B"}, {a->count, p * 4, R, "count plane"},
                                                               {a->budget, p * 2, W, "budget plane"}, {a->tile_error, nt * 4, W, "tile errors"}, {a->tile_active, nt * 4, W, "active tiles"}});
    if (e == hipSuccess) rec::fill_plan(a->tile_error, a->tile_active, a->num_tiles);
    return e;
}
hipError_t rt_launch_adaptive_combine(const float *a, const float *b, const uint32_t *count, float *frame, uint32_t *count_out, long long n, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("adaptive combine", stream, {{a, (size_t)n * 12, R, "half buffer A"}, {b, (size_t)n * 12, R, "half buffer B"}, {count, (size_t)n * 4, R, "count plane"},
                                                    {frame, (size_t)n * 12, W, "frame"}, {count_out, (size_t)n * 4, W, "counts out"}});
}
hipError_t rt_launch_rebuild(const rt_rebuild_args *a, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = (size_t)a->n, global = a->local_level > 0 ? 1 : 0;      // (the words and the two lists: only a mesh with levels above the workgroup-local ones)
    return rec::launch("rebuild", stream, {
        {a->pts, n * 36, R, "new vertices"},
        {a->segs, (size_t)RT_REBUILD_SEGS * sizeof(rt_rb_seg), R, "update plan"},
        {a->slots, (size_t)a->num_nodes * sizeof(rt_rb_slot), R, "update plan"},
        {a->boxes, (size_t)RT_REBUILD_SEGS * RT_REBUILD_BOX_FLOATS * 4, W, "update boxes"},
        {a->words, global * (size_t)a->pad_n * 8, W, "update sort words"},
        {a->perm_a, global * n * 4, W, "update lists"},
        {a->perm_b, global * n * 4, W, "update lists"},
        {f4(a->blob, a->off_tris + a->tri_base * 3), n * 48, W, "scene blob"},
        {f4(a->blob, a->off_nodes + a->node_base * 4), (size_t)a->num_nodes * 64, W, "scene blob"},
        {f4(a->blob, a->off_meshes + a->mesh_index * 2), 32, W, "scene blob"},
        {f4(a->blob, a->off_objtab + a->object_index * 3), 48, W, "scene blob"},
        {f4(a->blob, a->off_objlds + a->object_index * RT_OBJLDS_F4 + 2), 16, W, "scene blob"},
        {a->objects ? a->objects + a->object_index : nullptr, sizeof(rt_object), W, "scene objects"},
        {a->tri_uv ? a->tri_uv + (size_t)a->tri_base * 6 : nullptr, n * 24, W, "triangle uvs"},
        {a->tri_uv ? a->uv0 : nullptr, n * 24, R, "commit-order uvs"},
        {a->perm, n * 4, W, "triangle order"}});
}
hipError_t rt_launch_cull(const float *, int32_t width, int32_t height, int32_t, const rt_f4 *blob, int32_t off_nodes, int32_t num_nodes, int32_t off_meshes, int32_t num_meshes,
                          uint32_t *plane, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("cull pre-pass", stream, {{f4(blob, off_nodes), (size_t)num_nodes * 64, R, "scene blob"}, {f4(blob, off_meshes), (size_t)num_meshes * 32, R, "scene blob"},
                                                 {plane, rt_cull_words(width, height) * 4, W, "cull plane"}});
}
hipError_t rt_launch_nearest(const rt_nearest_args *a, rt_shape, int, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n;
    return rec::launch("nearest", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"}, {a->points, n * 12, R, "points"},
                                           {a->max_dist, n * 4, R, "limits"}, {a->out, n * sizeof(rt_nearest), W, "nearest records"}});
}
hipError_t rt_launch_sweep(const rt_sweep_args *a, rt_shape, int, int, size_t, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n;
    return rec::launch("sphere cast", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {a->blob, (size_t)a->blob_f4 * 16, R, "scene blob"}, {a->origins, n * 12, R, "origins"},
                                               {a->directions, n * 12, R, "directions"}, {a->radius, n * 4, R, "radii"}, {a->tmax, n * 4, R, "limits"},
                                               {a->nearest, n * sizeof(rt_nearest), R, "sweep start records"}, {a->out, n * sizeof(rt_sweep), W, "sweep records"}});
}
hipError_t rt_launch_winding(const rt_winding_args *a, int, hipStream_t stream)
{
    using namespace rec_detail;
    const size_t n = a->n, tris = (size_t)a->num_tris;
    return rec::launch("winding", stream, {{a->counter, COUNTER_BYTES, W, "ticket counter"}, {f4(a->blob, a->off_tris), tris * 48, R, "scene blob"},
                                           {f4(a->blob, a->off_objtab), (size_t)a->num_objects * 48, R, "scene blob"}, {a->perm, tris * 4, R, "triangle order"},
                                           {a->flip, (tris + 3) / 4 * 4, R, "flip bytes"}, {a->points, n * 12, R, "points"}, {a->winding, n * 4, W, "winding numbers"},
                                           {a->inside, n, W, "containment bytes"}, {a->sdf ? a->nearest : nullptr, n * sizeof(rt_nearest), R, "nearest records"},
                                           {a->sdf, n * 4, W, "signed distances"}});
}
hipError_t rt_launch_eval(int, const uint32_t *in, uint32_t *out, int n, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("eval", stream, {{in, (size_t)n * 4, R, "eval input"}, {out, (size_t)n * 4, W, "eval output"}});
}
hipError_t rt_launch_exhaustive(unsigned long long *out4, hipStream_t stream)
{
    using namespace rec_detail;
    return rec::launch("exhaustive", stream, {{out4, 32, rec_detail::W, "counters"}});
}
}
