/*
 * rt_capi.cpp — the device half of the C ABI (include/rt_amd.h): context and scene life cycle, the
 * tile-list cache, the view and its schedule, render launches (render_frames), their host-buffer forms,
 * timing, the debug hooks.  Replaces the reference's host<->device seam
 * (src/dispatch.cu:104-163): where the reference allocates and frees four device buffers per
 * frame and copies the frame element-wise out of managed memory, the context here keeps
 * persistent HBM frame buffers and the device-buffer entry point takes caller-owned HBM.
 * What the launches' tile orders are is worked out in rt_schedule.h; frames in flight are in
 * rt_pipeline_capi.cpp, tile ownership over GPUs and the multi-GPU entry points in rt_multi_capi.cpp.
 *
 * There is no CPU fallback: rt_ctx_create fails when HIP has no device.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "rt_internal.h"

std::mutex rt_detail::g_ctx_mutex;

namespace {

/* the live contexts: a root keeps a landing area per SOURCE context (rt_ctx::multi.stages), which has to go when the source does */
std::set<rt_ctx *> g_live_ctxs;

uint64_t fnv1a(const void *data, size_t bytes, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

/* `list` into the entry `dl` and on its way to the device on `stream`.  A recycled entry's new upload must not overtake a
 * queued launch that still reads the old content (same stream: stream order; another stream: an event), and the pinned
 * copy is rewritten only once ITS last upload is done - which it has been since `cap` lists ago, so that wait
 * returns at once.  On an error *what says which step failed. */
hipError_t fill_dev_list(DevList &dl, bool recycled, const uint32_t *list, int n, hipStream_t stream, const char **what)
{
    hipError_t e = hipSuccess;
    if (recycled) {
        *what = "ordering a tile list's reuse";
        e = hipEventRecord(dl.ev, dl.stream);
        if (e == hipSuccess && dl.stream != stream) e = hipStreamWaitEvent(stream, dl.ev, 0);
        if (e != hipSuccess) return e;
    }
    if (dl.d.cap < (size_t)n) {
        /* a larger buffer: the old one goes once the launches reading it are done (the event just recorded) */
        if (dl.d.p) (void)hipEventSynchronize(dl.ev);    /* (rare: lists of one image size share a capacity) */
        dl.clear();
        const size_t cap = (size_t)n + (size_t)n / 4 + 64;
        *what = "allocating a tile list";
        if ((e = dl.d.grow(cap)) != hipSuccess) return e;
        *what = "allocating a tile list's staging copy";
        if ((e = hipHostMalloc((void **)&dl.host, cap * 4, hipHostMallocDefault)) != hipSuccess) { dl.host = nullptr; return e; }
    } else if (dl.n > 0) {
        (void)hipEventSynchronize(dl.ev_up);
    }
    std::memcpy(dl.host, list, (size_t)n * 4);
    *what = "uploading a tile list";
    e = hipMemcpyAsync(dl.d.p, dl.host, (size_t)n * 4, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(dl.ev_up, stream);
    return e;
}

}  // namespace

/* `list` (host) on ctx's GPU, for launches the caller queues on `stream` after this call.  A list seen before costs a hash
 * and a compare.  A new one takes a free entry or recycles the least recently used one: its content goes into the entry's
 * pinned buffer and is uploaded asynchronously on `stream`, behind (hipStreamWaitEvent) whatever was queued on the stream
 * the entry last served - no host synchronisation on the steady-state path, and no device-wide one ever (round 3 emptied a
 * full cache after hipDeviceSynchronize and waited for every upload).  The pointer stays valid until the entry
 * is recycled: after `cap` other lists, and never while pinned.  An entry that fails is left empty (a new one is
 * dropped). */
rt_status TileListCache::on_device(rt_ctx *ctx, const uint32_t *list, int n, hipStream_t stream, const uint32_t **out)
{
    *out = nullptr;
    if (n <= 0) return RT_OK;
    const uint64_t h = fnv1a(list, (size_t)n * 4);
    for (DevList &dl : lists)
        if (dl.hash == h && dl.n == n && std::memcmp(dl.host, list, (size_t)n * 4) == 0) {
            if (dl.stream != stream) {
                /* handed to another stream than the one its upload (or last use) was queued on: order the two */
                RT_HIP(ctx, hipEventRecord(dl.ev, dl.stream), "recording a tile list's use");
                RT_HIP(ctx, hipStreamWaitEvent(stream, dl.ev, 0), "ordering a tile list's use");
                dl.stream = stream;
            }
            dl.seq = ++seq;
            *out = dl.d.p;
            return RT_OK;
        }
    DevList *slot = nullptr;
    if (lists.size() >= cap) {
        for (DevList &dl : lists)
            if ((pin_floor == ~0ull || dl.seq <= pin_floor) && (!slot || dl.seq < slot->seq)) slot = &dl;
        if (!slot) cap = lists.size() + 1;      /* everything is pinned by the running call: grow */
    }
    const bool recycled = slot != nullptr;
    if (!recycled) {
        lists.emplace_back();
        slot = &lists.back();
        hipError_t e = hipEventCreateWithFlags(&slot->ev.e, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&slot->ev_up.e, hipEventDisableTiming);
        if (e != hipSuccess) { lists.pop_back(); return hip_fail(ctx, e, "creating a tile list's event"); }
    }
    const char *what = "";
    const hipError_t e = fill_dev_list(*slot, recycled, list, n, stream, &what);
    if (e != hipSuccess) { slot->clear(); return hip_fail(ctx, e, what); }
    slot->hash = h; slot->n = n; slot->stream = stream; slot->seq = ++seq;
    *out = slot->d.p;
    return RT_OK;
}

uint32_t rt_detail::next_scene_uid()
{
    static std::atomic<uint32_t> next_uid{1};
    return next_uid.fetch_add(1);
}

int rt_detail::batch_cap(const rt_ctx *ctx, size_t plane_floats)
{
    const size_t plane_bytes = plane_floats * 4;
    if (plane_bytes == 0 || ctx->total_mem == 0) return RT_MAX_BATCH_FRAMES;
    const size_t k = (ctx->total_mem / 4) / plane_bytes;
    return k >= RT_MAX_BATCH_FRAMES ? RT_MAX_BATCH_FRAMES : (k < 1 ? 1 : (int)k);
}

/* an integer RT_AMD_* variable: its value if that lies in lo..hi, otherwise (or when it is not set) `def` */
static int env_int(const char *name, int lo, int hi, int def)
{
    const char *e = getenv(name);
    if (!e) return def;
    const int v = atoi(e);
    return v >= lo && v <= hi ? v : def;
}

extern "C" const char *rt_version(void) { return "ray-tracer_amd 0.4.1 (gfx950)"; }

extern "C" rt_status rt_ctx_create(int32_t device, rt_ctx **out)
{
    if (!out) return RT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return RT_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RT_ERR_INVALID;
    rt_ctx *ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return RT_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return RT_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete ctx; return RT_ERR_NO_DEVICE; }
    ctx->num_cus = prop.multiProcessorCount;
    ctx->total_mem = prop.totalGlobalMem;
    Knobs &k = ctx->knobs;
    for (const rt_sched::KnobRange &r : rt_sched::KNOB_RANGES) k.*r.field = env_int(r.env, r.lo, r.hi, k.*r.field);
    k.descend_keep_given = env_int("RT_AMD_DESCEND_KEEP", 0, 64, -1) >= 0;      /* (an explicit value replaces the per-shape default: rt_sched::render_descend_keep) */
    ctx->multi.careful = env_int("RT_AMD_MULTI_CAREFUL", INT_MIN, INT_MAX, 0) != 0;
    ctx->cull.enabled = env_int("RT_AMD_PRIMARY_CULL", 0, 1, 1) != 0;
    ctx->cull.gates = env_int("RT_AMD_SUBTREE_CULL", 0, 1, 1) != 0;
    ctx->cull.entry = env_int("RT_AMD_PRIMARY_ENTRY", 0, 1, 1) != 0;
    ctx->cull.sub = env_int("RT_AMD_PRIMARY_SUBENTRY", 0, 1, 1) != 0;
    ctx->cull.sub_threshold = env_int("RT_AMD_SUBENTRY_SAMPLES", 0, 1 << 30, RT_SUB_THRESHOLD_SAMPLES);
    if (ctx->tile_counter.grow(256) != hipSuccess ||
        hipEventCreate(&ctx->ev_start.e) != hipSuccess || hipEventCreate(&ctx->ev_stop.e) != hipSuccess) {
        delete ctx;
        return RT_ERR_HIP;
    }
    {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        g_live_ctxs.insert(ctx);
    }
    *out = ctx;
    return RT_OK;
}

extern "C" void rt_ctx_destroy(rt_ctx *ctx)
{
    if (!ctx) return;
    {
        /* landing areas other contexts keep for this one (it was a rank of their multi-GPU calls) */
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        g_live_ctxs.erase(ctx);
        for (rt_ctx *r : g_live_ctxs) {
            auto it = r->multi.stages.find(ctx);
            if (it == r->multi.stages.end()) continue;
            (void)hipSetDevice(r->device);
            if (it->second.ev_free) (void)hipEventSynchronize(it->second.ev_free);
            r->multi.stages.erase(it);
        }
    }
    (void)hipSetDevice(ctx->device);
    delete ctx;                          /* (everything it owns goes with it, the streams first: see rt_ctx) */
}

extern "C" const char *rt_last_error(const rt_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" rt_status rt_scene_commit(rt_ctx *ctx, const rt_scene_builder *b, rt_scene **out)
{
    if (!ctx || !b || !out) return RT_ERR_INVALID;
    *out = nullptr;
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) return RT_ERR_NOMEM;
    s->ctx = ctx;
    s->uid = next_scene_uid();
    std::string err = rt_flatten(*b, s->flat);
    if (!err.empty()) { delete s; return set_err(ctx, RT_ERR_UNSUPPORTED, err); }

    /* the kernel shape (rt_sched::choose_shape) from the runtime's occupancy answers; the RT_AMD_* overrides are development knobs */
    rt_sched::ShapeOverrides ov;
    if (const char *e = getenv("RT_AMD_THREADS")) { ov.threads_set = true; ov.threads = atoi(e); }
    if (const char *e = getenv("RT_AMD_SCENE_MODE")) ov.hybrid = atoi(e) != RT_SCENE_GLOBAL;   /* 0: no hybrid kernels */
    if (const char *e = getenv("RT_AMD_BLOCKS_PER_CU")) ov.blocks_per_cu = atoi(e);
    const size_t blob_bytes = s->flat.blob.size() * sizeof(rt_f4);
    /* one spare stack entry: the traversal loop always writes the slot above the top */
    const size_t per_thread = s->flat.has_mesh ? (size_t)(s->flat.stack_entries + 1) * 8 : 0;
    const char *shape_err = nullptr;
    (void)hipSetDevice(ctx->device);
    /* which render kernel of a shape the scene runs (rt_sched::choose_variant) is fixed by its traits: the occupancy probes ask about that kernel */
    const uint32_t traits = s->flat.traits;
    const bool generic = rt_sched::variant_forced_generic(getenv("RT_AMD_KERNEL_VARIANT"));
    const rt_status st = rt_sched::choose_shape(s->flat.has_mesh, blob_bytes, (size_t)s->flat.off_tris * sizeof(rt_f4), per_thread, ov,
                                                [traits, generic](rt_shape shape, size_t lds_bytes) {
                                                    shape.variant = rt_sched::choose_variant(traits, generic, shape);
                                                    return rt_kernel_blocks_per_cu(shape, lds_bytes);
                                                },
                                                s->kernel, &shape_err);
    if (st != RT_OK) { delete s; return set_err(ctx, st, shape_err); }
    s->kernel.shape.variant = rt_sched::choose_variant(traits, generic, s->kernel.shape);
    s->kernel.shape.mesh_obj = s->flat.mesh_obj;
    /* the occupancy probes discard their errors: a failed probe must not surface later as a launch error */
    (void)hipGetLastError();

    hipError_t e = s->d_blob.grow(s->flat.blob.size());
    if (e == hipSuccess && blob_bytes) e = hipMemcpy(s->d_blob.p, s->flat.blob.data(), blob_bytes, hipMemcpyHostToDevice);
    const size_t obj_bytes = s->flat.objects.size() * sizeof(rt_object);
    if (e == hipSuccess) e = s->d_objects.grow(s->flat.objects.size());
    if (e == hipSuccess && obj_bytes) e = hipMemcpy(s->d_objects.p, s->flat.objects.data(), obj_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && !s->flat.tri_uv.empty()) {
        e = s->d_tri_uv.grow(s->flat.tri_uv.size());
        if (e == hipSuccess) e = hipMemcpy(s->d_tri_uv.p, s->flat.tri_uv.data(), s->flat.tri_uv.size() * 4, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !s->flat.tex_data.empty()) {
        e = s->d_tex.grow(s->flat.tex_data.size());
        if (e == hipSuccess) e = hipMemcpy(s->d_tex.p, s->flat.tex_data.data(), s->flat.tex_data.size() * 4, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        rt_scene_destroy(s);
        return hip_fail(ctx, e, "uploading scene");
    }
    *out = s;
    return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene *s)
{
    if (!s) return;
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    delete s;                            /* (the device buffers go with it) */
}

extern "C" rt_status rt_scene_get_info(const rt_scene *s, rt_scene_info *out)
{
    if (!s || !out) return RT_ERR_INVALID;
    out->num_objects = (int32_t)s->flat.objects.size();
    out->num_triangles = s->flat.num_tris;
    out->num_nodes = s->flat.num_nodes;
    out->lds_bytes = (int32_t)s->kernel.lds_bytes;
    out->scene_in_lds = s->kernel.shape.mode;
    out->threads_per_block = s->kernel.shape.threads;
    out->stack_entries = s->flat.stack_entries;
    out->blocks_per_cu = s->kernel.blocks_per_cu;
    out->kernel_variant = s->kernel.shape.variant;
    return RT_OK;
}

extern "C" int32_t rt_tile_owned_rows(const rt_tile_spec *t, int32_t height)
{
    if (!t || t->band_rows <= 0 || t->band_stride <= 0 || t->band_first < 0 || t->band_first >= t->band_stride) return -1;
    rt_tile_spec bands = *t;
    bands.tile_list = nullptr;           /* (the band fields of any spec) */
    return rt_sched::Layout(bands, 0, height).owned_rows();
}

extern "C" int32_t rt_max_batch_frames(rt_ctx *ctx, int32_t width, int32_t height)
{
    if (!ctx || width <= 0 || height <= 0) return 1;
    return batch_cap(ctx, (size_t)width * (size_t)height * 3);
}

/* persistent waves: enough workgroups to fill the chip, each wave pulls 8x8 tiles */
int rt_detail::launch_blocks(const rt_ctx *ctx, const rt_scene *scene, int num_tiles)
{
    const int waves_per_block = scene->kernel.shape.threads / 64;
    int blocks = ctx->num_cus * scene->kernel.blocks_per_cu;
    const int needed = (num_tiles + waves_per_block - 1) / waves_per_block;
    return blocks > needed ? needed : blocks;
}

namespace {

/* the render kernels of every pipelined frame have finished (host wait); with_folds: so have the blends that read their planes
 * and the view's tile list */
rt_status drain_pipeline(rt_ctx *ctx, bool with_folds)
{
    for (FrameSlot &fs : ctx->pipe.slots) {
        if (fs.used) RT_HIP(ctx, hipEventSynchronize(fs.ev_done), "waiting for the frames in flight");
        if (with_folds && fs.folded) RT_HIP(ctx, hipEventSynchronize(fs.ev_free), "waiting for the frames in flight");
    }
    return RT_OK;
}

}  // namespace

/* d_prev and d_out of exactly `bytes` */
rt_status rt_detail::ensure_frame_buffers(rt_ctx *ctx, size_t bytes)
{
    const size_t floats = bytes / 4;
    if (ctx->d_prev.cap == floats && ctx->d_out.cap == floats) return RT_OK;
    ctx->d_prev.release();
    ctx->d_out.release();
    RT_HIP(ctx, ctx->d_prev.grow(floats), "allocating previous-frame buffer");
    RT_HIP(ctx, ctx->d_out.grow(floats), "allocating frame buffer");
    return RT_OK;
}

namespace {

/* `v` into `buf` (grown to fit) on `stream`; the host waits for the copy, as `v` is often a local */
rt_status upload(rt_ctx *ctx, DevBuf<uint32_t> &buf, const std::vector<uint32_t> &v, hipStream_t stream, const char *what)
{
    RT_HIP(ctx, buf.grow(v.size()), what);
    RT_HIP(ctx, hipMemcpyAsync(buf.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, stream), what);
    RT_HIP(ctx, hipStreamSynchronize(stream), what);
    return RT_OK;
}

/* The view's measured costs are on the device: bring them to the host on `stream` (one synchronisation).  Then, when the
 * view uses a tile order, move the most expensive tiles to its front (rt_sched::refined_order). */
rt_status read_costs_and_refine(rt_ctx *ctx, hipStream_t stream)
{
    View &v = ctx->view;
    const uint32_t n = (uint32_t)v.tiles.size();
    if (v.costs == Costs::on_device) {
        /* on the launch stream: the launch that collected the costs ran on it (or this stream has been ordered
         * behind it), and a blocking copy on the null stream would not wait for a non-blocking stream's kernel */
        std::vector<uint32_t> cost(n), peak(n);
        RT_HIP(ctx, hipMemcpyAsync(cost.data(), v.d_cost.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream), "reading tile costs");
        RT_HIP(ctx, hipMemcpyAsync(peak.data(), v.d_peak.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream), "reading tile costs");
        RT_HIP(ctx, hipStreamSynchronize(stream), "reading tile costs");
        v.cost.swap(cost);
        v.peak.swap(peak);
    }
    if (v.use_order) {
        /* nothing may still be indexing the old order: the stream was synchronised above, or (caller-supplied costs)
         * the order has not been used by a launch yet */
        std::vector<uint32_t> order;
        const uint32_t top = rt_sched::refined_order(v.order, v.cost, order);
        rt_status st = upload(ctx, v.d_order, order, stream, "uploading tile order");
        if (st != RT_OK) return st;
        v.order.swap(order);
        v.num_heavy = (int)top;
    }
    v.costs = Costs::on_host;
    v.job_frames = 0;                    /* any uploaded schedule is for another view */
    return RT_OK;
}

}  // namespace

/* (c + prev * n) / (n + 1) over the pixels a launch owns, frame by frame (src/raytracer.cu:109-112): `planes` holds n_frames planes of
 * per-pixel means in the output layout L.  Compact layouts, and a full frame rendered whole: one pass over the buffer; a
 * full-layout frame of which the launch owns some bands / tiles: only those are folded (tiles: d_tile_list, the list on the device) */
rt_status rt_detail::fold(rt_ctx *ctx, const rt_sched::Layout &L, const float *planes, int n_frames, int frame_num, float *d_out, const uint32_t *d_tile_list,
                          hipStream_t stream)
{
    const long long plane = (long long)L.plane_floats();
    if (L.compact || L.whole_frame()) {
        RT_HIP(ctx, rt_launch_blend(planes, plane, n_frames, frame_num, d_out, plane, stream), "launching blend kernel");
    } else if (L.listed) {
        RT_HIP(ctx, rt_launch_blend_tiles(planes, plane, n_frames, frame_num, d_out, d_tile_list, L.num_tiles, L.tiles_x, L.width, L.height, stream),
               "launching blend kernel");
    } else {
        for (int k = 0; k < L.owned_bands(); k++) {
            const long long off = (long long)L.band(k) * L.band_rows * L.width * 3, cnt = (long long)L.rows_of(L.band(k)) * L.width * 3;
            RT_HIP(ctx, rt_launch_blend(planes + off, plane, n_frames, frame_num, d_out + off, cnt, stream), "launching blend kernel");
        }
    }
    return RT_OK;
}

/* ---- one launch, step by step (render_frames below) ----------------------------------------------------------------------- */

static rt_status check_launch(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, const rt_tile_spec *t, bool have_out)
{
    if (!ctx || !scene || !cam || !rs || !have_out) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (scene->ctx != ctx) return set_err(ctx, RT_ERR_INVALID, "scene belongs to another context");
    if (rt_status st = check_image_size(ctx, cam->width, cam->height)) return st;
    if (rs->rays_per_pixel < 0 || rs->reflection_limit < 0) return set_err(ctx, RT_ERR_INVALID, "bad render settings");
    if (!t->tile_list && (t->tile_cost || t->tile_peak)) return set_err(ctx, RT_ERR_INVALID, "bad tile spec (tile_cost / tile_peak need a tile_list)");
    if (const char *bad = rt_sched::tile_spec_error(*t, (cam->width + 7) / 8, (cam->height + 7) / 8)) return set_err(ctx, RT_ERR_INVALID, bad);
    return RT_OK;
}

rt_kernel_args rt_detail::kernel_args(const rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, const int32_t *times_ms,
                                      int32_t n_frames, int32_t frame_num, const rt_sched::Layout &L, const float *d_prev, float *d_out, uint32_t *tile_counter)
{
    rt_kernel_args a;
    std::memset(&a, 0, sizeof a);
    camera_floats(*cam, a.cam);
    a.width = cam->width;
    a.height = cam->height;
    a.rays_per_pixel = rs->rays_per_pixel;
    a.reflection_limit = rs->reflection_limit;
    a.antialias = rs->antialias ? 1 : 0;
    std::memcpy(a.sky, rs->sky_colour, 12);
    for (int i = 0; i < n_frames; i++) a.seeds[i] = (uint32_t)times_ms[i] * 6291469u;       /* src/raytracer.cu:127 */
    a.num_frames = n_frames;
    a.frame_num = frame_num;
    a.band_rows = L.band_rows;
    a.band_first = L.band_first;
    a.band_stride = L.band_stride;
    a.compact = L.compact ? 1 : 0;
    a.tiles_x = L.tiles_x;
    a.num_tiles = L.num_tiles;
    a.tile_stride = rt_sched::coprime_stride((uint32_t)a.num_tiles);

    a.objects = scene->d_objects.p;
    a.num_objects = (int32_t)scene->flat.objects.size();
    a.blob = scene->d_blob.p;
    a.blob_f4 = (int32_t)scene->flat.blob.size();
    a.off_nodes = scene->flat.off_nodes;
    a.off_tris = scene->flat.off_tris;
    a.off_objlds = scene->flat.off_objlds;
    a.off_meshes = scene->flat.off_meshes;
    a.off_objtab = scene->flat.off_objtab;
    a.num_meshes = scene->flat.num_meshes;
    a.stack_entries = scene->flat.stack_entries;
    /* (the mapping keeps hit_low <= hit_break, without which the kernel's loops can stop making progress: rt_sched::kernel_knobs) */
    const rt_sched::KernelKnobs k = rt_sched::kernel_knobs(ctx->knobs, scene->kernel.shape.threads);
    a.work_threshold = k.work_threshold;
    a.ready_break = k.ready_break;
    a.hit_break = k.hit_break;
    a.hit_low = k.hit_low;
    a.mix_break = k.mix_break;
    a.shade_batch = k.shade_batch;
    a.descend_keep = rt_sched::render_descend_keep(ctx->knobs, scene->kernel.shape);
    a.tri_uv = scene->d_tri_uv.p;
    a.tex_data = scene->d_tex.p;
    a.prev = d_prev;
    a.out = d_out;
    a.tile_counter = tile_counter;
    a.stats = (unsigned long long *)(a.tile_counter + 16);   /* 48 x u64 after the counter; used by -DRT_STATS builds only */
    return a;
}

void rt_detail::push_camera(std::vector<uint32_t> &key, const rt_camera *cam)
{
    float f[12];
    camera_floats(*cam, f);
    key.resize(key.size() + 12);
    std::memcpy(&key[key.size() - 12], f, sizeof f);
}

static std::vector<uint32_t> view_key(const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, const rt_tile_spec *t, uint32_t n)
{
    std::vector<uint32_t> key;
    key.push_back(scene->uid);
    push_camera(key, cam);
    key.push_back((uint32_t)cam->width); key.push_back((uint32_t)cam->height);
    key.push_back((uint32_t)rs->reflection_limit);      /* (a launch at bounce limit 0 or 1 says nothing about one at 8) */
    if (t->tile_list) {
        uint64_t h = fnv1a(t->tile_list, (size_t)n * 4);
        if (t->tile_cost) h = fnv1a(t->tile_cost, (size_t)n * 4, h);
        if (t->tile_cost && t->tile_peak) h = fnv1a(t->tile_peak, (size_t)n * 4, h);
        key.push_back(0xffffffffu); key.push_back(n); key.push_back((uint32_t)h); key.push_back((uint32_t)(h >> 32)); key.push_back(t->tile_cost ? 1u : 0u);
    } else {
        key.push_back((uint32_t)t->band_rows); key.push_back((uint32_t)t->band_first); key.push_back((uint32_t)t->band_stride);
    }
    return key;
}

/* Pilot: a view's first launch would run on the guessed order (measured: 315 instead of 228 ms per frame for the monkey's first
 * five frames).  One sample per pixel of the launch's first frame, rendered into a scratch plane, measures the tiles well
 * enough to schedule by (~1/spp of a frame + one synchronisation); the launch itself then measures them properly for the
 * launches after it.  Nothing of the pilot reaches the image. */
static bool wants_pilot(const View &v, const rt_render_settings *rs)
{
    return v.use_order && rs->rays_per_pixel >= rt_sched::PILOT_MIN_SPP && rs->reflection_limit > 0;
}

/* the launch `a` adds up what its tiles cost */
static rt_status collect_costs(rt_ctx *ctx, rt_kernel_args &a, hipStream_t stream)
{
    View &v = ctx->view;
    RT_HIP(ctx, hipMemsetAsync(v.d_cost.p, 0, (size_t)a.num_tiles * 4, stream), "clearing tile costs");
    RT_HIP(ctx, hipMemsetAsync(v.d_peak.p, 0, (size_t)a.num_tiles * 4, stream), "clearing tile costs");
    a.tile_cost = v.d_cost.p;
    a.tile_peak = v.d_peak.p;
    return RT_OK;
}

/* Pipelined frames overlap as long as they only READ the view (tile order, tile list).  A launch that writes it - a new view, a
 * pilot, a launch that measures tile costs, the one that sorts by them - first waits (on the host) for the frames in flight:
 * once or twice per view.  A listed view's tile list is the pipeline's own copy. */
static rt_status pipeline_view(rt_ctx *ctx, const rt_render_settings *rs, const rt_tile_spec *t, uint32_t n, bool new_view, bool cost_fits, bool provisional)
{
    Pipeline &pl = ctx->pipe;
    const View &v = ctx->view;
    const bool listed = t->tile_list != nullptr;
    const bool list_changed = listed && (pl.list_host.size() != (size_t)n || std::memcmp(pl.list_host.data(), t->tile_list, (size_t)n * 4) != 0);
    if (list_changed)
        for (int j = 0; j < pl.pending; j++)
            if (pl.slots[pl.order[j]].layout.listed)
                return set_err(ctx, RT_ERR_BUSY, "frames of another tile list are waiting to be collected (rt_frame_collect; d_frame == NULL discards one)");
    if (new_view || list_changed || (v.costs == Costs::none && (cost_fits || wants_pilot(v, rs))) || (v.costs == Costs::on_device && v.use_order) || provisional) {
        rt_status st = drain_pipeline(ctx, new_view || list_changed);
        if (st != RT_OK) return st;
    }
    if (listed && (list_changed || !pl.d_list.p)) {
        RT_HIP(ctx, pl.d_list.grow(n), "allocating the pipeline's tile list");
        pl.list_host.clear();
        RT_HIP(ctx, hipMemcpy(pl.d_list.p, t->tile_list, (size_t)n * 4, hipMemcpyHostToDevice), "uploading the pipeline's tile list");
        pl.list_host.assign(t->tile_list, t->tile_list + n);
    }
    return RT_OK;
}

/* a new view: its tiles, the first guess of their order, and the costs the caller may know (an earlier launch of the view,
 * possibly on other GPUs) */
static rt_status new_view(rt_ctx *ctx, const rt_scene *scene, const rt_tile_spec *t, const rt_kernel_args &a, const std::vector<uint32_t> &key, hipStream_t stream)
{
    View &v = ctx->view;
    std::vector<uint32_t> tiles;
    if (!rt_sched::view_tiles(*t, a.width, a.height, tiles)) return set_err(ctx, RT_ERR_INVALID, "bad tile spec (a tile index outside the image, or listed twice)");
    const uint32_t n = (uint32_t)tiles.size();
    v.key.clear();                       /* (until everything below has succeeded) */
    v.tiles.swap(tiles);
    v.costs = Costs::none;
    v.cost.clear();
    v.peak.clear();
    v.num_heavy = 0;
    v.job_frames = 0;
    RT_HIP(ctx, v.d_cost.grow(n), "allocating tile costs");
    RT_HIP(ctx, v.d_peak.grow(n), "allocating tile costs");
    v.use_order = scene->flat.num_meshes > 0 && n > 1;
    rt_status st;
    if (v.use_order) {
        std::vector<uint32_t> order = rt_sched::guessed_order(v.tiles, a.tiles_x, a.cam, scene->flat.objects);
        if ((st = upload(ctx, v.d_order, order, stream, "uploading tile order")) != RT_OK) return st;
        v.order.swap(order);
    }
    if (t->tile_list && t->tile_cost) {
        v.cost.assign(t->tile_cost, t->tile_cost + n);
        if (t->tile_peak) v.peak.assign(t->tile_peak, t->tile_peak + n);
        else v.peak = v.cost;
        if ((st = read_costs_and_refine(ctx, stream)) != RT_OK) return st;
    }
    v.key = key;
    return RT_OK;
}

static rt_status run_pilot(rt_ctx *ctx, const rt_scene *scene, const rt_kernel_args &a, size_t plane_floats, size_t n_planes, hipStream_t stream)
{
    View &v = ctx->view;
    RT_HIP(ctx, ctx->d_partial.grow(plane_floats * n_planes), "allocating the pilot's scratch plane");
    rt_kernel_args ap = a;
    ap.rays_per_pixel = 1;
    ap.num_frames = 1;
    ap.partial = ctx->d_partial.p;
    ap.partial_plane = (int64_t)(plane_floats / 3);
    ap.prev = nullptr;
    ap.tile_order = v.d_order.p;
    rt_status st = collect_costs(ctx, ap, stream);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipMemsetAsync(ap.tile_counter, 0, 512, stream), "clearing tile counter");
    RT_HIP(ctx, rt_launch_render(&ap, scene->kernel.shape, launch_blocks(ctx, scene, ap.num_tiles), scene->kernel.lds_bytes, stream),
           "launching the pilot");
    v.costs = Costs::on_device;
    v.cost_spp = 1;
    return read_costs_and_refine(ctx, stream);      /* -> on_host: a provisional schedule */
}

/* Multi-frame launch of a view whose tile costs are known: the host lays out the whole schedule.  A job is one tile of one
 * frame; a pixel's samples are one sequential random stream, so a job cannot be split and the launch is at least as long as
 * its longest job - which therefore has to start at once, for EVERY frame (frames only meet in the blend behind the kernel).
 * Longest processing time first (rt_sched::build_job_order).  Consecutive tickets are also similar in cost, so the lanes a
 * wave refills as its cheap pixels finish collect pixels of one kind.  (Measured, 20 frames of the monkey configuration: +6 %
 * on one GPU and +25 % on the share one of 8 GPUs renders, against "the 1,024 most expensive tiles of frame 0, of frame 1,
 * ... first".) */
static rt_status tile_schedule(rt_ctx *ctx, rt_kernel_args &a, hipStream_t stream)
{
    View &v = ctx->view;
    const uint32_t n = (uint32_t)a.num_tiles;
    const bool known = v.costs == Costs::on_host && a.num_frames > 1;
    a.num_heavy_tiles = known ? v.num_heavy : 0;
    a.tile_order = v.d_order.p;
    if (!known || n > RT_JOB_TILE_MASK + 1u || v.cost.size() != n || v.peak.size() != n) return RT_OK;
    if (v.job_frames != a.num_frames) {
        std::vector<uint32_t> jobs;
        rt_sched::build_job_order(v.order, v.cost, v.peak, (uint32_t)a.num_frames, jobs);
        rt_status st = upload(ctx, v.d_jobs, jobs, stream, "uploading the launch schedule");
        if (st != RT_OK) return st;
        v.job_frames = a.num_frames;
    }
    a.job_order = v.d_jobs.p;
    return RT_OK;
}

/* The view of a launch with tiles: which ones, in which order, at what cost.  The first launch of a view adds up, per tile,
 * the work of its pixels (*collecting); the next reads the sums back (one synchronisation) and moves the most expensive
 * tiles to the front of the order.  In a multi-frame launch those tiles go first for ALL frames (see px_fetch): with the
 * true costs that is worth 10 % at three frames per launch (with the guess, nothing). */
static rt_status prepare_view(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, const rt_tile_spec *t,
                              rt_kernel_args &a, size_t plane_floats, bool in_place, FrameSlot *slot, hipStream_t stream, bool *collecting)
{
    View &v = ctx->view;
    const uint32_t n = (uint32_t)a.num_tiles;
    const std::vector<uint32_t> key = view_key(scene, cam, rs, t, n);
    /* a pixel's cost counter is 26 bits wide (rt_device_scene.h RT_COST_*): launches that could overflow it (65,536 or
     * more bounces per pixel) do not collect costs and run on the schedule the view already has */
    const bool cost_fits = (long long)rs->rays_per_pixel * (long long)(rs->reflection_limit > 0 ? rs->reflection_limit : 1) < 65536ll;
    /* figures from a launch with far fewer samples (a 1-spp preview, a profiler's warm-up launch) are provisional
     * like a pilot's: this launch runs on them and measures again */
    const bool is_new = key != v.key;
    const bool provisional = !is_new && v.costs == Costs::on_host && v.cost_spp > 0 && (long long)v.cost_spp * 8 <= (long long)rs->rays_per_pixel &&
                             !(t->tile_list && t->tile_cost) && cost_fits;
    rt_status st;
    if (slot && (st = pipeline_view(ctx, rs, t, n, is_new, cost_fits, provisional)) != RT_OK) return st;
    if (is_new && (st = new_view(ctx, scene, t, a, key, stream)) != RT_OK) return st;
    if (t->tile_list) {
        if (slot) a.tile_list = ctx->pipe.d_list.p;
        else if ((st = ctx->tile_lists.on_device(ctx, t->tile_list, (int)n, stream, &a.tile_list)) != RT_OK) return st;
    }
    if (v.costs == Costs::none) {
        if (wants_pilot(v, rs) && (st = run_pilot(ctx, scene, a, plane_floats, in_place ? (size_t)a.num_frames : 1, stream)) != RT_OK) return st;
        *collecting = cost_fits;
    } else {
        if (v.costs == Costs::on_device && v.use_order && (st = read_costs_and_refine(ctx, stream)) != RT_OK) return st;
        *collecting = provisional;
    }
    if (*collecting && (st = collect_costs(ctx, a, stream)) != RT_OK) return st;
    return v.use_order ? tile_schedule(ctx, a, stream) : RT_OK;
}

/* where the launch's per-frame means go: a pipelined frame's plane, the planes of a multi-frame launch, or nowhere (a plain
 * one-frame launch writes d_out itself) */
static rt_status bind_output(rt_ctx *ctx, rt_kernel_args &a, const rt_sched::Layout &L, bool in_place, FrameSlot *slot)
{
    const size_t plane_floats = L.plane_floats();
    if (slot) {
        if (slot->plane.cap < plane_floats && slot->folded) RT_HIP(ctx, hipEventSynchronize(slot->ev_free), "waiting for a frame's blend");   /* (the plane is about to be replaced) */
        RT_HIP(ctx, slot->plane.grow(plane_floats), "allocating a pipelined frame's plane");
        a.partial = slot->plane.p;
        slot->layout = L;
    } else if (in_place) {
        RT_HIP(ctx, ctx->d_partial.grow(plane_floats * (size_t)a.num_frames), "allocating the per-frame planes of a multi-frame launch");
        a.partial = ctx->d_partial.p;
    } else {
        return RT_OK;
    }
    a.partial_plane = (int64_t)(plane_floats / 3);
    return RT_OK;
}

/* The view's cull plane for the launch `a` (rt_cull.h): reused if it was computed for this scene revision, camera, image size and antialias
 * flag, else computed now by the pre-pass on the launch's stream - no host wait, the render kernel is the next kernel on that stream.  A
 * scene's uid changes with every update of its geometry (rt_update_capi.cpp), so a commit and an update both find the plane stale.  Nothing
 * here fails the launch: without an allocation, a launcher or an event the launch renders without a plane, which costs time and nothing else.
 * Only a scene whose kernel reads the plane gets one (rt_loop_culls). */
static void bind_cull(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, rt_kernel_args &a, FrameSlot *slot, hipStream_t stream)
{
    CullPlane &cp = ctx->cull;
    const rt_shape &sh = scene->kernel.shape;
    const bool enabled = cp.enabled && scene->flat.num_meshes > 0 && rt_loop_culls(sh.has_mesh, sh.mode, sh.threads, sh.variant);
    rt_cull_host::Key k;
    k.scene_uid = scene->uid;
    camera_floats(*cam, k.cam);
    k.width = cam->width; k.height = cam->height; k.antialias = rs->antialias ? 1 : 0;
    /* (the sub-entry tables, rt_entry.h: only the one-mesh scene whose triangles the flags can name has them) */
    const bool entry = cp.entry && scene->flat.num_meshes == 1 && scene->flat.off_tris >= 0 && scene->flat.off_tris < (1 << (31 - RT_CULL_TRIS_SHIFT));
    cp.plan.want_tables = cp.sub && entry;
    const rt_cull_host::Step step = cp.plan.next(k, enabled, [&](size_t words) {
        /* (the old plane is freed first, which waits for the launches that read it) */
        /* the bits and, behind them, the gate words and the entry words; with `tables` the sub-entry tables behind those */
        const bool ok = cp.d.grow(cp.plan.tables ? rt_sub_alloc_words(words) : rt_cull_alloc_words_entry(words)) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    });
    if (step == rt_cull_host::Step::none) return;
    const bool refine = cp.plan.refine(step, k, (int64_t)rs->rays_per_pixel * (int64_t)a.num_frames, cp.sub_threshold);
    bool ok = true;
    if (step == rt_cull_host::Step::reuse && cp.stream != stream) ok = hipStreamWaitEvent(stream, cp.ev, 0) == hipSuccess;
    if (step == rt_cull_host::Step::run || refine) {
        /* the plane is rewritten: ordinary launches are already behind every launch that read it (render_frames); a pipelined frame
         * overlaps the others in flight, whose render kernels are waited for here - once per view, and once more where its refinement
         * is queued by a later launch */
        if (slot)
            for (FrameSlot &fs : ctx->pipe.slots)
                if (fs.used && &fs != slot) ok = ok && hipEventSynchronize(fs.ev_done) == hipSuccess;
        if (ok && !cp.ev.e) ok = hipEventCreateWithFlags(&cp.ev.e, hipEventDisableTiming) == hipSuccess;
        /* (the entry words need the triangles: where they start rides in the flags' upper bits, rt_entry.h.  A reused plane has its
         * words: RT_CULL_WITH_SUBENTRY without RT_CULL_WITH_ENTRY queues the refinement alone) */
        const bool pre_pass = step == rt_cull_host::Step::run;
        const int32_t view_flags = (k.antialias ? RT_CULL_ANTIALIAS : 0) | (cp.gates ? RT_CULL_WITH_GATES : 0) | (entry && pre_pass ? RT_CULL_WITH_ENTRY : 0) |
                                   (refine ? RT_CULL_WITH_SUBENTRY : 0) | (entry ? scene->flat.off_tris << RT_CULL_TRIS_SHIFT : 0);
        ok = ok && rt_launch_cull(k.cam, k.width, k.height, view_flags, scene->d_blob.p, scene->flat.off_nodes, scene->flat.num_nodes, scene->flat.off_meshes,
                                  scene->flat.num_meshes, cp.d.p, stream) == hipSuccess;
        ok = ok && hipEventRecord(cp.ev, stream) == hipSuccess;
        cp.stream = stream;
        if (pre_pass) cp.plan.ran(k, ok);
        else if (!ok) cp.plan.refine_failed();
    }
    if (!ok) { (void)hipGetLastError(); return; }
    rt_kernel_args_set_cull(a, cp.d.p);
    cp.plan.used_last = true;
}

static rt_status launch(rt_ctx *ctx, const rt_scene *scene, const rt_kernel_args &a, bool pipelined, hipStream_t stream)
{
    int blocks = launch_blocks(ctx, scene, a.num_tiles);
    /* A pipelined frame gets its share of the CUs, not all of them: a frame alone on the GPU is as long as its longest
     * pixel and leaves most CUs idle (or held by a workgroup with one busy wave) for half of that time; on 1 / depth of
     * the CUs the same frame is bound by its work instead, and `depth` of them fill the GPU (measured, monkey 1080p
     * 1024 spp, 4 in flight: 286 ms per frame with full-size launches, 242 with quarter-size ones).
     * Only where a workgroup has its CU to itself (a mesh that fills the LDS): smaller workgroups of several launches share
     * CUs anyway, and full-size launches are then the faster ones (three-sphere 61.7 against 65.1 ms, cube 112.8 against 118.0). */
    if (pipelined && scene->kernel.blocks_per_cu == 1) blocks = (blocks + ctx->pipe.depth - 1) / ctx->pipe.depth;
    RT_HIP(ctx, hipMemsetAsync(a.tile_counter, 0, 512, stream), "clearing tile counter");
    RT_HIP(ctx, rt_launch_render(&a, scene->kernel.shape, blocks, scene->kernel.lds_bytes, stream), "launching render kernel");
    return RT_OK;
}

/* One launch rendering n_frames consecutive progressive frames (n_frames == 1: a plain frame with an optional separate previous
 * frame; > 1, or in_place: d_out is updated in place through one plane of per-pixel means per frame).
 * slot != NULL: a pipelined frame (rt_frame_submit) - the launch runs on the slot's stream with the slot's ticket counter, its
 * pixels' means go to the slot's plane and nothing is folded here; d_prev, d_out and hip_stream are not used. */
rt_status rt_detail::render_frames(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                   const int32_t *times_ms, int32_t n_frames, int32_t frame_num, const rt_tile_spec *tiles,
                                   const float *d_prev, float *d_out, void *hip_stream, bool in_place, FrameSlot *slot)
{
    const rt_tile_spec full = rt_sched::whole_image_spec();
    const rt_tile_spec *t = tiles ? tiles : &full;
    rt_status st = check_launch(ctx, scene, cam, rs, t, d_out || slot);
    if (st != RT_OK) return st;
    hipStream_t stream = slot ? slot->stream : (hipStream_t)hip_stream;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* one launch in flight per context: the scratch is shared (see rt_ctx) ... */
    if (ctx->launched && (slot || ctx->last_stream != stream)) RT_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_stop, 0), "ordering the launch behind the previous one");
    /* ... except pipelined frames, which bring their own (FrameSlot) and only read the view's: they overlap each other, and an
     * ordinary launch is queued behind all of them */
    if (!slot)
        for (FrameSlot &fs : ctx->pipe.slots)
            if (fs.used) RT_HIP(ctx, hipStreamWaitEvent(stream, fs.ev_done, 0), "ordering the launch behind the frames in flight");

    const rt_sched::Layout L(*t, cam->width, cam->height);
    rt_kernel_args a = kernel_args(ctx, scene, cam, rs, times_ms, n_frames, frame_num, L, d_prev, d_out, slot ? slot->counter.p : ctx->tile_counter.p);
    bool collecting = false;
    if (a.num_tiles > 0 && (st = prepare_view(ctx, scene, cam, rs, t, a, L.plane_floats(), in_place, slot, stream, &collecting)) != RT_OK) return st;
    if ((st = bind_output(ctx, a, L, in_place, slot)) != RT_OK) return st;
    if (a.num_tiles > 0) bind_cull(ctx, scene, cam, rs, a, slot, stream);
    if (!slot) {
        RT_HIP(ctx, hipEventRecord(ctx->ev_start, stream), "recording start event");
        ctx->have_timing = false;
    }
    if (a.num_tiles > 0) {
        if ((st = launch(ctx, scene, a, slot != nullptr, stream)) != RT_OK) return st;
        if (collecting) { ctx->view.costs = Costs::on_device; ctx->view.cost_spp = rs->rays_per_pixel; }   /* only now: a failed launch leaves no costs to sort on */
    }
    if (slot) {
        RT_HIP(ctx, hipEventRecord(slot->ev_done, stream), "recording a pipelined frame's end");
        slot->used = true;
        return RT_OK;
    }
    if (in_place && a.num_tiles > 0 && (st = fold(ctx, L, ctx->d_partial.p, n_frames, frame_num, d_out, a.tile_list, stream)) != RT_OK) return st;
    RT_HIP(ctx, hipEventRecord(ctx->ev_stop, stream), "recording stop event");
    ctx->have_timing = true;
    ctx->launched = true;
    ctx->last_stream = stream;
    return RT_OK;
}

extern "C" rt_status rt_render_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                      int32_t time_ms, int32_t frame_num, const rt_tile_spec *tiles,
                                      const float *d_prev, float *d_out, void *hip_stream)
{
    return render_frames(ctx, scene, cam, rs, &time_ms, 1, frame_num, tiles, d_prev, d_out, hip_stream, false);
}

/* n_frames consecutive progressive frames (frame_num, frame_num + 1, ...; seeds times_ms[i]) in ONE
 * launch, accumulated in place in d_frame (layout of rt_render_device's d_out; its content is the
 * previous frame when frame_num > 0, ignored otherwise).  The result is bit-identical to n_frames
 * calls of rt_render_device; the point is that frame k + 1 is traced while the expensive pixels of
 * frame k are still running, which a launch per frame cannot do. */
extern "C" rt_status rt_render_device_batch(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                            const int32_t *times_ms, int32_t n_frames, int32_t frame_num, const rt_tile_spec *tiles,
                                            float *d_frame, void *hip_stream)
{
    if (!times_ms || n_frames < 1 || n_frames > RT_MAX_BATCH_FRAMES) return set_err(ctx, RT_ERR_INVALID, "n_frames must be 1..32");
    if (frame_num < 0) return set_err(ctx, RT_ERR_INVALID, "bad frame number");
    return render_frames(ctx, scene, cam, rs, times_ms, n_frames, frame_num, tiles, nullptr, d_frame, hip_stream, true);
}

extern "C" rt_status rt_tile_costs(rt_ctx *ctx, uint32_t *tile_ids, uint32_t *costs, uint32_t *peaks, int32_t capacity, int32_t *count)
{
    if (!ctx || !count || capacity < 0 || (capacity > 0 && (!tile_ids || !costs))) return set_err(ctx, RT_ERR_INVALID, "null argument");
    *count = 0;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const View &v = ctx->view;
    if (v.key.empty() || v.costs == Costs::none) return set_err(ctx, RT_ERR_INVALID, "no launch of the current view has collected tile costs");
    if (v.costs == Costs::on_device) {
        rt_status st = drain_pipeline(ctx, false);       /* (a pipelined frame may be the launch that measures, or be reading the order) */
        if (st != RT_OK) return st;
        st = read_costs_and_refine(ctx, ctx->last_stream);
        if (st != RT_OK) return st;
    }
    const size_t n = v.tiles.size();
    if (v.cost.size() != n || v.peak.size() != n) return set_err(ctx, RT_ERR_INVALID, "no launch of the current view has collected tile costs");
    const size_t m = n < (size_t)capacity ? n : (size_t)capacity;
    for (size_t i = 0; i < m; i++) { tile_ids[i] = v.tiles[i]; costs[i] = v.cost[i]; if (peaks) peaks[i] = v.peak[i]; }
    *count = (int32_t)n;
    return RT_OK;
}

extern "C" rt_status rt_tiles_copy_device(rt_ctx *ctx, float *d_compact, float *d_frame, int32_t width, int32_t height,
                                          const uint32_t *tile_list, int32_t num_tiles, int32_t to_frame, void *hip_stream)
{
    if (!ctx || !d_compact || !d_frame || width <= 0 || height <= 0 || num_tiles < 0 || (num_tiles > 0 && !tile_list)) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (!rt_sched::tiles_in_image(tile_list, num_tiles, tiles_x, tiles_y)) return set_err(ctx, RT_ERR_INVALID, "a tile index outside the image");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const uint32_t *d_list = nullptr;
    rt_status st = ctx->tile_lists.on_device(ctx, tile_list, num_tiles, (hipStream_t)hip_stream, &d_list);
    if (st != RT_OK) return st;
    RT_HIP(ctx, rt_launch_tiles_copy(d_compact, d_frame, d_list, num_tiles, tiles_x, width, height, to_frame ? 1 : 0, (hipStream_t)hip_stream), "launching the tile copy");
    return RT_OK;
}

/* test hook: evaluates one function of rt_math.h / rt_rng.h on the DEVICE for n inputs given
 * and returned as raw 32-bit patterns in host memory */
extern "C" rt_status rt_debug_eval(rt_ctx *ctx, int32_t op, const uint32_t *in, uint32_t *out, int32_t n)
{
    if (!ctx || !in || !out || n <= 0 || op < 0 || op > 15) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    uint32_t *d_in = nullptr, *d_out = nullptr;
    RT_HIP(ctx, hipMalloc((void **)&d_in, (size_t)n * 4), "allocating eval input");
    hipError_t e = hipMalloc((void **)&d_out, (size_t)n * 4);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rt_launch_eval(op, d_in, d_out, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return hip_fail(ctx, e, "evaluating on the device");
    return RT_OK;
}

/* test hook: the short reciprocal and square root of the device code (rt_vec.h rt_rcp_short / rt_sqrt_short) against the
 * compiler's IEEE expansions for every one of the 2^32 binary32 inputs, on the device.  out4 = {reciprocal: inputs inside its
 * range that differ, inputs inside its range; square root: likewise} */
extern "C" rt_status rt_debug_exhaustive(rt_ctx *ctx, unsigned long long *out4)
{
    if (!ctx || !out4) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    unsigned long long *d = nullptr;
    RT_HIP(ctx, hipMalloc((void **)&d, 32), "allocating counters");
    hipError_t e = hipMemset(d, 0, 32);
    if (e == hipSuccess) e = rt_launch_exhaustive(d, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out4, d, 32, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(ctx, e, "exhaustive check on the device");
    return RT_OK;
}

/* development hook: copies the 48 section counters / timers of a -DRT_STATS build (zeros otherwise) */
extern "C" rt_status rt_debug_read_stats(rt_ctx *ctx, unsigned long long *out48)
{
    if (!ctx || !out48) return RT_ERR_INVALID;
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for render kernel");
    RT_HIP(ctx, hipMemcpy(out48, ctx->tile_counter.p + 16, 48 * 8, hipMemcpyDeviceToHost), "reading stats");
    return RT_OK;
}

/* test hook: the cull plane the last render launch of the context was handed, read back (waits for the device).  info4 = {1 if that launch
 * was handed a plane else 0, the plane's image width, its height, its words}; with words == NULL or too small a capacity only info4 is written */
extern "C" rt_status rt_debug_primary_cull(rt_ctx *ctx, uint32_t *words, int32_t capacity_words, int32_t *info4)
{
    if (!ctx || !info4 || capacity_words < 0) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    const CullPlane &cp = ctx->cull;
    const bool have = cp.plan.valid && cp.plan.used_last && cp.d.p;
    const size_t n = have ? rt_cull_words(cp.plan.key.width, cp.plan.key.height) : 0;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? cp.plan.key.width : 0;
    info4[2] = have ? cp.plan.key.height : 0;
    info4[3] = (int32_t)n;
    if (!have || !words || (size_t)capacity_words < n) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for the device");
    RT_HIP(ctx, hipMemcpy(words, cp.d.p, n * 4, hipMemcpyDeviceToHost), "reading the cull plane");
    return RT_OK;
}

/* test hook: the subtree cull's gate words (rt_cull.h) the last render launch of the context was handed, one per pixel, read back (waits for
 * the device).  info4 as rt_debug_primary_cull's, with the pixel count as the words */
extern "C" rt_status rt_debug_subtree_cull(rt_ctx *ctx, uint32_t *words, int32_t capacity_words, int32_t *info4)
{
    if (!ctx || !info4 || capacity_words < 0) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    const CullPlane &cp = ctx->cull;
    const bool have = cp.plan.valid && cp.plan.used_last && cp.d.p;
    const size_t n = have ? (size_t)cp.plan.key.width * (size_t)cp.plan.key.height : 0;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? cp.plan.key.width : 0;
    info4[2] = have ? cp.plan.key.height : 0;
    info4[3] = (int32_t)n;
    if (!have || !words || (size_t)capacity_words < n) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for the device");
    RT_HIP(ctx, hipMemcpy(words, cp.d.p + rt_cull_words(cp.plan.key.width, cp.plan.key.height), n * 4, hipMemcpyDeviceToHost), "reading the gate words");
    return RT_OK;
}

/* test hook: the primary entry words (rt_entry.h) the last render launch of the context was handed, one per pixel, read back (waits for the
 * device).  info4 as rt_debug_subtree_cull's */
extern "C" rt_status rt_debug_primary_entry(rt_ctx *ctx, uint32_t *words, int32_t capacity_words, int32_t *info4)
{
    if (!ctx || !info4 || capacity_words < 0) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    const CullPlane &cp = ctx->cull;
    const bool have = cp.plan.valid && cp.plan.used_last && cp.d.p;
    const size_t n = have ? (size_t)cp.plan.key.width * (size_t)cp.plan.key.height : 0;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? cp.plan.key.width : 0;
    info4[2] = have ? cp.plan.key.height : 0;
    info4[3] = (int32_t)n;
    if (!have || !words || (size_t)capacity_words < n) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for the device");
    RT_HIP(ctx, hipMemcpy(words, cp.d.p + rt_cull_entry_base(rt_cull_words(cp.plan.key.width, cp.plan.key.height)), n * 4, hipMemcpyDeviceToHost), "reading the entry words");
    /* (a pixel with a sub-entry table carries its slot here: its own word is 0, and rt_debug_primary_subentry has its table) */
    for (size_t i = 0; i < n; i++)
        if (rt_sub_slot_plus1(words[i]) != 0u) words[i] = 0u;
    return RT_OK;
}

/* test hook: the sub-entry tables (rt_entry.h) the last render launch of the context was handed, read back (waits for the device) and keyed
 * by pixel, in ascending order of the pixel: pixels[i] = py * width + px, words[64 * i + idx] its sub-word of sub-box idx.  info4 = {1 if
 * that launch was handed a plane whose view is refined else 0, the image's width, its height, the tables in use}; with pixels or words NULL
 * or too small a capacity only info4 is written */
extern "C" rt_status rt_debug_primary_subentry(rt_ctx *ctx, uint32_t *pixels, uint32_t *words, int32_t capacity_tables, int32_t *info4)
{
    if (!ctx || !info4 || capacity_tables < 0) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    const CullPlane &cp = ctx->cull;
    const bool have = cp.plan.valid && cp.plan.used_last && cp.d.p && cp.plan.tables && cp.plan.refined;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? cp.plan.key.width : 0;
    info4[2] = have ? cp.plan.key.height : 0;
    info4[3] = 0;
    if (!have) return RT_OK;
    const size_t pw = rt_cull_words(cp.plan.key.width, cp.plan.key.height);
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, hipDeviceSynchronize(), "waiting for the device");
    uint32_t counter = 0;
    RT_HIP(ctx, hipMemcpy(&counter, cp.d.p + rt_sub_header_base(pw), 4, hipMemcpyDeviceToHost), "reading the slot counter");
    const size_t n = (size_t)counter < rt_sub_cap(pw) ? (size_t)counter : rt_sub_cap(pw);
    info4[3] = (int32_t)n;
    if (!pixels || !words || (size_t)capacity_tables < n || n == 0) return RT_OK;
    std::vector<uint32_t> by_slot(n), table(n * RT_SUB_WORDS), order(n);
    RT_HIP(ctx, hipMemcpy(by_slot.data(), cp.d.p + rt_sub_pixels_base(pw), n * 4, hipMemcpyDeviceToHost), "reading the slots' pixels");
    RT_HIP(ctx, hipMemcpy(table.data(), cp.d.p + rt_sub_tables_base(pw), n * RT_SUB_WORDS * 4, hipMemcpyDeviceToHost), "reading the sub-entry tables");
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return by_slot[x] < by_slot[y]; });
    for (size_t i = 0; i < n; i++) {
        pixels[i] = by_slot[order[i]];
        for (size_t k = 0; k < RT_SUB_WORDS; k++) words[i * RT_SUB_WORDS + k] = rt_sub_word_of(table[(size_t)order[i] * RT_SUB_WORDS + k]);   /* (as stored: rt_entry.h) */
    }
    return RT_OK;
}

/* test / development hook, host only (no device is touched): the sub-entry tables of `cam`'s image on a flattened scene as the refinement
 * writes them, keyed by pixel in ascending order.  cap < 0: the image's own (rt_sub_cap); else at most `cap` pixels get a table, the first
 * in pixel order (the device hands its slots out in no particular order).  pixels / words as rt_debug_primary_subentry's, for at most
 * capacity_tables tables (NULL: only the statistics).  stats8, or NULL: {pixels that want a table, tables handed out, sub-words `triangle`,
 * `nothing`, not known, the table pixels' centre-ray gated node steps summed over their resolved sub-boxes, the same over all 64, 0} - what
 * tools/primary_cull_estimate.py prints.  A view without jitter or a scene of several meshes has no tables. */
extern "C" rt_status rt_debug_primary_subentry_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, int32_t cap, uint32_t *pixels, uint32_t *words,
                                                    int32_t capacity_tables, int64_t *stats8)
{
    if (!view || !cam || !view->blob || cam->width <= 0 || cam->height <= 0 || (int64_t)cam->width * cam->height > (1 << 28) || capacity_tables < 0) return RT_ERR_INVALID;
    float c12[12];
    camera_floats(*cam, c12);
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t limit = cap < 0 ? rt_sub_cap(rt_cull_words(cam->width, cam->height)) : (size_t)cap;
    const bool one = view->num_meshes == 1 && antialias;
    for (int py = 0; one && py < cam->height; py++)
        for (int px = 0; px < cam->width; px++) {
            float P[3];
            rt_cull_primary(c12, px, py, P);
            const rt_cull_cone cone = rt_cull_cone_of(P, c12, 1);
            const bool flagged = rt_cull_no_leaf(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 1, rt_cull_local_stack());
            const uint32_t word = rt_entry_word(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, view->off_tris, view->num_triangles, rt_cull_local_stack(),
                                                rt_cull_local_stack());
            if (!rt_sub_wants_table(flagged, word)) continue;
            st[0]++;
            if ((size_t)st[1] >= limit) continue;
            const size_t slot = (size_t)st[1]++;
            const uint32_t gates = rt_cull_gate_word(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, rt_cull_local_stack());
            const float inv[3] = {1.0f / P[0], 1.0f / P[1], 1.0f / P[2]};
            int64_t steps = rt_cull_walk_steps(view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, c12, P, inv, gates);
            if (steps < 0) steps = 0;
            const bool keep = pixels && words && slot < (size_t)capacity_tables;
            if (keep) pixels[slot] = (uint32_t)((size_t)py * (size_t)cam->width + (size_t)px);
            for (uint32_t idx = 0; idx < RT_SUB_WORDS; idx++) {
                const uint32_t w = rt_entry_word(rt_sub_cone_of(P, c12, idx), view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, view->off_tris, view->num_triangles,
                                                 rt_cull_local_stack(), rt_cull_local_stack());
                if (keep) words[slot * RT_SUB_WORDS + idx] = w;
                st[(w & RT_ENTRY_TAG) ? 2 : (w == RT_ENTRY_NOTHING ? 3 : 4)]++;
                if (w != 0u) st[5] += steps;
                st[6] += steps;
            }
        }
    if (stats8) std::memcpy(stats8, st, sizeof st);
    return RT_OK;
}

/* test / development hook, host only (no device is touched): rt_entry_word per pixel of `cam`'s image on a flattened scene, as the pre-pass
 * writes it (0 everywhere unless the scene has exactly one mesh).  words: width * height, or NULL.  stats12, or NULL: over the unflagged
 * pixels whose cone may enter the root box, by class of the word - `triangle`, `nothing`, 0 - {pixels x 3, the centre ray's node steps x 3,
 * its triangle tests x 3} walked in the render kernel's order with the pixel's gate word and the kernel's float tests, then {triangles
 * the predicate classified, 0, 0} - what tools/primary_cull_estimate.py prints. */
extern "C" rt_status rt_debug_primary_entry_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, uint32_t *words, int64_t *stats12)
{
    if (!view || !cam || !view->blob || cam->width <= 0 || cam->height <= 0 || (int64_t)cam->width * cam->height > (1 << 28)) return RT_ERR_INVALID;
    float c12[12];
    camera_floats(*cam, c12);
    int64_t st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool one = view->num_meshes == 1;
    for (int py = 0; py < cam->height; py++)
        for (int px = 0; px < cam->width; px++) {
            float P[3];
            rt_cull_primary(c12, px, py, P);
            const rt_cull_cone cone = rt_cull_cone_of(P, c12, antialias);
            const uint32_t word = one ? rt_entry_word(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, view->off_tris, view->num_triangles,
                                                      rt_cull_local_stack(), rt_cull_local_stack(), &st[9]) : 0u;
            if (words) words[(size_t)py * (size_t)cam->width + (size_t)px] = word;
            if (!one) continue;
            const float *m0 = view->blob + 4 * (size_t)view->off_meshes;
            if (rt_cull_box_missed(cone, m0[0], m0[1], m0[2], m0[3], m0[4], m0[5])) continue;
            if (rt_cull_no_leaf(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 1, rt_cull_local_stack())) continue;
            const uint32_t gates = rt_cull_gate_word(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, rt_cull_local_stack());
            const float inv[3] = {1.0f / P[0], 1.0f / P[1], 1.0f / P[2]};
            const int cls = (word & RT_ENTRY_TAG) ? 0 : (word == RT_ENTRY_NOTHING ? 1 : 2);
            float best; int32_t prim;
            int64_t tests = 0;
            const int64_t steps = rt_cull_walk(view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, c12, P, inv, gates, best, prim,
                                               rt_entry_leaf_tests{view->blob + 4 * (size_t)view->off_tris, c12, P, &tests});
            st[cls]++;
            st[3 + cls] += steps > 0 ? steps : 0;
            st[6 + cls] += tests;
        }
    if (stats12) std::memcpy(stats12, st, sizeof st);
    return RT_OK;
}

/* test / development hook, host only (no device is touched): rt_cull_gate_word per pixel of `cam`'s image on a flattened scene, as the
 * pre-pass writes it (0 everywhere unless the scene has exactly one mesh; a pixel the bit plane flags has every gate dead).  words: width * height, or NULL.
 * stats4, or NULL: over the unflagged pixels whose cone may enter the root box, the centre ray's walk in the render kernel's order (far
 * child first, the pop rule, the med3 or the min / max slab form as the kernel picks it; no triangle is tested, so `best` stays infinite
 * and this counts at least the steps of the real traversal) - {those pixels, its node steps ungated, its node steps with the pixel's word,
 * pixels whose word is not 0} - what tools/primary_cull_estimate.py prints. */
extern "C" rt_status rt_debug_subtree_cull_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, uint32_t *words, int64_t *stats4)
{
    if (!view || !cam || !view->blob || cam->width <= 0 || cam->height <= 0 || (int64_t)cam->width * cam->height > (1 << 28)) return RT_ERR_INVALID;
    float c12[12];
    camera_floats(*cam, c12);
    int64_t st[4] = {0, 0, 0, 0};
    for (int py = 0; py < cam->height; py++)
        for (int px = 0; px < cam->width; px++) {
            float P[3];
            rt_cull_primary(c12, px, py, P);
            const rt_cull_cone cone = rt_cull_cone_of(P, c12, antialias);
            const bool flagged = rt_cull_no_leaf(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, view->num_meshes, rt_cull_local_stack());
            const uint32_t word = view->num_meshes == 1 ? rt_cull_gate_word(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, rt_cull_local_stack()) : 0u;
            if (words) words[(size_t)py * (size_t)cam->width + (size_t)px] = word;
            if (flagged || view->num_meshes != 1) continue;
            const float *m0 = view->blob + 4 * (size_t)view->off_meshes;
            if (rt_cull_box_missed(cone, m0[0], m0[1], m0[2], m0[3], m0[4], m0[5])) continue;
            const float inv[3] = {1.0f / P[0], 1.0f / P[1], 1.0f / P[2]};
            st[0]++;
            st[1] += rt_cull_walk_steps(view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, c12, P, inv, 0u);
            st[2] += rt_cull_walk_steps(view->blob, view->off_nodes, view->num_nodes, view->off_meshes, 0, c12, P, inv, word);
            st[3] += word != 0u;
        }
    if (stats4) std::memcpy(stats4, st, sizeof st);
    return RT_OK;
}

/* test / development hook, host only (no device is touched): the predicate of rt_cull.h evaluated per pixel of `cam`'s image on a flattened
 * scene (rt_debug_flatten's view, or rt_debug_scene_read's).  words: rt_cull_words-many, or NULL.  stats6, or NULL: {pixels whose cone may
 * enter some mesh's root box, those of them that are flagged, nodes the centre direction's walk visits in flagged pixels, ... in all
 * root-entering pixels, pixels flagged in all, words of the plane} - what tools/primary_cull_estimate.py prints. */
extern "C" rt_status rt_debug_primary_cull_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, uint32_t *words, int64_t *stats6)
{
    if (!view || !cam || !view->blob || cam->width <= 0 || cam->height <= 0 || (int64_t)cam->width * cam->height > (1 << 28)) return RT_ERR_INVALID;
    float c12[12];
    camera_floats(*cam, c12);
    const size_t n_words = rt_cull_words(cam->width, cam->height);
    if (words) std::memset(words, 0, n_words * 4);
    int64_t st[6] = {0, 0, 0, 0, 0, (int64_t)n_words};
    for (int py = 0; py < cam->height; py++)
        for (int px = 0; px < cam->width; px++) {
            float P[3];
            rt_cull_primary(c12, px, py, P);
            const rt_cull_cone cone = rt_cull_cone_of(P, c12, antialias);
            const bool flagged = rt_cull_no_leaf(cone, view->blob, view->off_nodes, view->num_nodes, view->off_meshes, view->num_meshes, rt_cull_local_stack());
            const size_t pixel = (size_t)py * (size_t)cam->width + (size_t)px;
            if (flagged && words) words[pixel >> 5] |= 1u << (pixel & 31);
            st[4] += flagged;
            bool enters = false;
            for (int32_t m = 0; m < view->num_meshes && !enters; m++) {
                const float *m0 = view->blob + 4 * ((size_t)view->off_meshes + 2 * (size_t)m);
                enters = !rt_cull_box_missed(cone, m0[0], m0[1], m0[2], m0[3], m0[4], m0[5]);
            }
            if (!enters) continue;
            /* what the pixel's centre ray walks: the single direction P, every node whose box it may enter */
            int32_t steps = 0;
            (void)rt_cull_no_leaf(rt_cull_cone_of(P, c12, 0), view->blob, view->off_nodes, view->num_nodes, view->off_meshes, view->num_meshes, rt_cull_local_stack(), &steps, false);
            st[0]++;
            st[1] += flagged;
            st[2] += flagged ? steps : 0;
            st[3] += steps;
        }
    if (stats6) std::memcpy(stats6, st, sizeof st);
    return RT_OK;
}

extern "C" rt_status rt_last_kernel_ms(rt_ctx *ctx, float *ms)
{
    if (!ctx || !ms) return RT_ERR_INVALID;
    if (!ctx->have_timing) return set_err(ctx, RT_ERR_INVALID, "no render has been launched yet");
    RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for render kernel");
    RT_HIP(ctx, hipEventElapsedTime(ms, ctx->ev_start, ctx->ev_stop), "reading kernel time");
    return RT_OK;
}

/* the host has the frame once the device is idle */
static rt_status wait_for_device(rt_ctx *ctx)
{
    RT_HIP(ctx, hipDeviceSynchronize(), "render kernel");
    return RT_OK;
}

extern "C" rt_status rt_render(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                               int32_t time_ms, int32_t *frame_num, float *previous_render)
{
    return host_round_trip(ctx, cam, 1, frame_num, previous_render, &rt_ctx::d_prev, [&](size_t) -> rt_status {
        const rt_status st = rt_render_device(ctx, scene, cam, rs, time_ms, *frame_num, nullptr, ctx->d_prev.p, ctx->d_out.p, nullptr);
        return st != RT_OK ? st : wait_for_device(ctx);
    });
}

/* the same for n_frames consecutive frames at once (seeds times_ms[i]): one multi-frame launch per
 * rt_max_batch_frames frames; *frame_num advances by n_frames */
extern "C" rt_status rt_render_frames(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                      const int32_t *times_ms, int32_t n_frames, int32_t *frame_num, float *previous_render)
{
    if (!times_ms || n_frames < 1) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return host_round_trip(ctx, cam, n_frames, frame_num, previous_render, &rt_ctx::d_out, [&](size_t bytes) -> rt_status {
        const int32_t cap = batch_cap(ctx, bytes / 4);
        for (int32_t done = 0; done < n_frames;) {
            const int32_t k = n_frames - done < cap ? n_frames - done : cap;
            const rt_status st = rt_render_device_batch(ctx, scene, cam, rs, times_ms + done, k, *frame_num + done, nullptr, ctx->d_out.p, nullptr);
            if (st != RT_OK) return st;
            done += k;
        }
        return wait_for_device(ctx);
    });
}

/* waits for the most recent launch of this context */
extern "C" rt_status rt_ctx_synchronize(rt_ctx *ctx)
{
    if (!ctx) return RT_ERR_INVALID;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    {
        rt_status st = drain_pipeline(ctx, true);
        if (st != RT_OK) return st;
    }
    if (!ctx->launched) return RT_OK;
    RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for render kernel");
    return RT_OK;
}

extern "C" rt_status rt_to_rgba8_device(rt_ctx *ctx, const float *d_rgb, int32_t width, int32_t height, uint8_t *d_rgba, void *hip_stream)
{
    if (!ctx || !d_rgb || !d_rgba || width <= 0 || height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, rt_launch_rgba8(d_rgb, width * height, d_rgba, (hipStream_t)hip_stream), "launching rgba8 kernel");
    return RT_OK;
}
