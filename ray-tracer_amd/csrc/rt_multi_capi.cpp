/*
 * rt_multi_capi.cpp — tile ownership over GPUs and the multi-GPU entry points (include/rt_amd.h: rt_partition_tiles,
 * rt_peer_access, rt_gather, rt_render_multi[_device]).  A context's state as a rank is rt_ctx::multi (MultiRank, rt_internal.h);
 * the ranks' launches are rt_render_device_batch calls (rt_capi.cpp).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <queue>
#include <vector>

#include "rt_internal.h"

/* Longest-processing-time-first ownership (see include/rt_amd.h) */
extern "C" rt_status rt_partition_tiles(const uint32_t *cost, int32_t tiles_x, int32_t tiles_y, int32_t n_ranks, int32_t *owner)
{
    if (!owner || tiles_x <= 0 || tiles_y <= 0 || n_ranks <= 0 || (int64_t)tiles_x * tiles_y > (int64_t)RT_JOB_TILE_MASK + 1) return RT_ERR_INVALID;
    const int n = tiles_x * tiles_y;
    if (!cost) {
        for (int ty = 0; ty < tiles_y; ty++)
            for (int tx = 0; tx < tiles_x; tx++) owner[ty * tiles_x + tx] = (tx + ty) % n_ranks;
        return RT_OK;
    }
    std::vector<uint32_t> idx((size_t)n);
    for (int i = 0; i < n; i++) idx[(size_t)i] = (uint32_t)i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
    /* (load, rank): the least loaded rank first, the lower rank on a tie */
    typedef std::pair<uint64_t, int> LR;
    std::priority_queue<LR, std::vector<LR>, std::greater<LR>> heap;
    for (int r = 0; r < n_ranks; r++) heap.push(LR(0, r));
    for (uint32_t t : idx) {
        LR top = heap.top();
        heap.pop();
        owner[t] = top.second;
        top.first += cost[t];
        heap.push(top);
    }
    return RT_OK;
}

/* =============================================================================================
 * Multi-GPU from one host thread (SURVEY.md §8(b) "rt_gather", §8(e)): every rank renders the tiles it
 * owns on its own GPU into a compact buffer; the buffers travel to the root's GPU with one peer copy per
 * rank (xGMI) and are de-interleaved there.  No collective is needed: nothing is reduced, every pixel has
 * one owner.  Ownership is either static (bands: rank i owns the bands b % n == i) or cost-balanced (tile
 * lists dealt longest-processing-time-first from the costs the view's first launch measures).
 * ============================================================================================= */
namespace {

/* A compact image of layout L and the width x height frame, both on the current device: the image into the frame (to_frame) or
 * out of it.  A list's tiles go through rt_launch_tiles_copy (d_tile_list: the list on this device); bands through one 2D copy
 * of the whole bands and one of the valid rows of a ragged last band (only those exist in the frame). */
hipError_t exchange(const rt_sched::Layout &L, float *compact, float *frame, bool to_frame, const uint32_t *d_tile_list, hipStream_t stream)
{
    if (L.listed) return rt_launch_tiles_copy(compact, frame, d_tile_list, L.num_tiles, L.tiles_x, L.width, L.height, to_frame ? 1 : 0, stream);
    const int nb = L.owned_bands(), whole = L.whole_bands();
    const size_t chunk_bytes = L.band_floats() * 4, frame_pitch = chunk_bytes * (size_t)L.band_stride;
    float *frame0 = frame + (size_t)L.band_first * L.band_floats();
    hipError_t e = hipSuccess;
    if (whole > 0) {
        e = to_frame ? hipMemcpy2DAsync(frame0, frame_pitch, compact, chunk_bytes, chunk_bytes, (size_t)whole, hipMemcpyDeviceToDevice, stream)
                     : hipMemcpy2DAsync(compact, chunk_bytes, frame0, frame_pitch, chunk_bytes, (size_t)whole, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
    }
    if (whole < nb) {
        const int b = L.band(nb - 1);
        const size_t bytes = (size_t)L.rows_of(b) * (size_t)L.width * 12;
        float *f = frame + (size_t)b * L.band_floats(), *c = compact + (size_t)(nb - 1) * L.band_floats();
        e = to_frame ? hipMemcpyAsync(f, c, bytes, hipMemcpyDeviceToDevice, stream) : hipMemcpyAsync(c, f, bytes, hipMemcpyDeviceToDevice, stream);
    }
    return e;
}

rt_status multi_prepare(rt_ctx *ctx)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    if (!ctx->multi.stream) RT_HIP(ctx, hipStreamCreateWithFlags(&ctx->multi.stream.s, hipStreamNonBlocking), "creating the rank's stream");
    if (!ctx->multi.ev) RT_HIP(ctx, hipEventCreateWithFlags(&ctx->multi.ev.e, hipEventDisableTiming), "creating the rank's event");
    return RT_OK;
}

/* device-to-device bytes between two contexts' GPUs (a plain copy when they share one), on a stream of
 * the CURRENT device */
hipError_t copy_between(float *dst, int dst_dev, const float *src, int src_dev, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return hipSuccess;
    if (dst_dev == src_dev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream);
    return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream);
}

/* The root's landing area for src's compact image, at least `need` floats, ready to be written in the order of `s0`:
 * s0 has been made to wait for the last de-interleave that read it (which may have been queued on another stream
 * of the root by an earlier call).  Leaves the root's device current. */
rt_status stage_for(rt_ctx *root, rt_ctx *src, size_t need, hipStream_t s0, Stage **out)
{
    RT_HIP(root, hipSetDevice(root->device), "selecting device");
    /* rt_ctx_destroy of a source erases its entry from every live root's map under g_ctx_mutex: look the
     * entry up under the same lock.  (std::map nodes do not move: the reference stays valid while src is alive.) */
    Stage *sgp;
    { std::lock_guard<std::mutex> lock(g_ctx_mutex); sgp = &root->multi.stages[src]; }
    Stage &sg = *sgp;
    if (!sg.ev_free) RT_HIP(root, hipEventCreateWithFlags(&sg.ev_free.e, hipEventDisableTiming), "creating the staging event");
    if (sg.d.cap < need || !sg.d.p) {
        /* nothing may still be reading or writing the old area */
        if (sg.used) RT_HIP(root, hipEventSynchronize(sg.ev_free), "waiting for the staging area");
        if (src->multi.stream) { (void)hipSetDevice(src->device); (void)hipStreamSynchronize(src->multi.stream); (void)hipSetDevice(root->device); }
        RT_HIP(root, sg.d.grow(need), "allocating the gather staging area");
        sg.used = false;
    }
    if (sg.used) RT_HIP(root, hipStreamWaitEvent(s0, sg.ev_free, 0), "ordering behind the previous de-interleave");
    *out = &sg;
    return RT_OK;
}

int peer_access(rt_ctx *a, rt_ctx *b)
{
    if (a->device == b->device) return 1;
    auto it = a->multi.peer_ok.find(b->device);
    if (it != a->multi.peer_ok.end()) return it->second;
    int ok = 1;
    for (int dir = 0; dir < 2; dir++) {
        const int from = dir ? b->device : a->device, to = dir ? a->device : b->device;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, from, to) != hipSuccess || !can) { ok = 0; continue; }
        if (hipSetDevice(from) != hipSuccess) { ok = 0; continue; }
        const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) ok = 0;
    }
    (void)hipGetLastError();           /* "already enabled" must not surface as a later launch error */
    (void)hipSetDevice(a->device);
    a->multi.peer_ok[b->device] = ok;
    b->multi.peer_ok[a->device] = ok;
    return ok;
}

}  // namespace

extern "C" int32_t rt_peer_access(rt_ctx *a, rt_ctx *b)
{
    if (!a || !b) return -RT_ERR_INVALID;
    return peer_access(a, b);
}

/* The exchange step alone: the compact buffer `d_bands` of the rank described by `src_tiles`
 * (on src's GPU) lands in the full frame `d_frame` on root's GPU.  Ordered behind src's most recent
 * launch; the frame is complete in `root_stream` order. */
extern "C" rt_status rt_gather(rt_ctx *root, float *d_frame, int32_t width, int32_t height, rt_ctx *src, const float *d_bands,
                               const rt_tile_spec *src_tiles, void *root_stream)
{
    if (!root || !src || !d_frame || !d_bands || !src_tiles) return set_err(root, RT_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0) return set_err(root, RT_ERR_INVALID, "bad image size");
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (const char *bad = rt_sched::tile_spec_error(*src_tiles, tiles_x, tiles_y)) return set_err(root, RT_ERR_INVALID, bad);
    if (src_tiles->tile_list && !rt_sched::tiles_in_image(src_tiles->tile_list, src_tiles->num_tiles, tiles_x, tiles_y))
        return set_err(root, RT_ERR_INVALID, "a tile index outside the image");
    const rt_sched::Layout L(*src_tiles, width, height);
    rt_status st = multi_prepare(root);
    if (st != RT_OK) return st;
    hipStream_t s0 = (hipStream_t)root_stream;
    float *from = const_cast<float *>(d_bands);
    Stage *sg = nullptr;
    if (src->device != root->device) {
        /* one peer copy of the whole compact buffer into the root's staging area for this source: behind src's last
         * launch, and behind the de-interleave of the PREVIOUS gather from this source, which reads the same area on the
         * root's stream (src may be a frame ahead of the root) */
        if ((st = multi_prepare(src)) != RT_OK) return set_err(root, st, rt_last_error(src));
        (void)peer_access(src, root);
        if ((st = stage_for(root, src, L.compact_floats(), s0, &sg)) != RT_OK) return st;
        RT_HIP(src, hipSetDevice(src->device), "selecting device");
        if (sg->used) RT_HIP(src, hipStreamWaitEvent(src->multi.stream, sg->ev_free, 0), "ordering the copy behind the previous de-interleave");
        if (src->launched) RT_HIP(src, hipStreamWaitEvent(src->multi.stream, src->ev_stop, 0), "ordering the gather behind the render");
        RT_HIP(src, copy_between(sg->d.p, root->device, d_bands, src->device, L.compact_floats() * 4, src->multi.stream), "copying the rank's image to the root GPU");
        RT_HIP(src, hipEventRecord(src->multi.ev, src->multi.stream), "recording the gather event");
        RT_HIP(root, hipSetDevice(root->device), "selecting device");
        RT_HIP(root, hipStreamWaitEvent(s0, src->multi.ev, 0), "ordering the de-interleave behind the copy");
        from = sg->d.p;
    } else {
        RT_HIP(root, hipSetDevice(root->device), "selecting device");
        if (src->launched) RT_HIP(root, hipStreamWaitEvent(s0, src->ev_stop, 0), "ordering the gather behind the render");
    }
    const uint32_t *d_list = nullptr;
    if (L.listed && (st = root->tile_lists.on_device(root, src_tiles->tile_list, L.num_tiles, s0, &d_list)) != RT_OK) return st;
    RT_HIP(root, exchange(L, from, d_frame, true, d_list, s0), L.listed ? "de-interleaving tiles" : "de-interleaving bands");
    if (sg) {
        RT_HIP(root, hipEventRecord(sg->ev_free, s0), "recording the staging event");
        sg->used = true;
    }
    return RT_OK;
}

namespace {

/* what rank i of a multi-GPU call renders and where its image lives */
struct RankPlan {
    rt_ctx *c = nullptr;
    const rt_scene *scene = nullptr;
    rt_tile_spec spec;
    rt_sched::Layout layout;             /* compact: the rank's bands, or its tile list */
    const uint32_t *root_list = nullptr; /* tile lists: the rank's list on the ROOT's GPU (for the copies to and from the frame) */
    Stage *stage = nullptr;              /* the root's landing area for the rank's image */
};

/* the arguments; then every rank's stream and event, and direct xGMI copies to and from the root where the platform allows
 * (instead of staging through the host).  Leaves the root's device current. */
rt_status check_and_ready(rt_ctx *root, const std::vector<RankPlan> &plan, const rt_camera *cam, const rt_render_settings *rs, const int32_t *times_ms,
                          int32_t n_frames, int32_t frame_num, int32_t band_rows, const float *d_frame)
{
    if (!cam || !rs || !times_ms || !d_frame || n_frames < 1 || frame_num < 0) return set_err(root, RT_ERR_INVALID, "null argument");
    if (cam->width <= 0 || cam->height <= 0 || band_rows < 0 || (band_rows & 7)) return set_err(root, RT_ERR_INVALID, "bad image size or band_rows (0, or a positive multiple of 8)");
    for (size_t i = 0; i < plan.size(); i++) {
        if (!plan[i].c || !plan[i].scene || plan[i].scene->ctx != plan[i].c) return set_err(root, RT_ERR_INVALID, "rank without a context, or a scene committed on another context");
        for (size_t j = 0; j < i; j++) if (plan[j].c == plan[i].c) return set_err(root, RT_ERR_INVALID, "a context may appear once (its launch scratch is not shared between ranks)");
    }
    rt_status st;
    if ((st = multi_prepare(root)) != RT_OK) return st;
    for (const RankPlan &p : plan) {
        if ((st = multi_prepare(p.c)) != RT_OK) return set_err(root, st, rt_last_error(p.c));
        (void)peer_access(p.c, root);
    }
    RT_HIP(root, hipSetDevice(root->device), "selecting device");
    return RT_OK;
}

/* Cost-balanced ownership of the tiles, in root->multi.state.  A new view is dealt out interleaved, and the calls on it measure what
 * the tiles cost until one has done so.  The call after that collects every rank's figures (this waits for those launches,
 * which the caller has normally consumed already) and deals the tiles out again by cost.  All read-backs happen here,
 * before any rank is launched, so no rank's launch waits on another rank's kernel. */
rt_status balance(rt_ctx *root, const std::vector<RankPlan> &plan, const rt_camera *cam, const rt_render_settings *rs)
{
    MultiState &ms = root->multi.state;
    const int n = (int)plan.size(), tiles_x = (cam->width + 7) / 8, tiles_y = (cam->height + 7) / 8;
    /* (the bounce limit, and preview (< 8 samples) or real: ownership measured on the one says little about the other) */
    std::vector<uint32_t> key;
    push_camera(key, cam);
    key.push_back((uint32_t)cam->width); key.push_back((uint32_t)cam->height); key.push_back((uint32_t)n);
    key.push_back((uint32_t)rs->reflection_limit); key.push_back(rs->rays_per_pixel < 8 ? 0u : 1u);
    for (const RankPlan &p : plan) { key.push_back(p.scene->uid); key.push_back((uint32_t)p.c->device); }
    std::vector<int32_t> owner((size_t)tiles_x * tiles_y);
    rt_status st;
    if (key != ms.key || ms.lists.size() != (size_t)n) {
        if ((st = rt_partition_tiles(nullptr, tiles_x, tiles_y, n, owner.data())) != RT_OK) return set_err(root, st, "cannot partition the image");
        rt_sched::deal_tiles(owner, n, nullptr, nullptr, ms.lists, ms.costs, ms.peaks);
        ms.key = key;
        ms.owners = Owners::interleaved;
    } else if (ms.owners == Owners::measured) {
        std::vector<uint32_t> cost(owner.size(), 0u), peak(owner.size(), 0u);
        bool have_all = true;
        for (size_t i = 0; i < plan.size() && have_all; i++) {
            const std::vector<uint32_t> &list = ms.lists[i];
            if (list.empty()) continue;
            std::vector<uint32_t> ids(list.size()), cs(list.size()), ps(list.size());
            int32_t got = 0;
            have_all = rt_tile_costs(plan[i].c, ids.data(), cs.data(), ps.data(), (int32_t)list.size(), &got) == RT_OK && (size_t)got == list.size() && ids == list;
            for (size_t k = 0; k < list.size() && have_all; k++) { cost[ids[k]] = cs[k]; peak[ids[k]] = ps[k]; }
        }
        RT_HIP(root, hipSetDevice(root->device), "selecting device");
        if (!have_all) { ms.owners = Owners::interleaved; return RT_OK; }    /* (a rank's context has rendered another view since: measure again) */
        if ((st = rt_partition_tiles(cost.data(), tiles_x, tiles_y, n, owner.data())) != RT_OK) return set_err(root, st, "cannot partition the image");
        rt_sched::deal_tiles(owner, n, cost.data(), peak.data(), ms.lists, ms.costs, ms.peaks);
        ms.owners = Owners::balanced;
    }
    return RT_OK;
}

/* who renders what, each rank into a compact image (a tile list goes to the root's GPU as well) */
rt_status plan_ranks(rt_ctx *root, std::vector<RankPlan> &plan, const rt_camera *cam, const rt_render_settings *rs, int32_t band_rows, hipStream_t s0)
{
    const bool listed = band_rows == 0;
    rt_status st;
    if (listed && (st = balance(root, plan, cam, rs)) != RT_OK) return st;
    const MultiState &ms = root->multi.state;
    for (size_t i = 0; i < plan.size(); i++) {
        RankPlan &p = plan[i];
        std::memset(&p.spec, 0, sizeof p.spec);
        p.spec.compact = 1;
        if (listed) {
            const bool costed = ms.owners == Owners::balanced && !ms.lists[i].empty();
            static const uint32_t none = 0;      /* (an empty vector's data() may be null, which would read as "no list") */
            p.spec.tile_list = ms.lists[i].empty() ? &none : ms.lists[i].data();
            p.spec.num_tiles = (int32_t)ms.lists[i].size();
            p.spec.tile_cost = costed ? ms.costs[i].data() : nullptr;
            p.spec.tile_peak = costed ? ms.peaks[i].data() : nullptr;
        } else {
            p.spec.band_rows = band_rows; p.spec.band_first = (int32_t)i; p.spec.band_stride = (int32_t)plan.size();
        }
        p.layout = rt_sched::Layout(p.spec, cam->width, cam->height);
        if (listed && (st = root->tile_lists.on_device(root, p.spec.tile_list, p.spec.num_tiles, s0, &p.root_list)) != RT_OK) return st;
    }
    return RT_OK;
}

/* RT_AMD_MULTI_CAREFUL=1 (diagnosis): the host waits for every stream involved after each phase, so that no ordering between
 * devices rests on an event - if a frame is wrong or a call hangs in the asynchronous form but not in this one, the
 * fault is in the event choreography, otherwise in the copies themselves; an error names the phase it was found in.
 * bench.py's capi_multi leg falls back to it by itself (this path has never run on two physical GPUs). */
rt_status careful(rt_ctx *root, const std::vector<RankPlan> &plan, hipStream_t s0, const char *phase)
{
    if (!root->multi.careful) return RT_OK;
    for (const RankPlan &p : plan) {
        hipError_t e = hipSetDevice(p.c->device);
        if (e == hipSuccess) e = hipStreamSynchronize(p.c->multi.stream);
        if (e != hipSuccess) { (void)hipSetDevice(root->device); return hip_fail(root, e, phase); }
    }
    hipError_t e = hipSetDevice(root->device);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    if (e != hipSuccess) return hip_fail(root, e, phase);
    return RT_OK;
}

/* The ranks' buffers, then their images travel and are rendered, in three phases.  (root->multi.ev is recorded twice: in the
 * first phase, on the caller's stream, as "the ranks may start", and in the second on rank 0's stream as "rank 0's image is
 * in the staging area"; a hipStreamWaitEvent captures the record that precedes it, and the calls are in that order.) */
rt_status render_ranks(rt_ctx *root, std::vector<RankPlan> &plan, const rt_camera *cam, const rt_render_settings *rs, const int32_t *times_ms,
                       int32_t n_frames, int32_t frame_num, float *d_frame, hipStream_t s0)
{
    /* ---- every rank's compact image on its GPU, and a landing area per rank on the root's */
    rt_status st;
    for (RankPlan &p : plan) {
        const size_t floats = p.layout.compact_floats();
        if (p.c->multi.d_bands.cap < floats || !p.c->multi.d_bands.p) {
            RT_HIP(p.c, hipSetDevice(p.c->device), "selecting device");
            RT_HIP(p.c, hipStreamSynchronize(p.c->multi.stream), "waiting for the rank's image buffer");
            if (hipError_t e = p.c->multi.d_bands.grow(floats)) return set_err(root, hip_fail(p.c, e, "allocating the rank's image buffer"), p.c->err);
        }
        if ((st = stage_for(root, p.c, floats, s0, &p.stage)) != RT_OK) return st;
    }

    /* ---- the image so far goes out to its owners, through their landing areas.  (Frame 0 ignores the buffers' content, but
     * the landing areas may still be read by an earlier call's de-interleave: stage_for has ordered s0 behind that.) */
    RT_HIP(root, hipSetDevice(root->device), "selecting device");
    for (const RankPlan &p : plan)
        if (frame_num > 0 && p.layout.compact_floats() > 0)
            RT_HIP(root, exchange(p.layout, p.stage->d.p, d_frame, false, p.root_list, s0), p.layout.listed ? "interleaving tiles" : "interleaving bands");
    RT_HIP(root, hipEventRecord(root->multi.ev, s0), "recording the start event");
    if ((st = careful(root, plan, s0, "careful mode: waiting for the caller's stream before the ranks start")) != RT_OK) return st;
    for (const RankPlan &p : plan) {
        RT_HIP(p.c, hipSetDevice(p.c->device), "selecting device");
        RT_HIP(p.c, hipStreamWaitEvent(p.c->multi.stream, root->multi.ev, 0), "ordering the ranks behind the caller's stream");
        if (frame_num > 0)
            RT_HIP(p.c, copy_between(p.c->multi.d_bands.p, p.c->device, p.stage->d.p, root->device, p.layout.compact_floats() * 4, p.c->multi.stream), "copying the image so far to its owner");
    }
    if ((st = careful(root, plan, s0, "careful mode: waiting for the image so far to reach its owners (scatter-out)")) != RT_OK) return st;

    /* ---- every rank renders its tiles (asynchronous launches from this one thread) and sends its image to its landing area */
    for (const RankPlan &p : plan) {
        const size_t floats = p.layout.compact_floats();
        if (floats == 0) continue;
        RT_HIP(p.c, hipSetDevice(p.c->device), "selecting device");
        const int32_t cap = batch_cap(p.c, floats);
        for (int32_t done = 0; done < n_frames;) {
            const int32_t k = std::min<int32_t>(n_frames - done, cap);
            st = rt_render_device_batch(p.c, p.scene, cam, rs, times_ms + done, k, frame_num + done, &p.spec, p.c->multi.d_bands.p, p.c->multi.stream);
            if (st != RT_OK) return set_err(root, st, rt_last_error(p.c));
            done += k;
        }
        RT_HIP(p.c, copy_between(p.stage->d.p, root->device, p.c->multi.d_bands.p, p.c->device, floats * 4, p.c->multi.stream), "copying the rank's image to the root GPU");
        RT_HIP(p.c, hipEventRecord(p.c->multi.ev, p.c->multi.stream), "recording the gather event");
    }
    if ((st = careful(root, plan, s0, "careful mode: waiting for the ranks' kernels and their copies to the root GPU")) != RT_OK) return st;

    /* ---- every rank's image into the frame, in s0's order behind its copy */
    RT_HIP(root, hipSetDevice(root->device), "selecting device");
    for (const RankPlan &p : plan) {
        if (p.layout.compact_floats() == 0) continue;
        RT_HIP(root, hipStreamWaitEvent(s0, p.c->multi.ev, 0), "ordering the de-interleave behind the copies");
        RT_HIP(root, exchange(p.layout, p.stage->d.p, d_frame, true, p.root_list, s0), p.layout.listed ? "de-interleaving tiles" : "de-interleaving bands");
        RT_HIP(root, hipEventRecord(p.stage->ev_free, s0), "recording the staging event");
        p.stage->used = true;
    }
    return careful(root, plan, s0, "careful mode: waiting for the de-interleave into the frame");
}

}  // namespace

/* n_frames consecutive progressive frames over n_ranks GPUs, accumulated in place in d_frame (a full
 * frame on ranks[0]'s GPU).  Replaces run_ray_tracer src/dispatch.cu:127-153 for a node: what one
 * device did there, n do here, each for the tiles it owns. */
extern "C" rt_status rt_render_multi_device(const rt_rank *ranks, int32_t n_ranks, const rt_camera *cam, const rt_render_settings *rs,
                                            const int32_t *times_ms, int32_t n_frames, int32_t frame_num, int32_t band_rows,
                                            float *d_frame, void *hip_stream)
{
    if (!ranks || n_ranks < 1 || !ranks[0].ctx) return RT_ERR_INVALID;
    rt_ctx *root = ranks[0].ctx;
    hipStream_t s0 = (hipStream_t)hip_stream;
    std::vector<RankPlan> plan((size_t)n_ranks);
    for (int i = 0; i < n_ranks; i++) { plan[(size_t)i].c = ranks[i].ctx; plan[(size_t)i].scene = ranks[i].scene; }
    rt_status st;
    if ((st = check_and_ready(root, plan, cam, rs, times_ms, n_frames, frame_num, band_rows, d_frame)) != RT_OK) return st;
    /* this call holds every rank's list on the root's GPU at once (the copies to and from the frame), and rank 0's launch
     * looks its own up as well: what the cache hands out from here on is not recycled before the call has queued its work */
    const TileListCache::Pin pin(root->tile_lists);
    if ((st = plan_ranks(root, plan, cam, rs, band_rows, s0)) != RT_OK) return st;
    const bool measuring = band_rows == 0 && root->multi.state.owners == Owners::interleaved;    /* (this call's launches measure the tiles) */
    if ((st = render_ranks(root, plan, cam, rs, times_ms, n_frames, frame_num, d_frame, s0)) != RT_OK) return st;
    if (measuring) root->multi.state.owners = Owners::measured;
    return RT_OK;
}

/* render() src/dispatch.cu:156-163 for a node: host-buffer form of the above */
extern "C" rt_status rt_render_multi(const rt_rank *ranks, int32_t n_ranks, const rt_camera *cam, const rt_render_settings *rs,
                                     const int32_t *times_ms, int32_t n_frames, int32_t *frame_num, float *previous_render)
{
    if (!ranks || n_ranks < 1 || !ranks[0].ctx) return RT_ERR_INVALID;
    rt_ctx *ctx = ranks[0].ctx;
    if (!times_ms || n_frames < 1) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return host_round_trip(ctx, cam, n_frames, frame_num, previous_render, &rt_ctx::d_out, [&](size_t) -> rt_status {
        rt_status st = rt_render_multi_device(ranks, n_ranks, cam, rs, times_ms, n_frames, *frame_num, 0, ctx->d_out.p, nullptr);
        if (st != RT_OK) return st;
        RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
        RT_HIP(ctx, hipStreamSynchronize(nullptr), "render kernels");
        for (int i = 0; i < n_ranks; i++)
            if ((st = rt_ctx_synchronize(ranks[i].ctx)) != RT_OK) return set_err(ctx, st, rt_last_error(ranks[i].ctx));
        RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
        return RT_OK;
    });
}
