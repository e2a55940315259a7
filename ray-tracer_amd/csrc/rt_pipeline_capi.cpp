/*
 * rt_pipeline_capi.cpp — frames in flight (include/rt_amd.h: rt_frame_submit ... rt_frame_wait): up to rt_frame_depth launches of
 * one context overlap, each on a slot's own stream with the slot's ticket counter and plane (FrameSlot, rt_internal.h), and are
 * folded into the caller's frame in the order they were submitted.  The launch itself is render_frames (rt_capi.cpp), which also
 * orders the context's other launches behind the frames in flight.
 */
#include <hip/hip_runtime.h>

#include "rt_internal.h"

static rt_status init_slot(rt_ctx *ctx, FrameSlot &fs)
{
    /* (each member on its own: a call that failed half-way is finished by the next one) */
    if (!fs.stream) {
        /* Frames only overlap if their streams sit on different hardware queues.  The runtime keeps a pool of them per stream
         * priority (four each by default, GPU_MAX_HW_QUEUES) and the caller's own streams - the null stream, PyTorch's - already
         * live in the normal-priority pool: a fourth frame's stream would share a queue there and run behind its neighbour
         * (measured: 4 in flight 333 ms per frame, worse than 3; with streams of the high-priority pool 286-290).  Slots 0-3 take
         * the high-priority pool, 4-7 the low-priority one; the priority itself is immaterial (the frames are each other's only
         * competitors: alternating the pools over the slots measures the same at every depth). */
        int lo = 0, hi = 0;
        const int k = (int)(&fs - ctx->pipe.slots);
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            RT_HIP(ctx, hipStreamCreateWithPriority(&fs.stream.s, hipStreamNonBlocking, k < 4 ? hi : lo), "creating a pipelined frame's stream");
        else
            RT_HIP(ctx, hipStreamCreateWithFlags(&fs.stream.s, hipStreamNonBlocking), "creating a pipelined frame's stream");
    }
    if (!fs.counter.p) RT_HIP(ctx, fs.counter.grow(256), "allocating a pipelined frame's ticket counter");
    if (!fs.ev_done) RT_HIP(ctx, hipEventCreateWithFlags(&fs.ev_done.e, hipEventDisableTiming), "creating a pipelined frame's event");
    if (!fs.ev_free) RT_HIP(ctx, hipEventCreateWithFlags(&fs.ev_free.e, hipEventDisableTiming), "creating a pipelined frame's event");
    if (!fs.ev_call) RT_HIP(ctx, hipEventCreateWithFlags(&fs.ev_call.e, hipEventDisableTiming), "creating a pipelined frame's event");
    return RT_OK;
}

extern "C" rt_status rt_frame_submit(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                     int32_t time_ms, const rt_tile_spec *tiles)
{
    if (!ctx) return RT_ERR_INVALID;
    Pipeline &pl = ctx->pipe;
    if (pl.pending >= pl.depth) return set_err(ctx, RT_ERR_BUSY, "as many frames as rt_frame_depth allows are in flight: collect one first");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* a free slot: one that is not waiting to be collected */
    int k = -1;
    for (int i = 0; i < RT_PIPELINE_DEPTH && k < 0; i++) {
        bool busy = false;
        for (int j = 0; j < pl.pending; j++) busy = busy || pl.order[j] == i;
        if (!busy) k = i;
    }
    FrameSlot &fs = pl.slots[k];
    rt_status st = init_slot(ctx, fs);
    if (st != RT_OK) return st;
    /* (the slot's plane is rewritten behind the blend that read it last: that ran on the slot's stream) */
    st = render_frames(ctx, scene, cam, rs, &time_ms, 1, 0, tiles, nullptr, nullptr, nullptr, true, &fs);
    if (st != RT_OK) return st;
    pl.order[pl.pending++] = k;
    return RT_OK;
}

extern "C" rt_status rt_frame_collect(rt_ctx *ctx, int32_t frame_num, float *d_frame, void *hip_stream)
{
    if (!ctx) return RT_ERR_INVALID;
    Pipeline &pl = ctx->pipe;
    if (pl.pending <= 0) return set_err(ctx, RT_ERR_INVALID, "no frame has been submitted");
    if (frame_num < 0) return set_err(ctx, RT_ERR_INVALID, "bad frame number");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    FrameSlot &fs = pl.slots[pl.order[0]];
    if (d_frame && fs.layout.num_tiles > 0) {
        /* The blend runs on the frame's own stream, right behind its render kernel, and the caller's stream only waits for it
         * (a kernel queued on the caller's stream may sit behind whatever shares that stream's hardware queue).  Ordered behind
         * what the caller has queued so far (it may still be reading d_frame) and behind the previous frame's blend. */
        hipStream_t stream = (hipStream_t)hip_stream;
        RT_HIP(ctx, hipEventRecord(fs.ev_call, stream), "recording the collector's position");
        RT_HIP(ctx, hipStreamWaitEvent(fs.stream, fs.ev_call, 0), "ordering the blend behind the collector's stream");
        if (pl.last_fold >= 0 && pl.last_fold != pl.order[0])
            RT_HIP(ctx, hipStreamWaitEvent(fs.stream, pl.slots[pl.last_fold].ev_free, 0), "ordering the blend behind the previous frame's");
        rt_status st = fold(ctx, fs.layout, fs.plane.p, 1, frame_num, d_frame, pl.d_list.p, fs.stream);
        if (st != RT_OK) return st;
        RT_HIP(ctx, hipEventRecord(fs.ev_free, fs.stream), "recording a pipelined frame's blend");
        fs.folded = true;
        pl.last_fold = pl.order[0];
        RT_HIP(ctx, hipStreamWaitEvent(stream, fs.ev_free, 0), "ordering the collector's stream behind the blend");
    }
    for (int j = 1; j < pl.pending; j++) pl.order[j - 1] = pl.order[j];
    pl.pending--;
    return RT_OK;
}

extern "C" int32_t rt_frames_pending(const rt_ctx *ctx) { return ctx ? ctx->pipe.pending : 0; }

extern "C" rt_status rt_frame_depth(rt_ctx *ctx, int32_t depth)
{
    if (!ctx) return RT_ERR_INVALID;
    if (depth < 1 || depth > RT_PIPELINE_DEPTH) return set_err(ctx, RT_ERR_INVALID, "the depth of the frame pipeline is 1..RT_PIPELINE_DEPTH");
    if (ctx->pipe.pending > 0) return set_err(ctx, RT_ERR_BUSY, "frames are in flight: collect them before changing the depth");
    ctx->pipe.depth = depth;
    return RT_OK;
}

/* host-buffer form of rt_frame_collect, with rt_render's contract for previous_render and *frame_num */
extern "C" rt_status rt_frame_collect_host(rt_ctx *ctx, int32_t *frame_num, float *previous_render)
{
    if (!ctx || !frame_num) return set_err(ctx, RT_ERR_INVALID, "null argument");
    Pipeline &pl = ctx->pipe;
    if (pl.pending <= 0) return set_err(ctx, RT_ERR_INVALID, "no frame has been submitted");
    if (!previous_render) return rt_frame_collect(ctx, 0, nullptr, nullptr);          /* discard */
    if (*frame_num < 0) return set_err(ctx, RT_ERR_INVALID, "bad frame number");
    FrameSlot &fs = pl.slots[pl.order[0]];
    if (!fs.layout.whole_frame()) return set_err(ctx, RT_ERR_INVALID, "the host-buffer form collects whole frames (submitted without a tile spec)");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t bytes = (size_t)fs.layout.width * (size_t)fs.layout.height * 3 * sizeof(float);
    rt_status st = ensure_frame_buffers(ctx, bytes);
    if (st != RT_OK) return st;
    /* everything on the frame's own stream, behind its render kernel; the host waits for that stream only - the younger frames
     * keep running (a hipDeviceSynchronize, as in rt_render, would wait for them too) */
    if (*frame_num > 0) RT_HIP(ctx, hipMemcpyAsync(ctx->d_out.p, previous_render, bytes, hipMemcpyHostToDevice, fs.stream), "copying previous frame");
    st = rt_frame_collect(ctx, *frame_num, ctx->d_out.p, fs.stream);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipMemcpyAsync(previous_render, ctx->d_out.p, bytes, hipMemcpyDeviceToHost, fs.stream), "copying frame to host");
    RT_HIP(ctx, hipStreamSynchronize(fs.stream), "render kernel");
    *frame_num += 1;                                   /* src/dispatch.cu:159 */
    return RT_OK;
}

extern "C" rt_status rt_frame_wait(rt_ctx *ctx)
{
    if (!ctx) return RT_ERR_INVALID;
    const Pipeline &pl = ctx->pipe;
    if (pl.last_fold < 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    RT_HIP(ctx, hipEventSynchronize(pl.slots[pl.last_fold].ev_free), "waiting for the collected frame");
    return RT_OK;
}
