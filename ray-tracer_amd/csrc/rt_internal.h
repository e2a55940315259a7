/*
 * rt_internal.h — what the translation units behind the C ABI share: the holders that free HIP handles with their owner (DevBuf, Event,
 * Stream), the context and its parts (rt_ctx: the tile-list cache, the view, the frame pipeline, the multi-GPU rank state, the knobs), the
 * committed scene (rt_scene), the error helpers, the functions of rt_capi.cpp that the other translation units call, the host-buffer round
 * trip and, at the end, what the entry points beside the renderer (rt_query_capi.cpp, rt_occlusion_capi.cpp, rt_ao_capi.cpp,
 * rt_denoise_capi.cpp, rt_adaptive_capi.cpp, rt_views_capi.cpp, rt_sky_capi.cpp, rt_update_capi.cpp, rt_nearest_capi.cpp, rt_multihit_capi.cpp,
 * rt_winding_capi.cpp) have in common: the argument checks, the context's launch bracket and the
 * ray kernels' argument block and launch.  It includes rt_launch.h, the kernel launchers' declarations: no translation unit declares one
 * itself.  rt_capi.cpp owns the life cycle (rt_ctx_create / rt_ctx_destroy, rt_scene_commit).  Not installed: include/rt_amd.h is the interface.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "rt_cull.h"           /* the primary-ray cull: its plane's bookkeeping */
#include "rt_entry.h"          /* ... and the entry words behind the plane */
#include "rt_host.h"
#include "rt_launch.h"         /* the kernel launchers: the seam to rt_kernel.hip */
#include "rt_query.h"          /* RT_QUERY_MAX_RAYS */
#include "rt_rebuild.h"        /* the per-mesh plan of rt_scene_update_mesh */
#include "rt_schedule.h"

/* what crosses the library's translation units without being part of its interface: not in the dynamic symbol table */
#define RT_HIDDEN __attribute__((visibility("hidden")))

namespace rt_detail {

/* A device buffer of at least `cap` elements, freed with its owner.  grow() keeps a large enough buffer and otherwise
 * replaces it (the content is not kept; an empty request still gets 16 bytes); a failure leaves {nullptr, 0}. */
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t grow(size_t need)
    {
        if (cap >= need && p) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void **)&p, need ? need * sizeof(T) : 16);
        if (e == hipSuccess) cap = need; else p = nullptr;
        return e;
    }
};

/* A HIP event and a HIP stream, created by whoever uses them first (null until then) and destroyed with their owner.  The stream
 * is synchronised first: what is still queued on it may use its owner's buffers and events, so in a struct the stream goes LAST
 * (members go in reverse order). */
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    operator hipStream_t() const { return s; }
};

/* a tile list on the device, found again by content (lists are a few KB to ~130 KB and change only with the view).
 * `host` is a pinned copy: what a hash hit is compared with (a 64-bit hash alone would render the wrong
 * tiles on a collision) and what the asynchronous upload reads.  An entry is recycled least-recently-used first; the
 * upload of its new content is ordered behind every launch that read the old one by events, never by a host wait. */
struct DevList {
    uint64_t hash = 0;
    int n = 0;
    DevBuf<uint32_t> d;
    uint32_t *host = nullptr;            /* pinned, d.cap entries */
    uint64_t seq = 0;                    /* TileListCache::seq when last handed out (LRU order; > pin_floor: not recyclable) */
    hipStream_t stream = nullptr;        /* the stream of the launches it was last handed out for (the caller's: not owned) */
    Event ev;                            /* scratch: "everything queued on `stream` so far" (orders a reuse on another stream) */
    Event ev_up;                         /* "the upload from `host` is done": the pinned copy may be rewritten */
    ~DevList() { clear(); }
    /* no content and no buffers: what every failure leaves behind */
    void clear() { d.release(); if (host) (void)hipHostFree(host); host = nullptr; n = 0; hash = 0; }
};

/* The context's tile lists on its GPU, content-addressed (rt_capi.cpp).  Errors are reported through the owning context. */
struct TileListCache {
    std::deque<DevList> lists;           /* (a deque: an entry stays where it is while others are added) */
    size_t cap = 64;                     /* cached tile lists; beyond that the least recently used entry is recycled (raised when one call pins more) */
    uint64_t seq = 0, pin_floor = ~0ull; /* entries handed out after pin_floor are held by the running call (rt_render_multi_device) */
    RT_HIDDEN rt_status on_device(rt_ctx *ctx, const uint32_t *list, int n, hipStream_t stream, const uint32_t **out);
    /* A call that holds several lists at once (rt_render_multi_device: every rank's list on the root) pins what it is handed
     * while this lives: pinned entries are not recycled, the cache grows instead.  It goes when the call has queued its work. */
    struct Pin {
        TileListCache &c;
        explicit Pin(TileListCache &c_) : c(c_) { c.pin_floor = c.seq; }
        ~Pin() { c.pin_floor = ~0ull; }
    };
};

/* the root's landing area for one source context's compact image (rt_gather, rt_render_multi_device) */
struct Stage {
    DevBuf<float> d;
    Event ev_free;                       /* recorded on the root's stream after the last de-interleave that read the area */
    bool used = false;
};

/* cost-balanced multi-GPU calls: a new view's interleaved deal (calls on it measure the tiles), measured, dealt by cost */
enum class Owners { interleaved, measured, balanced };

/* rt_render_multi[_device] with cost-balanced tile lists: what the root remembers between calls */
struct MultiState {
    std::vector<uint32_t> key;           /* camera, image size, number of ranks, scene ids */
    Owners owners = Owners::interleaved;
    std::vector<std::vector<uint32_t>> lists, costs, peaks;   /* per rank: its tiles (image indices), their measured costs and peak pixel costs */
};

/* a context as a rank of the multi-GPU entry points (rt_multi_capi.cpp): its compact buffer, its stream and "my image is in the
 * root's staging area" event; on the root also the staging areas, one per source context, and the ownership of the tiles */
struct MultiRank {
    DevBuf<float> d_bands;
    std::map<rt_ctx *, Stage> stages;
    Event ev;
    MultiState state;
    std::map<int, int> peer_ok;          /* device -> 1 direct access both ways, 0 refused */
    int careful = 0;                     /* RT_AMD_MULTI_CAREFUL=1: rt_render_multi_device waits on the host after every phase (diagnosis) */
    Stream stream;
};

/* where the measured tile costs of the current view are */
enum class Costs { none, on_device, on_host };

/* the current view: (scene, camera, image, tile spec).  Its tiles, their order and what they cost */
struct View {
    std::vector<uint32_t> key;           /* what the state below was built for */
    std::vector<uint32_t> tiles;         /* local tile t of the launch -> the tile's index in the image */
    bool use_order = false;              /* the scene has a mesh: tickets go through `order` (else the kernel scatters raster order) */
    std::vector<uint32_t> order;         /* ticket -> local tile (host copy of d_order) */
    DevBuf<uint32_t> d_order;
    DevBuf<uint32_t> d_cost, d_peak;     /* per tile: the weighted work of its pixels and of its most expensive one, collected by a launch */
    Costs costs = Costs::none;           /* on_device: a launch of this view collected them; on_host: cost / peak hold them and the order is refined */
    int cost_spp = 0;                    /* rays_per_pixel of the launch the figures come from (a pilot: 1) */
    std::vector<uint32_t> cost, peak;    /* the measured (or caller-supplied) costs and peak pixel costs, per local tile */
    int num_heavy = 0;                   /* refined order: how many leading tiles go first for ALL frames of a multi-frame launch */
    /* multi-frame launches, once the tile costs of the view are known: the whole schedule (ticket -> tile, frame),
     * longest job first over all frames (rt_sched::build_job_order) */
    DevBuf<uint32_t> d_jobs;
    int job_frames = 0;                  /* what the uploaded schedule was built for */
};

/* rt_render_views[_device] (rt_views_capi.cpp): what a launch reads beside the scene - the camera table (RT_VIEWS_MAX x 12 floats) and
 * behind it the launch's schedule (rt_sched::views_job_order) - in one device buffer, written by one copy per call from `host`; ev_up:
 * that copy has run, `host` may be rewritten.  d_frames: the host form's frames on the device. */
struct ViewsState {
    std::vector<uint32_t> host;
    DevBuf<uint32_t> d_table;
    DevBuf<float> d_frames;
    Event ev_up;
    bool uploaded = false;               /* ev_up has been recorded */
};

/* The primary-ray cull's bit plane of the current view (rt_cull.h), beside the view's tile costs: one bit per pixel of the full image, written by
 * the pre-pass on the stream of the launch that found the view new and read by every render launch of the view after it - tile lists, bands
 * and batches alike.  `plan` says what a launch does (rt_cull_host::Plan); ev / stream order a reader on another stream behind the pre-pass. */
struct CullPlane {
    DevBuf<uint32_t> d;
    rt_cull_host::Plan plan;
    Event ev;                            /* recorded behind the pre-pass */
    hipStream_t stream = nullptr;        /* ... on this stream (the caller's: not owned) */
    bool enabled = true;                 /* RT_AMD_PRIMARY_CULL=0: every launch renders without the plane */
    bool gates = true;                   /* RT_AMD_SUBTREE_CULL=0: the pre-pass writes every gate word as 0 (the kernel then gates nothing) */
    bool entry = true;                   /* RT_AMD_PRIMARY_ENTRY=0: the pre-pass writes every entry word as 0 (rt_entry.h: every primary ray starts at the root) */
    bool sub = true;                     /* RT_AMD_PRIMARY_SUBENTRY=0: no sub-entry tables (rt_entry.h): the allocation ends with the entry words and nothing is refined */
    int64_t sub_threshold = 0;           /* RT_AMD_SUBENTRY_SAMPLES: a view's first launch queues the refinement if it draws at least this many samples per pixel (rt_cull_host::Plan::refine) */
};

/* knobs (RT_AMD_*), none changes an image: rt_schedule.h has them, their accepted ranges and what the kernel is handed for them
 * (rt_sched::kernel_knobs; RT_AMD_HIT_LOW is clamped to RT_AMD_HIT_BREAK there) */
using rt_sched::Knobs;

}  // namespace rt_detail
using namespace rt_detail;

/* One frame in flight of the pipelined per-frame entry points (rt_frame_submit / rt_frame_collect): everything a launch
 * writes that the context otherwise holds once - its stream, its ticket counter, the plane its pixels' means go to.
 * (The stream goes last: it is synchronised before what its work uses is released.) */
struct FrameSlot {
    DevBuf<uint32_t> counter;           /* 1 KB like rt_ctx::tile_counter */
    DevBuf<float> plane;
    Event ev_done;                      /* the frame's render kernel has finished (recorded on `stream`) */
    Event ev_free;                      /* the blend that read the plane has finished (recorded on `stream` too: the blend runs there) */
    Event ev_call;                      /* where the collector's stream stood when it asked for the frame */
    bool used = false, folded = false;  /* ev_done / ev_free have been recorded at least once */
    rt_sched::Layout layout;            /* the launch's output layout: how rt_frame_collect folds the plane into the caller's frame */
    Stream stream;
};

struct Pipeline {
    int order[RT_PIPELINE_DEPTH];       /* submitted and not collected, oldest first */
    int pending = 0;
    int depth = RT_PIPELINE_DEFAULT_DEPTH;   /* rt_frame_depth: how many frames the caller keeps in flight */
    int last_fold = -1;                 /* the slot whose frame was folded last (folds into one frame happen in collection order) */
    DevBuf<uint32_t> d_list;            /* the view's tile list (listed tile specs), shared by the frames in flight */
    std::vector<uint32_t> list_host;
    FrameSlot slots[RT_PIPELINE_DEPTH]; /* (last: their streams are synchronised before d_list goes) */
};

/* Members go in reverse order, and rt_ctx_destroy relies on it: a stream is synchronised (Stream) before any buffer or event
 * that work queued on it may use is released.  So the two parts that own streams come last - the frames in flight read the
 * view, the rank's stream runs launches that use everything above it - and inside each part the stream is the last member.
 * (A frame's stream may still hold a wait for a younger slot's event that is already gone: the runtime keeps a destroyed
 * event until the waits queued on it have passed.) */
struct rt_ctx {
    int device = 0;
    int num_cus = 0;
    size_t total_mem = 0;
    std::string err;
    DevBuf<uint32_t> tile_counter;      /* 1 KB: the ticket counter, and from tile_counter + 16 the 48 x u64 of a -DRT_STATS build */
    Event ev_start, ev_stop;
    bool have_timing = false;
    /* The launch scratch below (ticket counter, per-frame planes, tile order / costs, the two events) is
     * per context, so launches of one context are kept in order: a launch on another stream than the
     * previous one first waits for that one's stop event (one launch in flight per context). */
    hipStream_t last_stream = nullptr;
    bool launched = false;
    /* persistent frame buffers for the host-buffer entry point */
    DevBuf<float> d_prev, d_out;
    View view;
    DevBuf<float> d_partial;             /* multi-frame launches: one plane of per-pixel frame means per frame; the pilot's scratch plane */
    CullPlane cull;
    TileListCache tile_lists;
    Knobs knobs;
    /* the host-buffer forms of the ray queries and the AOV pass (rt_query_capi.cpp): the rays on the device, and the records / planes */
    DevBuf<float> d_query_in;
    DevBuf<rt_f4> d_query_out;
    /* rt_denoise[_device] (rt_denoise_capi.cpp): per pixel the guide record and the two colour records the levels alternate between */
    DevBuf<rt_f4> d_denoise;
    /* rt_render_adaptive (rt_adaptive_capi.cpp): the half buffers A and B (W*H*3 each, one after the other), their count planes (W*H each),
     * the per-tile error and active-pixel planes (one after the other), the budget plane and the pass's tile list */
    DevBuf<float> d_adaptive_ab;
    DevBuf<uint32_t> d_adaptive_count, d_adaptive_tiles;
    DevBuf<uint16_t> d_adaptive_budget;
    /* rt_scene_update_mesh[_device] (rt_update_capi.cpp): the segments' boxes, the sort's words, two generations of the triangle list, and the
     * host form's vertices on the device.  Shared by the updates of every scene of the context, in the launch order */
    DevBuf<float> d_update_boxes, d_update_pts;
    DevBuf<unsigned long long> d_update_words;
    DevBuf<int32_t> d_update_perm;
    ViewsState views;
    Pipeline pipe;
    MultiRank multi;
};


/* What rt_scene_update_mesh[_device] keeps per mesh of a scene, made at the mesh's first update (rt_update_capi.cpp) */
struct MeshUpdate {
    int32_t n = 0, tri_base = 0, node_base = 0, mesh_index = 0;
    rt_rb_plan plan;                     /* from n alone, checked against the tree the builder made */
    DevBuf<rt_rb_seg> d_segs;
    DevBuf<rt_rb_slot> d_slots;
    DevBuf<float> d_uv0;                 /* the mesh's texture coordinates in commit order (scenes with UVs) */
};

struct rt_scene {
    rt_ctx *ctx = nullptr;
    std::map<int32_t, MeshUpdate> updates;   /* by object index */
    DevBuf<int32_t> d_perm;              /* per triangle of a mesh: the commit index of the one at that leaf position, as of the last update */
    DevBuf<uint32_t> d_flip;             /* flat.tri_flip_commit, four bytes to a word: made at the scene's first winding-number query (rt_winding_capi.cpp) */
    /* the fast winding numbers' cluster trees, made at the scene's first fast query (rt_winding_capi.cpp): the topology on the host and on the
     * device (d_wn_ints: object_range, inv and levels back to back), the records gathered in cluster order, the clusters' sums and moments.
     * wn_stale: the moments are not those of the vertices on the device - the refit runs ahead of the next fast query */
    rt_wn_tree wn_tree;
    bool wn_built = false, wn_stale = true;
    DevBuf<rt_f4> d_wn_topo, d_wn_rec, d_wn_sums, d_wn_moments;
    DevBuf<int32_t> d_wn_ints;
    std::vector<float> wn_read;          /* rt_debug_scene_winding_tree's copy of the moments on the device ... */
    std::vector<int32_t> wn_position;    /* ... and where the device's triangle list has every triangle of the cluster order now */
    FlatScene debug_read;                /* rt_debug_scene_read's copy of what is on the device */
    /* (members go in reverse order: the blob is freed first, the texels last) */
    DevBuf<float> d_tex;
    DevBuf<float> d_tri_uv;
    DevBuf<rt_object> d_objects;
    DevBuf<rt_f4> d_blob;
    FlatScene flat;          /* host copy (sizes, offsets) */
    rt_sched::KernelShape kernel;   /* the kernel shape chosen for this scene */
    uint32_t uid = 0;        /* distinguishes scenes in the tile-order cache (addresses get reused) */
};

/* a cube-map sky (rt_sky_capi.cpp, rt_sky.h): its context, the side of a face, the texels on the device (RT_SKY_TEXEL_FLOATS each) */
struct rt_sky {
    rt_ctx *ctx = nullptr;
    int32_t face_size = 0;
    DevBuf<float> d_texels;
};

/* check_cuda_error src/utils.cu:5-10 */
inline rt_status hip_fail(rt_ctx *ctx, hipError_t e, const char *what)
{
    if (ctx) ctx->err = std::string("Error from HIP (") + what + "): " + hipGetErrorString(e);
    return RT_ERR_HIP;
}

#define RT_HIP(ctx, call, what)                         \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, what); \
    } while (0)

inline rt_status set_err(rt_ctx *ctx, rt_status code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

/* a camera as the kernels take it (rt_kernel_args::cam, a row of the views table): cam_pos, tl_pixel_pos, delta_u, delta_v */
inline void camera_floats(const rt_camera &c, float out[12])
{
    std::memcpy(out + 0, c.cam_pos, 12);
    std::memcpy(out + 3, c.tl_pixel_pos, 12);
    std::memcpy(out + 6, c.delta_u, 12);
    std::memcpy(out + 9, c.delta_v, 12);
}

/* ---- what the other translation units call in rt_capi.cpp ------------------------------------------------------------------------- */
namespace rt_detail {

/* guards the set of live contexts and every root's rt_ctx::multi.stages: rt_ctx_destroy of a source erases its entry there */
extern RT_HIDDEN std::mutex g_ctx_mutex;

RT_HIDDEN rt_status render_frames(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                  const int32_t *times_ms, int32_t n_frames, int32_t frame_num, const rt_tile_spec *tiles,
                                  const float *d_prev, float *d_out, void *hip_stream, bool in_place, FrameSlot *slot = nullptr);
RT_HIDDEN rt_status fold(rt_ctx *ctx, const rt_sched::Layout &L, const float *planes, int n_frames, int frame_num, float *d_out, const uint32_t *d_tile_list,
                         hipStream_t stream);
RT_HIDDEN rt_status ensure_frame_buffers(rt_ctx *ctx, size_t bytes);
/* the render kernel's argument block for a launch of layout L (tile order, tile list and outputs beyond d_out are the caller's to add),
 * and the size of its grid: what rt_adaptive_capi.cpp launches the budget variant with */
RT_HIDDEN rt_kernel_args kernel_args(const rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, const int32_t *times_ms,
                                     int32_t n_frames, int32_t frame_num, const rt_sched::Layout &L, const float *d_prev, float *d_out, uint32_t *tile_counter);
RT_HIDDEN int launch_blocks(const rt_ctx *ctx, const rt_scene *scene, int num_tiles);
RT_HIDDEN int batch_cap(const rt_ctx *ctx, size_t plane_floats);
/* a scene's uid: at commit, and again after an update of its geometry (what was cached for the old one - the view, its tile costs - is then not found) */
RT_HIDDEN uint32_t next_scene_uid();
RT_HIDDEN void push_camera(std::vector<uint32_t> &key, const rt_camera *cam);

/* ---- what rt_sky_capi.cpp calls in rt_views_capi.cpp: the camera sequences with the kernel left open ---- */
/* launches the views kernel, or a variant of it, for one block of arguments and the device's camera table */
using ViewsLauncher = std::function<hipError_t(const rt_kernel_args &a, const float *d_cams, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream)>;
/* a device form with everything but the views of one chunk bound: (cams, times_ms, n_views, frame_num, d_frames) */
using ViewsDeviceForm = std::function<rt_status(const rt_camera *, const int32_t *, int32_t, int32_t, float *)>;
RT_HIDDEN rt_status check_views(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms, int32_t n_views, const rt_render_settings *rs,
                                int32_t accumulate, int32_t frame_num, const void *frames, bool device);
RT_HIDDEN rt_status views_launch(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms, int32_t n_views, const rt_render_settings *rs,
                                 int32_t accumulate, int32_t frame_num, float *d_frames, hipStream_t stream, const ViewsLauncher &launcher);
RT_HIDDEN rt_status views_host_form(rt_ctx *ctx, const rt_camera *cams, const int32_t *times_ms, int32_t n_views, int32_t accumulate, int32_t *frame_num, float *frames,
                                    const ViewsDeviceForm &device_form);

/* The host-buffer forms' round trip (render() src/dispatch.cu:156-163): the caller's frame goes into the persistent buffer `into`
 * (d_prev or d_out), `render_and_wait(bytes)` renders n_frames frames into d_out and waits for them, the frame comes back and
 * *frame_num advances. */
template <class Render>
rt_status host_round_trip(rt_ctx *ctx, const rt_camera *cam, int32_t n_frames, int32_t *frame_num, float *previous_render, DevBuf<float> rt_ctx::*into,
                          Render render_and_wait)
{
    if (!ctx || !cam || !frame_num || !previous_render) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (cam->width <= 0 || cam->height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t bytes = (size_t)cam->width * (size_t)cam->height * 3 * sizeof(float);
    rt_status st = ensure_frame_buffers(ctx, bytes);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipMemcpy((ctx->*into).p, previous_render, bytes, hipMemcpyHostToDevice), "copying previous frame");
    if ((st = render_and_wait(bytes)) != RT_OK) return st;
    RT_HIP(ctx, hipMemcpy(previous_render, ctx->d_out.p, bytes, hipMemcpyDeviceToHost), "copying frame to host");
    *frame_num += n_frames;                            /* src/dispatch.cu:159 */
    RT_HIP(ctx, hipPeekAtLastError(), "final check after render");   /* src/dispatch.cu:161-162 */
    return RT_OK;
}

}  // namespace rt_detail

/* ---- argument checks shared by the entry points ------------------------------------------------------------------------------- */
inline rt_status check_scene(rt_ctx *ctx, const rt_scene *scene)
{
    if (!ctx || !scene) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (scene->ctx != ctx) return set_err(ctx, RT_ERR_INVALID, "scene belongs to another context");
    return RT_OK;
}

/* n rays on a scene: their origins, their directions and where the answers go */
inline rt_status check_rays(rt_ctx *ctx, const rt_scene *scene, const void *origins, const void *directions, int64_t n, const void *answers)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (n < 0 || n > RT_QUERY_MAX_RAYS) return set_err(ctx, RT_ERR_INVALID, "bad ray count (0 .. 2^30)");
    if (n > 0 && (!origins || !directions || !answers)) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return RT_OK;
}

/* n points on a scene (rt_nearest_capi.cpp, rt_winding_capi.cpp; where the answers go is the caller's to check) */
static_assert(RT_NEAREST_MAX_POINTS == RT_WINDING_MAX_POINTS, "one check serves both families");
inline rt_status check_points(rt_ctx *ctx, const rt_scene *scene, const void *points, int64_t n)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (n < 0 || n > RT_NEAREST_MAX_POINTS) return set_err(ctx, RT_ERR_INVALID, "bad point count (0 .. 2^30)");
    if (n > 0 && !points) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return RT_OK;
}

/* The scene's "leaf position -> commit index" list on the device, made by whoever needs it first: a mesh's first update (rt_update_capi.cpp:
 * the rebuild kernels keep it current from then on) or the scene's first winding-number query (rt_winding_capi.cpp reads it).  It starts as
 * the flattener's tri_order.  A failure leaves the scene without the list, as it was. */
inline rt_status ensure_scene_perm(rt_ctx *ctx, rt_scene *scene)
{
    if (scene->d_perm.p) return RT_OK;
    const std::vector<int32_t> &order = scene->flat.tri_order;
    RT_HIP(ctx, scene->d_perm.grow(order.size()), "allocating the scene's triangle order");
    const hipError_t e = order.empty() ? hipSuccess : hipMemcpy(scene->d_perm.p, order.data(), order.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        scene->d_perm.release();
        return hip_fail(ctx, e, "uploading the scene's triangle order");
    }
    return RT_OK;
}

/* (2^28 pixels are 2^22 tiles of 8x8: RT_JOB_TILE_MASK, and 64 * tiles fits the ray kernels' 32-bit ids) */
inline rt_status check_image_size(rt_ctx *ctx, int32_t width, int32_t height)
{
    if (width <= 0 || height <= 0 || width > 32768 || height > 32768 || (int64_t)width * height > (1 << 28))
        return set_err(ctx, RT_ERR_INVALID, "bad image size (at most 32768 pixels on a side and 2^28 in all)");
    return RT_OK;
}

/* ---- the launch bracket ------------------------------------------------------------------------------------------------------ */
/* `work` (kernel launches and copies on `stream`, nothing that waits) in the context's launch order and between its timing events, as
 * render_frames does it (rt_capi.cpp): one launch in flight per context, because the scratch is shared (see rt_ctx) - behind the previous
 * launch if that ran on another stream, and behind every pipelined frame in flight.  A step that fails ends the call where it stands: after
 * ev_start is recorded that leaves have_timing == false, and launched / last_stream as they were. */
template <class Work>
rt_status launch_bracket(rt_ctx *ctx, hipStream_t stream, Work work)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    if (ctx->launched && ctx->last_stream != stream) RT_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_stop, 0), "ordering the launch behind the previous one");
    for (FrameSlot &fs : ctx->pipe.slots)
        if (fs.used) RT_HIP(ctx, hipStreamWaitEvent(stream, fs.ev_done, 0), "ordering the launch behind the frames in flight");
    RT_HIP(ctx, hipEventRecord(ctx->ev_start, stream), "recording start event");
    ctx->have_timing = false;
    const rt_status st = work();
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipEventRecord(ctx->ev_stop, stream), "recording stop event");
    ctx->have_timing = true;
    ctx->launched = true;
    ctx->last_stream = stream;
    return RT_OK;
}

/* ---- the ray kernels' argument blocks and launch (rt_query.h, rt_occlusion.h, rt_ray_kernel.h) ---------------------------- */
/* a zeroed block (rt_query_args or rt_occlusion_args: the fields carry the same names) with the scene and the work filled in: n rays, or tile
 * slots, handed out from the context's ticket counter */
template <class Args>
Args ray_args_scene(const rt_ctx *ctx, const rt_scene *scene, uint32_t n)
{
    Args a;
    std::memset(&a, 0, sizeof a);
    a.blob = scene->d_blob.p;
    a.blob_f4 = (int32_t)scene->flat.blob.size();
    a.off_nodes = scene->flat.off_nodes;
    a.off_tris = scene->flat.off_tris;
    a.off_objlds = scene->flat.off_objlds;
    a.off_meshes = scene->flat.off_meshes;
    a.off_objtab = scene->flat.off_objtab;
    a.num_objects = (int32_t)scene->flat.objects.size();
    a.num_meshes = scene->flat.num_meshes;
    a.descend_keep = ctx->knobs.descend_keep;
    a.n = n;
    a.num_chunks = (n + 63u) / 64u;
    a.counter = ctx->tile_counter.p;
    return a;
}

/* ... and for a pass over a view: one slot per pixel of every 8x8 tile (at most 2^22 tiles: check_image_size), and the camera */
template <class Args>
Args ray_args_view(const rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam)
{
    const int tiles_x = (cam->width + 7) / 8, tiles_y = (cam->height + 7) / 8;
    Args a = ray_args_scene<Args>(ctx, scene, (uint32_t)tiles_x * (uint32_t)tiles_y * 64u);
    a.tiles_x = tiles_x;
    camera_floats(*cam, a.cam);
    a.width = cam->width;
    a.height = cam->height;
    return a;
}

/* A ray kernel of the scene's shape queued on `stream` behind the clearing of its ticket counter (`launcher`: rt_launch_query, rt_launch_occlusion,
 * rt_launch_ao, rt_launch_nearest, rt_launch_sweep, rt_launch_multihit, rt_launch_overlap or rt_launch_tritri, with its `front`: read by the
 * first two only).  Without the bracket: for the work of a caller that is inside one. */
template <class Args>
rt_status enqueue_rays(rt_ctx *ctx, const rt_scene *scene, const Args &a, hipError_t (*launcher)(const Args *, rt_shape, int, int, size_t, hipStream_t), int front,
                       const char *what_clear, const char *what, hipStream_t stream)
{
    RT_HIP(ctx, hipMemsetAsync(a.counter, 0, 512, stream), what_clear);
    RT_HIP(ctx, launcher(&a, scene->kernel.shape, front, ctx->num_cus, scene->kernel.lds_bytes, stream), what);
    return RT_OK;
}

/* One launch of a ray kernel in the launch bracket: the ticket counter is shared with the render launches. */
template <class Args>
rt_status launch_rays(rt_ctx *ctx, const rt_scene *scene, const Args &a, hipError_t (*launcher)(const Args *, rt_shape, int, int, size_t, hipStream_t), int front,
                      const char *what, hipStream_t stream)
{
    return launch_bracket(ctx, stream, [&]() -> rt_status { return enqueue_rays(ctx, scene, a, launcher, front, "clearing the ray counter", what, stream); });
}
