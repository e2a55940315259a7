/*
 * rt_amd.h — C ABI of the MI355X path tracer (libraytracer_amd.so).
 *
 * The reference (Ben-Edwards44/Ray-Tracer) has no FFI; the seam its hot path sits behind is
 * the host<->device edge in src/dispatch.cu plus three __constant__ uploads.  Each entry
 * point below names the reference interface it replaces (file:line relative to the
 * reference checkout).  Plain pointers and sizes only; nothing throws across this boundary:
 * every call returns an rt_status and leaves a message for rt_last_error().
 *
 * Threading: one rt_ctx per GPU, used from one host thread at a time (the reference is a
 * single host thread with blocking launches, src/dispatch.cu:139-141).  There are no hidden
 * globals: scene, camera and settings are arguments (the reference's __constant__ symbols
 * make it non-reentrant).
 *
 * One launch in flight per context.  A context owns the scratch its launches use (tile ticket
 * counter, the per-frame planes of a multi-frame launch, tile order and costs, timing events), so
 * the device-buffer entry points keep a context's launches in order: a launch on a different
 * stream than the previous one is queued behind it (hipStreamWaitEvent), it does not overlap it.
 * To overlap renders on one GPU use two contexts; to use several GPUs use one context per GPU
 * (rt_render_multi below, or one process per GPU).  The exception is rt_frame_submit / rt_frame_collect:
 * up to RT_PIPELINE_DEPTH progressive frames of one context in flight, each with scratch of its own.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t rt_status;
enum {
    RT_OK = 0,
    RT_ERR_INVALID = 1,      /* bad argument */
    RT_ERR_IO = 2,           /* "Could not find file to open."  (src/obj_read.cu:10) */
    RT_ERR_UNSUPPORTED = 3,  /* e.g. "Only triangle or quad meshes are supported." (src/main.cu:141) */
    RT_ERR_HIP = 4,          /* "Error from HIP (<what>): <hipGetErrorString>"  (src/utils.cu:5-10) */
    RT_ERR_NOMEM = 5,
    RT_ERR_NO_DEVICE = 6,    /* the HIP runtime reports no usable GPU: there is NO CPU fallback */
    RT_ERR_BUSY = 7          /* rt_frame_submit: RT_PIPELINE_DEPTH frames are in flight */
};

typedef struct rt_ctx rt_ctx;
typedef struct rt_scene rt_scene;
typedef struct rt_scene_builder rt_scene_builder;
typedef struct rt_obj rt_obj;

/* ---- materials: Texture / Material, src/material.cu:4-186 ------------------------------- */
enum { RT_TEX_COLOUR = 0, RT_TEX_GRADIENT = 1, RT_TEX_CHECKERBOARD = 2, RT_TEX_IMAGE = 3 };   /* :7-10 */
enum { RT_MAT_STANDARD = 0, RT_MAT_EMISSIVE = 1, RT_MAT_REFRACTIVE = 2 };                     /* :131-133 */

typedef struct rt_material {
    int32_t type;              /* RT_MAT_* */
    int32_t tex_type;          /* RT_TEX_* */
    float colour[3];           /* Texture::create_const_colour :21-26 */
    float light[3], dark[3];   /* Texture::create_checkerboard :32-40 */
    int32_t num_squares;
    float smoothness;          /* [0,1]: 0 diffuse, 1 mirror ("metal" = STANDARD with smoothness > 0) */
    int32_t need_uv;
    float emitted_light[3];    /* colour * strength, :170 */
    float refractive_index;
    int32_t img_w, img_h;      /* Texture::create_image :42-51 */
    const float *img_rgb;      /* img_w*img_h*3 floats, row-major; copied when the object is added */
} rt_material;

/* Material::create_standard(Texture::create_const_colour(colour), smoothness)  :157-165 */
void rt_material_standard(rt_material *m, const float colour[3], float smoothness);
/* Material::create_standard(Texture::create_checkerboard(light, dark, n), smoothness) */
void rt_material_checkerboard(rt_material *m, const float light[3], const float dark[3], int32_t num_squares, float smoothness);
/* Material::create_standard(Texture::create_gradient(), smoothness) */
void rt_material_gradient(rt_material *m, float smoothness);
/* Material::create_emissive(colour, strength) :167-173.  The reference leaves smoothness,
 * need_uv and texture uninitialised there; this ABI defines them as 0 / false / COLOUR(0,0,0). */
void rt_material_emissive(rt_material *m, const float colour[3], float strength);
/* Material::create_refractive(Texture::create_const_colour(colour), n) :175-185 (smoothness = 1) */
void rt_material_refractive(rt_material *m, const float colour[3], float n);
/* Material::create_standard(Texture::create_image(width, height, rgb), smoothness) :42-51;
 * nearest-texel lookup :119-124 (an out-of-range texel index is clamped, the reference reads
 * out of bounds) */
void rt_material_image(rt_material *m, int32_t width, int32_t height, const float *rgb, float smoothness);
/* ImageTexture src/main.cu:40-91: the entry `name` of a baked texture file
 * (textures/parse_textures.py format: name \n W \n H \n "r g b r g b ... ").  *rgb is malloc'ed;
 * release it with rt_image_texture_free.  RT_ERR_IO: file missing; RT_ERR_INVALID: name not
 * found ("Image file not found.", src/main.cu:72) */
rt_status rt_image_texture_load(const char *parsed_textures_path, const char *name, int32_t *width, int32_t *height, float **rgb);
void rt_image_texture_free(float *rgb);

/* ---- scene: Object::create_* src/objects.cu:845-906, SceneObjects src/main.cu:94-296 ------ */
rt_status rt_scene_builder_create(rt_scene_builder **out);
void rt_scene_builder_destroy(rt_scene_builder *b);
const char *rt_scene_builder_error(const rt_scene_builder *b);
/* objects are kept in call order = the reference's std::vector<Object> order (ties go to
 * the later object, src/raytracer.cu:36) */
rt_status rt_scene_add_sphere(rt_scene_builder *b, const float center[3], float radius, const rt_material *m);          /* :845-852 */
rt_status rt_scene_add_triangle(rt_scene_builder *b, const float p1[3], const float p2[3], const float p3[3], const rt_material *m);  /* :854-861 */
rt_status rt_scene_add_triangle_uv(rt_scene_builder *b, const float p[9], const float uv[6], const rt_material *m);    /* :863-870 */
rt_status rt_scene_add_quad(rt_scene_builder *b, const float p1[3], const float p2[3], const float p3[3], const float p4[3], const rt_material *m);  /* :872-879 */
rt_status rt_scene_add_one_way_quad(rt_scene_builder *b, const float p1[3], const float p2[3], const float p3[3], const float p4[3], int32_t invert_normal, const rt_material *m);  /* :881-888 */
rt_status rt_scene_add_cuboid(rt_scene_builder *b, const float tl_near_pos[3], float width, float height, float depth, const rt_material *m);  /* :890-897 */
/* Object::create_mesh :899-906 — triangles: n*9 floats; the fixed-depth-10 BVH of
 * src/objects.cu:602-719 is rebuilt host-side and stored compactly */
rt_status rt_scene_add_mesh(rt_scene_builder *b, const float *triangles, int32_t n, const rt_material *m);
/* SceneObjects::create_mesh src/main.cu:127-148 — faces of a loaded .obj (3 or 4 vertices) */
rt_status rt_scene_add_obj_mesh(rt_scene_builder *b, const rt_obj *o, const rt_material *m);
int32_t rt_scene_builder_num_objects(const rt_scene_builder *b);

/* ---- .obj loader: ObjFileMesh src/obj_read.cu:47-147 ------------------------------------- */
rt_status rt_obj_load(const char *filename, rt_obj **out);          /* ObjFileMesh(filename) :52-57 */
void rt_obj_destroy(rt_obj *o);
void rt_obj_enlarge(rt_obj *o, float scale_fact);                   /* :59-64 */
void rt_obj_rotate(rt_obj *o, float x_angle, float y_angle, float z_angle);   /* :66-76; sin/cos from rt_math.h */
void rt_obj_translate(rt_obj *o, float dx, float dy, float dz);     /* :78-86 */
int32_t rt_obj_num_vertices(const rt_obj *o);
int32_t rt_obj_num_faces(const rt_obj *o);
int32_t rt_obj_face_arity(const rt_obj *o, int32_t face);
void rt_obj_get_face(const rt_obj *o, int32_t face, int32_t *out /* arity 0-based vertex indices */);
/* the same object from arrays already in memory: vertices n*3 floats, faces as a flat 0-based
 * index list with one arity per face */
rt_status rt_obj_from_arrays(const float *vertices, int32_t num_vertices, const int32_t *face_indices,
                             const int32_t *face_arity, int32_t num_faces, rt_obj **out);
void rt_obj_get_vertices(const rt_obj *o, float *out /* num_vertices*3 */);
int32_t rt_obj_num_triangles(const rt_obj *o);                       /* after the quad split; -1 if a face is not 3/4-sided */
rt_status rt_obj_get_triangles(const rt_obj *o, float *out /* num_triangles*9 */);     /* RT_ERR_INVALID: a face names a vertex the file does not have */

/* ---- camera: src/camera.cu:12-21 (DeviceCamData) and :34-108 (Camera) -------------------- */
typedef struct rt_camera {
    float cam_pos[3];
    float tl_pixel_pos[3];
    float delta_u[3];
    float delta_v[3];
    int32_t width, height;     /* SCREEN_WIDTH / SCREEN_HEIGHT src/camera.cu:4-5, a parameter here */
} rt_camera;

/* Camera::assign_constant_mem :46-60 with the reference's pose constants (:34-41: origin,
 * FOV 60 deg, focal length 0.1, no rotation); tan/sin/cos from rt_math.h */
void rt_camera_default(int32_t width, int32_t height, rt_camera *out);
/* same with pose parameters (angles in radians, rotation order Rx*Ry*Rz as :63-69) */
void rt_camera_make(int32_t width, int32_t height, const float pos[3], float fov, float focal_len,
                    float x_rot, float y_rot, float z_rot, rt_camera *out);

/* ---- render settings: RenderData src/raytracer.cu:4-12 ----------------------------------- */
typedef struct rt_render_settings {
    int32_t rays_per_pixel;
    int32_t reflection_limit;
    int32_t antialias;
    float sky_colour[3];
} rt_render_settings;

/* ---- context + scene upload -------------------------------------------------------------- */
/* fails with RT_ERR_NO_DEVICE when HIP has no device: the product has no CPU path */
rt_status rt_ctx_create(int32_t device, rt_ctx **out);
void rt_ctx_destroy(rt_ctx *ctx);
const char *rt_last_error(const rt_ctx *ctx);
/* replaces create_gpu_struct src/main.cu:290-295 + allocate_constant_mem src/dispatch.cu:104-108:
 * flattens the builder's objects into the compact device layout and uploads it */
rt_status rt_scene_commit(rt_ctx *ctx, const rt_scene_builder *b, rt_scene **out);
void rt_scene_destroy(rt_scene *s);
/* introspection for tests: bytes of LDS per workgroup, node / triangle counts, the launch shape chosen for the
 * scene (workgroup size and how many workgroups are resident per CU); scene_in_lds: 1 the whole scene is staged
 * into LDS, 2 everything but the triangles (a mesh of more than ~1,500 triangles: its BVH still fits), 0 nothing
 * (the kernel reads the scene from global memory / L2); kernel_variant: which render kernel of that shape plain frames run
 * (rt_render_device, rt_render_device_batch, the frame pipeline, rt_render_multi_device) - 0 the generic one, 1 the one compiled
 * for scenes whose objects besides at most one mesh are all spheres and whose materials need no texture coordinates, refraction or
 * texture.  Decided at commit from the scene alone; RT_AMD_KERNEL_VARIANT=generic in the environment of rt_scene_commit keeps 0.
 * Both compute the same frames bit for bit */
#define RT_KERNEL_VARIANT_GENERIC 0
#define RT_KERNEL_VARIANT_TRAITS 1
typedef struct rt_scene_info {
    int32_t num_objects, num_triangles, num_nodes, lds_bytes, scene_in_lds, threads_per_block, stack_entries, blocks_per_cu;
    int32_t kernel_variant;
} rt_scene_info;
rt_status rt_scene_get_info(const rt_scene *s, rt_scene_info *out);

/* ---- time-varying geometry: a committed mesh rebuilt from new vertices, on the device -------------------------------------------------
 * A committed scene renders many frames, views and queries; these two calls give it the next time step.  The mesh keeps its triangle count, and
 * with it everything the reference's builder derives from the count alone (node indices, child references, leaf ranges, the chain edges,
 * the per-lane stack depth, every offset of the device layout, the LDS placement and the kernel shape: DESIGN.md section 21); the triangles' order
 * in the leaves and every box are rebuilt by kernels, exactly as the host builder would make them: */
/* object_index names an RT_OBJ_MESH of n triangles (its count at commit); triangle i of the mesh (commit input order: row i of rt_scene_add_mesh's array,
 * or of rt_obj_get_triangles for an .obj mesh) becomes the three points d_triangles[9 i .. 9 i + 9). */
rt_status rt_scene_update_mesh_device(rt_ctx *ctx, rt_scene *scene, int32_t object_index, const float *d_triangles, int32_t n, void *hip_stream);
rt_status rt_scene_update_mesh(rt_ctx *ctx, rt_scene *scene, int32_t object_index, const float *triangles, int32_t n);   /* host memory; returns when done */
/* Result: everything the kernels read of the scene is then, as bytes, what rt_scene_commit uploads for a builder that differs only in this
 * mesh's triangles - its triangle records and their order, its node boxes, its entry of the mesh table, its object record (both copies), the
 * box in its shading record, its rows of the texture coordinates (a triangle keeps the coordinates it had at commit) - and nothing else is
 * written: every entry point's output on the updated scene is its output on a scene committed with the new triangles.
 * Inputs: finite coordinates of magnitude at most 2^28; the host form refuses others (RT_ERR_INVALID), the device form cannot look: with other
 * inputs the scene's content is unspecified, but the call stays memory-safe.  A zero-area triangle's normal is a NaN, as at commit.
 * Order: the device form is asynchronous on hip_stream (d_triangles is read there) and takes its place in the context's launch order like
 * rt_render_device: a launch issued before it reads the old mesh, a launch issued after it the new one, on whatever streams; it is queued
 * behind the frames in flight.  The context owns the scratch.  The scene's cached view (tile order and costs) is dropped.
 * RT_ERR_INVALID, with the scene and the launch order untouched: a null pointer, a scene of another context, an index that is out of range
 * or names no mesh, n different from the mesh's count.  n == 0 for an empty mesh succeeds and does nothing.  A mesh whose triangle count
 * changes is rt_scene_commit's. */
#define RT_REBUILD_LDS_TRIS 2048   /* the most triangles of a tree level's segment that one workgroup rebuilds in LDS (sized in rt_rebuild.h): a mesh up to this size is one launch */

/* ---- the per-frame call: render() src/dispatch.cu:156-163 --------------------------------- */
/* Host-buffer form, same contract as the reference: previous_render (W*H*3 floats, row-major
 * interleaved RGB) is read, blended as (colour + prev*frame_num)/(frame_num+1)
 * (src/raytracer.cu:109-112) and overwritten; *frame_num is incremented.  time_ms is the seed
 * term the reference takes from the wall clock (src/main.cu:18-25). */
rt_status rt_render(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                    int32_t time_ms, int32_t *frame_num, float *previous_render);
/* n_frames passes of that loop body in one call (frame i seeded with times_ms[i]); the frames are
 * rendered by multi-frame launches (rt_render_device_batch below), the result is the same image. */
rt_status rt_render_frames(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                           const int32_t *times_ms, int32_t n_frames, int32_t *frame_num, float *previous_render);

/* Device-buffer form for callers that own HBM (PyTorch tensors) and streams.
 * Which pixels a call renders is given in one of two forms ("tile rows or tile list"):
 *  - bands: rows are handed out in bands of `band_rows` rows; the call renders the bands whose index b
 *    satisfies b % band_stride == band_first (band_stride = number of GPUs, band_first = rank);
 *  - a tile list (tile_list != NULL; the band fields are then ignored): the call renders the 8x8 tiles
 *    tile_list[0..num_tiles), each named by its index ty * ceil(width / 8) + tx in the image and listed at
 *    most once.  This is the form cost-balanced ownership over GPUs uses (rt_partition_tiles below).
 * d_prev (nullable = zeros) is always a full W*H*3 frame.  If compact == 0, d_out is a full frame and only
 * the owned pixels are written; if compact != 0, d_out holds only what the call owns: the owned bands back
 * to back (band k of this rank at row k*band_rows: the shape an all-gather wants), or the listed tiles back
 * to back (tile k at floats [192 k, 192 k + 192): its 64 pixels row by row; slots of a ragged edge tile that
 * lie outside the image are never written).
 * tile_cost, tile_peak (nullable, with a tile list only): per listed tile, its cost and the cost of its most
 * expensive pixel as rt_tile_costs reported them for an earlier launch of the same view; the launch is then
 * scheduled longest job first at once instead of measuring the tiles itself first (tile_peak == NULL: ordered
 * by tile_cost).  The arrays are host memory, read during the call.
 * The launch is asynchronous on `hip_stream` (a hipStream_t, NULL = default stream). */
typedef struct rt_tile_spec {
    int32_t band_rows;       /* > 0, multiple of 8 */
    int32_t band_first;
    int32_t band_stride;
    int32_t compact;
    const uint32_t *tile_list;
    const uint32_t *tile_cost;
    const uint32_t *tile_peak;
    int32_t num_tiles;
} rt_tile_spec;

rt_status rt_render_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                           int32_t time_ms, int32_t frame_num, const rt_tile_spec *tiles,
                           const float *d_prev, float *d_out, void *hip_stream);

/* n_frames (1..32) consecutive progressive frames of one view in ONE launch: what the reference's main
 * loop (src/main.cu:415-431) does with one render() per frame - frames frame_num, frame_num + 1, ...,
 * seeded with times_ms[0..n_frames) - accumulated IN PLACE in d_frame (same layout as d_out above; when
 * frame_num > 0 its content is the image after frame_num - 1, otherwise it is ignored).  The result is
 * bit-identical to n_frames rt_render_device calls.  Every frame has its own random stream, so frame
 * k + 1 of a pixel is traced while the expensive pixels of frame k are still running; each frame stores
 * its per-pixel mean into a scratch plane and a small kernel behind the render kernel folds the planes
 * into d_frame in frame order ((c + prev * n) / (n + 1), src/raytracer.cu:109-112).  A launch per frame
 * leaves most of the GPU idle while the few most expensive tiles finish.  The context
 * keeps n_frames planes of the frame's size in HBM. */
rt_status rt_render_device_batch(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                 const int32_t *times_ms, int32_t n_frames, int32_t frame_num, const rt_tile_spec *tiles,
                                 float *d_frame, void *hip_stream);
/* Pipelined frames: the reference's main loop (src/main.cu:415-431: seed from the wall clock, render(), draw, poll) with the next
 * frame's launch issued BEFORE the previous frame is waited for.  A 1920x1080x1024-spp frame is as long as its most expensive
 * pixel - half of it runs on a nearly empty GPU - and rt_render_device_batch only fills that time when the
 * seeds of the coming frames are known in advance, which a loop that draws each seed at call time cannot offer.  Here it can:
 *   rt_frame_submit   queues ONE frame seeded with time_ms on a stream of the context's own (up to rt_frame_depth submitted
 *                     and not yet collected; RT_ERR_BUSY beyond).  The frame's per-pixel means go to a plane the context keeps;
 *                     nothing the caller owns is touched.  Frames in flight run side by side on the GPU.
 *   rt_frame_collect  takes the OLDEST submitted frame and folds it into d_frame as progressive frame `frame_num`
 *                     ((c + prev * frame_num) / (frame_num + 1), src/raytracer.cu:109-112; d_frame has the layout of
 *                     rt_render_device's d_out for the tile spec the frame was submitted with, and is ignored as input when
 *                     frame_num == 0).  Asynchronous: the fold runs behind the frame's render kernel and behind whatever the caller
 *                     has queued on `hip_stream` so far, and work queued on `hip_stream` afterwards sees the folded frame.
 *                     d_frame == NULL discards the frame (the camera moved: the reference restarts at frame 0,
 *                     src/main.cu:392-407).  Frames submitted with a tile LIST must be collected (or discarded) before frames of
 *                     another list are submitted (RT_ERR_BUSY).
 * Frames are collected in submission order, and the image after collecting frames 0..k is bit-identical to k + 1 calls of
 * rt_render_device with the same seeds (tests/test_gpu_pipeline.py).  The loop becomes
 *     submit(t0); for (;;) { submit(now()); collect(n++, d_frame, s); draw(d_frame); }
 * i.e. the picture on screen lags the newest seed by the frames in flight.  Measured (monkey, 1920x1080x1024 spp, bench.py
 * "pipelined"): 8,950 Msamples/s with 4 frames in flight and 9,800 with 8, against 4,600 one launch at a time and 10,800 for
 * rt_render_device_batch.
 * A view's first frame or two (new scene / camera / size / tile spec) run alone: they measure the tiles and sort the schedule,
 * and the host waits for the frames in flight before it rewrites either.  rt_last_kernel_ms does not see pipelined frames;
 * rt_ctx_synchronize waits for them; launches of the other entry points are queued behind them. */
#define RT_PIPELINE_DEPTH 8            /* at most */
#define RT_PIPELINE_DEFAULT_DEPTH 4
/* How many frames the caller is going to keep in flight (1..RT_PIPELINE_DEPTH; a context starts with RT_PIPELINE_DEFAULT_DEPTH):
 * rt_frame_submit refuses more, and - for scenes whose workgroup has a CU to itself, i.e. a mesh that fills the LDS - every frame is
 * launched on 1 / depth of the GPU's CUs: `depth` frames side by side, each bound by its work instead of by its longest pixel (alone
 * on the GPU a frame leaves most CUs idle for half its duration).  Other scenes' launches are full size and share the CUs.
 * Throughput grows with the depth, and so does a frame's latency (depth x the time per frame); 2, 4 and 8 are the useful values
 * (the depths in between measure no better than the next lower one).  depth 1 is rt_render_device with a plane in between.
 * The context keeps one plane (12 bytes per pixel of the launch's layout) per frame in flight.  Only while no frame is in flight
 * (RT_ERR_BUSY otherwise). */
rt_status rt_frame_depth(rt_ctx *ctx, int32_t depth);
rt_status rt_frame_submit(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                          int32_t time_ms, const rt_tile_spec *tiles);
rt_status rt_frame_collect(rt_ctx *ctx, int32_t frame_num, float *d_frame, void *hip_stream);
/* Host-buffer form of rt_frame_collect for whole frames (submitted with tiles == NULL), with rt_render's contract: previous_render
 * (W*H*3 floats) is read (when *frame_num > 0), blended with the oldest submitted frame and overwritten; *frame_num is incremented.
 * Returns when the frame is in previous_render; the younger frames keep running.  previous_render == NULL discards the frame. */
rt_status rt_frame_collect_host(rt_ctx *ctx, int32_t *frame_num, float *previous_render);
/* frames submitted and not collected */
int32_t rt_frames_pending(const rt_ctx *ctx);
/* blocks until the frame collected last has been folded into its d_frame (what a host that draws the frame itself waits for:
 * the cudaDeviceSynchronize of src/dispatch.cu:141 for this loop) - the younger frames keep running */
rt_status rt_frame_wait(rt_ctx *ctx);

/* ---- camera sequences: many views of a scene in one launch ---------------------------------------
 * Everything above that keeps the GPU full renders many frames of ONE view; a caller whose camera moves (the reference's main loop with its
 * WASD / arrow keys, src/main.cu:373-407; a turntable, a fly-through, a stereo pair, the six faces of a cube map, a light field) starts
 * every frame cold and alone, and a launch that runs alone is as long as its longest pixel.  Here one launch renders n_views views:
 * view i has the camera cams[i] and the seed times_ms[i] (the stream of rt_render_device: state = (uint32)((py * W + px) * 3) * 3145739u +
 * (uint32)times_ms[i] * 6291469u, src/raytracer.cu:127), and every view's expensive tiles start at once.  All cameras share cams[0]'s
 * width and height; whole images only (there is no tile spec).  Two modes:
 *   accumulate == 0, separate frames: d_frames is n_views full W*H*3 frames back to back; frame i is, as uint32, what
 *     rt_render_device(cams[i], times_ms[i], frame_num = 0, tiles = NULL, d_prev = NULL) writes - that is (c + 0 * 0) / 1 of the pixel's
 *     mean c with a NaN stored as the canonical quiet NaN 0x7FC00000 (so a mean of -0 comes out +0).  d_frames is never read; frame_num
 *     must be 0.
 *   accumulate != 0, one frame: d_frames is ONE W*H*3 frame; view i is progressive frame frame_num + i, folded in order with
 *     (c + prev * n) / (n + 1) (src/raytracer.cu:109-112): as uint32 what n_views chained calls of rt_render_device give, and with n_views
 *     identical cameras what rt_render_device_batch gives.  The frame's content is ignored when frame_num == 0.  Cameras that differ by a
 *     lens offset (rt_camera_lens) make this depth of field; cameras along a path, camera motion blur.
 * Device form: n_views is 1 .. RT_VIEWS_MAX, and when accumulating at most rt_max_batch_frames (the context keeps one plane per view).
 * Asynchronous on hip_stream and ordered like rt_render_device: one launch in flight per context, queued behind frames in flight.
 * rt_last_kernel_ms reports it from the render kernel to the last fold.  The launch runs on a guessed schedule built from every view's own
 * centre rays (no pilot, no cost collection) and does not touch the context's cached view: a warm view stays warm, rt_tile_costs answers as
 * before.  RT_ERR_INVALID: a null ctx, scene, cams, times_ms, rs or d_frames; a scene of another context; n_views out of range; a
 * negative frame_num, or a non-zero one with accumulate == 0; a negative rays_per_pixel or reflection_limit; a bad image size; a camera
 * whose width or height differs from cams[0]'s.  A refused call touches nothing. */
#define RT_VIEWS_MAX 32                /* = the frames of one multi-frame launch: views one launch renders */
rt_status rt_render_views_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms,
                                 int32_t n_views, const rt_render_settings *rs, int32_t accumulate, int32_t frame_num,
                                 float *d_frames, void *hip_stream);
/* Host-buffer form: frames is host memory (n_views frames, or one); any n_views >= 1, rendered in launches of up to the device form's
 * limit.  When accumulating, frames is read (if *frame_num > 0) and *frame_num advances by n_views; otherwise *frame_num must be 0 and
 * stays 0.  Returns when frames is filled.  A null frame_num is RT_ERR_INVALID too. */
rt_status rt_render_views(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms,
                          int32_t n_views, const rt_render_settings *rs, int32_t accumulate, int32_t *frame_num, float *frames);
/* One thin-lens sample of a pinhole camera: the image plane moved out to the focus distance and the eye moved by (lens_u, lens_v) on the
 * lens, along the camera's own axes.  focal_len is what the caller gave rt_camera_make (0.1 for rt_camera_default).  Defined in binary32,
 * every operation rounded once, in this order, nothing fused (k over x, y, z; du = cam->delta_u, dv = cam->delta_v):
 *     s = focus_dist / focal_len
 *     out.delta_u.k = du.k * s;   out.delta_v.k = dv.k * s
 *     out.tl_pixel_pos.k = (tl_pixel_pos.k - cam_pos.k) * s + cam_pos.k
 *     eu.k = du.k * (1.0f / sqrtf((du.x*du.x + du.y*du.y) + du.z*du.z));   ev likewise from dv
 *     out.cam_pos.k = (eu.k * lens_u + ev.k * lens_v) + cam_pos.k
 * width and height are copied; out may be cam.  So tl_pixel_pos, delta_u and delta_v of the result do not depend on the offset: every
 * sample's ray of pixel (px, py) passes through the same point of the focus plane, and rt_render_views with accumulate != 0 over n such
 * cameras is a depth-of-field frame of n lens samples.  RT_ERR_INVALID (out untouched): a null pointer, a focal_len or focus_dist that is
 * not positive and finite, an offset that is not finite, a delta_u or delta_v of length 0. */
rt_status rt_camera_lens(const rt_camera *cam, float focal_len, float focus_dist, float lens_u, float lens_v, rt_camera *out);

/* ---- environment lighting: a cube-map sky ------------------------------------------------------
 * Everywhere else a ray that leaves the scene sees one constant, rt_render_settings::sky_colour.  Here it sees a texel of a cube map: six
 * square faces of n x n texels, 1 <= n <= RT_SKY_MAX_FACE, three binary32 values each.  No texel value is inspected: HDR values, Inf and
 * NaN pass through.  The faces are numbered 0..5 = +X, -X, +Y, -Y, +Z, -Z; the caller's array is faces[face][row][col][3], row-major.
 * (A cube map and not a latitude / longitude image: the lookup is compares, two divisions, two multiply-adds and two conversions, once per
 * sample, and needs no inverse trigonometric function.)
 *
 * Lookup of a direction d = (x, y, z) - the ray's direction at the miss, the jittered, renormalised direction it was traced with.  Every
 * operation is binary32, rounded once, nothing fused:
 *     ax = |x|, ay = |y|, az = |z|
 *     axis = (ax >= ay && ax >= az) ? X : (ay >= az ? Y : Z)          (a NaN compares false)
 *     c = d[axis];  m = |c|;  face = 2 * axis + (c < 0 ? 1 : 0)       (-0 is the positive face)
 *     (a, b) = the other two components in cyclic order: X: (y, z)   Y: (z, x)   Z: (x, y)
 *     s = a / m;  t = b / m
 *     col = clamp(f2i((s * 0.5f + 0.5f) * (float)n), 0, n - 1)        (mul, add, mul: three roundings)
 *     row = clamp(f2i((t * 0.5f + 0.5f) * (float)n), 0, n - 1)
 *     texel = faces[face][row][col]
 * f2i converts towards zero, saturating, NaN -> 0.  The miss then adds, per channel, L = texel * sky_colour (one rounding) as
 * fin = fin + L * thr: the renderer's own line with L in the place of sky_colour.  So rs->sky_colour is the map's tint and exposure,
 * (1,1,1) leaves the map as it is, and two identities hold as uint32: a map of all 1.0f renders what rt_render_views_device renders with the
 * same sky_colour, and a constant map c with tint s renders what sky_colour = fl(c * s) renders.
 *
 * The inverse mapping, for filling a map from any function of direction: rt_sky_texel_direction gives the direction through the centre of
 * texel (face, row, col) of an n-face map:
 *     s = ((float)col + 0.5f) / (float)n * 2.0f - 1.0f                 (t from row likewise)
 * the major component is +1 or -1 and s, t are placed by the table above; the result is not normalised.  The lookup of that direction is
 * (face, row, col) again - also of the direction normalised, and of the direction scaled by 1e-3f.  RT_ERR_INVALID: a null out, a
 * face_size outside 1 .. RT_SKY_MAX_FACE, a face outside 0 .. 5, a row or col outside 0 .. face_size - 1 (out untouched). */
typedef struct rt_sky rt_sky;
#define RT_SKY_MAX_FACE 2048
/* faces_rgb is host memory, 6 * face_size * face_size * 3 floats; it is copied and uploaded, and the call returns when the copy is done.
 * The sky belongs to ctx.  RT_ERR_INVALID: a null ctx, faces_rgb or out; face_size out of range. */
rt_status rt_sky_create(rt_ctx *ctx, int32_t face_size, const float *faces_rgb, rt_sky **out);
/* waits for the context's launches first, as rt_ctx_synchronize does; destroy a context's skies before the context */
void rt_sky_destroy(rt_sky *sky);
rt_status rt_sky_texel_direction(int32_t face_size, int32_t face, int32_t row, int32_t col, float out[3]);
/* rt_render_views_device with a sky: its modes, limits, seeds, schedule, launch order and rt_last_kernel_ms window, and like it the call
 * leaves the context's cached view alone.  One camera repeated is a progressive batch of a still view; n_views = 1 is a single frame.
 * RT_ERR_INVALID: everything rt_render_views_device refuses, a null sky, a sky of another context.  A refused call touches nothing. */
rt_status rt_render_sky_device(rt_ctx *ctx, const rt_scene *scene, const rt_sky *sky, const rt_camera *cams, const int32_t *times_ms,
                               int32_t n_views, const rt_render_settings *rs, int32_t accumulate, int32_t frame_num,
                               float *d_frames, void *hip_stream);
/* Host-buffer form, with rt_render_views' contract */
rt_status rt_render_sky(rt_ctx *ctx, const rt_scene *scene, const rt_sky *sky, const rt_camera *cams, const int32_t *times_ms,
                        int32_t n_views, const rt_render_settings *rs, int32_t accumulate, int32_t *frame_num, float *frames);

/* number of rows a rank owns under a band tile spec (host helper for sizing compact buffers) */
int32_t rt_tile_owned_rows(const rt_tile_spec *tiles, int32_t height);

/* What the tiles of this context's current view cost: the first launch of a view (scene, camera, image size,
 * tile spec) adds up, per tile, the work of its pixels (traversal steps, generated rays and shaded hits,
 * weighted); this call waits for that launch and copies the figures out: tile_ids[i] = the tile's index in
 * the image (ty * ceil(width / 8) + tx), costs[i] its cost (opaque units; bit 0 says whether a ray of the tile
 * entered a mesh), peaks[i] (nullable) the cost of its most expensive pixel, for i < *count (= the tiles of
 * that launch, at most `capacity`).  The sum is what balances GPUs (rt_partition_tiles), the peak what orders
 * a launch: a tile of one frame is a job as long as its longest pixel, and the longest jobs must start first.  RT_ERR_INVALID if no launch of the current view has collected costs.  The reference
 * has no counterpart (one GPU, one thread per pixel, src/dispatch.cu:136-139); this is what lets N GPUs
 * share a frame by cost instead of by area. */
rt_status rt_tile_costs(rt_ctx *ctx, uint32_t *tile_ids, uint32_t *costs, uint32_t *peaks, int32_t capacity, int32_t *count);

/* Ownership of the tiles_x x tiles_y tiles of an image over n_ranks GPUs: owner[ty * tiles_x + tx] = rank.
 * cost == NULL: interleaved, owner = (tx + ty) % n_ranks (what a view's first, cost-collecting launch uses).
 * Otherwise cost[tile] is its measured cost (rt_tile_costs, summed over the ranks that rendered the view)
 * and tiles are dealt longest-processing-time-first: by decreasing cost, each to the rank with the least
 * cost so far (ties: the lower tile index first, the lower rank).  Deterministic: every rank that calls it
 * with the same costs gets the same owners.  Any partition renders the same image (a pixel depends only on
 * its index, seed and previous value, src/raytracer.cu:118-131). */
rt_status rt_partition_tiles(const uint32_t *cost, int32_t tiles_x, int32_t tiles_y, int32_t n_ranks, int32_t *owner);

/* The exchange step for tile lists on one GPU: copies between a compact image (the listed tiles back to
 * back, as a compact tile-list render writes them) and a full W*H*3 frame, both on ctx's GPU, asynchronously
 * on hip_stream.  to_frame != 0: frame <- compact (what the root does with every rank's gathered tiles);
 * to_frame == 0: compact <- frame (handing the image so far to its owners).  tile_list is host memory. */
rt_status rt_tiles_copy_device(rt_ctx *ctx, float *d_compact, float *d_frame, int32_t width, int32_t height,
                               const uint32_t *tile_list, int32_t num_tiles, int32_t to_frame, void *hip_stream);

/* How many progressive frames the multi-frame entry points put into one launch for an image of this size on
 * this context's GPU: at most 32, fewer when that many per-frame planes (12 bytes per pixel each) would take
 * more than a quarter of the GPU's memory. */
int32_t rt_max_batch_frames(rt_ctx *ctx, int32_t width, int32_t height);

/* Kernel timing by HIP events recorded on the launch stream around the render kernel of the
 * most recent rt_render / rt_render_device call; blocks until that kernel has finished. */
rt_status rt_last_kernel_ms(rt_ctx *ctx, float *ms);
/* Blocks until the most recent launch of this context has finished and returns its status: the
 * cudaDeviceSynchronize + cudaPeekAtLastError pair of src/dispatch.cu:141,161 for callers of the
 * asynchronous device-buffer entry points. */
rt_status rt_ctx_synchronize(rt_ctx *ctx);

/* ---- closest-hit ray queries and first-hit planes ------------------------------------------------
 * What get_ray_collision (src/raytracer.cu:24-46) answers for one ray, for n rays at once, with the hit written out instead
 * of shaded: picking, focus, visibility and collision probes need a closest hit and no path.  The rules are the render
 * kernel's (objects in list order, the later one wins a tie; one-way quads; the BVH meshes), the bits are the reference
 * algorithm's (tests/test_gpu_query.py: equal to the CPU oracle's orc_trace_one as uint32, not to a tolerance).
 * The ray is taken as given (Ray::change_direction src/ray.cu:198-202): the direction is NOT normalised and the distance is in
 * units of its length; a direction with a NaN component hits nothing. */
typedef struct rt_hit {
    float t;               /* distance along the ray; RT_HIT_MISS_T for a miss */
    float point[3];        /* direction * t + origin (Ray::get_pos src/ray.cu:63-65) */
    float normal[3];       /* the shading normal: sphere normalised(point - centre) (src/objects.cu:66); triangle its unit normal, negated when it faces along the ray (:158) */
    int32_t object;        /* index in the scene's object list (call order of rt_scene_add_*); -1: a miss */
    int32_t triangle;      /* index of the triangle in the flattened scene (rt_debug_flatten order); -1 for a sphere or a miss */
    float u, v;            /* texture coordinates when the object's material needs them (rt_material.need_uv; src/objects.cu:82-97, :196-199), else 0 */
    int32_t reserved;      /* 0 */
} rt_hit;                  /* 48 bytes.  A miss is {RT_HIT_MISS_T, {0,0,0}, {0,0,0}, -1, -1, 0, 0, 0} bit for bit */
#define RT_HIT_MISS_T 1073741824.0f   /* the reference's "infinity", `1 << 31 - 1` == 1 << 30 (src/objects.cu:6) */

/* Device-buffer form: d_origins, d_directions (n x 3 floats each) and d_hits (n records, 16-byte aligned) are device memory of
 * ctx's GPU; asynchronous on hip_stream and ordered like rt_render_device (one launch in flight per context).  n == 0 succeeds
 * and touches nothing; n < 0, n > 2^30, a null pointer with n > 0, a misaligned d_hits and a scene committed on another context
 * are RT_ERR_INVALID.  rt_last_kernel_ms then reports the query kernel.  The grid grows with n (a wave per 64 rays, up to every
 * CU filled): a few rays stage the scene into LDS once, not once per CU. */
rt_status rt_trace_rays_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions, int64_t n,
                               rt_hit *d_hits, void *hip_stream);
/* Host-buffer form: uploads the rays, traces, downloads the records and returns when they are in `hits` (the context keeps the
 * device buffers). */
rt_status rt_trace_rays(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, int64_t n, rt_hit *hits);

/* The first-hit planes of a view (what a denoiser, an edge-aware filter or a compositor wants beside the colour): for every pixel
 * the renderer's primary ray with antialiasing off (normalised((tl_pixel_pos + (delta_u * px + delta_v * py)) - cam_pos),
 * src/camera.cu:24-29, src/raytracer.cu:123-127), its closest hit, and the planes below in rt_render's full-frame row-major
 * layout.  Every plane is optional: a NULL pointer is not written; all NULL is RT_ERR_INVALID.
 *   depth   W*H   floats   rt_hit.t                                                          miss: RT_HIT_MISS_T
 *   normal  W*H*3 floats   rt_hit.normal                                                     miss: 0, 0, 0
 *   albedo  W*H*3 floats   what trace_ray (src/raytracer.cu:86-90) does with the first hit:  miss: sky_colour
 *                          the material's texture colour at (u, v) that multiplies the
 *                          throughput; for an emissive material the emitted light it adds
 *   object  W*H   int32    rt_hit.object                                                     miss: -1
 *   ray     W*H*3 floats   the primary direction itself (origin cam_pos): rt_trace_rays on these rays gives these planes
 * Device-buffer form: the planes are device memory; asynchronous on hip_stream like rt_render_device. */
rt_status rt_render_aov_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float sky_colour[3],
                               float *d_depth, float *d_normal, float *d_albedo, int32_t *d_object, float *d_ray, void *hip_stream);
/* Host-buffer form: returns when the requested planes are in host memory. */
rt_status rt_render_aov(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float sky_colour[3],
                        float *depth, float *normal, float *albedo, int32_t *object, float *ray);

/* ---- nearest-surface queries: closest point and distance ------------------------------------------
 * "How far is this point from the scene, and where is the closest surface point?" - the question a particle, a cloth vertex, a
 * distance-field bake or a snap-to-surface asks, which no ray answers: a ray probes one direction somebody chose.  For n points at
 * once, over the records the kernels read (rt_debug_flatten: spheres (c, r), triangles (p0, s1, s2), the meshes' trees).  The
 * distance is UNSIGNED; its sign - inside or outside - comes from the winding-number queries below (rt_signed_distance).
 *
 * The result is DEFINED, not approximated: binary32 + - * / sqrt, comparisons and selects, every operation rounded once (no fused
 * multiply-add), in the order written here, so tests/nearest_ref.py (NumPy float32, every candidate of every point, no traversal)
 * gives the same bytes.  dot(a, b) = (ax*bx + ay*by) + az*bz; sq(a) = dot(a, a).
 *
 * Candidates: every object of the scene, for the point p.
 *   sphere (c, r):   v = p - c; l = sqrt(sq(v)); s = l - r; d2 = s*s; point = c + v * (r / l) (the quotient first, then three
 *                    products, then three sums); for l == 0, point = c + (r, 0, 0).  triangle = -1.
 *   triangle record (p0, s1, s2) - a loose triangle, the two of a quad (a one-way quad counts from both sides), the twelve of a
 *   cuboid, every triangle of a mesh: the closest point of the triangle by the region test of Ericson, Real-Time Collision Detection
 *   5.1.5, with a = p0, ab = s1, ac = s2 on the record as stored (the second and third vertex are not formed again):
 *                    ap = p - p0; bp = ap - s1; cp = ap - s2;
 *                    d1 = dot(s1, ap); d2 = dot(s2, ap); d3 = dot(s1, bp); d4 = dot(s2, bp); d5 = dot(s1, cp); d6 = dot(s2, cp);
 *                    vc = d1*d4 - d3*d2; vb = d5*d2 - d1*d6; va = d3*d6 - d5*d4;
 *                    the first of these that holds gives the barycentrics (v, w):
 *                      d1 <= 0 and d2 <= 0                        (0, 0)
 *                      d3 >= 0 and d4 <= d3                       (1, 0)
 *                      vc <= 0 and d1 >= 0 and d3 <= 0            (d1 / (d1 - d3), 0)
 *                      d6 >= 0 and d5 <= d6                       (0, 1)
 *                      vb <= 0 and d2 >= 0 and d6 <= 0            (0, d2 / (d2 - d6))
 *                      va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
 *                      otherwise                                  k = 1 / ((va + vb) + vc), v = vb * k, w = vc * k
 *                    q = s1*v + s2*w (per component: two products, one sum); point = p0 + q; r = ap - q; dist2 = sq(r).
 *                    (A comparison with a NaN does not hold; a NaN then reaches dist2.)
 *   a mesh's triangle, additionally: dist2 = B where dist2 < B, with B the largest BOX DISTANCE over the boxes on the path from the
 *   mesh's root box to the triangle's leaf (the root box, then the child box stored in each node on the way down).  The box distance
 *   of (lo, hi): per axis e = max(max(lo - p, p - hi), 0), then sq(e).  Rounded subtraction, squaring and addition are monotone, so an
 *   enclosing box never computes a larger distance than a box inside it, and a candidate that is by definition no nearer than every box
 *   on its path can be pruned by "this subtree's path value is greater than the best so far" without an error analysis: the result
 *   is the exhaustive minimum in whatever order a traversal visits the tree.  The clamp only bites where rounding put a triangle's
 *   dist2 a few ulps under a bound that exact arithmetic guarantees.
 * Winner: the smallest dist2; on equal dist2 the lower object index, then the lower triangle index; a NaN dist2 never wins.  With a
 * limit max_dist a candidate needs dist2 <= max_dist * max_dist (one rounding); +Inf, or no limit array, is unbounded; a limit that
 * is NaN or below zero gives a miss; so does a point with a NaN or infinite coordinate. */
typedef struct __attribute__((aligned(16))) rt_nearest {
    float distance;        /* sqrt(distance2), correctly rounded; RT_HIT_MISS_T for a miss */
    float distance2;       /* the winner's dist2; RT_HIT_MISS_T for a miss */
    float point[3];        /* the closest surface point */
    int32_t object;        /* index in the scene's object list, as rt_hit.object; -1: a miss */
    int32_t triangle;      /* index of the triangle in the flattened scene, as rt_hit.triangle; -1 for a sphere or a miss */
    int32_t reserved;      /* 0 */
} rt_nearest;              /* 32 bytes.  A miss is {RT_HIT_MISS_T, RT_HIT_MISS_T, {0,0,0}, -1, -1, 0} bit for bit */

/* Device-buffer form: d_points (n x 3 floats), d_max_dist (n floats, or NULL: unbounded) and d_out (n records, 16-byte aligned) are
 * device memory of ctx's GPU; asynchronous on hip_stream and ordered like rt_trace_rays_device (one launch in flight per context).
 * n == 0 succeeds and touches nothing; n < 0, n > 2^30, a null pointer (other than d_max_dist) with n > 0, a misaligned d_out and a
 * scene committed on another context are RT_ERR_INVALID and leave the launch order as it was.  rt_last_kernel_ms then reports the
 * kernel.  A scene updated by rt_scene_update_mesh_device answers for its new geometry. */
rt_status rt_nearest_points_device(rt_ctx *ctx, const rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n,
                                   rt_nearest *d_out, void *hip_stream);
/* Host-buffer form: uploads the points (and limits), answers, downloads the records and returns when they are in `out`. */
rt_status rt_nearest_points(rt_ctx *ctx, const rt_scene *scene, const float *points, const float *max_dist, int64_t n, rt_nearest *out);

/* ---- winding-number queries: point containment and signed distance -------------------------------
 * "Is this point inside?" - what a voxeliser, a particle or cloth step, a CSG preview and a signed distance field need, and what no
 * count of ray crossings answers here: the strict slab test drops hits, a sphere offers one root, and meshes from files are not
 * watertight.  The answer that survives open, overlapping and leaky meshes is the GENERALIZED WINDING NUMBER (Jacobson, Kavan,
 * Sorkine-Hornung 2013): the signed solid angle the surface subtends at the point over 4 pi, 1 inside a closed surface, 0 outside, a
 * fraction near a hole.  Per triangle it is the angle of Van Oosterom and Strackee 1983, summed over the triangle records the kernels
 * read (rt_debug_flatten).
 *
 * Orientation.  The stored records do not all turn the way their faces do: the second triangle of every quad is stored as
 * (p1, p4, p3), against the first (p1, p2, p3).  So a quad's second record counts negated, and for a mesh the builder keeps one FLIP
 * bit per triangle - 1 for the second triangle of a quad face of an .obj, 0 for a triangle face and for every triangle of
 * rt_scene_add_mesh, whose orientation is the caller's - which follows the triangle through the tree build and through
 * rt_scene_update_mesh[_device] (rt_flat_view.tri_flip).
 *
 * The result is DEFINED, like the nearest-surface record: binary32 + - * / sqrt, comparisons and selects, every operation rounded once
 * (no fused multiply-add), in the order written here, so tests/winding_ref.py (NumPy float32) gives the same bytes.
 * dot(a, b) = (ax*bx + ay*by) + az*bz; sq(a) = dot(a, a).
 *
 * rt_wn_atan2(y, x), no libm:  ay = |y|; ax = |x|; steep = ay > ax; mn = steep ? ax : ay; mx = steep ? ay : ax; q = mn / mx; s = q*q;
 *   P = C8; P = P*s + C7; ... P = P*s + C0 (Horner, RT_WN_C8 down to RT_WN_C0); r = q*P; r = steep ? RT_WN_PI_2 - r : r;
 *   r = x < 0 ? RT_WN_PI - r : r; result = y < 0 ? -r : r (the sign bit flipped).  The coefficients are a minimax fit of atan on [0, 1]
 *   rounded to binary32 (on [0, 1] the polynomial is within 1.72 * 2^-24 of atan); measured against binary64's atan2 over 10^7 random
 *   arguments the result is within 5.1 * 2^-24 (absolute, radians) - most of it the spacing 2^-22 of the results near pi and the
 *   rounding of pi itself (tests/winding_ref.py atan2_error, tests/golden/winding_meta.json).
 * Term of a triangle record (p0, s1, s2) for the point p:
 *   a = p0 - p; b = a + s1; c = a + s2; la = sqrt(sq(a)); lb = sqrt(sq(b)); lc = sqrt(sq(c));
 *   nrm = (s1.y*s2.z - s1.z*s2.y, s1.z*s2.x - s1.x*s2.z, s1.x*s2.y - s1.y*s2.x); det = dot(a, nrm);
 *   den = ((la*lb)*lc + dot(a, b)*lc) + (dot(a, c)*lb + dot(b, c)*la);
 *   t = 0.0f where det == 0 (the point lies in the triangle's plane: both sides count evenly), else rt_wn_atan2(det, den);
 *   term = t, or -t (the sign bit flipped) where the record's sign is -1.
 * Winding number of an object: A = 0.0f; A = A + term over its records in ascending flattened index; w = A * RT_INV_2PI.
 *   mesh:                every record of its range, signed by the flip bit (-1 where it is 1)
 *   loose triangle:      its one record, +
 *   quad, one-way quad:  its two records, the second negated
 *   sphere (c, r):       no record: 1.0f where sq(p - c) < r*r, else 0.0f
 *   cuboid:              no record is summed (its near and far faces are stored with the same orientation): 1.0f where lo < p < hi
 *                        strictly on all three axes, else 0.0f, lo and hi being the componentwise min and max of p0 over its twelve
 *                        records (every corner coordinate occurs among them)
 * object >= 0: the answer is that object's w; an open surface (a loose triangle, a quad) gives the fractional value.
 * object == RT_WINDING_SOLIDS: w = 0.0f; w = w + w_obj over the spheres, cuboids and meshes in list order (loose triangles and quads
 * are skipped: they enclose nothing).
 * A point with a NaN or infinite coordinate, and a sum that is a NaN, give w = 0x7FC00000.
 * inside = |w| >= 0.5f (an inverted mesh still encloses; a NaN is outside).  sdf = inside ? -distance : distance with `distance` from the
 * rt_nearest record of the same point and w of RT_WINDING_SOLIDS; a miss under a limit gives -RT_HIT_MISS_T or RT_HIT_MISS_T.
 * The sum is sequential per point and linear in the triangles: a few points against a very large mesh are slow. */
#define RT_WINDING_SOLIDS (-1)
#define RT_WN_C0 0x1.fffffcp-1f
#define RT_WN_C1 (-0x1.555368p-2f)
#define RT_WN_C2 0x1.994fb6p-3f
#define RT_WN_C3 (-0x1.2205ap-3f)
#define RT_WN_C4 0x1.ae096ep-4f
#define RT_WN_C5 (-0x1.2856fcp-4f)
#define RT_WN_C6 0x1.45e34ap-5f
#define RT_WN_C7 (-0x1.d7e76p-7f)
#define RT_WN_C8 0x1.420206p-9f
#define RT_WN_PI 0x1.921fb6p+1f         /* pi, pi / 2 and 1 / (2 pi) as the nearest binary32 values */
#define RT_WN_PI_2 0x1.921fb6p+0f
#define RT_INV_2PI 0x1.45f306p-3f
/* Device-buffer form: d_points (n x 3 floats), d_winding (n floats) and d_inside (n bytes, 0 or 1) are device memory of ctx's GPU;
 * either output may be NULL, not both.  Asynchronous on hip_stream and ordered like rt_nearest_points_device (one launch in flight per
 * context).  n == 0 succeeds and touches nothing; n < 0, n > 2^30, null points or both outputs null with n > 0, an `object` that is
 * neither RT_WINDING_SOLIDS nor an index of the scene's object list and a scene committed on another context are RT_ERR_INVALID and
 * leave the launch order as it was.  The scene's first winding query uploads its flip bytes (and its triangle order, unless an update
 * already has) before it returns.  rt_last_kernel_ms then reports the kernel.  A scene updated by rt_scene_update_mesh[_device] answers
 * for its new geometry. */
rt_status rt_winding_numbers_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, int64_t n, int32_t object, float *d_winding,
                                    uint8_t *d_inside, void *hip_stream);
/* Host-buffer form: uploads the points, answers, and returns when the outputs that are not NULL are in host memory. */
rt_status rt_winding_numbers(rt_ctx *ctx, rt_scene *scene, const float *points, int64_t n, int32_t object, float *winding, uint8_t *inside);
/* The signed distance of n points: rt_nearest_points_device's launch (d_max_dist: n limits, or NULL) into d_nearest (n records, 16-byte
 * aligned; NULL: a buffer of the context's), then the winding kernel over RT_WINDING_SOLIDS, which reads the records and writes d_sdf (n
 * floats) - both on hip_stream, as ONE launch of the context's launch order; rt_last_kernel_ms reports the two together.  Refusals as
 * above; d_sdf may not be NULL. */
rt_status rt_signed_distance_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n,
                                    rt_nearest *d_nearest, float *d_sdf, void *hip_stream);
/* Host-buffer form: `nearest` (n records) may be NULL. */
rt_status rt_signed_distance(rt_ctx *ctx, rt_scene *scene, const float *points, const float *max_dist, int64_t n, rt_nearest *nearest,
                             float *sdf);

/* ---- fast winding numbers: a dipole cluster tree per mesh ----------------------------------------
 * The queries above visit every triangle record for every point.  These replace a far CLUSTER of a mesh's triangles by its dipole (Barill,
 * Dickson, Schmidt, Levin, Jacobson 2018, first order): an approximation of the winding number, but again a function DEFINED to the bit -
 * given the cluster tree (reported by rt_debug_winding_tree / rt_debug_scene_winding_tree; the topology is no part of the definition),
 * binary32, nothing fused, in the order written here - so tests/winding_fast_ref.py gives the same bytes.  How far it lies from the exact
 * answer is measured separately (tests/golden/winding_fast_meta.json).  Only an object of type mesh goes through its tree: spheres,
 * cuboids, loose triangles and quads answer exactly as above, so a scene without a mesh answers the exact query's bytes.
 *
 * The tree of a mesh.  Topology: built on the host at the scene's first fast query from the commit-time records in commit order -
 * recursively the axis with the longest extent of the triangle centroids, a stable sort along it, the first ceil(m / 2) triangles to the
 * left, until a set holds at most RT_WINDING_LEAF_TRIS.  Clusters are stored in preorder, left child first (the left child of cluster i
 * is i + 1, the right one skip[i + 1]); skip: the next cluster not in the subtree; a leaf has count > 0 and holds the triangles at
 * positions first .. first + count - 1 of the CLUSTER ORDER, which the order list maps to commit indices.  It never changes afterwards.
 * Moments: recomputed on the device, on the caller's stream ahead of the query, at the first fast query and after every
 * rt_scene_update_mesh[_device] of the scene.
 *   leaf, over its triangles in cluster order: n = (s1.y*s2.z - s1.z*s2.y, s1.z*s2.x - s1.x*s2.z, s1.x*s2.y - s1.y*s2.x), every component's
 *     sign bit flipped where the flip bit is 1; a = sqrt(dot(n, n)); g = p0 + (s1 + s2) * RT_WN_THIRD per component;
 *     Msum = Msum + n; Asum = Asum + a; Gsum = Gsum + a * g (all from 0.0f); lo, hi: from p0 of the first triangle, then over the corners
 *     p0, p0 + s1, p0 + s2 of every triangle in that order lo = c < lo ? c : lo, hi = hi < c ? c : hi per component.
 *   internal cluster: the left child's sums + the right child's, left operand first; lo = R.lo < L.lo ? R.lo : L.lo, hi = L.hi < R.hi ? R.hi : L.hi.
 *   per cluster: c = Asum > 0 ? Gsum / Asum : lo (three divisions); M = 0.25f * Msum (a dipole term is then in the unit of atan2(det, den),
 *     half a solid angle); e_k = (c_k - lo_k) > (hi_k - c_k) ? (c_k - lo_k) : (hi_k - c_k); r2 = dot(e, e).
 * The answer of a mesh whose clusters are [c0, c1) for the point p, beta2 = beta * beta rounded once on the host:
 *   i = c0; A = 0.0f
 *   while i < c1:  d = c_i - p; d2 = dot(d, d)
 *     if d2 > beta2 * r2_i:   A = A + dot(M_i, d) / (d2 * sqrt(d2)); i = skip_i
 *     else if count_i > 0:    A = A + term (negated where the flip bit is 1) over the leaf's triangles in cluster order; i = skip_i
 *     else:                   i = i + 1
 *   w = A * RT_INV_2PI
 * beta = +inf: nothing is far (inf * 0 is a NaN and the compare false), the answer is the exact terms summed in cluster order.  Everything
 * else - the other object types, RT_WINDING_SOLIDS' sum in list order, points that are not finite, a NaN sum, inside, sdf - is as above.
 * A smaller beta visits fewer clusters and errs more; RT_WINDING_BETA_DEFAULT is Barill's 2.  The fast path pays on large meshes; on a mesh
 * of a few hundred triangles the exact query can be as quick (DESIGN.md section 28 has the measurements). */
#define RT_WINDING_LEAF_TRIS 8
#define RT_WINDING_BETA_DEFAULT 2.0f
#define RT_WN_THIRD 0x1.555556p-2f      /* the binary32 nearest to 1 / 3 */
/* As rt_winding_numbers[_device], with `beta` > 0 (+inf allowed; a NaN, zero or a negative beta is RT_ERR_INVALID).  The scene's first fast
 * query also builds and uploads its cluster trees before it returns; a failed allocation leaves the scene as it was. */
rt_status rt_winding_numbers_fast_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, int64_t n, int32_t object, float beta,
                                         float *d_winding, uint8_t *d_inside, void *hip_stream);
rt_status rt_winding_numbers_fast(rt_ctx *ctx, rt_scene *scene, const float *points, int64_t n, int32_t object, float beta, float *winding,
                                  uint8_t *inside);
/* As rt_signed_distance[_device]: the nearest-surface launch, then the fast kernel over RT_WINDING_SOLIDS signing the distance. */
rt_status rt_signed_distance_fast_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n, float beta,
                                         rt_nearest *d_nearest, float *d_sdf, void *hip_stream);
rt_status rt_signed_distance_fast(rt_ctx *ctx, rt_scene *scene, const float *points, const float *max_dist, int64_t n, float beta,
                                  rt_nearest *nearest, float *sdf);

/* ---- multi-hit ray queries: the first k hits of a ray, and hit counts ----------------------------
 * What lies BEHIND the first surface: transparency and x-ray views, the thickness of a part along a ray, "select through" picking,
 * the number of surfaces between two points, crossing counts.  One launch instead of k chained rt_trace_rays calls re-rooted at
 * hit + epsilon, which skip or repeat surfaces and trace rays of other floats than the one asked about.
 *
 * The answer is DEFINED to the bit.  The ray (o, d) is taken as given, as for rt_trace_rays: d is not normalised, t is in units of its
 * length, inv = 1.0f / d per component; a direction with a NaN component has no candidate.  Binary32, nothing fused.
 *
 * Candidates: triples (t, object, triangle) from the tests rt_trace_rays runs (src/objects.cu), on the records of rt_debug_flatten.
 *   sphere:         Sphere::hit's near root, accepted when > 1e-6; triangle = -1.  At most one candidate: the far root (the exit
 *                   point, or the only hit from inside) is OUT OF SCOPE, as it is for rt_trace_rays.
 *   loose triangle: Triangle::hit (Moller-Trumbore, two-sided; t > 1e-6, u >= 0, v >= 0, 1 - u - v >= 0).
 *   quad, one-way quad: Quad::hit's ONE candidate - the first record if it hits, else the second.  A one-way quad offers nothing when
 *                   dot(d, normal) < 0.
 *   cuboid:         each of its six quads offers its one candidate.
 *   mesh:           every triangle record of the mesh that Triangle::hit accepts and whose every box on the path passes the strict slab
 *                   test (BoundingBox::ray_hits: per axis t1 = (lo - o) * inv, t2 = (hi - o) * inv, tmin = max(tmin, min(t1, t2)),
 *                   tmax = min(tmax, max(t1, t2)), from tmin = 0 and tmax = RT_HIT_MISS_T, min / max dropping a NaN operand; passed
 *                   when tmin < tmax and tmax > 0).  The path runs over the flattened tree: the mesh table's root box, then the child
 *                   box stored in each node on the way down to the triangle's leaf.
 * Key: K = max(t, B), with B the largest slab ENTRY DISTANCE tmin over the boxes of the candidate's path, 0 for a candidate of no
 * mesh (tmin starts from 0 and drops NaNs: B is never a NaN).  K orders and limits the candidates; the record reports the raw t, so
 * record 0 stays the float rt_trace_rays reports.  Every candidate below a box has, by definition, a key no smaller than that box's
 * entry distance, so "skip a subtree whose box fails the slab test or whose entry distance is GREATER than the threshold (the limit, or
 * the k-th best key so far)" is exact in whatever order a traversal visits the tree, without an error analysis; a subtree entered AT
 * the threshold must still be visited, because of the tie rule.  The clamp only bites where rounding put a triangle's t a few ulps
 * under the entry distance of a box that contains it: there the reported t of successive records can STEP DOWN by those few ulps.
 * Limit: lim = min(tmax, RT_HIT_MISS_T), or RT_HIT_MISS_T without a limit array; a candidate counts when K <= lim.  A NaN tmax counts
 * nothing (nor does one that is not positive: K > 1e-6).
 * Order: ascending K; on equal K the higher object index first (the reference's "later object wins"), within one object the lower
 * flattened triangle index first.
 * Output, for ray i: d_counts[i] = min(k, candidates that count) for k > 0; for k == 0, COUNT-ONLY mode, the number of ALL candidates
 * that count (nothing is recorded, nothing but the limit prunes).  Records 0 .. count-1 (d_hits[i * k + rank]) are rt_hit records
 * formed exactly as rt_trace_rays forms one for that (t, object, triangle); records count .. k-1 are the miss pattern, bit for bit.
 * Where rt_trace_rays and record 0 can differ: equal t inside one mesh (the reference keeps the first triangle its traversal meets,
 * here the lower index), and where the clamp reorders; tests/golden/multihit_meta.json has the measured share of such rays. */
#define RT_MULTIHIT_MAX 8               /* records per ray, at most */
/* Device-buffer form: d_origins, d_directions (n x 3 floats each), d_tmax (n floats, or NULL), d_hits (n * k records, [ray][rank],
 * 16-byte aligned) and d_counts (n int32, may be NULL when k > 0) are device memory of ctx's GPU; asynchronous on hip_stream and
 * ordered like rt_trace_rays_device.  n == 0 succeeds and touches nothing.  RT_ERR_INVALID, leaving the launch order as it was: n < 0
 * or n > 2^30; k < 0 or k > RT_MULTIHIT_MAX; a null ray pointer with n > 0; d_hits null or misaligned while k > 0; d_counts null
 * while k == 0; a scene of another context; a scene of more than 4,096 objects (an object's index shares a register with the
 * triangle's).  rt_last_kernel_ms then reports the multi-hit kernel. */
rt_status rt_trace_rays_multi_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions,
                                     const float *d_tmax, int64_t n, int32_t k, rt_hit *d_hits, int32_t *d_counts, void *hip_stream);
/* Host-buffer form: uploads the rays (and limits), answers, downloads the records and counts (each where its pointer is not NULL) and
 * returns when they are in host memory (the context keeps the device buffers). */
rt_status rt_trace_rays_multi(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, const float *tmax,
                              int64_t n, int32_t k, rt_hit *hits, int32_t *counts);

/* ---- sphere-cast queries: where a moving ball first touches the scene ------------------------------
 * "How far can a ball of radius r travel along d before it touches anything, and where does it touch?" - what a particle, a cloth
 * vertex, a collision probe, a camera rig and a ball-nose tool path ask.  A ray has no thickness and slips between triangles a ball
 * would hit; a chain of rt_nearest_points launches (step by distance - r, ask again) takes an unbounded number of launches and never
 * ends on the surface.  Here: one call, n balls.
 *
 * The answer is DEFINED to the bit, like the nearest-surface and the multi-hit records: binary32 + - * / sqrt, comparisons and selects,
 * every operation rounded once, nothing fused, in the order written here, so tests/sweep_ref.py (NumPy float32, every candidate of
 * every query, no traversal) gives the same bytes.  dot and sq as above; cross(a, b) = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx).
 * The ball (o, d, r) is taken as given, as a ray is for rt_trace_rays: d is not normalised, t is in units of its length.
 *
 * 1. Invalid input - a miss: a NaN or infinite component of o or d; dx == dy == dz == 0; r NaN, below zero or infinite; with a limit
 *    array, tmax NaN or not above zero.  lim = min(tmax, RT_HIT_MISS_T), or RT_HIT_MISS_T without the array.
 * 2. Start overlap - decided by the nearest-surface definition as it stands: if rt_nearest_points at o with the limit r is a hit, the
 *    record is t = 0, centre = o, point / object / triangle those of that nearest record, feature = -1, overlap = 1.
 * 3. Candidates otherwise, a time t each; dd = sq(d); `floor0(t)` is t <= 0 ? 0 : t (a NaN stays; a root that rounding put a hair
 *    below zero is a contact at the start, not a tunnel: the tests are "approaching", never "t > epsilon").  The roots of the sphere and
 *    the cylinder are NOT taken from the origin: the discriminant's rounding error grows with the square of the length of m, so m is
 *    first moved to the path's point of closest approach, where it is about as long as the miss distance.
 *    ball(m, rad) - the near root of |m + t d| = rad:  b = dot(m, d); t0 = -b / dd; n = d*t0 + m (per component one product, one sum);
 *                    b2 = dot(n, d); c2 = sq(n) - rad*rad; disc = b2*b2 - dd*c2; offered when disc >= 0 and b < 0:
 *                    t = floor0(t0 + (-b2 - sqrt(disc)) / dd).  The far root, farball(m, rad): the same with + sqrt(disc), offered when
 *                    disc >= 0.
 *    sphere (c, R):  m = o - c; outside when sq(m) > R*R: ball(m, R + r).  Inside: the FAR root on the inner surface (a sphere is a
 *                    surface, as for rt_nearest_points), farball(m, R - r), only when R - r > 0.  feature = -1, triangle = -1;
 *                    point = the nearest-surface definition's sphere point for p = centre.
 *    triangle record (p0, s1, s2) - a loose triangle, both records of a quad (a one-way quad counts from both sides), a cuboid's
 *    twelve, every mesh triangle: ap = o - p0; bp = ap - s1; cp = ap - s2; e3 = s2 - s1; rr = r*r.  Seven features in index order; the
 *    candidate is the smallest t, on equal t the lower index (a NaN t is never smaller):
 *      0 the face:   nrm = cross(s1, s2); nn = sq(nrm); len = sqrt(nn); h = dot(ap, nrm); dn = dot(d, nrm); neg = h < 0;
 *                    hs = neg ? -h : h; ds = neg ? -dn : dn; rl = r * len.  Offered when nn > 0 and hs >= rl and ds < 0:
 *                    t = floor0((rl - hs) / ds); centre = d*t + o; k = r / len; ks = neg ? -k : k; point = centre - nrm*ks;
 *                    w = point - p0; d00 = sq(s1); d01 = dot(s1, s2); d11 = sq(s2); d20 = dot(w, s1); d21 = dot(w, s2);
 *                    vn = d11*d20 - d01*d21; wn = d00*d21 - d01*d20; den = d00*d11 - d01*d01; accepted when vn >= 0 and wn >= 0
 *                    and vn + wn <= den.
 *      1..3 the edges (A, e, m) = (p0, s1, ap), (p0, s2, ap), (p0 + s1, e3, bp) - the infinite cylinder about the edge (Ericson,
 *                    Real-Time Collision Detection 5.3.7), from the foot of the common perpendicular of the path and the edge's line:
 *                    ee = sq(e); de = dot(d, e); me = dot(m, e); md = dot(m, d); a = ee*dd - de*de; b = ee*md - de*me; t0 = -b / a;
 *                    n = d*t0 + m; s0 = dot(n, e) / ee; p = n - e*s0; me2 = dot(p, e); md2 = dot(p, d); mm2 = sq(p);
 *                    b2 = ee*md2 - de*me2; c2 = ee*(mm2 - rr) - me2*me2; disc = b2*b2 - a*c2; t1 = (-b2 - sqrt(disc)) / a.  Offered
 *                    when a > 0 and disc >= 0 and b < 0:  t = floor0(t0 + t1); s = s0 + (me2 + t1*de) / ee; accepted when
 *                    0 <= s <= 1; point = A + e*s.
 *      4..6 the vertices: ball(ap, r), ball(bp, r), ball(cp, r); point = p0, p0 + s1, p0 + s2.
 *    The smallest accepted t is the first contact of a ball that does not overlap at the start: the volume the triangle sweeps out
 *    against the ball's centre is the union of a prism, three capped cylinders and three spheres, and the prism's sides and the
 *    cylinders' caps lie inside the other pieces.
 *    a mesh's triangle, additionally: every box on its path - the mesh table's root box, then the child box stored in each node down to
 *    the leaf - inflated by r (lo - r, hi + r, one rounding each) must pass the multi-hit section's slab test from tmin = 0, and the
 *    key is K = max(t, B), B the largest entry distance over those inflated boxes (K = t outside a mesh).  K orders and limits, the
 *    record reports the raw t.  The multi-hit section's argument holds word for word: every candidate below a box has a key no
 *    smaller than that box's entry distance, so "skip a subtree whose inflated box fails the slab test or is entered beyond the best
 *    key so far" is exact in any visiting order; a subtree entered AT the best key is still visited, because of the tie rule.
 * 4. Winner: the smallest K; on equal K the lower object index, then the lower triangle index; a candidate counts when K <= lim; a
 *    NaN never wins.  The record: t; centre = d*t + o (per component one product, one sum); point, formed again from the winner's
 *    record; object; triangle (-1 on a sphere); feature; overlap = 0. */
typedef struct __attribute__((aligned(16))) rt_sweep {
    float t;               /* time of first contact, in units of |d|; RT_HIT_MISS_T for a miss */
    float centre[3];       /* the ball's centre then: o + d * t */
    float point[3];        /* the contact point on the surface */
    int32_t object;        /* as rt_nearest.object; -1: a miss */
    int32_t triangle;      /* as rt_nearest.triangle; -1 for a sphere or a miss */
    int32_t feature;       /* -1 a scene sphere, a start overlap or a miss; 0 the face; 1..3 the edges (p0, s1), (p0, s2), (p0 + s1, s2 - s1);
                              4..6 the vertices p0, p0 + s1, p0 + s2 */
    int32_t overlap;       /* 1: the ball touches the scene already at t = 0 */
    int32_t reserved;      /* 0 */
} rt_sweep;                /* 48 bytes.  A miss is {RT_HIT_MISS_T, {0,0,0}, {0,0,0}, -1, -1, -1, 0, 0} bit for bit */

/* Device-buffer form: d_origins, d_directions (n x 3 floats each), d_radius (n floats), d_tmax (n floats, or NULL) and d_out (n records,
 * 16-byte aligned) are device memory of ctx's GPU.  Two launches inside one launch bracket: the nearest-surface kernel over d_origins
 * with d_radius itself as its limits, into records the context keeps, then the sweep kernel, which reads them.  Asynchronous on
 * hip_stream and ordered like rt_nearest_points_device.  n == 0 succeeds and touches nothing; n < 0, n > 2^30, a null pointer (other
 * than d_tmax) with n > 0, a misaligned d_out and a scene committed on another context are RT_ERR_INVALID and leave the launch order
 * as it was.  rt_last_kernel_ms then reports the sweep kernel (the second of the two).  A scene updated by
 * rt_scene_update_mesh_device answers for its new geometry. */
rt_status rt_sweep_spheres_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions,
                                  const float *d_radius, const float *d_tmax, int64_t n, rt_sweep *d_out, void *hip_stream);
/* Host-buffer form: uploads the balls (and limits), answers, downloads the records and returns when they are in `out`. */
rt_status rt_sweep_spheres(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, const float *radius,
                           const float *tmax, int64_t n, rt_sweep *out);

/* ---- box-overlap queries: which surfaces touch a box ----------------------------------------------
 * The VOLUME question beside the ray and the point questions: "which surfaces lie in this region?" - what a voxeliser, the broad phase
 * of a collision test, a "select everything in this box" tool and an octree or sparse-grid builder ask.  Thresholding a distance grid
 * at a cell's half diagonal gives a superset and does not say which triangles; with rt_winding_numbers' containment for the interior,
 * the surface test here completes a voxeliser.
 *
 * The answer is DEFINED to the bit, like its neighbours: binary32, every operation rounded once, nothing fused, in the order written
 * here, so tests/overlap_ref.py (NumPy float32, every candidate of every box, no traversal) gives the same bytes.  dot, sq and cross as
 * above.  A box (lo, hi) is axis-aligned and CLOSED: touching counts.
 *
 * Validity: all six floats finite and lo.a <= hi.a on every axis.  A box that is not valid overlaps nothing.
 * Centre and half extents: c = lo*0.5f + hi*0.5f, h = hi*0.5f - lo*0.5f (two products, then one sum or difference, per component:
 * no overflow for finite input).
 * Candidates: the nearest-surface section's - every sphere, as a SURFACE, and every triangle record (p0, s1, s2): loose triangles, both
 * records of a quad (a one-way quad counts from both sides), a cuboid's twelve, every mesh triangle.
 *   sphere (cs, R): per axis e = max(max(lo - cs, cs - hi), 0) (the nearest section's box distance) and g = max(cs - lo, hi - cs);
 *                   dmin2 = (sq(e.x) + sq(e.y)) + sq(e.z), dmax2 likewise from g, rr = R*R.  Overlaps when dmin2 <= rr and dmax2 >= rr:
 *                   a box wholly inside the ball touches no surface.
 *   triangle record: the separating-axis test of Akenine-Moller (2001) on the record as stored.  q0 = p0, q1 = p0 + s1, q2 = p0 + s2.
 *                   Overlaps when none of thirteen axes separates:
 *       the box's axes (3): axis a separates when all three q_i.a > hi.a or all three q_i.a < lo.a (compares on lo and hi themselves).
 *       the plane (1):      v_i = q_i - c; nrm = cross(s1, s2); d = dot(nrm, v0); r = (h.x*|nrm.x| + h.y*|nrm.y|) + h.z*|nrm.z|;
 *                           separates when d > r or d < -r.
 *       the edges (9):      for f in f0 = s1, f1 = s2 - s1, f2 = -s2 the three axes
 *                             px(v) = v.z*f.y - v.y*f.z, rad = h.y*|f.z| + h.z*|f.y|;
 *                             py(v) = v.x*f.z - v.z*f.x, rad = h.x*|f.z| + h.z*|f.x|;
 *                             pz(v) = v.y*f.x - v.x*f.y, rad = h.x*|f.y| + h.y*|f.x|;
 *                           an axis separates when all three projections > rad or all three < -rad.
 *     A compare with a NaN does not hold: an overflowed product leaves its axis unseparated, which is conservative.  A degenerate
 *     record (s1 and s2 parallel, or zero) is tested as it stands and may be reported conservatively.  The thirteen verdicts have no
 *     side effects: an implementation may take them in any order and leave at the first that separates.
 *   a mesh's triangle, additionally: every box on its path - the mesh table's root box, then the child box stored in each node down to
 *     the leaf - must overlap the query box by compares alone: nlo.a <= hi.a and lo.a <= nhi.a on all three axes.  This is the multi-hit
 *     section's path rule without arithmetic: "skip a subtree whose box does not overlap" is exact in any visiting order, with no error
 *     analysis.  The rule only bites where p0 + s1 rounds a hair outside a box built from the vertex itself;
 *     tests/golden/overlap_meta.json has the measured share of such pairs.
 * What the test is not: exact near touching.  Within a band of a few ulps of the scene's scale around "just touching" the thirteen
 * rounded verdicts may fall either way (tests/golden/overlap_meta.json has the measured band).
 * Output, for box i (each pointer optional, at least one given): d_counts[i] = the number of ALL candidates that overlap; d_any[i] =
 * count > 0; for k > 0, d_ids[i*k + rank] = the k overlapping candidates lowest in (object, then triangle) order, ascending; slots past
 * the count are {-1, -1}.  ANY-ONLY mode - only d_any asked for (k == 0, d_counts NULL): a box may stop at its first overlapping
 * candidate; the byte is the same by definition. */
#define RT_OVERLAP_MAX 8                /* ids per box, at most */
typedef struct rt_overlap_id {
    int32_t object;        /* index in the scene's object list; -1: no candidate at this rank */
    int32_t triangle;      /* index of the triangle record in the flattened scene; -1 for a sphere or an empty slot */
} rt_overlap_id;           /* 8 bytes */
/* Device-buffer form: d_lo, d_hi (n x 3 floats each), d_ids (n * k records, [box][rank], 8-byte aligned), d_counts (n int32) and d_any
 * (n bytes) are device memory of ctx's GPU; asynchronous on hip_stream and ordered like rt_trace_rays_device.  n == 0 succeeds and
 * touches nothing.  RT_ERR_INVALID, leaving the launch order as it was: n < 0 or n > 2^30; k < 0 or k > RT_OVERLAP_MAX; a null box
 * pointer with n > 0; d_ids null or misaligned while k > 0; d_ids, d_counts and d_any all null; a scene of another context; a scene of
 * more than 4,096 objects (an id is one 32-bit word, object << 20 | triangle, a sphere's triangle field all ones).
 * rt_last_kernel_ms then reports the overlap kernel.  A scene updated by rt_scene_update_mesh[_device] answers for its new geometry. */
rt_status rt_overlap_boxes_device(rt_ctx *ctx, const rt_scene *scene, const float *d_lo, const float *d_hi, int64_t n, int32_t k,
                                  rt_overlap_id *d_ids, int32_t *d_counts, uint8_t *d_any, void *hip_stream);
/* Host-buffer form: uploads the boxes, answers, downloads each output whose pointer is not NULL and returns when they are in host
 * memory (the context keeps the device buffers). */
rt_status rt_overlap_boxes(rt_ctx *ctx, const rt_scene *scene, const float *lo, const float *hi, int64_t n, int32_t k, rt_overlap_id *ids,
                           int32_t *counts, uint8_t *any);

/* ---- triangle-overlap queries: which surfaces a triangle cuts, and where ---------------------------
 * The NARROW phase behind the box query's broad phase: "does this part cut the scene, which triangles, and along which curve?" - a
 * mesh-scene collision test, the intersection curve of two surfaces (the CSG preview of the winding section), a cross-section (tile the
 * cutting plane into triangles).  The query is a triangle (a0, a1, a2), n x 9 floats as given.
 *
 * The answer is DEFINED to the bit, like its neighbours: binary32, every operation rounded once, nothing fused, in the order written
 * here, so tests/tritri_ref.py (NumPy float32, every candidate of every query, no traversal) gives the same bytes.  dot(a, b) =
 * (a.x*b.x + a.y*b.y) + a.z*b.z; cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).
 *
 * Validity: all nine floats finite.  A query that is not valid overlaps nothing.  A zero-area query is tested as it stands.
 * Of the query: lo.a = min(min(a0.a, a1.a), a2.a), hi.a likewise with max; z = a0 - a0 (the zero vector), e1 = a1 - a0, e2 = a2 - a0,
 * na = cross(e1, e2).
 * Candidates: the box section's - every sphere, as a SURFACE, and every triangle record (p0, s1, s2): q0 = p0, q1 = p0 + s1, q2 = p0 + s2.
 *   triangle record, in this order (nb = cross(s1, s2); d_j = q_j - a0):
 *     1. the query's bounding box: no overlap when on some axis all three q_j.a > hi.a or all three q_j.a < lo.a (compares alone).
 *     2. hA_i = dot(nb, a_i - q0): no overlap when all three are > 0 or all three are < 0.  Zero counts as touching.
 *     3. hB_j = dot(na, d_j): likewise.
 *     4. if hA_0 == hA_1 == hA_2 == 0 or hB_0 == hB_1 == hB_2 == 0 the pair is COPLANAR (or a normal vanished) and is decided by six
 *        in-plane axes: X = cross(na, f) for f in e1, a2 - a1, a0 - a2, then X = cross(nb, g) for g in s1, s2 - s1, -s2.  On an axis
 *        the query projects to u = dot(X, z), dot(X, e1), dot(X, e2) and the record to w_j = dot(X, d_j); the axis separates when all nine
 *        u_i < w_j hold or all nine u_i > w_j hold.  The pair overlaps when no axis separates: a vanished normal gives axes that
 *        separate nothing and is reported conservatively.  Such a pair has no segment (kind 2).
 *     5. otherwise Moeller's interval test (1997) on D = cross(na, nb): pA = dot(D, z), dot(D, e1), dot(D, e2); pB_j = dot(D, d_j).
 *        A triangle's LONE vertex l from its heights (h0, h1, h2), Moeller's sign rule: h0*h1 > 0: l = 2; else h0*h2 > 0: l = 1; else
 *        h1*h2 > 0 or h0 != 0: l = 0; else h1 != 0: l = 1; else l = 2.  The other two, o and o', in index order.  Its interval's two ends,
 *        end 1 towards o and end 2 towards o': x = p_l + (p_o - p_l) * (h_l / (h_l - h_o)) - one IEEE division, then the product, then
 *        the sum; x = p_l when h_l - h_o == 0.  No overlap when all four xA < xB hold (xA_1 < xB_1, xA_1 < xB_2, xA_2 < xB_1,
 *        xA_2 < xB_2: the query's maximum below the record's minimum), or all four xB < xA.  A compare with a NaN does not hold: an
 *        overflowed product leaves the pair reported, which is conservative.
 *   The verdicts of steps 1 to 3 have no side effects: an implementation may leave at the first that separates.
 *   a mesh's triangle, additionally: the box section's path rule, with (lo, hi) the query's bounding box.
 *   sphere (c, R): near2 = the nearest section's point-triangle dist2 of the point c and the record (a0, e1, e2); far2 =
 *     max(max(dot(v0, v0), dot(v1, v1)), dot(v2, v2)) with v_i = a_i - c; rr = R*R.  Overlaps when near2 <= rr and far2 >= rr: a triangle
 *     wholly inside the ball touches no surface.
 * The SEGMENT of an overlapping pair of step 5 (kind 1) is the overlap of its two intervals.  An interval's minimum is its end 1 where
 * x_1 <= x_2, else its end 2; the maximum is the other.  p belongs to the record where minB > minA, else to the query (a tie goes to the
 * query); q to the record where maxB < maxA, else to the query.  The point of an end is its edge crossing: per component
 * v_l + (v_o - v_l) * (h_l / (h_l - h_o)), the same quotient as the end's, v_l where the denominator is zero; v are a0..a2 of the
 * query, q0..q2 of the record.  A point contact has p == q.
 * What the test is not: exact near touching, or for nearly coplanar pairs - the rounded heights and interval ends may fall either way
 * within a band of the scene's scale (tests/golden/tritri_meta.json has the measured share against exact rational arithmetic) - and not
 * a self-intersection test: asked with a mesh's own triangles, every neighbour that shares a vertex touches by definition and crowds out
 * the eight ids.
 * Output, for query i: d_counts, d_any and d_ids exactly as in the box section, ANY-ONLY mode included.  d_segments[i*k + rank]
 * (needs k > 0 and d_ids) is the segment of the pair in d_ids[i*k + rank]. */
typedef struct rt_tri_segment {
    float p[3];            /* the segment's ends (kind 1); zeros in an empty slot; NaNs (0x7fc00000) for kind 2 */
    float q[3];
    int32_t kind;          /* 0: an empty slot; 1: a segment from p to q; 2: a pair that has no segment - a sphere, or a coplanar pair */
    int32_t reserved;      /* 0 */
} rt_tri_segment;          /* 32 bytes */
/* Device-buffer form: d_tris (n x 9 floats), d_ids (n * k records, [query][rank], 8-byte aligned), d_counts (n int32), d_any (n bytes)
 * and d_segments (n * k records, 16-byte aligned) are device memory of ctx's GPU; asynchronous on hip_stream and ordered like
 * rt_trace_rays_device.  n == 0 succeeds and touches nothing.  RT_ERR_INVALID, leaving the launch order as it was: n < 0 or n > 2^30;
 * k < 0 or k > RT_OVERLAP_MAX; a null d_tris with n > 0; d_ids null or misaligned while k > 0; d_ids, d_counts and d_any all null;
 * d_segments given with k == 0, or misaligned; a scene of another context; a scene of more than 4,096 objects.  rt_last_kernel_ms then
 * reports the triangle-overlap kernel.  A scene updated by rt_scene_update_mesh[_device] answers for its new geometry. */
rt_status rt_overlap_triangles_device(rt_ctx *ctx, const rt_scene *scene, const float *d_tris, int64_t n, int32_t k, rt_overlap_id *d_ids,
                                      int32_t *d_counts, uint8_t *d_any, rt_tri_segment *d_segments, void *hip_stream);
/* Host-buffer form: uploads the triangles, answers, downloads each output whose pointer is not NULL and returns when they are in host
 * memory (the context keeps the device buffers). */
rt_status rt_overlap_triangles(rt_ctx *ctx, const rt_scene *scene, const float *tris, int64_t n, int32_t k, rt_overlap_id *ids,
                               int32_t *counts, uint8_t *any, rt_tri_segment *segments);

/* ---- occlusion (any-hit) ray queries and the light-visibility plane ------------------------------
 * "Is anything in the way?": line of sight, shadow masks, reachability probes.  For a ray (o, d) taken as given and a limit tmax,
 *     occluded(o, d, tmax) := get_ray_collision (src/raytracer.cu:24-46; what rt_trace_rays answers) finds a hit AND its t <= tmax.
 * The direction is not normalised and t, tmax are in units of its length (Ray::change_direction src/ray.cu:198-202); the reference's
 * acceptance rules (dist > 1e-6 in Sphere::hit and Triangle::hit src/objects.cu:40-79,135-163, one-way quads :273-280, the strict slab
 * test) are unchanged; a direction with a NaN component hits nothing; a NaN tmax compares false (not occluded); tmax >= RT_HIT_MISS_T
 * means "any hit at all".  The answer is exact, not approximate: the kernel stops a ray as soon as one object's running best
 * (src/objects.cu:487-532) is within the limit, which is when the final distance is (tests/test_gpu_occlusion.py: equal to the CPU
 * oracle's orc_trace_one, every byte).  One byte per ray instead of rt_trace_rays' 48.
 *
 * Device-buffer form: d_origins, d_directions (n x 3 floats each), d_tmax (n floats, or NULL = RT_HIT_MISS_T for every ray) and
 * d_occluded (n bytes: 1 occluded, 0 not) are device memory of ctx's GPU; asynchronous on hip_stream and ordered like
 * rt_render_device.  n == 0 succeeds and touches nothing; n < 0, n > 2^30, a null pointer (other than d_tmax) with n > 0 and a scene
 * committed on another context are RT_ERR_INVALID.  rt_last_kernel_ms then reports the occlusion kernel. */
rt_status rt_occluded_rays_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions,
                                  const float *d_tmax, int64_t n, uint8_t *d_occluded, void *hip_stream);
/* Host-buffer form: uploads the rays, answers, downloads the bytes and returns when they are in `occluded`. */
rt_status rt_occluded_rays(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions,
                           const float *tmax, int64_t n, uint8_t *occluded);

/* The light-visibility plane of a view: a shadow mask for a point light, W*H bytes in rt_render's row-major layout.  Per pixel
 *   1. rt_render_aov's primary ray (antialiasing off, src/camera.cu:24-29, src/raytracer.cu:123-127) and its closest hit; none:
 *      RT_VIS_NO_SURFACE;
 *   2. from the hit's point P and shading normal N exactly as rt_hit reports them (Ray::get_pos src/ray.cu:63-65, src/objects.cu:66,
 *      :158): o' = P + N * bias per component in two binary32 roundings (N.x * bias, then + P.x), d' = light_pos - o' (not normalised);
 *   3. occluded(o', d', 1.0f): RT_VIS_BLOCKED, otherwise RT_VIS_LIT.
 * A visibility bit: no facing test, no falloff, no light radius; an emissive first hit is a surface like any other. */
#define RT_VIS_BLOCKED 0
#define RT_VIS_LIT 1
#define RT_VIS_NO_SURFACE 2
rt_status rt_render_visibility_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float light_pos[3], float bias,
                                      uint8_t *d_visibility, void *hip_stream);
/* Host-buffer form: returns when the plane is in host memory. */
rt_status rt_render_visibility(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float light_pos[3], float bias,
                               uint8_t *visibility);

/* The ambient-occlusion plane of a view: from every pixel's first hit, how much of the cosine-weighted hemisphere within `radius` is
 * free.  Per pixel (px, py) of the cam->width x cam->height image, in rt_render's row-major full-frame layout:
 *   1. rt_render_aov's primary ray (antialiasing off) and its closest hit; none: count = RT_AO_NO_SURFACE, ao = 1.0f;
 *   2. from the hit's point P and shading normal N exactly as rt_hit reports them: o' = N * bias + P per component in two binary32
 *      roundings (the visibility plane's step 2);
 *   3. the renderer's per-pixel random state (src/raytracer.cu:127): state = (uint32)((py * W + px) * 3) * 3145739u +
 *      (uint32)time_ms * 6291469u;
 *   4. for k = 0 .. samples-1, in order, on that one stream: r = (g(), g(), g()) with g = normally_dist_num (src/utils.cu:234-239: the
 *      angle draw first, then the radius draw; rho * cos(theta)); if dot(r, N) < 0 then r = -r; r = normalised(r); d = normalised(N + r)
 *      - Ray::true_lambertian_reflect (src/ray.cu:157-178), with dot = (x*x' + y*y') + z*z' and normalised = a * (1.0f /
 *      sqrtf((x*x + y*y) + z*z)), nothing fused.  The sample is free iff !occluded(o', d, radius), occluded as rt_occluded_rays defines
 *      it; a radius >= RT_HIT_MISS_T (or +inf) means "any hit at all".  Every sample consumes exactly six draws whatever its outcome;
 *   5. count = the number of free samples, ao = (float)count / (float)samples (one IEEE division).
 * With samples = 1, bias = 0 and an unlimited radius the count is what rt_render gives at one sample per pixel, reflection limit 2,
 * antialiasing off and a white sky for a scene whose materials are all white and diffuse: the first bounce ray escapes or it does not.
 * samples outside 1 .. RT_AO_MAX_SAMPLES, a radius that is NaN or <= 0, a bias that is negative or not finite, both output pointers
 * NULL (either alone may be), a null context, scene or camera and a scene of another context are RT_ERR_INVALID.
 * Device-buffer form: d_count (W*H uint16) and d_ao (W*H floats) are device memory of ctx's GPU; asynchronous on hip_stream and ordered
 * like rt_render_device (one launch in flight per context); rt_last_kernel_ms reports it. */
#define RT_AO_NO_SURFACE 0xFFFFu
#define RT_AO_MAX_SAMPLES 4096
rt_status rt_render_ao_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, int32_t samples, float radius, float bias,
                              int32_t time_ms, uint16_t *d_count, float *d_ao, void *hip_stream);
/* Host-buffer form: returns when the planes are in host memory. */
rt_status rt_render_ao(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, int32_t samples, float radius, float bias,
                       int32_t time_ms, uint16_t *count, float *ao);

/* ---- edge-avoiding a-trous denoiser driven by the first-hit planes ------------------------------
 * An image-space filter for a noisy low-sample frame (Dammertz et al. 2010, "Edge-avoiding A-Trous wavelet transform for fast global
 * illumination filtering"; the spatial filter of SVGF without its temporal part).  It takes plain planes in rt_render's row-major
 * full-frame layout and needs no scene: C colour (W*H*3 floats), N normal (W*H*3), Z depth (W*H), O object id (W*H int32, optional:
 * NULL means "all equal"), A albedo (W*H*3, optional) - N, Z, O, A are what rt_render_aov writes.
 *
 * The result is DEFINED, not approximated: only binary32 + - * /, comparisons and selects, every operation rounded once (no fused
 * multiply-add), in the order written here, so tests/denoise_ref.py (NumPy float32) gives the same bits for every pixel.
 *   1. Demodulate: F0[p].k = C[p].k / max(A[p].k, albedo_floor) per channel k when A is given (max(a, f) = a > f ? a : f), else F0 = C.
 *   2. For level i = 0 .. iterations-1, s = 1 << i; sc = sigma_colour * 2^-i, kc = 1.0f / (sc * sc) (on the host, binary32).
 *      Per centre pixel p: kz = 1.0f / (sigma_depth * Z[p]); acc = (0, 0, 0), wsum = 0.
 *      Taps q = p + (dx*s, dy*s), dy = -2..2 outer, dx = -2..2 inner, in that order; a tap outside the image is skipped.
 *        hw = h[dy+2] * h[dx+2] rounded once, h = {1/6, 2/3, 1, 2/3, 1/6} as the nearest binary32 values
 *          = {0x3E2AAAAB, 0x3F2AAAAB, 0x3F800000, 0x3F2AAAAB, 0x3E2AAAAB} (the B3 spline 1:4:6:4:1 scaled so that the centre is 1).
 *        The centre tap has w = 1.0f and its weight functions are not evaluated (a pixel whose neighbours are all rejected comes back
 *        bit for bit).  Otherwise, with k(x) = (x < 1.0f) ? (1.0f - x) * (1.0f - x) : 0.0f (a NaN gives 0):
 *          O[q] != O[p]: the tap is skipped;
 *          dn = (N[p].x*N[q].x + N[p].y*N[q].y) + N[p].z*N[q].z; wn = dn > 0 ? dn : 0; then wn = wn * wn, normal_power_log2 times;
 *          r = max(|dx|, |dy|) * s; g = ((Z[q] - Z[p]) * kz) * (1.0f / r); wz = k(g * g);
 *          d = Fi[q] - Fi[p] per channel; x = ((d.r*d.r + d.g*d.g) + d.b*d.b) * kc; wc = k(x);
 *          w = hw * ((wn * wz) * wc); a tap with w == 0 is skipped (a non-finite colour behind a zero weight does not spread).
 *        acc.k = acc.k + w * Fi[q].k (two roundings), wsum = wsum + w, in tap order, the centre in its place.
 *      F(i+1)[p].k = acc.k / wsum (wsum >= 1).  The guides N, Z, O are always the original planes; only the colour comes from level i.
 *   3. Remodulate: out[p].k = F[p].k * max(A[p].k, albedo_floor) when A is given, else out = F.
 * What follows: a miss (normal 0, 0, 0) keeps its own colour; the depth tolerance grows with the tap's distance in pixels (the 1 / r), so
 * a slanted plane is not cut into strips at the large steps; sigma_depth is relative to the centre's depth; the colour tolerance halves
 * per level.  d_out may be d_colour: the passes run on buffers of the context's own (48 bytes per pixel, kept until the context goes). */
typedef struct rt_denoise_params {
    int32_t iterations;          /* levels, 1 .. 8: level i has step 2^i; the last level's outermost tap is 1 << iterations pixels from its centre, the whole cascade gathers from up to 2 * ((1 << iterations) - 1) pixels away */
    float sigma_colour;          /* > 0 and finite: the distance in (demodulated) colour at which the first level's weight reaches 0 */
    float sigma_depth;           /* > 0 and finite: the same for |Z[q] - Z[p]| / Z[p] per pixel of distance */
    int32_t normal_power_log2;   /* 0 .. 8: the normal weight is max(0, N[p].N[q]) ^ (2 ^ this) */
    float albedo_floor;          /* > 0 and finite; only read (and only checked) when an albedo plane is given */
    int32_t reserved[3];         /* 0 */
} rt_denoise_params;             /* 32 bytes */
/* The defaults: iterations 5, sigma_colour 4, sigma_depth 0.02, normal_power_log2 5, albedo_floor 0.01.  Tuned on the CPU oracle alone
 * (three-sphere, cube and monkey scenes, 128 x 128, default camera, 8 bounces, input 4 spp x 1 frame, target 1024 spp): the one set of
 * those scanned that lowers the RMSE against the target on all three markedly (to 0.28 / 0.37 / 0.58 of the noisy frame's) - a
 * sigma_colour <= 1 leaves the monkey scene's fireflies (values of 4 .. 7.5) where they are, a looser sigma_depth starts to blur the
 * two smooth scenes (tests/test_denoise_ref.py). */
void rt_denoise_params_default(rt_denoise_params *p);
/* Device-buffer form: every plane and d_out are device memory of ctx's GPU; asynchronous on hip_stream and ordered like
 * rt_render_device (one launch in flight per context).  A null ctx, d_colour, d_normal, d_depth, params or d_out, a size that is not
 * positive (or above 32768 on a side, 2^28 pixels in all), parameters outside the ranges above and a non-zero `reserved` are
 * RT_ERR_INVALID.  rt_last_kernel_ms then reports the denoise passes from first to last. */
rt_status rt_denoise_device(rt_ctx *ctx, int32_t width, int32_t height, const float *d_colour, const float *d_normal,
                            const float *d_depth, const int32_t *d_object, const float *d_albedo,
                            const rt_denoise_params *params, float *d_out, void *hip_stream);
/* Host-buffer form: uploads the planes, filters, and returns when `out` (W*H*3 floats) is filled. */
rt_status rt_denoise(rt_ctx *ctx, int32_t width, int32_t height, const float *colour, const float *normal, const float *depth,
                     const int32_t *object, const float *albedo, const rt_denoise_params *params, float *out);

/* ---- per-pixel sample budgets and the adaptive sampling loop -------------------------------------
 * rt_render_device spends rays_per_pixel samples on every pixel; here every pixel has a sample count of its own, so that samples go
 * where the noise is.  Three layers, each defined to the bit: all arithmetic is binary32, every operation is rounded once, nothing is
 * fused.
 *
 * 1. Budget render.  d_budget (W*H uint16) and d_count (W*H uint32, or NULL) are planes in rt_render's row-major full-frame layout,
 *    d_frame a full W*H*3 frame.  rs->rays_per_pixel is not read; reflection_limit, antialias and sky_colour apply as in
 *    rt_render_device.  Per pixel, with n = d_budget[pixel] and m = d_count[pixel] (0 for every pixel when d_count == NULL):
 *      n == 0: nothing of the pixel is read or written;
 *      n >  0: c = the per-pixel mean rt_render_device computes for the pixel with rays_per_pixel = n and this time_ms: the same stream
 *              (state = (uint32)((py * W + px) * 3) * 3145739u + (uint32)time_ms * 6291469u, src/raytracer.cu:127), its n samples summed
 *              in order and divided by (float)n; a reflection_limit <= 0 gives (0, 0, 0), as there.
 *              m == 0: frame = c (the old content is not read: an uninitialised frame is fine);
 *              else    frame.k = (c.k * (float)n + frame.k * (float)m) / (float)(n + m) per channel k.
 *              A NaN result is stored as the canonical quiet NaN 0x7FC00000.  count = m + n (not written when d_count == NULL).
 *    So a pixel rendered with budget n from count 0 IS the pixel rt_render_device renders at rays_per_pixel = n, frame_num = 0
 *    (tests/test_gpu_adaptive.py: equal as uint32), and a frame accumulated over calls is the sample-count-weighted mean of their means.
 *    tiles == NULL: the whole image; a tile list with compact == 0: only the listed tiles' pixels are considered, and the tiles are
 *    handed to the waves in list order (the caller orders them: the launch neither collects nor uses tile costs).  Bands (a tile spec
 *    without a list), compact != 0 and tile_cost / tile_peak are RT_ERR_INVALID, as are a null ctx, scene, cam, rs, d_budget or
 *    d_frame, a scene of another context, a negative reflection_limit, a bad image size and a list with an index outside the image or
 *    listed twice.  A budget is at most RT_BUDGET_MAX, the plane's type.
 *    The launch is asynchronous on hip_stream and ordered like rt_render_device; rt_last_kernel_ms reports it. */
#define RT_BUDGET_MAX 65535
rt_status rt_render_budget_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                  int32_t time_ms, const rt_tile_spec *tiles, const uint16_t *d_budget, uint32_t *d_count,
                                  float *d_frame, void *hip_stream);
/* Host-buffer form: budget (W*H), count (W*H, or NULL) and frame (W*H*3) are host memory; count and frame are read, updated and
 * written back; returns when they are. */
rt_status rt_render_budget(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                           int32_t time_ms, const rt_tile_spec *tiles, const uint16_t *budget, uint32_t *count, float *frame);

/* 2. Plan.  Image-space, no scene: the two-half-buffer stopping rule of Dammertz et al. 2010, "A hierarchical automatic stopping
 *    condition for Monte Carlo global illumination", on the renderer's 8x8 tiles.  A and B (W*H*3 each) are two independent
 *    accumulations of one view, count (W*H uint32) the samples in EACH of them.  Per pixel
 *      I.k = (A.k + B.k) * 0.5f;  num = (|A.r - B.r| + |A.g - B.g|) + |A.b - B.b|;  s = (I.r + I.g) + I.b;
 *      e = num / sqrtf(s > floor ? s : floor); a NaN e becomes 0 (a NaN pixel never converges, so it is not sampled for its own sake).
 *    Per tile: E = (the sum of e over the tile's 64 slots, a slot outside the image counting 0.0f) / (float)(the tile's pixels inside
 *    the image).  The sum is the xor butterfly over slot = row * 8 + column: v[i] = v[i] + v[i ^ 1], then ^ 2, ^ 4, ... ^ 32 - a
 *    pairwise tree: neighbours, then pairs of pairs, ...
 *    A pixel is active iff count < max_spp and (E > threshold or e > pixel_threshold); its budget is min(step_spp, max_spp - count)
 *    if active, else 0.  Outputs: d_budget (W*H uint16), d_tile_error (one float per tile, E) and d_tile_active (one uint32 per tile,
 *    its number of active pixels); tile ty * ceil(W / 8) + tx.  pilot_spp and max_passes are not read by the plan (checked all the
 *    same). */
typedef struct rt_adaptive_params {
    int32_t pilot_spp;           /* 1 .. 65535: the samples every pixel gets in each half buffer before the first plan */
    int32_t step_spp;            /* 1 .. 65535: an active pixel's samples per pass and half buffer */
    int32_t max_spp;             /* pilot_spp .. 2^24: no pixel gets more per half buffer */
    int32_t max_passes;          /* 0 .. 64: passes after the pilot (0: the pilot only) */
    float threshold;             /* > 0 and finite: a tile whose mean error E is above it keeps all its pixels sampling */
    float pixel_threshold;       /* > 0, +inf: off: a pixel whose own e is above it keeps sampling whatever its tile says */
    float floor;                 /* > 0 and finite: the least brightness the error is taken relative to */
    int32_t reserved[1];         /* 0 */
} rt_adaptive_params;            /* 32 bytes */
#define RT_ADAPTIVE_MAX_SPP 16777216
#define RT_ADAPTIVE_MAX_PASSES 64
/* The defaults: pilot_spp 8, step_spp 16, max_spp 512, max_passes 16, threshold 0.05, pixel_threshold +inf, floor 0.01.  Tuned on the
 * CPU oracle alone (cube and monkey scenes, 128 x 128, default camera, 8 bounces, target 1024 spp; tests/test_adaptive_ref.py and
 * DESIGN.md §16 have the figures). */
void rt_adaptive_params_default(rt_adaptive_params *p);
/* Asynchronous on hip_stream and ordered like rt_render_device.  A null pointer, a bad image size, parameters outside the ranges above
 * and a non-zero `reserved` are RT_ERR_INVALID. */
rt_status rt_adaptive_plan_device(rt_ctx *ctx, int32_t width, int32_t height, const float *d_a, const float *d_b, const uint32_t *d_count,
                                  const rt_adaptive_params *params, uint16_t *d_budget, float *d_tile_error, uint32_t *d_tile_active,
                                  void *hip_stream);

/* 3. Driver.  The loop, on buffers of the context's own (A, B, their count planes, the budget plane, the per-tile planes: 34 bytes per
 *    pixel, kept until the context goes):
 *      pass 0:                  a uniform budget pilot_spp over all tiles, into A with seed time_ms, into B with seed time_ms + 1;
 *      pass k = 1..max_passes:  plan; stop if no tile has an active pixel; the tile list is the tiles with an active pixel by
 *                               decreasing E, ties by the lower index (the longest jobs first); budget render of the list into A with
 *                               seed time_ms + 2k and into B with seed time_ms + 2k + 1 (seeds wrap as 32-bit integers);
 *      end:                     d_frame = (A + B) * 0.5f, a NaN as the canonical quiet NaN; d_count (W*H uint32, or NULL) = 2 * count.
 *    d_frame and d_count are device memory.  The call BLOCKS until they are written: it reads the per-tile planes back between passes.
 *    Its work runs on hip_stream.  stats (or NULL) reports what was done. */
typedef struct rt_adaptive_stats {
    int32_t passes;              /* passes rendered after the pilot */
    int32_t reserved;            /* 0 */
    uint64_t total_samples;      /* over all pixels and both half buffers: the sum of d_count */
    int32_t active_tiles[RT_ADAPTIVE_MAX_PASSES];   /* [k - 1]: the tiles pass k rendered; 0 beyond `passes` */
} rt_adaptive_stats;             /* 272 bytes */
rt_status rt_render_adaptive(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, int32_t time_ms,
                             const rt_adaptive_params *params, float *d_frame, uint32_t *d_count, rt_adaptive_stats *stats,
                             void *hip_stream);
/* Host-buffer form: frame (W*H*3) and count (W*H, or NULL) are host memory. */
rt_status rt_render_adaptive_host(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, int32_t time_ms,
                                  const rt_adaptive_params *params, float *frame, uint32_t *count, rt_adaptive_stats *stats);

/* ---- several GPUs of one node from one host thread ---------------------------------------------
 * What run_ray_tracer (src/dispatch.cu:127-153) does on one device, n devices do for the bands they
 * own: rank i of n_ranks renders the bands b with b % n_ranks == i (a pixel depends
 * only on its own coordinates, seed and previous value, so any partition gives the single-GPU image bit
 * for bit) on its own context, asynchronously; the band buffers travel to ranks[0]'s GPU with one peer
 * copy per rank (xGMI) and are de-interleaved there.  There is no reduction, hence no collective.
 * Every rank needs the scene committed on ITS context; a context may appear once.
 * rt_render_multi[_device] own the partition: the first call for a view deals the tiles out interleaved and
 * measures what they cost; from the second call on every rank owns a cost-balanced tile list
 * (rt_partition_tiles), so the ranks finish together. */
typedef struct rt_rank {
    rt_ctx *ctx;
    const rt_scene *scene;
} rt_rank;

/* render() src/dispatch.cu:156-163 for a node, host-buffer form: n_frames passes of the main loop body
 * (frame i seeded with times_ms[i]) accumulated into previous_render; *frame_num advances by n_frames.
 * Same image as rt_render_frames on one GPU. */
rt_status rt_render_multi(const rt_rank *ranks, int32_t n_ranks, const rt_camera *cam, const rt_render_settings *rs,
                          const int32_t *times_ms, int32_t n_frames, int32_t *frame_num, float *previous_render);
/* Device-buffer form: d_frame is a full W*H*3 frame on ranks[0]'s GPU, updated in place (its content is
 * the image after frame_num - 1 when frame_num > 0, ignored otherwise).  band_rows > 0 (a multiple of 8):
 * the static partition of round 2 - rank i owns the bands b % n_ranks == i; band_rows == 0: cost-balanced
 * tile lists as described above.  Asynchronous: the frame is complete in the order of hip_stream (a stream of
 * ranks[0]'s GPU, NULL = default stream); rt_ctx_synchronize on each rank reports kernel errors. */
/* (Diagnosis: with RT_AMD_MULTI_CAREFUL=1 in the environment when the ROOT context is created, the call waits on the host for
 * every stream involved after each of its phases - scatter-out, the ranks' kernels and copies, de-interleave - and an error names
 * the phase: same frames, no overlap.) */
rt_status rt_render_multi_device(const rt_rank *ranks, int32_t n_ranks, const rt_camera *cam, const rt_render_settings *rs,
                                 const int32_t *times_ms, int32_t n_frames, int32_t frame_num, int32_t band_rows,
                                 float *d_frame, void *hip_stream);
/* The exchange step alone, for callers that launch the ranks themselves (rt_render_device[_batch] with a
 * compact tile spec, bands or list): the compact buffer d_bands of the rank `src_tiles` describes, on src's GPU,
 * lands in the full frame d_frame on root's GPU - one peer copy + a de-interleave on root_stream - ordered
 * behind src's most recent launch. */
rt_status rt_gather(rt_ctx *root, float *d_frame, int32_t width, int32_t height, rt_ctx *src, const float *d_bands,
                    const rt_tile_spec *src_tiles, void *root_stream);

/* Direct (xGMI) access from a's GPU to b's memory and back: enables it if need be and reports 1 (peer access is
 * on in both directions: copies between the two go GPU to GPU), 0 (refused or unavailable: the runtime stages
 * them through the host - still correct, slower) or 1 when both contexts share a GPU; < 0: -rt_status. */
int32_t rt_peer_access(rt_ctx *a, rt_ctx *b);

/* float -> RGBA8 display conversion of src/main.cu:343-371 (int(px*255), clamp, alpha 255),
 * on the device: d_rgb W*H*3 floats -> d_rgba W*H*4 bytes */
rt_status rt_to_rgba8_device(rt_ctx *ctx, const float *d_rgb, int32_t width, int32_t height, uint8_t *d_rgba, void *hip_stream);

/* ---- introspection (tests only): the flattened device layout of a builder ---------------- */
/* Pointers stay valid until the next rt_debug_flatten call on the same builder or its
 * destruction.  blob is the LDS-staged part in 16-byte units (see
 * ray-tracer_amd/csrc/rt_device_scene.h); objects is the scalar-loaded object table. */
typedef struct rt_flat_view {
    const float *blob; int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, num_meshes, stack_entries;
    const void *objects; int32_t num_objects, object_stride;
    const float *tri_uv; int32_t num_triangles, num_nodes, has_mesh;
    /* traits: bit 0 every object that is not a mesh is a sphere, bit 1 at most one mesh, bit 2 no material needs texture coordinates,
     * refracts or carries a texture; kernel_variant: the render kernel a scene of these traits runs, as rt_scene_info reports it (decided
     * on the host from the traits and RT_AMD_KERNEL_VARIANT alone: rt_debug_flatten needs no device for it) */
    int32_t traits, kernel_variant;
    /* one byte per triangle record in the flattened order, or NULL without triangles: 1 where a mesh's record is oriented against the face
     * it came from (the second triangle of a quad face of an .obj), 0 elsewhere and for records of objects that are not meshes: what the
     * winding-number queries sign a mesh's terms by.  rt_debug_scene_read reports it as the device has it after updates. */
    const uint8_t *tri_flip;
} rt_flat_view;
rt_status rt_debug_flatten(rt_scene_builder *b, rt_flat_view *out);
/* the same view of a committed scene AS IT IS ON THE DEVICE (waits for the device first): what rt_scene_update_mesh[_device] is tested by.
 * Pointers stay valid until the next call on the same scene or its destruction. */
rt_status rt_debug_scene_read(rt_ctx *ctx, rt_scene *scene, rt_flat_view *out);
/* The cluster trees of the fast winding numbers (tests only).  Clusters of all meshes back to back; skip and first are indices into these
 * arrays (first: into order); object_range: per object of the list (c0, c1), its clusters, (0, 0) for what is not a mesh; order: per
 * flattened triangle index, for a mesh's range [prim_start + position in cluster order] = the commit index within the mesh, elsewhere 0;
 * position: likewise, = the flattened index of the record that holds that triangle now (the BVH's leaf order, which an update changes);
 * moments: per cluster 8 floats (c.xyz, r2, M.xyz, 0). */
typedef struct rt_winding_tree_view {
    const int32_t *skip, *first, *count; int32_t num_clusters;
    const int32_t *object_range; int32_t num_objects;
    const int32_t *order; int32_t num_triangles;
    const int32_t *position;
    const float *moments;
} rt_winding_tree_view;
/* from a builder, no device: the topology and the moments as the host text computes them from the commit-time records.  Pointers stay valid
 * until the next call on the same builder or its destruction. */
rt_status rt_debug_winding_tree(rt_scene_builder *b, rt_winding_tree_view *out);
/* from a committed scene: the same as the device holds it now (builds and refits first if no fast query has; waits for the device).
 * Pointers stay valid until the next call on the same scene or its destruction. */
rt_status rt_debug_scene_winding_tree(rt_ctx *ctx, rt_scene *scene, rt_winding_tree_view *out);
/* The primary-ray cull (ray-tracer_amd/csrc/rt_cull.h): render launches of a mesh scene that runs rt_traits_kernel on 1024 threads are handed one bit per
 * pixel of the view, "no primary ray of this pixel can reach a leaf of any mesh", computed on the device once per (scene revision, camera, image size,
 * antialias flag); RT_AMD_PRIMARY_CULL=0 (read by rt_ctx_create) renders without it.  Frames are bit-identical either way.
 * rt_debug_primary_cull: the plane the context's last render launch was handed, read back (waits for the device).  info4 = {1 if that launch
 * was handed a plane else 0, the plane's image width, its height, its 32-bit words: pixel py * width + px is bit (pixel & 31) of word
 * pixel >> 5}; words may be NULL or capacity_words too small: then only info4 is written. */
rt_status rt_debug_primary_cull(rt_ctx *ctx, uint32_t *words, int32_t capacity_words, int32_t *info4);
/* the same plane computed on the HOST (no device is touched) from a flattened scene - rt_debug_flatten's view or rt_debug_scene_read's - with the
 * same predicate.  words: ((width * height + 63) / 64) * 2 of them, or NULL.  stats6, or NULL: {pixels whose jitter cone may enter some mesh's
 * root box, those of them that are flagged, nodes the centre direction visits in the flagged ones, ... in all root-entering pixels, flagged
 * pixels in all, words of the plane} */
rt_status rt_debug_primary_cull_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, uint32_t *words, int64_t *stats6);
/* The subtree cull (rt_cull.h): behind its bit each pixel of the view has a 32-bit word, bit g set iff gate g of the scene's one mesh - the g-th
 * non-root reference of its tree in breadth-first order, g = 1..31 - leads the pixel's primary rays to no leaf; the kernel above does not enter such a
 * reference with a primary ray.  RT_AMD_SUBTREE_CULL=0 (read by rt_ctx_create) writes every word as 0.  Frames are bit-identical either way.
 * rt_debug_subtree_cull: the words the context's last render launch was handed, read back (waits for the device).  info4 as above, its fourth
 * entry the word count width * height: pixel py * width + px is word py * width + px. */
rt_status rt_debug_subtree_cull(rt_ctx *ctx, uint32_t *words, int32_t capacity_words, int32_t *info4);
/* the same words computed on the HOST (no device is touched) from a flattened scene.  words: width * height of them, or NULL.  stats4, or NULL, over
 * the unflagged pixels whose jitter cone may enter the root box, their centre ray walked in the kernel's order: {those pixels, its node steps
 * ungated, its node steps with the pixel's word, pixels whose word is not 0} */
rt_status rt_debug_subtree_cull_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, uint32_t *words, int64_t *stats4);
/* The primary entry word (rt_entry.h): behind the gate words each pixel of the view has a third word that says where its primary rays end in the
 * scene's one mesh - T << 1 | 1: every one of them ends on triangle T, and the kernel above starts it there; 2: none hits a triangle, and the pixel is
 * treated as a flagged one; 0: not known.  RT_AMD_PRIMARY_ENTRY=0 (read by rt_ctx_create) writes every word as 0.  Frames are bit-identical either way.
 * rt_debug_primary_entry: the words the context's last render launch was handed, read back (waits for the device); info4 and the layout as
 * rt_debug_subtree_cull's. */
rt_status rt_debug_primary_entry(rt_ctx *ctx, uint32_t *words, int32_t capacity_words, int32_t *info4);
/* the same words computed on the HOST (no device is touched) from a flattened scene.  words: width * height of them, or NULL.  stats12, or NULL, over
 * the unflagged pixels whose jitter cone may enter the root box, by class of their word - `triangle`, `nothing`, 0: {pixels x 3, the centre ray's node
 * steps x 3, its triangle tests x 3}, walked in the kernel's order with the pixel's gate word, then {triangles the predicate looked at, 0, 0} */
rt_status rt_debug_primary_entry_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, uint32_t *words, int64_t *stats12);
/* The sub-entry words (rt_entry.h): a pixel of a jittered view whose entry word is 0 gets a table of 64 such words, one per sub-box of the jitter
 * cube split in four per axis, and a primary ray whose jitter falls in a sub-box with a non-zero word starts as above.  The tables are filled in by
 * the first launch of a view that draws at least RT_AMD_SUBENTRY_SAMPLES samples per pixel (spp x frames; default 2200), else by the view's first
 * reuse.  RT_AMD_PRIMARY_SUBENTRY=0 (read by rt_ctx_create): no tables.  Frames are bit-identical either way.
 * rt_debug_primary_subentry: the tables the context's last render launch was handed, read back (waits for the device), in ascending order of the
 * pixel: pixels[i] = py * width + px, words[64 * i + idx] its sub-word of sub-box idx = jx + 4 jy + 16 jz.  info4 = {1 if that launch was handed
 * a plane with the view's tables else 0, width, height, tables in use}; with pixels or words NULL or too small a capacity only info4 is written.
 * rt_debug_primary_entry reports a pixel that has a table with its own word, 0. */
rt_status rt_debug_primary_subentry(rt_ctx *ctx, uint32_t *pixels, uint32_t *words, int32_t capacity_tables, int32_t *info4);
/* the same tables computed on the HOST (no device is touched).  cap < 0: as many tables as the image's allocation holds, else at most cap (the first
 * pixels in order).  stats8, or NULL: {pixels that want a table, tables handed out, sub-words `triangle`, `nothing`, 0, the table pixels' centre-ray
 * gated node steps summed over their non-zero sub-words, the same over all 64, 0} */
rt_status rt_debug_primary_subentry_host(const rt_flat_view *view, const rt_camera *cam, int32_t antialias, int32_t cap, uint32_t *pixels, uint32_t *words,
                                         int32_t capacity_tables, int64_t *stats8);
/* evaluates one function of the shared math / RNG headers ON THE DEVICE, element-wise, on raw
 * 32-bit patterns (host pointers).  op: 0 rt_logf, 1 rt_cosf, 2 rt_sinf, 3 rt_asinf, 4 rt_acosf,
 * 5 rt_u01, 6 rt_jitter, 7 rt_theta (5-7 take the uint32 hash output), 8 sqrtf, 9 1.0f/x,
 * 10 (float)rt_pow5, 11 / 12 the guarded short 1 / x and sqrt, 13 / 15 rt_logf_0_1(rt_u01(hash)) with the short / the operator's division, 14 rt_cosf_0_2pi(rt_theta(hash)):
 * the Box-Muller calls on a hash output */
rt_status rt_debug_eval(rt_ctx *ctx, int32_t op, const uint32_t *in, uint32_t *out, int32_t n);
/* test hook: the device code's short 1 / x and sqrt(x) against the compiler's IEEE expansions for all 2^32 inputs; out4 = {differing
 * inputs inside the reciprocal's range, inputs inside it, the same two for the square root}.  (The reference divides and takes roots
 * with CUDA's IEEE operators, src/utils.cu:118-128, src/objects.cu:40-79,135-163; the short forms are the same function there.) */
rt_status rt_debug_exhaustive(rt_ctx *ctx, unsigned long long *out4);
/* 48 section counters / timers of a development build compiled with -DRT_STATS (all zero otherwise) */
rt_status rt_debug_read_stats(rt_ctx *ctx, unsigned long long *out48);

const char *rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
