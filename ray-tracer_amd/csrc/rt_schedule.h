/*
 * rt_schedule.h — the host arithmetic of the render schedule: which kernel shape a scene runs, which tiles a launch renders,
 * where their pixels go, in which order its waves take them, and which rank of a multi-GPU call renders which.  Plain
 * functions of vectors and scalars; no HIP.  Any order renders the same image: the schedule only decides how long a launch
 * takes ("Multi-frame launches and their schedule").  A tile is 8 x 8 pixels; "local tile" t of a launch is its
 * t-th, image tile tiles[t].
 * Header only: rt_capi.cpp, and the host-only sanitizer build of it, need nothing else to link.
 */
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <vector>

#include "rt_amd.h"
#include "rt_device_scene.h"

namespace rt_sched {

/* the refined one-frame order moves at most this many measured tiles to its front */
constexpr uint32_t HEAVY_TOP = 1024;
/* a new view's first launch is preceded by a one-sample-per-pixel pilot from this many samples per pixel on */
constexpr int PILOT_MIN_SPP = 32;

/* a stride near n / golden ratio, coprime to n (1 for n <= 2) */
inline uint32_t coprime_stride(uint32_t n)
{
    auto gcd = [](uint32_t x, uint32_t y) { while (y) { uint32_t t = x % y; x = y; y = t; } return x; };
    if (n <= 2u) return 1u;
    uint32_t st = (uint32_t)(n * 0.6180339887) | 1u;
    while (gcd(st, n) != 1u) st += 2u;
    return st % n ? st % n : 1u;
}

/* appends cls[(i * st) % m] for i < m, st = coprime_stride(m): the m entries spread out, so that neighbouring tickets
 * (waves of one workgroup, workgroups of one CU) take tiles far apart */
inline void append_scattered(const uint32_t *cls, uint32_t m, std::vector<uint32_t> &out)
{
    const uint32_t st = coprime_stride(m);
    for (uint32_t i = 0; i < m; i++) out.push_back(cls[(size_t)(((uint64_t)i * st) % m)]);
}

/* What is wrong with a tile spec for an image of tiles_x x tiles_y tiles (nullptr: nothing).  Listed tiles are checked
 * here for their number only: tiles_in_image / view_tiles check the indices. */
inline const char *tile_spec_error(const rt_tile_spec &t, int tiles_x, int tiles_y)
{
    if (t.tile_list) return t.num_tiles < 0 || t.num_tiles > tiles_x * tiles_y ? "bad tile spec (num_tiles)" : nullptr;
    if (t.band_rows <= 0 || (t.band_rows & 7) || t.band_stride <= 0 || t.band_first < 0 || t.band_first >= t.band_stride)
        return "bad tile spec (band_rows must be a positive multiple of 8, 0 <= band_first < band_stride)";
    return nullptr;
}

/* the spec of a launch that renders the whole image in place: every band of 8 rows, nothing listed, not compact */
inline rt_tile_spec whole_image_spec()
{
    rt_tile_spec t{};
    t.band_rows = 8;
    t.band_stride = 1;
    return t;
}

inline bool tiles_in_image(const uint32_t *list, int32_t n, int tiles_x, int tiles_y)
{
    for (int32_t i = 0; i < n; i++)
        if (list[i] >= (uint32_t)(tiles_x * tiles_y)) return false;
    return true;
}

/* The output layout of a launch with a valid tile spec over a width x height image: which tiles it renders and where their
 * pixels go.  A full layout writes them in place in the frame; a compact one packs the owned bands one after another (a
 * ragged last band padded to a whole one), or the listed tiles, 192 floats each in list order.  A list counts as bands
 * of 8 rows, all of them (8 / 0 / 1, as the kernel sees it). */
struct Layout {
    int width = 0, height = 0, tiles_x = 0;
    bool compact = false, listed = false;
    int band_rows = 8, band_first = 0, band_stride = 1;
    int num_tiles = 0;                   /* the tiles the launch renders */

    Layout() = default;
    Layout(const rt_tile_spec &t, int w, int h)
        : width(w), height(h), tiles_x((w + 7) / 8), compact(t.compact != 0), listed(t.tile_list != nullptr), band_rows(listed ? 8 : t.band_rows),
          band_first(listed ? 0 : t.band_first), band_stride(listed ? 1 : t.band_stride), num_tiles(listed ? t.num_tiles : owned_rows() / 8 * tiles_x) {}
    int bands_total() const { return (height + band_rows - 1) / band_rows; }        /* the image's bands, a ragged last one included */
    int owned_bands() const { const int t = bands_total(); return t > band_first ? (t - band_first + band_stride - 1) / band_stride : 0; }
    int owned_rows() const { return owned_bands() * band_rows; }        /* a ragged last band counts whole (rt_tile_owned_rows) */
    int band(int k) const { return band_first + k * band_stride; }      /* the k-th owned band's index in the image */
    int rows_of(int b) const { return std::min(band_rows, height - b * band_rows); }   /* band b's rows inside the image */
    int whole_bands() const { const int n = owned_bands(); return n > 0 && rows_of(band(n - 1)) < band_rows ? n - 1 : n; }   /* (all but a ragged last) */
    bool whole_frame() const { return !compact && !listed && band_stride == 1; }
    size_t band_floats() const { return (size_t)band_rows * (size_t)width * 3; }
    size_t compact_floats() const { return listed ? (size_t)num_tiles * 192 : (size_t)owned_bands() * band_floats(); }
    size_t plane_floats() const { return compact ? compact_floats() : (size_t)height * (size_t)width * 3; }   /* one plane of the layout */
};

/* A valid spec's tiles: tiles[t] is local tile t's index in a width x height image.  A list is taken as it is (false if
 * an index is outside the image or listed twice); bands give their rows of tiles, band after band. */
inline bool view_tiles(const rt_tile_spec &t, int width, int height, std::vector<uint32_t> &tiles)
{
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (t.tile_list) {
        const uint32_t n = (uint32_t)t.num_tiles;
        std::vector<char> seen((size_t)tiles_x * tiles_y, 0);
        tiles.assign(n, 0u);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t g = t.tile_list[i];
            if (g >= (uint32_t)(tiles_x * tiles_y) || seen[g]) return false;
            seen[g] = 1;
            tiles[i] = g;
        }
        return true;
    }
    const Layout L(t, width, height);
    const int band_tiles = L.band_rows / 8 * tiles_x;       /* (a band's tiles are consecutive in the image) */
    tiles.clear();
    for (int k = 0; k < L.owned_bands(); k++)
        for (int g = L.band(k) * band_tiles; g < (L.band(k) + 1) * band_tiles; g++) tiles.push_back((uint32_t)g);
    return true;
}

/* Does the centre ray of image tile `tile` enter the root box of a mesh, enlarged by a margin?  What the guessed orders below class a
 * tile by, before anything is measured.  cam: rt_kernel_args::cam (cam_pos, tl_pixel_pos, delta_u, delta_v).  Host float math, a
 * heuristic only. */
inline bool centre_ray_enters_mesh(uint32_t tile, int tiles_x, const float cam[12], const std::vector<rt_object> &objects)
{
    const int ty = (int)(tile / (uint32_t)tiles_x), tx = (int)(tile % (uint32_t)tiles_x);
    const float px = tx * 8 + 4.0f, py = ty * 8 + 4.0f;
    float d[3], o[3];
    for (int k = 0; k < 3; k++) { o[k] = cam[k]; d[k] = cam[3 + k] + cam[6 + k] * px + cam[9 + k] * py - o[k]; }
    bool hit = false;
    for (size_t m = 0; m < objects.size() && !hit; m++) {
        const rt_object &ob = objects[m];
        if (ob.type != RT_OBJ_MESH) continue;
        float tmin = 0.0f, tmax = 3.0e38f;
        for (int k = 0; k < 3; k++) {
            /* grow the box by a margin: the tile is 8 pixels wide and paths leave it */
            const float ext = 0.15f * (ob.v[3 + k] - ob.v[k]) + 1e-3f;
            const float inv = 1.0f / d[k];
            float t1 = (ob.v[k] - ext - o[k]) * inv, t2 = (ob.v[3 + k] + ext - o[k]) * inv;
            if (t1 > t2) { float s = t1; t1 = t2; t2 = s; }
            if (t1 > tmin) tmin = t1;
            if (t2 < tmax) tmax = t2;
        }
        hit = tmin <= tmax;
    }
    return hit;
}

/* The first guess of a view's order (ticket -> local tile), before anything is measured: tiles whose centre ray enters
 * the root box of a mesh, enlarged by a margin, first, then the others; each class scattered.  cam: rt_kernel_args::cam. */
inline std::vector<uint32_t> guessed_order(const std::vector<uint32_t> &tiles, int tiles_x, const float cam[12], const std::vector<rt_object> &objects)
{
    const uint32_t n = (uint32_t)tiles.size();
    std::vector<uint32_t> heavy, light;
    for (uint32_t i = 0; i < n; i++) (centre_ray_enters_mesh(tiles[i], tiles_x, cam, objects) ? heavy : light).push_back(i);
    std::vector<uint32_t> order;
    order.reserve(n);
    append_scattered(heavy.data(), (uint32_t)heavy.size(), order);
    append_scattered(light.data(), (uint32_t)light.size(), order);
    return order;
}

/* The ticket -> (tile | view << RT_JOB_FRAME_SHIFT) table of a views launch (rt_render_views_device): n_views cameras (cams: 12 floats
 * each, as rt_kernel_args::cam) over the n_tiles tiles of a whole image, tile t being image tile t.  Every view's tiles are classed by that
 * view's own centre rays, each class scattered.  First the heavy jobs, round-robin over the views, so that every view's long jobs start
 * at once; then the light ones, view by view.  Every (tile, view) pair appears exactly once.  A guess, like guessed_order: nothing of
 * these views has been measured. */
inline void views_job_order(uint32_t n_tiles, int tiles_x, const float *cams, uint32_t n_views, const std::vector<rt_object> &objects, std::vector<uint32_t> &jobs)
{
    std::vector<std::vector<uint32_t>> heavy(n_views), light(n_views);
    std::vector<uint32_t> cls;
    size_t longest = 0;
    for (uint32_t v = 0; v < n_views; v++) {
        std::vector<uint32_t> h, l;
        for (uint32_t t = 0; t < n_tiles; t++) (centre_ray_enters_mesh(t, tiles_x, cams + 12 * (size_t)v, objects) ? h : l).push_back(t);
        append_scattered(h.data(), (uint32_t)h.size(), heavy[v]);
        append_scattered(l.data(), (uint32_t)l.size(), light[v]);
        longest = std::max(longest, heavy[v].size());
    }
    jobs.clear();
    jobs.reserve((size_t)n_tiles * n_views);
    for (size_t r = 0; r < longest; r++)
        for (uint32_t v = 0; v < n_views; v++)
            if (r < heavy[v].size()) jobs.push_back(heavy[v][r] | (v << RT_JOB_FRAME_SHIFT));
    for (uint32_t v = 0; v < n_views; v++)
        for (uint32_t t : light[v]) jobs.push_back(t | (v << RT_JOB_FRAME_SHIFT));
}

/* The order once the tiles are measured: the HEAVY_TOP mesh tiles (bit 0 of cost[t]: a ray of the tile entered a mesh) of
 * largest cost, most expensive first and scattered, then every other tile in `order`'s order.  Returns how many lead. */
inline uint32_t refined_order(const std::vector<uint32_t> &order, const std::vector<uint32_t> &cost, std::vector<uint32_t> &out)
{
    const uint32_t n = (uint32_t)order.size();
    std::vector<uint32_t> idx;
    idx.reserve(n);
    for (uint32_t t : order) if (cost[t] & 1u) idx.push_back(t);          /* tiles with a ray in a mesh */
    /* by the tile's summed cost (by its peak pixel instead, same-box A/B, one 1080p frame: monkey 526 against 509 ms, cube 178
     * against 171, reference scene 0 3,083 against 3,104) */
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
    const uint32_t top = HEAVY_TOP < (uint32_t)idx.size() ? HEAVY_TOP : (uint32_t)idx.size();
    out.clear();
    out.reserve(n);
    append_scattered(idx.data(), top, out);
    std::vector<char> taken(n, 0);
    for (uint32_t i = 0; i < top; i++) taken[idx[i]] = 1;
    for (uint32_t t : order) if (!taken[t]) out.push_back(t);
    return top;
}

/* The ticket -> (tile | frame << RT_JOB_FRAME_SHIFT) table of a multi-frame launch, longest job first: the mesh tiles by
 * decreasing peak pixel cost, the frames of a tile together; the other tiles follow frame by frame in `order`'s order. */
inline void build_job_order(const std::vector<uint32_t> &order, const std::vector<uint32_t> &cost, const std::vector<uint32_t> &peak,
                            uint32_t frames, std::vector<uint32_t> &jobs)
{
    const uint32_t n = (uint32_t)order.size();
    std::vector<uint32_t> idx;
    idx.reserve(n);
    for (uint32_t t : order) if (cost[t] & 1u) idx.push_back(t);
    /* a job lasts as long as its longest pixel: by decreasing peak pixel cost (measured at N = 8, 1024 spp: ordering by
     * the tile's SUM left a rank in four with a long pixel started late - ranks 611-718 ms; by peak 612-631) */
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return peak[x] > peak[y]; });
    const uint32_t top = (uint32_t)idx.size();
    jobs.clear();
    jobs.reserve((size_t)n * frames);
    /* by decreasing cost, the frames of a tile together */
    for (uint32_t r = 0; r < top; r++)
        for (uint32_t f = 0; f < frames; f++) jobs.push_back(idx[r] | (f << RT_JOB_FRAME_SHIFT));
    /* everything else frame by frame, in the launch's tile order */
    std::vector<char> taken(n, 0);
    for (uint32_t r = 0; r < top; r++) taken[idx[r]] = 1;
    for (uint32_t f = 0; f < frames; f++)
        for (uint32_t t : order) if (!taken[t]) jobs.push_back(t | (f << RT_JOB_FRAME_SHIFT));
}

#define RT_LDS_LIMIT 163840   /* 160 KiB per CU / per workgroup on gfx950 */
#define RT_MAX_BLOCKS_PER_CU 6

/* The development overrides of a scene's kernel shape, as read from the environment */
struct ShapeOverrides {
    bool threads_set = false;
    int threads = 0;              /* RT_AMD_THREADS: the workgroup size (256, 512, 768 or 1024) of the staged placements - the scene in LDS, the hybrid */
    bool hybrid = true;           /* RT_AMD_SCENE_MODE=0 turns the hybrid kernels off */
    int blocks_per_cu = 0;        /* RT_AMD_BLOCKS_PER_CU: replaces the probed figure when 1..8 */
};

/* the kernel shape a scene runs, the dynamic LDS it launches with, and how many of its workgroups are resident on a CU */
struct KernelShape {
    rt_shape shape{};
    size_t lds_bytes = 0;
    int blocks_per_cu = 1;
};

/* The kernel shape of a scene with a blob of blob_bytes, the first prefix_bytes of it before the triangles, and per_thread
 * bytes of traversal stack per lane (0 without a mesh).  probe(shape, lds_bytes) is the runtime's count of resident
 * workgroups, clamped to [1, RT_MAX_BLOCKS_PER_CU] here; it is called for the candidates in RT_SHAPES' order.  On an error
 * returns its status and sets *err.
 *   The whole scene in LDS (every workgroup stages its own copy) when a shape fits: the one with the most resident waves per
 *   CU, on a tie the earlier one of RT_SHAPES - the smaller workgroup without a mesh (six 256-thread workgroups unless the
 *   object list is so long that only one or two copies fit), the larger with one (fewer copies to stage).
 *   Else, for a mesh, everything before the triangles in LDS when that fits (a depth-10 tree is at most 1,023 nodes whatever
 *   the triangle count), the triangles from global memory: worth it while at least half a CU's wave slots stay filled.
 *   Else the scene in global memory (L2-resident), LDS holding only the traversal stacks.
 *   RT_AMD_THREADS leaves the two staged placements only their shape of that size: one that does not fit, or that the placement
 *   has no shape of (a 256-thread hybrid), passes the scene on to the next placement.  The global shapes are one per mesh flag
 *   and ignore it. */
template <class Probe>
inline rt_status choose_shape(bool has_mesh, size_t blob_bytes, size_t prefix_bytes, size_t per_thread, const ShapeOverrides &o, Probe &&probe,
                              KernelShape &out, const char **err)
{
    if (o.threads_set && o.threads != 256 && o.threads != 512 && o.threads != 768 && o.threads != 1024) {
        *err = "RT_AMD_THREADS must be 256, 512, 768 or 1024";
        return RT_ERR_INVALID;
    }
    auto blocks = [&](rt_shape s, size_t lds) { return std::min(std::max(probe(s, lds), 1), RT_MAX_BLOCKS_PER_CU); };
    auto best_of = [&](int mode, size_t scene_bytes) {
        int best_waves = 0;
        for (const rt_shape &s : RT_SHAPES) {
            if (s.has_mesh != (int)has_mesh || s.mode != mode) continue;
            if (o.threads_set && o.threads != s.threads) continue;       /* (a size no shape of the placement has: on to the next placement) */
            const size_t lds = scene_bytes + per_thread * (size_t)s.threads;
            if (lds > RT_LDS_LIMIT) continue;
            const int nb = blocks(s, lds);
            if (nb * (s.threads / 64) > best_waves) { best_waves = nb * (s.threads / 64); out = {s, lds, nb}; }
        }
        return best_waves > 0;
    };
    if (!best_of(RT_SCENE_LDS, blob_bytes) && !(o.hybrid && best_of(RT_SCENE_HYBRID, prefix_bytes))) {   /* (hybrid shapes have a mesh) */
        /* (one global shape per mesh flag: five or six waves per SIMD as 5-6 x 256 threads were measured on the 50,880- and
         * 6,000-triangle scenes: 80.3 / 80.2 against 80.6 Msamples/s and 57.4 / 57.5 against 57.5 - the path is bound by the
         * L1's address processing, not by latency: profiles/r04/experiments/big_mesh_global_5_waves.txt, pmc_vmem_sphere50k.txt) */
        const rt_shape s = *std::find_if(std::begin(RT_SHAPES), std::end(RT_SHAPES),
                                         [&](const rt_shape &t) { return t.has_mesh == (int)has_mesh && t.mode == RT_SCENE_GLOBAL; });
        const size_t lds = per_thread * (size_t)s.threads;
        if (lds > RT_LDS_LIMIT) {
            *err = "BVH too deep for the per-lane LDS traversal stack";
            return RT_ERR_UNSUPPORTED;
        }
        /* (a 256-thread workgroup is admitted at most 6 times at this kernel's SGPR count, whatever the API says:
         * MI355X_MICROARCH.md, residency; surplus workgroups would only queue behind the resident ones) */
        out = {s, lds, blocks(s, lds)};
    }
    if (o.blocks_per_cu >= 1 && o.blocks_per_cu <= 8) out.blocks_per_cu = o.blocks_per_cu;
    return RT_OK;
}

/* The render kernel's scheduling knobs (RT_AMD_*) as a context holds them; none changes an image (tests/test_gpu_shapes.py renders
 * with each control path forced) */
struct Knobs {
    int work_threshold = RT_DEF_WORK_THRESHOLD;      /* lanes; RT_AMD_WORK_THRESHOLD */
    int descend_keep = RT_DEF_DESCEND_KEEP;       /* RT_AMD_DESCEND_KEEP (0..64): 0 = run every descent to its end */
    bool descend_keep_given = false;              /* RT_AMD_DESCEND_KEEP was set to an accepted value: every kernel gets it as it is (render_descend_keep) */
    int ready_break = RT_DEF_READY_BREAK;        /* lanes; RT_AMD_READY_BREAK; 65 = never */
    int hit_break = RT_DEF_HIT_BREAK;          /* lanes; RT_AMD_HIT_BREAK */
    /* RT_AMD_HIT_LOW, RT_AMD_MIX_BREAK (0 = that rule off; -1 = not set: the default of the scene's workgroup shape).  The kernel gets
     * min(hit_low, hit_break): see kernel_knobs */
    int hit_low = RT_DEF_HIT_LOW, mix_break = -1;
    int shade_batch = RT_DEF_SHADE_BATCH;        /* lanes; RT_AMD_SHADE_BATCH (1..64) */
};

/* the environment variable of each knob and the values rt_ctx_create accepts for it (anything else leaves the default) */
struct KnobRange {
    const char *env;
    int Knobs::*field;
    int lo, hi;
};
inline constexpr KnobRange KNOB_RANGES[] = {
    {"RT_AMD_WORK_THRESHOLD", &Knobs::work_threshold, 1, 64}, {"RT_AMD_DESCEND_KEEP", &Knobs::descend_keep, 0, 64},
    {"RT_AMD_HIT_BREAK", &Knobs::hit_break, 1, 65},           {"RT_AMD_HIT_LOW", &Knobs::hit_low, 0, 65},
    {"RT_AMD_MIX_BREAK", &Knobs::mix_break, 0, 130},          {"RT_AMD_SHADE_BATCH", &Knobs::shade_batch, 1, 64},
    {"RT_AMD_READY_BREAK", &Knobs::ready_break, 1, 65},
};

/* what a launch of a `threads`-wide workgroup hands the render kernel for the knobs (rt_kernel_args' fields of the same names) */
struct KernelKnobs {
    int work_threshold, descend_keep, ready_break, hit_break, hit_low, mix_break, shade_batch;
};

/* The knobs as the kernel reads them.  The mix rule (hit_low, mix_break) is off when either of its knobs is 0: hit_low then equals
 * hit_break and mix_break is out of reach.
 * hit_low <= hit_break always, a larger RT_AMD_HIT_LOW is clamped: the traversal loop leaves with a batch of hit_break hits, and the
 * step that shades them takes a batch only from hit_low on (or when fewer than work_threshold lanes traverse).  With hit_break <=
 * hits < hit_low and nothing else to do the wave would leave the loop, shade nothing and come back for ever;
 * tests/sanitize/capi_host_fuzz.cpp (check_progress) enumerates every accepted knob value and wave state for that. */
inline KernelKnobs kernel_knobs(const Knobs &k, int threads)
{
    const int mix_break = k.mix_break >= 0 ? k.mix_break : (threads == 1024 ? RT_DEF_MIX_BREAK_1024 : RT_DEF_MIX_BREAK);
    const bool mix = k.hit_low > 0 && mix_break > 0;
    KernelKnobs a;
    a.work_threshold = k.work_threshold;
    a.descend_keep = k.descend_keep;
    a.ready_break = k.ready_break;
    a.hit_break = k.hit_break;
    a.hit_low = mix ? std::min(k.hit_low, k.hit_break) : k.hit_break;
    a.mix_break = mix ? mix_break : 1000;
    a.shade_batch = k.shade_batch;
    return a;
}

/* The descend_keep a render, budget or views launch of `shape` runs with: RT_AMD_DESCEND_KEEP as given, whatever the shape (63 means 63/64);
 * without it the default of the shape's descend loop - RT_DEF_DESCEND_KEEP_POP_LDS where the loop pops inside (rt_descend_pops) and the scene is
 * in LDS, RT_DEF_DESCEND_KEEP (k.descend_keep) everywhere else.  The ray kernels take k.descend_keep: their loop is rt_descend. */
inline int render_descend_keep(const Knobs &k, const rt_shape &shape)
{
    if (k.descend_keep_given) return k.descend_keep;
    return shape.has_mesh && shape.mode == RT_SCENE_LDS && rt_descend_pops(shape.threads, shape.mode) ? RT_DEF_DESCEND_KEEP_POP_LDS : k.descend_keep;
}

/* Which of a shape's two render kernels a scene of these traits (RT_TRAIT_*) runs: rt_traits_kernel if it has all three, else
 * rt_render_kernel.  force_generic (RT_AMD_KERNEL_VARIANT=generic, the A side of an A/B and of the tests) keeps rt_render_kernel.  Next to the
 * shape and not part of it: both kernels of a shape have its launch bounds and its LDS.  This form depends on the scene alone (what
 * rt_debug_flatten reports without a device) ... */
inline int choose_variant(uint32_t traits, bool force_generic)
{
    return !force_generic && (traits & RT_TRAITS_ALL) == RT_TRAITS_ALL ? RT_VARIANT_TRAITS_KERNEL : RT_VARIANT_GENERIC;
}
/* ... and on the shape chosen for it: a shape without a traits kernel (rt_variant_traits: the hybrid and the global ones) keeps rt_render_kernel */
inline int choose_variant(uint32_t traits, bool force_generic, const rt_shape &shape)
{
    return rt_variant_traits(shape.has_mesh, shape.mode, shape.threads) != 0 ? choose_variant(traits, force_generic) : RT_VARIANT_GENERIC;
}
/* the value of RT_AMD_KERNEL_VARIANT (may be NULL): "generic" forces rt_render_kernel, anything else leaves the choice to the traits */
inline bool variant_forced_generic(const char *env)
{
    const char *g = "generic";
    if (!env) return false;
    while (*g && *env == *g) { env++; g++; }
    return *g == 0 && *env == 0;
}

/* rt_partition_tiles' owner table dealt out per rank: its tiles (ascending image indices) and, with cost and peak
 * (indexed by image tile), their costs and peaks; without them the rank's costs and peaks stay empty */
inline void deal_tiles(const std::vector<int32_t> &owner, int n_ranks, const uint32_t *cost, const uint32_t *peak, std::vector<std::vector<uint32_t>> &lists,
                       std::vector<std::vector<uint32_t>> &costs, std::vector<std::vector<uint32_t>> &peaks)
{
    lists.assign((size_t)n_ranks, std::vector<uint32_t>());
    costs.assign((size_t)n_ranks, std::vector<uint32_t>());
    peaks.assign((size_t)n_ranks, std::vector<uint32_t>());
    for (size_t g = 0; g < owner.size(); g++) {
        const size_t r = (size_t)owner[g];
        lists[r].push_back((uint32_t)g);
        if (cost) { costs[r].push_back(cost[g]); peaks[r].push_back(peak[g]); }
    }
}

}  // namespace rt_sched
