// The GPU-free entry points of rt_capi.cpp, rt_pipeline_capi.cpp and rt_multi_capi.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; test infrastructure):
// rt_partition_tiles (longest-processing-time-first ownership), rt_tile_owned_rows, the render schedule, the output layout,
// the kernel shape choice and the scheduling knobs' mapping (rt_schedule.h) with their properties asserted, and every entry
// point's refusal of null / bad arguments before it touches HIP.  The three files are compiled as host C++ against the HIP runtime's API header and linked with the runtime library; the
// kernel launchers (rt_render_kernel.h, rt_frame_kernels.h, rt_debug_kernels.h) are replaced by stubs that fail - nothing here reaches a launch.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "rt_amd.h"
#include "rt_device_scene.h"
#include "rt_schedule.h"

#include "launcher_stubs.h"

#define CHECK(cond, what)                                                      \
    do {                                                                       \
        if (!(cond)) { std::fprintf(stderr, "schedule: %s\n", what); return false; } \
    } while (0)

static bool is_permutation_of_iota(const std::vector<uint32_t> &v, uint32_t n)
{
    if (v.size() != n) return false;
    std::vector<char> seen(n, 0);
    for (uint32_t t : v) {
        if (t >= n || seen[t]) return false;
        seen[t] = 1;
    }
    return true;
}

/* the guess's rule on a ray from the origin (doubles): 1 enters the enlarged box, 0 misses it, -1 too close to call */
static int enters_box(const double d[3], const rt_object &ob)
{
    double tmin = 0.0, tmax = 3.0e38;
    for (int k = 0; k < 3; k++) {
        const double ext = 0.15 * ((double)ob.v[3 + k] - ob.v[k]) + 1e-3;
        double t1 = (ob.v[k] - ext) / d[k], t2 = (ob.v[3 + k] + ext) / d[k];
        if (t1 > t2) std::swap(t1, t2);
        tmin = std::max(tmin, t1);
        tmax = std::min(tmax, t2);
    }
    if (!std::isfinite(tmin) || !std::isfinite(tmax) || std::fabs(tmin - tmax) <= 1e-3 * std::fabs(tmax)) return -1;
    return tmin <= tmax ? 1 : 0;
}

/* the output layout of a valid spec whose tile map has n tiles, in full and compact form: its tile count is the map's; a plane
 * holds the frame, or 192 floats per listed tile, or the owned (padded) rows */
static bool check_layout(rt_tile_spec ts, int W, int H, size_t n)
{
    for (ts.compact = 0; ts.compact < 2; ts.compact++) {
        const rt_sched::Layout L(ts, W, H);
        const size_t compact = ts.tile_list ? 192 * n : (size_t)rt_tile_owned_rows(&ts, H) * W * 3;
        CHECK(L.num_tiles >= 0 && (size_t)L.num_tiles == n, "layout: tile count");
        CHECK(L.compact_floats() == compact && L.plane_floats() == (ts.compact ? compact : (size_t)W * H * 3), "layout: plane floats");
        CHECK(L.whole_frame() == (!ts.compact && !ts.tile_list && ts.band_stride == 1), "layout: whole frame");
    }
    return true;
}

/* A band spec's layout for every band_first: the ranks' in-image rows add up to the image, and each rank's band copy (its
 * whole bands, then a ragged last one) stays inside its compact image and the W x H frame and covers exactly its rows. */
static bool check_band_layout(rt_tile_spec ts, int W, int H)
{
    std::vector<int> covered((size_t)H, 0);
    long long rows = 0;
    ts.compact = 1;
    for (ts.band_first = 0; ts.band_first < ts.band_stride; ts.band_first++) {
        const rt_sched::Layout L(ts, W, H);
        const int nb = L.owned_bands(), whole = L.whole_bands();
        CHECK(nb * ts.band_rows == rt_tile_owned_rows(&ts, H) && (whole == nb || whole == nb - 1), "band copy: whole bands");
        for (int k = 0; k < nb; k++) {
            const int b = L.band(k), r0 = b * ts.band_rows, in_image = L.rows_of(b);
            const int copied = k < whole ? ts.band_rows : in_image;      /* exchange: one 2D copy of the whole bands, then the tail */
            rows += in_image;
            CHECK(in_image > 0 && copied == in_image && r0 + copied <= H, "band copy: rows outside the image");
            CHECK((size_t)(k + 1) * L.band_floats() <= L.compact_floats() && (size_t)r0 * W * 3 + (size_t)copied * W * 3 <= (size_t)W * H * 3,
                  "band copy: outside the compact image or the frame");
            for (int r = r0; r < r0 + copied; r++) {
                CHECK((r / ts.band_rows) % ts.band_stride == ts.band_first, "band copy: a row of another rank");
                covered[(size_t)r]++;
            }
        }
    }
    CHECK(rows == H, "band layout: the ranks' in-image rows do not add up to the image");
    for (int c : covered) CHECK(c == 1, "band copy: the ranks do not cover the image once");
    return true;
}

/* one random view through the schedule functions: tile map, output layout, guessed and refined order, job order, stride */
template <class Rng> static bool check_schedule(Rng &rng)
{
    auto irand = [&](long long lo, long long hi) { return (long long)std::uniform_int_distribution<long long>(lo, hi)(rng); };
    const int W = (int)irand(1, 420), H = (int)irand(1, 300);
    const int tiles_x = (W + 7) / 8, tiles_y = (H + 7) / 8, tiles = tiles_x * tiles_y;
    rt_tile_spec ts;
    std::memset(&ts, 0, sizeof ts);
    std::vector<uint32_t> map;
    std::vector<uint32_t> list;
    if (irand(0, 1)) {
        /* bands: every owned band's tiles, row by row; a ragged last band is padded to whole bands */
        ts.band_rows = 8 * (int)irand(1, 6); ts.band_stride = (int)irand(1, 5); ts.band_first = (int)irand(0, ts.band_stride - 1);
        CHECK(rt_sched::tile_spec_error(ts, tiles_x, tiles_y) == nullptr, "a valid band spec refused");
        CHECK(rt_sched::view_tiles(ts, W, H, map), "a band spec has no tile map");
        CHECK(map.size() == (size_t)(rt_tile_owned_rows(&ts, H) / 8) * tiles_x, "band tile count");
        const int rows_per_band = ts.band_rows / 8, bands_total = (H + ts.band_rows - 1) / ts.band_rows;
        std::set<uint32_t> distinct(map.begin(), map.end());
        CHECK(distinct.size() == map.size(), "a band tile mapped twice");
        size_t in_image = 0;
        for (uint32_t g : map) {
            const int band = (int)(g / tiles_x) / rows_per_band;
            CHECK(band < bands_total && band % ts.band_stride == ts.band_first, "a band tile outside the spec's bands");
            in_image += g < (uint32_t)tiles;
        }
        size_t want = 0;
        for (int r = 0; r < tiles_y; r++) want += (r / rows_per_band) % ts.band_stride == ts.band_first ? tiles_x : 0;
        CHECK(in_image == want, "a band tile of the image missing");
        if (!check_layout(ts, W, H, map.size()) || !check_band_layout(ts, W, H)) return false;
    } else {
        std::vector<uint32_t> all((size_t)tiles);
        for (int i = 0; i < tiles; i++) all[(size_t)i] = (uint32_t)i;
        std::shuffle(all.begin(), all.end(), rng);
        list.assign(all.begin(), all.begin() + irand(0, tiles));
        static const uint32_t none = 0;                      /* (an empty vector's data() may be null, which would read as "no list") */
        ts.tile_list = list.empty() ? &none : list.data(); ts.num_tiles = (int32_t)list.size();
        CHECK(rt_sched::tile_spec_error(ts, tiles_x, tiles_y) == nullptr && rt_sched::tiles_in_image(list.data(), ts.num_tiles, tiles_x, tiles_y), "a valid list refused");
        CHECK(rt_sched::view_tiles(ts, W, H, map) && map == list, "list tile map");
        if (!list.empty()) {
            std::vector<uint32_t> bad = list;
            const size_t i = (size_t)irand(0, (long long)bad.size() - 1);
            const bool dup = bad.size() > 1 && irand(0, 1);
            bad[i] = dup ? bad[(i + 1) % bad.size()] : (uint32_t)irand(tiles, tiles + 100);
            rt_tile_spec tb = ts;
            tb.tile_list = bad.data();
            std::vector<uint32_t> m2;
            CHECK(!rt_sched::view_tiles(tb, W, H, m2), "a tile outside the image or listed twice accepted");
            CHECK(dup || !rt_sched::tiles_in_image(bad.data(), tb.num_tiles, tiles_x, tiles_y), "a tile outside the image accepted");
        }
        if (!check_layout(ts, W, H, map.size())) return false;
        ts.num_tiles = tiles + 1;
        CHECK(rt_sched::tile_spec_error(ts, tiles_x, tiles_y) != nullptr, "more tiles than the image has accepted");
    }
    const uint32_t n = (uint32_t)map.size();
    for (uint32_t m : {n, (uint32_t)irand(0, 5000000)}) {
        const uint32_t st = rt_sched::coprime_stride(m);
        uint32_t a = st, b = m;
        while (b) { const uint32_t t = a % b; a = b; b = t; }
        CHECK(m <= 2 ? st == 1 : (a == 1 && st < m), "coprime_stride");
    }
    if (n == 0) return true;

    /* guessed order: a camera at the origin looking down -z, meshes beyond z = -5 (and a sphere, which never counts) */
    float cam[12] = {0, 0, 0, -0.5f, 0.5f * H / W, -1, 1.0f / W, 0, 0, 0, -1.0f / W, 0};
    std::vector<rt_object> objects((size_t)irand(0, 3));
    for (rt_object &ob : objects) {
        std::memset(&ob, 0, sizeof ob);
        ob.type = irand(0, 3) ? RT_OBJ_MESH : RT_OBJ_SPHERE;
        const float z0 = -5.0f - (float)irand(0, 100) * 0.1f;
        ob.v[2] = z0 - 1.0f; ob.v[5] = z0;
        for (int k = 0; k < 2; k++) { ob.v[k] = (float)irand(-40, 40) * 0.1f + 0.0123f; ob.v[3 + k] = ob.v[k] + (float)irand(1, 30) * 0.1f; }
    }
    const std::vector<uint32_t> guess = rt_sched::guessed_order(map, tiles_x, cam, objects);
    CHECK(is_permutation_of_iota(guess, n), "the guessed order is not a permutation");
    long long last_heavy = -1, first_light = (long long)n;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t g = map[guess[k]];
        const double px = (g % tiles_x) * 8 + 4.0, py = (g / tiles_x) * 8 + 4.0;
        const double d[3] = {cam[3] + cam[6] * px + cam[9] * py, cam[4] + cam[7] * px + cam[10] * py, cam[5] + cam[8] * px + cam[11] * py};
        int cls = 0;
        for (const rt_object &ob : objects)
            if (ob.type == RT_OBJ_MESH) {
                const int e = enters_box(d, ob);
                if (e != 0) cls = e == 1 && cls != -1 ? 1 : -1;
                if (cls == 1) break;
            }
        if (cls == 1) last_heavy = k;
        if (cls == 0 && first_light == (long long)n) first_light = k;
    }
    CHECK(last_heavy < first_light, "a light tile ahead of a heavy one in the guessed order");

    /* refined order: the top mesh tiles by summed cost lead, the others keep the guess's order */
    std::vector<uint32_t> cost(n), peak(n);
    const int kind = (int)irand(0, 2);
    for (uint32_t t = 0; t < n; t++) {
        cost[t] = kind == 0 ? (uint32_t)irand(0, 3) : kind == 1 ? (uint32_t)irand(0, 0xffffffffll) : (uint32_t)irand(0, 1) | (uint32_t)irand(0, 50) << 1;
        peak[t] = (uint32_t)irand(0, kind == 0 ? 3 : 100000);
    }
    std::vector<uint32_t> refined;
    const uint32_t top = rt_sched::refined_order(guess, cost, refined);
    uint32_t mesh = 0;
    for (uint32_t t = 0; t < n; t++) mesh += cost[t] & 1u;
    CHECK(is_permutation_of_iota(refined, n), "the refined order is not a permutation");
    CHECK(top == std::min(rt_sched::HEAVY_TOP, mesh), "the refined order's number of leading tiles");
    std::vector<char> lead(n, 0);
    uint32_t least = 0xffffffffu;
    for (uint32_t k = 0; k < top; k++) {
        CHECK(cost[refined[k]] & 1u, "a tile without a mesh among the leading ones");
        lead[refined[k]] = 1;
        least = std::min(least, cost[refined[k]]);
    }
    std::vector<uint32_t> rest;
    for (uint32_t t : guess) {
        if (lead[t]) continue;
        CHECK(!(cost[t] & 1u) || cost[t] <= least, "a more expensive mesh tile left out of the leading ones");
        rest.push_back(t);
    }
    CHECK(std::equal(rest.begin(), rest.end(), refined.begin() + top), "the other tiles do not keep their order");

    /* job order: each (tile, frame) once; the mesh tiles first, frames together and ascending, by non-increasing peak; the
     * others frame by frame in the launch's order */
    const uint32_t frames = (uint32_t)irand(2, RT_MAX_BATCH_FRAMES);
    std::vector<uint32_t> jobs;
    rt_sched::build_job_order(refined, cost, peak, frames, jobs);
    CHECK(jobs.size() == (size_t)n * frames, "job count");
    std::vector<char> done((size_t)n * frames, 0);
    for (uint32_t j : jobs) {
        const uint32_t t = j & RT_JOB_TILE_MASK, f = j >> RT_JOB_FRAME_SHIFT;
        CHECK(t < n && f < frames && !done[(size_t)t * frames + f], "a job outside the launch or listed twice");
        done[(size_t)t * frames + f] = 1;
    }
    for (uint32_t r = 0; r < mesh; r++)
        for (uint32_t f = 0; f < frames; f++) {
            const uint32_t j = jobs[(size_t)r * frames + f], t = j & RT_JOB_TILE_MASK;
            CHECK((cost[t] & 1u) && (j >> RT_JOB_FRAME_SHIFT) == f && t == (jobs[(size_t)r * frames] & RT_JOB_TILE_MASK), "a leading tile's frames are not together in order");
            CHECK(r == 0 || peak[t] <= peak[jobs[(size_t)(r - 1) * frames] & RT_JOB_TILE_MASK], "leading tiles not by non-increasing peak");
        }
    size_t k = (size_t)mesh * frames;
    for (uint32_t f = 0; f < frames; f++)
        for (uint32_t t : refined)
            if (!(cost[t] & 1u)) {
                CHECK(jobs[k] == (t | f << RT_JOB_FRAME_SHIFT), "the other tiles do not follow frame by frame");
                k++;
            }
    return true;
}

/* rt_sched::choose_shape with a fake occupancy probe on random scene sizes and overrides: the shape is built and its LDS fits;
 * blocks per CU are the clamped probe or the override; within the chosen mode no candidate keeps more waves resident and a tie
 * goes to the smaller workgroup without a mesh, the larger with one; the mode is LDS, then hybrid, then global; the two errors */
template <class Rng> static bool check_shape(Rng &rng)
{
    auto irand = [&](long long lo, long long hi) { return (long long)std::uniform_int_distribution<long long>(lo, hi)(rng); };
    const int n_shapes = (int)(sizeof RT_SHAPES / sizeof RT_SHAPES[0]);
    int probe_table[sizeof RT_SHAPES / sizeof RT_SHAPES[0]][4];
    for (auto &row : probe_table) for (int &v : row) v = (int)irand(-1, 9);
    auto probe_of = [&](rt_shape s, size_t lds) { return probe_table[rt_shape_index(s)][(lds >> 12) & 3]; };
    auto blocks_of = [&](rt_shape s, size_t lds) { return std::min(std::max(probe_of(s, lds), 1), RT_MAX_BLOCKS_PER_CU); };
    const bool mesh = irand(0, 2) != 0;
    const size_t per_thread = mesh ? (size_t)irand(2, 27) * 8 : 0;
    const size_t blob = (size_t)std::max(0ll, irand(0, 1) ? irand(0, 2 * RT_LDS_LIMIT) : RT_LDS_LIMIT + irand(-8192, 4096)) & ~(size_t)15;
    const size_t prefix = (size_t)irand(0, (long long)blob) & ~(size_t)15;
    rt_sched::ShapeOverrides o;
    const int forced[] = {256, 512, 768, 1024, 0, 300};
    if (irand(0, 3) == 0) { o.threads_set = true; o.threads = forced[irand(0, 5)]; }
    o.hybrid = irand(0, 3) != 0;
    o.blocks_per_cu = irand(0, 2) == 0 ? (int)irand(-1, 10) : 0;
    std::vector<int> calls;
    rt_sched::KernelShape k;
    const char *err = nullptr;
    const rt_status st = rt_sched::choose_shape(mesh, blob, prefix, per_thread, o, [&](rt_shape s, size_t lds) {
        calls.push_back(rt_shape_index(s));
        return probe_of(s, lds);
    }, k, &err);
    for (size_t i = 1; i < calls.size(); i++) CHECK(calls[i - 1] < calls[i], "shape: probes out of RT_SHAPES' order");
    const bool bad_threads = o.threads_set && o.threads != 256 && o.threads != 512 && o.threads != 768 && o.threads != 1024;
    CHECK((st == RT_ERR_INVALID) == bad_threads, "shape: RT_AMD_THREADS refused iff it is none of the four sizes");
    if (bad_threads) {
        CHECK(calls.empty() && err, "shape: probed before refusing RT_AMD_THREADS");
        return true;
    }
    /* the candidates of a mode: base LDS bytes, and whether a shape takes part (a forced size leaves the staged modes, LDS and hybrid,
     * only their shape of that size; the global shapes are not chosen among) */
    auto base_of = [&](int mode) { return mode == RT_SCENE_LDS ? blob : mode == RT_SCENE_HYBRID ? prefix : (size_t)0; };
    auto candidate = [&](const rt_shape &s, int mode) {
        return s.has_mesh == (int)mesh && s.mode == mode && base_of(mode) + per_thread * (size_t)s.threads <= RT_LDS_LIMIT &&
               !(o.threads_set && o.threads != s.threads) && (mode != RT_SCENE_HYBRID || o.hybrid);
    };
    auto any_of_mode = [&](int mode) { for (const rt_shape &s : RT_SHAPES) if (candidate(s, mode)) return true; return false; };
    const int want_mode = any_of_mode(RT_SCENE_LDS) ? RT_SCENE_LDS : any_of_mode(RT_SCENE_HYBRID) ? RT_SCENE_HYBRID : RT_SCENE_GLOBAL;
    const bool too_deep = want_mode == RT_SCENE_GLOBAL && per_thread * (mesh ? 1024 : 256) > RT_LDS_LIMIT;
    CHECK((st == RT_ERR_UNSUPPORTED) == too_deep, "shape: BVH too deep iff the global kernel's stacks do not fit");
    if (too_deep) {
        CHECK(err, "shape: no message");
        return true;
    }
    CHECK(st == RT_OK, "shape: status");
    const int ki = rt_shape_index(k.shape);
    CHECK(ki >= 0 && ki < n_shapes && k.shape.has_mesh == (int)mesh, "shape: not a built shape of the scene's mesh flag");
    CHECK(k.shape.mode == want_mode, "shape: fallback order LDS, hybrid, global");
    CHECK(!o.threads_set || want_mode == RT_SCENE_GLOBAL || k.shape.threads == o.threads, "shape: a staged shape of another size than RT_AMD_THREADS");
    CHECK(k.lds_bytes == base_of(want_mode) + per_thread * (size_t)k.shape.threads && k.lds_bytes <= RT_LDS_LIMIT, "shape: LDS bytes");
    const bool overridden = o.blocks_per_cu >= 1 && o.blocks_per_cu <= 8;
    CHECK(k.blocks_per_cu == (overridden ? o.blocks_per_cu : blocks_of(k.shape, k.lds_bytes)), "shape: blocks per CU");
    CHECK(overridden || (k.blocks_per_cu >= 1 && k.blocks_per_cu <= RT_MAX_BLOCKS_PER_CU), "shape: blocks per CU out of [1, 6]");
    if (want_mode == RT_SCENE_GLOBAL) return true;
    const int waves = blocks_of(k.shape, k.lds_bytes) * k.shape.threads / 64;
    for (const rt_shape &s : RT_SHAPES) {
        if (!candidate(s, want_mode)) continue;
        const int w = blocks_of(s, base_of(want_mode) + per_thread * (size_t)s.threads) * s.threads / 64;
        CHECK(w <= waves, "shape: a candidate keeps more waves resident");
        CHECK(w < waves || s.threads == k.shape.threads || (mesh ? s.threads < k.shape.threads : s.threads > k.shape.threads), "shape: tie rule");
    }
    return true;
}

/* ---- progress of the render kernel's wave loop under every accepted knob value ------------------------------------------------------
 * rt_render_kernel (rt_render_kernel.h) is a loop of rounds: finish misses, SHADE a batch of hits if the shade condition holds, fetch pixels,
 * generate rays, enter meshes, then run traversal steps until the traversal loop's break condition holds.  The two conditions are the kernel's
 * own statement of them, rt_traversal_yields and RT_ROUND_SHADES of rt_device_scene.h, here on rt_sched::KernelKnobs:
 *   n_hit lanes hold a hit to shade, n_trav == n_active lanes traverse, n_light lanes have cheap work, the rest are done. */

/* the mapping before rt_sched::kernel_knobs existed (rt_capi.cpp filled the kernel's arguments with this expression): kept to show that
 * check_progress tells the two apart */
static rt_sched::KernelKnobs mapping_without_clamp(const rt_sched::Knobs &k, int threads)
{
    const int mix_break = k.mix_break >= 0 ? k.mix_break : (threads == 1024 ? RT_DEF_MIX_BREAK_1024 : RT_DEF_MIX_BREAK);
    rt_sched::KernelKnobs a = rt_sched::kernel_knobs(k, threads);
    a.hit_low = k.hit_low > 0 && mix_break > 0 ? k.hit_low : k.hit_break;
    a.mix_break = k.hit_low > 0 && mix_break > 0 ? mix_break : 1000;
    return a;
}

static const rt_sched::KnobRange &range_of(int rt_sched::Knobs::*field)
{
    for (const rt_sched::KnobRange &r : rt_sched::KNOB_RANGES) if (r.field == field) return r;
    std::abort();
}

/* A round changes the wave's state, so the loop ends, whenever
 *   - a lane has cheap work: a missed ray is finished on the spot (px_shade_miss) and the lane generates its next one; a lane without a pixel
 *     takes one (px_fetch) or, the tickets used up, is done; a lane with a ray to generate generates it (px_gen); a lane between meshes
 *     moves on to the next mesh or to its hit.  Each of these happens in the round unconditionally - no knob gates them - and moves the lane
 *     forward in a finite sequence (meshes of the scene, bounces of a sample, samples of a pixel, pixels of the launch);
 *   - or a traversal step runs (a traversal is finite);
 *   - or a batch of hits is shaded.
 * What is left are the waves WITHOUT a cheap-work lane: every lane holds a hit, traverses or is done, and nothing in the round changes that
 * unless it shades or steps.  With a mesh: if the traversal loop breaks before its first step, the round that follows sees the same counts
 * and must shade - "breaks" implies "shades", for every such state and every knob value rt_ctx_create accepts (rt_sched::KNOB_RANGES):
 * work_threshold, hit_break and hit_low over their whole ranges; mix_break unset, 0, 1, both defaults and 130; 256- and 1024-thread shapes
 * (the default mix_break differs).  ready_break is at least 1 and n_light is 0, so that term is false whatever its value; descend_keep and
 * shade_batch are in neither condition.  Without a mesh there is no traversal loop: a wave whose lanes all hold a hit or are done has no
 * "others", for every shade_batch.  Returns the number of (knobs, state) pairs checked, or -1 and the first counter-example on stderr. */
template <class Mapping> static long long check_progress(Mapping mapping, const rt_sched::Knobs *only = nullptr)
{
    using rt_sched::Knobs;
    const rt_sched::KnobRange &wt = range_of(&Knobs::work_threshold), &hb = range_of(&Knobs::hit_break), &hl = range_of(&Knobs::hit_low),
                              &mb = range_of(&Knobs::mix_break), &sb = range_of(&Knobs::shade_batch), &rb = range_of(&Knobs::ready_break);
    if (rb.lo < 1 || mb.lo > 0 || mb.hi < 130 || wt.lo < 1) { std::fprintf(stderr, "progress: the accepted ranges are not the ones this check was written for\n"); return -1; }
    const int mixes[] = {-1, 0, 1, RT_DEF_MIX_BREAK, RT_DEF_MIX_BREAK_1024, 130};
    long long checked = 0;
    for (int threads : {256, 1024})
        for (int mix : mixes)
            for (int w = wt.lo; w <= wt.hi; w++)
                for (int b = hb.lo; b <= hb.hi; b++)
                    for (int l = hl.lo; l <= hl.hi; l++) {
                        Knobs k;
                        k.mix_break = mix; k.work_threshold = w; k.hit_break = b; k.hit_low = l;
                        if (only && (only->mix_break != mix || only->work_threshold != w || only->hit_break != b || only->hit_low != l)) continue;
                        const rt_sched::KernelKnobs a = mapping(k, threads);
                        for (int n_hit = 1; n_hit <= 63; n_hit++)
                            for (int n_active = 1; n_hit + n_active <= 64; n_active++) {
                                checked++;
                                if (rt_traversal_yields(a, n_hit, n_active, 0) && !RT_ROUND_SHADES(a, true, n_hit, n_active, false)) {
                                    std::fprintf(stderr, "progress: %d threads, RT_AMD_MIX_BREAK%s%d RT_AMD_WORK_THRESHOLD=%d RT_AMD_HIT_BREAK=%d RT_AMD_HIT_LOW=%d (kernel: hit_low %d, mix_break %d): "
                                                 "a wave of %d hits, %d traversing, %d done leaves the traversal loop and shades nothing\n",
                                                 threads, mix < 0 ? " unset: " : "=", mix < 0 ? a.mix_break : mix, w, b, l, a.hit_low, a.mix_break, n_hit, n_active, 64 - n_hit - n_active);
                                    return -1;
                                }
                            }
                    }
    if (only) return checked;
    for (int s = sb.lo; s <= sb.hi; s++) {
        Knobs k;
        k.shade_batch = s;
        const rt_sched::KernelKnobs a = mapping(k, 256);
        for (int n_hit = 1; n_hit <= 64; n_hit++) {
            checked++;
            if (!RT_ROUND_SHADES(a, false, n_hit, 0, false)) { std::fprintf(stderr, "progress: no mesh, RT_AMD_SHADE_BATCH=%d: %d hits and no other lane, nothing shaded\n", s, n_hit); return -1; }
        }
    }
    return checked;
}

/* kernel_knobs on every accepted value: what it promises beside progress */
static bool check_knob_mapping()
{
    using rt_sched::Knobs;
    for (int threads : {256, 512, 768, 1024})
        for (int mix = -1; mix <= range_of(&Knobs::mix_break).hi; mix++)
            for (int b = range_of(&Knobs::hit_break).lo; b <= range_of(&Knobs::hit_break).hi; b++)
                for (int l = range_of(&Knobs::hit_low).lo; l <= range_of(&Knobs::hit_low).hi; l++) {
                    Knobs k;
                    k.mix_break = mix; k.hit_break = b; k.hit_low = l;
                    const rt_sched::KernelKnobs a = rt_sched::kernel_knobs(k, threads);
                    const int mb = mix >= 0 ? mix : threads == 1024 ? RT_DEF_MIX_BREAK_1024 : RT_DEF_MIX_BREAK;
                    const bool on = l > 0 && mb > 0;
                    CHECK(a.hit_low <= a.hit_break && a.hit_break == b, "knobs: hit_low above hit_break");
                    CHECK(a.hit_low == (on ? std::min(l, b) : b) && a.mix_break == (on ? mb : 1000), "knobs: the mix rule");
                    CHECK(a.work_threshold == k.work_threshold && a.ready_break == k.ready_break && a.descend_keep == k.descend_keep && a.shade_batch == k.shade_batch, "knobs: passed through");
                }
    const Knobs def;
    const rt_sched::KernelKnobs d = rt_sched::kernel_knobs(def, 256), e = rt_sched::kernel_knobs(def, 1024);
    CHECK(d.hit_low == RT_DEF_HIT_LOW && d.mix_break == RT_DEF_MIX_BREAK && e.mix_break == RT_DEF_MIX_BREAK_1024 && d.hit_break == RT_DEF_HIT_BREAK, "knobs: the defaults");
    return true;
}

/* `progress`: the whole enumeration on the library's mapping.  `progress-without-clamp`: the same on the mapping before the clamp, which must
 * produce a counter-example (first the enumeration's, then the one RT_AMD_HIT_BREAK=8 alone gives): exit status 0 iff it does. */
static int progress_main(const char *mode)
{
    if (!std::strcmp(mode, "progress")) {
        const long long n = check_progress(rt_sched::kernel_knobs);
        if (n < 0 || !check_knob_mapping()) return 1;
        std::printf("capi host fuzz: progress holds for %lld (knobs, wave state) pairs\n", n);
        return 0;
    }
    rt_sched::Knobs eight;
    eight.hit_break = 8;
    const bool found = check_progress(mapping_without_clamp) < 0 && check_progress(mapping_without_clamp, &eight) < 0;
    const bool clean = check_progress(rt_sched::kernel_knobs, &eight) > 0;
    std::printf("capi host fuzz: without the clamp %s; with it RT_AMD_HIT_BREAK=8 %s\n", found ? "counter-examples found" : "NO counter-example", clean ? "makes progress" : "FAILS");
    return found && clean ? 0 : 1;
}

/* rt_partition_tiles' owner table dealt out: a partition of the image's tiles, with each tile's cost and peak */
static bool check_deal(const std::vector<int32_t> &owner, int n_ranks, const std::vector<uint32_t> &cost, const std::vector<uint32_t> &peak)
{
    std::vector<std::vector<uint32_t>> lists, costs, peaks;
    rt_sched::deal_tiles(owner, n_ranks, cost.data(), peak.data(), lists, costs, peaks);
    CHECK(lists.size() == (size_t)n_ranks && costs.size() == (size_t)n_ranks && peaks.size() == (size_t)n_ranks, "deal: number of ranks");
    std::vector<int> seen(owner.size(), 0);
    for (int r = 0; r < n_ranks; r++) {
        CHECK(costs[(size_t)r].size() == lists[(size_t)r].size() && peaks[(size_t)r].size() == lists[(size_t)r].size(), "deal: costs per tile");
        for (size_t i = 0; i < lists[(size_t)r].size(); i++) {
            const uint32_t g = lists[(size_t)r][i];
            CHECK(g < owner.size() && owner[g] == r && (i == 0 || lists[(size_t)r][i - 1] < g), "deal: a tile in the wrong rank or out of order");
            CHECK(costs[(size_t)r][i] == cost[g] && peaks[(size_t)r][i] == peak[g], "deal: a tile's cost");
            seen[g]++;
        }
    }
    for (int c : seen) CHECK(c == 1, "deal: not a partition of the image");
    return true;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strncmp(argv[1], "progress", 8)) return progress_main(argv[1]);
    if (!check_knob_mapping()) return 1;
    std::mt19937_64 rng((unsigned long long)(argc > 1 ? std::atoll(argv[1]) : 1));
    const int cases = argc > 2 ? std::atoi(argv[2]) : 1000;
    auto irand = [&](long long lo, long long hi) { return (long long)std::uniform_int_distribution<long long>(lo, hi)(rng); };
    for (int c = 0; c < cases; c++) {
        const int tx = (int)irand(-1, 40), ty = (int)irand(-1, 30), n = (int)irand(-1, 9);
        const long long tiles = (long long)(tx > 0 ? tx : 0) * (ty > 0 ? ty : 0);
        std::vector<uint32_t> cost((size_t)tiles + 1);
        const int kind = (int)irand(0, 3);
        for (auto &x : cost) x = kind == 0 ? 0u : kind == 1 ? (uint32_t)irand(0, 5) : kind == 2 ? (uint32_t)irand(0, 0xffffffffll) : 0xffffffffu;
        std::vector<int32_t> owner((size_t)tiles + 1, -7);
        const rt_status st = rt_partition_tiles(irand(0, 3) ? cost.data() : nullptr, tx, ty, n, owner.data());
        if (st == RT_OK) {
            std::vector<unsigned long long> load((size_t)n, 0ull);
            for (long long i = 0; i < tiles; i++) {
                if (owner[(size_t)i] < 0 || owner[(size_t)i] >= n) { std::fprintf(stderr, "owner out of range\n"); return 1; }
                load[(size_t)owner[(size_t)i]] += cost[(size_t)i];
            }
            if (owner[(size_t)tiles] != -7) { std::fprintf(stderr, "wrote past the end\n"); return 1; }
            std::vector<int32_t> own(owner.begin(), owner.end() - 1);
            std::vector<uint32_t> cs(cost.begin(), cost.end() - 1), pk(cs.size());
            for (auto &x : pk) x = (uint32_t)irand(0, 1000);
            if (!check_deal(own, n, cs, pk)) return 1;
        }
        if (!check_schedule(rng) || !check_shape(rng)) return 1;
        rt_tile_spec ts;
        std::memset(&ts, 0, sizeof ts);
        ts.band_rows = (int32_t)irand(-8, 64); ts.band_first = (int32_t)irand(-1, 5); ts.band_stride = (int32_t)irand(-1, 5);
        (void)rt_tile_owned_rows(&ts, (int32_t)irand(-5, 5000));
        (void)rt_tile_owned_rows(nullptr, 10);
    }
    /* null / bad arguments: refused before HIP is touched (there is no GPU here; rt_ctx_create must say so, not crash) */
    rt_ctx *ctx = nullptr;
    const rt_status cs = rt_ctx_create(0, &ctx);
    if (cs == RT_OK) { rt_ctx_destroy(ctx); std::printf("(a GPU is present: context created and destroyed)\n"); }
    (void)rt_ctx_create(0, nullptr);
    (void)rt_ctx_create(-3, &ctx);
    rt_ctx_destroy(nullptr);
    rt_scene_destroy(nullptr);
    (void)rt_last_error(nullptr);
    int32_t fn = 0;
    (void)rt_render(nullptr, nullptr, nullptr, nullptr, 0, &fn, nullptr);
    (void)rt_render_frames(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &fn, nullptr);
    (void)rt_render_device(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr);
    (void)rt_render_device_batch(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);
    (void)rt_frame_submit(nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    (void)rt_frame_collect(nullptr, 0, nullptr, nullptr);
    (void)rt_frame_collect_host(nullptr, &fn, nullptr);
    (void)rt_frame_wait(nullptr);
    (void)rt_frame_depth(nullptr, 3);
    (void)rt_frames_pending(nullptr);
    (void)rt_tile_costs(nullptr, nullptr, nullptr, nullptr, 0, &fn);
    (void)rt_tiles_copy_device(nullptr, nullptr, nullptr, 8, 8, nullptr, 0, 1, nullptr);
    (void)rt_max_batch_frames(nullptr, 8, 8);
    (void)rt_last_kernel_ms(nullptr, nullptr);
    (void)rt_ctx_synchronize(nullptr);
    (void)rt_render_multi(nullptr, 0, nullptr, nullptr, nullptr, 0, &fn, nullptr);
    (void)rt_render_multi_device(nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr);
    (void)rt_gather(nullptr, nullptr, 8, 8, nullptr, nullptr, nullptr, nullptr);
    (void)rt_peer_access(nullptr, nullptr);
    (void)rt_scene_commit(nullptr, nullptr, nullptr);
    (void)rt_scene_get_info(nullptr, nullptr);
    std::printf("capi host fuzz: %d partitions and deals, %d schedules, %d kernel shapes, sanitizers silent\n", cases, cases, cases);
    return 0;
}
