// What a context remembers about its primary-ray cull plane: rt_cull_host::Plan (ray-tracer_amd/csrc/rt_cull.h), under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU (test infrastructure; tests/test_primary_cull.py compiles and runs it).
// This tests Plan, NOT the C ABI path: a context needs a device (rt_ctx_create fails without one), so rt_capi.cpp's bind_cull cannot run here.
// launch() below restates bind_cull's sequence around the plan - next(), the pre-pass, ran(), used_last - with an allocator that counts, can
// refuse, and owns real memory the "pre-pass" writes to its last word.  What bind_cull adds to that sequence - the event that orders a reader on
// another stream behind the pre-pass, the wait for pipelined frames before the plane is rewritten, the HIP calls' failure paths - is checked only
// on the device (tests/test_gpu_primary_cull.py, and the launch-order tests of tests/test_gpu_streams.py run with the plane bound).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rt_cull.h"

using rt_cull_host::Key;
using rt_cull_host::Plan;
using rt_cull_host::Step;

#define CHECK(cond, what)                                                        \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "cull key: %s (line %d)\n", what, __LINE__); return 1; } \
    } while (0)

struct Device {
    std::vector<uint32_t> plane;
    int allocations = 0, runs = 0;
    bool refuse = false;
    bool grow(size_t words)
    {
        if (refuse) { plane.clear(); plane.shrink_to_fit(); return false; }
        plane.assign(words, 0u);
        plane.shrink_to_fit();
        allocations++;
        return true;
    }
    // the pre-pass: writes every word of the view's plane (ASan sees an allocation that is too small)
    void prepass(const Key &k) { for (size_t i = 0; i < rt_cull_words(k.width, k.height); i++) plane[i] = k.scene_uid; runs++; }
};

// one launch as bind_cull does it: the plane it is handed (null: none)
static const uint32_t *launch(Plan &plan, Device &dev, const Key &k, bool enabled, bool prepass_ok = true)
{
    const Step s = plan.next(k, enabled, [&](size_t words) { return dev.grow(words); });
    if (s == Step::none) return nullptr;
    if (s == Step::run) {
        if (prepass_ok) dev.prepass(k);
        plan.ran(k, prepass_ok);
        if (!prepass_ok) return nullptr;
    }
    plan.used_last = true;
    return dev.plane.data();
}

static Key key(uint32_t uid, float cam0, int w, int h, int aa)
{
    Key k;
    k.scene_uid = uid;
    for (int i = 0; i < 12; i++) k.cam[i] = cam0 + (float)i;
    k.width = w; k.height = h; k.antialias = aa;
    return k;
}

int main(int argc, char **argv)
{
    Plan plan;
    Device dev;
    const Key a = key(1, 0.5f, 96, 64, 1);
    CHECK(rt_cull_words(96, 64) == 192 && rt_cull_words(1, 1) == 2 && rt_cull_words(101, 67) == 212, "words of a plane");
    // a new view runs the pre-pass once; the same view reuses the plane
    CHECK(launch(plan, dev, a, true) && dev.runs == 1 && dev.allocations == 1 && plan.used_last, "first launch of a view");
    CHECK(launch(plan, dev, a, true) && dev.runs == 1 && dev.allocations == 1 && plan.used_last, "same view: reuse");
    // every part of the key invalidates; the allocation stays while the image does not grow
    Key b = a; b.cam[7] = 9.0f;
    CHECK(launch(plan, dev, b, true) && dev.runs == 2 && dev.allocations == 1, "camera changed");
    Key c = b; c.scene_uid = 2;          // a commit, or an update of the scene's geometry (its uid changes)
    CHECK(launch(plan, dev, c, true) && dev.runs == 3 && dev.allocations == 1 && dev.plane[0] == 2u, "scene revision changed");
    Key d = c; d.antialias = 0;
    CHECK(launch(plan, dev, d, true) && dev.runs == 4 && dev.allocations == 1, "antialias changed");
    Key e = d; e.width = 64; e.height = 48;
    CHECK(launch(plan, dev, e, true) && dev.runs == 5 && dev.allocations == 1 && plan.cap_words == 192, "a smaller image keeps the allocation");
    Key f = e; f.width = 200; f.height = 100;
    CHECK(launch(plan, dev, f, true) && dev.runs == 6 && dev.allocations == 2 && plan.cap_words == rt_cull_words(200, 100), "a larger image reallocates");
    CHECK(launch(plan, dev, f, true) && dev.runs == 6, "same view again");
    // back to an earlier view: computed again (one plane per context)
    CHECK(launch(plan, dev, a, true) && dev.runs == 7 && dev.allocations == 2, "an earlier view is computed again");
    // the switch: no plane, and the cached one survives
    CHECK(!launch(plan, dev, a, false) && !plan.used_last && dev.runs == 7, "switched off");
    CHECK(launch(plan, dev, a, true) && dev.runs == 7 && plan.used_last, "switched on again: the plane is still this view's");
    // an allocation failure renders without the plane and does not stick
    Key g = a; g.width = 4000; g.height = 3000;
    dev.refuse = true;
    CHECK(!launch(plan, dev, g, true) && !plan.used_last && !plan.valid && plan.cap_words == 0 && dev.runs == 7, "allocation refused");
    CHECK(!launch(plan, dev, a, true) && dev.runs == 7, "still refused: the old plane is gone with the failed growth");
    dev.refuse = false;
    CHECK(launch(plan, dev, g, true) && dev.runs == 8 && dev.allocations == 3, "allocation possible again");
    // a pre-pass that could not be queued leaves no valid plane: the next launch tries again
    Key h = g; h.cam[0] = -3.0f;
    CHECK(!launch(plan, dev, h, true, false) && !plan.valid && !plan.used_last, "pre-pass failed");
    CHECK(launch(plan, dev, h, true) && dev.runs == 9 && plan.valid, "pre-pass tried again");
    // random walk: the plane handed out always holds the launch's scene uid in every word of its view
    std::mt19937 rng(argc > 1 ? (unsigned)atoi(argv[1]) : 1u);
    for (int it = 0; it < 20000; it++) {
        const Key k = key(1 + rng() % 3, (float)(rng() % 3), 8 + (int)(rng() % 5) * 37, 8 + (int)(rng() % 4) * 29, (int)(rng() % 2));
        dev.refuse = rng() % 17 == 0;
        const bool enabled = rng() % 11 != 0;
        const uint32_t *p = launch(plan, dev, k, enabled, rng() % 13 != 0);
        CHECK(!p || enabled, "a plane although switched off");
        if (p) {
            const size_t n = rt_cull_words(k.width, k.height);
            CHECK(plan.valid && plan.key.same(k) && dev.plane.size() >= n && p[0] == k.scene_uid && p[n - 1] == k.scene_uid, "a stale plane was handed out");
        }
    }
    std::printf("cull key: %d pre-passes, %d allocations, sanitizers silent\n", dev.runs, dev.allocations);
    return 0;
}
