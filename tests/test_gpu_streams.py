"""The launch-order contract of include/rt_amd.h on the device: "asynchronous on hip_stream and ordered like rt_render_device", "one launch in
flight per context", "queued behind frames in flight" - for every device-form entry point, with no host synchronisation between what
produces a call's inputs, the call and what consumes its outputs.

One table of adapters (ADAPTERS), one per device-form entry point and mode.  An adapter knows its device buffers (inputs with their real
content, outputs), how to make the call on a stream, and what to expect: the bytes the same call leaves when it is made fully synchronised
on a fresh context - which test_the_synchronised_results_equal_the_yardsticks ties to the oracle, or the family's yardstick, once per family,
with the helpers the family's own test file uses.

The hazard window is a sleeping stream (torch.cuda._sleep, calibrated once per module), not a big workload: (a) the inputs are copied into
place and the outputs filled with garbage on the caller's stream behind the sleep, so a kernel that ran early reads garbage or is
overwritten; (b) an event behind the call has not completed when the call returns; (c) a second call on another stream of the same context
is ordered behind the first (events), for every shared piece of scratch; (d) calls behind frames in flight; (e) a larger call that regrows
scratch a pending call uses; (f) the pairs of (c) over two contexts.  Sizes are the smallest with ragged tiles and more than one
workgroup's worth of work.  Run with -m gpu on an MI355X."""
import time
import zlib

import numpy as np
import pytest

import adaptive_ref
import views_ref
from denoise_ref import denoise_ref
from test_gpu_occlusion import expected as occlusion_expected
from test_gpu_occlusion import oracle_hits, oracle_visibility
from test_gpu_pipeline import frame_by_frame
from test_gpu_query import _rays, assert_equal_to_oracle, oracle_records, primaries, u32

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 74, 42                        # 10 x 6 tiles, ragged on both axes
SMALL = (24, 16)                     # the small call of case (e)
N_RAYS = 4096 + 17
SPP, LIMIT = 3, 4
AO = dict(samples=4, radius=0.5, bias=1e-3, time_ms=12345)
LIGHT, BIAS = (1.5, 2.0, 0.2), 1e-3
SKY_AOV = (1.0, 1.0, 1.0)
TIMES = [12345, -99, 777]
DENOISE = dict(iterations=2)
PLAN = dict(step_spp=3, max_spp=11, threshold=0.25, floor=0.01)
SCENES = ["three_sphere", "monkey"]  # no mesh; a mesh staged in LDS
IN_GARBAGE, OUT_GARBAGE = 0x01, 0x77  # bytes: a budget of 257 samples, floats of 2e-38 / 5e33 - wrong, and harmless to read
MIN_WINDOW_MS = 20.0

# Where a call waits on the HOST although the header calls its entry point asynchronous (DESIGN.md section 19 has the same table): the
# situations in which (c) and (e) do not require the first call to be still pending when the second returns.  Warm and on its own - case
# (b) - no entry point waits.
WAITS_ON_HOST = {
    "views -> views": "rt_views_capi.cpp:53 hipEventSynchronize(vs.ev_up): the camera table's host copy is rewritten only after the previous call's upload",
    "regrow": "rt_internal.h:40 DevBuf::release -> hipFree: a buffer that must grow is freed, and hipFree waits for the device (DevBuf::grow relies on it)",
    "a view's first launches": "rt_capi.cpp:323 and :339 hipStreamSynchronize: with a mesh the tile order, then the measured costs and the schedule sorted by them, go through locals",
    "tile list recycled": "rt_capi.cpp:67 hipEventSynchronize(dl.ev_up) before the pinned copy is rewritten, :59 hipEventSynchronize(dl.ev) before an entry too small is freed",
    "a frame's plane regrown": "rt_capi.cpp:641 hipEventSynchronize(slot->ev_free): the blend that reads the old plane",
    "frames in flight, view rewritten": "rt_capi.cpp:506 drain_pipeline (:296) and the blocking copy of a new tile list (:512): once or twice per view",
    "the adaptive loop": "rt_adaptive_capi.cpp:203 and :220 hipStreamSynchronize: one per pass for the per-tile planes, one for the total",
    "host form": "the host-buffer forms block by contract: blocking copies and hipDeviceSynchronize (e.g. rt_capi.cpp:832, rt_query_capi.cpp:56)",
}


# ---- adapters ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """one adapter on one scene and image size: inputs (name -> array with the real content), outputs (name -> bytes; a name that is
    also an input is updated in place), call(rt, ctx, scene, ptr, stream) with ptr: name -> device pointer"""

    def __init__(self, key, family, inputs, outputs, call, host=None):
        self.key, self.family, self.inputs, self.outputs, self.call, self.host = key, family, inputs, outputs, call, host


def tile_list(w, h, which):
    n = ((w + 7) // 8) * ((h + 7) // 8)
    ids = list(range(which % 2, n, 2))
    return ids[::-1] if which >= 2 else ids


def _image(rng, w, h, c=3):
    return rng.random((h, w, c), dtype=F) if c > 1 else rng.random((h, w), dtype=F)


def make_case(rt, adapter, name, size=(W, H)):
    """the table: every device-form entry point and mode"""
    w, h = size
    px = w * h
    rng = np.random.default_rng(zlib.crc32(("%s %d %d" % (adapter, w, h)).encode()))
    sky = rt.scenes.CONFIG_SCENES[name or "three_sphere"]()[1]
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, LIMIT, True, sky)
    frame = _image(rng, w, h)
    key = (adapter, name, w, h)
    L1, L2 = tile_list(w, h, 0), tile_list(w, h, 3)
    if adapter == "render_device":
        return Case(key, "render", {"prev": frame}, {"out": px * 12},
                    lambda rt, c, s, p, st: rt.render_device(c, s, cam, rd, TIMES[0], 1, p["out"], d_prev=p["prev"], stream=st))
    if adapter == "render_device bands":
        return Case(key, "render", {"prev": frame}, {"out": px * 12},
                    lambda rt, c, s, p, st: rt.render_device(c, s, cam, rd, TIMES[0], 2, p["out"], d_prev=p["prev"], band_rows=16, band_first=1, band_stride=2, stream=st))
    if adapter == "render_device tile list":
        return Case(key, "render", {"prev": frame}, {"out": len(L1) * 192 * 4},
                    lambda rt, c, s, p, st: rt.render_device(c, s, cam, rd, TIMES[1], 1, p["out"], d_prev=p["prev"], tile_list=L1, compact=True, stream=st))
    if adapter == "render_device_batch":
        return Case(key, "render", {"frame": frame}, {"frame": px * 12},
                    lambda rt, c, s, p, st: rt.render_device_batch(c, s, cam, rd, TIMES, 1, p["frame"], stream=st))
    if adapter == "frame_submit / frame_collect":
        def pipeline(rt, c, s, p, st):
            rt.frame_submit(c, s, cam, rd, TIMES[0])
            rt.frame_submit(c, s, cam, rd, TIMES[1])
            rt.frame_collect(c, 1, p["frame"], stream=st)
            rt.frame_collect(c, 2, p["frame"], stream=st)
        return Case(key, "pipeline", {"frame": frame}, {"frame": px * 12}, pipeline)
    if adapter == "render_views_device other cameras":
        # two views where the others have three, from other places: another camera table, another schedule behind it, other seeds
        others = [rt.Camera(w, h, pos=(-0.25, 0.05, 0.1), rot=(0.0, 0.15, 0.0)), rt.Camera(w, h, pos=(0.0, 0.2, -0.3), rot=(0.1, 0.0, 0.0))]
        return Case(key, "views", {}, {"frames": 2 * px * 12}, lambda rt, c, s, p, st: rt.render_views_device(c, s, others, rd, [5150, -7], p["frames"], stream=st))
    if adapter in ("render_views_device", "render_views_device accumulated"):
        acc = adapter.endswith("accumulated")
        cams = [rt.Camera(w, h), rt.Camera(w, h, pos=(0.3, 0.1, -0.2)), rt.Camera(w, h, pos=(0.2, 0.0, 0.1), rot=(0.05, -0.2, 0.1))]
        if acc:
            return Case(key, "views", {"frame": frame}, {"frame": px * 12},
                        lambda rt, c, s, p, st: rt.render_views_device(c, s, cams, rd, TIMES, p["frame"], accumulate=True, frame_num=2, stream=st))
        return Case(key, "views", {}, {"frames": 3 * px * 12}, lambda rt, c, s, p, st: rt.render_views_device(c, s, cams, rd, TIMES, p["frames"], stream=st))
    if adapter in ("render_budget_device", "render_budget_device tile list"):
        tl = L1 if adapter.endswith("tile list") else None
        budget = rng.choice(np.array([0, 0, 1, 2, 4], np.uint16), size=(h, w))
        count = rng.integers(0, 6, size=(h, w)).astype(np.uint32)
        return Case(key, "budget", {"budget": budget, "frame": frame, "count": count}, {"frame": px * 12, "count": px * 4},
                    lambda rt, c, s, p, st: rt.render_budget_device(c, s, cam, rd, TIMES[2], p["budget"], p["frame"], d_count=p["count"], tile_list=tl, stream=st))
    if adapter == "adaptive_plan_device":
        a = _image(rng, w, h)
        b = (a + (rng.random((h, w, 3), dtype=F) - F(0.5)) * F(0.4)).astype(F)
        count = rng.choice(np.array([2, 5, 9, 10, 11, 12, 400], np.uint32), size=(h, w))
        n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
        return Case(key, "plan", {"a": a, "b": b, "count": count}, {"budget": px * 2, "tile_error": n_tiles * 4, "tile_active": n_tiles * 4},
                    lambda rt, c, s, p, st: rt.adaptive_plan_device(c, w, h, p["a"], p["b"], p["count"], p["budget"], p["tile_error"], p["tile_active"],
                                                                    rt.AdaptiveParams(pilot_spp=2, max_passes=4, **PLAN), stream=st))
    if adapter in ("trace_rays_device", "occluded_rays_device", "occluded_rays_device limits"):
        o, d = _rays(N_RAYS, 5)
        if adapter == "trace_rays_device":
            return Case(key, "query", {"origins": o, "directions": d}, {"hits": N_RAYS * rt.HIT_DTYPE.itemsize},
                        lambda rt, c, s, p, st: rt.trace_rays_device(c, s, p["origins"], p["directions"], N_RAYS, p["hits"], stream=st),
                        host=lambda rt, c, s: rt.trace_rays(c, s, o, d))
        if adapter.endswith("limits"):
            tmax = (rng.random(N_RAYS, dtype=F) * F(4.0)).astype(F)
            return Case(key, "occlusion", {"origins": o, "directions": d, "tmax": tmax}, {"occluded": N_RAYS},
                        lambda rt, c, s, p, st: rt.occluded_rays_device(c, s, p["origins"], p["directions"], p["tmax"], N_RAYS, p["occluded"], stream=st))
        return Case(key, "occlusion", {"origins": o, "directions": d}, {"occluded": N_RAYS},
                    lambda rt, c, s, p, st: rt.occluded_rays_device(c, s, p["origins"], p["directions"], None, N_RAYS, p["occluded"], stream=st))
    if adapter == "render_aov_device":
        return Case(key, "query", {}, {"depth": px * 4, "normal": px * 12, "albedo": px * 12, "object": px * 4, "ray": px * 12},
                    lambda rt, c, s, p, st: rt.render_aov_device(c, s, cam, SKY_AOV, d_depth=p["depth"], d_normal=p["normal"], d_albedo=p["albedo"], d_object=p["object"],
                                                                 d_ray=p["ray"], stream=st))
    if adapter == "render_visibility_device":
        return Case(key, "occlusion", {}, {"visibility": px}, lambda rt, c, s, p, st: rt.render_visibility_device(c, s, cam, LIGHT, BIAS, p["visibility"], stream=st))
    if adapter == "render_ao_device":
        return Case(key, "ao", {}, {"count": px * 2, "ao": px * 4},
                    lambda rt, c, s, p, st: rt.render_ao_device(c, s, cam, d_count=p["count"], d_ao=p["ao"], stream=st, **AO),
                    host=lambda rt, c, s: rt.render_ao(c, s, cam, planes=("ao", "count"), **AO))
    if adapter in ("denoise_device", "denoise_device in place"):
        n = rng.normal(size=(h, w, 3)).astype(F)
        planes = {"colour": frame, "normal": (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F), "depth": (F(1.0) + _image(rng, w, h, 1) * F(2.0)).astype(F),
                  "object": rng.integers(0, 3, size=(h, w)).astype(np.int32), "albedo": (F(0.2) + _image(rng, w, h) * F(0.8)).astype(F)}
        out = "colour" if adapter.endswith("in place") else "out"
        return Case(key, "denoise", planes, {out: px * 12},
                    lambda rt, c, s, p, st: rt.denoise_device(c, w, h, p["colour"], p["normal"], p["depth"], p["object"], p["albedo"], p[out], rt.DenoiseParams(**DENOISE), stream=st),
                    host=lambda rt, c, s: rt.denoise(c, planes["colour"], planes["normal"], planes["depth"], planes["object"], planes["albedo"], rt.DenoiseParams(**DENOISE)))
    if adapter == "to_rgba8_device":
        rgb = (_image(rng, w, h) * F(1.5) - F(0.25)).astype(F)
        return Case(key, "display", {"rgb": rgb}, {"rgba": px * 4}, lambda rt, c, s, p, st: rt.to_rgba8_device(c, p["rgb"], w, h, p["rgba"], stream=st))
    if adapter in ("tiles_copy_device to frame", "tiles_copy_device to compact"):
        compact = rng.random(len(L2) * 192, dtype=F)
        if adapter.endswith("to frame"):
            return Case(key, "tiles", {"compact": compact, "frame": frame}, {"frame": px * 12},
                        lambda rt, c, s, p, st: rt.tiles_copy_device(c, p["compact"], p["frame"], w, h, L2, to_frame=True, stream=st))
        return Case(key, "tiles", {"compact": compact, "frame": frame}, {"compact": compact.nbytes},
                    lambda rt, c, s, p, st: rt.tiles_copy_device(c, p["compact"], p["frame"], w, h, L2, to_frame=False, stream=st))
    raise KeyError(adapter)


SCENE_ADAPTERS = ["render_device", "render_device bands", "render_device tile list", "render_device_batch", "frame_submit / frame_collect", "render_views_device",
                  "render_views_device other cameras",
                  "render_views_device accumulated", "render_budget_device", "render_budget_device tile list", "trace_rays_device", "render_aov_device", "occluded_rays_device",
                  "occluded_rays_device limits", "render_visibility_device", "render_ao_device"]
PLAIN_ADAPTERS = ["adaptive_plan_device", "denoise_device", "denoise_device in place", "to_rgba8_device", "tiles_copy_device to frame", "tiles_copy_device to compact"]
ADAPTERS = [(a, n) for a in SCENE_ADAPTERS for n in SCENES] + [(a, None) for a in PLAIN_ADAPTERS]
ADAPTER_IDS = [("%s-%s" % (a, n)).replace(" / ", "+").replace(" ", "_") for a, n in ADAPTERS]
FAMILIES = {"render", "pipeline", "views", "budget", "plan", "query", "occlusion", "ao", "denoise", "display", "tiles"}


# ---- the rig: contexts, buffers, the calibrated sleep ------------------------------------------------------------------------------
class Rig:
    """what the module shares: the sleep's rate, a warm context per scene (and a second one for case (f)), three streams, the cases with
    their device buffers and their synchronised results"""

    def __init__(self, rt, models_dir):
        import torch
        self.rt, self.models_dir, self.torch = rt, models_dir, torch
        self.dev = torch.device("cuda:0")
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(3)]
        # a stream's first use sets up its hardware queue, and the host waits meanwhile (seen: 20 ms into the first chain): have that behind us
        for s in self.streams:
            with torch.cuda.stream(s):
                torch.zeros(16, device=self.dev).add_(1.0)
            s.synchronize()
        self.contexts, self.cases, self.buffers, self.expected, self.windows, self.opened, self.pending = {}, {}, {}, {}, {}, {}, {}
        self.rate = self.calibrate()

    def calibrate(self):
        """cycles of torch.cuda._sleep per millisecond: a fixed count timed with events (doubled until it takes 2 ms)"""
        torch = self.torch
        torch.cuda._sleep(100000)
        torch.cuda.synchronize()
        cycles = 1000000
        for _ in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0:
                break
            cycles *= 2
        assert ms >= 2.0, ("torch.cuda._sleep does not sleep", cycles, ms)
        rate = cycles / ms
        print("sleep calibration: %d cycles in %.3f ms: %.0f cycles per millisecond" % (cycles, ms, rate))
        return rate

    def sleep(self, ms):
        self.torch.cuda._sleep(int(ms * self.rate))

    def fresh(self, name):
        """(context, committed scene) nobody has used"""
        rt = self.rt
        ctx = rt.Context(0)
        return ctx, ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name or "three_sphere"]()[0], self.models_dir))

    def context(self, name, second=False):
        key = (name or "three_sphere", second)
        if key not in self.contexts:
            self.contexts[key] = self.fresh(name)
        return self.contexts[key]

    def case(self, adapter, name, size=(W, H)):
        key = (adapter, name) + tuple(size)
        if key not in self.cases:
            self.cases[key] = make_case(self.rt, adapter, name, size)
        return self.cases[key]

    def buffers_of(self, case, tag=""):
        """the case's device buffers, as bytes: src (the real inputs), buf (what the call is handed), res (where the outputs are copied to)"""
        torch = self.torch
        key = (case.key, tag)
        if key not in self.buffers:
            src = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).to(self.dev) for k, v in case.inputs.items()}
            sizes = {k: int(v.numel()) for k, v in src.items()}
            sizes.update(case.outputs)
            buf = {k: torch.empty(n, dtype=torch.uint8, device=self.dev) for k, n in sizes.items()}
            res = {k: torch.empty(n, dtype=torch.uint8, device=self.dev) for k, n in case.outputs.items()}
            torch.cuda.synchronize()
            self.buffers[key] = (src, buf, res)
        return self.buffers[key]

    def stage(self, case, B, real):
        """on the current stream: the inputs (real: their content, else garbage), and garbage in the outputs that are not inputs"""
        src, buf, _ = B
        for k in buf:
            if k in src and real:
                buf[k].copy_(src[k], non_blocking=True)
            else:
                buf[k].fill_(IN_GARBAGE if k in src else OUT_GARBAGE)

    def synchronised(self, case, ctx, scene, tag=""):
        """the call with the host waiting before and after; -> (outputs as bytes, host milliseconds of the call)"""
        torch = self.torch
        B = self.buffers_of(case, tag)
        self.stage(case, B, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        case.call(self.rt, ctx, scene, {k: v.data_ptr() for k, v in B[1].items()}, None)
        host_ms = 1e3 * (time.perf_counter() - t0)
        ctx.synchronize()
        torch.cuda.synchronize()
        return {k: B[1][k].cpu().numpy().copy() for k in case.outputs}, host_ms

    def expect(self, case, name):
        """the synchronised result on a fresh context, once per case"""
        if case.key not in self.expected:
            ctx, scene = self.fresh(name)
            self.expected[case.key] = self.synchronised(case, ctx, scene)[0]
            for k, v in self.expected[case.key].items():
                assert (v != OUT_GARBAGE).any(), (case.key, k, "the call wrote nothing")
        return self.expected[case.key]

    def warm(self, case, ctx, scene, tag=""):
        """Three synchronised calls, made every time (another call in between may have changed the context's view): scratch growth, tile-list
        uploads, a view's cost measurement and the schedule built from it are then behind the context (measure; read back and sort; run
        sorted).  -> the window for this case: ten times the warm call's host time, at least MIN_WINDOW_MS"""
        host = [self.synchronised(case, ctx, scene, tag)[1] for _ in range(3)]
        window = max(MIN_WINDOW_MS, 10.0 * host[-1])
        self.windows[case.key] = (host[-1], window)
        return window

    def queue(self, case, ctx, scene, stream, sleep_ms=0.0, tag=""):
        """case (a)'s sequence on `stream`, nothing waited for: [sleep,] the inputs copied into place, garbage into the outputs, the call, an
        event, the outputs copied out.  -> (the event, whether it was still pending when the call had returned, host ms of the call)"""
        torch = self.torch
        B = self.buffers_of(case, tag)
        with torch.cuda.stream(stream):
            if sleep_ms:
                self.sleep(sleep_ms)
            self.stage(case, B, True)
            t0 = time.perf_counter()
            case.call(self.rt, ctx, scene, {k: v.data_ptr() for k, v in B[1].items()}, stream.cuda_stream)
            host_ms = 1e3 * (time.perf_counter() - t0)
            ev = torch.cuda.Event()
            ev.record(stream)
            pending = not ev.query()
            for k, r in B[2].items():
                r.copy_(B[1][k], non_blocking=True)
        return ev, pending, host_ms

    def spoil(self, *cases_and_tags):
        """garbage where the real inputs will go, and the host waits: the state every case starts from"""
        for case, tag in cases_and_tags:
            self.stage(case, self.buffers_of(case, tag), False)
            for r in self.buffers_of(case, tag)[2].values():
                r.fill_(OUT_GARBAGE)
        self.torch.cuda.synchronize()

    def results(self, case, tag=""):
        return {k: v.cpu().numpy() for k, v in self.buffers_of(case, tag)[2].items()}

    def check(self, case, name, tag="", what=""):
        want = self.expect(case, name)
        for k, got in self.results(case, tag).items():
            assert got.tobytes() == want[k].tobytes(), (what, case.key, k, "%d of %d bytes differ from the synchronised result" % (int((got != want[k]).sum()), got.size))


@pytest.fixture(scope="module")
def rig(rt, models_dir):
    r = Rig(rt, models_dir)
    yield r
    r.torch.cuda.synchronize()
    if r.opened:
        print("sleep rate %.0f cycles per millisecond; windows (ms) per adapter:" % r.rate)
        for key, (window, host_ms) in sorted(r.opened.items(), key=str):
            print("  %-55s window %6.1f ms  (the call took %.3f ms on the host with the window open)" % (" ".join(str(k) for k in key), window, host_ms))


# ---- the synchronised results are the oracle's --------------------------------------------------------------------------------------
def _f(a, shape):
    return np.frombuffer(a.tobytes(), F).reshape(shape)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_synchronised_results_equal_the_yardsticks(rig, rt, orc, models_dir, family):
    """what every other test here compares with, tied to the oracle (or the family's yardstick) once per family, on the scene with a mesh
    where the yardstick is quick enough and on the three spheres otherwise"""
    name = "monkey" if family in ("render", "pipeline", "views", "budget") else "three_sphere"
    objs, sky = rt.scenes.CONFIG_SCENES[name]()
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    cam = rt.Camera(W, H).floats()
    if family == "render":
        case = rig.case("render_device", name)
        want = oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=TIMES[0], frame_num=1, prev=case.inputs["prev"])
        assert np.array_equal(u32(_f(rig.expect(case, name)["out"], (H, W, 3))), u32(want))
        case = rig.case("render_device_batch", name)
        want = case.inputs["frame"]
        for i, t in enumerate(TIMES):
            want = oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=t, frame_num=1 + i, prev=want)
        assert np.array_equal(u32(_f(rig.expect(case, name)["frame"], (H, W, 3))), u32(want))
    elif family == "pipeline":
        case = rig.case("frame_submit / frame_collect", name)
        want = case.inputs["frame"]
        for i, t in enumerate(TIMES[:2]):
            want = oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=t, frame_num=1 + i, prev=want)
        assert np.array_equal(u32(_f(rig.expect(case, name)["frame"], (H, W, 3))), u32(want))
    elif family == "views":
        cams = [rt.Camera(W, H).floats(), rt.Camera(W, H, pos=(0.3, 0.1, -0.2)).floats(), rt.Camera(W, H, pos=(0.2, 0.0, 0.1), rot=(0.05, -0.2, 0.1)).floats()]
        want = views_ref.separate(oracle, cams, W, H, SPP, LIMIT, sky, TIMES)
        assert np.array_equal(u32(_f(rig.expect(rig.case("render_views_device", name), name)["frames"], (3, H, W, 3))), u32(want))
        case = rig.case("render_views_device accumulated", name)
        want = views_ref.accumulated(oracle, cams, W, H, SPP, LIMIT, sky, TIMES, 2, case.inputs["frame"])
        assert np.array_equal(u32(_f(rig.expect(case, name)["frame"], (H, W, 3))), u32(want))
    elif family == "budget":
        for adapter, tl in (("render_budget_device", None), ("render_budget_device tile list", tile_list(W, H, 0))):
            case = rig.case(adapter, name)
            frame, count = adaptive_ref.budget_render(oracle, cam, W, H, case.inputs["budget"], LIMIT, sky, TIMES[2], case.inputs["frame"], case.inputs["count"], True, tl)
            got = rig.expect(case, name)
            assert np.array_equal(u32(_f(got["frame"], (H, W, 3))), u32(frame)) and got["count"].tobytes() == count.tobytes(), adapter
    elif family == "plan":
        case = rig.case("adaptive_plan_device", None)
        budget, err, active, _ = adaptive_ref.plan(case.inputs["a"], case.inputs["b"], case.inputs["count"], pixel_threshold=np.inf, **PLAN)
        got = rig.expect(case, None)
        assert got["budget"].tobytes() == budget.tobytes() and got["tile_error"].tobytes() == err.astype(F).tobytes() and got["tile_active"].tobytes() == active.tobytes()
        assert 0 < np.count_nonzero(active) < len(active) and (budget == 0).any() and (budget > 0).any()
    elif family == "query":
        case = rig.case("trace_rays_device", name)
        o, d = case.inputs["origins"], case.inputs["directions"]
        ohit, oout = oracle_records(oracle, o, d)
        assert 0.25 <= ohit.mean() <= 0.90
        assert_equal_to_oracle(np.frombuffer(rig.expect(case, name)["hits"].tobytes(), rt.HIT_DTYPE), ohit, oout, "trace_rays_device")
        got = rig.expect(rig.case("render_aov_device", name), name)
        pd = primaries(cam, W, H).reshape(-1, 3)
        phit, pout = oracle_records(oracle, np.broadcast_to(np.asarray(cam[0:3], F), pd.shape), pd)
        obj = np.frombuffer(got["object"].tobytes(), np.int32)
        assert np.array_equal(u32(_f(got["ray"], (H * W, 3))), u32(pd)) and np.array_equal(obj >= 0, phit) and np.array_equal(obj[phit], pout[phit, 7].astype(np.int32))
        assert np.array_equal(u32(_f(got["depth"], (H * W,))[phit]), u32(pout[phit, 0])) and np.array_equal(u32(_f(got["normal"], (H * W, 3))[phit]), u32(pout[phit, 4:7]))
    elif family == "occlusion":
        case = rig.case("occluded_rays_device limits", name)
        hit, t, _ = oracle_hits(oracle, case.inputs["origins"], case.inputs["directions"])
        assert 0.10 <= hit.mean() <= 0.90
        assert rig.expect(case, name)["occluded"].tobytes() == occlusion_expected(hit, t, case.inputs["tmax"]).tobytes()
        assert rig.expect(rig.case("occluded_rays_device", name), name)["occluded"].tobytes() == hit.astype(np.uint8).tobytes()
        assert rig.expect(rig.case("render_visibility_device", name), name)["visibility"].tobytes() == oracle_visibility(oracle, cam, W, H, LIGHT, BIAS).tobytes()
    elif family == "ao":
        import ao_ref
        ref = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, AO["samples"], AO["radius"], AO["bias"], AO["time_ms"])
        got = rig.expect(rig.case("render_ao_device", name), name)
        assert got["count"].tobytes() == ref["count"].tobytes() and np.array_equal(u32(_f(got["ao"], (H, W))), u32(ref["ao"]))
    elif family == "denoise":
        for adapter, out in (("denoise_device", "out"), ("denoise_device in place", "colour")):
            case = rig.case(adapter, None)
            p = case.inputs
            want = denoise_ref(p["colour"], p["normal"], p["depth"], p["object"], p["albedo"], **rt.DenoiseParams(**DENOISE).as_dict())
            assert np.array_equal(u32(_f(rig.expect(case, None)[out], (H, W, 3))), u32(want)), adapter
            # (from the yardstick alone, the bound test_gpu_denoise.py uses: an entry point that copied its input could not pass)
            assert (u32(want) != u32(p["colour"])).any(axis=2).mean() >= 0.10
    elif family == "display":
        import ctypes as C
        case = rig.case("to_rgba8_device", None)
        want = np.zeros((H, W, 4), np.uint8)
        orc.lib().orc_to_rgba8(np.ascontiguousarray(case.inputs["rgb"]).ctypes.data_as(C.POINTER(C.c_float)), W, H, want.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rig.expect(case, None)["rgba"].tobytes() == want.tobytes()
    else:
        # tiles: slot k of the compact image is tile L2[k], 64 pixels row by row; slots outside the image are never touched
        tiles_x, ids = (W + 7) // 8, tile_list(W, H, 3)
        for adapter in ("tiles_copy_device to frame", "tiles_copy_device to compact"):
            case = rig.case(adapter, None)
            frame, compact = case.inputs["frame"].copy(), case.inputs["compact"].reshape(len(ids), 8, 8, 3).copy()
            for k, t in enumerate(ids):
                y0, x0 = 8 * (t // tiles_x), 8 * (t % tiles_x)
                hh, ww = min(8, H - y0), min(8, W - x0)
                if adapter.endswith("to frame"):
                    frame[y0:y0 + hh, x0:x0 + ww] = compact[k, :hh, :ww]
                else:
                    compact[k, :hh, :ww] = frame[y0:y0 + hh, x0:x0 + ww]
            got = rig.expect(case, None)
            assert (got["frame"].tobytes() == frame.tobytes()) if adapter.endswith("to frame") else (got["compact"].tobytes() == compact.tobytes()), adapter


# ---- (a) inputs in stream order, (b) the window really was open -----------------------------------------------------------------------
def run_behind_a_sleep(rig, adapter, name):
    """once per adapter and scene: -> whether the event behind the call was pending when the call returned"""
    key = (adapter, name)
    if key not in rig.opened:
        case = rig.case(adapter, name)
        ctx, scene = rig.context(name)
        rig.expect(case, name)
        window = rig.warm(case, ctx, scene)
        rig.spoil((case, ""))
        ev, pending, host_ms = rig.queue(case, ctx, scene, rig.streams[0], window)
        ev.synchronize()
        rig.streams[0].synchronize()
        rig.opened[key] = (window, host_ms)
        rig.pending[key] = pending
    return rig.pending[key]


@pytest.mark.parametrize("adapter,name", ADAPTERS, ids=ADAPTER_IDS)
def test_inputs_produced_on_the_stream_just_ahead_of_the_call(rig, adapter, name):
    """(a) sleep, copies of the real inputs over garbage, garbage into the outputs, the call, a copy of the outputs: one stream, no host wait"""
    run_behind_a_sleep(rig, adapter, name)
    rig.check(rig.case(adapter, name), name, what="(a)")


@pytest.mark.parametrize("adapter,name", ADAPTERS, ids=ADAPTER_IDS)
def test_the_window_was_open(rig, adapter, name):
    """(b) warm, no entry point waits on the host: the event recorded behind the call had not completed when the call returned.  Nothing is
    waived here (WAITS_ON_HOST lists the waits of cold and of cross-stream situations)."""
    assert run_behind_a_sleep(rig, adapter, name), (adapter, name, "the call returned only after the stream's sleep had ended: it waited on the host", rig.opened[(adapter, name)])


def test_every_family_has_an_open_window_case(rig):
    """from the runs themselves: the families of the cases whose window was open cover every family"""
    assert {rig.case(a, n).family for a, n in ADAPTERS if run_behind_a_sleep(rig, a, n)} == FAMILIES


# ---- (c) another stream, same context; (f) two contexts ---------------------------------------------------------------------------------
# tiles_copy_device and to_rgba8_device use none of the context's launch scratch and their header comments promise "asynchronously on
# hip_stream", not the launch order: they are ordered by their stream alone (and, for the tile list, by the cache's own events)
NOT_IN_THE_LAUNCH_ORDER = ("tiles_copy_device to frame", "tiles_copy_device to compact", "to_rgba8_device")
A, B = 0, 1
# (what it is about, the calls in order as (adapter, size, stream), which entry of WAITS_ON_HOST excuses a first call that is no longer pending, if any)
CHAINS = [
    ("ticket counter", [("render_device", None, A), ("trace_rays_device", None, B)], None),
    ("per-frame planes", [("render_views_device accumulated", None, A), ("render_device_batch", None, B), ("render_views_device accumulated", None, A)], None),
    ("camera table and its upload", [("render_views_device", None, A), ("render_views_device other cameras", None, B), ("render_views_device accumulated", None, A)], "views -> views"),
    ("denoise records", [("denoise_device", None, A), ("denoise_device", SMALL, B)], None),
    ("tile-list cache", [("render_budget_device tile list", None, A), ("tiles_copy_device to frame", None, B), ("render_device tile list", None, B)], None),
    ("ambient occlusion, then occlusion", [("render_ao_device", None, A), ("occluded_rays_device limits", None, B)], None),
    ("plan, then budget render", [("adaptive_plan_device", None, A), ("render_budget_device", None, B)], None),
]


def run_chain(rig, name, chain, two_contexts):
    """the calls on their streams (those on stream B on a second context with two_contexts), the first behind a sleep, nothing waited for;
    -> per call [case, tag, context, scene, window, stream, the first call was still pending once this one was queued], and the events"""
    calls = []
    for i, (adapter, size, stream) in enumerate(chain):
        case = rig.case(adapter, name if adapter in SCENE_ADAPTERS else None, size or (W, H))
        ctx, scene = rig.context(name, second=two_contexts and stream == B)
        tag = "chain%d" % i
        rig.expect(case, name)
        calls.append([case, tag, ctx, scene, rig.warm(case, ctx, scene, tag), stream])
    rig.spoil(*[(c[0], c[1]) for c in calls])
    events = []
    for i, (case, tag, ctx, scene, window, stream) in enumerate(calls):
        ev, _, _ = rig.queue(case, ctx, scene, rig.streams[stream], max(c[4] for c in calls) if i == 0 else 0.0, tag)
        events.append(ev)
        calls[i].append(not events[0].query())
    return calls, events


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("what,chain,waits", CHAINS, ids=[c[0].replace(" ", "_").replace(",", "") for c in CHAINS])
def test_two_streams_of_one_context_are_ordered(rig, name, what, chain, waits):
    """(c) X on stream A behind a sleep, Y at once on stream B[, Z]: once a later call's event has completed, the event of every earlier
    call in the launch order has, and every result is right"""
    calls, events = run_chain(rig, name, chain, False)
    for j in range(1, len(events)):
        if calls[j][0].key[0] in NOT_IN_THE_LAUNCH_ORDER:
            continue
        events[j].synchronize()
        for i in range(j):
            if calls[i][0].key[0] not in NOT_IN_THE_LAUNCH_ORDER or calls[i][5] == calls[j][5]:
                assert events[i].query(), (what, "call %d (%s) finished before call %d (%s) of the same context" % (j, calls[j][0].key[0], i, calls[i][0].key[0]))
    rig.torch.cuda.synchronize()
    for case, tag, *_ in calls:
        rig.check(case, name, tag, what)
    if waits is None:
        assert all(c[6] for c in calls), (what, "the first call had finished before the others were queued: some call waited on the host", [c[6] for c in calls])
    else:
        print("%s: first call still pending after each call was queued: %s (%s)" % (what, [c[6] for c in calls], WAITS_ON_HOST[waits]))


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("what,chain,waits", CHAINS, ids=[c[0].replace(" ", "_").replace(",", "") for c in CHAINS])
def test_two_contexts_on_two_streams(rig, name, what, chain, waits):
    """(f) the same chains with the calls of stream B on another context: they may overlap, and every result is right"""
    calls, _ = run_chain(rig, name, chain, True)
    rig.torch.cuda.synchronize()
    for case, tag, *_ in calls:
        rig.check(case, name, tag, what)


@pytest.mark.parametrize("adapter", ["trace_rays_device", "render_ao_device", "denoise_device"])
def test_a_device_form_then_the_host_form(rig, rt, adapter):
    """(c) a device form pending on a side stream, then the same family's host form (the null stream, blocking copies): both are right, and
    the host form returns after the device form has finished (WAITS_ON_HOST["host form"])"""
    name = "monkey"
    case = rig.case(adapter, name if adapter in SCENE_ADAPTERS else None)
    ctx, scene = rig.context(name)
    fresh_ctx, fresh_scene = rig.fresh(name)
    want = case.host(rt, fresh_ctx, fresh_scene)
    rig.expect(case, name)
    window = rig.warm(case, ctx, scene)
    case.host(rt, ctx, scene)                              # (warm: the host form's own buffers)
    rig.spoil((case, ""))
    ev, pending, _ = rig.queue(case, ctx, scene, rig.streams[0], window)
    got = case.host(rt, ctx, scene)
    assert ev.query(), "the host form returned before the context's pending launch had finished"
    assert pending
    rig.torch.cuda.synchronize()
    rig.check(case, name, what="device form")
    for k in (want if isinstance(want, dict) else {"": want}):
        a, b = (got[k], want[k]) if isinstance(want, dict) else (got, want)
        assert a.tobytes() == b.tobytes(), (adapter, k, "host form")


# ---- (d) behind frames in flight -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("adapter", ["trace_rays_device", "occluded_rays_device limits", "render_ao_device", "denoise_device", "render_budget_device tile list", "render_views_device accumulated",
                                     "render_views_device"])
def test_behind_frames_in_flight(rig, rt, name, adapter):
    """two frames submitted and not collected - held back by a sleeping launch of the same context - then one call on a third stream, then
    the frames are collected: the frames equal frame-by-frame rendering and the call its synchronised result"""
    torch = rig.torch
    case = rig.case(adapter, name if adapter in SCENE_ADAPTERS else None)
    holder = rig.case("adaptive_plan_device", None)
    ctx, scene = rig.context(name)
    sky = rt.scenes.CONFIG_SCENES[name]()[1]
    cam, rd = rt.Camera(W, H), rt.RenderData(SPP, LIMIT, True, sky)
    rig.expect(case, name)
    window = max(rig.warm(case, ctx, scene, "d"), rig.warm(holder, ctx, scene, "d"))
    want = frame_by_frame(rt, ctx, scene, cam, rd, TIMES[:2], W, H, None)
    rt.frame_depth(ctx, 2)
    for _ in range(2):                                     # (warm: the view's first frames measure and sort)
        rt.frame_submit(ctx, scene, cam, rd, TIMES[0]); rt.frame_submit(ctx, scene, cam, rd, TIMES[1])
        rt.frame_collect(ctx, 0, None); rt.frame_collect(ctx, 0, None)
    ctx.synchronize()
    frame = torch.full((H, W, 3), 7.0, device=rig.dev)
    rig.spoil((case, "d"), (holder, "d"))
    rig.queue(holder, ctx, scene, rig.streams[0], window, "d")     # the context's last launch sleeps: the frames queue up behind it
    rt.frame_submit(ctx, scene, cam, rd, TIMES[0])
    rt.frame_submit(ctx, scene, cam, rd, TIMES[1])
    assert rt.frames_pending(ctx) == 2
    ev, pending, _ = rig.queue(case, ctx, scene, rig.streams[2], 0.0, "d")
    assert pending, "the call on the third stream had finished although the frames ahead of it cannot have started"
    rt.frame_collect(ctx, 0, frame.data_ptr(), stream=rig.streams[1].cuda_stream)
    rt.frame_collect(ctx, 1, frame.data_ptr(), stream=rig.streams[1].cuda_stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(u32(frame.cpu().numpy()), u32(want)), "the collected frames differ from frame-by-frame rendering"
    rig.check(case, name, "d", "(d)")


# ---- (e) regrow under pending work -----------------------------------------------------------------------------------------------------
# (the small call, the large call, the scenes, the scratch that grows)
REGROW = [
    ("denoise_device", "denoise_device", SCENES, "d_denoise: three records per pixel"),
    ("render_device_batch", "render_device_batch", SCENES, "d_partial: one plane per frame"),
    ("render_views_device accumulated", "render_views_device accumulated", SCENES, "d_partial: one plane per view"),
    # (separate frames go straight to the caller's buffer: only the schedule behind the camera table grows, and only a mesh has one)
    ("render_views_device other cameras", "render_views_device", ["monkey"], "ViewsState::d_table: 6 tiles x 2 views of schedule, then 60 x 3"),
]
REGROW_CASES = [(s, l, n, g) for s, l, names, g in REGROW for n in names]


@pytest.mark.parametrize("small_adapter,large_adapter,name,grows", REGROW_CASES, ids=["%s-%s" % (l.replace(" ", "_"), n) for _, l, n, _ in REGROW_CASES])
def test_regrow_under_pending_work(rig, small_adapter, large_adapter, name, grows):
    """a small call pending behind a sleep on stream A, then a larger one of the same family on stream B of a context that has only seen
    the small size: DevBuf::grow frees scratch the pending call uses - hipFree waits for the device (WAITS_ON_HOST["regrow"]) - and both
    results are right"""
    scene_name = name if large_adapter in SCENE_ADAPTERS else None
    small, large = rig.case(small_adapter, scene_name, SMALL), rig.case(large_adapter, scene_name)
    ctx, scene = rig.fresh(name)
    rig.expect(small, name)
    rig.expect(large, name)
    window = rig.warm(small, ctx, scene, "e")
    rig.spoil((small, "e"), (large, "e"))
    ev_small, _, _ = rig.queue(small, ctx, scene, rig.streams[0], window, "e")
    ev_large, _, host_ms = rig.queue(large, ctx, scene, rig.streams[1], 0.0, "e")
    ev_large.synchronize()
    assert ev_small.query(), "the larger call finished before the pending smaller one of the same context"
    rig.torch.cuda.synchronize()
    print("%s %s (%s): the larger call took %.1f ms on the host behind a window of %.1f ms" % (large_adapter, name, grows, host_ms, window))
    rig.check(small, name, "e", "(e) small")
    rig.check(large, name, "e", "(e) large")


# ---- the tile-list cache recycles an entry a pending launch reads -------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_a_tile_list_recycled_under_pending_work(rig, rt, name):
    """The context's cache holds 64 lists: 63 others and L1, the most recently used.  A budget render with L1 is pending behind a sleep on
    stream A; 64 lists the cache has not seen then go through it on stream B, each taking over the least recently used entry, the 64th
    L1's: its upload has to wait for the pending launch (the entry's event, fill_dev_list), or that launch would render the wrong tiles.
    The order is asserted by events, then both results.  (Entries are reused at their size: nothing is allocated inside the window.)"""
    torch = rig.torch
    case, copy = rig.case("render_budget_device tile list", name), rig.case("tiles_copy_device to frame", None)
    ctx, scene = rig.fresh(name)
    rig.expect(case, name)
    B_copy = rig.buffers_of(copy, "lru")
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
    distinct = [[k] for k in range(n_tiles)] + [[k, k + 1] for k in range(n_tiles - 1)] + [[k, k + 2] for k in range(n_tiles - 2)]
    first, lists = distinct[:63], distinct[63:127]
    assert len(lists) == 64 and tile_list(W, H, 0) not in distinct
    for ids in first:
        rt.tiles_copy_device(ctx, B_copy[1]["compact"].data_ptr(), B_copy[1]["frame"].data_ptr(), W, H, ids, to_frame=True)
    torch.cuda.synchronize()
    window = rig.warm(case, ctx, scene, "lru")
    rig.spoil((case, "lru"), (copy, "lru"))
    ev_a, pending, _ = rig.queue(case, ctx, scene, rig.streams[0], 2.0 * window, "lru")
    with torch.cuda.stream(rig.streams[1]):
        rig.stage(copy, B_copy, True)
        for ids in lists:
            rt.tiles_copy_device(ctx, B_copy[1]["compact"].data_ptr(), B_copy[1]["frame"].data_ptr(), W, H, ids, to_frame=True, stream=rig.streams[1].cuda_stream)
        ev_b = torch.cuda.Event()
        ev_b.record(rig.streams[1])
        still_pending = not ev_a.query()
        B_copy[2]["frame"].copy_(B_copy[1]["frame"], non_blocking=True)
    ev_b.synchronize()
    assert ev_a.query(), "the upload into the recycled entry finished before the pending launch that reads the entry"
    torch.cuda.synchronize()
    assert pending and still_pending, "the window closed before the 64 lists were queued: a call waited on the host"
    rig.check(case, name, "lru", "the pending launch")
    # the copies: tile k of the compact image into tile ids[k] of the frame, in order
    frame, compact = copy.inputs["frame"].copy(), copy.inputs["compact"].reshape(-1, 8, 8, 3)
    for ids in lists:
        for k, t in enumerate(ids):
            y0, x0 = 8 * (t // ((W + 7) // 8)), 8 * (t % ((W + 7) // 8))
            hh, ww = min(8, H - y0), min(8, W - x0)
            frame[y0:y0 + hh, x0:x0 + ww] = compact[k, :hh, :ww]
    assert rig.results(copy, "lru")["frame"].tobytes() == frame.tobytes()
