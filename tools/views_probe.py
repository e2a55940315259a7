"""Measurements of the camera sequences on the GPU (one JSON line), the sibling of tools/adaptive_probe.py.  Every figure is the median of
--runs runs after a warm-up round, with the spread (max - min) beside it; the legs of a section alternate run by run.  Times are wall
milliseconds (time.perf_counter) around work that starts on an idle device and ends with a device synchronisation: the pipelined leg runs on
streams of the context's own, which an event on the caller's stream would not bracket.

  A  the reference's own workload: scene 0 (the monkey in the Cornell box), 1000 x 800, 100 samples x 5 bounces, a 32-camera orbit
  B  the metric scene: monkey, 1920 x 1080, 64 samples x 8 bounces, 16 cameras
     legs:  views      one render_views_device launch of all cameras (separate frames)
            singles    one render_device call per camera: what a caller whose camera moves had before
            pipelined  frame_submit / frame_collect at depth 4 with the camera changing every frame
     the three legs' frames are compared once, bit for bit
  C  the price of the variant: 20 identical cameras accumulated by render_views_device against render_device_batch of the same 20 frames
     (monkey, 1920 x 1080, 1024 samples x 8 bounces): a guessed schedule and a per-lane camera against a measured schedule

    python tools/views_probe.py [--runs 5] [--legs A,B,C]
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(x):
    return {"median": statistics.median(x), "spread": max(x) - min(x), "runs": [round(v, 3) for v in x]}


def orbit(rt, w, h, n, centre_z=1.6, radius=1.6, span=0.8):
    """n cameras on an arc about the point (0, 0, centre_z), each turned to face it"""
    cams = []
    for i in range(n):
        a = (i / max(n - 1, 1) - 0.5) * span
        cams.append(rt.Camera(w, h, pos=(radius * math.sin(a), 0.0, centre_z - radius * math.cos(a)), rot=(0.0, a, 0.0)))
    return cams


class Bench:
    def __init__(self, runs):
        import torch
        self.torch = torch
        self.rt = importlib.import_module("ray-tracer_amd")
        self.ctx = self.rt.Context(0)
        self.runs = runs

    def scene(self, name):
        objs, sky = self.rt.scenes.CONFIG_SCENES[name]()
        return self.ctx.commit(self.rt.SceneObjects(objs, self.rt.scenes.models_dir())), sky

    def timed(self, fn):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        self.ctx.synchronize()
        self.torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(self, legs):
        """{name: fn} -> {name: med(ms)}: one warm-up round, then --runs rounds, the legs in turn"""
        for fn in legs.values():
            self.timed(fn)
        ms = {k: [] for k in legs}
        for _ in range(self.runs):
            for k, fn in legs.items():
                ms[k].append(self.timed(fn))
        return {k: med(v) for k, v in ms.items()}

    def moving_camera(self, name, w, h, spp, limit, n):
        rt, ctx, torch = self.rt, self.ctx, self.torch
        scene, sky = self.scene(name)
        rd = rt.RenderData(spp, limit, True, sky)
        cams, times = orbit(rt, w, h, n), [1000 + 7 * i for i in range(n)]
        out = {k: torch.zeros((n, h, w, 3), dtype=torch.float32, device="cuda:0") for k in ("views", "singles", "pipelined")}
        plane = h * w * 3 * 4

        def views():
            rt.render_views_device(ctx, scene, cams, rd, times, out["views"].data_ptr())

        def singles():
            for i in range(n):
                rt.render_device(ctx, scene, cams[i], rd, times[i], 0, out["singles"].data_ptr() + i * plane)

        def pipelined():
            sent = got = 0
            while got < n:
                while sent < n and rt.frames_pending(ctx) < 4:
                    rt.frame_submit(ctx, scene, cams[sent], rd, times[sent])
                    sent += 1
                rt.frame_collect(ctx, 0, out["pipelined"].data_ptr() + got * plane)
                got += 1
            rt.frame_wait(ctx)

        rt.frame_depth(ctx, 4)
        res = self.alternate({"views": views, "singles": singles, "pipelined": pipelined})
        same = bool(torch.equal(out["views"].view(torch.int32), out["singles"].view(torch.int32)) and
                    torch.equal(out["views"].view(torch.int32), out["pipelined"].view(torch.int32)))
        samples = n * w * h * spp
        for k in res:
            res[k]["frames_per_s"] = n / (res[k]["median"] * 1e-3)
            res[k]["msamples_per_s"] = samples / (res[k]["median"] * 1e-3) / 1e6
        res["frames_bit_identical"] = same
        res["views_minus_singles_ms"] = res["views"]["median"] - res["singles"]["median"]
        res["gate_views_not_slower_than_singles_by_more_than_its_spread"] = res["views_minus_singles_ms"] <= res["singles"]["spread"]
        res["what"] = "%s %dx%d %d spp x %d bounces, %d cameras" % (name, w, h, spp, limit, n)
        res["scene"] = scene.info()
        return res

    def variant_price(self):
        rt, ctx, torch = self.rt, self.ctx, self.torch
        w, h, spp, limit, n = 1920, 1080, 1024, 8, 20
        scene, sky = self.scene("monkey")
        rd = rt.RenderData(spp, limit, True, sky)
        cam, times = rt.Camera(w, h), [1000 + 7 * i for i in range(n)]
        a = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        b = torch.zeros_like(a)
        kernel_ms = {"views": [], "batch": []}

        def views():
            rt.render_views_device(ctx, scene, [cam] * n, rd, times, a.data_ptr(), accumulate=True)
            kernel_ms["views"].append(ctx.last_kernel_ms())

        def batch():
            rt.render_device_batch(ctx, scene, cam, rd, times, 0, b.data_ptr())
            kernel_ms["batch"].append(ctx.last_kernel_ms())

        res = self.alternate({"views": views, "batch": batch})
        for k in res:
            res[k]["kernel_ms"] = med(kernel_ms[k][1:])
            res[k]["msamples_per_s"] = n * w * h * spp / (res[k]["median"] * 1e-3) / 1e6
        res["frames_bit_identical"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        res["views_over_batch"] = res["views"]["median"] / res["batch"]["median"]
        res["what"] = "monkey %dx%d %d spp x %d bounces, %d identical cameras accumulated" % (w, h, spp, limit, n)
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--legs", default="A,B,C")
    args = ap.parse_args()
    b = Bench(args.runs)
    out = {"runs": args.runs}
    legs = args.legs.split(",")
    if "A" in legs:
        out["A"] = b.moving_camera("reference_scene0", 1000, 800, 100, 5, 32)
    if "B" in legs:
        out["B"] = b.moving_camera("monkey", 1920, 1080, 64, 8, 16)
    if "C" in legs:
        out["C"] = b.variant_price()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
