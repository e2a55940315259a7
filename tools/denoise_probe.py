"""Measurements of the denoiser on the GPU (one JSON line per image size):

  total     rt_denoise_device on a low-sample frame of the metric scene (monkey) and its first-hit planes, iterations = 1 .. 5, with and
            without the albedo plane: kernel ms from rt_last_kernel_ms (HIP events around the passes), after a warm-up, median and
            spread (max - min) of `--repeats` runs
  levels    the time of level k (k = 1 .. 4, step 2^k) as the difference of the medians for iterations = k + 1 and k; iterations = 1
            is the pack pass plus level 0
  copy      next to it, in the same run: a device-to-device copy that moves a level's compulsory bytes - the two 16-byte records of
            every pixel read once and one written once are 48 bytes of traffic per pixel, as a copy of 24 bytes per pixel is - timed with
            events on the same stream, one copy per event pair (so its spread is mostly launch jitter; read the median); level /
            copy says how far a pass is from the floor of the memory system (at 1920 x 1080 the records fit the 256 MiB Infinity
            Cache, so that floor is a cache-to-cache copy, not an HBM one)

    python tools/denoise_probe.py [--sizes 1920x1080,3840x2160] [--repeats 15] [--spp 4]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med_spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "spread_ms": round(max(xs) - min(xs), 4)}


def probe(rt, ctx, torch, W, H, repeats, spp):
    dev = torch.device("cuda:0")
    objs, sky = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, rt.scenes.models_dir()))
    cam, rs = rt.Camera(W, H), rt.RenderData(spp, 8, True, sky)
    frame = torch.zeros((H, W, 3), device=dev)
    out = torch.empty_like(frame)
    normal, albedo = torch.empty_like(frame), torch.empty_like(frame)
    depth = torch.empty((H, W), device=dev)
    obj = torch.empty((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    res = {"width": W, "height": H, "spp": spp, "repeats": repeats}
    frame_ms, aov_ms = [], []
    for k in range(3 + repeats):
        rt.render_device(ctx, scene, cam, rs, 100 + k, 0, frame.data_ptr())
        frame_ms.append(ctx.last_kernel_ms())
        rt.render_aov_device(ctx, scene, cam, sky, d_depth=depth.data_ptr(), d_normal=normal.data_ptr(), d_albedo=albedo.data_ptr(), d_object=obj.data_ptr())
        aov_ms.append(ctx.last_kernel_ms())
    res["frame"] = med_spread(frame_ms[3:])
    res["aov"] = med_spread(aov_ms[3:])

    def run(iterations, with_albedo):
        p = rt.DenoiseParams(iterations=iterations)
        rt.denoise_device(ctx, W, H, frame.data_ptr(), normal.data_ptr(), depth.data_ptr(), obj.data_ptr(), albedo.data_ptr() if with_albedo else None,
                          out.data_ptr(), p)
        return ctx.last_kernel_ms()

    src = torch.empty(W * H * 24, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy():
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for with_albedo in (True, False):
        totals = {}
        copies = []
        for it in range(1, 6):
            for _ in range(3):
                run(it, with_albedo)
                copy()
            xs = []
            for _ in range(repeats):
                xs.append(run(it, with_albedo))
                copies.append(copy())
            totals[it] = med_spread(xs)
        c = med_spread(copies)
        levels = [round(totals[it + 1]["median_ms"] - totals[it]["median_ms"], 4) for it in range(1, 5)]
        res["albedo" if with_albedo else "no_albedo"] = {
            "total_by_iterations": totals, "copy_24B_per_pixel": c, "levels_1_to_4_ms": levels,
            "level_over_copy": [round(x / c["median_ms"], 2) for x in levels],
            "pack_plus_level_0_ms": totals[1]["median_ms"], "total_5_over_aov": round(totals[5]["median_ms"] / res["aov"]["median_ms"], 2),
            "total_5_over_frame": round(totals[5]["median_ms"] / res["frame"]["median_ms"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--spp", type=int, default=4)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    ctx = rt.Context(0)
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        print(json.dumps(probe(rt, ctx, torch, W, H, a.repeats, a.spp)), flush=True)


if __name__ == "__main__":
    main()
