"""Measurements of the ray queries and the AOV pass on the GPU (one JSON line):

  aov        the AOV pass of the metric scene (monkey, 1920x1080, all planes) against its yardstick, rt_render_device of the same scene
             and camera at 1 spp, reflection limit 1, antialias off (the identical primary rays, shaded as well): the two alternate,
             `--pairs` pairs after a warm-up; kernel ms from rt_last_kernel_ms, medians, and the yardstick's own spread; a third leg
             writes the depth and object planes only (8 instead of 44 bytes per pixel)
  incoherent 2^22 seeded random rays on monkey, soup6k and sphere50k through trace_rays_device: kernel ms, Mrays/s
  small      1 / 64 / 4,096 / 65,536 rays on monkey through trace_rays_device: ms per call end to end (launch + wait on the host clock)

    python tools/query_probe.py [--pairs 12] [--rays 4194304]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = (rng.normal(size=(n, 3)) * 0.8 + np.array((0.0, 0.0, 2.0))).astype(np.float32)
    o[: n // 2] = 0
    t = (rng.normal(size=(n, 3)) * 1.2 + np.array((0.0, 0.0, 2.0))).astype(np.float32)
    d = t - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--rays", type=int, default=1 << 22)
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    dev = torch.device("cuda:0")
    ctx = rt.Context(0)
    models = rt.scenes.models_dir()
    out = {"tool": "query_probe", "version": rt.lib().rt_version().decode()}

    # ---- AOV pass against the one-bounce render of the same primary rays
    objs, _ = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, models))
    W, H = 1920, 1080
    cam = rt.Camera(W, H)
    planes = {"d_depth": torch.empty((H, W), device=dev), "d_normal": torch.empty((H, W, 3), device=dev), "d_albedo": torch.empty((H, W, 3), device=dev),
              "d_object": torch.empty((H, W), dtype=torch.int32, device=dev), "d_ray": torch.empty((H, W, 3), device=dev)}
    frame = torch.empty((H, W, 3), device=dev)
    rd = rt.RenderData(1, 1, False, (1.0, 1.0, 1.0))

    def aov():
        rt.render_aov_device(ctx, scene, cam, (1.0, 1.0, 1.0), **{k: v.data_ptr() for k, v in planes.items()})
        return ctx.last_kernel_ms()

    def yardstick():
        rt.render_device(ctx, scene, cam, rd, 4242, 0, frame.data_ptr())
        return ctx.last_kernel_ms()

    def aov_depth_object():          # 8 of the 44 bytes per pixel: less written than the yardstick's 12
        rt.render_aov_device(ctx, scene, cam, (1.0, 1.0, 1.0), d_depth=planes["d_depth"].data_ptr(), d_object=planes["d_object"].data_ptr())
        return ctx.last_kernel_ms()

    for _ in range(3):
        aov(); yardstick(); aov_depth_object()
    a_ms, y_ms, s_ms = [], [], []
    for _ in range(args.pairs):
        a_ms.append(aov())
        y_ms.append(yardstick())
        s_ms.append(aov_depth_object())
    am, ym = statistics.median(a_ms), statistics.median(y_ms)
    out["aov"] = {"scene": "monkey", "width": W, "height": H, "pairs": args.pairs, "aov_kernel_ms_median": am, "aov_kernel_ms": a_ms,
                  "aov_mrays_per_s": W * H / am / 1e3, "yardstick": "rt_render_device 1 spp, limit 1, antialias off", "yardstick_kernel_ms_median": ym,
                  "yardstick_kernel_ms": y_ms, "yardstick_spread_ms": max(y_ms) - min(y_ms), "aov_over_yardstick": am / ym,
                  "aov_depth_object_only_kernel_ms_median": statistics.median(s_ms), "aov_depth_object_only_kernel_ms": s_ms}

    # ---- incoherent queries
    n = args.rays
    o, d = random_rays(n, 21)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_h = torch.empty(n * rt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    out["incoherent"] = {}
    for name in ("monkey", "soup6k", "sphere50k"):
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        sc = ctx.commit(rt.SceneObjects(objs, models))
        ms = []
        for k in range(7):
            rt.trace_rays_device(ctx, sc, t_o.data_ptr(), t_d.data_ptr(), n, t_h.data_ptr())
            ms.append(ctx.last_kernel_ms())
        med = statistics.median(ms[2:])
        hits = t_h.cpu().numpy().view(rt.HIT_DTYPE)
        out["incoherent"][name] = {"rays": n, "kernel_ms_median": med, "kernel_ms": ms, "mrays_per_s": n / med / 1e3, "hit_fraction": float((hits["object"] >= 0).mean()),
                                   "placement": sc.info()["scene_in_lds"], "threads": sc.info()["threads_per_block"]}
        if name == "monkey":
            small = {}
            for k in (1, 64, 4096, 65536):
                for _ in range(3):
                    rt.trace_rays_device(ctx, sc, t_o.data_ptr(), t_d.data_ptr(), k, t_h.data_ptr())
                ctx.synchronize()
                reps = 20
                t0 = time.perf_counter()
                for _ in range(reps):
                    rt.trace_rays_device(ctx, sc, t_o.data_ptr(), t_d.data_ptr(), k, t_h.data_ptr())
                    ctx.synchronize()
                small[str(k)] = {"ms_per_call": (time.perf_counter() - t0) * 1e3 / reps, "kernel_ms_last": ctx.last_kernel_ms()}
            out["small_batches_monkey"] = small
    print(json.dumps(out))


if __name__ == "__main__":
    main()
