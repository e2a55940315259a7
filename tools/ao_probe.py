"""Measurements of the ambient-occlusion plane on the GPU (one JSON line), the sibling of tools/occlusion_probe.py:

  fused       render_ao_device on the metric scene (monkey, 1920x1080, 16 samples, radius 0.5): kernel ms from rt_last_kernel_ms, the median
              and spread (max - min) of --runs runs after 2 warm-ups
  unfused     the same plane from the entry points the library had before, leg by leg in the same loop: trace_rays_device on the primary
              rays (kernel ms), the segments of the pixels that hit made with torch on the device (the same distribution, not the same
              bits: torch.randn; CUDA-event ms), occluded_rays_device on them (kernel ms), a torch reduction into the count plane (event
              ms); each leg's median and the per-run sums' median and spread.  Acceptance: fused median <= unfused sum median + its spread
  occlusion   the fused pass against occluded_rays_device alone on the same number of rays: what drawing the directions in the kernel costs
  sweep       samples 4 / 16 / 64 on monkey, soup6k and sphere50k (--sweep-size, default 960x540); with --sweep 8,16,24,32 the same in a fresh
              child process per value, each loading the development build libraytracer_amd_aorefill<N>.so
              (build.build_variant("aorefill<N>", ["-DRT_AO_REFILL=<N>"])), the metric scene at full size included

    python tools/ao_probe.py [--runs 7] [--sweep 8,16,24,32] [--sweep-size 960x540]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRIC = dict(scene="monkey", width=1920, height=1080, samples=16, radius=0.5, bias=1e-3, time_ms=12345)
WARMUPS = 2


def spread(x):
    return max(x) - min(x)


def summary(ms):
    return {"kernel_ms_median": statistics.median(ms), "spread_ms": spread(ms), "kernel_ms": ms}


def fused_runs(rt, ctx, torch, scene, W, H, samples, radius, runs):
    dev = torch.device("cuda:0")
    cam = rt.Camera(W, H)
    t_count = torch.empty((H, W), dtype=torch.int16, device=dev)
    t_ao = torch.empty((H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ms = []
    for i in range(WARMUPS + runs):
        rt.render_ao_device(ctx, scene, cam, samples=samples, radius=radius, bias=METRIC["bias"], time_ms=METRIC["time_ms"], d_count=t_count.data_ptr(),
                            d_ao=t_ao.data_ptr())
        ms.append(ctx.last_kernel_ms())
    count = t_count.cpu().numpy().view(np.uint16)
    surface = count != rt.AO_NO_SURFACE
    res = summary(ms[WARMUPS:])
    res.update(surface_pixels=int(surface.sum()), mean_ao=float(t_ao.mean().item()), segments=int(surface.sum()) * samples,
               msegments_per_s=int(surface.sum()) * samples / res["kernel_ms_median"] / 1e3)
    return res


def primaries(torch, cam_floats, W, H, dev):
    """the view's primary rays on the device (made once, outside every timed leg)"""
    c = torch.tensor(np.asarray(cam_floats, np.float32), device=dev)
    pos, tl, du, dv = c[0:3], c[3:6], c[6:9], c[9:12]
    px = torch.arange(W, device=dev, dtype=torch.float32)[None, :, None]
    py = torch.arange(H, device=dev, dtype=torch.float32)[:, None, None]
    a = (tl + (du * px + dv * py)) - pos
    d = a / a.norm(dim=2, keepdim=True)
    return pos.expand(H, W, 3).contiguous().reshape(-1, 3), d.reshape(-1, 3).contiguous()


def unfused_runs(rt, ctx, torch, scene, W, H, samples, radius, runs):
    dev = torch.device("cuda:0")
    n = W * H
    rec = rt.HIT_DTYPE.itemsize // 4
    t_o, t_d = primaries(torch, rt.Camera(W, H).floats(), W, H, dev)
    t_h = torch.empty((n, rec), dtype=torch.float32, device=dev)
    obj_col = rt.HIT_DTYPE.fields["object"][1] // 4
    t_count = torch.empty(n, dtype=torch.int16, device=dev)
    legs = {"primary_kernel_ms": [], "directions_torch_ms": [], "occlusion_kernel_ms": [], "reduction_torch_ms": []}
    sums, rays = [], 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for i in range(WARMUPS + runs):
        rt.trace_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), n, t_h.data_ptr())
        primary = ctx.last_kernel_ms()                       # (waits for the kernel)
        ev[0].record()
        idx = torch.nonzero(t_h[:, obj_col].view(torch.int32) >= 0).squeeze(1)
        P, N = t_h[idx, 1:4], t_h[idx, 4:7]
        o2 = N * METRIC["bias"] + P
        r = torch.randn((idx.numel(), samples, 3), device=dev)
        r = torch.where(((r * N[:, None, :]).sum(2, keepdim=True) < 0), -r, r)
        r = r / r.norm(dim=2, keepdim=True)
        d = N[:, None, :] + r
        d = (d / d.norm(dim=2, keepdim=True)).reshape(-1, 3).contiguous()
        o = o2[:, None, :].expand(-1, samples, -1).reshape(-1, 3).contiguous()
        tmax = torch.full((o.shape[0],), radius, dtype=torch.float32, device=dev)
        occ = torch.empty(o.shape[0], dtype=torch.uint8, device=dev)
        ev[1].record()
        torch.cuda.synchronize()
        rt.occluded_rays_device(ctx, scene, o.data_ptr(), d.data_ptr(), tmax.data_ptr(), o.shape[0], occ.data_ptr())
        occlusion = ctx.last_kernel_ms()
        ev[2].record()
        t_count.fill_(-1)
        t_count[idx] = (samples - occ.view(-1, samples).sum(1, dtype=torch.int32)).to(torch.int16)
        ev[3].record()
        torch.cuda.synchronize()
        rays = int(o.shape[0])
        if i >= WARMUPS:
            row = (primary, ev[0].elapsed_time(ev[1]), occlusion, ev[2].elapsed_time(ev[3]))
            for k, v in zip(legs, row):
                legs[k].append(v)
            sums.append(sum(row))
        del o, d, r, tmax, occ, o2, P, N, idx
    res = {k.replace("_ms", "_ms_median"): statistics.median(v) for k, v in legs.items()}
    res.update(legs)
    res.update(sum_ms_median=statistics.median(sums), sum_spread_ms=spread(sums), sum_ms=sums, occlusion_rays=rays)
    return res


def sweep_leg(rt, ctx, torch, runs, size, with_metric):
    models = rt.scenes.models_dir()
    W, H = size
    out = {}
    for name in ("monkey", "soup6k", "sphere50k"):
        sc = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models))
        out[name] = {"width": W, "height": H, "placement": sc.info()["scene_in_lds"], "threads": sc.info()["threads_per_block"]}
        for samples in (4, 16, 64):
            r = fused_runs(rt, ctx, torch, sc, W, H, samples, METRIC["radius"], runs)
            out[name]["samples_%d" % samples] = {k: r[k] for k in ("kernel_ms_median", "spread_ms", "msegments_per_s")}
        if with_metric and name == METRIC["scene"]:
            r = fused_runs(rt, ctx, torch, sc, METRIC["width"], METRIC["height"], METRIC["samples"], METRIC["radius"], runs)
            out["metric"] = {k: r[k] for k in ("kernel_ms_median", "spread_ms", "msegments_per_s")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--sweep-size", default="960x540")
    ap.add_argument("--sweep-leg", action="store_true", help="(child of --sweep) the sweep legs with the library RT_AMD_LIB names")
    args = ap.parse_args()
    assert args.runs >= 5, "medians of at least 5 runs"
    size = tuple(int(x) for x in args.sweep_size.split("x"))
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    ctx = rt.Context(0)
    if args.sweep_leg:
        print(json.dumps(sweep_leg(rt, ctx, torch, args.runs, size, True)))
        return
    out = {"tool": "ao_probe", "version": rt.lib().rt_version().decode(), "runs": args.runs, "warmups": WARMUPS, "metric": METRIC}
    scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[METRIC["scene"]]()[0], rt.scenes.models_dir()))
    W, H, samples, radius = METRIC["width"], METRIC["height"], METRIC["samples"], METRIC["radius"]
    out["fused"] = f = fused_runs(rt, ctx, torch, scene, W, H, samples, radius, args.runs)
    out["unfused"] = u = unfused_runs(rt, ctx, torch, scene, W, H, samples, radius, args.runs)
    out["acceptance"] = {"fused_ms_median": f["kernel_ms_median"], "unfused_sum_ms_median": u["sum_ms_median"], "unfused_sum_spread_ms": u["sum_spread_ms"],
                         "fused_over_unfused": f["kernel_ms_median"] / u["sum_ms_median"],
                         "met": bool(f["kernel_ms_median"] <= u["sum_ms_median"] + u["sum_spread_ms"])}
    out["occlusion_only"] = {"fused_ms_median": f["kernel_ms_median"], "fused_segments": f["segments"], "occlusion_kernel_ms_median": u["occlusion_kernel_ms_median"],
                             "occlusion_rays": u["occlusion_rays"], "fused_over_occlusion": f["kernel_ms_median"] / u["occlusion_kernel_ms_median"]}
    out["sweep"] = sweep_leg(rt, ctx, torch, args.runs, size, False)
    if args.sweep:
        out["refill_sweep"] = {}
        del scene, ctx
        torch.cuda.empty_cache()
        for v in args.sweep.split(","):
            lib = os.path.join(ROOT, "ray-tracer_amd", "libraytracer_amd_aorefill%s.so" % v)
            if not os.path.exists(lib):
                out["refill_sweep"][v] = "no such build: " + os.path.basename(lib)
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-leg", "--runs", str(args.runs), "--sweep-size", args.sweep_size],
                               env=dict(os.environ, RT_AMD_LIB=lib), capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                out["refill_sweep"][v] = "child failed (%d): %s" % (r.returncode, r.stderr[-300:])
                break                                   # nothing more is started on the GPU after a failure
            out["refill_sweep"][v] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
