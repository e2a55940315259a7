"""What the cube-map sky costs on the GPU (one JSON line), the sibling of tools/views_probe.py and on its leg B: 1920 x 1080, 64 samples x 8
bounces, 16 cameras on an orbit, separate frames.  Every figure is the median of --runs runs after a warm-up round, with the spread
(max - min) beside it; the legs alternate run by run.  Times are wall milliseconds around work that starts on an idle device and ends with
a device synchronisation, and beside them the kernel's own (rt_last_kernel_ms).

    legs:  views     render_views_device under the constant sky: the baseline, the parent's unchanged rt_views_kernel
           sky1      render_sky_device under a map of one texel per face, all 1.0f: every lookup hits the same 6 lines; the frames must be
                     the views leg's, bit for bit
           sky1024   render_sky_device under a random 1024-texel map (75 MB at 12 bytes per texel, 100 MB padded): an incoherent load per
                     sample that ends in the sky
    scenes: monkey (the metric scene) and three_sphere (most paths end in the sky)

The texel layout is the library's (RT_SKY_TEXEL_FLOATS, rt_sky.h): run once with the shipped library and once with RT_AMD_LIB pointing at a
build of the other layout (tools/build_variants.py sky12=-DRT_SKY_TEXEL_FLOATS=3); --tag names the run in the output.

    python tools/sky_probe.py [--runs 5] [--tag padded16] [--scenes monkey,three_sphere]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from views_probe import Bench, med, orbit  # noqa: E402


def sky_price(b, name, w=1920, h=1080, spp=64, limit=8, n=16):
    rt, ctx, torch = b.rt, b.ctx, b.torch
    scene, sky_colour = b.scene(name)
    tint = sky_colour if any(sky_colour) else (0.8, 1.0, 1.0)               # (a black sky would multiply the map away)
    rd = rt.RenderData(spp, limit, True, tint)
    cams, times = orbit(rt, w, h, n), [1000 + 7 * i for i in range(n)]
    maps = {"sky1": rt.Sky(ctx, np.ones((6, 1, 1, 3), np.float32)),
            "sky1024": rt.Sky(ctx, np.random.default_rng(1).uniform(0.0, 2.0, (6, 1024, 1024, 3)).astype(np.float32))}
    out = {k: torch.zeros((n, h, w, 3), dtype=torch.float32, device="cuda:0") for k in ("views", "sky1", "sky1024")}
    kernel_ms = {k: [] for k in out}

    def views():
        rt.render_views_device(ctx, scene, cams, rd, times, out["views"].data_ptr())
        kernel_ms["views"].append(ctx.last_kernel_ms())

    def under(k):
        def run():
            rt.render_sky_device(ctx, scene, maps[k], cams, rd, times, out[k].data_ptr())
            kernel_ms[k].append(ctx.last_kernel_ms())
        return run

    res = b.alternate({"views": views, "sky1": under("sky1"), "sky1024": under("sky1024")})
    for k in list(res):
        res[k]["kernel_ms"] = med(kernel_ms[k][1:])
        res[k]["msamples_per_s"] = n * w * h * spp / (res[k]["median"] * 1e-3) / 1e6
    base = res["views"]
    res["sky1_frames_are_the_views_frames"] = bool(torch.equal(out["views"].view(torch.int32), out["sky1"].view(torch.int32)))
    for k in ("sky1", "sky1024"):
        res[k + "_over_views"] = res[k]["median"] / base["median"]
        res[k + "_over_views_kernel"] = res[k]["kernel_ms"]["median"] / base["kernel_ms"]["median"]
    res["views_spread_over_median"] = base["spread"] / base["median"]
    res["views_kernel_spread_over_median"] = base["kernel_ms"]["spread"] / base["kernel_ms"]["median"]
    res["what"] = "%s %dx%d %d spp x %d bounces, %d cameras, tint %s" % (name, w, h, spp, limit, n, tint)
    res["scene"] = scene.info()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--scenes", default="monkey,three_sphere")
    args = ap.parse_args()
    b = Bench(args.runs)
    out = {"runs": args.runs, "tag": args.tag, "library": os.environ.get("RT_AMD_LIB", "the tree's")}
    for name in args.scenes.split(","):
        out[name] = sky_price(b, name)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
