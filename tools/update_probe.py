"""Measurements of Scene.update_mesh / update_mesh_device on the GPU (one JSON line at the end), the sibling of tools/views_probe.py.  Every
figure is the median of --runs runs after a warm-up round, with the spread (max - min) beside it; the legs of a mesh alternate run by run, in
one process on one build.  A step's vertices alternate between two displaced copies of the mesh, so no update is a no-op.

  per mesh (the monkey, soup6k, sphere50k, a 200,003-triangle soup):
     device   update_mesh_device from a tensor on the GPU: device milliseconds between two events around the call, and wall milliseconds of the
              call with a synchronisation behind it
     host     update_mesh from a NumPy array (wall): the copy to the device, the same kernels, the wait
     today    what a caller has without the update, from the same tensor (wall): copy the vertices to the host, a new builder, its host tree build
              (rt_scene_add_mesh), rt_scene_commit, the old scene destroyed
     The updated scene's device content is compared once with the recommitted scene's, bit for bit.
  loop: the monkey scene at 1920 x 1080, 64 samples x 8 bounces: frames per second of (update + one frame) against (recommit + one frame)

    python tools/update_probe.py [--runs 7] [--meshes monkey,soup6k,sphere50k,soup200k] [--loop-steps 6]
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


def med(x):
    return {"median": round(statistics.median(x), 4), "spread": round(max(x) - min(x), 4), "runs": [round(v, 4) for v in x]}


def soup200k(n=200003, seed=17):
    rng = np.random.default_rng(seed)
    centres = rng.uniform([-1.2, -0.6, 1.2], [1.2, 0.8, 3.5], (n, 3))
    tris = (centres[:, None, :] + rng.normal(0, 0.01, (n, 3, 3))).astype(np.float32).reshape(n, 9)
    return [("mesh", tris, ("standard", (0.8, 0.7, 0.6), 0.1)), ("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), 0.3))], (0.8, 1.0, 1.0)


class Probe:
    def __init__(self, runs):
        import torch
        self.torch = torch
        self.rt = importlib.import_module("ray-tracer_amd")
        self.ctx = self.rt.Context(0)
        self.models = self.rt.scenes.models_dir()
        self.runs = runs

    def scene_objs(self, name):
        objs, sky = soup200k() if name == "soup200k" else self.rt.scenes.CONFIG_SCENES[name]()
        index = next(i for i, o in enumerate(objs) if o[0] in ("mesh", "obj"))
        o = objs[index]
        if o[0] == "obj":
            m = self.rt.ObjFileMesh(os.path.join(self.models, o[1]))
            for t in o[2]:
                getattr(m, t[0])(*t[1:])
            base = m.triangles()
        else:
            base = np.asarray(o[1], np.float32).reshape(-1, 9)
        return list(objs), sky, index, base

    def displaced(self, base, k):
        t = base.copy().reshape(-1, 3, 3)
        t[:, :, 1] += (np.float32(0.03) * np.sin(np.float32(1 + k) + np.float32(3) * t[:, :, 0])).astype(np.float32)
        return t.reshape(-1, 9)

    def wall(self, fn):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        self.ctx.synchronize()
        self.torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def recommit(self, objs, index, d_tris):
        """today's path from vertices on the device -> the new scene"""
        rt = self.rt
        host = d_tris.cpu().numpy()
        replaced = list(objs)
        replaced[index] = ("mesh", host, objs[index][-1])
        return self.ctx.commit(rt.SceneObjects(replaced, self.models))

    def mesh(self, name):
        rt, torch = self.rt, self.torch
        objs, _, index, base = self.scene_objs(name)
        steps = [self.displaced(base, k) for k in (0, 1)]
        d_steps = [torch.from_numpy(s).to("cuda:0") for s in steps]
        scene = self.ctx.commit(rt.SceneObjects(objs, self.models))
        stream = torch.cuda.current_stream().cuda_stream
        # once: the update gives what the recommit gives
        scene.update_mesh_device(index, d_steps[0], stream=stream)
        other = self.recommit(objs, index, d_steps[0])
        a, b = scene.debug_read(), other.debug_read()
        same = a["blob"].tobytes() == b["blob"].tobytes() and a["objects"].tobytes() == b["objects"].tobytes()
        del other
        device_ms, device_wall, host_wall, today_wall = [], [], [], []
        for run in range(self.runs + 1):                 # run 0 warms every leg up
            k = (run + 1) % 2
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def device():
                e0.record()
                scene.update_mesh_device(index, d_steps[k], stream=stream)
                e1.record()
            w_dev, _ = self.wall(device)
            w_host, _ = self.wall(lambda: scene.update_mesh(index, steps[1 - k]))
            w_today, _ = self.wall(lambda: self.recommit(objs, index, d_steps[k]) and None)      # (the new scene is destroyed inside the window)
            if run:
                device_ms.append(e0.elapsed_time(e1)); device_wall.append(w_dev); host_wall.append(w_host); today_wall.append(w_today)
        out = {"triangles": int(base.shape[0]), "equal_to_recommit": bool(same), "device_ms": med(device_ms), "device_wall_ms": med(device_wall),
               "host_form_wall_ms": med(host_wall), "today_wall_ms": med(today_wall)}
        out["faster_than_today_by_more_than_its_spread"] = bool(out["today_wall_ms"]["median"] - out["device_wall_ms"]["median"] > out["today_wall_ms"]["spread"])
        return out

    def loop(self, steps):
        rt, torch = self.rt, self.torch
        objs, sky, index, base = self.scene_objs("monkey")
        W, H = 1920, 1080
        cam, rd = rt.Camera(W, H), rt.RenderData(64, 8, True, sky)
        frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
        d_steps = [torch.from_numpy(self.displaced(base, k)).to("cuda:0") for k in range(steps)]
        stream = torch.cuda.current_stream().cuda_stream
        scene = self.ctx.commit(rt.SceneObjects(objs, self.models))

        def updating():
            for k in range(steps):
                scene.update_mesh_device(index, d_steps[k], stream=stream)
                rt.render_device(self.ctx, scene, cam, rd, 100 + k, 0, frame.data_ptr(), stream=stream)

        def recommitting():
            for k in range(steps):
                s = self.recommit(objs, index, d_steps[k])
                rt.render_device(self.ctx, s, cam, rd, 100 + k, 0, frame.data_ptr(), stream=stream)
                self.ctx.synchronize()                   # (the scene goes at the end of the step)

        up, re = [], []
        for run in range(self.runs + 1):
            a, _ = self.wall(updating)
            b, _ = self.wall(recommitting)
            if run:
                up.append(steps / (a / 1e3)); re.append(steps / (b / 1e3))
        return {"scene": "monkey 1920x1080, 64 spp x 8 bounces", "steps": steps, "update_fps": med(up), "recommit_fps": med(re)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--meshes", default="monkey,soup6k,sphere50k,soup200k")
    ap.add_argument("--loop-steps", type=int, default=6)
    args = ap.parse_args()
    p = Probe(max(5, args.runs))
    out = {"probe": "update", "runs": p.runs, "meshes": {}}
    for name in [m for m in args.meshes.split(",") if m]:
        out["meshes"][name] = p.mesh(name)
        r = out["meshes"][name]
        print("%-10s %7d triangles: device %.3f ms (events; spread %.3f), %.3f ms wall; host form %.3f ms; today %.3f ms (spread %.3f); equal %s" % (
            name, r["triangles"], r["device_ms"]["median"], r["device_ms"]["spread"], r["device_wall_ms"]["median"], r["host_form_wall_ms"]["median"],
            r["today_wall_ms"]["median"], r["today_wall_ms"]["spread"], r["equal_to_recommit"]), flush=True)
    if args.loop_steps > 0:
        out["loop"] = p.loop(args.loop_steps)
        print("loop: update %.2f fps, recommit %.2f fps" % (out["loop"]["update_fps"]["median"], out["loop"]["recommit_fps"]["median"]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
