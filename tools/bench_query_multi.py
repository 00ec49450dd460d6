"""Multi-hit ray queries against closest-hit queries: python tools/bench_query_multi.py [--rounds N] [--json out.json]

Device path only (rays already in a torch tensor, rr_query_rays[_multi]_device on torch's stream), on monkey.obj, ott.obj, the
131 072-triangle procedural sphere and C4, for the coherent / incoherent / shadow ray sets of tools/bench_query.py (one 1920x1080
frame's worth each).  Per scene and ray set the variants below run in interleaved rounds in one process -- every round runs each
variant once -- and each is timed with HIP events around the call; the median over the rounds is reported in Mrays/s:
  * closest:        k_query_rays, closest hit
  * k1, k4, k16:    k_query_multi, pruned (no counts)
  * k1c, k4c, k16c: the same with counts (unpruned)
  * loop4:          the workaround k4 replaces: four closest-hit queries, tmin advanced to each hit's t between them (torch ops)
Under rocprofv3 --kernel-trace the launches give the kernel times alone.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from bench_query import load, primary_rays, random_rays, shadow_rays, xf  # noqa: E402
from bench_refit import sphere_grid  # noqa: E402

VARIANTS = ["closest", "k1", "k4", "k16", "k1c", "k4c", "k16c", "loop4"]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="monkey.obj,ott.obj,sphere grid 131072,C4")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    scenes = [("monkey.obj", [load("monkey.obj")], None), ("ott.obj", [load("ott.obj")], None),
              ("sphere grid 131072", [sphere_grid(256)], None),
              ("C4", [load("shell.obj"), load("cube.obj"), load("ott.obj")], rr.make_instances(
                  transforms=[xf(0, 0, 0), xf(0, 0, -4.0), xf(0, 0, 4.0)], meshes=[0, 1, 2]))]
    want = a.scenes.split(",")
    out = {"unit": "Mrays/s (median of %d interleaved rounds, HIP events)" % a.rounds, "scenes": {}}
    prim = primary_rays()
    print("%-20s %-10s %8s | " % ("scene", "rays", "n") + " ".join("%7s" % v for v in VARIANTS) + " | mean count", flush=True)
    for name, meshes, inst in scenes:
        if name not in want:
            continue
        ids = []
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for k, (v, i) in enumerate(meshes):
            mid = r.upload_mesh(v, i)
            r.build_blas(mid)
            ids.append(mid)
            off = inst["transform"][k].reshape(3, 4)[:, 3] if inst is not None else 0.0
            lo = np.minimum(lo, v["position"].min(0) + off)
            hi = np.maximum(hi, v["position"].max(0) + off)
        ii = rr.make_instances(meshes=[ids[0]]) if inst is None else inst.copy()
        if inst is not None:
            ii["blas"] = [ids[int(b)] for b in inst["blas"]]
        r.build_tlas(ii)
        sets = {"coherent": prim, "incoherent": random_rays(len(prim), lo, hi)}
        sets["shadow"] = shadow_rays(prim, r.query_rays(prim))
        row = {}
        for sname, rays in sets.items():
            n = len(rays)
            if n == 0:
                continue
            t = torch.from_numpy(rays.view(np.int32).reshape(-1, 12).copy()).to(dev)
            loop_rays = t.clone()

            def loop4():
                loop_rays.copy_(t)
                f = loop_rays.view(torch.float32)
                for _ in range(4):
                    h = r.query_rays(loop_rays)
                    f[:, 3] = torch.where(h[:, 5] != 0, h[:, 0].view(torch.float32), f[:, 3])

            fns = {"closest": lambda: r.query_rays(t), "loop4": loop4}
            for k in (1, 4, 16):
                fns["k%d" % k] = (lambda k=k: r.query_rays_multi(t, k))
                fns["k%dc" % k] = (lambda k=k: r.query_rays_multi(t, k, counts=True))
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            ts = {v: [] for v in VARIANTS}
            for _ in range(a.rounds):
                for v in VARIANTS:
                    torch.cuda.synchronize()
                    r.timing_begin()
                    fns[v]()
                    ts[v].append(r.timing_end())
            res = {"n": n}
            for v in VARIANTS:
                res[v] = n / float(np.median(ts[v])) / 1e3
            _, c = r.query_rays_multi(t, 0, counts=True)
            res["mean_count"] = float(c.float().mean())
            row[sname] = res
            print("%-20s %-10s %8d | " % (name, sname, n) + " ".join("%7.0f" % res[v] for v in VARIANTS)
                  + " | %.2f" % res["mean_count"], flush=True)
            del t, loop_rays
        out["scenes"][name] = row
    r.reset_stream()
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
