#!/usr/bin/env python3
"""rt_gather_surface beside rt_gather(RT_GATHER_COSINE) (DESIGN.md "Surface
gathers"): what the call costs, what it buys, and how far the two estimators
lie apart.  Prints log lines like profiles/gather_ab.log's.

The points are 2^20 surface points of the scene: the rt_trace_rays hits of the
camera rays of a 1024 x 1024 frame (p = o + t d, n = the hit normal; a miss
becomes the box centre), one id per point, kept on the device.

  cost:     one warm-up call and `--calls` timed calls (rt_last_render_kernel_ms)
            of rt_gather_device COSINE and, where the library has it, of
            rt_gather_surface_device.  RTGPU_LIB_DIR selects another in-tree
            build, e.g. the parent's, which then times COSINE alone.
  variance: (--variance) a fixed subset of 4096 of the points, `--samples`
            samples, 32 seeds: per point the variance over seeds of rgb/samples
            (summed over the channels) for COSINE and for SURFACE and the
            median of their ratio over the points where both are positive; and
            the mean over points and seeds of each estimator and their ratio.

    python tools/surface_rate.py --tag branch-run-1
    RTGPU_LIB_DIR=lib_parent python tools/surface_rate.py --tag parent-run-1
    python tools/surface_rate.py --variance
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-lucy")
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--seed", type=int, default=29)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--variance", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as ge
    g = ge.load_package()

    s = g.Scene(a.scene, width=a.side, aspect=1.0)
    cam = s.camera
    ctx = g.Context(0)
    ctx.upload(s.desc)
    n = cam.image_width * cam.image_height
    _, _, _, ray = ctx.extend_hits(cam, a.seed, 0, 0)
    o, d = ray[:, 0:3], ray[:, 3:6]
    top, _, t, _, nrm, _ = ctx.trace_rays(o, d)
    hit = top >= 0
    p = (o + t[:, None] * d).astype(np.float32)
    p[~hit] = (278.0, 278.0, 278.0)
    nrm = nrm.copy()
    nrm[~hit] = (0.0, 0.0, 1.0)
    pts = g.make_gather_points(p, nrm)
    has_surface = hasattr(ctx._lib, "rt_gather_surface_device")
    print(f"[{a.tag}] lib {os.path.basename(g.LIB_DIR)} points {n} hits {int(hit.sum())} depth {a.depth} samples {a.samples}",
          flush=True)

    def on_device(q):
        return torch.from_numpy(np.ascontiguousarray(q).view(np.int32).reshape(len(q), 8).copy()).to("cuda:0")

    if not a.variance:
        d_pts = on_device(pts)
        d_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        sides = [("rt_gather_device COSINE", lambda: ctx.gather_device(
            d_pts.data_ptr(), n, g.gather_params(g.RT_GATHER_COSINE, a.samples, a.depth, seed=a.seed, camera=cam),
            d_rgb.data_ptr()))]
        if has_surface:
            sides.append(("rt_gather_surface_device", lambda: ctx.gather_surface_device(
                d_pts.data_ptr(), n, g.surface_params(a.samples, a.depth, seed=a.seed, camera=cam), d_rgb.data_ptr())))
            sides.append(("rt_gather_device COSINE (again)", sides[0][1]))
        for name, fn in sides:
            ms = []
            for k in range(1 + a.calls):
                fn()
                ctx.sync()
                ms.append(ctx.last_render_kernel_ms())
            timed = ms[1:]
            med = statistics.median(timed)
            total = float(d_rgb.double().sum().item())
            print(f"[{a.tag}] {name:32s} ms " + " ".join(f"{x:9.3f}" for x in timed) + f"  median {med:9.3f}  Msamples/s "
                  f"{n * a.samples / med / 1e3:8.1f}  (first call {ms[0]:.3f})  sum {total:.6e}", flush=True)
    else:
        sub = np.random.default_rng(7).choice(np.flatnonzero(hit), 4096, replace=False)
        sub.sort()
        q = pts[sub]
        seeds = range(100, 132)
        est = {"cosine": [], "surface": []}
        for seed in seeds:
            c, _ = ctx.gather(q, g.RT_GATHER_COSINE, a.samples, a.depth, seed=seed, camera=cam)
            f, _ = ctx.gather_surface(q, a.samples, a.depth, seed=seed, camera=cam)
            est["cosine"].append(c.astype(np.float64) / a.samples)
            est["surface"].append(f.astype(np.float64) / a.samples)
        ec, es = np.array(est["cosine"]), np.array(est["surface"])        # (seeds, points, 3)
        vc, vs = ec.var(axis=0, ddof=1).sum(axis=1), es.var(axis=0, ddof=1).sum(axis=1)
        both = (vc > 0) & (vs > 0)
        ratio = vc[both] / vs[both]
        mc, msf = ec.mean(axis=0).sum(axis=1), es.mean(axis=0).sum(axis=1)
        lit = (mc > 0) & (msf > 0)
        print(f"[{a.tag}] variance over {len(seeds)} seeds, {len(q)} points x {a.samples} samples, depth {a.depth}: "
              f"median var(COSINE) / var(SURFACE) {np.median(ratio):.2f} (quartiles {np.percentile(ratio, 25):.2f} .. "
              f"{np.percentile(ratio, 75):.2f}, {int(both.sum())} points)", flush=True)
        print(f"[{a.tag}] estimator gap: mean over points of mean(SURFACE) / mean(COSINE) {np.mean(msf[lit] / mc[lit]):.4f} "
              f"({int(lit.sum())} points); ratio of the overall means {msf.sum() / mc.sum():.4f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
