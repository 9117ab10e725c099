#!/usr/bin/env python3
"""The ray queries' rate beside k_extend's (DESIGN.md "Ray queries").  Prints
one JSON line.

The rays are the headline scene's own: the bounce-0 and bounce-1 rays of
`--samples` samples of every pixel, taken from rt_extend_hits on the GPU and
concatenated in the order the render's streams hold them (sample by sample,
bounce by bounce, pixel order) into a few million rt_ray with tmin = 0.001,
tmax = +inf.  rt_trace_rays_device and rt_occluded_device over that array are
timed with HIP events on a stream of their own, alternating, after a warm-up;
median and min..max over `--reps` repetitions.  Beside them: k_extend's time
for the same rays, from rt_last_kernel_times of a render of the same samples
to depth 2 (its two k_extend launches trace exactly these rays), repeated the
same number of times.

    python tools/query_rate.py --scene cornell-lucy --width 1200 --samples 3
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-lucy")
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--aspect", type=float, default=16.0 / 9.0)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--nodes", choices=["fp32", "quant8", "wide8"], default="fp32")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as ge
    g = ge.load_package()

    s = g.Scene(a.scene, width=a.width, aspect=a.aspect)
    cam = s.camera
    ctx = g.Context(0)
    ctx.set_node_format(a.nodes)
    ctx.upload(s.desc)
    parts, per_bounce = [], [0, 0]
    for smp in range(a.samples):
        for b in (0, 1):
            top, _, _, ray = ctx.extend_hits(cam, a.seed, smp, b)
            live = np.flatnonzero(top != -2)
            parts.append(g.make_rays(ray[live, 0:3], ray[live, 3:6]))
            per_bounce[b] += len(live)
    rays = np.concatenate(parts)
    n = len(rays)

    dev = "cuda:0"
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).to(dev)
    d_hits = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    d_occ = torch.zeros((n,), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    fns = [lambda: ctx.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=st.cuda_stream),
           lambda: ctx.occluded_device(d_rays.data_ptr(), n, d_occ.data_ptr(), stream=st.cuda_stream)]
    ms = [[] for _ in fns]
    for k in range(a.warmup + a.reps):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ctx.sync()
            if k >= a.warmup:
                ms[j].append(e0.elapsed_time(e1))
    hits = d_hits.cpu().numpy().view(g.RAY_HIT_DTYPE).reshape(n)
    occ = d_occ.cpu().numpy()
    assert np.array_equal(occ != 0, hits["prim"] >= 0), "occluded differs from trace_rays hitting"

    # k_extend over the same rays: bounces 0 and 1 of the same samples
    ctx.set_kernel_timing(True)
    p = g.make_params(a.samples, 2, seed=a.seed)
    ext = []
    for k in range(a.warmup + a.reps):
        ctx.render(cam, p)
        t = ctx.last_kernel_times()
        if k >= a.warmup:
            ext.append(t["extend_ms"])
    ctx.set_kernel_timing(False)
    info = ctx.info()
    ctx.close()

    def rate(v):
        return round(n / (statistics.median(v) * 1e-3) / 1e6, 1)

    print(json.dumps(dict(scene=a.scene, width=cam.image_width, height=cam.image_height, nodes=a.nodes, samples=a.samples,
                          rays=n, rays_bounce0=per_bounce[0], rays_bounce1=per_bounce[1],
                          hit_share=round(float((hits["prim"] >= 0).mean()), 4), triangles=info.triangles,
                          trace_rays_ms=spread(ms[0]), occluded_ms=spread(ms[1]), k_extend_ms=spread(ext),
                          extend_launches=t["extend_launches"],
                          trace_rays_mrays_s=rate(ms[0]), occluded_mrays_s=rate(ms[1]), k_extend_mrays_s=rate(ext),
                          trace_rays_ns_per_ray=round(statistics.median(ms[0]) * 1e6 / n, 3),
                          occluded_ns_per_ray=round(statistics.median(ms[1]) * 1e6 / n, 3),
                          k_extend_ns_per_ray=round(statistics.median(ext) * 1e6 / n, 3))))


if __name__ == "__main__":
    main()
