#!/usr/bin/env python3
"""What adaptive sampling costs and what it buys (DESIGN.md "Adaptive
sampling").  Each mode prints one JSON line.

--mode cost: the price of the rounds.  rt_render_adaptive_device with
rel_error = 0, lum_floor = 0 (every pixel with any variance runs every round)
beside one rt_render_moments_device of max_spp samples, alternating in one
session; HIP events on the call's stream, warm-up then `--reps` repetitions,
median and min..max (tools/moments_denoise_time.py's method).

    python tools/adaptive_time.py --mode cost --scene cornell-lucy --width 1200 --max-spp 128

--mode quality: the benefit at equal work.  For the four scenes of the
denoiser tables at width 96, depth 5: the adaptive frame at the defaults with
max_spp 256, normalized, against a uniform render whose spp is the adaptive
run's mean count rounded up (uniform never gets fewer samples); MSE of the
per-pixel means against a 1024-spp frame of another seed.

    python tools/adaptive_time.py --mode quality --width 96 --max-spp 256
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = [("cornell", {}), ("random", {}), ("hdri-test", {}), ("cornell-lucy", dict(lucy_rings=60, lucy_cols=80))]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def cost(g, a):
    import torch
    s = g.Scene(a.scene, width=a.width, aspect=a.aspect)
    cam = s.camera
    W, H = cam.image_width, cam.image_height
    ctx = g.Context(0)
    ctx.upload(s.desc)
    dev = "cuda:0"
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    mom = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
    cnt = torch.zeros((H, W), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    p = g.make_params(a.max_spp, a.depth, seed=1)
    stats = {}

    def adaptive():
        stats["last"] = ctx.render_adaptive_device(cam, p, accum.data_ptr(), mom.data_ptr(), cnt.data_ptr(),
                                                   st.cuda_stream, rel_error=0.0, lum_floor=0.0)

    def uniform():
        ctx.render_moments_device(cam, p, accum.data_ptr(), mom.data_ptr(), st.cuda_stream)

    fns = [uniform, adaptive]
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
    sa = stats["last"]
    rounds = sa.rounds
    res = dict(mode="cost", scene=a.scene, width=W, height=H, depth=a.depth, max_spp=a.max_spp,
               render_moments_ms=spread(ms[0]), render_adaptive_ms=spread(ms[1]),
               adaptive_over_uniform=round(statistics.median(ms[1]) / statistics.median(ms[0]), 4),
               extra_ms=round(statistics.median(ms[1]) - statistics.median(ms[0]), 4),
               extra_ms_per_later_round=round((statistics.median(ms[1]) - statistics.median(ms[0])) / max(1, rounds - 1), 4),
               rounds=rounds, samples=int(sa.samples), pixels_at_max=sa.pixels_at_max,
               samples_share_of_uniform=round(sa.samples / (W * H * a.max_spp), 4),
               last_render_kernel_ms=round(ctx.last_render_kernel_ms(), 4))
    ctx.close()
    return res


def quality(g, a):
    import numpy as np
    F = np.float32
    res = dict(mode="quality", width=a.width, depth=a.depth, max_spp=a.max_spp, scenes={})
    for name, kw in SCENES:
        s = g.Scene(name, width=a.width, **kw)
        cam = s.camera
        c = g.Context(0)
        c.upload(s.desc)
        ref = c.render(cam, g.make_params(1024, a.depth, seed=977))[0] / F(1024)
        accum, _, counts, st = c.render_adaptive(cam, g.make_params(a.max_spp, a.depth, seed=5))
        norm = c.normalize_samples(accum, counts, a.max_spp) / F(a.max_spp)
        mean_count = float(counts.mean())
        spp_u = int(math.ceil(mean_count))
        uni = c.render(cam, g.make_params(spp_u, a.depth, seed=5))[0] / F(spp_u)
        c.close()
        mse_a = float(np.mean((norm.astype(np.float64) - ref) ** 2))
        mse_u = float(np.mean((uni.astype(np.float64) - ref) ** 2))
        res["scenes"][name] = dict(mean_count=round(mean_count, 3), uniform_spp=spp_u, rounds=st.rounds,
                                   pixels_at_max_share=round(st.pixels_at_max / counts.size, 4),
                                   at_min_share=round(float((counts == counts.min()).mean()), 4),
                                   mse_adaptive=mse_a, mse_uniform=mse_u, ratio=round(mse_a / mse_u, 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["cost", "quality"], required=True)
    ap.add_argument("--scene", default="cornell-lucy")
    ap.add_argument("--width", type=int, default=0, help="0: 1200 (cost), 96 (quality)")
    ap.add_argument("--aspect", type=float, default=16.0 / 9.0)
    ap.add_argument("--max-spp", type=int, default=0, help="0: 128 (cost), 256 (quality)")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    a.width = a.width or (1200 if a.mode == "cost" else 96)
    a.max_spp = a.max_spp or (128 if a.mode == "cost" else 256)

    import __graft_entry__ as ge
    g = ge.load_package()
    print(json.dumps(cost(g, a) if a.mode == "cost" else quality(g, a)))


if __name__ == "__main__":
    main()
