#!/usr/bin/env python3
"""Device time of the moments render beside the plain render, and of
rt_denoise_variance beside rt_denoise (DESIGN.md "Radiance moments and the
variance-guided filter").  The method is tools/feature_denoise_time.py's:
HIP events on the call's stream, warm-up then `--reps` repetitions, median and
min..max.  Renders are timed at 4 spp and at a quarter of the headline's
samples (`--spp` / 4) at the scene's depth, the two kinds alternating in one
session; the filters at 4 spp (moments) and at 1 spp (spatial estimate).
Prints one JSON line.

    python tools/moments_denoise_time.py --scene cornell-lucy --width 1200 --reps 15
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
    ap.add_argument("--spp", type=int, default=500, help="the headline's samples per pixel")
    ap.add_argument("--depth", type=int, default=0, help="0: scene default")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    g = ge.load_package()
    s = g.Scene(a.scene, width=a.width, aspect=a.aspect)
    cam = s.camera
    W, H = cam.image_width, cam.image_height
    depth = a.depth or cam.max_depth
    ctx = g.Context(0)
    ctx.upload(s.desc)
    dev = "cuda:0"
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    mom = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
    feat = torch.zeros((H, W, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    var = torch.zeros((H, W), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def timed(fns):
        """Every fn in turn per repetition (interleaved), one list of ms per fn."""
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
        return ms

    res = dict(scene=a.scene, width=W, height=H, depth=depth, headline_spp=a.spp)
    for spp in (4, max(1, a.spp // 4)):
        p = g.make_params(spp, depth, seed=1)
        plain, moments = timed([lambda: ctx.render_device(cam, p, accum.data_ptr(), st.cuda_stream),
                                lambda: ctx.render_moments_device(cam, p, accum.data_ptr(), mom.data_ptr(),
                                                                  st.cuda_stream)])
        res[f"render_{spp}spp_ms"] = spread(plain)
        res[f"render_moments_{spp}spp_ms"] = spread(moments)
        res[f"moments_over_plain_{spp}spp"] = round(statistics.median(moments) / statistics.median(plain), 4)
    # the filters: over a 4-spp frame with its moments, then over the 1-spp preview
    p4 = g.make_params(4, depth, seed=1)
    ctx.render_moments_device(cam, p4, accum.data_ptr(), mom.data_ptr(), st.cuda_stream)
    ctx.render_features_device(cam, p4, feat.data_ptr(), st.cuda_stream)
    ctx.sync()
    den, denv, denv_novar = timed([
        lambda: ctx.denoise_device(accum.data_ptr(), feat.data_ptr(), W, H, 4, out.data_ptr(), st.cuda_stream),
        lambda: ctx.denoise_variance_device(accum.data_ptr(), feat.data_ptr(), mom.data_ptr(), W, H, 4, out.data_ptr(),
                                            var.data_ptr(), st.cuda_stream),
        lambda: ctx.denoise_variance_device(accum.data_ptr(), feat.data_ptr(), mom.data_ptr(), W, H, 4, out.data_ptr(),
                                            0, st.cuda_stream)])
    res["denoise_4spp_ms"] = spread(den)
    res["denoise_variance_4spp_ms"] = spread(denv)
    res["denoise_variance_4spp_no_out_var_ms"] = spread(denv_novar)
    p1 = g.make_params(1, 3, seed=1)
    ctx.render_device(cam, p1, accum.data_ptr(), st.cuda_stream)
    ctx.render_features_device(cam, p1, feat.data_ptr(), st.cuda_stream)
    ctx.sync()
    den1, denv1 = timed([
        lambda: ctx.denoise_device(accum.data_ptr(), feat.data_ptr(), W, H, 1, out.data_ptr(), st.cuda_stream),
        lambda: ctx.denoise_variance_device(accum.data_ptr(), feat.data_ptr(), 0, W, H, 1, out.data_ptr(),
                                            var.data_ptr(), st.cuda_stream)])
    res["denoise_1spp_ms"] = spread(den1)
    res["denoise_variance_1spp_spatial_ms"] = spread(denv1)
    res["covered_share"] = float((feat[..., 7] > 0).float().mean())
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
