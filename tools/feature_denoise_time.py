#!/usr/bin/env python3
"""Device time of the feature pass and the denoiser beside the preview pass
they accompany (DESIGN.md "Feature buffers and denoiser").

HIP events on the call's stream around rt_render_features_device (1 spp) and
rt_denoise_device (default parameters), warm-up then `--reps` repetitions,
median and min..max; the 1-spp depth-3 preview render's own kernel time
(rt_last_render_kernel_ms) from the same session; and the denoiser's
bytes-moved floor.  Prints one JSON line.

    python tools/feature_denoise_time.py --scene cornell-lucy --width 1200 --reps 15
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    g = ge.load_package()
    s = g.Scene(a.scene, width=a.width, aspect=a.aspect)
    cam = s.camera
    W, H = cam.image_width, cam.image_height
    ctx = g.Context(0)
    ctx.upload(s.desc)
    dev = "cuda:0"
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    feat = torch.zeros((H, W, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    p = g.make_params(1, 3, seed=1)   # the first progressive pass: 1 spp, depth 3

    def timed(fn):
        ms = []
        for k in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ctx.sync()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    render_ms = []
    for k in range(a.warmup + a.reps):
        ctx.render_device(cam, p, accum.data_ptr(), st.cuda_stream)
        t = ctx.last_render_kernel_ms()
        if k >= a.warmup:
            render_ms.append(t)
    feat_ms = timed(lambda: ctx.render_features_device(cam, p, feat.data_ptr(), st.cuda_stream))
    den_ms = timed(lambda: ctx.denoise_device(accum.data_ptr(), feat.data_ptr(), W, H, 1, out.data_ptr(),
                                              st.cuda_stream, iterations=a.iterations))
    # per pixel: the first pass reads the sums (12 + 32 B) and writes the guide and
    # its image (16 + 16); middle passes read image + guide and write an image
    # (32 + 16); the last reads image + guide + the albedo half of the features
    # (32 + 16) and writes the sums (12)
    it = a.iterations
    floor_b = W * H * ((44 + 32) + max(0, it - 2) * 48 + (60 if it > 1 else 0))
    bw = ctx.measure_read_bandwidth(1 << 30, 5)
    res = dict(scene=a.scene, width=W, height=H, preview_render_1spp_depth3_kernel_ms=spread(render_ms),
               feature_pass_1spp_ms=spread(feat_ms), denoise_ms=spread(den_ms), denoise_iterations=it,
               denoise_floor_bytes=floor_b, measured_read_gbs=round(bw, 1),
               denoise_floor_ms=round(floor_b / (bw * 1e6), 4), covered_share=float((feat[..., 7] > 0).float().mean()))
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
