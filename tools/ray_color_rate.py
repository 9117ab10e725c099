#!/usr/bin/env python3
"""rt_ray_color's rate beside rt_render's (DESIGN.md "Ray colour").  Prints one
JSON line.

The rays are the headline frame's own camera rays: rt_extend_hits' bounce-0
rays of `--samples` samples of every pixel, id = pixel, kept on the device.
Two comparisons, both with HIP events on a stream of their own, alternating
the two sides repetition by repetition after a warm-up; median and min..max
over `--reps` repetitions:

  replay: per sample s, rt_ray_color_device(rays of sample s, samples = 1,
          sample_offset = s, accumulate) against rt_render_device(1 sample,
          sample_offset = s, accumulate): the same paths, launch for launch
          but for the ray source.  The two frames must be equal bit for bit.
  batch:  rt_ray_color_device(rays of sample 0, samples = `--samples`) against
          rt_render_device(`--samples` samples): one call each, the form a
          bake takes (a ray keeps its direction over its samples).

Beside them the span and the kernel classes' times (rt_last_kernel_times) of
one one-sample call of each side.  The classes overlap between the twin
streams, so they do not add up to the span; k_ray_source is in no class: its
share comes from a kernel trace of this tool in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/ray_color_rate.py --reps 2).

    python tools/ray_color_rate.py --scene cornell-lucy --width 1200 --samples 16 --depth 5
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
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as ge
    g = ge.load_package()

    s = g.Scene(a.scene, width=a.width, aspect=a.aspect)
    cam = s.camera
    ctx = g.Context(0)
    ctx.upload(s.desc)
    n = cam.image_width * cam.image_height
    dev = "cuda:0"
    d_rays = []
    for smp in range(a.samples):
        top, _, _, ray = ctx.extend_hits(cam, a.seed, smp, 0)
        rays = g.make_path_rays(ray[:, 0:3], ray[:, 3:6])
        d_rays.append(torch.from_numpy(rays.view(np.int32).reshape(n, 8).copy()).to(dev))
    d_ray_rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    d_frame = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def replay_rays():
        for smp in range(a.samples):
            p = g.ray_color_params(1, a.depth, seed=a.seed, sample_offset=smp, camera=cam, accumulate=smp > 0)
            ctx.ray_color_device(d_rays[smp].data_ptr(), n, p, d_ray_rgb.data_ptr(), stream=st.cuda_stream)

    def replay_render():
        for smp in range(a.samples):
            ctx.render_device(cam, g.make_params(1, a.depth, seed=a.seed, sample_offset=smp, accumulate=smp > 0),
                              d_frame.data_ptr(), stream=st.cuda_stream)

    def batch_rays():
        p = g.ray_color_params(a.samples, a.depth, seed=a.seed, camera=cam)
        ctx.ray_color_device(d_rays[0].data_ptr(), n, p, d_ray_rgb.data_ptr(), stream=st.cuda_stream)

    def batch_render():
        ctx.render_device(cam, g.make_params(a.samples, a.depth, seed=a.seed), d_frame.data_ptr(), stream=st.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ctx.sync()
        return e0.elapsed_time(e1)

    out = {}
    for name, sides in (("replay", (replay_rays, replay_render)), ("batch", (batch_rays, batch_render))):
        ms = [[], []]
        for k in range(a.warmup + a.reps):
            for j, fn in enumerate(sides):
                t = timed(fn)
                if k >= a.warmup:
                    ms[j].append(t)
        if name == "replay":
            same = bool(torch.equal(d_ray_rgb.view(torch.int32), d_frame.view(torch.int32)))
            assert same, "the replayed frame differs from the rendered one"
            out["replay_bit_equal"] = same
        msamples = n * a.samples / 1e6
        rr, rd = statistics.median(ms[0]), statistics.median(ms[1])
        out[name] = dict(ray_color_ms=spread(ms[0]), render_ms=spread(ms[1]),
                         ray_color_msamples_s=round(msamples / (rr * 1e-3), 1), render_msamples_s=round(msamples / (rd * 1e-3), 1),
                         ratio=round(rd / rr, 4))

    # the kernel classes of one timed sample on each side (timing events slow the host: not part of the rates above)
    ctx.set_kernel_timing(True)
    classes = {}
    for side, fn in (("ray_color", lambda: ctx.ray_color_device(
            d_rays[0].data_ptr(), n, g.ray_color_params(1, a.depth, seed=a.seed, camera=cam), d_ray_rgb.data_ptr(),
            stream=st.cuda_stream)),
                     ("render", lambda: ctx.render_device(cam, g.make_params(1, a.depth, seed=a.seed), d_frame.data_ptr(),
                                                          stream=st.cuda_stream))):
        rest = []
        for k in range(a.warmup + a.reps):
            fn()
            st.synchronize()
            ctx.sync()
            t = ctx.last_kernel_times()
            span = ctx.last_render_kernel_ms()
            if k >= a.warmup:
                rest.append(dict(span=span, extend=t["extend_ms"], shade=t["shade_ms"], shadow=t["shadow_ms"]))
        classes[side] = {k: round(statistics.median(r[k] for r in rest), 4) for k in rest[0]}
    ctx.set_kernel_timing(False)
    info = ctx.info()
    ctx.close()
    out["one_sample_kernel_ms"] = classes
    print(json.dumps(dict(scene=a.scene, width=cam.image_width, height=cam.image_height, samples=a.samples, depth=a.depth,
                          rays=n, triangles=info.triangles, **out)))


if __name__ == "__main__":
    main()
