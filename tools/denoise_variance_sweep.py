#!/usr/bin/env python3
"""sigma_lum sweep of rt_denoise_variance beside rt_denoise (DESIGN.md
"Radiance moments and the variance-guided filter").

Four scenes at width 96, both preview passes (4 spp at depth 5 with its
moments, 1 spp at depth 3 through the spatial estimate), seed 5; MSE of the
per-pixel means against a 1024-spp depth-5 frame of seed 977, as a ratio to
the unfiltered pass's.  One JSON line per (scene, sigma_lum, iterations),
with rt_denoise's ratios (its defaults at the same iteration count) beside,
then a summary line: per setting the worst ratio over the eight cells.

    python tools/denoise_variance_sweep.py > profiles/denoise_variance_sweep.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
SCENES = [("cornell", {}), ("random", {}), ("hdri-test", {}), ("cornell-lucy", dict(lucy_rings=60, lucy_cols=80))]


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--sigmas", default="1,2,4,8,16")
    ap.add_argument("--iterations", default="3,5")
    a = ap.parse_args()
    sigmas = [float(x) for x in a.sigmas.split(",")]
    its = [int(x) for x in a.iterations.split(",")]

    import __graft_entry__ as ge
    g = ge.load_package()
    worst = {}
    for name, kw in SCENES:
        s = g.Scene(name, width=a.width, **kw)
        cam = s.camera
        c = g.Context(0)
        c.upload(s.desc)
        ref = c.render(cam, g.make_params(1024, 5, seed=977))[0] / F(1024)
        p4, p1 = g.make_params(4, 5, seed=5), g.make_params(1, 3, seed=5)
        a4, m4, _ = c.render_moments(cam, p4)
        f4 = c.render_features(cam, p4)[0]
        a1, f1 = c.render(cam, p1)[0], c.render_features(cam, p1)[0]
        n4, n1 = mse(a4 / F(4), ref), mse(a1, ref)
        for it in its:
            d4 = mse(c.denoise(a4, f4, 4, iterations=it) / F(4), ref) / n4
            d1 = mse(c.denoise(a1, f1, 1, iterations=it), ref) / n1
            for sg in sigmas:
                v4 = mse(c.denoise_variance(a4, f4, m4, 4, iterations=it, sigma_lum=sg) / F(4), ref) / n4
                v1 = mse(c.denoise_variance(a1, f1, None, 1, iterations=it, sigma_lum=sg), ref) / n1
                print(json.dumps(dict(scene=name, sigma_lum=sg, it=it, ratio4=round(v4, 4), ratio1=round(v1, 4),
                                      denoise_ratio4=round(d4, 4), denoise_ratio1=round(d1, 4),
                                      noisy_mse4=n4, noisy_mse1=n1)), flush=True)
                if it == 5:
                    worst[sg] = max(worst.get(sg, 0.0), v4, v1)
        c.close()
    if worst:
        best = min(worst, key=lambda k: worst[k])
        print(json.dumps(dict(summary="worst ratio over the eight cells at 5 iterations",
                              worst={str(k): round(v, 4) for k, v in worst.items()}, lowest=best)))


if __name__ == "__main__":
    main()
