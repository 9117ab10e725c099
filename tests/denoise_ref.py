"""numpy float32 restatement of rt_denoise (include/rtgpu.h; the kernel is
go-raytracing_amd/csrc/denoise.hip) with the kernel's operation order: the 25
taps row-major with dy outer, every sum and product in float32 in the same
association.  Also the synthetic test images the host and GPU tests share."""
import numpy as np

F = np.float32
HK = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
DEFAULTS = dict(iterations=5, normal_power_log2=5, demodulate=1, sigma_color=4.0, sigma_depth=0.1, albedo_eps=1e-3)
BAR = 1e-5   # tests/test_gpu_parity.py: every pixel within BAR * max(1, |ref|)
FP32_OFF = 1e-3


def denoise_ref(accum, feat, spp, **params):
    p = dict(DEFAULTS, **params)
    accum = np.ascontiguousarray(accum, F)
    feat = np.ascontiguousarray(feat, F)
    if p["iterations"] == 0:
        return accum.copy()
    H, W = accum.shape[:2]
    sp = F(spp)
    eps = F(p["albedo_eps"])
    with np.errstate(all="ignore"):
        c = accum / sp
        a = feat[..., 0:3] / sp
        n = feat[..., 3:6] / sp
        z = feat[..., 6] / sp
        k = feat[..., 7] / sp
        m = np.where(a > eps, a, eps).astype(F)
        e = (c / m if p["demodulate"] else c).astype(F)
        through = k < F(0.5)
        zden = F(p["sigma_depth"]) * np.abs(z) + F(1e-6)
        ys, xs = np.mgrid[0:H, 0:W]
        for i in range(p["iterations"]):
            s = 1 << i
            sigma = F(np.ldexp(F(p["sigma_color"]), -i))
            sig2 = F(sigma * sigma + F(1e-8))
            wsum = np.zeros((H, W), F)
            acc = np.zeros((H, W, 3), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    valid = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    eq = e[qy, qx]
                    if dx == 0 and dy == 0:
                        w = np.ones((H, W), F)
                    else:
                        valid &= ~through[qy, qx]
                        nq = n[qy, qx]
                        d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                        wn = np.where(d > 0, d, F(0)).astype(F)
                        for _ in range(p["normal_power_log2"]):
                            wn = wn * wn
                        wz = np.exp(-(np.abs(z - z[qy, qx]) / zden))
                        u = e - eq
                        d2 = (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]
                        wc = np.exp(-(d2 / sig2))
                        w = (wn * wz) * wc
                    hw = F(HK[dy + 2] * HK[dx + 2]) * w
                    hw = np.where(valid, hw, F(0)).astype(F)
                    wsum = wsum + hw
                    acc = acc + np.where(valid[..., None], hw[..., None] * eq, F(0)).astype(F)
            e = np.where(through[..., None], e, acc / wsum[..., None]).astype(F)
        out = (e * m) * sp if p["demodulate"] else e * sp
    assert out.dtype == F
    return np.where(through[..., None], accum, out).astype(F)


def synthetic(w, h, spp=4, seed=0):
    """A noisy frame with its features: three surfaces (a slanted floor, a
    wall facing +z and a tilted box with its own normal), textured albedo,
    an uncovered band (coverage 0: sky / emitter) and a few half-covered
    pixels (coverage 1/spp .. 1), noise of O(1) on radiance of O(1)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    region = (xs * 3 // w + (ys > h // 2)) % 3
    normals = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]], F)
    n = normals[region]
    z = (F(2.0) + F(0.05) * xs + F(0.5) * region + F(0.02) * ys).astype(F)
    alb = (F(0.2) + F(0.6) * (((xs // 5) + (ys // 3)) % 2)[..., None] * np.array([1.0, 0.5, 0.25], F)).astype(F)
    cover = np.ones((h, w), F) * spp
    cover[(ys >= h // 3) & (ys < h // 3 + 3) & (xs > w // 4)] = 0      # pass-through band
    part = rng.random((h, w)) < 0.03
    cover[part & (cover > 0)] = rng.integers(1, spp + 1, (h, w))[part & (cover > 0)]
    feat = np.zeros((h, w, 8), F)
    feat[..., 0:3] = alb * cover[..., None]
    feat[..., 3:6] = n * cover[..., None]
    feat[..., 6] = z * cover
    feat[..., 7] = cover
    light = (F(0.5) + F(0.5) * np.sin(xs / F(7.0)) * np.cos(ys / F(5.0)))[..., None].astype(F)
    rad = alb * light * (F(1.0) + F(0.8) * rng.standard_normal((h, w, 3)).astype(F))
    accum = (np.abs(rad) * spp).astype(F)
    accum[cover == 0] = (F(3.0) * rng.random((h, w, 3)).astype(F))[cover == 0] * spp   # sky / emitter radiance
    return np.ascontiguousarray(accum), np.ascontiguousarray(feat)


def two_regions(w, h, spp=2, seed=1, right_scale=1.0):
    """Left half normals +x, right half +y (w_n is exactly 0 across the
    edge); `right_scale` changes the right half's colours only."""
    rng = np.random.default_rng(seed)
    feat = np.zeros((h, w, 8), F)
    left = np.arange(w) < w // 2
    feat[:, left, 3] = spp
    feat[:, ~left, 4] = spp
    feat[..., 0:3] = F(0.5) * spp
    feat[..., 6] = F(3.0) * spp
    feat[..., 7] = spp
    accum = (rng.random((h, w, 3)).astype(F) * spp).astype(F)
    accum[:, ~left] = accum[:, ~left] * F(right_scale) + F(right_scale - 1.0)
    return np.ascontiguousarray(accum), feat
