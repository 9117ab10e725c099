"""numpy float32 restatement of rt_denoise_variance (include/rtgpu.h; the
kernels are go-raytracing_amd/csrc/denoise_var.hip) with the kernels' operation
order: every window row-major with dy outer, every sum and product in float32
in the same association.  Also the test images the host and GPU tests share
(the synthetic frames themselves are tests/denoise_ref.py's)."""
import numpy as np

from tests.denoise_ref import BAR, HK, synthetic, two_regions  # noqa: F401  (re-exported)

F = np.float32
GK = [F(0.25), F(0.5), F(0.25)]
DEFAULTS = dict(iterations=5, normal_power_log2=5, demodulate=1, spatial_below=4, sigma_lum=8.0, sigma_depth=0.1,
                albedo_eps=1e-3)


def lum(e):
    return (F(0.2126) * e[..., 0] + F(0.7152) * e[..., 1]) + F(0.0722) * e[..., 2]


def _shift(ys, xs, dy, dx, H, W):
    qy, qx = ys + dy, xs + dx
    valid = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    return np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1), valid


def denoise_var_ref(accum, feat, moments, spp, **params):
    """(out_rgb, out_var) of rt_denoise_variance."""
    p = dict(DEFAULTS, **params)
    accum = np.ascontiguousarray(accum, F)
    feat = np.ascontiguousarray(feat, F)
    H, W = accum.shape[:2]
    sp = F(spp)
    eps = F(p["albedo_eps"])
    spatial = spp < p["spatial_below"]
    assert p["spatial_below"] >= 2 and (spatial or moments is not None)
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

        def geom(qy, qx):
            nq = n[qy, qx]
            d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            wn = np.where(d > 0, d, F(0)).astype(F)
            for _ in range(p["normal_power_log2"]):
                wn = wn * wn
            wz = np.exp(-(np.abs(z - z[qy, qx]) / zden))
            return (wn * wz).astype(F)

        if spatial:
            l = lum(e)
            sw = np.zeros((H, W), F)
            s1 = np.zeros((H, W), F)
            s2 = np.zeros((H, W), F)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qy, qx, valid = _shift(ys, xs, dy, dx, H, W)
                    if dx == 0 and dy == 0:
                        w = np.ones((H, W), F)
                    else:
                        valid = valid & ~through[qy, qx]
                        w = geom(qy, qx)
                    w = np.where(valid, w, F(0)).astype(F)
                    lq = l[qy, qx]
                    sw = sw + w
                    s1 = s1 + np.where(valid, w * lq, F(0)).astype(F)
                    s2 = s2 + np.where(valid, w * (lq * lq), F(0)).astype(F)
            mean = s1 / sw
            r = s2 / sw - mean * mean
            v = np.where(r > 0, r, F(0)).astype(F)
        else:
            mom = np.ascontiguousarray(moments, F)
            mu = mom[..., 0] / sp
            r = mom[..., 1] / sp - mu * mu
            vy = np.where(r > 0, r, F(0)).astype(F) / (sp - F(1.0))
            mu2 = mu * mu
            le = lum(e)
            v = ((vy / np.where(mu2 > F(1e-12), mu2, F(1e-12)).astype(F)) * (le * le)).astype(F)
        v = np.where(through, F(0), v).astype(F)
        if p["iterations"] == 0:
            return accum.copy(), v
        for i in range(p["iterations"]):
            s = 1 << i
            gs = np.zeros((H, W), F)
            gw = np.zeros((H, W), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx, valid = _shift(ys, xs, dy, dx, H, W)
                    if dx == 0 and dy == 0:
                        w = np.ones((H, W), F)
                    else:
                        valid = valid & ~through[qy, qx]
                        w = geom(qy, qx)
                    wq = F(GK[dy + 1] * GK[dx + 1]) * w
                    gw = gw + np.where(valid, wq, F(0)).astype(F)
                    gs = gs + np.where(valid, wq * v[qy, qx], F(0)).astype(F)
            lden = F(p["sigma_lum"]) * np.sqrt(gs / gw) + F(1e-6)
            lp = lum(e)
            wsum = np.zeros((H, W), F)
            acc = np.zeros((H, W, 3), F)
            sv = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx, valid = _shift(ys, xs, dy * s, dx * s, H, W)
                    eq = e[qy, qx]
                    if dx == 0 and dy == 0:
                        w = np.ones((H, W), F)
                    else:
                        valid = valid & ~through[qy, qx]
                        wl = np.exp(-(np.abs(lp - lp[qy, qx]) / lden))
                        w = geom(qy, qx) * wl
                    hw = F(HK[dy + 2] * HK[dx + 2]) * w
                    hw = np.where(valid, hw, F(0)).astype(F)
                    wsum = wsum + hw
                    acc = acc + np.where(valid[..., None], hw[..., None] * eq, F(0)).astype(F)
                    sv = sv + np.where(valid, (hw * hw) * v[qy, qx], F(0)).astype(F)
            e = np.where(through[..., None], e, acc / wsum[..., None]).astype(F)
            v = np.where(through, F(0), sv / (wsum * wsum)).astype(F)
        out = (e * m) * sp if p["demodulate"] else e * sp
    assert out.dtype == F and v.dtype == F
    return np.where(through[..., None], accum, out).astype(F), v


def moments_of(samples):
    """(H, W, 2) float32 moments of (S, H, W, 3) float32 per-sample radiance,
    as rt_render_moments forms them: fp64, in sample order."""
    m1 = np.zeros(samples.shape[1:3], np.float64)
    m2 = np.zeros(samples.shape[1:3], np.float64)
    for L in samples.astype(np.float64):
        y = (0.2126 * L[..., 0] + 0.7152 * L[..., 1]) + 0.0722 * L[..., 2]
        m1 = m1 + y
        m2 = m2 + y * y
    return np.stack([m1, m2], axis=-1).astype(F)


def synthetic_moments(accum, spp, seed):
    """Moments consistent with `accum`: spp per-pixel samples that sum to it
    (random positive shares of each pixel's sum), and their moments."""
    rng = np.random.default_rng(seed)
    h, w = accum.shape[:2]
    share = rng.random((spp, h, w, 1)) + 0.05
    share = share / share.sum(axis=0, keepdims=True)
    samples = (share * accum.astype(np.float64)[None]).astype(F)
    return moments_of(samples)


def firefly(w, h, spp=4, seed=7):
    """A flat lit wall at `spp` samples with constant features and mild
    noise; at the centre pixel one sample is 1000 times the others.  Returns
    accum, feat, moments and the firefly's (y, x)."""
    rng = np.random.default_rng(seed)
    samples = (F(0.4) * (F(1.0) + F(0.05) * rng.standard_normal((spp, h, w, 1)))).astype(F) * np.ones(3, F)
    fy, fx = h // 2, w // 2
    samples[0, fy, fx] = samples[1, fy, fx] * F(1000.0)
    accum = samples.astype(np.float64).sum(axis=0).astype(F)
    feat = np.zeros((h, w, 8), F)
    feat[..., 0:3] = F(0.5) * spp
    feat[..., 5] = spp
    feat[..., 6] = F(3.0) * spp
    feat[..., 7] = spp
    return np.ascontiguousarray(accum), feat, moments_of(samples), (fy, fx)
