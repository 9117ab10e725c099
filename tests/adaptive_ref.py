"""numpy restatement of rt_render_adaptive (include/rtgpu.h): the selection in
float32 with adaptive.hip's operations in their order, the rounds over
per-sample frames with the render's own fp64 sums, and rt_normalize_samples.
Also the synthetic selection inputs the host-emulation and GPU tests share."""
import numpy as np

F = np.float32
DEFAULTS = dict(min_spp=16, step_spp=16, neighbourhood=1, rel_error=0.05, lum_floor=0.01)


def _params(overrides):
    unknown = set(overrides) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown adaptive parameter(s) {sorted(unknown)}")
    return dict(DEFAULTS, **overrides)


def unconverged(m1, m2, n, rel_error, lum_floor):
    """var > tol * tol per pixel, float32 throughout:
    nf = float(n), mu = m1 / nf, var = max(0, m2 / nf - mu * mu) / (nf - 1),
    tol = rel_error * max(mu, lum_floor).  (n = 0 or 1 give what IEEE gives;
    the callers mask n = 0.)"""
    m1, m2 = np.asarray(m1, F), np.asarray(m2, F)
    with np.errstate(all="ignore"):
        nf = np.asarray(n).astype(F)
        mu = m1 / nf
        r = m2 / nf - mu * mu
        var = np.where(r > F(0), r, F(0)).astype(F) / (nf - F(1))
        tol = F(rel_error) * np.where(mu > F(lum_floor), mu, F(lum_floor)).astype(F)
        assert mu.dtype == F and var.dtype == F and tol.dtype == F
        return var > tol * tol


def active_mask(counts, max_spp, cur=0):
    a = (counts != 0) & (counts < max_spp)
    return a & (counts == cur) if cur else a


def dilate3(mask):
    """3x3 dilation; pixels outside the image count as False."""
    h, w = mask.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = mask
    out = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def select_mask(moments, counts, max_spp, cur=0, **params):
    p = _params(params)
    act = active_mask(counts, max_spp, cur)
    unc = act & unconverged(moments[..., 0], moments[..., 1], counts, p["rel_error"], p["lum_floor"])
    return act & dilate3(unc) if p["neighbourhood"] else unc


def select(moments, counts, max_spp, cur=0, **params):
    """Ascending ids (y * W + x) of the pixels that stay active."""
    return np.flatnonzero(select_mask(moments, counts, max_spp, cur, **params)).astype(np.uint32)


def _sum_frames(frames):
    s = np.zeros(frames[0].shape, np.float64)
    for f in frames:
        s = s + f.astype(np.float64)
    return s


def _sum_moments(frames):
    """tests/test_gpu_moments.py's moments_of arithmetic: per sample
    Y = (0.2126 x + 0.7152 y) + 0.0722 z, m1 += Y, m2 += Y * Y, in fp64."""
    m1 = np.zeros(frames[0].shape[:2], np.float64)
    m2 = np.zeros(frames[0].shape[:2], np.float64)
    for f in frames:
        L = f.astype(np.float64)
        y = (0.2126 * L[..., 0] + 0.7152 * L[..., 1]) + 0.0722 * L[..., 2]
        m1 = m1 + y
        m2 = m2 + y * y
    return np.stack([m1, m2], axis=-1)


def run(per_sample_frames, listed_mask, max_spp, params=None, detail=False):
    """The rounds over per-sample frames f_s (spp = 1, sample_offset = s).
    Returns accum (H, W, 3), moments (H, W, 2), counts (H, W) uint32, rounds;
    with detail=True also a dict: samples, pixels_at_max, and `history`, per
    selection (n, moments before it, the mask it kept)."""
    p = _params(params or {})
    fr = per_sample_frames
    h, w = fr[0].shape[:2]
    accum, mom = np.zeros((h, w, 3), F), np.zeros((h, w, 2), F)
    counts = np.zeros((h, w), np.uint32)
    n = min(p["min_spp"], max_spp)
    act = np.asarray(listed_mask, bool).copy()
    accum[act] = _sum_frames(fr[:n]).astype(F)[act]          # overwriting: float(fp64 sum)
    mom[act] = _sum_moments(fr[:n]).astype(F)[act]
    counts[act] = n
    rounds, samples, history = 1, int(act.sum()) * n, []
    while n < max_spp:
        keep = select_mask(mom, counts, max_spp, cur=n, **p)
        history.append((n, mom.copy(), keep.copy()))
        if not keep.any():
            act = keep
            break
        step = min(p["step_spp"], max_spp - n)
        # accumulating: float(double(previous) + fp64 sum of the round's samples)
        accum[keep] = (_sum_frames(fr[n:n + step]) + accum.astype(np.float64)).astype(F)[keep]
        mom[keep] = (_sum_moments(fr[n:n + step]) + mom.astype(np.float64)).astype(F)[keep]
        counts[keep] = n + step
        samples += int(keep.sum()) * step
        n += step
        rounds += 1
        act = keep
    if not detail:
        return accum, mom, counts, rounds
    return accum, mom, counts, rounds, dict(samples=samples, pixels_at_max=int(act.sum()) if n >= max_spp else 0,
                                            history=history)


def borderline(history, listed_mask, max_spp, params=None):
    """Pixels whose decision at some round flips when either moment moves by
    one float32 step."""
    p = _params(params or {})
    out = np.zeros(np.asarray(listed_mask).shape, bool)
    for n, mom, _ in history:
        m1, m2 = mom[..., 0], mom[..., 1]
        base = unconverged(m1, m2, np.full(m1.shape, n), p["rel_error"], p["lum_floor"])
        for a, b in ((np.nextafter(m1, F(np.inf)), m2), (np.nextafter(m1, F(-np.inf)), m2),
                     (m1, np.nextafter(m2, F(np.inf))), (m1, np.nextafter(m2, F(-np.inf)))):
            out |= unconverged(a, b, np.full(m1.shape, n), p["rel_error"], p["lum_floor"]) != base
    return out & np.asarray(listed_mask, bool)


def normalize(sums, counts, target_spp):
    """(sums / float(counts)) * float(target_spp) in float32; counts == 0 copies the bits."""
    sums = np.asarray(sums, F)
    c = counts.reshape(counts.shape + (1,) * (sums.ndim - counts.ndim))
    with np.errstate(all="ignore"):
        out = ((sums / c.astype(F)) * F(target_spp)).astype(F)
    zero = np.broadcast_to(c == 0, sums.shape)
    out.view(np.uint32)[zero] = sums.view(np.uint32)[zero]
    return out


# ---- synthetic selection inputs

PATTERNS = ("none", "all", "last", "first", "third", "corner", "edge", "interior", "mixed")
PATTERN_MAX_SPP = 64


def pattern(name, w, h, seed=0):
    """(moments (h, w, 2), counts (h, w) uint32) at PATTERN_MAX_SPP.  A pixel
    with n samples of luminance 1 has m1 = m2 = n (variance 0: converged at
    any tolerance); one with half its samples 0 and half 2 has m1 = n, m2 = 2n
    (variance 1 / (n - 1) of the mean against a tolerance of 0.05^2).  "mixed"
    also has pixels outside the call (counts 0), finished ones (counts =
    max_spp) and differing counts beside the unconverged ones."""
    n = 8
    unc = np.zeros((h, w), bool)
    counts = np.full((h, w), n, np.uint32)
    if name == "all":
        unc[:] = True
    elif name == "last":
        unc[-1, -1] = True
    elif name == "first":
        unc[0, 0] = True
    elif name == "third":
        unc.reshape(-1)[::3] = True
    elif name == "corner":
        unc[h - 1, 0] = True
    elif name == "edge":
        unc[h // 2, w - 1] = True
    elif name == "interior":
        unc[h // 2, w // 2] = True
    elif name == "mixed":
        rng = np.random.default_rng(1000 + seed + 7 * w + h)
        unc = rng.random((h, w)) < 0.3
        counts = rng.integers(2, 12, (h, w)).astype(np.uint32)
        kind = rng.random((h, w))
        counts[kind < 0.2] = 0
        counts[kind > 0.8] = PATTERN_MAX_SPP
    elif name != "none":
        raise ValueError(name)
    nf = counts.astype(F)
    mom = np.stack([nf, np.where(unc, F(2) * nf, nf)], axis=-1).astype(F)
    if name == "mixed":   # and values near the tolerance, where every operation matters
        rng = np.random.default_rng(2000 + seed + w)
        near = rng.random((h, w)) < 0.3
        mom[..., 1] = np.where(near, nf * F(1.0) + nf * (nf - F(1)) * F(0.0025) * rng.uniform(0.9, 1.1, (h, w)).astype(F),
                               mom[..., 1]).astype(F)
    return mom, counts
