"""rt_gather's ray of one sample, restated in numpy uint32 / float32 from the
text of include/rtgpu.h ("Gathers") and DESIGN.md's RNG section, not from the
kernel: lowbias32, path_key, ctr, rnd, random_unit_vector, the three sources
and the validity rule.  Every float operation is a float32 numpy operation in
the order the header writes it, so there is no fused multiply-add and the
kernel's bits are expected exactly.

    rays(pts, source, seed, sample) -> PATH_RAY_DTYPE-shaped array
"""
import numpy as np

RAY, COSINE, SPHERE = 0, 1, 2
DOM_CAMERA, DOM_SOURCE = 0, 7
MAX_UNIT_TRIES = 64

POINT_DTYPE = np.dtype([("p", np.float32, 3), ("id", np.uint32), ("n", np.float32, 3), ("reserved", np.uint32)])
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("id", np.uint32), ("d", np.float32, 3), ("reserved", np.uint32)])

U = np.uint32
F = np.float32


def lowbias32(x):
    x = np.asarray(x, U).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U(16)
        x *= U(0x7FEB352D)
        x ^= x >> U(15)
        x *= U(0x846CA68B)
        x ^= x >> U(16)
    return x


def path_key(seed, pixel, sample):
    with np.errstate(over="ignore"):
        k = lowbias32(U(seed) ^ U(0xA511E9B3))
        k = lowbias32(k ^ np.asarray(pixel, U))
        return lowbias32(k + np.asarray(sample, U) * U(0x9E3779B9))


def ctr(bounce, dom, idx):
    return (U(bounce) << U(16)) | (U(dom) << U(12)) | np.asarray(idx, U)


def rnd(key, counter):
    h = lowbias32(np.asarray(key, U) ^ lowbias32(np.asarray(counter, U) ^ U(0x632BE5AB)))
    return (h >> U(8)).astype(F) * F(2.0 ** -24)


def random_unit_vector(key, bounce, dom, base):
    """(directions (n, 3) float32, tries (n,)): rejection in the cube, try k at
    counters base + 3k .. base + 3k + 2; accepted when 0 < |p|^2 <= 1, then
    p * (1 / sqrt(|p|^2)); (0, 0, 1) after 64 rejections."""
    key = np.atleast_1d(np.asarray(key, U))
    out = np.zeros((key.size, 3), F)
    out[:, 2] = F(1.0)
    tries = np.full(key.size, MAX_UNIT_TRIES, np.int32)
    todo = np.arange(key.size)
    for k in range(MAX_UNIT_TRIES):
        if todo.size == 0:
            break
        c = ctr(bounce, dom, base + 3 * k)
        kk = key[todo]
        x = F(-1.0) + F(2.0) * rnd(kk, c)
        y = F(-1.0) + F(2.0) * rnd(kk, c + U(1))
        z = F(-1.0) + F(2.0) * rnd(kk, c + U(2))
        l2 = (x * x + y * y) + z * z
        ok = (F(0.0) < l2) & (l2 <= F(1.0))
        inv = F(1.0) / np.sqrt(l2[ok])
        sel = todo[ok]
        out[sel, 0], out[sel, 1], out[sel, 2] = inv * x[ok], inv * y[ok], inv * z[ok]
        tries[sel] = k + 1
        todo = todo[~ok]
    return out, tries


def length(v):
    """len(): sqrt(x*x + y*y + z*z) in float32, summed left to right."""
    v = np.asarray(v, F)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def valid(pts, source):
    """The validity rule: p finite; for RAY and COSINE also n finite and len(n)
    neither 0 nor non-finite."""
    ok = np.isfinite(pts["p"]).all(axis=1)
    if source != SPHERE:
        l = length(pts["n"])
        ok &= np.isfinite(pts["n"]).all(axis=1) & (l != 0) & np.isfinite(l)
    return ok


def rays(pts, source, seed, sample):
    """The rt_path_ray sample `sample` of every point traces; an invalid point
    gives {p, id, (0, 0, 0), 0}."""
    pts = np.ascontiguousarray(pts, POINT_DTYPE)
    out = np.zeros(pts.shape[0], RAY_DTYPE)
    out["o"], out["id"] = pts["p"], pts["id"]
    ok = valid(pts, source)
    q = pts[ok]
    if q.size == 0:
        return out
    key = path_key(seed, q["id"], sample)
    if source == RAY:
        d = q["n"]
    else:
        u, _ = random_unit_vector(key, 0, DOM_SOURCE, 0)
        if source == SPHERE:
            d = u
        else:
            nh = (F(1.0) / length(q["n"]))[:, None] * q["n"]          # unit(n) = n * (1 / len(n))
            d = nh + u
            near_zero = (np.abs(d) < F(1e-8)).all(axis=1)
            d[near_zero] = nh[near_zero]
    out["d"][ok] = d
    return out
