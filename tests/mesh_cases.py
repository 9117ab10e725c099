"""Seeded meshes for the device BVH build's tests (tests/test_device_build_host.py,
tests/test_gpu_device_build.py): the shapes at which an LBVH goes wrong.

  grid        height field, two triangles per cell: the baseline; n around the
              launch geometry (16 = the smallest mesh flatten hands to the
              device builder, 17, 255, 256, 257, 1000)
  coincident  64 nested triangles whose boxes share one centre exactly (every
              coordinate a dyadic fraction): all Morton codes equal, so the
              radix tree splits on the positions alone
  planar      200 triangles in z = const: one flat frame axis
  collinear   100 triangles in z = const with one common y range: centroids on
              a line; with `flat=True` the boxes are also flat in y (emulation
              only: such triangles have no area), two flat frame axes
  skewed      1000 triangles at distance 2^(-i/40) from the origin, i < 1000,
              spread over a cone about (1, 1, 1) and sized with their
              distance: a deep radix chain and a large need4; from the origin
              every triangle subtends the same angle
  outlier     299 triangles inside one Morton cell and one more triangle
              1000 cell widths away: a long run of equal codes beside a
              distinct one, and the clamp at 1023
  duplicate   64 triangles, each present twice (the copy has another
              material): the tie rule on the carried ranks (the copy, of
              the higher DFS rank, is the hit)
  large       a grid with jittered vertices, about 20 000 triangles on the
              GPU and 4 000 in the host emulation

A mesh is `Mesh(tris (n, 3, 3) float64, mats (n,) material slot 0 / 1, cams)`,
z up.  `cams` are the views (mesh coordinates) that, together with front(),
side() and top(), let every triangle be some ray's first hit where the case
allows it.  `boxes64` is Builder.triangle()'s box (with its pad of flat axes),
`boxes32` flatten's outward rounding of it to the fp32 boxes the builder gets.
"""
from collections import namedtuple

import numpy as np

Mesh = namedtuple("Mesh", "tris mats cams")
View = namedtuple("View", "origin target up half res")   # half: half-width of the image at distance 1


def view_rays(v):
    """(origin, pixel00, du, dv) of a pinhole with square pixels."""
    o, t, up = (np.asarray(a, float) for a in (v.origin, v.target, v.up))
    # the image plane passes through the target, so the pixel grid keeps its
    # precision in fp32 whatever the scene's scale
    dist = np.linalg.norm(t - o)
    f = (t - o) / dist
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    half = v.half * dist
    step = 2.0 * half / v.res
    du, dv = r * step, -u * step
    p00 = t - r * half + u * half + 0.5 * (du + dv)
    return o, p00, du, dv


def front(lo, hi):
    c, e = 0.5 * (lo + hi), float(np.max(hi - lo))
    return View(c + np.array([0.1 * e, -2.5 * e, 0.8 * e]), c, (0, 0, 1), 0.33, 96)


def side(lo, hi):
    c, e = 0.5 * (lo + hi), float(np.max(hi - lo))
    return View(c + np.array([2.5 * e, 0.15 * e, 0.6 * e]), c, (0, 0, 1), 0.33, 96)


def top(lo, hi, res=96):
    c, e = 0.5 * (lo + hi), float(np.max(hi[:2] - lo[:2]))
    return View(c + np.array([0.0, 0.0, 4.0 * e]), c, (0, 1, 0), 0.53 / 4.0, res)


def top_tiles(lo, hi, k, res=96):
    """k x k views straight down, each over one tile (plus a margin) of the xy extent."""
    e = (hi[:2] - lo[:2]) / k
    h = 5.0 * float(np.max(hi - lo))
    out = []
    for j in range(k):
        for i in range(k):
            c = np.array([lo[0] + (i + 0.5) * e[0], lo[1] + (j + 0.5) * e[1], 0.5 * (lo[2] + hi[2])])
            out.append(View(c + np.array([0.0, 0.0, h]), c, (0, 1, 0), 0.56 * float(np.max(e)) / h, res))
    return out


def bounds(tris):
    return tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)


def _grid(n, seed, jitter=0.0):
    rng = np.random.default_rng(seed)
    cells = (n + 1) // 2
    cols = int(np.ceil(np.sqrt(cells)))
    rows = (cells + cols - 1) // cols
    x = 0.25 + np.arange(cols + 1) / cols
    y = 0.25 + np.arange(rows + 1) / cols
    X, Y = np.meshgrid(x, y)
    if jitter:
        X[1:-1, 1:-1] += (rng.random((rows - 1, cols - 1)) - 0.5) * 2 * jitter / cols
        Y[1:-1, 1:-1] += (rng.random((rows - 1, cols - 1)) - 0.5) * 2 * jitter / cols
    Z = 0.5 + 0.12 * np.sin(3.0 * X) * np.cos(2.0 * Y) + (rng.random(X.shape) - 0.5) * 0.2 / cols
    P = np.stack([X, Y, Z], -1)
    tris = []
    for c in range(cells):
        j, i = divmod(c, cols)
        tris.append([P[j, i], P[j, i + 1], P[j + 1, i + 1]])
        tris.append([P[j, i], P[j + 1, i + 1], P[j + 1, i]])
    return np.array(tris[:n])


def grid(n, seed=1):
    t = _grid(n, seed)
    return Mesh(t, np.zeros(n, int), [])


def large(n=20000, seed=7, tiles=6):
    t = _grid(n, seed, jitter=0.25)
    return Mesh(t, np.zeros(n, int), top_tiles(*bounds(t), tiles))


def planar(n=200, seed=2):
    t = _grid(n, seed, jitter=0.3)
    t[:, :, 2] = 0.5
    return Mesh(t, np.zeros(n, int), [])


def collinear(n=100, flat=False):
    w = 1.0 / n
    x = 0.25 + np.arange(n) * w
    t = np.zeros((n, 3, 3))
    t[:, 0] = np.stack([x, np.full(n, 0.5), np.full(n, 0.5)], -1)
    t[:, 1] = np.stack([x + 0.9 * w, np.full(n, 0.5), np.full(n, 0.5)], -1)
    t[:, 2] = np.stack([x + 0.45 * w, np.full(n, 0.5 if flat else 0.6), np.full(n, 0.5)], -1)
    cams = [View([0.25 + (q + 0.5) * 0.25, 0.55, 3.0], [0.25 + (q + 0.5) * 0.25, 0.55, 0.5], (0, 1, 0), 0.054, 96)
            for q in range(4)]
    return Mesh(t, np.zeros(n, int), cams)


def coincident(n=64):
    """Triangle k: half-width r = (k + 1) / 128 about (0.75, 0.75), z box
    0.5 -+ (k + 2)^2 / 32768: every box centre is (0.75, 0.75, 0.5) exactly in
    fp32, and the frame maps it to 512.0 exactly on each axis."""
    t = np.zeros((n, 3, 3))
    for k in range(n):
        r, d = (k + 1) / 128.0, (k + 2) ** 2 / 32768.0
        t[k] = [[0.75 - r, 0.75 - r, 0.5 - d], [0.75 + r, 0.75 - r, 0.5 - d], [0.75, 0.75 + r, 0.5 + d]]
    return Mesh(t, np.zeros(n, int), [])


# The reference's triangle test drops a triangle whose determinant is below 1e-8, edges under about 1e-4:
# the skewed mesh starts far enough out (and the outlier's board is coarse enough) for its smallest to be seen.
SKEW_L = 2.0 ** 20


def skewed(n=1000, seed=3):
    rng = np.random.default_rng(seed)
    f = np.ones(3) / np.sqrt(3.0)
    u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    v = np.cross(f, u)
    side_cells, span = 32, 0.36
    cell = 2.0 * span / side_cells
    where = rng.permutation(side_cells * side_cells)[:n]
    t = np.zeros((n, 3, 3))
    for i in range(n):
        a = -span + (where[i] % side_cells + 0.5) * cell
        b = -span + (where[i] // side_cells + 0.5) * cell
        rho, s = SKEW_L * 2.0 ** (-i / 40.0), 0.42 * cell
        # vertices on the plane at distance 1 along f, then scaled: the same angles for every i
        t[i] = [rho * (f + (a - s) * u + (b - s) * v), rho * (f + (a + s) * u + (b - s) * v),
                rho * (f + a * u + (b + s) * v)]
    cams = [View([0.0, 0.0, 0.0], f + qa * u + qb * v, tuple(v), 0.5 * span + 0.01, 96)
            for qa in (-0.5 * span, 0.5 * span) for qb in (-0.5 * span, 0.5 * span)]
    return Mesh(t, np.zeros(n, int), cams)


def outlier(n=300, seed=4):
    """A 17 x 18 board of small triangles within 0.85 W of the frame's low
    corner (256 on every axis, W = 1) and one triangle of width 0.8 W whose
    box centre is 1000 W from that corner on every axis: the frame is 1000.4 W
    wide, so the board lies in cell 0 and the far triangle's centre beyond
    cell 1023."""
    rng = np.random.default_rng(seed)
    W, m, o = 1.0, n - 1, 256.0
    cols = 17
    pitch = 0.7 * W / 18.0
    t = np.zeros((n, 3, 3))
    for i in range(m):
        j, c = divmod(i, cols)
        p = np.array([o + 0.15 * W + c * pitch, o + 0.15 * W + j * pitch, o + 0.3 * W + 0.2 * W * rng.random()])
        t[i] = [p, p + [0.8 * pitch, 0.0, 0.02 * W], p + [0.4 * pitch, 0.8 * pitch, 0.04 * W]]
    t[0, 0] = [o, o, o]   # pins the frame's low corner
    c, r = o + 1000.0 * W, 0.4 * W
    t[m] = [[c - r, c - r, c - r], [c + r, c - r, c], [c, c + r, c + r]]
    b = o + 0.495 * W
    cams = [View([b, b, o + 4.5 * W], [b, b, o + 0.5 * W], (0, 1, 0), 0.38 / 4.0, 96),
            View([c, c, c + 4.0 * W], [c, c, c], (0, 1, 0), 0.6 / 4.0, 32)]
    return Mesh(t, np.zeros(n, int), cams)


def duplicate(n=128, seed=5):
    h = _grid(n // 2, seed, jitter=0.2)
    t = np.concatenate([h, h])   # the copies come after every original in the caller's order
    return Mesh(t, np.concatenate([np.zeros(n // 2, int), np.ones(n // 2, int)]), [])


def boxes64(tris, pad=True):
    """(n, 6) lo x, hi x, lo y, hi y, lo z, hi z, as Builder.triangle() states
    them; pad=False leaves a flat axis flat (boxes fed straight to the emulation)."""
    lo, hi = tris.min(axis=1), tris.max(axis=1)
    if pad:
        flat = hi - lo < 1e-4
        lo, hi = np.where(flat, lo - 1e-4, lo), np.where(flat, hi + 1e-4, hi)
    b = np.empty((len(tris), 6))
    b[:, 0::2], b[:, 1::2] = lo, hi
    return b


def boxes32(b64):
    """fp32 boxes rounded outward (flatten's store_box): lo (n, 3), hi (n, 3),
    and the frame, the union's corners."""
    lo, hi = b64[:, 0::2], b64[:, 1::2]
    l32, h32 = lo.astype(np.float32), hi.astype(np.float32)
    l32 = np.where(l32.astype(np.float64) > lo, np.nextafter(l32, np.float32(-np.inf)), l32)
    h32 = np.where(h32.astype(np.float64) < hi, np.nextafter(h32, np.float32(np.inf)), h32)
    return l32, h32, l32.min(axis=0), h32.max(axis=0)
