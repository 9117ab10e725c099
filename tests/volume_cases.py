"""Volume.Hit (volume.go:34-79) across boundary kinds, placements and
fallbacks: hand-built scenes for tests/test_volume_host.py (the kernels
compiled for the host) and tests/test_gpu_volumes.py (the GPU).

Three device functions implement Volume.Hit.  volume_hit_rec (a lifted volume's
DVolRec record: at most 6 quads, each through one of six axis-aligned forms or
the general quad_t, the wrapper chain field by field), and volume_hit's two
branches for volumes left in the world BVH: the cached one (at most 6
primitives of any kind) and the two-pass loop (more).  The flattener picks
between them by a chain of conditions (flatten.cpp flatten_scene,
build_vol_recs; api.cpp's shading variant); every row below is there for one
link of that chain, and declares where its volumes must end up (`lifted`) and
which k_shade variant must shade it (`shade`), for tests/test_volume_host.py
to hold the flattener to.

Every case shares one frame: a Lambertian back wall (z = -4) and floor
(y = -5), one quad light above (listed in `lights`, so the NEE shadow rays of
wall, floor and medium cross the medium), a 48 x 32 pinhole camera at
(0, 0, 6) looking down -z with max_depth 5, and a medium around the origin
whose density makes about half of the rays that cross it scatter
(rho * L ~ 0.7).  The camera never sees the floor directly (no wall / floor
edge among the camera rays).

Closed forms (expected()): for `sphere`, `box_uv`, `inside` and `leaf2` the
bounce-0 result in numpy float64 from volume.go alone: t1, t2 from the
quadratic or the slabs, U from kat_cases.rnd (the larger of the two draws for
`leaf2`: BVHNode{leaf, leaf} calls Hit twice and the closer of the two
independent free flights wins), the volume at t1 - ln U / (rho |d|) when that
lies inside, else the back wall.  A pixel is compared only where float64
decides with a margin: |hd - dist| > 1e-4 dist, and for the sphere an impact
parameter outside (1 +- 1e-3) r; at most MAX_EXCLUDED of a case's pixels may
be left out (asserted on the closed form alone, tests/test_volume_host.py).
The rays are the camera rays in fp32 (the fp32 oracle's bounce-0 record, which
the device's get_ray matches bit for bit): an input, like the scene.
"""
import math

import numpy as np

from tests.kat_cases import DOM_VOL, rnd
from tests.scene_builder import Builder, pinhole

SEED, SAMPLE = 41, 0
W, H = 48, 32
CAM_O = np.array([0.0, 0.0, 6.0])
PIX = 0.015                                   # image plane z = 5: x in [-0.36, 0.36], y in [-0.24, 0.24]
WALL_Z, FLOOR_Y = -4.0, -5.0
TMIN = 0.001                                  # camera.go:449: world.Hit(r, Interval{0.001, inf})
MAX_EXCLUDED = 0.02
SHADE_LEAN, SHADE_MAT, SHADE_FULL, SHADE_VOL = 0, 1, 2, 3     # dev_layout.h
AXIS_CODES = {0x80, 0x81, 0x82, 0x84, 0x85, 0x86}             # flatten.cpp quad_axis_code
HALF = 1.5                                    # the box medium [-HALF, HALF]^3, the sphere's radius
INSIDE_LO, INSIDE_HI = (-1.5, -1.5, 4.0), (1.5, 1.5, 7.0)    # `inside`: the box around the camera


def rho_for(length):
    return 0.7 / length


class Case:
    """name, Builder, desc, camera; vols: the volumes' hittable ids; lifted:
    whether RT_VOLUMES_LIFTED lifts them; shade: the k_shade variant when
    lifted / when in the BVH; analytic: the closed form's kind or None."""

    def __init__(self, name, b, root, vols, lifted, shade_in_bvh=SHADE_MAT, analytic=None, rho=None, wall=None):
        self.name, self.b, self.vols, self.lifted = name, b, vols, lifted
        self.shade = {True: SHADE_VOL if lifted else shade_in_bvh, False: shade_in_bvh}   # by "lift asked for"
        self.analytic, self.rho, self.wall = analytic, rho, wall
        self.desc = b.desc(root)
        self.cam = camera(b.g)

    def placements(self):
        """The volume placements worth running: lifted only where lifting happens."""
        return ["lifted", "in_bvh"] if self.lifted else ["in_bvh"]


def camera(g):
    p00 = (-0.5 * W * PIX + 0.5 * PIX, 0.5 * H * PIX - 0.5 * PIX, CAM_O[2] - 1.0)
    return pinhole(g, W, H, tuple(CAM_O), p00, (PIX, 0, 0), (0, -PIX, 0), max_depth=5)


def frame(b, lights=1):
    """Back wall, floor and `lights` quad lights (all listed); returns the
    world's items and the wall's id."""
    wall = b.quad((-12, -12, WALL_Z), (24, 0, 0), (0, 24, 0), b.lambertian((0.73, 0.73, 0.73)))
    floor = b.quad((-12, FLOOR_Y, -4), (24, 0, 0), (0, 0, 16), b.lambertian((0.2, 0.5, 0.3)))
    lm = b.light((15, 15, 15))
    if lights == 1:
        ls = [b.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2), lm)]
    else:       # a row of small lights at y = 5
        ls = [b.quad((-4.25 + 0.5 * i, 5, -0.2), (0.4, 0, 0), (0, 0, 0.4), lm) for i in range(lights)]
    b.lights = list(ls)
    return [wall, floor] + ls, wall


def medium(b, boundary, rho):
    return b.volume(boundary, rho, b.mat(b.g.RT_ISOTROPIC, b.solid((0.9, 0.9, 0.9))))


def _box_case(g, name, swap=False, lifted=True, shade_in_bvh=SHADE_MAT, extra=None, lights=1, analytic=None):
    b = Builder(g)
    items, wall = frame(b, lights)
    bm = b.lambertian((0.5, 0.5, 0.5))
    rho = rho_for(2 * HALF)
    vol = medium(b, b.listing(b.box_quads((-HALF,) * 3, (HALF,) * 3, bm, swap)), rho)
    if extra:
        items = items + extra(b)
    return Case(name, b, b.listing(items + [vol]), [vol], lifted, shade_in_bvh, analytic, rho, wall)


def _single(g, name, make_boundary, length, lifted, analytic=None):
    b = Builder(g)
    items, wall = frame(b)
    rho = rho_for(length)
    vol = medium(b, make_boundary(b, b.lambertian((0.5, 0.5, 0.5))), rho)
    return Case(name, b, b.listing(items + [vol]), [vol], lifted, SHADE_MAT, analytic, rho, wall)


def _sheared(b, m):
    e = [np.array(x) for x in ((3.0, 0.0, 0.6), (0.5, 3.0, 0.0), (0.0, 0.7, 3.0))]
    p0 = -(e[0] + e[1] + e[2]) / 2
    faces = []
    for k in range(3):
        u, v, w = e[k], e[(k + 1) % 3], e[(k + 2) % 3]
        faces += [b.quad(p0, u, v, m), b.quad(p0 + w, u, v, m)]
    return b.listing(faces)


def _box_srt(b, m):
    inner = b.listing(b.box_quads((-1, -1, -1), (1, 1, 1), m))
    return b.translate(b.rotate_y(b.scale(inner, (1.5, 1.0, 0.75)), 0.6, 0.8), (0.2, 0.0, 0.0))


def _mixed(b, m):
    # the sphere's front, the cutting quad z = 0 behind it, a large triangle at z = -2.5 behind both
    return b.listing([b.sphere((0, 0, 0), HALF, m), b.quad((-2.5, -2, 0), (5, 0, 0), (0, 4, 0), m),
                      b.triangle((-6, -4, -2.5), (6, -4, -2.5), (0, 8, -2.5), m)])


def _tetra(b, m):
    p = [np.array(x, float) * 1.6 for x in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    return b.listing([b.triangle(p[i], p[j], p[k], m) for i, j, k in ((0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2))])


def _octa(b, m):
    r = 2.0
    tris = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                tris.append(b.triangle((sx * r, 0, 0), (0, sy * r, 0), (0, 0, sz * r), m))
    return b.listing(tris)


def _box8(b, m):
    q = b.box_quads((-HALF,) * 3, (HALF,) * 3, m)
    front = [b.quad((-HALF + i, -HALF, HALF), (1, 0, 0), (0, 2 * HALF, 0), m) for i in range(3)]   # +z in three strips
    return b.listing(q[:5] + front)


def _tube(sides):
    """A tube of `sides` quads around the z axis (circumradius 1.2, z in
    [-1.5, 1.5]) closed by two circles of that radius: the camera looks
    straight at a cap."""
    def make(b, m):
        r = 1.2
        ang = [2 * math.pi * (i + 0.5) / sides for i in range(sides + 1)]
        pts = [np.array([r * math.cos(a), r * math.sin(a), -HALF]) for a in ang]
        quads = [b.quad(pts[i], pts[i + 1] - pts[i], (0, 0, 2 * HALF), m) for i in range(sides)]
        return b.listing([b.circle((0, 0, HALF), (0, 0, 1), r, m)] + quads + [b.circle((0, 0, -HALF), (0, 0, 1), r, m)])
    return make


def _many(g, name, n, lifted):
    b = Builder(g)
    items, wall = frame(b)
    bm = b.lambertian((0.5, 0.5, 0.5))
    rho = rho_for(0.8)
    vols = []
    for i in range(n):
        c = np.array([-1.2 + 1.2 * (i % 3), -1.2 + 1.2 * (i // 3), 0.0])
        vols.append(medium(b, b.listing(b.box_quads(c - 0.4, c + 0.4, bm)), rho))
    return Case(name, b, b.listing(items + vols), vols, lifted, SHADE_MAT, None, rho, wall)


def _inside(g):
    b = Builder(g)
    items, wall = frame(b)
    rho = rho_for(2.0)
    vol = medium(b, b.listing(b.box_quads(INSIDE_LO, INSIDE_HI, b.lambertian((0.5, 0.5, 0.5)))), rho)
    return Case("inside", b, b.listing(items + [vol]), [vol], True, SHADE_MAT, "inside", rho, wall)


def _leaf2(g):
    b = Builder(g)
    items, wall = frame(b)
    rho = rho_for(2 * HALF)
    vol = medium(b, b.listing(b.box_quads((-HALF,) * 3, (HALF,) * 3, b.lambertian((0.5, 0.5, 0.5)))), rho)
    root = b.bvh_node(b.leaf_node([vol]), b.listing(items, g.RT_BVH_LEAF))
    return Case("leaf2", b, root, [vol], True, SHADE_MAT, "leaf2", rho, wall)


def _image_wall(b):
    tex = b.image_texture(2, 2, [[[0.9, 0.1, 0.1], [0.1, 0.9, 0.1]], [[0.1, 0.1, 0.9], [0.8, 0.8, 0.2]]])
    return [b.quad((3, -2, -3.5), (0, 0, 5), (0, 4, 0), b.mat(b.g.RT_LAMBERTIAN, tex))]


def _a_circle(b):
    return [b.circle((-3.0, -1.0, -1.0), (1, 0.2, 0.5), 1.25, b.lambertian((0.3, 0.3, 0.8)))]


def _pad(b):
    b.pad_tables(385)
    return []


BUILDERS = {
    "box_uv": lambda g: _box_case(g, "box_uv", analytic="box"),
    "box_vu": lambda g: _box_case(g, "box_vu", swap=True),
    "sheared": lambda g: _single(g, "sheared", _sheared, 3.0, True),
    "box_srt": lambda g: _single(g, "box_srt", _box_srt, 2.0, True),
    "inside": _inside,
    "leaf2": _leaf2,
    "sphere": lambda g: _single(g, "sphere", lambda b, m: b.listing([b.sphere((0, 0, 0), HALF, m)]), 2 * HALF, False,
                                "sphere"),
    "moving_sphere": lambda g: _single(g, "moving_sphere",
                                       lambda b, m: b.listing([b.sphere((-0.3, 0, 0), HALF, m, vel=(0.6, 0.25, 0))]),
                                       2 * HALF, False),
    "mixed": lambda g: _single(g, "mixed", _mixed, 2.0, False),
    "tetra": lambda g: _single(g, "tetra", _tetra, 2.0, False),
    "octa": lambda g: _single(g, "octa", _octa, 2.5, False),
    "box8": lambda g: _single(g, "box8", _box8, 2 * HALF, False),
    "vol8": lambda g: _many(g, "vol8", 8, True),
    "vol9": lambda g: _many(g, "vol9", 9, False),
    "with_image": lambda g: _box_case(g, "with_image", lifted=False, shade_in_bvh=SHADE_FULL, extra=_image_wall),
    "with_circle": lambda g: _box_case(g, "with_circle", lifted=False, extra=_a_circle),
    "big_tables": lambda g: _box_case(g, "big_tables", lifted=False, shade_in_bvh=SHADE_FULL, extra=_pad),
    "lights17": lambda g: _box_case(g, "lights17", lifted=False, shade_in_bvh=SHADE_FULL, lights=17),
    "disc_capped": lambda g: _single(g, "disc_capped", _tube(4), 2 * HALF, False),    # 6 primitives: the cached branch
    "disc_capped8": lambda g: _single(g, "disc_capped8", _tube(6), 2 * HALF, False),  # 8: the two-pass loop
}
NAMES = list(BUILDERS)
ANALYTIC = ["sphere", "box_uv", "inside", "leaf2"]
# t against the closed form: test_gpu_kat's rtol 2e-6.  The fp32 oracle's own
# worst relative error against the closed form over the compared pixels,
# measured on the CPU (tests/test_volume_host.py prints it): box_uv and leaf2
# 8.1e-8, inside 2.1e-7, sphere 6.5e-7.  The sphere's cancellation in
# h * h - a * cc (|o| = 6, r = 1.5) stays under 2e-6, so the curved boundary
# takes no wider tolerance than the flat ones (4 x 6.5e-7 would be 2.6e-6).
T_RTOL = {"sphere": 2e-6, "box_uv": 2e-6, "inside": 2e-6, "leaf2": 2e-6}
NODE_FORMAT_CASES =["box_uv", "sphere", "vol9"]     # also run with quant8 and wide8 nodes

_cases = {}


def case(g, name):
    """The case, built once."""
    if name not in _cases:
        _cases[name] = BUILDERS[name](g)
    return _cases[name]


# refusals (flatten must answer RT_ERR_UNSUPPORTED) -----------------------------
def refusal(g, kind):
    b = Builder(g)
    items, _ = frame(b)
    m = b.lambertian((0.5, 0.5, 0.5))
    iso = b.mat(g.RT_ISOTROPIC, b.solid((0.9, 0.9, 0.9)))
    if kind == "bvh_boundary":       # the boundary is a BVH node over two leaves
        q = b.box_quads((-HALF,) * 3, (HALF,) * 3, m)
        items.append(b.volume(b.bvh_node(b.listing(q[:3], g.RT_BVH_LEAF), b.listing(q[3:], g.RT_BVH_LEAF)), 0.2, iso))
    elif kind == "wrapped_volume":   # Translate(volume)
        vol = b.volume(b.listing(b.box_quads((-HALF,) * 3, (HALF,) * 3, m)), 0.2, iso)
        items.append(b.translate(vol, (0.5, 0, 0)))
    elif kind == "volumes_1025":
        q = b.listing(b.box_quads((-HALF,) * 3, (HALF,) * 3, m))
        items += [b.volume(q, 0.2, iso) for _ in range(1025)]
    else:
        raise KeyError(kind)
    return b, b.desc(b.listing(items))


REFUSALS = ["bvh_boundary", "wrapped_volume", "volumes_1025"]


# closed forms ------------------------------------------------------------------
_rays = {}


def camera_rays(O, c):
    """(n, 3) origins and directions of the case's bounce-0 rays, fp32 values in float64."""
    if c.name not in _rays:
        ray = O.path_records(c.desc, c.cam, SEED, SAMPLE, 1, fp32=True)[3][0]
        o, d = np.array(ray[:, 0:3]), np.array(ray[:, 3:6])
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[c.name] = (o, d)
    return _rays[c.name]


def _slabs(o, d, lo, hi):
    """Entry and exit of the line o + t d through the box (both signs of t), or None."""
    t0, t1 = -math.inf, math.inf
    for a in range(3):
        if d[a] == 0.0:
            if not lo[a] <= o[a] <= hi[a]:
                return None
            continue
        ta, tb = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return (t0, t1) if t0 <= t1 else None


def expected(c, o, d):
    """Per pixel of an analytic case, from volume.go in float64: prim (the
    volume's or the wall's id), t, and `decided` (False: the pixel is left out
    of every comparison)."""
    n = o.shape[0]
    prim, t, decided = np.zeros(n, np.int64), np.zeros(n), np.ones(n, bool)
    vol = c.vols[0]
    for p in range(n):
        op, dp = o[p], d[p]
        rl = math.sqrt(float(dp @ dp))
        t_wall = (WALL_Z - op[2]) / dp[2]
        prim[p], t[p] = c.wall, t_wall
        if c.analytic == "sphere":
            a, h, cc = float(dp @ dp), float(dp @ -op), float(op @ op) - HALF * HALF
            impact = math.sqrt(max(float(op @ op) - h * h / a, 0.0))
            if abs(impact - HALF) <= 1e-3 * HALF:
                decided[p] = False
                continue
            disc = h * h - a * cc
            if disc < 0:
                continue
            seg = ((h - math.sqrt(disc)) / a, (h + math.sqrt(disc)) / a)
        else:
            lo, hi = (INSIDE_LO, INSIDE_HI) if c.analytic == "inside" else ((-HALF,) * 3, (HALF,) * 3)
            seg = _slabs(op, dp, lo, hi)
            if seg is None:
                continue
        t1, t2 = seg
        if not t2 >= t1 + 1e-4:            # volume.go:45: the second hit from t1 + 0.0001
            decided[p] = False
            continue
        t1 = max(t1, TMIN)                 # volume.go:56-68
        if t1 >= t2:
            continue
        t1 = max(t1, 0.0)
        dist = (t2 - t1) * rl
        u = rnd(SEED, p, SAMPLE, 0, DOM_VOL, 0)
        if c.analytic == "leaf2":
            u = max(u, rnd(SEED, p, SAMPLE, 0, DOM_VOL, 1))
        hd = -math.log(u) / c.rho if u > 0 else math.inf
        if abs(hd - dist) <= 1e-4 * dist:
            decided[p] = False
            continue
        if hd <= dist:
            prim[p], t[p] = vol, t1 + hd / rl
    return prim, t, decided
