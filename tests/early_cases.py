"""Scenes for the early-miss tests (RT_OPT_EARLY_MISS: rays that miss the world
box resolved in k_shade), shared by tests/test_early_host.py and
tests/test_gpu_early_miss.py.

Every room here is a world list of at most eight quads (so all of them are
lifted out of the world BVH) and one small mesh instance, which is then all
the world BVH holds: where that instance stands decides which rays miss the
world box.
"""
import numpy as np

from tests.scene_builder import Builder, pinhole

W, H, SPP = 37, 29, 3      # counts that are no multiple of 256
R = 512.0                  # the room's edge


class Case:
    def __init__(self, name, desc, cam, keep):
        self.name, self.desc, self.cam, self.keep = name, desc, cam, keep


def _mesh(b, lo, hi, mat):
    """A two-triangle mesh under a translate whose box is [lo, hi]: a triangle
    at each end of the box's diagonal."""
    lo, hi = np.array(lo, float), np.array(hi, float)
    e = (hi - lo) * 0.25
    t0 = b.triangle(lo * 0, [e[0], 0, 0], [0, e[1], e[2]], mat)
    s = hi - lo
    t1 = b.triangle(s, s - [e[0], 0, 0], s - [0, e[1], e[2]], mat)
    return b.translate(b.bvh_node(t0, t1), list(lo))


def _look_down_camera(g, max_depth):
    """Inside the room near the ceiling's corner, looking at the floor: no
    camera ray reaches the light in the ceiling."""
    o = np.array([100.0, 400.0, 100.0])
    du, dv = np.array([240.0 / W, 0, 0]), np.array([0, 0, -240.0 / H])
    p00 = np.array([40.0, 100.0, 340.0]) + 0.5 * (du + dv)
    return pinhole(g, W, H, o, p00, du, dv, max_depth=max_depth)


def room(g, name, inst_lo, inst_hi, max_depth=3, closed=True, env=None, lit=True, sky=False):
    """Lambertian walls (six when closed, else a floor only), a light quad
    under the ceiling (listed as a light unless `lit` is off) and the instance.
    With only Lambertian walls in view every path survives bounce 0."""
    b = Builder(g)
    white, green = b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.12, 0.45, 0.15))
    if closed:
        quads = b.box_quads((0, 0, 0), (R, R, R), white)
    else:
        quads = [b.quad((0, 0, 0), (R, 0, 0), (0, 0, R), white)]
    light = b.quad((300, R - 4, 300), (96, 0, 0), (0, 0, 96), b.light((15, 15, 15)))
    quads.append(light)
    b.lights = [light] if lit else []
    inst = _mesh(b, inst_lo, inst_hi, green)
    if env is not None:
        b.environment(env, importance=True)
    desc = b.desc(b.listing(quads + [inst]))
    cam = _look_down_camera(g, max_depth)
    cam.use_sky_gradient = 1 if sky else 0
    return Case(name, desc, cam, (b, desc))


def closed_room(g, max_depth=3):
    """The instance stands on the floor like a Cornell block."""
    return room(g, "closed-room", (180, 0, 200), (300, 200, 300), max_depth)


def all_pass_room(g, max_depth=3):
    """The instance's box holds the whole room: no ray misses the world box."""
    return room(g, "all-pass", (-8, -8, -8), (R + 8, R + 8, R + 8), max_depth)


def all_miss_room(g, max_depth=3):
    """A small instance far below the floor: every scattered ray and every
    light sample of this seed misses the world box."""
    return room(g, "all-miss", (250, -4010, 250), (260, -4000, 260), max_depth)


def env_room(g, max_depth=4):
    """A floor, a light, an instance and an importance-sampled environment with
    one bright region: NEE jobs of two rays."""
    h, w = 8, 16
    px = np.full((h, w, 3), 0.2)
    px[1:3, 3:6] = (6.0, 5.0, 4.0)
    return room(g, "env-room", (180, 0, 200), (300, 200, 300), max_depth, closed=False, env=px)


def unlit_floor(g, max_depth=12):
    """A floor and the instance under the sky, no light listed: a deep render
    without NEE, the kind that may hand its last paths to the long-tail kernel."""
    return room(g, "unlit-floor", (180, 0, 200), (300, 200, 300), max_depth, closed=False, lit=False, sky=True)


def named(g, name, **kw):
    s = g.Scene(name, width=W, aspect=W / H, **kw)
    return Case(name, s.desc, s.camera, s)


def rim_rays(box, n, rng, any_hit):
    """n rays around the box [xmin xmax ymin ymax zmin zmax] (float32) for the
    predicate tests: (origins, directions, tmax).  A quarter each: random rays;
    rays aimed at a point of a face, edge or corner moved up to 4 ulps off it;
    rays with one or two zero direction components, from origins level with a
    face; rays from inside the box.  Any-hit rays end within 4 ulps of where
    they would enter the box, or at a random distance."""
    box = np.asarray(box, np.float32)
    lo, hi = box[0::2].astype(np.float64), box[1::2].astype(np.float64)
    size = hi - lo
    q = n // 4

    def ulps(x, k):
        x = np.asarray(x, np.float32).copy()
        for _ in range(4):
            up = np.nextafter(x, np.float32(np.inf))
            dn = np.nextafter(x, np.float32(-np.inf))
            x = np.where(k > 0, up, np.where(k < 0, dn, x))
            k = k - np.sign(k)
        return x

    def outside(m):
        side = rng.integers(0, 2, (m, 3))
        off = rng.uniform(0.05, 2.0, (m, 3)) * size
        o = np.where(side == 1, hi + off, lo - off)
        inside_axis = rng.integers(0, 3, m)          # one axis may lie within the slab
        within = lo + rng.uniform(0, 1, (m, 3)) * size
        pick = rng.uniform(size=m) < 0.5
        o[np.arange(m)[pick], inside_axis[pick]] = within[np.arange(m)[pick], inside_axis[pick]]
        return o

    # random
    o0 = lo - size + rng.uniform(0, 3, (q, 3)) * size
    d0 = rng.normal(size=(q, 3))
    # rim: a target on the box's surface, each coordinate on a face plane or within
    o1 = outside(q)
    on = rng.integers(0, 3, (q, 3))                  # 0: lo plane, 1: hi plane, 2: within
    on[np.arange(q), rng.integers(0, 3, q)] = rng.integers(0, 2, q)   # at least one on a plane
    tgt = np.where(on == 0, lo, np.where(on == 1, hi, lo + rng.uniform(0, 1, (q, 3)) * size))
    tgt = ulps(tgt.astype(np.float32), np.where(on == 2, 0, rng.integers(-4, 5, (q, 3)))).astype(np.float64)
    o1 = o1.astype(np.float32).astype(np.float64)
    d1 = tgt - o1
    # zero components, origins level with a face
    o2 = outside(q)
    lvl = rng.integers(0, 3, q)
    o2[np.arange(q), lvl] = np.where(rng.integers(0, 2, q) == 1, hi[lvl], lo[lvl])
    d2 = rng.normal(size=(q, 3))
    z = rng.integers(0, 3, q)
    d2[np.arange(q), z] = 0.0
    two = rng.uniform(size=q) < 0.4
    d2[np.arange(q)[two], (z[two] + 1) % 3] = 0.0
    neg0 = rng.uniform(size=q) < 0.3                 # some of the zeros are -0
    d2[np.arange(q)[neg0], z[neg0]] = -0.0
    # inside
    m = n - 3 * q
    o3 = lo + rng.uniform(0, 1, (m, 3)) * size
    d3 = rng.normal(size=(m, 3))
    o = np.concatenate([o0, o1, o2, o3]).astype(np.float32)
    d = np.concatenate([d0, d1, d2, d3]).astype(np.float32)
    tmax = np.full(n, np.inf, np.float32)
    if any_hit:
        tmax = rng.uniform(0.01, 4.0, n).astype(np.float32) * np.float32(np.linalg.norm(size))
        tmax /= np.maximum(np.linalg.norm(d, axis=1), np.float32(1e-6)).astype(np.float32)
        # rim rays reach their target at t = 1
        tmax[q:2 * q] = ulps(np.ones(q, np.float32), rng.integers(-4, 5, q))
        far = rng.uniform(size=n) < 0.25
        tmax[far] = np.inf
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(tmax)
