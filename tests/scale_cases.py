"""One scene at many scales and distances from the origin, with views whose
ray origins lie up to 64 room sizes from what they hit (tests/test_scale_host.py,
tests/test_gpu_scale.py).

room(g, s, k): every coordinate is base * s + c, c = k * ROOM * s * (1, -1, 1).
The base layout is in integers (ROOM = 512 across), s is a power of two and
k is 0 or 16, so every coordinate of the scene and of every camera is exact in
fp32 at every scale: what differs between the fp32 code under test and the
fp64 oracle is the arithmetic, never the input.

The scene (a world RT_LIST; the flattener builds its own world BVH over it):
  * six flat quads: floor y = 0, left wall x = 0 and back wall z = 0 (planes
    exactly at coordinate 0 when k = 0) cover their whole side; the ceiling
    y = ROOM and the right wall x = ROOM cover z in [0, ROOM / 2], the front
    wall z = ROOM covers x in [0, ROOM / 2].  So the room is open over half of
    each of its three high sides, and a camera outside it, beyond +x, +y or
    +z, sees the outside of the half wall and, through the opening, the
    objects and the full wall opposite;
  * a light quad under the covered half of the ceiling (listed in lights);
  * in the quadrant x, z >= ROOM / 2 behind all three openings, one above the
    other and one beside the other so that no two overlap seen along any
    axis: a box of six quads under rotate_y (sin 0.6, cos 0.8) and translate;
    a 12-triangle axis-aligned cube mesh (flat triangles: every triangle's
    own box is 2e-4 thick) as a bvh_node tree under translate; the same tree
    under scale and translate; a sphere.  Nothing touches anything else (no
    ties between coplanar faces).
No box is thickened: the Builder's 1e-4 pad, as the reference's padToMinimums.

Views.  A view is a RES x RES pinhole camera whose image plane lies ON its
target, perpendicular to a coordinate axis: a window of half-size h around a
point P of a primitive.  (The image plane at the target keeps the pixel
positions, computed in fp32 at the scene's magnitude, thousands of ulps apart
at every distance.)  Why windows and not one picture of the room: the tests
pin ids on a view's interior pixels (the fp64 oracle's ids constant over the
3 x 3 neighbourhood) and require at least 75 % of every view to be interior;
at 32 x 32 a picture with four objects and the room's edges in it is mostly
silhouette and pins nothing.  A window shows one face (two triangles and their
diagonal) or one wall.  Kinds:
  * far: the camera outside the room, straight in front of P, 1, 8 and 64
    room sizes beyond the room's high side of the axis; every primitive with
    a face towards +x, +y or +z is looked at from all three distances, the
    full walls through the openings;
  * inside: the camera inside the room, 16 units from the low wall of the
    axis, in front of P: the faces towards -x, -y, -z, and the light;
  * fan: axis-parallel rays.  The camera lies IN its own image plane (pixel00
    and the camera centre share one coordinate, and both pixel steps are 0 on
    that axis), so that component of every ray direction is exactly 0, 1 / d
    is +-inf, and every slab plane on that axis is +-inf, or NaN where the
    origin lies exactly on the plane (aabb.go:59-116: neither may cull).  One
    fan runs from 8 room sizes outside through the opening to the left wall
    (plane z = 440); one from inside to the cube's -x face, in a plane y
    through the cube; one from inside to the left wall in the plane
    z = ROOM / 2, exactly the high z plane of the boxes of the ceiling and the
    right wall (NaN planes).

Every (s, k) cell is kept: the fp64 oracle resolves every view of every cell
(2e-4 is 2^13 fp64 ulps at the largest coordinate, 2^25 + 2^23 + 2^19), and
tests/test_scale_host.py asserts the interior share on its output alone.
"""
import numpy as np

from tests.scene_builder import Builder, pinhole

ROOM = 512.0
RES = 32
SCALES = [2.0 ** -6, 1.0, 2.0 ** 2, 2.0 ** 6, 2.0 ** 10]
OFFSETS = [0, 16]                       # k: c = k * ROOM * s along (1, -1, 1)
DIAG = np.array([1.0, -1.0, 1.0])
FAR = [1, 8, 64]                        # room sizes beyond the room's high side
SIN, COS = 0.6, 0.8

# object centres and half sizes (base units): distinct slots on every axis
BOX_C, BOX_H = np.array([296.0, 120.0, 408.0]), np.array([20.0, 32.0, 20.0])     # half sizes before the rotation
CUBE_C, CUBE_H = np.array([352.0, 216.0, 296.0]), np.array([24.0, 24.0, 24.0])
SCUBE_C, SCUBE_F = np.array([408.0, 312.0, 464.0]), np.array([0.5, 1.5, 1.0])   # the cube tree times SCUBE_F
SPHERE_C, SPHERE_R = np.array([464.0, 408.0, 352.0]), 32.0


def cell_id(s, k):
    return f"s2^{int(np.log2(s))}-c{k}"


class View:
    def __init__(self, name, kind, cam, origin):
        self.name, self.kind, self.cam, self.origin = name, kind, cam, origin


class Room:
    """The scene of one (s, k) cell: desc, views, and `expect`, the set of
    (top, prim) pairs the views must reach between them."""

    def __init__(self, g, s, k):
        self.g, self.s, self.k = g, float(s), k
        self.c = k * ROOM * self.s * DIAG
        b = self.b = Builder(g)
        white, red, green, blue = (b.lambertian(x) for x in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15),
                                                               (0.2, 0.3, 0.7)))
        R, H = ROOM, ROOM / 2
        W = self.W
        quad = lambda Q, u, v, m: b.quad(W(Q), self.s * np.array(u, float), self.s * np.array(v, float), m)
        self.floor = quad((0, 0, 0), (R, 0, 0), (0, 0, R), white)
        self.left = quad((0, 0, 0), (0, R, 0), (0, 0, R), red)
        self.back = quad((0, 0, 0), (R, 0, 0), (0, R, 0), white)
        self.ceiling = quad((0, R, 0), (R, 0, 0), (0, 0, H), white)
        self.right = quad((R, 0, 0), (0, R, 0), (0, 0, H), green)
        self.front = quad((0, 0, R), (H, 0, 0), (0, R, 0), white)
        self.light = quad((32, 480, 32), (128, 0, 0), (0, 0, 128), b.light((15, 15, 15)))
        b.lights = [self.light]
        self.sphere = b.sphere(W(SPHERE_C), SPHERE_R * self.s, blue)
        # the box: six quads around the object-space origin, RotateY, Translate
        h = BOX_H * self.s
        oq = lambda Q, u, v: b.quad(np.array(Q, float) * h, np.array(u, float) * h, np.array(v, float) * h, white)
        self.box_quads = {
            "+x": oq((1, -1, -1), (0, 2, 0), (0, 0, 2)), "-x": oq((-1, -1, -1), (0, 2, 0), (0, 0, 2)),
            "+y": oq((-1, 1, -1), (2, 0, 0), (0, 0, 2)), "-y": oq((-1, -1, -1), (2, 0, 0), (0, 0, 2)),
            "+z": oq((-1, -1, 1), (2, 0, 0), (0, 2, 0)), "-z": oq((-1, -1, -1), (2, 0, 0), (0, 2, 0)),
        }
        self.box = b.translate(b.rotate_y(b.listing(list(self.box_quads.values())), SIN, COS), list(W(BOX_C)))
        # the cube mesh: faces in the order +x -x +y -y +z -z, two triangles each
        ch = CUBE_H * self.s
        self.cube_tris = {}
        ids = []
        for a in range(3):
            for sg in (1.0, -1.0):
                u, v = (a + 1) % 3, (a + 2) % 3
                p = [np.zeros(3) for _ in range(4)]
                for i, (su, sv) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
                    p[i][a], p[i][u], p[i][v] = sg * ch[a], su * ch[u], sv * ch[v]
                pair = [b.triangle(p[0], p[1], p[2], blue), b.triangle(p[0], p[2], p[3], blue)]
                self.cube_tris[("+" if sg > 0 else "-") + "xyz"[a]] = pair
                ids += pair
        tree = self._tree(ids)
        self.cube = b.translate(tree, list(W(CUBE_C)))
        self.scube = b.translate(b.scale(tree, list(SCUBE_F)), list(W(SCUBE_C)))
        self.walls = [self.floor, self.ceiling, self.left, self.right, self.back, self.front]
        self.tops = self.walls + [self.light, self.sphere, self.box, self.cube, self.scube]
        self.desc = b.desc(b.listing(self.tops))
        self.expect = {(w, w) for w in self.walls} | {(self.light, self.light), (self.sphere, self.sphere)}
        self.expect |= {(self.box, q) for q in self.box_quads.values()}
        self.expect |= {(top, t) for top in (self.cube, self.scube) for t in ids}
        self.views = self._views()

    def W(self, p):
        """World coordinates of a base point."""
        return np.array(p, float) * self.s + self.c

    def _tree(self, ids):
        if len(ids) == 1:
            return ids[0]
        mid = len(ids) // 2
        return self.b.bvh_node(self._tree(ids[:mid]), self._tree(ids[mid:]))

    # cameras ------------------------------------------------------------------
    def window(self, origin, P, axis, h, res=RES):
        """Base-unit camera at `origin` whose image plane is the window of
        half-size h around P, perpendicular to `axis`."""
        u, v = (axis + 1) % 3, (axis + 2) % 3
        du, dv = np.zeros(3), np.zeros(3)
        du[u], dv[v] = 2.0 * h / res, 2.0 * h / res
        p00 = np.array(P, float).copy()
        p00[u] -= h
        p00[v] -= h
        p00 = p00 + 0.5 * (du + dv)
        return pinhole(self.g, res, res, self.W(origin), self.W(p00), du * self.s, dv * self.s, max_depth=5)

    def _look(self, name, P, axis, sign, h, out):
        """Views of the window around P from the side `sign` of `axis`: from
        1, 8 and 64 room sizes outside (sign > 0), or from inside (sign < 0).
        The camera is 1 / 4 unit off the window's centre line, so that no
        pixel centre lies straight ahead."""
        P = np.array(P, float)
        if sign > 0:
            for far in FAR:
                o = P + 0.25
                o[axis] = ROOM + far * ROOM
                out.append(View(f"far{far}{'xyz'[axis]}:{name}", "far", self.window(o, P, axis, h), o))
        else:
            o = P + 0.25
            o[axis] = 16.0
            out.append(View(f"inside{'xyz'[axis]}:{name}", "inside", self.window(o, P, axis, h), o))

    def fan(self, name, origin, lo, hi, axis):
        """Rays from `origin` to a grid over [lo, hi] in the plane through the
        origin perpendicular to `axis`: that component of every direction is
        exactly 0."""
        u, v = (axis + 1) % 3, (axis + 2) % 3
        origin, lo, hi = (np.array(x, float) for x in (origin, lo, hi))
        du, dv = np.zeros(3), np.zeros(3)
        du[u], dv[v] = (hi[u] - lo[u]) / RES, (hi[v] - lo[v]) / RES
        p00 = lo + 0.5 * (du + dv)
        p00[axis] = origin[axis]
        cam = pinhole(self.g, RES, RES, self.W(origin), self.W(p00), du * self.s, dv * self.s, max_depth=5)
        assert cam.center[axis] == cam.pixel00[axis] and cam.pixel_delta_u[axis] == 0.0 == cam.pixel_delta_v[axis]
        return View(f"fan{'xyz'[axis]}:{name}", "fan", cam, origin)

    def _views(self):
        out = []
        R, H = ROOM, ROOM / 2
        # the full walls through the openings, in a band no object reaches (objects: y >= 88, x and z >= 272)
        self._look("left", (0, 32, 480), 0, 1, 24, out)
        self._look("floor", (40, 0, 472), 1, 1, 24, out)
        self._look("back", (480, 32, 0), 2, 1, 24, out)
        # the half walls from outside
        self._look("right", (R, H, 128), 0, 1, 96, out)
        self._look("ceiling", (H, R, 128), 1, 1, 96, out)
        self._look("front", (128, H, R), 2, 1, 96, out)
        self._look("light", (96, 480, 96), 1, -1, 32, out)
        self._look("sphere", SPHERE_C + [SPHERE_R, 0, 0], 0, 1, 12, out)
        # the box: top and bottom, and each side face from the side its rotated normal points to most
        self._look("box+y", BOX_C + [0, BOX_H[1], 0], 1, 1, 8, out)
        self._look("box-y", BOX_C - [0, BOX_H[1], 0], 1, -1, 8, out)
        back = lambda p: np.array([COS * p[0] + SIN * p[2], p[1], -SIN * p[0] + COS * p[2]])   # RotateY's back-map
        for face, n in (("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1))):
            wn = back(np.array(n, float))
            axis = int(np.argmax(np.abs(wn)))
            self._look(f"box{face}", BOX_C + back(np.array(n, float) * BOX_H), axis, 1 if wn[axis] > 0 else -1, 8, out)
        for nm, C, Hs in (("cube", CUBE_C, CUBE_H), ("scube", SCUBE_C, CUBE_H * SCUBE_F)):
            for a in range(3):
                u, v = (a + 1) % 3, (a + 2) % 3
                for sg in (1, -1):
                    P = C.copy()
                    P[a] += sg * Hs[a]
                    self._look(f"{nm}{'+' if sg > 0 else '-'}{'xyz'[a]}", P, a, sg, 0.5 * min(Hs[u], Hs[v]), out)
        # axis-parallel rays
        out.append(self.fan("left-from-8-rooms", (R + 8 * R, 32, 440), (16, 8, 0), (80, 56, 0), 2))
        out.append(self.fan("cube-x", (16, CUBE_C[1] + 8, CUBE_C[2] - 4), (CUBE_C[0] - 56, 0, CUBE_C[2] - 20),
                            (CUBE_C[0] - 40, 0, CUBE_C[2] + 12), 1))
        out.append(self.fan("left-nan-planes", (240, 128, H), (16, 96, 0), (80, 160, 0), 2))
        return out

    def room_camera(self, res=RES):
        """A picture of the room from inside (radiance, bounce records): from
        the low corner towards the objects."""
        o, t = np.array([40.0, 300.0, 24.0]), np.array([400.0, 240.0, 400.0])
        w = (o - t) / np.linalg.norm(o - t)
        u = np.cross([0.0, 1.0, 0.0], w)
        u /= np.linalg.norm(u)
        v = np.cross(w, u)
        f, half = 64.0, 48.0
        du, dv = u * (2 * half / res), -v * (2 * half / res)
        p00 = o - f * w - half * u + half * v + 0.5 * (du + dv)
        return pinhole(self.g, res, res, self.W(o), self.W(p00), du * self.s, dv * self.s, max_depth=5)


_rooms = {}


def room(g, s, k):
    """The (s, k) cell's Room, built once."""
    if (s, k) not in _rooms:
        _rooms[(s, k)] = Room(g, s, k)
    return _rooms[(s, k)]


def interior(top, prim, res=RES):
    """Pixels whose (top, prim) equals that of all eight neighbours (border
    pixels: of the neighbours inside the image)."""
    t, p = top.reshape(res, res), prim.reshape(res, res)
    ok = np.ones((res, res), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, yd = slice(max(dy, 0), res + min(dy, 0)), slice(max(-dy, 0), res + min(-dy, 0))
            xs, xd = slice(max(dx, 0), res + min(dx, 0)), slice(max(-dx, 0), res + min(-dx, 0))
            ok[yd, xd] &= (t[ys, xs] == t[yd, xd]) & (p[ys, xs] == p[yd, xd])
    return ok.reshape(-1)


# references and the checks both test files share -------------------------------
SEED, SAMPLE = 37, 0
MAX_SILHOUETTE = 0.25     # of a view's pixels, on the fp64 oracle alone
MAX_DIFFERENT = 0.02      # of a view's rays may differ from the fp64 oracle's ids (silhouette pixels only)


class Ref:
    """Per view of a cell, computed once and never written again: the fp64
    oracle's ids (the Go arithmetic) and their interior mask, the fp32
    oracle's ids and t, and the camera rays in fp32 (the fp32 oracle's
    bounce-0 rays: the device's get_ray, bit for bit)."""

    def __init__(self, O, room, view):
        self.view = view
        self.top64, self.prim64, _ = O.primary_hits(room.desc, view.cam, SEED, SAMPLE, fp32=False)
        self.top32, self.prim32, t32 = O.primary_hits(room.desc, view.cam, SEED, SAMPLE, fp32=True)
        self.t32 = t32.astype(np.float32)
        self.interior = interior(self.top64, self.prim64)
        ray = O.path_records(room.desc, view.cam, SEED, SAMPLE, 1, fp32=True)[3][0]
        self.o = np.ascontiguousarray(ray[:, 0:3], np.float32)
        self.d = np.ascontiguousarray(ray[:, 3:6], np.float32)
        for a in (self.top64, self.prim64, self.top32, self.prim32, self.t32, self.interior, self.o, self.d):
            a.setflags(write=False)


_refs = {}


def references(g, O, s, k):
    if (s, k) not in _refs:
        r = room(g, s, k)
        _refs[(s, k)] = [Ref(O, r, v) for v in r.views]
    return _refs[(s, k)]


def reached(refs):
    """(top, prim) pairs that are the fp64 oracle's first hit on an interior pixel of some view."""
    out = set()
    for r in refs:
        m = r.interior & (r.prim64 >= 0)
        out |= set(zip(r.top64[m].tolist(), r.prim64[m].tolist()))
    return out


def check_view(what, ref, top, prim, t):
    """The assertions on one view's first hits (top, prim, t as
    rt_primary_hits returns them).  Returns a failure message or None, so a
    caller can report every failing view of a cell at once."""
    diff = (top != ref.top64) | (prim != ref.prim64)
    inner = int(np.sum(diff & ref.interior))
    if inner:
        p = np.flatnonzero(diff & ref.interior)[:3]
        got = [(int(top[i]), int(prim[i])) for i in p]
        want = [(int(ref.top64[i]), int(ref.prim64[i])) for i in p]
        return f"{what}: {inner} interior pixels differ from the fp64 oracle, first {p.tolist()} got {got} want {want}"
    if diff.mean() > MAX_DIFFERENT:
        return f"{what}: {diff.mean():.3f} of the rays differ from the fp64 oracle"
    same = (top == ref.top32) & (prim == ref.prim32) & (prim >= 0)
    tb = np.ascontiguousarray(t, np.float32).view(np.uint32)
    bad = same & (tb != ref.t32.view(np.uint32))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return f"{what}: t differs from the fp32 oracle on {int(bad.sum())} rays, first {i}: {t[i]!r} vs {ref.t32[i]!r}"
    return None


def check_references(room, refs):
    """What must hold before anything is asserted about the code under test,
    on the oracle's output alone: every view is mostly interior and every ray
    of it hits the scene; between them the views reach every primitive on an
    interior pixel; the fans' rays are axis-parallel; the far views start at
    least 63 room sizes (1.6e8 box thicknesses at s = 1) from what they hit.
    And the fp32 oracle itself passes check_view, so that the bit-exact t
    comparison covers every interior pixel."""
    for r in refs:
        sil = 1.0 - r.interior.mean()
        assert sil <= MAX_SILHOUETTE, f"{r.view.name}: {sil:.3f} of the pixels are silhouette"
        assert (r.prim64 >= 0).all(), f"{r.view.name}: a ray of the fp64 oracle misses the scene"
        if r.view.kind == "fan":
            assert np.any(np.all(r.d == 0.0, axis=0)), f"{r.view.name}: no direction component is 0 on every ray"
        msg = check_view(r.view.name, r, r.top32, r.prim32, r.t32)
        assert msg is None, f"the fp32 oracle: {msg}"
    missing = room.expect - reached(refs)
    assert not missing, f"(top, prim) {sorted(missing)} are no interior pixel's first hit"
    assert reached(refs) == room.expect
    far = [r for r in refs if r.view.name.startswith("far64")]
    assert len(far) >= 16
    for r in far:
        dist = r.t32.astype(np.float64) * np.linalg.norm(r.d.astype(np.float64), axis=1)
        assert dist.min() >= 63 * ROOM * room.s, r.view.name
