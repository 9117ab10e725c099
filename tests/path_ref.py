"""The path integral a second time, in float64: a plain recursive `ray_color`
written from camera.go:443-678 (rayColorInternal, sampleLightMIS,
sampleHDRILight, sampleAreaLight), material.go, quad.go:87-97 and
volume.go:34-79 alone, on the primitives of tests/shade_ref.py and the counter
RNG of tests/kat_cases.py, with the draws named as dev_layout.h names them:
(bounce, DOM_CAMERA ..), (bounce, DOM_SCATTER, 3k..), (bounce, DOM_FRESNEL, 0),
(bounce, DOM_NEE, 0: light select; 1, 2: light point; 3, 4: HDRI xi1, xi2),
(bounce, DOM_VOL, 0) for the one volume on a path ray and (bounce,
DOM_VOL_SH_AREA / DOM_VOL_SH_HDRI, 0) on that bounce's two shadow rays.

The world is a short flat list (HittableList.Hit, hittable_list.go:31-45: the
closest hit of the interval) of quads, spheres (at rest or moving), triangles
(triangle.go:57-104), circles (circle.go:34-74), at most one slab volume whose
boundary is a list of two quads, and `wrapped` objects: a primitive or a list
of primitives under a chain of transform.go's Translate, RotateX, RotateY,
RotateZ and Scale, restated from the Go text as written (wrap_ray,
unwrap_hit: RotateX and RotateZ turn rec.P and rec.Normal by +theta after
turning the ray by +theta, transform.go:244-262, 325-343, so the reported
point is not on the incoming ray).  The closest hit is found by brute force,
or, with Scene.tree, by BVHNode.Hit's walk (bvh.go:219-239) over the boxes the
scene description carries, AABB.Hit restated from aabb.go:59-116.

Besides the radiance, `trace` returns per bounce the hit (object, t), the
incoming ray, whether the path ended, and the NEE record: which of the two
shadow rays was wanted (the cos(theta) <= 0 cut passed, so the reference asks
world.Hit), each one's direction, end and contribution, whether it was
visible, and the light chosen.

Margins.  Every comparison float64 makes along the path is recorded as the
distance to its threshold divided by the figure below; a bounce whose smallest
ratio is under 1 is undecided, the path is left out from that bounce on and
its pixel is left out of the radiance.  From shade_ref / shade_cases: branch
(TIR, Fresnel draw, Metal's dot) 1e-5, a sphere's silhouette 1e-3 of its
radius, a CDF entry 1e-6, a free flight 1e-4 of the distance inside the
medium.  Added here:

  quad alpha, beta against 0 and 1    1e-5   (dimensionless, a few fp32 operations: error ~ 1e-6;
                                              closest hit and every occluder of every shadow ray)
  t against an end of the interval    2e-6   as a distance along the quad's normal, |t - end| |n.d|: the fp32
                                              error of the numerator D - n.o for coordinates up to 4 is below
                                              1e-6; this is the 0.001 of a ray leaving its own surface, the 0.001
                                              that keeps the light out of its shadow ray, and an occluder's t
                                              against the ray's end.  It does not apply where fp32 evaluates that
                                              numerator exactly: an axis-aligned normal (components 0, +-1) and
                                              at most one non-zero term among D and the n_i o_i, as for a plane
                                              x = 0 (`edge_on`) or a ray from the origin.  And 1e-5 max(1, end)
                                              as a distance along the ray, always
  closest t against the runner-up     1e-5   relative
  cos(theta) against 0                1e-5   (unit vectors)
  cos(light) against 0.001            1e-5
  U n against the next integer        1e-6   (U a multiple of 2^-24, as for a CDF entry)
  a contribution channel against 20   1e-5   relative
  a volume's free flight and exit     1e-4   relative (shade_cases' MARGIN_FLIGHT), for path and shadow rays

Wrapped objects.  The inner tests keep their margins and are evaluated in
object space, where fp32 evaluates them.  MARGIN_PLANE's derivation assumes
coordinates up to 4 and one rounding of the ray; a chain breaks both, so
every margin of an inner test (alpha / beta, the barycentrics, the plane
distance, t against an end, the silhouette, the runner-up) is multiplied by

  k = (1 + wrappers) max(1, m / 4)

m the largest coordinate magnitude the ray's origin takes on its way through
the chain, or an inner primitive's defining points have.  Derivation: a
wrapper's map of a coordinate is at most three fp32 roundings (c x - s z), each
half an ulp of a value up to m, about 3 * 2^-25 m ~ 1e-7 m: 4e-7 per wrapper at
m = 4, a fifth of MARGIN_PLANE, against the 1e-6 the unwrapped numerator is
allowed; (1 + wrappers) keeps that ratio, and m / 4 scales the absolute
figures with the coordinates fp32 rounds.  The dimensionless margins take the
same factor: their fp32 error grows with the same roundings of P - Q against
an edge.  A box test of the world tree is undecided when a slab interval's
two ends lie within 1e-5 max(1, |t|) of each other.  A triangle's determinant
against its 1e-8 cut is held as the cosine it is, 1e-5.

Departures of the project the comparison encodes: those of shade_ref;
SHADOW_END leaves `dist - 0.001` alone below dist = 1048, every scene here."""
import math

import numpy as np

from tests import shade_ref as R
from tests.kat_cases import random_unit_vector, rnd

DOM_CAMERA, DOM_SCATTER, DOM_FRESNEL, DOM_NEE, DOM_VOL, DOM_VOL_SH_AREA, DOM_VOL_SH_HDRI = 0, 1, 2, 3, 4, 5, 6

MARGIN_BRANCH = 1e-5
MARGIN_EDGE = 1e-3
MARGIN_CDF = 1e-6
MARGIN_FLIGHT = 1e-4
MARGIN_AB = 1e-5
MARGIN_PLANE = 2e-6
MARGIN_T = 1e-5
MARGIN_COS = 1e-5
MARGIN_SELECT = 1e-6
MARGIN_CLAMP = 1e-5
CLAMP = 20.0
INF = math.inf


def _v(x):
    return np.asarray(x, np.float64)


# ---------------------------------------------------------------------------
# the scene: plain data
# ---------------------------------------------------------------------------
def solid(rgb):
    return ("solid", tuple(float(x) for x in rgb))


def checker(scale, even, odd):
    return ("checker", float(scale), tuple(even), tuple(odd))


def tex_value(tex, p):
    """SolidColor / CheckerTexture.Value (texture.go:63-77) at the point p."""
    if tex[0] == "solid":
        return _v(tex[1])
    inv = 1.0 / tex[1]
    s = sum(int(math.floor(inv * float(c) + 1e-4)) for c in p)
    return _v(tex[2] if s % 2 == 0 else tex[3])


def lambertian(rgb):
    return dict(kind="lambertian", tex=solid(rgb))


def light(rgb):
    return dict(kind="light", tex=solid(rgb))


def light_tex(tex):
    return dict(kind="light", tex=tex)


def metal(rgb, fuzz):
    return dict(kind="metal", albedo=tuple(rgb), fuzz=min(float(fuzz), 1.0))


def dielectric(ior):
    return dict(kind="dielectric", ior=float(ior))


def quad(Q, u, v, mat, name=""):
    return dict(kind="quad", Q=_v(Q), u=_v(u), v=_v(v), mat=mat, name=name)


def sphere(c, r, mat, name="", vel=(0, 0, 0)):
    """vel: Center.dir (sphere.go:49-51), the centre at time 1 less the centre at time 0."""
    return dict(kind="sphere", c=_v(c), r=float(r), mat=mat, name=name, vel=_v(vel))


def tri(a, b, c, mat, name=""):
    return dict(kind="tri", a=_v(a), b=_v(b), c=_v(c), mat=mat, name=name)


def circle(c, n, r, mat, name=""):
    """NewCircle (circle.go:14-29): the normal is made unit."""
    return dict(kind="circle", c=_v(c), n=R.unit(n), r=float(r), mat=mat, name=name)


def wrapped(chain, inner, name=""):
    """A primitive, or a list of primitives (HittableList), under transform.go's
    wrappers, outermost first: ("translate", off), ("rot_x" | "rot_y" |
    "rot_z", sin, cos), ("scale", factor)."""
    ch = []
    for w in chain:
        if w[0] in ("translate", "scale"):
            ch.append((w[0], _v(w[1])))
        else:
            assert w[0] in ("rot_x", "rot_y", "rot_z"), w
            ch.append((w[0], float(w[1]), float(w[2])))
    prims = list(inner) if isinstance(inner, (list, tuple)) else [inner]
    assert all(p["kind"] in ("quad", "sphere", "tri", "circle") for p in prims)
    return dict(kind="wrapped", chain=ch, inner=prims, name=name)


def node(left, right, box=None):
    """BVHNode{left, right} over the world list: a child is an index into
    Scene.objects or another node; box (xmin, xmax, ymin, ymax, zmin, zmax) is
    the one the scene description carries, the caller's data."""
    return dict(left=left, right=right, box=box)


def slab(front, back, rho, albedo, name="fog"):
    """Volume (volume.go:9-31) over a boundary list of two quads (Q, u, v each)."""
    return dict(kind="volume", faces=[tuple(_v(x) for x in front), tuple(_v(x) for x in back)], rho=float(rho),
                mat=dict(kind="isotropic", tex=solid(albedo)), name=name)


class Scene:
    """objects: the world list, in order; lights: indices into it (Camera.Lights);
    env: None or dict(img, rotation, importance); sky / background / phantom /
    cam_max_depth: the camera's fields rayColorInternal reads; tree: None (the
    world is the flat list) or the world's root `node`."""

    def __init__(self, objects, lights=(), env=None, sky=False, background=(0, 0, 0), phantom=False, cam_max_depth=0,
                 tree=None):
        self.objects, self.lights = list(objects), list(lights)
        self.tree = tree
        self.env, self.sky, self.background, self.phantom = env, sky, _v(background), phantom
        self.cam_max_depth = cam_max_depth
        self.dist = R.build_distribution(env["img"]) if env and env["importance"] else None


# ---------------------------------------------------------------------------
# hits over an interval, with the margins of every comparison made
# ---------------------------------------------------------------------------
def _bound_ratio(t, bound, denom, exact, k=1.0):
    if math.isinf(bound):
        return INF
    along = abs(t - bound) / (MARGIN_T * k * max(1.0, abs(bound)))
    return along if exact else min(abs(t - bound) * abs(denom) / (MARGIN_PLANE * k), along)


def quad_test(o, d, Q, u, v, tmin, tmax, k=1.0):
    """Quad.Hit (quad.go:44-71) over [tmin, tmax]: (hit or None, ratio).  hit as shade_ref.quad_hit.
    k: the factor a wrapper chain puts on every margin (wrapped_test); 1 in the world."""
    n = R.unit(np.cross(u, v))
    denom = float(n @ d)
    if abs(denom) < 1e-8:
        return None, INF
    D = float(n @ Q)
    t = (D - float(n @ o)) / denom
    # the numerator D - n.o is exact in fp32: nothing to round
    exact = k == 1.0 and all(abs(c) in (0.0, 1.0) for c in n) and sum(1 for x in [D] + list(n * o) if x != 0.0) <= 1
    ratio = min(_bound_ratio(t, tmin, denom, exact, k), _bound_ratio(t, tmax, denom, exact, k))
    mab = MARGIN_AB * k
    if not (tmin <= t <= tmax):
        # outside the interval by a margin: whether the point is interior no longer matters
        if ratio >= 1:
            return None, INF
        a, b = R.quad_uv(o + d * t, Q, u, v)
        return None, (ratio if (-mab < a < 1 + mab and -mab < b < 1 + mab) else INF)
    P = o + d * t
    a, b = R.quad_uv(P, Q, u, v)
    ab = min(abs(a), abs(a - 1), abs(b), abs(b - 1)) / mab
    if not (0 <= a <= 1 and 0 <= b <= 1):
        return None, ab
    front, N = R.face_normal(d, n)
    return (t, P, front, N, a, b), min(ratio, ab)


def tri_test(o, d, v0, v1, v2, tmin, tmax, k=1.0):
    """Triangle.Hit (triangle.go:57-104) over [tmin, tmax]: (hit or None,
    ratio), u and v the barycentrics.  Margins: the determinant against its
    1e-8 cut as the cosine it is (a / (|e1 x e2| |d|), MARGIN_COS); u, v and
    u + v against 0 and 1 (MARGIN_AB); t against the interval's ends as a
    quad's."""
    e1, e2 = v1 - v0, v2 - v0
    h = np.cross(d, e2)
    a = float(e1 @ h)
    cr = np.cross(e1, e2)
    scale = math.sqrt(float(cr @ cr)) * math.sqrt(float(d @ d))
    ratio = abs(abs(a) - 1e-8) / (MARGIN_COS * k * scale)
    if abs(a) < 1e-8:
        return None, ratio
    f = 1.0 / a
    s = o - v0
    u = f * float(s @ h)
    q = np.cross(s, e1)
    v = f * float(d @ q)
    t = f * float(e2 @ q)
    n = R.unit(cr)                                            # NewTriangle (triangle.go:23)
    denom = float(n @ d)
    bound = min(_bound_ratio(t, tmin, denom, False, k), _bound_ratio(t, tmax, denom, False, k))
    mab = MARGIN_AB * k
    ab = min(abs(u), abs(u - 1), abs(v), abs(u + v - 1)) / mab
    inside = not (u < 0.0 or u > 1.0) and not (v < 0.0 or u + v > 1.0)
    if not (tmin <= t <= tmax):
        if bound >= 1:
            return None, ratio
        return None, min(ratio, bound if (inside or ab < 1) else INF)
    if not inside:
        return None, min(ratio, ab)
    front, N = R.face_normal(d, n)
    return (t, o + d * t, front, N, u, v), min(ratio, bound, ab)


def circle_test(o, d, c, n, r, tmin, tmax, k=1.0):
    """Circle.Hit (circle.go:34-74) over [tmin, tmax]: (hit or None, ratio).
    The distance from the centre against the radius: MARGIN_EDGE of the radius."""
    denom = float(n @ d)
    if abs(denom) < 1e-8:
        return None, INF
    t = (float(n @ c) - float(n @ o)) / denom
    bound = min(_bound_ratio(t, tmin, denom, False, k), _bound_ratio(t, tmax, denom, False, k))
    P = o + d * t
    lp = P - c
    dist = math.sqrt(float(lp @ lp))
    edge = abs(dist / r - 1.0) / (MARGIN_EDGE * k)
    if not (tmin <= t <= tmax):
        if bound >= 1:
            return None, INF
        return None, (bound if (dist <= r or edge < 1) else INF)
    if dist > r:
        return None, edge
    front, N = R.face_normal(d, n)
    u, v = R.circle_uv(P, c, n, r)
    return (t, P, front, N, u, v), min(bound, edge)


def sphere_test(o, d, c, r, tmin, tmax, k=1.0, vel=None, time=0.0):
    """Sphere.Hit (sphere.go:63-94) over (tmin, tmax): (hit or None, ratio)."""
    assert tmin == 0.001
    moving = vel is not None and bool(np.any(vel))
    cen = c + vel * time if moving else c                    # Center.At(r.Time()) (sphere.go:49-51, 64)
    b_imp = float(np.linalg.norm(np.cross(d, cen - o)) / np.linalg.norm(d))
    ratio = abs(b_imp / r - 1.0) / (MARGIN_EDGE * k)
    h = R.sphere_hit(o, d, c, r, vel, time) if moving else R.sphere_hit(o, d, c, r)
    if h is None:
        return None, ratio
    t = h[0]
    ratio = min(ratio, abs(t - tmin) / (MARGIN_T * k),
                INF if math.isinf(tmax) else abs(t - tmax) / (MARGIN_T * k * max(1.0, tmax)))
    if not t < tmax:        # the far root is farther still (Surrounds, interval.go:61-63)
        return None, ratio
    return h, ratio


# ---------------------------------------------------------------------------
# transform.go: the five wrappers, as written
# ---------------------------------------------------------------------------
def _turn(p, i, j, s, c, sign):
    """p with p_i' = c p_i - sign s p_j, p_j' = sign s p_i + c p_j."""
    q = p.copy()
    q[i] = c * p[i] - sign * s * p[j]
    q[j] = sign * s * p[i] + c * p[j]
    return q


def wrap_ray(w, o, d):
    """A wrapper's map of the ray on the way in: (origin, direction)."""
    if w[0] == "translate":                                  # Translate.Hit (transform.go:94): the origin only
        return o - w[1], d
    if w[0] == "scale":                                      # Scale.Hit (transform.go:409-418): both by InvFactor
        inv = 1.0 / w[1]                                     # NewScale (transform.go:368-372)
        return o * inv, d * inv
    s, c = w[1], w[2]
    if w[0] == "rot_y":                                      # RotateY.Hit (transform.go:163-167): x' = c x - s z, z' = s x + c z
        return _turn(o, 0, 2, s, c, 1.0), _turn(d, 0, 2, s, c, 1.0)
    if w[0] == "rot_x":                                      # RotateX.Hit (transform.go:244-248): y' = c y - s z, z' = s y + c z
        return _turn(o, 1, 2, s, c, 1.0), _turn(d, 1, 2, s, c, 1.0)
    return _turn(o, 0, 1, s, c, 1.0), _turn(d, 0, 1, s, c, 1.0)   # RotateZ.Hit (transform.go:325-329): x' = c x - s y, y' = s x + c y


def unwrap_hit(w, P, N):
    """A wrapper's map of rec.P and rec.Normal on the way out."""
    if w[0] == "translate":                                  # transform.go:100: P only
        return P + w[1], N
    if w[0] == "scale":                                      # transform.go:426-437: P by Factor, N by InvFactor, Unit()
        return P * w[1], R.unit(N * (1.0 / w[1]))
    s, c = w[1], w[2]
    if w[0] == "rot_y":                                      # transform.go:175-181: x' = c x + s z, z' = -s x + c z, the inverse turn
        return _turn(P, 0, 2, s, c, -1.0), _turn(N, 0, 2, s, c, -1.0)
    if w[0] == "rot_x":                                      # transform.go:256-262: the same turn as the ray's, +theta again
        return _turn(P, 1, 2, s, c, 1.0), _turn(N, 1, 2, s, c, 1.0)
    return _turn(P, 0, 1, s, c, 1.0), _turn(N, 0, 1, s, c, 1.0)   # transform.go:337-343: as RotateX, +theta again


def _extent(pr):
    """The largest coordinate magnitude among a primitive's defining points."""
    if pr["kind"] == "quad":
        pts = [pr["Q"], pr["Q"] + pr["u"], pr["Q"] + pr["v"], pr["Q"] + pr["u"] + pr["v"]]
    elif pr["kind"] == "tri":
        pts = [pr["a"], pr["b"], pr["c"]]
    elif pr["kind"] == "circle":
        pts = [pr["c"] - pr["r"], pr["c"] + pr["r"]]
    else:
        pts = [pr["c"] - pr["r"], pr["c"] + pr["r"], pr["c"] + pr["vel"] - pr["r"], pr["c"] + pr["vel"] + pr["r"]]
    return float(np.abs(np.array(pts)).max())


def prim_test(pr, o, d, time, tmin, tmax, k=1.0):
    """One primitive's Hit: (hit (t, P, front, N, u, v) or None, ratio)."""
    if pr["kind"] == "quad":
        return quad_test(o, d, pr["Q"], pr["u"], pr["v"], tmin, tmax, k)
    if pr["kind"] == "tri":
        return tri_test(o, d, pr["a"], pr["b"], pr["c"], tmin, tmax, k)
    if pr["kind"] == "circle":
        return circle_test(o, d, pr["c"], pr["n"], pr["r"], tmin, tmax, k)
    h, rt = sphere_test(o, d, pr["c"], pr["r"], tmin, tmax, k, pr.get("vel"), time)
    return (h[:6] if h else None), rt


def chain_margin(ob, o):
    """The factor a chain puts on the margins of its inner tests (the module's
    docstring): (1 + wrappers) max(1, m / 4), m the largest coordinate the
    ray's origin takes through the chain or an inner primitive has."""
    m = float(np.abs(o).max())
    d = np.zeros(3)
    for w in ob["chain"]:
        o, d = wrap_ray(w, o, d)
        m = max(m, float(np.abs(o).max()))
    m = max([m] + [_extent(pr) for pr in ob["inner"]])
    return (1.0 + len(ob["chain"])) * max(1.0, m / 4.0)


def wrapped_test(o, d, time, ob, tmin, tmax):
    """The Hit of a chain of transform.go's wrappers over a primitive or a
    HittableList of primitives: (hit or None, ratio, the inner primitive hit, k).
    The ray goes in wrapper by wrapper and keeps its time, the interval and t
    are unchanged (every wrapper hands rayT on), rec.P and rec.Normal come
    back wrapper by wrapper, FrontFace, u and v stay as the primitive set
    them.  The inner list is HittableList.Hit (hittable_list.go:31-45): the
    closest of its hits, by brute force; no inner box is tested."""
    k = chain_margin(ob, o)
    for w in ob["chain"]:
        o, d = wrap_ray(w, o, d)
    found, ratio = [], INF
    for j, pr in enumerate(ob["inner"]):
        h, rt = prim_test(pr, o, d, time, tmin, tmax, k)
        ratio = min(ratio, rt)
        if h:
            found.append((h[0], j, h))
    if not found:
        return None, ratio, -1, k
    found.sort(key=lambda x: x[0])
    if len(found) > 1:
        ratio = min(ratio, (found[1][0] - found[0][0]) / max(found[0][0], 1e-30) / (MARGIN_T * k))
    t, j, h = found[0]
    P, N = h[1], h[3]
    for w in reversed(ob["chain"]):
        P, N = unwrap_hit(w, P, N)
    return (t, P, h[2], N, h[4], h[5]), ratio, j, k


def aabb_test(box, o, d, tmin, tmax):
    """AABB.Hit (aabb.go:59-116): (hit, ratio).  Undecided when a slab
    interval's two ends lie within MARGIN_T max(1, |t|) of each other."""
    ratio = INF
    for a in range(3):
        adinv = 1.0 / d[a] if d[a] != 0.0 else math.copysign(INF, d[a])
        t0, t1 = (box[2 * a] - o[a]) * adinv, (box[2 * a + 1] - o[a]) * adinv
        if adinv < 0:
            t0, t1 = t1, t0
        if t0 > tmin:
            tmin = t0
        if t1 < tmax:
            tmax = t1
        if not (math.isinf(tmax) or math.isinf(tmin) or math.isnan(tmax) or math.isnan(tmin)):
            ratio = min(ratio, abs(tmax - tmin) / (MARGIN_T * max(1.0, abs(tmin), abs(tmax))))
        if tmax <= tmin:
            return False, ratio
    return True, ratio


def volume_test(o, d, vol, tmin, tmax, u_flight):
    """Volume.Hit (volume.go:34-79) over [tmin, tmax] for a boundary list of
    quads: (t or None, ratio)."""
    def boundary(lo):
        best, ratio = None, INF
        for Q, u, v in vol["faces"]:
            h, rt = quad_test(o, d, Q, u, v, lo, INF if best is None else best)
            ratio = min(ratio, rt)
            if h:
                best = h[0]
        return best, ratio
    t1, r1 = boundary(-INF)
    if t1 is None:
        return None, r1
    t2, r2 = boundary(t1 + 0.0001)
    ratio = min(r1, r2)
    if t2 is None:
        return None, ratio
    ln = math.sqrt(float(d @ d))
    if t1 < tmin:
        t1 = tmin
    if t2 > tmax:
        t2 = tmax
    ratio = min(ratio, abs(t2 - t1) * ln / MARGIN_T)
    if t1 >= t2:
        return None, ratio
    if t1 < 0:
        t1 = 0.0
    inside = (t2 - t1) * ln
    hd = -math.log(u_flight) / vol["rho"] if u_flight > 0 else INF
    ratio = min(ratio, abs(hd - inside) / inside / MARGIN_FLIGHT)
    if hd > inside:
        return None, ratio
    return t1 + hd / ln, ratio


def object_test(scene, k, o, d, tmin, tmax, key, bounce, vol_dom, time):
    """World object k's Hit over the interval: (hit or None, ratio, the inner
    primitive hit (-1: the object is one), the factor on the margins)."""
    ob = scene.objects[k]
    if ob["kind"] == "wrapped":
        return wrapped_test(o, d, time, ob, tmin, tmax)
    if ob["kind"] == "volume":
        t, rt = volume_test(o, d, ob, tmin, tmax, rnd(*key, bounce, vol_dom, 0))
        return ((t, o + d * t, True, _v((1.0, 0.0, 0.0)), 0.0, 0.0) if t is not None else None), rt, -1, 1.0
    h, rt = prim_test(ob, o, d, time, tmin, tmax)
    return h, rt, -1, 1.0


def tree_hit(scene, nd, o, d, tmin, tmax, key, bounce, vol_dom, time):
    """BVHNode.Hit (bvh.go:219-239): the node tests its own box, the left
    child is walked over the interval, the right child over [tmin, the left's
    hit]; a child that is a world object tests no box of its own (no wrapper's
    Hit does).  (None or (k, hit, sub), ratio)."""
    if not isinstance(nd, dict):
        h, rt, sub, _ = object_test(scene, nd, o, d, tmin, tmax, key, bounce, vol_dom, time)
        return ((nd, h, sub) if h else None), rt
    ok, ratio = aabb_test(nd["box"], o, d, tmin, tmax)
    if not ok:
        return None, ratio
    left, rl = tree_hit(scene, nd["left"], o, d, tmin, tmax, key, bounce, vol_dom, time)
    right, rr = tree_hit(scene, nd["right"], o, d, tmin, left[1][0] if left else tmax, key, bounce, vol_dom, time)
    return (right or left), min(ratio, rl, rr)


def world_hit(scene, o, d, tmin, tmax, key, bounce, vol_dom, time=0.0):
    """HittableList.Hit over the world (or BVHNode.Hit over scene.tree):
    (index, hit) of the closest hit or (None, None), the ratio of every
    comparison made, and whether a volume was among the hits of the interval.
    hit: (t, P, front, N, u, v, sub) (a volume: the arbitrary normal (1, 0,
    0), front face; sub: the inner primitive of a wrapped list, else -1)."""
    if scene.tree is not None:
        got, ratio = tree_hit(scene, scene.tree, o, d, tmin, tmax, key, bounce, vol_dom, time)
        if got is None:
            return None, None, ratio, False
        return got[0], got[1] + (got[2],), ratio, False
    found, ratio = [], INF
    for k in range(len(scene.objects)):
        h, rt, sub, kk = object_test(scene, k, o, d, tmin, tmax, key, bounce, vol_dom, time)
        ratio = min(ratio, rt)
        if h:
            found.append((h[0], k, h + (sub,), kk))
    if not found:
        return None, None, ratio, False
    by_vol = any(scene.objects[k]["kind"] == "volume" for _, k, _, _ in found)
    found.sort(key=lambda x: x[0])
    if len(found) > 1:
        ratio = min(ratio, (found[1][0] - found[0][0]) / max(found[0][0], 1e-30) / (MARGIN_T * max(found[0][3], found[1][3])))
    return found[0][1], found[0][2], ratio, by_vol


def material_of(scene, k, sub):
    ob = scene.objects[k]
    return ob["inner"][sub]["mat"] if ob["kind"] == "wrapped" else ob["mat"]


# ---------------------------------------------------------------------------
# the path
# ---------------------------------------------------------------------------
class Path:
    """What `trace` returns: L; bounces: per bounce dict(o, d, obj (-1 a miss),
    t, nee, ratio: the smallest ratio of the bounce's closest hit, ratio_shade:
    of what the bounce decides after it); the path has no ray at bounces past
    len(bounces): it ended.  margin: the smallest ratio of the path."""

    def __init__(self):
        self.bounces = []
        self.L = None

    @property
    def margin(self):
        return min([min(b["ratio"], b["ratio_shade"]) for b in self.bounces] + [INF])

    def decided_hits(self):
        """How many bounces' hits float64 decides with a margin: bounce b's
        hit counts when every decision up to it does."""
        n = 0
        for b in self.bounces:
            if b["ratio"] < 1:
                break
            n += 1
            if b["ratio_shade"] < 1:
                break
        return n

    def decided_shades(self):
        n = 0
        for b in self.bounces:
            if b["ratio"] < 1 or b["ratio_shade"] < 1:
                break
            n += 1
        return n


def miss_colour(scene, d, depth):
    """camera.go:451-466."""
    if scene.env is not None:
        if scene.phantom and depth == scene.cam_max_depth:
            return np.zeros(3)
        return R.env_sample(scene.env["img"], scene.env["rotation"], d)[0]
    if scene.sky:                                           # SkyGradient (camera.go:520-526)
        a = 0.5 * (R.unit(d)[1] + 1.0)
        return _v((1.0, 1.0, 1.0)) * (1.0 - a) + _v((0.5, 0.7, 1.0)) * a
    return scene.background


def lambert_pdf(normal, wo):
    """Lambertian.PDF (material.go:70-76)."""
    c = float(normal @ wo)
    return 0.0 if c < 0 else c / math.pi


def _clamp(con):
    ratio = float(np.abs(con / CLAMP - 1.0).min()) / MARGIN_CLAMP
    return np.minimum(con, CLAMP), ratio, con


def sample_hdri(scene, P, N, att, key, bounce):
    """sampleHDRILight (camera.go:565-607): the NEE record's HDRI half."""
    env, dist = scene.env, scene.dist
    img = env["img"]
    H, W = img.shape[:2]
    xi1, xi2 = rnd(*key, bounce, DOM_NEE, 3), rnd(*key, bounce, DOM_NEE, 4)
    y = R.search_cdf(dist["marginal"], xi1)
    x = R.search_cdf(dist["cond"][y], xi2)
    ratio = min(float(np.abs(dist["marginal"] - xi1).min()), float(np.abs(dist["cond"][y] - xi2).min())) / MARGIN_CDF
    ld = R.uv_to_dir((x + 0.5) / W, (y + 0.5) / H, env["rotation"])
    pdf_h = R.env_pdf(img, dist, env["rotation"], ld)
    cos_t = float(N @ ld)
    ratio = min(ratio, abs(cos_t) / MARGIN_COS)
    rec = dict(wanted=False, visible=False, by_volume=False, dir=ld, end=INF, con=np.zeros(3), raw=np.zeros(3), texel=(x, y))
    if cos_t <= 0:
        return rec, ratio
    rec["wanted"] = True
    k, _, rt, rec["by_volume"] = world_hit(scene, P, ld, 0.001, INF, key, bounce, DOM_VOL_SH_HDRI)
    rec["occluder"] = k
    ratio = min(ratio, rt)
    if k is not None:
        return rec, ratio
    rec["visible"] = True
    pdf_b = lambert_pdf(N, ld)
    wgt = pdf_h / (pdf_h + pdf_b)
    con = img[y, x] * (cos_t / pdf_h * wgt) * att
    rec["con"], rc, rec["raw"] = _clamp(con)
    return rec, min(ratio, rc)


def sample_area(scene, P, N, att, li, key, bounce):
    """sampleAreaLight (camera.go:610-678): the NEE record's area half."""
    rec = dict(wanted=False, visible=False, by_volume=False, cut=False, dir=np.zeros(3), end=0.0, con=np.zeros(3),
               raw=np.zeros(3), light=li, lp=np.zeros(3), clamped=np.zeros(3, bool))
    ob = scene.objects[scene.lights[li]]
    if ob["kind"] != "quad":                                 # light.(*Quad) fails (camera.go:616-619)
        return rec, INF
    al, be = rnd(*key, bounce, DOM_NEE, 1), rnd(*key, bounce, DOM_NEE, 2)
    lp = ob["Q"] + ob["u"] * al + ob["v"] * be               # Quad.SamplePoint (quad.go:87-92)
    to = lp - P
    dist = math.sqrt(float(to @ to))
    ld = R.unit(to)
    cos_t = float(N @ ld)
    ratio = abs(cos_t) / MARGIN_COS
    rec.update(dir=ld, end=dist - 0.001, lp=lp)
    if cos_t <= 0:
        return rec, ratio
    rec["wanted"] = True
    # the cut of camera.go:651, worked out for every wanted ray: the reference applies it after the shadow
    # test, the device before it queues the ray (rec["cut"]: what the device's wanted bit also needs)
    n_l = R.unit(np.cross(ob["u"], ob["v"]))
    cos_l = abs(float(n_l @ -ld))
    ratio = min(ratio, abs(cos_l - 0.001) / MARGIN_COS)
    rec["cut"] = cos_l < 0.001
    k, _, rt, rec["by_volume"] = world_hit(scene, P, ld, 0.001, dist - 0.001, key, bounce, DOM_VOL_SH_AREA)
    rec["occluder"] = k                                      # the shadow ray's time is 0 (camera.go:636)
    ratio = min(ratio, rt)
    if k is not None:
        return rec, ratio
    rec["visible"] = True
    emission = tex_value(ob["mat"]["tex"], lp)               # Emitted(0, 0, lightPoint): u = v = 0, only p matters here
    area = float(np.linalg.norm(np.cross(ob["u"], ob["v"])))
    if cos_l < 0.001:
        return rec, ratio
    pdf_l = dist * dist / (cos_l * area)
    pdf_b = lambert_pdf(N, ld)
    wgt = pdf_l / (pdf_l + pdf_b)
    con = emission * (cos_t / pdf_l * wgt) * att * float(len(scene.lights))
    rec["con"], rc, rec["raw"] = _clamp(con)
    rec["clamped"] = con > CLAMP
    return rec, min(ratio, rc)


def ray_color(scene, ray, depth, allow, key, path=None, bounce=0):
    """rayColorInternal (camera.go:443-518).  ray = (origin, direction[,
    time]), key = (seed, pixel, sample); fills `path` (a Path) with the bounces'
    records.  A scattered ray keeps its parent's time (material.go:64, 116, 185, 267)."""
    if depth <= 0:
        return np.zeros(3)
    o, d = ray[0], ray[1]
    time = ray[2] if len(ray) > 2 else 0.0
    path = path if path is not None else Path()
    k, h, ratio, _ = world_hit(scene, o, d, 0.001, INF, key, bounce, DOM_VOL, time)
    b = dict(sub=-1 if k is None else h[6], hit=h, o=o, d=d, obj=-1 if k is None else k, t=-1.0 if k is None else h[0], nee=None, ratio=ratio, ratio_shade=INF,
             allow=allow, depth=depth, Le=np.zeros(3), att=None)
    path.bounces.append(b)
    if k is None:
        b["Le"] = miss_colour(scene, d, depth)
        return b["Le"]
    t, P, front, N, u, v = h[:6]
    mat = material_of(scene, k, h[6])
    if mat["kind"] == "light":
        # Emitted(rec.U, rec.V, rec.P) (camera.go:471-481): solid and checker textures read P only
        b["Le"] = tex_value(mat["tex"], P) if allow else np.zeros(3)
        b["light_hit"] = True
        return b["Le"]
    if mat["kind"] == "lambertian":
        sd = N + random_unit_vector(*key, bounce)
        if all(abs(c) < 1e-8 for c in sd):
            sd = N
        att = tex_value(mat["tex"], P)
    elif mat["kind"] == "isotropic":
        sd = random_unit_vector(*key, bounce)
        att = tex_value(mat["tex"], P)
    elif mat["kind"] == "metal":
        sd, dot = R.metal_scatter(d, N, mat["fuzz"], random_unit_vector(*key, bounce))
        att = _v(mat["albedo"])
        b["ratio_shade"] = abs(dot) / MARGIN_BRANCH
        if not dot > 0:                                      # Scatter false: the emission, 0 (camera.go:473-481)
            return np.zeros(3)
    else:
        sd, br, (m_tir, m_fr) = R.dielectric_scatter(d, N, front, mat["ior"], rnd(*key, bounce, DOM_FRESNEL, 0))
        att = np.ones(3)
        b["ratio_shade"] = min(abs(m_tir), abs(m_fr) if m_tir < 0 else INF) / MARGIN_BRANCH
        b["branch"] = br
    b["att"], b["scatter"] = att, (P, sd)
    use_mis = mat["kind"] == "lambertian" and len(scene.lights) > 0
    if not use_mis:
        return att * ray_color(scene, (P, sd, time), depth - 1, True, key, path, bounce + 1)
    nl = len(scene.lights)
    un = rnd(*key, bounce, DOM_NEE, 0) * nl
    li = min(int(un), nl - 1)
    b["ratio_shade"] = min(b["ratio_shade"], min(abs(un - math.floor(un)), abs(math.floor(un) + 1 - un)) / MARGIN_SELECT
                           if nl > 1 else INF)
    nee = dict(light=li, hdri=None, area=None)
    direct = np.zeros(3)
    if scene.env is not None and scene.env["importance"]:
        nee["hdri"], rt = sample_hdri(scene, P, N, att, key, bounce)
        b["ratio_shade"] = min(b["ratio_shade"], rt)
        direct = direct + nee["hdri"]["con"]
    nee["area"], rt = sample_area(scene, P, N, att, li, key, bounce)
    b["ratio_shade"] = min(b["ratio_shade"], rt)
    direct = direct + nee["area"]["con"]
    nee["direct"] = direct
    b["nee"] = nee
    indirect = att * ray_color(scene, (P, sd, time), depth - 1, False, key, path, bounce + 1)
    return direct + indirect                                 # colorFromEmission is 0 for every scattering material


def trace(scene, cam, i, j, seed, sample, depth):
    """One pixel-sample: RayColor (camera.go:438-441) of GetRay's ray."""
    o, d, time, _ = R.get_ray(cam, i, j, seed, sample)
    path = Path()
    path.L = ray_color(scene, (o, d, time), depth, True, (seed, j * cam.image_width + i, sample), path)
    return path
