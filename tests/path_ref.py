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
closest hit of the interval) of quads and spheres, plus at most one slab
volume whose boundary is a list of two quads.  The closest hit is found by
brute force.

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


def sphere(c, r, mat, name=""):
    return dict(kind="sphere", c=_v(c), r=float(r), mat=mat, name=name)


def slab(front, back, rho, albedo, name="fog"):
    """Volume (volume.go:9-31) over a boundary list of two quads (Q, u, v each)."""
    return dict(kind="volume", faces=[tuple(_v(x) for x in front), tuple(_v(x) for x in back)], rho=float(rho),
                mat=dict(kind="isotropic", tex=solid(albedo)), name=name)


class Scene:
    """objects: the world list, in order; lights: indices into it (Camera.Lights);
    env: None or dict(img, rotation, importance); sky / background / phantom /
    cam_max_depth: the camera's fields rayColorInternal reads."""

    def __init__(self, objects, lights=(), env=None, sky=False, background=(0, 0, 0), phantom=False, cam_max_depth=0):
        self.objects, self.lights = list(objects), list(lights)
        self.env, self.sky, self.background, self.phantom = env, sky, _v(background), phantom
        self.cam_max_depth = cam_max_depth
        self.dist = R.build_distribution(env["img"]) if env and env["importance"] else None


# ---------------------------------------------------------------------------
# hits over an interval, with the margins of every comparison made
# ---------------------------------------------------------------------------
def _bound_ratio(t, bound, denom, exact):
    if math.isinf(bound):
        return INF
    along = abs(t - bound) / (MARGIN_T * max(1.0, abs(bound)))
    return along if exact else min(abs(t - bound) * abs(denom) / MARGIN_PLANE, along)


def quad_test(o, d, Q, u, v, tmin, tmax):
    """Quad.Hit (quad.go:44-71) over [tmin, tmax]: (hit or None, ratio).  hit as shade_ref.quad_hit."""
    n = R.unit(np.cross(u, v))
    denom = float(n @ d)
    if abs(denom) < 1e-8:
        return None, INF
    D = float(n @ Q)
    t = (D - float(n @ o)) / denom
    # the numerator D - n.o is exact in fp32: nothing to round
    exact = all(abs(c) in (0.0, 1.0) for c in n) and sum(1 for x in [D] + list(n * o) if x != 0.0) <= 1
    ratio = min(_bound_ratio(t, tmin, denom, exact), _bound_ratio(t, tmax, denom, exact))
    if not (tmin <= t <= tmax):
        # outside the interval by a margin: whether the point is interior no longer matters
        if ratio >= 1:
            return None, INF
        a, b = R.quad_uv(o + d * t, Q, u, v)
        return None, (ratio if (-MARGIN_AB < a < 1 + MARGIN_AB and -MARGIN_AB < b < 1 + MARGIN_AB) else INF)
    P = o + d * t
    a, b = R.quad_uv(P, Q, u, v)
    ab = min(abs(a), abs(a - 1), abs(b), abs(b - 1)) / MARGIN_AB
    if not (0 <= a <= 1 and 0 <= b <= 1):
        return None, ab
    front, N = R.face_normal(d, n)
    return (t, P, front, N, a, b), min(ratio, ab)


def sphere_test(o, d, c, r, tmin, tmax):
    """Sphere.Hit (sphere.go:63-94) over (tmin, tmax): (hit or None, ratio)."""
    assert tmin == 0.001
    b_imp = float(np.linalg.norm(np.cross(d, c - o)) / np.linalg.norm(d))
    ratio = abs(b_imp / r - 1.0) / MARGIN_EDGE
    h = R.sphere_hit(o, d, c, r)
    if h is None:
        return None, ratio
    t = h[0]
    ratio = min(ratio, abs(t - tmin) / MARGIN_T, INF if math.isinf(tmax) else abs(t - tmax) / (MARGIN_T * max(1.0, tmax)))
    if not t < tmax:        # the far root is farther still (Surrounds, interval.go:61-63)
        return None, ratio
    return h, ratio


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


def world_hit(scene, o, d, tmin, tmax, key, bounce, vol_dom):
    """HittableList.Hit over the world: (index, hit) of the closest hit or
    (None, None), the ratio of every comparison made, and whether a volume
    was among the hits of the interval.  hit: (t, P, front,
    N, u, v) (a volume: the arbitrary normal (1, 0, 0), front face)."""
    found, ratio = [], INF
    for k, ob in enumerate(scene.objects):
        if ob["kind"] == "quad":
            h, rt = quad_test(o, d, ob["Q"], ob["u"], ob["v"], tmin, tmax)
        elif ob["kind"] == "sphere":
            h, rt = sphere_test(o, d, ob["c"], ob["r"], tmin, tmax)
            h = h[:6] if h else None
        else:
            t, rt = volume_test(o, d, ob, tmin, tmax, rnd(*key, bounce, vol_dom, 0))
            h = (t, o + d * t, True, _v((1.0, 0.0, 0.0)), 0.0, 0.0) if t is not None else None
        ratio = min(ratio, rt)
        if h:
            found.append((h[0], k, h))
    if not found:
        return None, None, ratio, False
    by_vol = any(scene.objects[k]["kind"] == "volume" for _, k, _ in found)
    found.sort(key=lambda x: x[0])
    if len(found) > 1:
        ratio = min(ratio, (found[1][0] - found[0][0]) / max(found[0][0], 1e-30) / MARGIN_T)
    return found[0][1], found[0][2], ratio, by_vol


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
    """rayColorInternal (camera.go:443-518).  ray = (origin, direction), key =
    (seed, pixel, sample); fills `path` (a Path) with the bounces' records."""
    if depth <= 0:
        return np.zeros(3)
    o, d = ray
    path = path if path is not None else Path()
    k, h, ratio, _ = world_hit(scene, o, d, 0.001, INF, key, bounce, DOM_VOL)
    b = dict(o=o, d=d, obj=-1 if k is None else k, t=-1.0 if k is None else h[0], nee=None, ratio=ratio, ratio_shade=INF,
             allow=allow, depth=depth, Le=np.zeros(3), att=None)
    path.bounces.append(b)
    if k is None:
        b["Le"] = miss_colour(scene, d, depth)
        return b["Le"]
    t, P, front, N, u, v = h
    mat = scene.objects[k]["mat"]
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
        return att * ray_color(scene, (P, sd), depth - 1, True, key, path, bounce + 1)
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
    indirect = att * ray_color(scene, (P, sd), depth - 1, False, key, path, bounce + 1)
    return direct + indirect                                 # colorFromEmission is 0 for every scattering material


def trace(scene, cam, i, j, seed, sample, depth):
    """One pixel-sample: RayColor (camera.go:438-441) of GetRay's ray."""
    o, d, _, _ = R.get_ray(cam, i, j, seed, sample)
    path = Path()
    path.L = ray_color(scene, (o, d), depth, True, (seed, j * cam.image_width + i, sample), path)
    return path
