"""The scenes that hold shading to tests/shade_ref.py: one small frame per
row, built with the Builder, and per row the expected rays, branches and
radiance worked out in float64 from the Go text alone (shade_ref).  Every row
first asserts, on the reference alone, that it is what it claims to be (its
branches, texels, seam / pole pixels, rejected disk tries), and that the
pixels it cannot decide (MARGINS) are at most LEFT_OUT_CAP of the frame.

Three consumers: tests/test_shade_kat.py (the oracle in both modes, and the
production shade_path on the host), tests/test_gpu_shade_kat.py (the C-ABI).

The grid camera: 24 x 16 pixels from the origin, pixel00 (-1.15, 0.75, -1),
0.1 per pixel: incidence 0 to 55 degrees on a plane z = const."""
import math

import numpy as np

from tests import shade_ref as R
from tests.kat_cases import DOM_VOL, VOL_RHO, random_unit_vector, rnd, straight_camera
from tests.scene_builder import Builder, defocus_pinhole, pinhole

SEED = 3
SAMPLE = 0
GW, GH = 24, 16

# A pixel is left out of a comparison when float64 decides it by less than this
MARGIN_BRANCH = 1e-5      # |ri sin(theta) - 1|, |reflectance - U|, |dot(sd, N)|
MARGIN_DISK = 1e-6        # |x^2 + y^2 - 1| on any disk try up to the accepted one
MARGIN_TEXEL = 1e-4       # distance of an image lookup to a texel border, in texels
MARGIN_CDF = 1e-6         # distance of an HDRI xi to a CDF entry (fp32 CDF, xi a multiple of 2^-24)
MARGIN_EDGE = 1e-3        # relative distance to a silhouette (sphere, circle rim) or a shared triangle edge
MARGIN_FLIGHT = 1e-4      # a free flight within this (relative) of the distance inside the medium
LEFT_OUT_CAP = 0.02

WALL = ((-10, -10, -3), (20, 0, 0), (0, 20, 0))
WALL_REV = ((-10, -10, -3), (0, 20, 0), (20, 0, 0))
METAL_ALBEDO = (0.8, 0.6, 0.2)
ISO_ALBEDO = (0.7, 0.5, 0.3)
TEX_QUAD = ((-4, -3, -3), (8, 0, 0), (0, 6, 0))
NOISE_SCALE = 4.0
SPHERE_C, SPHERE_R = (0.0, 0.0, -3.0), 2.0
CIRCLE_C, CIRCLE_N, CIRCLE_R = (0.0, 0.0, -3.0), (0.0, 0.0, 1.0), 3.0
INST_SIN, INST_COS, INST_OFF = 0.6, 0.8, (0.0, 0.0, -3.0)
MOVING_C, MOVING_R, MOVING_VEL = (0.0, 0.0, -3.0), 1.5, (0.4, 0.2, 0.0)
FLOOR_ALBEDO = (0.5, 0.25, 0.125)
ENV_IS_N = 64
DISK_U, DISK_V = (0.05, 0, 0), (0, 0.05, 0)


def grid_camera(g, depth, bg=(0, 0, 0), look="-z", defocus=False):
    """The grid camera along -z, or turned to look along +x, -x or +y."""
    p00, du, dv = {"-z": ((-1.15, 0.75, -1), (0.1, 0, 0), (0, -0.1, 0)),
                   "+x": ((1, 0.75, -1.15), (0, 0, 0.1), (0, -0.1, 0)),
                   "-x": ((-1, 0.75, 1.15), (0, 0, -0.1), (0, -0.1, 0)),
                   "+y": ((-1.15, 1, -0.75), (0.1, 0, 0), (0, 0, 0.1))}[look]
    if defocus:
        return defocus_pinhole(g, GW, GH, (0, 0, 0), p00, du, dv, 1.0, DISK_U, DISK_V, max_depth=depth, bg=bg)
    return pinhole(g, GW, GH, (0, 0, 0), p00, du, dv, max_depth=depth, bg=bg)


def perlin_tables():
    """numpy.random.default_rng(7): three permutations of 0..255, then 256 unit vectors."""
    rng = np.random.default_rng(7)
    perms = [rng.permutation(256) for _ in range(3)]
    v = rng.normal(size=(256, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v, perms[0], perms[1], perms[2]


def image_4x3():
    """Twelve distinct texels, every channel a multiple of 1/16 (exact in fp32)."""
    k = np.arange(12)
    img = np.stack([(k + 1) / 16.0, (12 - k) / 16.0, ((k * 5) % 12 + 1) / 16.0], axis=1).reshape(3, 4, 3)
    assert len({tuple(t) for t in img.reshape(12, 3)}) == 12
    return img


def env_8x4(f32_texel=False, black_col0=False):
    """8 x 4 texels in [0.25, 4], each (m + 0.5) 2^(e - 136) with one e per
    texel (rgbeToColor image_loader.go:364-383); with f32_texel one texel is
    not of that form (its channels are still exact in fp32); with black_col0
    every row starts with a black texel (RGBE's e = 0)."""
    rng = np.random.default_rng(11)
    img = np.zeros((4, 8, 3))
    for y in range(4):
        for x in range(8):
            e = int(rng.integers(135, 138))                       # scale 2^-1, 1, 2
            lo, hi = math.ceil(0.25 / 2.0 ** (e - 136) - 0.5), math.floor(4.0 / 2.0 ** (e - 136) - 0.5)
            m = rng.integers(max(lo, 0), min(hi, 255) + 1, size=3)
            img[y, x] = (m + 0.5) * 2.0 ** (e - 136)
    if f32_texel:
        img[1, 3] = [float(np.float32(1.0 / 3.0)), float(np.float32(0.7)), float(np.float32(1.1))]
    assert img.min() >= 0.25 and img.max() <= 4.0
    if black_col0:
        img[:, 0] = 0.0
    return img


class Case:
    """name; build(g, variant) -> (builder, desc, camera); expected(g) -> dict;
    sample: the sample index the row runs at; quant8: also run with RT_NODES_QUANT8."""

    def __init__(self, name, build, expect, variants=("",), quant8=False, sample=SAMPLE):
        self.name, self._build, self._expect, self.variants, self.quant8 = name, build, expect, variants, quant8
        self.sample = sample
        self._exp = None

    def build(self, g, variant=""):
        return self._build(g, variant)

    def expected(self, g):
        """Computed once, read-only.  Keys (n = pixels, all per pixel):
        counts / compared / left_out: what the row is (printed by the tests);
        ray0, ray0_ok: the camera ray; t0, t0_ok: its hit distance;
        ended1, ended1_ok: the path has no bounce-1 ray;
        ray1, ray1_ok: the bounce-1 ray;
        L[variant], L_ok, L_depth[variant], L_kind ('exact', 'rounded': one fp32 rounding of a
        constant, or 'measured': the group's measured bar);
        nee (HDRI NEE rows): dict(dh, ch, traced) the HDRI shadow ray, its contribution, whether it is wanted."""
        if self._exp is None:
            e = self._expect(g, self)
            n = e["n"]
            left = np.zeros(n, bool)
            for k in [k for k in e if k.endswith("_ok")]:
                left |= ~e[k]
            e["left_out"] = int(left.sum())
            e["compared"] = n - e["left_out"]
            assert e["left_out"] <= LEFT_OUT_CAP * n, f"{self.name}: {e['left_out']} of {n} pixels left out"
            for v in e.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._exp = e
        return self._exp

    def summary(self, g):
        e = self.expected(g)
        return f"{self.name}: compared {e['compared']} left_out {e['left_out']} counts {e['counts']}"


def _rays(cam, sample=SAMPLE):
    """The reference's camera rays of the frame: (o (n, 3), d (n, 3), time (n), disk margins per pixel)."""
    W, H = cam.image_width, cam.image_height
    o, d, tm, mg = np.zeros((W * H, 3)), np.zeros((W * H, 3)), np.zeros(W * H), []
    for j in range(H):
        for i in range(W):
            p = j * W + i
            o[p], d[p], tm[p], m = R.get_ray(cam, i, j, SEED, sample)
            mg.append(m)
    return o, d, tm, mg


# ---------------------------------------------------------------------------
# metal, glass, defocus: the wall
# ---------------------------------------------------------------------------
def _wall_scene(mat_of, wall=WALL, defocus=False, depth=2):
    def build(g, variant):
        b = Builder(g)
        q = b.quad(*wall, mat_of(b))
        return b, b.desc(b.listing([q])), grid_camera(g, depth, defocus=defocus)
    return build


def _metal_expect(fuzz, absorbed_want):
    def expect(g, case):
        cam = grid_camera(g, 2)
        o, d, _, _ = _rays(cam)
        n = len(o)
        e = dict(n=n, t0=np.zeros(n), t0_ok=np.ones(n, bool), ray1=np.zeros((n, 6)), ray1_ok=np.ones(n, bool),
                 ended1=np.zeros(n, bool), ended1_ok=np.ones(n, bool))
        for p in range(n):
            t, P, front, N, _, _ = R.quad_hit(o[p], d[p], *WALL)
            assert front and N[2] == 1.0
            sd, dot = R.metal_scatter(d[p], N, fuzz, random_unit_vector(SEED, p, SAMPLE, 0))
            e["t0"][p] = t
            e["ray1"][p] = np.concatenate([P, sd])
            e["ended1"][p] = dot <= 0
            if abs(dot) < MARGIN_BRANCH:
                e["ended1_ok"][p] = e["ray1_ok"][p] = False
        e["ray1_cmp"] = ~e["ended1"] & e["ended1_ok"]
        absorbed = int(e["ended1"].sum())
        e["counts"] = dict(absorbed=absorbed, scattered=n - absorbed)
        assert absorbed == absorbed_want, f"{case.name}: {absorbed} absorbed"
        return e
    return expect


def _glass_expect(wall, front_want, counts_want, ior=1.5, camera=None, tie=None):
    """tie = (pixel, reflectance): that pixel's Fresnel draw equals its
    reflectance exactly, both exact in fp32 and fp64, so the `>` of
    material.go:180 decides it (refract) with no margin."""
    def expect(g, case):
        cam = camera(g) if camera else grid_camera(g, 2)
        o, d, _, _ = _rays(cam, case.sample)
        n = len(o)
        e = dict(n=n, t0=np.zeros(n), t0_ok=np.ones(n, bool), ray1=np.zeros((n, 6)), ray1_ok=np.ones(n, bool),
                 ended1=np.zeros(n, bool), ended1_ok=np.ones(n, bool), branch=[])
        for p in range(n):
            t, P, front, N, _, _ = R.quad_hit(o[p], d[p], *wall)
            assert front == front_want and N[2] == 1.0
            u = rnd(SEED, p, case.sample, 0, R.DOM_FRESNEL, 0)
            sd, br, (m_tir, m_fr) = R.dielectric_scatter(d[p], N, front, ior, u)
            if tie and p == tie[0]:
                assert u == tie[1] and m_fr == 0.0 and br == "refract", (u, m_fr, br)
                assert float(np.float32(tie[1])) == tie[1] and float(np.float32(ior)) == ior
                m_fr = math.inf                                       # an exact tie of exact numbers: decided
            e["t0"][p] = t
            e["ray1"][p] = np.concatenate([P, sd])
            e["branch"].append(br)
            if abs(m_tir) < MARGIN_BRANCH or (m_tir < 0 and abs(m_fr) < MARGIN_BRANCH):
                e["ray1_ok"][p] = False
        e["ray1_cmp"] = e["ray1_ok"].copy()
        e["counts"] = {k: e["branch"].count(k) for k in ("tir", "reflect", "refract")}
        assert counts_want is None or e["counts"] == counts_want, f"{case.name}: {e['counts']}"
        return e
    return expect


def _defocus_expect(g, case):
    cam = grid_camera(g, 2, defocus=True)
    o, d, _, mg = _rays(cam)
    n = len(o)
    e = dict(n=n, ray0=np.concatenate([o, d], axis=1), ray0_ok=np.ones(n, bool), t0=np.zeros(n), t0_ok=np.ones(n, bool))
    for p in range(n):
        e["t0"][p] = R.quad_hit(o[p], d[p], *WALL)[0]
        if min(abs(m) for m in mg[p]) < MARGIN_DISK:
            e["ray0_ok"][p] = e["t0_ok"][p] = False
    tries = np.array([len(m) for m in mg])
    e["counts"] = dict(first_try_rejected=int((tries > 1).sum()), max_tries=int(tries.max()))
    assert 0.15 * n < e["counts"]["first_try_rejected"] < 0.30 * n and tries.max() <= 4, e["counts"]   # 1 - pi/4 = 21.5 %
    assert (np.abs(o[:, :2]).max(axis=1) > 0).all() and (o[:, 2] == 0).all()
    return e


# ---------------------------------------------------------------------------
# iso: the slab medium of kat_cases.volume_scene under the grid camera
# ---------------------------------------------------------------------------
SLAB_FRONT = ((-1, -1, -2), (2, 0, 0), (0, 2, 0))
SLAB_BACK = ((-1, -1, -4), (2, 0, 0), (0, 2, 0))
BACK_WALL = ((-5, -5, -10), (10, 0, 0), (0, 10, 0))


def _plane_t(o, d, quad):
    """Quad.Hit over the universe interval: t or None."""
    h = R.quad_hit(o, d, *quad, tmin=-math.inf)
    return h[0] if h else None


def slab_volume_hit(o, d, u_flight, tmin=0.001):
    """Volume.Hit (volume.go:34-79) for the slab's two-quad boundary list:
    (t or None, margin): margin = the relative distance of the free flight to
    the distance inside (inf where no flight is compared)."""
    ts = [t for t in (_plane_t(o, d, SLAB_FRONT), _plane_t(o, d, SLAB_BACK)) if t is not None]
    if not ts:
        return None, math.inf
    t1 = min(ts)                                             # HittableList.Hit keeps the closest of the interval
    later = [t for t in ts if t >= t1 + 0.0001]
    if not later:
        return None, math.inf
    t2 = min(later)
    t1 = max(t1, tmin)
    if t1 >= t2:
        return None, math.inf
    t1 = max(t1, 0.0)
    ln = math.sqrt(float(d @ d))
    inside = (t2 - t1) * ln
    hd = -math.log(u_flight) / VOL_RHO if u_flight > 0 else math.inf
    margin = abs(hd - inside) / inside
    return (None if hd > inside else t1 + hd / ln), margin


def _iso_build(g, variant):
    b = Builder(g)
    wm = b.lambertian((0.5, 0.5, 0.5))
    boundary = b.listing([b.quad(*SLAB_FRONT, wm), b.quad(*SLAB_BACK, wm)])
    vol = b.volume(boundary, VOL_RHO, b.mat(g.RT_ISOTROPIC, b.solid(ISO_ALBEDO)))
    back = b.quad(*BACK_WALL, wm)
    return b, b.desc(b.listing([vol, back])), grid_camera(g, 2, bg=(1, 1, 1))


def _iso_expect(g, case):
    cam = grid_camera(g, 2, bg=(1, 1, 1))
    o, d, _, _ = _rays(cam)
    n = len(o)
    e = dict(n=n, t0=np.zeros(n), t0_ok=np.ones(n, bool), ray1=np.zeros((n, 6)), ray1_ok=np.ones(n, bool),
             L={"": np.zeros((n, 3))}, L_ok=np.ones(n, bool), L_depth={"": 2}, L_kind="rounded")
    scat = np.zeros(n, bool)
    escaped = 0
    for p in range(n):
        t, m = slab_volume_hit(o[p], d[p], rnd(SEED, p, SAMPLE, 0, DOM_VOL, 0))
        if m < MARGIN_FLIGHT:
            e["t0_ok"][p] = e["ray1_ok"][p] = e["L_ok"][p] = False
        if t is None:
            h = R.quad_hit(o[p], d[p], *BACK_WALL)                 # the back wall, or past it
            e["t0"][p] = h[0] if h else -1.0
            continue
        scat[p] = True
        P = o[p] + d[p] * t
        sd = random_unit_vector(SEED, p, SAMPLE, 0)                # Isotropic.Scatter (material.go:266-270)
        e["t0"][p] = t
        e["ray1"][p] = np.concatenate([P, sd])
        # bounce 1: the medium again, the back wall, or out to the white background
        t2, m2 = slab_volume_hit(P, sd, rnd(SEED, p, SAMPLE, 1, DOM_VOL, 0))
        if m2 < MARGIN_FLIGHT:
            e["L_ok"][p] = False
        if t2 is None and R.quad_hit(P, sd, *BACK_WALL) is None:
            e["L"][""][p] = ISO_ALBEDO
            escaped += 1
    e["ray1_cmp"] = scat & e["ray1_ok"]
    e["L_cmp"] = scat & e["L_ok"]          # radiance on the scattering pixels: albedo where bounce 1 leaves the scene, else 0
    e["counts"] = dict(scatter=int(scat.sum()), escaped=escaped)
    assert scat.sum() >= 6 and escaped >= 3, e["counts"]
    return e


# ---------------------------------------------------------------------------
# lambert_moving
# ---------------------------------------------------------------------------
def _moving_build(g, variant):
    b = Builder(g)
    s = b.sphere(MOVING_C, MOVING_R, b.lambertian((0.5, 0.5, 0.5)), vel=MOVING_VEL)
    return b, b.desc(b.listing([s])), grid_camera(g, 2)


def _moving_expect(g, case):
    cam = grid_camera(g, 2)
    o, d, tm, _ = _rays(cam)
    n = len(o)
    e = dict(n=n, t0=np.zeros(n), t0_ok=np.ones(n, bool), ray1=np.zeros((n, 6)), ray1_ok=np.ones(n, bool))
    hit = np.zeros(n, bool)
    for p in range(n):
        cen = np.array(MOVING_C) + np.array(MOVING_VEL) * tm[p]
        b_imp = np.linalg.norm(np.cross(d[p], cen - o[p])) / np.linalg.norm(d[p])
        if abs(b_imp / MOVING_R - 1) < MARGIN_EDGE:
            e["t0_ok"][p] = e["ray1_ok"][p] = False
        h = R.sphere_hit(o[p], d[p], MOVING_C, MOVING_R, MOVING_VEL, tm[p])
        if h is None:
            e["t0"][p] = -1.0
            continue
        hit[p] = True
        t, P, front, N = h[:4]
        assert front
        np.testing.assert_allclose(N, (P - cen) / MOVING_R, atol=1e-15)
        e["t0"][p] = t
        e["ray1"][p] = np.concatenate([P, N + random_unit_vector(SEED, p, SAMPLE, 0)])   # material.go:57-68
    e["ray1_cmp"] = hit & e["ray1_ok"]
    e["hit0"] = hit
    e["counts"] = dict(hit=int(hit.sum()), miss=int(n - hit.sum()))
    assert hit.sum() > 100 and tm.std() > 0.2 and (n - hit.sum()) > 50
    return e


# ---------------------------------------------------------------------------
# textures as emitter (depth 1) and as Lambertian (depth 2, white background)
# ---------------------------------------------------------------------------
def _textured_mat(b, tex, variant):
    return b.mat(b.g.RT_DIFFUSE_LIGHT, tex) if variant == "emit" else b.mat(b.g.RT_LAMBERTIAN, tex)


def _tex_camera(g, variant, look="-z"):
    return grid_camera(g, 1, look=look) if variant == "emit" else grid_camera(g, 2, bg=(1, 1, 1), look=look)


def _noise_build(g, variant):
    b = Builder(g)
    q = b.quad(*TEX_QUAD, _textured_mat(b, b.noise_texture(NOISE_SCALE, *perlin_tables()), variant))
    return b, b.desc(b.listing([q])), _tex_camera(g, variant)


def _noise_expect(variant):
    def expect(g, case):
        cam = _tex_camera(g, variant)
        o, d, _, _ = _rays(cam)
        n = len(o)
        tab = perlin_tables()
        L = np.zeros((n, 3))
        P = np.zeros((n, 3))
        for p in range(n):
            P[p] = R.quad_hit(o[p], d[p], *TEX_QUAD)[1]
            L[p] = R.noise_value(tab, NOISE_SCALE, P[p])
        e = dict(n=n, L={variant: L}, L_ok=np.ones(n, bool), L_depth={variant: 1 if variant == "emit" else 2},
                 L_kind="measured", group="noise")
        e["counts"] = dict(x_neg=int((P[:, 0] < 0).sum()), y_neg=int((P[:, 1] < 0).sum()),
                           octave7_reach=float(np.abs(P * NOISE_SCALE * 64).max()))
        # both signs of x and y; the seventh octave's lattice index leaves 0..255 on both sides (the & 255 wrap)
        assert (P[:, 0] < 0).any() and (P[:, 0] > 0).any() and (P[:, 1] < 0).any() and (P[:, 1] > 0).any()
        assert (P[:, :2] * NOISE_SCALE * 64).max() > 800 and (P[:, :2] * NOISE_SCALE * 64).min() < -800
        assert L[:, 0].std() > 0.1
        return e
    return expect


def image_16x12():
    """192 distinct texels, every channel a multiple of 1/64 (exact in fp32): columns a twelfth
    of a sphere's visible u range wide, so an offset or scale of u inside a 4 x 3 texel shows."""
    j, i = np.mgrid[0:12, 0:16]
    img = np.stack([(4 * i + 1) / 64.0, (4 * j + 3) / 64.0, ((7 * i + 3 * j) % 32 + 1) / 64.0], axis=2)
    assert len({tuple(t) for t in img.reshape(-1, 3)}) == 192
    return img


# Sphere rows: centre, the camera's look, the image, the RotateY (sin, cos) and Translate of an instance
SEAM_SIN, SEAM_COS = 0.96, 0.28            # the object's -x axis (u = 0 / 1, sphere.go:55-56) turned towards the camera
POLE_C = (0.0, 3.0, 0.0)                   # over the +y camera: the pole v = 0 (sphere.go:54) in the frame's middle
SPHERES = dict(sphere=dict(c=SPHERE_C, look="-z", image=image_4x3, rot=None),
               inst=dict(c=INST_OFF, look="-z", image=image_4x3, rot=(INST_SIN, INST_COS)),
               sphere_fine=dict(c=SPHERE_C, look="-z", image=image_16x12, rot=None),
               inst_seam=dict(c=INST_OFF, look="-z", image=image_16x12, rot=(SEAM_SIN, SEAM_COS)),
               sphere_pole=dict(c=POLE_C, look="+y", image=image_16x12, rot=None))


def _inst_to_object(p, is_dir, off, rot):
    q = np.array(p, float) if is_dir else np.array(p, float) - np.array(off)              # transform.go:93-102
    return R.rotate_y_in(q, rot[0], rot[1])                                                # transform.go:163-167


def _image_uv(kind, o, d):
    """(u, v, edge margin ok) of the camera ray's hit on the image case's
    object, or None for a miss."""
    if kind == "quad":
        h = R.quad_hit(o, d, *TEX_QUAD)
        return h[4], h[5], True
    if kind in SPHERES:
        sp = SPHERES[kind]
        if sp["rot"]:
            o, d = _inst_to_object(o, False, sp["c"], sp["rot"]), _inst_to_object(d, True, sp["c"], sp["rot"])
            c = (0.0, 0.0, 0.0)
        else:
            c = sp["c"]
        b_imp = np.linalg.norm(np.cross(d, np.array(c) - o)) / np.linalg.norm(d)
        ok = abs(b_imp / SPHERE_R - 1) >= MARGIN_EDGE
        h = R.sphere_hit(o, d, c, SPHERE_R)
        return (h[4], h[5], ok) if h else (None, None, ok)
    if kind == "tri":
        Q, u, v = (np.array(x, float) for x in TEX_QUAD)
        a, b = R.quad_uv(R.quad_hit(o, d, Q, u, v)[1], Q, u, v)
        ok = abs(a + b - 1) >= MARGIN_EDGE
        for tri in _triangles():
            h = R.tri_uv(o, d, *tri)
            if h:
                return h[1], h[2], ok
        raise AssertionError("image_tri: a ray misses both triangles")
    if kind == "circle":
        den = d[2]
        P = o + d * ((CIRCLE_C[2] - o[2]) / den)
        rr = np.linalg.norm(P - np.array(CIRCLE_C))
        ok = abs(rr / CIRCLE_R - 1) >= MARGIN_EDGE
        uv = R.circle_uv(P, CIRCLE_C, CIRCLE_N, CIRCLE_R)
        return (uv[0], uv[1], ok) if uv else (None, None, ok)
    raise KeyError(kind)


def _triangles():
    Q, u, v = (np.array(x, float) for x in TEX_QUAD)
    return [(Q, Q + u, Q + v), (Q + u + v, Q + v, Q + u)]


def _image_look(kind):
    return SPHERES[kind]["look"] if kind in SPHERES else "-z"


def _image_build(kind):
    def build(g, variant):
        b = Builder(g)
        img = SPHERES[kind]["image"]() if kind in SPHERES else image_4x3()
        m = _textured_mat(b, b.image_texture(img.shape[1], img.shape[0], img), variant)
        if kind == "quad":
            objs = [b.quad(*TEX_QUAD, m)]
        elif kind in SPHERES and not SPHERES[kind]["rot"]:
            objs = [b.sphere(SPHERES[kind]["c"], SPHERE_R, m)]
        elif kind == "tri":
            objs = [b.triangle(*t, m) for t in _triangles()]
        elif kind == "circle":
            objs = [b.circle(CIRCLE_C, CIRCLE_N, CIRCLE_R, m)]
        else:
            sp = SPHERES[kind]
            objs = [b.translate(b.rotate_y(b.sphere((0, 0, 0), SPHERE_R, m), *sp["rot"]), sp["c"])]
        return b, b.desc(b.listing(objs)), _tex_camera(g, variant, _image_look(kind))
    return build


# Texels a shape can show at all.  From the origin the sphere shows a cap of
# half-angle acos(2/3) = 48 degrees around its +z pole, cut further by the
# frame: u = (atan2(-z, x) + pi) / 2 pi stays in (0.13, 0.35), two of the four
# columns, and v = acos(-y) / pi in (0.30, 0.66), two of the three rows.
# image_inst's RotateY turns the object's frame by asin 0.6 = 36.9 degrees,
# u - 0.102: one column, which a lookup with the world-space normal would
# leave.  A triangle's barycentrics keep u + v <= 1, which excludes the three
# texels with (u >= 1/2, v >= 2/3) or (u >= 3/4, v >= 1/3).
# The three rows over the 16 x 12 image close what that leaves open: sphere_fine
# resolves u and v inside those 4 x 3 texels, inst_seam turns the u = 0 / 1 seam
# of atan2 into view, sphere_pole looks at the pole v = 0 with every u around it.
IMAGE_TEXELS = dict(quad=12, circle=12, tri=9, sphere=4, inst=2)


def _image_expect(kind):
    def expect(g, case):
        cam = _tex_camera(g, "emit", _image_look(kind))
        o, d, _, _ = _rays(cam)
        n = len(o)
        img = SPHERES[kind]["image"]() if kind in SPHERES else image_4x3()
        L = np.zeros((n, 3))
        ok = np.ones(n, bool)
        hit = np.zeros(n, bool)
        seen = set()
        for p in range(n):
            u, v, edge_ok = _image_uv(kind, o[p], d[p])
            ok[p] = edge_ok
            if u is None:
                continue
            hit[p] = True
            L[p], ij, border = R.image_value(img, u, v)
            seen.add(ij)
            if border < MARGIN_TEXEL:
                ok[p] = False
        e = dict(n=n, L_ok=ok, L_kind="exact", hit0=hit,
                 L={"emit": L, "albedo": np.where(hit[:, None], L, 1.0)},      # a miss shows the white background
                 L_depth={"emit": 1, "albedo": 2})
        e["counts"] = dict(texels=len(seen), on_object=int(hit.sum()))
        cols, rows = {ij[0] for ij in seen}, {ij[1] for ij in seen}
        if kind in IMAGE_TEXELS:
            assert len(seen) == IMAGE_TEXELS[kind], f"{case.name}: {len(seen)} texels"
        else:
            e["counts"].update(columns=sorted(cols), rows=sorted(rows))
        if kind == "sphere_fine":                     # u in (0.13, 0.35), v in (0.30, 0.66) at a sixteenth / twelfth
            assert cols == {2, 3, 4, 5} and rows == {4, 5, 6, 7, 8} and len(seen) == 20, e["counts"]
        if kind == "inst_seam":                       # both sides of the seam
            assert {0, 1, 14, 15} <= cols and len(cols) <= 10, e["counts"]
        if kind == "sphere_pole":                     # every u around the pole, and the pole's own row (v < 1/12)
            assert cols == set(range(16)) and 11 in rows, e["counts"]
        if kind == "quad":
            assert hit.all()
        return e
    return expect


# ---------------------------------------------------------------------------
# environment lookups and HDRI NEE
# ---------------------------------------------------------------------------
def _env_build(look, rotation, f32):
    def build(g, variant):
        b = Builder(g)
        back = {"+x": (-100, 0, 0), "-x": (100, 0, 0), "+y": (0, -100, 0)}[look]
        s = b.sphere(back, 1e-3, b.lambertian((0.5, 0.5, 0.5)))
        b.environment(env_8x4(f32), rotation)
        return b, b.desc(b.listing([s])), grid_camera(g, 1, look=look)
    return build


def _env_expect(look, rotation, f32):
    def expect(g, case):
        cam = grid_camera(g, 1, look=look)
        o, d, _, _ = _rays(cam)
        n = len(o)
        img = env_8x4(f32)
        L = np.zeros((n, 3))
        raw = np.zeros((n, 4), int)
        for p in range(n):
            L[p], raw[p] = R.env_sample(img, rotation, d[p])
        e = dict(n=n, L={"": L}, L_ok=np.ones(n, bool), L_depth={"": 1}, L_kind="measured", group="env",
                 env_rgbe=not f32)          # uploaded as RGBE words, or (one texel not of that form) as fp32 texels
        e["counts"] = dict(x0_neg=int((raw[:, 0] == -1).sum()), x1_wrap=int((raw[:, 1] == 8).sum()),
                           y0_neg=int((raw[:, 2] == -1).sum()), y1_over=int((raw[:, 3] == 4).sum()))
        if case.name == "env_nx":      # both sides of the seam: x0 = -1 (u just above 0) and x1 = 8 (u just below 1)
            assert e["counts"]["x0_neg"] > 0 and e["counts"]["x1_wrap"] > 0, e["counts"]
        if case.name == "env_py":
            assert e["counts"]["y0_neg"] > 0, e["counts"]
        return e
    return expect


def _env_is_build(rotation, black_col0=False):
    def build(g, variant):
        b = Builder(g)
        floor = b.quad((-5, 0, 5), (10, 0, 0), (0, 0, -10), b.lambertian(FLOOR_ALBEDO))
        lq = b.quad((-0.5, -1, -0.5), (1, 0, 0), (0, 0, 1), b.light((4.0, 4.0, 4.0)))
        b.lights = [lq]
        b.environment(env_8x4(black_col0=black_col0), rotation, importance=True)
        return b, b.desc(b.listing([floor, lq])), straight_camera(g, ENV_IS_N, (0, 1, 0), (0, -1, 0), 1)
    return build


def _env_is_expect(rotation, black_col0=False, tie=None):
    """tie = pixel: its xi2 is 0 and so is the row's first conditional CDF
    entry (a black texel's weight is 0 in any precision), so the `<=` of
    hdri.go:306 decides it (the search passes the black texel) with no margin."""
    def expect(g, case):
        n = ENV_IS_N
        img = env_8x4(black_col0=black_col0)
        dist = R.build_distribution(img)
        assert dist["marginal"][-1] == 1.0 or abs(dist["marginal"][-1] - 1) < 1e-15
        L = np.zeros((n, 3))
        dh = np.zeros((n, 3))
        ok = np.ones(n, bool)
        rows = []
        for p in range(n):
            xi1, xi2 = rnd(SEED, p, case.sample, 0, R.DOM_NEE, 3), rnd(SEED, p, case.sample, 0, R.DOM_NEE, 4)
            L[p], dh[p], (x, y), gaps = R.hdri_nee(img, dist, rotation, (0, 1, 0), (0, -1, 0), FLOOR_ALBEDO, xi1, xi2)
            rows.append(y)
            if tie is not None and p == tie:
                assert xi2 == 0.0 and dist["cond"][y][1] == 0.0 and dist["cond"][y][2] > MARGIN_CDF
                assert x == 1 and y < 2 and L[p].min() > 0, (x, y, L[p])
                gaps = (gaps[0], math.inf)                            # an exact tie with an exact 0: decided
            if min(gaps) < MARGIN_CDF:
                ok[p] = False
        above = sum(1 for y in rows if y < 2)
        e = dict(n=n, L={"": L}, L_ok=ok, L_depth={"": 1}, L_kind="measured", group="nee", env_rgbe=True,
                 nee=dict(dh=dh, ch=L, traced=L.any(axis=1)), t0=np.ones(n), t0_ok=np.ones(n, bool))
        e["counts"] = dict(rows_above=above, rows_below=n - above, rows=sorted(set(rows)))
        assert above > 0 and n - above > 0
        assert (L[[y >= 2 for y in rows]] == 0).all() and (L[[y < 2 for y in rows]] > 0).all()
        return e
    return expect


# Normal incidence on the back face of a Dielectric 3: ri = 3, cos(theta) = 1, reflectance = r0 = (2/4)^2 = 0.25
def _tie_glass_camera(g):
    return straight_camera(g, 8, (0, 0, 0), (0, 0, -1), 2)


def _tie_glass_build(g):
    b = Builder(g)
    q = b.quad(*WALL_REV, b.dielectric(3.0))
    return b, b.desc(b.listing([q])), _tie_glass_camera(g)


TIE_CDF_PIXEL, TIE_CDF_SAMPLE = 8, 3491665


def _lam(b):
    return b.lambertian((0.5, 0.5, 0.5))


ROT_100 = 100.0 * math.pi / 180.0          # SetRotation (hdri.go:51-53)

CASES = {c.name: c for c in [
    Case("metal_f0", _wall_scene(lambda b: b.metal(METAL_ALBEDO, 0.0)), _metal_expect(0.0, 0)),
    Case("metal_f03", _wall_scene(lambda b: b.metal(METAL_ALBEDO, 0.3)), _metal_expect(0.3, 0)),
    Case("metal_f1", _wall_scene(lambda b: b.metal(METAL_ALBEDO, 1.0)), _metal_expect(1.0, 48)),
    Case("glass_front", _wall_scene(lambda b: b.dielectric(1.5)),
         _glass_expect(WALL, True, dict(tir=0, reflect=14, refract=370))),
    Case("glass_back", _wall_scene(lambda b: b.dielectric(1.5), wall=WALL_REV),
         _glass_expect(WALL_REV, False, dict(tir=145, reflect=7, refract=232)), quant8=True),
    Case("iso", _iso_build, _iso_expect),
    Case("lambert_moving", _moving_build, _moving_expect),
    Case("noise_emit", lambda g, v: _noise_build(g, "emit"), _noise_expect("emit"), variants=("emit",)),
    Case("noise_albedo", lambda g, v: _noise_build(g, "albedo"), _noise_expect("albedo"), variants=("albedo",),
         quant8=True),
    Case("image_quad", _image_build("quad"), _image_expect("quad"), variants=("emit", "albedo")),
    Case("image_sphere", _image_build("sphere"), _image_expect("sphere"), variants=("emit", "albedo")),
    Case("image_tri", _image_build("tri"), _image_expect("tri"), variants=("emit", "albedo")),
    Case("image_circle", _image_build("circle"), _image_expect("circle"), variants=("emit", "albedo")),
    Case("image_inst", _image_build("inst"), _image_expect("inst"), variants=("emit", "albedo"), quant8=True),
    Case("image_sphere_fine", _image_build("sphere_fine"), _image_expect("sphere_fine"), variants=("emit", "albedo")),
    Case("image_inst_seam", _image_build("inst_seam"), _image_expect("inst_seam"), variants=("emit", "albedo")),
    Case("image_sphere_pole", _image_build("sphere_pole"), _image_expect("sphere_pole"), variants=("emit", "albedo")),
    Case("env_px", _env_build("+x", 0.0, False), _env_expect("+x", 0.0, False)),
    Case("env_nx", _env_build("-x", 0.0, False), _env_expect("-x", 0.0, False)),
    Case("env_py", _env_build("+y", 0.0, False), _env_expect("+y", 0.0, False)),
    Case("env_rot", _env_build("+x", ROT_100, False), _env_expect("+x", ROT_100, False)),
    Case("env_f32", _env_build("+x", 0.0, True), _env_expect("+x", 0.0, True)),
    Case("env_is", _env_is_build(0.0), _env_is_expect(0.0), quant8=True),
    Case("env_is_rot", _env_is_build(ROT_100), _env_is_expect(ROT_100)),
    Case("defocus", _wall_scene(_lam, defocus=True), _defocus_expect),
    # exact ties: the (pixel, sample) whose draw equals the other side of the comparison, found by a search
    # over samples (the draw is a 24-bit number; each row asserts the equality on the reference)
    Case("glass_tie", lambda g, v: _tie_glass_build(g),
         _glass_expect(WALL_REV, False, None, ior=3.0, camera=_tie_glass_camera, tie=(2, 0.25)), sample=1839552),
    Case("cdf_tie", _env_is_build(0.0, black_col0=True), _env_is_expect(0.0, black_col0=True, tie=TIE_CDF_PIXEL),
         sample=TIE_CDF_SAMPLE),
]}


# ---------------------------------------------------------------------------
# the comparisons, shared by the three consumers
# ---------------------------------------------------------------------------
def check_paths(case, e, rec0, rec1, atol, t_rtol):
    """rec0 = (top, t, ray) of bounce 0, rec1 = (top, ray) of bounce 1 (top -1
    a miss, -2 an ended path; ray (n, 6)), against the row's expected camera
    ray, hit distance, ended paths (exact) and bounce-1 ray."""
    top0, t0, ray0 = rec0
    top1, ray1 = rec1
    name = case.name
    if "ray0" in e:
        ok = e["ray0_ok"]
        np.testing.assert_allclose(np.asarray(ray0, np.float64)[ok], e["ray0"][ok], rtol=0, atol=atol, err_msg=f"{name}: camera ray")
    if "t0" in e:
        ok = e["t0_ok"]
        hit = e["t0"] > 0
        assert np.array_equal((np.asarray(top0) >= 0)[ok], hit[ok]), f"{name}: bounce-0 hit / miss"
        np.testing.assert_allclose(np.asarray(t0, np.float64)[ok & hit], e["t0"][ok & hit], rtol=t_rtol, err_msg=f"{name}: t")
    if "ended1" in e:
        ok = e["ended1_ok"]
        assert np.array_equal((np.asarray(top1) == -2)[ok], e["ended1"][ok]), f"{name}: ended paths"
    if "ray1" in e:
        cmp_ = e["ray1_cmp"]
        assert not (np.asarray(top1) == -2)[cmp_].any(), f"{name}: a path that scatters has ended"
        np.testing.assert_allclose(np.asarray(ray1, np.float64)[cmp_], e["ray1"][cmp_], rtol=0, atol=atol,
                                   err_msg=f"{name}: bounce-1 ray")


def radiance_error(e, variant, L, rtol=0.0):
    """Worst absolute error of the frame's radiance (n, 3) over the compared
    pixels, less rtol times the expected value: what an absolute bar is held
    against."""
    ok = e.get("L_cmp", e["L_ok"])
    want = e["L"][variant][ok]
    return float((np.abs(np.asarray(L, np.float64).reshape(-1, 3)[ok] - want) - rtol * np.abs(want)).max())
