"""A plain float64 restatement of what the path does after a hit, written from
the Go source alone (numpy / math, no ctypes): scattering, textures, the
environment and the lens.  Every function cites the reference file:line it
follows.  The random numbers are the project's counter RNG (DESIGN.md §3
"RNG", tests/kat_cases.py `rnd`), which replaces the reference's unseeded
math/rand: a draw is named by (bounce, domain, index).

Deliberate departures of the project from the Go text that the comparison
encodes:
  * `dir_to_uv` clamps d.y to [-1, 1] before the asin;
  * RandomUnitVector's lower bound 1e-160 is 0 in fp32 (kat_cases);
  * the defocus sample draws one disk point, not Go's two (camera.go:355 and
    :359: the first is dead, the counter RNG makes it free to drop);
  * SHADOW_END (the far end of an area-light shadow ray in fp32).

tests/shade_cases.py builds the scenes, tests/test_shade_kat.py holds the
oracle (both modes) and the production `shade_path` on the host to this
module, tests/test_gpu_shade_kat.py the GPU."""
import math

import numpy as np

from tests.kat_cases import rnd

DOM_CAMERA, DOM_SCATTER, DOM_FRESNEL, DOM_NEE = 0, 1, 2, 3   # DESIGN.md §3, dev_layout.h


def _v(x):
    return np.asarray(x, np.float64)


def unit(v):
    """Vec3.Unit (vec3.go:32-38)."""
    v = _v(v)
    l = math.sqrt(float(v @ v))
    return v if l == 0 else v * (1.0 / l)


# ---------------------------------------------------------------------------
# material.go, vec3.go
# ---------------------------------------------------------------------------
def reflect(v, n):
    """Reflect (vec3.go:106-108)."""
    v, n = _v(v), _v(n)
    return v - n * (2.0 * float(v @ n))


def refract(uv, n, eta):
    """Refract (vec3.go:110-117)."""
    uv, n = _v(uv), _v(n)
    cos_t = min(float(-uv @ n), 1.0)
    perp = (uv + n * cos_t) * eta
    par = n * -math.sqrt(abs(1.0 - float(perp @ perp)))
    return perp + par


def reflectance(cosine, ri):
    """Schlick (material.go:284-288)."""
    r0 = (1.0 - ri) / (1.0 + ri)
    r0 = r0 * r0
    return r0 + (1.0 - r0) * math.pow(1.0 - cosine, 5)


def metal_scatter(d, normal, fuzz, ruv):
    """Metal.Scatter (material.go:113-119): (direction, dot(direction, N));
    the path goes on iff the dot is > 0."""
    sd = unit(reflect(d, normal)) + _v(ruv) * fuzz
    return sd, float(sd @ _v(normal))


def dielectric_scatter(d, normal, front, ior, u_fresnel):
    """Dielectric.Scatter (material.go:164-188): (direction, branch, margins),
    branch one of 'tir' / 'reflect' / 'refract', margins = (ri sin(theta) - 1,
    reflectance - U): the signs that decide the branch."""
    ri = 1.0 / ior if front else ior
    ud = unit(d)
    cos_t = min(float(-ud @ _v(normal)), 1.0)
    sin_t = math.sqrt(1.0 - cos_t * cos_t)
    m_tir = ri * sin_t - 1.0
    m_fr = reflectance(cos_t, ri) - u_fresnel
    if m_tir > 0:
        return reflect(ud, normal), "tir", (m_tir, m_fr)
    if m_fr > 0:
        return reflect(ud, normal), "reflect", (m_tir, m_fr)
    return refract(ud, normal, ri), "refract", (m_tir, m_fr)


def unit_disk(seed, pixel, sample):
    """RandomInUnitDisk (vec3.go:66-77) on draws 3 + 2k, 4 + 2k of the camera
    domain: ((x, y) of the accepted try, [x^2 + y^2 - 1 of every try up to it])."""
    margins = []
    for k in range(64):
        x = -1.0 + 2.0 * rnd(seed, pixel, sample, 0, DOM_CAMERA, 3 + 2 * k)
        y = -1.0 + 2.0 * rnd(seed, pixel, sample, 0, DOM_CAMERA, 4 + 2 * k)
        margins.append(x * x + y * y - 1.0)
        if x * x + y * y < 1.0:
            return (x, y), margins
    raise AssertionError("unit_disk: no try accepted")


# ---------------------------------------------------------------------------
# camera.go
# ---------------------------------------------------------------------------
def get_ray(cam, i, j, seed, sample):
    """GetRay's static path (camera.go:368-388) for pixel (i, j): (origin,
    direction, time, disk margins).  Draws 0, 1 of the camera domain are the
    square sample (camera.go:346-352), draw 2 the time (camera.go:370)."""
    pix = j * cam.image_width + i
    ox = rnd(seed, pix, sample, 0, DOM_CAMERA, 0) - 0.5
    oy = rnd(seed, pix, sample, 0, DOM_CAMERA, 1) - 0.5
    time = rnd(seed, pix, sample, 0, DOM_CAMERA, 2)
    p = _v(list(cam.pixel00)) + _v(list(cam.pixel_delta_u)) * (i + ox) + _v(list(cam.pixel_delta_v)) * (j + oy)
    margins = []
    if cam.defocus_angle <= 0:
        o = _v(list(cam.center))
    else:
        (px, py), margins = unit_disk(seed, pix, sample)                 # camera.go:354-362
        o = _v(list(cam.center)) + _v(list(cam.defocus_disk_u)) * px + _v(list(cam.defocus_disk_v)) * py
    return o, p - o, time, margins


# ---------------------------------------------------------------------------
# primitives: hits and the (u, v) each hands to its texture
# ---------------------------------------------------------------------------
def face_normal(d, n):
    """SetFaceNormal (hittable.go:20-30): (front, the normal facing the ray)."""
    front = float(_v(d) @ _v(n)) < 0
    return front, (_v(n) if front else -_v(n))


def quad_uv(P, Q, u, v):
    """Quad.Hit's alpha, beta (quad.go:58-60, 81-82)."""
    P, Q, u, v = _v(P), _v(Q), _v(u), _v(v)
    n = np.cross(u, v)
    w = n * (1.0 / float(n @ n))                       # quad.go:29
    p = P - Q
    return float(w @ np.cross(p, v)), float(w @ np.cross(u, p))


def quad_hit(o, d, Q, u, v, tmin=0.001):
    """Quad.Hit (quad.go:44-71) over [tmin, inf): None or (t, P, front, N, alpha, beta)."""
    o, d, Q, u, v = _v(o), _v(d), _v(Q), _v(u), _v(v)
    n = unit(np.cross(u, v))
    denom = float(n @ d)
    if abs(denom) < 1e-8:
        return None
    t = (float(n @ Q) - float(n @ o)) / denom
    if not tmin <= t:
        return None
    P = o + d * t
    a, b = quad_uv(P, Q, u, v)
    if not (0 <= a <= 1 and 0 <= b <= 1):
        return None
    front, N = face_normal(d, n)
    return t, P, front, N, a, b


def sphere_uv(p):
    """getSphereUV (sphere.go:53-59) of the outward unit normal."""
    theta = math.acos(-p[1])
    phi = math.atan2(-p[2], p[0]) + math.pi
    return phi / (2 * math.pi), theta / math.pi


def sphere_hit(o, d, c, r, vel=(0, 0, 0), time=0.0):
    """Sphere.Hit (sphere.go:63-94): None or (t, P, front, N, u, v, outward)."""
    o, d = _v(o), _v(d)
    cen = _v(c) + _v(vel) * time                        # sphere.go:49-51
    oc = cen - o
    a = float(d @ d)
    h = float(d @ oc)
    cc = float(oc @ oc) - r * r
    disc = h * h - a * cc
    if disc < 0:
        return None
    sq = math.sqrt(disc)
    root = (h - sq) / a
    if not 0.001 < root:
        root = (h + sq) / a
        if not 0.001 < root:
            return None
    P = o + d * root
    out = (P - cen) * (1.0 / r)
    front, N = face_normal(d, out)
    uu, vv = sphere_uv(out)
    return root, P, front, N, uu, vv, out


def tri_uv(o, d, v0, v1, v2):
    """Triangle.Hit (triangle.go:57-104): None or (t, u, v), the barycentrics."""
    o, d, v0, v1, v2 = _v(o), _v(d), _v(v0), _v(v1), _v(v2)
    e1, e2 = v1 - v0, v2 - v0
    h = np.cross(d, e2)
    a = float(e1 @ h)
    if abs(a) < 1e-8:
        return None
    f = 1.0 / a
    s = o - v0
    u = f * float(s @ h)
    if u < 0.0 or u > 1.0:
        return None
    q = np.cross(s, e1)
    v = f * float(d @ q)
    if v < 0.0 or u + v > 1.0:
        return None
    t = f * float(e2 @ q)
    if not 0.001 <= t:
        return None
    return t, u, v


def circle_uv(P, c, n, r):
    """Circle.Hit's (u, v) (circle.go:58-71); None outside the radius (:47-51)."""
    P, c, n = _v(P), _v(c), unit(n)
    lp = P - c
    if math.sqrt(float(lp @ lp)) > r:
        return None
    if abs(n[1]) > 0.9:
        u = unit(np.cross([1.0, 0.0, 0.0], n))
    else:
        u = unit(np.cross([0.0, 1.0, 0.0], n))
    v = np.cross(n, u)
    return (float(lp @ u) / r + 1.0) * 0.5, (float(lp @ v) / r + 1.0) * 0.5


def rotate_y_in(p, s, c):
    """RotateY.Hit's map of the ray's origin / direction (transform.go:163-167)."""
    return np.array([c * p[0] - s * p[2], p[1], s * p[0] + c * p[2]])


# ---------------------------------------------------------------------------
# noise.go, texture.go
# ---------------------------------------------------------------------------
def perlin_noise(tab, p):
    """Perlin.Noise + perlinInterp (noise.go:29-51, 78-92).  tab = (randvec
    (256, 3), perm_x, perm_y, perm_z)."""
    rv, px, py, pz = tab
    fl = [math.floor(p[0]), math.floor(p[1]), math.floor(p[2])]
    u, v, w = p[0] - fl[0], p[1] - fl[1], p[2] - fl[2]
    i, j, k = int(fl[0]), int(fl[1]), int(fl[2])
    acc = 0.0
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                c = rv[int(px[(i + di) & 255]) ^ int(py[(j + dj) & 255]) ^ int(pz[(k + dk) & 255])]
                acc += ((di * u + (1 - di) * (1 - u)) * (dj * v + (1 - dj) * (1 - v)) * (dk * w + (1 - dk) * (1 - w))
                        * (c[0] * (u - di) + c[1] * (v - dj) + c[2] * (w - dk)))
    return acc


def perlin_turb(tab, p, depth=7):
    """Perlin.Turb (noise.go:53-63)."""
    acc, weight, q = 0.0, 1.0, _v(p).copy()
    for _ in range(depth):
        acc += weight * perlin_noise(tab, q)
        weight *= 0.5
        q = q * 2.0
    return abs(acc)


def noise_value(tab, scale, p):
    """NoiseTexture.Value (texture.go:81-85): the grey level."""
    p = _v(p)
    s = scale * p[2] + 10.0 * perlin_turb(tab, p * scale, 7)
    return 0.5 * (1.0 + math.sin(s))


# ---------------------------------------------------------------------------
# image_texture.go, image_loader.go
# ---------------------------------------------------------------------------
def clamp_int(x, low, high):
    """clamp (image_loader.go:112-120)."""
    if x < low:
        return low
    return x if x < high else high - 1


def image_value(img, u, v):
    """ImageTexture.Value (image_texture.go:26-41) over img (H, W, 3): (texel,
    (i, j), the distance of (u W, v H) to the nearest integer, in texels)."""
    H, W = img.shape[:2]
    u = min(max(u, 0.0), 1.0)
    v = 1.0 - min(max(v, 0.0), 1.0)
    x, y = u * W, v * H
    i, j = clamp_int(int(x), 0, W), clamp_int(int(y), 0, H)      # PixelData (image_loader.go:97-109)
    return img[j, i], (i, j), min(abs(x - round(x)), abs(y - round(y)))


def bilinear(img, u, v):
    """PixelDataBilinear (image_loader.go:399-436): (colour, (x0, x1, y0, y1)
    before the wrap and the clamp)."""
    H, W = img.shape[:2]
    px, py = u * W - 0.5, v * H - 0.5
    x0, y0 = int(math.floor(px)), int(math.floor(py))
    x1, y1 = x0 + 1, y0 + 1
    fx, fy = px - x0, py - y0
    raw = (x0, x1, y0, y1)
    x0, x1 = x0 % W, x1 % W                            # Python's % is the ((x % W) + W) % W of :418-419
    y0, y1 = clamp_int(y0, 0, H), clamp_int(y1, 0, H)
    c0 = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
    c1 = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
    return c0 * (1 - fy) + c1 * fy, raw


# ---------------------------------------------------------------------------
# hdri.go
# ---------------------------------------------------------------------------
def dir_to_uv(d, rotation):
    """DirectionToUV (hdri.go:75-94); d.y clamped to [-1, 1] (the project's
    departure: a unit vector's y can round past 1 in fp32)."""
    d = unit(d)
    phi = math.atan2(d[2], d[0])
    theta = math.asin(min(max(d[1], -1.0), 1.0))
    u = 0.5 + phi / (2 * math.pi)
    v = 0.5 - theta / math.pi
    u = u + rotation / (2 * math.pi)
    return u - math.floor(u), v


def uv_to_dir(u, v, rotation):
    """UVToDirection (hdri.go:97-113)."""
    u = u - rotation / (2 * math.pi)
    u = u - math.floor(u)
    phi = (u - 0.5) * 2 * math.pi
    theta = (0.5 - v) * math.pi
    ct = math.cos(theta)
    return np.array([ct * math.cos(phi), math.sin(theta), ct * math.sin(phi)])


def env_sample(img, rotation, d):
    """HDRIEnvironment.Sample (hdri.go:120-128)."""
    u, v = dir_to_uv(d, rotation)
    return bilinear(img, u, v)


def build_distribution(img):
    """BuildDistribution (hdri.go:145-224): dict(pdf (H*W), marginal (H+1),
    cond (H, W+1), total)."""
    H, W = img.shape[:2]
    pdf = np.zeros(H * W)
    cond = np.zeros((H, W + 1))
    rows = np.zeros(H)
    total = 0.0
    for y in range(H):
        v = (y + 0.5) / H
        sin_t = math.cos((0.5 - v) * math.pi)
        for x in range(W):
            c = img[y, x]
            wgt = (0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]) * sin_t
            if wgt < 0:
                wgt = 0.0
            pdf[y * W + x] = wgt
            rows[y] += wgt
            total += wgt
            cond[y, x + 1] = cond[y, x] + wgt
    for y in range(H):
        if rows[y] > 0:
            cond[y] /= rows[y]
    marg = np.zeros(H + 1)
    for y in range(H):
        marg[y + 1] = marg[y] + rows[y]
    if total > 0:
        marg /= total
        pdf /= total
    return dict(pdf=pdf, marginal=marg, cond=cond, total=total)


def search_cdf(cdf, xi):
    """searchCDF (hdri.go:300-322)."""
    n = len(cdf) - 1
    low, high = 0, n
    while low < high:
        mid = (low + high) // 2
        if cdf[mid + 1] <= xi:
            low = mid + 1
        else:
            high = mid
    if low >= n:
        low = n - 1
    return max(low, 0)


def env_pdf(img, dist, rotation, d):
    """HDRIEnvironment.PDF (hdri.go:262-297), importance sampling on."""
    H, W = img.shape[:2]
    u, v = dir_to_uv(d, rotation)
    x, y = clamp_int(int(u * W), 0, W), clamp_int(int(v * H), 0, H)
    sin_t = math.cos((0.5 - v) * math.pi)
    if sin_t < 1e-10:
        sin_t = 1e-10
    p = dist["pdf"][y * W + x] * float(W * H) / (2.0 * math.pi * math.pi * sin_t)
    return 1e-10 if p < 1e-10 else p


def hdri_nee(img, dist, rotation, normal, ray_d, attenuation, xi1, xi2):
    """SampleDirection (hdri.go:228-259) + sampleHDRILight (camera.go:565-607)
    with nothing in the shadow ray's way: (contribution, direction, (x, y),
    the distance of xi1 / xi2 to the nearest marginal / conditional CDF entry)."""
    H, W = img.shape[:2]
    y = search_cdf(dist["marginal"], xi1)
    x = search_cdf(dist["cond"][y], xi2)
    gaps = (float(np.abs(dist["marginal"] - xi1).min()), float(np.abs(dist["cond"][y] - xi2).min()))
    d = uv_to_dir((x + 0.5) / W, (y + 0.5) / H, rotation)
    emission = img[y, x]
    pdf_h = env_pdf(img, dist, rotation, d)
    cos_t = float(_v(normal) @ d)
    if cos_t <= 0:
        return np.zeros(3), d, (x, y), gaps
    wo_cos = float(_v(normal) @ d)                       # Lambertian.PDF (material.go:70-76)
    pdf_b = 0.0 if wo_cos < 0 else wo_cos / math.pi
    wgt = pdf_h / (pdf_h + pdf_b)
    con = emission * (cos_t / pdf_h * wgt) * _v(attenuation)
    return np.minimum(con, 20.0), d, (x, y), gaps
