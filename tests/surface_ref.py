"""rt_gather_surface a second time, in float64: `surface_color`, the Lambertian
branch of tests/path_ref.py's `ray_color` at bounce 0 entered with a given
vertex instead of a traced hit.  The point P and the normal N are the caller's;
the hit is a front face of a Lambertian of SolidColor(1, 1, 1), so att = 1 and
no emission is added; the scattered direction is unit(N) + the path's own
scatter draw of bounce 0 (Lambertian.Scatter, material.go:57-68); with lights
in the scene the light select, `sample_hdri` and `sample_area` run as at any
Lambertian hit and the path goes on at bounce 1 with depth - 1 and
allow = not use_mis (camera.go:502-517).  The ray time is the key's camera
draw 2 (camera.go:370), which a scattered ray inherits.

The reference's margins are carried along: the vertex's own decisions (light
select, cos(theta), cos(light), the clamp, every occluder of its shadow rays)
are bounce 0's `ratio_shade`, and the bounces after it are path_ref's own."""
import math

import numpy as np

from tests import path_ref as PR
from tests.kat_cases import random_unit_vector, rnd

INF = math.inf


def valid(P, N):
    """gather_point_valid: finite components, and a length of N that float32
    gives as neither 0 nor infinite (sqrtf((x*x + y*y) + z*z) in float32)."""
    P, N = np.asarray(P, np.float32), np.asarray(N, np.float32)
    if not (np.isfinite(P).all() and np.isfinite(N).all()):
        return False
    with np.errstate(over="ignore", under="ignore"):
        sq = N * N
        ln = np.sqrt(np.float32(np.float32(sq[0] + sq[1]) + sq[2]))
    return bool(ln != 0 and np.isfinite(ln))


def surface_color(scene, P, N, depth, key):
    """(L, path): the radiance of one sample of one point and its Path, whose
    first entry is the vertex (obj -3: given, not traced).  key = (seed, id,
    sample)."""
    path = PR.Path()
    P, N = np.asarray(P, np.float64), np.asarray(N, np.float64)
    if depth <= 0 or not valid(P, N):
        path.L = np.zeros(3)
        return path.L, path
    nh = N / math.sqrt(float(N @ N))
    time = rnd(*key, 0, PR.DOM_CAMERA, 2)
    b = dict(sub=-1, hit=None, o=P, d=nh, obj=-3, t=0.0, nee=None, ratio=INF, ratio_shade=INF, allow=True, depth=depth,
             Le=np.zeros(3), att=np.ones(3))
    path.bounces.append(b)
    sd = nh + random_unit_vector(*key, 0)
    if all(abs(c) < 1e-8 for c in sd):
        sd = nh
    b["scatter"] = (P, sd)
    att = np.ones(3)
    nl = len(scene.lights)
    if nl == 0:
        path.L = att * PR.ray_color(scene, (P, sd, time), depth - 1, True, key, path, 1)
        return path.L, path
    un = rnd(*key, 0, PR.DOM_NEE, 0) * nl
    li = min(int(un), nl - 1)
    if nl > 1:
        b["ratio_shade"] = min(abs(un - math.floor(un)), abs(math.floor(un) + 1 - un)) / PR.MARGIN_SELECT
    nee = dict(light=li, hdri=None, area=None)
    direct = np.zeros(3)
    if scene.env is not None and scene.env["importance"]:
        nee["hdri"], rt = PR.sample_hdri(scene, P, nh, att, key, 0)
        b["ratio_shade"] = min(b["ratio_shade"], rt)
        direct = direct + nee["hdri"]["con"]
    nee["area"], rt = PR.sample_area(scene, P, nh, att, li, key, 0)
    b["ratio_shade"] = min(b["ratio_shade"], rt)
    direct = direct + nee["area"]["con"]
    nee["direct"] = direct
    b["nee"] = nee
    path.L = direct + att * PR.ray_color(scene, (P, sd, time), depth - 1, False, key, path, 1)
    return path.L, path
