"""Scenes, rays and closed forms for the ray-query tests (rt_trace_rays /
rt_occluded), shared by the host emulation (tests/test_query_host.py) and the
GPU (tests/test_gpu_query.py).

Each check takes `trace(desc, rays, time, any)`: rays an array of rt_ray
(g.RAY_DTYPE); the result is the rt_ray_hit array (g.RAY_HIT_DTYPE) for any ==
False and the occlusion bytes for any == True.  Expected values are float64
closed forms of the numbers written here.

Tolerances: t rtol 2e-6 (tests/test_path_kat.py's bar for a hit distance),
normals atol 1e-5 (the project's fp32 bar); ids, material and flags exact.
tmin / tmax are kept away from exact hit distances: which end of the interval
is open is documented in include/rtgpu.h, not tested at the bit."""
import numpy as np

from tests.scene_builder import Builder

T_RTOL = 2e-6
N_ATOL = 1e-5
FRONT, INVALID = 1, 2
INF = float("inf")


# ---------------------------------------------------------------- five quads
QUAD_Z = (1.0, 2.0, 3.0, 4.0, 5.0)
RAY_O = np.array([[0.4, 0.3, 0.0], [0.25, 0.6, 0.0], [0.55, 0.45, 0.0]])
RAY_D = np.array([[0.01, 0.02, 1.0], [-0.015, 0.01, 1.0], [0.02, -0.03, 1.0]])   # slightly oblique, d.z = 1: t = z


def five_quads(g):
    """Five parallel unit quads at z = 1..5, materials 0..4; (desc, ids, keep)."""
    b = Builder(g)
    mats = [b.lambertian((0.1 * (k + 1), 0.5, 0.5)) for k in range(5)]
    ids = [b.quad((0, 0, z), (1, 0, 0), (0, 1, 0), mats[k]) for k, z in enumerate(QUAD_Z)]
    return b.desc(b.listing(ids)), ids, b


def check_intervals(g, trace):
    desc, ids, keep = five_quads(g)
    nr = len(RAY_O)
    # tmin between quad k and quad k + 1 (k = 0: before the first): the hit is quad k + 1
    for k in range(5):
        rays = g.make_rays(RAY_O, RAY_D, tmin=(0.001 if k == 0 else QUAD_Z[k - 1] + 0.5), tmax=INF)
        h = trace(desc, rays, 0.0, False)
        assert h["prim"].tolist() == [ids[k]] * nr and h["top"].tolist() == [ids[k]] * nr, (k, h)
        assert h["material"].tolist() == [k] * nr, (k, h["material"])
        np.testing.assert_allclose(h["t"].astype(np.float64), QUAD_Z[k], rtol=T_RTOL)
        assert trace(desc, rays, 0.0, True).tolist() == [1] * nr
    # ... and bounded above: between quads 2 and 3 with tmax before quad 3 nothing is left
    rays = g.make_rays(RAY_O, RAY_D, tmin=2.5, tmax=2.75)
    h = trace(desc, rays, 0.0, False)
    assert h["prim"].tolist() == [-1] * nr and h["t"].tolist() == [-1.0] * nr
    assert trace(desc, rays, 0.0, True).tolist() == [0] * nr
    # a tmax below the first quad: a miss, in full
    rays = g.make_rays(RAY_O, RAY_D, tmin=0.001, tmax=0.5)
    h = trace(desc, rays, 0.0, False)
    assert h["top"].tolist() == [-1] * nr and h["prim"].tolist() == [-1] * nr and h["material"].tolist() == [-1] * nr
    assert h["t"].tolist() == [-1.0] * nr and not h["n"].any() and not h["flags"].any()
    # any hit around the closest distance T = 1
    T = QUAD_Z[0]
    assert trace(desc, g.make_rays(RAY_O, RAY_D, 0.001, T * (1 - 2.0 ** -10)), 0.0, True).tolist() == [0] * nr
    assert trace(desc, g.make_rays(RAY_O, RAY_D, 0.001, T * (1 + 2.0 ** -10)), 0.0, True).tolist() == [1] * nr
    # an unnormalised direction: t is the ray parameter
    h = trace(desc, g.make_rays(RAY_O, 4.0 * RAY_D), 0.0, False)
    np.testing.assert_allclose(h["t"].astype(np.float64), QUAD_Z[0] / 4.0, rtol=T_RTOL)


# ---------------------------------------------------------------- hit records
SPH_C, SPH_R = np.array([0.0, 0.0, -5.0]), 1.0
QUAD = (np.array([3.0, -1.0, -4.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 2.0, 0.0]))      # normal +z
TRI = (np.array([-4.0, -1.0, -4.0]), np.array([-2.0, -1.0, -4.5]), np.array([-3.0, 1.0, -4.0]))


def record_scene(g):
    """A sphere (material 0), a quad (1) and a triangle (2), apart from each other."""
    b = Builder(g)
    m = [b.lambertian((0.8, 0.2, 0.2)), b.metal((0.7, 0.7, 0.7), 0.1), b.dielectric(1.5)]
    ids = [b.sphere(SPH_C, SPH_R, m[0]), b.quad(*QUAD, m[1]), b.triangle(*TRI, m[2])]
    return b.desc(b.listing(ids)), ids, b


def sphere_roots(o, d, c, r):
    oc = c - o
    a, h, cc = d @ d, d @ oc, oc @ oc - r * r
    sq = np.sqrt(h * h - a * cc)
    return (h - sq) / a, (h + sq) / a


def record_cases():
    """(name, o, d, object index, t, normal, front) in float64."""
    out = []
    o, d = np.array([0.2, 0.1, 0.0]), np.array([-0.03, 0.02, -1.0])
    t = sphere_roots(o, d, SPH_C, SPH_R)[0]
    out.append(("sphere-outside", o, d, 0, t, (o + t * d - SPH_C) / SPH_R, True))
    o, d = SPH_C + np.array([0.2, -0.1, 0.3]), np.array([0.5, 0.4, -0.6])
    t = sphere_roots(o, d, SPH_C, SPH_R)[1]
    out.append(("sphere-inside", o, d, 0, t, -(o + t * d - SPH_C) / SPH_R, False))
    n = np.array([0.0, 0.0, 1.0])
    o, d = np.array([3.5, 0.25, 0.0]), np.array([0.1, -0.05, -1.0])
    out.append(("quad-front", o, d, 1, 4.0, n, True))                  # against the normal: front face
    o, d = np.array([4.5, -0.5, -9.0]), np.array([-0.05, 0.1, 2.0])
    out.append(("quad-back", o, d, 1, 2.5, -n, False))
    tn = np.cross(TRI[1] - TRI[0], TRI[2] - TRI[0])
    tn /= np.linalg.norm(tn)
    o, d = np.array([-3.0, -0.25, 0.0]), np.array([0.01, 0.02, -1.0])
    t = ((TRI[0] - o) @ tn) / (d @ tn)
    front = d @ tn < 0
    out.append(("triangle", o, d, 2, t, tn if front else -tn, bool(front)))
    return out


def check_records(g, trace):
    desc, ids, keep = record_scene(g)
    cases = record_cases()
    rays = g.make_rays([c[1] for c in cases], [c[2] for c in cases])
    h = trace(desc, rays, 0.0, False)
    for k, (name, o, d, ob, t, n, front) in enumerate(cases):
        assert h["top"][k] == ids[ob] and h["prim"][k] == ids[ob], (name, h[k])
        assert h["material"][k] == ob, (name, h[k])                    # materials were added in object order
        assert h["flags"][k] == (FRONT if front else 0), (name, h[k])
        np.testing.assert_allclose(float(h["t"][k]), t, rtol=T_RTOL, err_msg=name)
        np.testing.assert_allclose(h["n"][k].astype(np.float64), n, atol=N_ATOL, err_msg=name)
        assert abs(np.linalg.norm(n) - 1.0) < 1e-12
    assert trace(desc, rays, 0.0, True).tolist() == [1] * len(cases)


# ---------------------------------------------------------------- moving sphere
MOV_C, MOV_V, MOV_R = np.array([-1.0, 0.25, -6.0]), np.array([2.0, 0.0, 0.5]), 0.75
TIMES = (0.0, 0.5, 1.0)


def moving_scene(g):
    b = Builder(g)
    s = b.sphere(MOV_C, MOV_R, b.lambertian((0.3, 0.3, 0.9)), vel=tuple(MOV_V))
    back = b.quad((-20, -20, -12), (40, 0, 0), (0, 40, 0), b.lambertian((0.5, 0.5, 0.5)))
    return b.desc(b.listing([s, back])), (s, back), b


def check_moving(g, trace):
    desc, (s, back), keep = moving_scene(g)
    for time in TIMES:
        c = MOV_C + time * MOV_V
        o = np.zeros((3, 3))
        d = np.array([c + [0.1, 0.05, 0.0], c + [-0.2, 0.1, 0.0], c + [0.0, -0.3, 0.0]])   # towards the centre at `time`
        h = trace(desc, g.make_rays(o, d), float(time), False)
        want = [sphere_roots(o[k], d[k], c, MOV_R)[0] for k in range(3)]
        assert h["prim"].tolist() == [s] * 3, (time, h)
        np.testing.assert_allclose(h["t"].astype(np.float64), want, rtol=T_RTOL, err_msg=f"time {time}")
        for k in range(3):
            np.testing.assert_allclose(h["n"][k].astype(np.float64), (o[k] + want[k] * d[k] - c) / MOV_R, atol=N_ATOL)
    # a ray at the time-0 centre's rim misses the sphere at time 1 and reaches the wall behind
    d = np.array([MOV_C + [0.0, 0.6, 0.0]])
    assert trace(desc, g.make_rays(np.zeros((1, 3)), d), 0.0, False)["prim"].tolist() == [s]
    assert trace(desc, g.make_rays(np.zeros((1, 3)), d), 1.0, False)["prim"].tolist() == [back]


# ---------------------------------------------------------------- invalid rays
def invalid_rays(g):
    """(rays, bad): five_quads' valid rays with one invalid ray after each."""
    nan = float("nan")
    bad = [((nan, 0.3, 0.0), (0.01, 0.02, 1.0), 0.001, INF),      # a NaN origin
           ((0.4, 0.3, 0.0), (0.01, INF, 1.0), 0.001, INF),       # an infinite direction
           ((0.4, 0.3, 0.0), (0.0, 0.0, 0.0), 0.001, INF),        # a zero direction
           ((0.4, 0.3, 0.0), (0.01, 0.02, 1.0), 2.0, 1.0),        # tmax < tmin
           ((0.4, 0.3, 0.0), (0.01, 0.02, 1.0), nan, INF),        # a NaN tmin
           ((0.4, 0.3, 0.0), (0.01, 0.02, 1.0), 0.001, nan),      # a NaN tmax
           ((0.4, -INF, 0.0), (0.01, 0.02, 1.0), 0.001, INF)]     # an infinite origin
    o, d, tmin, tmax, mask = [], [], [], [], []
    for k, (bo, bd, b0, b1) in enumerate(bad):
        v = k % len(RAY_O)
        o += [RAY_O[v], bo]; d += [RAY_D[v], bd]; tmin += [0.001, b0]; tmax += [INF, b1]; mask += [False, True]
    o.append(RAY_O[0]); d.append(RAY_D[0]); tmin.append(0.001); tmax.append(INF); mask.append(False)
    with np.errstate(invalid="ignore"):
        return g.make_rays(np.array(o), np.array(d), np.array(tmin), np.array(tmax)), np.array(mask)


def check_invalid(g, trace):
    """Invalid rays are misses with RT_HIT_INVALID_RAY; their neighbours'
    results are what they are without them.  (trace itself asserts that no
    error flag was raised.)"""
    desc, ids, keep = five_quads(g)
    rays, bad = invalid_rays(g)
    h, occ = trace(desc, rays, 0.0, False), trace(desc, rays, 0.0, True)
    alone, occ_alone = trace(desc, rays[~bad], 0.0, False), trace(desc, rays[~bad], 0.0, True)
    assert h[~bad].tobytes() == alone.tobytes() and alone["prim"].tolist() == [ids[0]] * int((~bad).sum())
    assert occ[~bad].tolist() == occ_alone.tolist() == [1] * int((~bad).sum())
    hb = h[bad]
    assert hb["flags"].tolist() == [INVALID] * int(bad.sum()), hb["flags"]
    assert hb["t"].tolist() == [-1.0] * len(hb) and hb["top"].tolist() == [-1] * len(hb) and hb["prim"].tolist() == [-1] * len(hb)
    assert hb["material"].tolist() == [-1] * len(hb) and not hb["n"].any()
    assert occ[bad].tolist() == [0] * int(bad.sum())
