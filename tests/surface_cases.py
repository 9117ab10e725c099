"""The rows that hold rt_gather_surface to tests/surface_ref.py.  Each row is a
grid of at most 16 x 12 points on the Lambertian walls of a tests/path_cases.py
scene, with the wall's normal, or free-standing points in mid-air with a chosen
normal; depth and samples are the scene's row's (at most 5 samples).  The
points of a wall row are where the reference's own grid-camera rays (every
second column of the first 12 rows, sample 0) first meet a Lambertian quad,
rounded to float32: they lie wherever the camera sees a wall, a few ulps off
its plane like the points rt_trace_rays hands a bake, and not within EDGE of a
wall's edge.  A point's id is its pixel's index, so its key is that pixel's.

Every row asserts, on the reference alone, that the events it is there for
happen (its counts) and that at most path_cases.LEFT_OUT_CAP of its
point-samples are undecided by path_ref's margins.

`white(name, variant)` is the scene with every Lambertian wall made
SolidColor(1, 1, 1): the scenes of the defining equality with rt_ray_color."""
import copy

import numpy as np

from tests import path_cases as PC
from tests import path_ref as PR
from tests import shade_ref as R
from tests import surface_ref as SR

SEED = PC.SEED
GRID_W, GRID_H = 16, 12
EDGE = 0.02                                   # alpha, beta of a wall point stay this far inside (0, 1)


def _normal(ob):
    n = np.cross(ob["u"], ob["v"])
    return n / np.linalg.norm(n)


def wall_points(g, case, variant):
    """(P float32 (n, 3), N float32 (n, 3), ids): the grid described above."""
    sc = case.scene(variant)
    cam = case.camera(g, variant)
    P, N, ids = [], [], []
    for j in range(GRID_H):
        for i in range(0, 2 * GRID_W, 2):
            if i >= PC.GW:
                continue
            pix = j * PC.GW + i
            o, d, time, _ = R.get_ray(cam, i, j, SEED, 0)
            k, h, ratio, _ = PR.world_hit(sc, o, d, 0.001, PR.INF, (SEED, pix, 0), 0, PR.DOM_VOL, time)
            if k is None or ratio < 1:
                continue
            ob = sc.objects[k]
            if ob["kind"] != "quad" or ob["mat"]["kind"] != "lambertian":
                continue
            rel = h[1] - ob["Q"]
            al, be = float(rel @ ob["u"]) / float(ob["u"] @ ob["u"]), float(rel @ ob["v"]) / float(ob["v"] @ ob["v"])
            if not (EDGE < al < 1 - EDGE and EDGE < be < 1 - EDGE):
                continue
            n = _normal(ob)
            P.append(np.float32(h[1]))
            N.append(np.float32(n if float(n @ d) < 0 else -n))
            ids.append(pix)
    return np.array(P, np.float32), np.array(N, np.float32), np.array(ids, np.uint32)


def _air_points(g, case, variant):
    """Free-standing points about clamp_b1's lamp (a 0.2 x 0.2 quad at z = 1.5
    that faces -z... and shines both ways: cosLight is an absolute value): a
    6 x 4 grid 0.3 in front of it facing it (the clamp), the same grid facing
    away (cos <= 0), a grid at z = 0 under tilted normals that are not unit,
    and a column far off to the side."""
    P, N = [], []
    for j in range(4):
        for i in range(6):
            x, y = -0.25 + 0.1 * i, -0.15 + 0.1 * j
            P += [(x, y, 1.2), (x, y, 1.2), (4 * x, 4 * y, 0.0)]
            N += [(0, 0, 1), (0, 0, -1), (0.5 * (i - 2.5), 0.25 * (j - 1.5), 2.5)]
    for j in range(8):
        P.append((2.5, -1 + 0.25 * j, 1.0))
        N.append((-3, 0, 1))
    return np.array(P, np.float32), np.array(N, np.float32), np.arange(len(P), dtype=np.uint32) + 5000


def white(name, variant):
    """path_cases' scene with every Lambertian made SolidColor(1, 1, 1), as a
    path_cases.Case (build, camera) of its own."""
    base = PC.CASES[name]

    def scene(v):
        sc = copy.deepcopy(base.scene(v))
        for ob in sc.objects:
            if ob.get("mat", {}).get("kind") == "lambertian":
                ob["mat"] = PR.lambertian((1, 1, 1))
        return sc
    return PC.Case(name + "_white", scene, base.variants, base.check, group=base.group)


class Row:
    """name: the path_cases scene; variant; points(g, case, variant); check(row,
    e) -> counts, asserted.  group: path_cases' group (the radiance bar)."""

    def __init__(self, name, variant, check, points=wall_points, label=None):
        self.name, self.variant, self.check, self.points_fn = name, variant, check, points
        self.label = label or (f"{name}-{variant}" if variant else name)
        self.case = PC.CASES[name]
        self.group = self.case.group
        self.depth, self.samples = self.case.variants[variant]
        self._exp = None

    def build(self, g):
        self._builder, d, cam, ids = self.case.build(g, self.variant)      # (the builder owns the description's arrays)
        return d, cam

    def expected(self, g):
        """Computed once, read-only: P, N, ids; paths[s][k]; L (n, 3) the sum
        of the samples; L_ok (n): every sample of the point is decided;
        left_out; counts."""
        if self._exp is not None:
            return self._exp
        sc = self.case.scene(self.variant)
        P, N, ids = self.points_fn(g, self.case, self.variant)
        n = len(P)
        assert 0 < n <= GRID_W * GRID_H and self.samples <= 5
        e = dict(P=P, N=N, ids=ids, depth=self.depth, samples=self.samples, scene=sc, paths=[], L=np.zeros((n, 3)),
                 L_ok=np.ones(n, bool))
        left = 0
        for s in range(self.samples):
            paths = []
            for k in range(n):
                L, pa = SR.surface_color(sc, P[k], N[k], self.depth, (SEED, int(ids[k]), s))
                paths.append(pa)
                e["L"][k] += L
                if pa.margin < 1:
                    e["L_ok"][k] = False
                    left += 1
            e["paths"].append(paths)
        e["left_out"], e["compared"] = left, n * self.samples - left
        assert left <= PC.LEFT_OUT_CAP * n * self.samples, f"{self.label}: {left} of {n * self.samples} point-samples left out"
        e["counts"] = self.check(self, e)
        for v in e.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        self._exp = e
        return e

    def summary(self, g):
        e = self.expected(g)
        return (f"{self.label} depth {e['depth']} samples {e['samples']} points {len(e['P'])}: compared {e['compared']} "
                f"left_out {e['left_out']} counts {e['counts']}")


def _decided(e):
    for paths in e["paths"]:
        for pa in paths:
            if pa.margin >= 1 and pa.bounces:
                yield pa


def _vertex_counts(e):
    """What happens at the given vertex (bounce 0) and to the scattered ray."""
    c = {}

    def add(k, n=1):
        c[k] = c.get(k, 0) + n
    for pa in _decided(e):
        b0 = pa.bounces[0]
        assert b0["obj"] == -3 and not b0["Le"].any()
        nee = b0["nee"]
        if nee:
            a, h = nee["area"], nee["hdri"]
            add(f"chosen{nee['light']}")
            if e["scene"].objects[e["scene"].lights[nee["light"]]]["kind"] != "quad":
                assert not a["wanted"] and not a["con"].any()
                add("no_area_ray")
            elif not a["wanted"]:
                add("cos_cut")
            elif a["cut"]:
                assert not a["con"].any()
                add("coslight_cut")
            elif a["visible"]:
                add("area_vis")
                add("area_clamped", int(a["clamped"].any()))
            else:
                add("area_by_fog" if a["by_volume"] and e["scene"].objects[a["occluder"]]["kind"] == "volume" else "area_occ")
            if h is not None and h["wanted"]:
                add("hdri_vis" if h["visible"] else "hdri_occ")
        else:
            add("no_nee")
        for k, b in enumerate(pa.bounces[1:], 1):
            if b.get("light_hit"):
                if k == 1:                                  # the scattered ray itself: allow = not use_mis at the vertex
                    assert b["allow"] == (nee is None)
                assert b["allow"] or not b["Le"].any()
                add("light_hit_counted" if b["allow"] else "light_hit_dropped")
        if len(pa.bounces) > 1:
            add("scattered_traced")
    return c


def _need(row, c, *keys):
    for k in keys:
        assert c.get(k, 0) > 0, f"{row.label}: no {k} in {c}"
    return c


def _check(*keys):
    return lambda row, e: _need(row, _vertex_counts(e), *keys)


def _check_depth_cut(row, e):
    c = _need(row, _vertex_counts(e), "no_nee", "scattered_traced")
    # no lights: the scattered ray's miss colour counts (allow), and nothing else lights the point
    assert "light_hit_dropped" not in c and (e["L"][e["L_ok"]] > 0).any()
    return c


def _check_air(row, e):
    c = _need(row, _vertex_counts(e), "area_vis", "area_clamped", "cos_cut")
    assert not np.isclose(np.linalg.norm(e["N"], axis=1), 1.0).all()      # normals that are not unit
    return c


ROWS = [
    Row("room", "d1", _check("area_vis", "area_occ")),                       # direct only: depth 1
    Row("room", "d2", _check("area_vis", "area_occ", "light_hit_dropped")),
    Row("room", "d6", _check("area_vis", "area_occ", "light_hit_dropped")),
    Row("lights3", "", _check("chosen0", "chosen1", "chosen2", "area_vis")),
    Row("clamp_b1", "", _check("area_vis", "scattered_traced")),
    Row("sphere_in_list", "", _check("no_area_ray", "area_vis", "light_hit_dropped")),
    Row("checker_light", "", _check("area_vis")),
    Row("env_is_area", "", _check("hdri_vis", "hdri_occ", "area_vis", "area_occ")),
    Row("edge_on", "", _check("coslight_cut", "area_vis")),
    Row("fog_shadow", "", _check("area_by_fog", "area_vis")),
    Row("depth_cut", "d2", _check_depth_cut),
    Row("depth_cut", "d3", _check_depth_cut),
    Row("clamp_b1", "", _check_air, points=_air_points, label="mid_air"),
]
BY_LABEL = {r.label: r for r in ROWS}
