"""The scenes that hold the path integral to tests/path_ref.py: NEE at every
bounce, the light-hit rule, depth, light selection, the clamp, area-light
geometry, shadow rays and the order of the adds.  One 24 x 16 frame per row
from shade_cases' grid camera at the origin, seed 3, up to 4 samples; every
row is plain data (path_ref.Scene) that `build` hands to the Builder, and
`expected` works the same data out in float64.  Each row asserts, on the
reference alone, that the events it is there for happen (its counts) and that
at most LEFT_OUT_CAP of its pixel-samples are left out (path_ref's margins).

Two consumers: tests/test_path_kat.py (the oracle in both modes, the
production wavefront pipeline and shade_path on the host) and
tests/test_gpu_path_kat.py (the C-ABI).

`edge_on` is not the issue's literal construction: the grid camera jitters
every pixel, so no column's rays have direction x exactly 0 and cosLight is
nowhere exactly 0.  The light stands in the plane x = 0 50 to 90 units behind
the camera instead, so cosLight = |P.x| / dist falls below 0.001 on the
middle of the wall (|P.x| under 0.05 to 0.09, part of columns 11 and 12) with
a margin, and the columns beside them are lit."""
import numpy as np

from tests import path_ref as P
from tests.scene_builder import Builder
from tests.shade_cases import GH, GW, env_8x4, grid_camera

SEED = 3
LEFT_OUT_CAP = 0.02
N = GW * GH

A_BACK, A_FLOOR, A_CEIL = (0.5, 0.25, 0.125), (0.75, 0.75, 0.25), (0.25, 0.5, 0.75)
A_LEFT, A_RIGHT, A_FRONT, A_BLOCK = (0.75, 0.125, 0.125), (0.125, 0.75, 0.125), (0.625, 0.375, 0.875), (0.375, 0.875, 0.5)
WALL = ((-10, -10, -3), (20, 0, 0), (0, 20, 0))           # faces +z, towards the camera


# ---------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------
def _room(variant):
    """x in [-2, 2], y in [-1.5, 1.5], z in [-4, 1], the camera inside.  The
    walls reach half a unit past each other, so no path leaks at an edge."""
    L = P.lambertian
    obs = [P.quad((-2.5, -2, -4), (5, 0, 0), (0, 4, 0), L(A_BACK), "back"),
           P.quad((-2.5, -1.5, 1.5), (5, 0, 0), (0, 0, -6), L(A_FLOOR), "floor"),
           P.quad((-2.5, 1.5, -4.5), (5, 0, 0), (0, 0, 6), L(A_CEIL), "ceiling"),
           P.quad((-2, -2, -4.5), (0, 0, 6), (0, 4, 0), L(A_LEFT), "left"),
           P.quad((2, -2, 1.5), (0, 0, -6), (0, 4, 0), L(A_RIGHT), "right"),
           P.quad((2.5, -2, 1), (-5, 0, 0), (0, 4, 0), L(A_FRONT), "front"),
           P.quad((-0.5, 1.45, -2.5), (1, 0, 0), (0, 0, 1), P.light((12, 10, 8)), "lamp"),
           P.quad((-1.7, 0.4, -3.2), (1.5, 0, 0), (0, 0, 1.6), L(A_BLOCK), "blocker")]
    return P.Scene(obs, lights=[6])


def _lights3(variant):
    """Three quad lights outside the camera's view over the wall z = -3: one
    facing it, one tilted, one with its back to it."""
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.quad((2.6, -0.5, -1.5), (0, 1, 0), (1, 0, 0), P.light((6, 6, 6)), "facing"),            # normal -z, area 1
           P.quad((-4.0, 1.4, -1.2), (1.5, 0, 0.5), (0, 0.5, 0), P.light((2, 8, 4)), "tilted"),
           P.quad((-1.0, -2.6, -1.0), (2, 0, 0), (0, 0.6, 0), P.light((9, 3, 1)), "back_to")]        # normal +z, area 1.2
    return P.Scene(obs, lights=[1, 2, 3])


def _clamp_b1(variant):
    """A wall behind the camera with a strong small light half a unit in front
    of it: bounce 0 is on the far wall (beta0 = A_BACK), bounce 1 lands near the light."""
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.quad((3, -3, 2), (-6, 0, 0), (0, 6, 0), P.lambertian((0.875, 0.625, 0.375)), "near_wall"),   # faces -z
           P.quad((-0.1, -0.1, 1.5), (0.2, 0, 0), (0, 0.2, 0), P.light((3000, 60, 3)), "lamp")]
    return P.Scene(obs, lights=[2])


def _sphere_in_list(variant):
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.sphere((-0.9, 0.3, -1.6), 0.6, P.light((3, 2, 1)), "ball"),
           P.quad((0.4, -0.2, -2.0), (0.6, 0, 0), (0, 0.6, 0), P.light((4, 4, 4)), "panel")]
    return P.Scene(obs, lights=[1, 2])


def _chain(variant):
    """wall -> a mirror (or a glass slab) behind the camera -> the light."""
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall")]
    if variant == "mirror":
        obs += [P.quad((4, -4, 1.5), (-8, 0, 0), (0, 8, 0), P.metal((0.75, 0.5, 0.25), 0.0), "mirror"),
                P.quad((3, -2, -2.5), (3, 0, 0), (0, 4, 0), P.light((5, 4, 3)), "lamp")]
        return P.Scene(obs, lights=[2])
    obs += [P.quad((2, -2, 1.0), (-4, 0, 0), (0, 4, 0), P.dielectric(1.5), "glass_in"),       # normal -z
            P.quad((-2, -2, 1.3), (4, 0, 0), (0, 4, 0), P.dielectric(1.5), "glass_out"),      # normal +z
            P.quad((4, -4, 2.0), (-8, 0, 0), (0, 8, 0), P.light((5, 4, 3)), "lamp")]
    return P.Scene(obs, lights=[3])


def _checker_light(variant):
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.quad((1.6, -1, -3), (0, 0, 2), (0, 2, 0), P.light_tex(P.checker(0.5, (6, 1, 1), (1, 1, 6))), "lamp")]
    return P.Scene(obs, lights=[1])


OPEN_WALL = ((-2, -1.5, -3), (4, 0, 0), (0, 3, 0))


def _env_gate(variant):
    kind, lit = variant.split("+") if "+" in variant else (variant, "")
    obs = [P.quad(*OPEN_WALL, P.lambertian(A_BACK), "wall")]
    lights = []
    if lit:
        obs.append(P.quad((3, -0.5, -1.5), (0, 1, 0), (0, 0, 1), P.light((4, 4, 4)), "lamp"))
        lights = [1]
    if kind == "env":
        return P.Scene(obs, lights, env=dict(img=env_8x4(), rotation=0.0, importance=False))
    if kind == "sky":
        return P.Scene(obs, lights, sky=True)
    return P.Scene(obs, lights, background=(0.25, 0.5, 0.875))


PHANTOM_CAM_DEPTH = 3


def _phantom(variant):
    obs = [P.quad(*OPEN_WALL, P.lambertian(A_BACK), "wall")]
    return P.Scene(obs, env=dict(img=env_8x4(), rotation=0.0, importance=False), phantom=True,
                   cam_max_depth=PHANTOM_CAM_DEPTH)


def _env_is_area(variant):
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.quad((2.6, -0.5, -1.5), (0, 1, 0), (1, 0, 0), P.light((6, 6, 6)), "lamp"),
           P.quad((-0.2, -1.0, -2.2), (1.6, 0, 0), (0, 2, 0), P.lambertian(A_BLOCK), "blocker"),
           P.quad((-3.6, -0.5, -1.5), (1, 0, 0), (0, 1, 0), P.light((3, 5, 7)), "lamp2")]
    return P.Scene(obs, lights=[1, 3], env=dict(img=env_8x4(), rotation=0.0, importance=True))


def _edge_on(variant):
    """A 40 x 40 light in the plane x = 0 behind the camera: seen from the wall
    z = -3 at |P.x| / dist, edge-on in the frame's middle."""
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.quad((0, -20, 50), (0, 40, 0), (0, 0, 40), P.light((300, 450, 600)), "lamp")]
    return P.Scene(obs, lights=[1])


def _depth_cut(variant):
    """No light: two walls that face each other under the sky gradient, so a
    path is still alive where the depth ends it."""
    obs = [P.quad(*OPEN_WALL, P.lambertian(A_BACK), "wall"),
           P.quad((3, -3, 2), (-6, 0, 0), (0, 6, 0), P.lambertian(A_FRONT), "behind")]
    return P.Scene(obs, sky=True)


def _fog_shadow(variant):
    obs = [P.quad(*WALL, P.lambertian(A_BACK), "wall"),
           P.slab(((-3, -3, -1), (6, 0, 0), (0, 6, 0)), ((-3, -3, -2), (6, 0, 0), (0, 6, 0)), 0.5, (0.75, 0.5, 0.25)),
           P.quad((2, -2, 1.0), (-4, 0, 0), (0, 4, 0), P.light((5, 5, 5)), "lamp")]
    return P.Scene(obs, lights=[2])


# ---------------------------------------------------------------------------
# a row
# ---------------------------------------------------------------------------
class Case:
    """name; scene(variant) -> path_ref.Scene; variants: {variant: (depth,
    samples)}; check(case, exp): the row's counts, asserted; quant8: also run
    with RT_NODES_QUANT8; tail: the variants without a light also run with the
    long-tail kernel taking every path after bounce 0 (the only place `cont`
    alone ends a path at the depth).  records(variant): whether the per-bounce
    records are compared too (not where the camera's MaxDepth differs from the
    depth rendered)."""

    def __init__(self, name, scene, variants, check, quant8=False, group="flat", tail=False):
        self.name, self.scene, self.variants, self.check, self.quant8, self.group = name, scene, variants, check, quant8, group
        self.tail = tail
        self._exp = {}

    def camera(self, g, variant):
        sc = self.scene(variant)
        depth = sc.cam_max_depth or self.variants[variant][0]
        cam = grid_camera(g, depth, bg=tuple(sc.background))
        cam.use_sky_gradient = 1 if sc.sky else 0
        cam.phantom_hdri = 1 if sc.phantom else 0
        return cam

    def records(self, variant):
        sc = self.scene(variant)
        return not sc.cam_max_depth or sc.cam_max_depth == self.variants[variant][0]

    def build(self, g, variant):
        """(builder, desc, camera, ids): ids[k] the hittable id of world object k."""
        sc = self.scene(variant)
        b = Builder(g)
        ids = []
        for ob in sc.objects:
            if ob["kind"] == "volume":
                wm = b.lambertian((0.5, 0.5, 0.5))
                faces = [b.quad(Q, u, v, wm) for Q, u, v in ob["faces"]]
                ids.append(b.volume(b.listing(faces), ob["rho"], b.mat(g.RT_ISOTROPIC, b.solid(ob["mat"]["tex"][1]))))
                continue
            m = ob["mat"]
            if m["kind"] in ("lambertian", "light"):
                t = m["tex"]
                tex = b.solid(t[1]) if t[0] == "solid" else b.checker(t[1], t[2], t[3])
                mat = b.mat(g.RT_LAMBERTIAN if m["kind"] == "lambertian" else g.RT_DIFFUSE_LIGHT, tex)
            elif m["kind"] == "metal":
                mat = b.metal(m["albedo"], m["fuzz"])
            else:
                mat = b.dielectric(m["ior"])
            ids.append(b.quad(ob["Q"], ob["u"], ob["v"], mat) if ob["kind"] == "quad" else b.sphere(ob["c"], ob["r"], mat))
        b.lights = [ids[k] for k in sc.lights]
        if sc.env is not None:
            b.environment(sc.env["img"], sc.env["rotation"], importance=sc.env["importance"])
        return b, b.desc(b.listing(ids)), self.camera(g, variant), ids

    def expected(self, g, variant):
        """Computed once, read-only.  depth, samples; paths[s][p]: the Path of
        pixel p's sample s; L (n, 3): the sum of the samples; L_ok (n): every
        sample of the pixel is decided; per sample s and bounce b (arrays
        [s][b] over pixels): obj (world index, -1 a miss, -2 the path has
        ended), t, ray (n, 6), hit_ok, nee (bits 0 / 1: the area / HDRI shadow
        ray wanted, 2 / 3: visible), nee_ok; nee_dev: the bits the device
        reports, which clears an area ray cut by cosLight < 0.001 before it
        queues it (the reference cuts after the shadow test); nee_lifted: those
        with a lifted volume, whose test runs in k_shade too, so a ray the fog
        stops is never traced either; counts, left_out, compared."""
        if variant in self._exp:
            return self._exp[variant]
        depth, samples = self.variants[variant]
        sc = self.scene(variant)
        cam = self.camera(g, variant)
        e = dict(depth=depth, samples=samples, scene=sc, paths=[], L=np.zeros((N, 3)), L_ok=np.ones(N, bool),
                 obj=[], t=[], ray=[], hit_ok=[], nee=[], nee_ok=[], nee_dev=[], nee_lifted=[])
        left = 0
        for s in range(samples):
            paths = [P.trace(sc, cam, p % GW, p // GW, SEED, s, depth) for p in range(N)]
            e["paths"].append(paths)
            obj, t = np.full((depth, N), -2, np.int32), np.full((depth, N), -1.0)
            ray, nee = np.zeros((depth, N, 6)), np.zeros((depth, N), np.int32)
            nee_dev, nee_lifted = np.zeros((depth, N), np.int32), np.zeros((depth, N), np.int32)
            hit_ok, nee_ok = np.zeros((depth, N), bool), np.zeros((depth, N), bool)
            for p, pa in enumerate(paths):
                e["L"][p] += pa.L
                if pa.margin < 1:
                    e["L_ok"][p] = False
                    left += 1
                nh, ns = pa.decided_hits(), pa.decided_shades()
                whole = pa.margin >= 1
                for k in range(depth):
                    # past the last ray the path has ended: known only where every decision before is
                    hit_ok[k, p] = k < nh or (k >= len(pa.bounces) and whole)
                    nee_ok[k, p] = k < ns or (k >= len(pa.bounces) and whole)
                for k, bn in enumerate(pa.bounces):
                    obj[k, p], t[k, p] = bn["obj"], bn["t"]
                    ray[k, p] = np.concatenate([bn["o"], bn["d"]])
                    if bn["nee"]:
                        a, h = bn["nee"]["area"], bn["nee"]["hdri"]
                        hb = h["wanted"] * 2 | h["visible"] * 8 if h else 0
                        nee[k, p] = a["wanted"] * 1 | a["visible"] * 4 | hb
                        ab = 0 if a["cut"] else a["wanted"] * 1 | a["visible"] * 4
                        nee_dev[k, p] = ab | hb
                        nee_lifted[k, p] = (0 if a["by_volume"] else ab) | (0 if h and h["by_volume"] else hb)
            for key, val in (("obj", obj), ("t", t), ("ray", ray), ("hit_ok", hit_ok), ("nee", nee), ("nee_ok", nee_ok),
                             ("nee_dev", nee_dev), ("nee_lifted", nee_lifted)):
                e[key].append(val)
        e["left_out"], e["compared"] = left, N * samples - left
        assert left <= LEFT_OUT_CAP * N * samples, f"{self.name}[{variant}]: {left} of {N * samples} pixel-samples left out"
        e["counts"] = self.check(self, variant, e)
        for v in e.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        self._exp[variant] = e
        return e

    def summary(self, g, variant):
        e = self.expected(g, variant)
        return (f"{self.name}[{variant}] depth {e['depth']} samples {e['samples']}: compared {e['compared']} "
                f"left_out {e['left_out']} counts {e['counts']}")


def _bounces(e):
    for paths in e["paths"]:
        for pa in paths:
            if pa.margin >= 1:
                for k, b in enumerate(pa.bounces):
                    yield pa, k, b


def _nee_counts(e):
    """Per bounce: area shadow rays visible / occluded, light hits dropped / counted."""
    c = {}
    for pa, k, b in _bounces(e):
        if b["nee"]:
            a = b["nee"]["area"]
            if a["wanted"]:
                c[f"b{k}_{'vis' if a['visible'] else 'occ'}"] = c.get(f"b{k}_{'vis' if a['visible'] else 'occ'}", 0) + 1
        if b.get("light_hit"):
            kind = "counted" if b["allow"] else "dropped"
            c[f"b{k}_light_{kind}"] = c.get(f"b{k}_light_{kind}", 0) + 1
    return c


def _need(case, variant, c, *keys):
    for k in keys:
        assert c.get(k, 0) > 0, f"{case.name}[{variant}]: no {k} in {c}"
    return c


def _check_room(case, variant, e):
    c = _nee_counts(e)
    depth = e["depth"]
    _need(case, variant, c, "b0_vis", "b0_occ")
    if depth >= 2:
        _need(case, variant, c, "b1_vis", "b1_occ", "b1_light_dropped")
    if depth >= 3:
        _need(case, variant, c, f"b{depth - 1}_vis", f"b{depth - 1}_occ")
        # NEE at the last bounce counts: some path's last bounce adds a visible contribution
        last = sum(1 for pa, k, b in _bounces(e) if k == depth - 1 and b["nee"] and b["nee"]["area"]["con"].any())
        c["last_bounce_nee"] = last
        assert last > 0
    assert "b0_light_dropped" not in c and not any(k.endswith("light_counted") and k != "b0_light_counted" for k in c), c
    return c


def _check_lights3(case, variant, e):
    c = _nee_counts(e)
    for pa, k, b in _bounces(e):
        if b["nee"]:
            li = b["nee"]["light"]
            c[f"chosen{li}"] = c.get(f"chosen{li}", 0) + 1
            if b["nee"]["area"]["con"].any():
                c[f"lit_by{li}"] = c.get(f"lit_by{li}", 0) + 1
    # lit_by2: the light with its back to the wall, abs() in cosLight
    return _need(case, variant, c, "chosen0", "chosen1", "chosen2", "lit_by0", "lit_by1", "lit_by2")


def _check_clamp(case, variant, e):
    c = dict(b1_some_clamped=0, b1_all_clamped=0, b1_none_clamped=0, b0_clamped=0)
    for pa, k, b in _bounces(e):
        if b["nee"] and b["nee"]["area"]["visible"]:
            cl = b["nee"]["area"]["clamped"]
            if k == 0:
                c["b0_clamped"] += int(cl.any())
            elif k == 1:
                c["b1_all_clamped" if cl.all() else "b1_some_clamped" if cl.any() else "b1_none_clamped"] += 1
    assert max(A_BACK) < 1 and c["b0_clamped"] == 0
    return _need(case, variant, c, "b1_some_clamped", "b1_none_clamped")


def _check_sphere_in_list(case, variant, e):
    c = _nee_counts(e)
    for pa, k, b in _bounces(e):
        if b["nee"]:
            a = b["nee"]["area"]
            if a["light"] == 0:
                assert not a["wanted"] and not a["con"].any()
                c["sphere_chosen"] = c.get("sphere_chosen", 0) + 1
            elif a["con"].any():
                c["quad_lit"] = c.get("quad_lit", 0) + 1
        if b.get("light_hit"):
            nm = e["scene"].objects[b["obj"]]["name"]
            c[f"b{k}_{nm}"] = c.get(f"b{k}_{nm}", 0) + 1
    assert "b1_light_counted" not in c
    return _need(case, variant, c, "sphere_chosen", "quad_lit", "b0_ball", "b0_panel", "b1_ball", "b1_panel", "b1_light_dropped")


def _check_chain(case, variant, e):
    c = _nee_counts(e)
    spec = sum(1 for pa, k, b in _bounces(e) if b.get("light_hit") and b["allow"] and k >= 2 and b["Le"].any())
    c["light_after_specular"] = spec
    assert spec > 0
    return _need(case, variant, c, "b1_light_dropped")


def _check_checker(case, variant, e):
    c = _nee_counts(e)
    sc = e["scene"]
    for pa, k, b in _bounces(e):
        if b.get("light_hit") and k == 0:
            key = "seen_even" if b["Le"][0] == 6 else "seen_odd"
            c[key] = c.get(key, 0) + 1
        if b["nee"] and b["nee"]["area"]["visible"]:
            key = "nee_even" if P.tex_value(sc.objects[1]["mat"]["tex"], b["nee"]["area"]["lp"])[0] == 6 else "nee_odd"
            c[key] = c.get(key, 0) + 1
    return _need(case, variant, c, "seen_even", "seen_odd", "nee_even", "nee_odd")


def _check_env_gate(case, variant, e):
    c = _nee_counts(e)
    c.update(b0_miss=0, b1_miss_allowed=0, b1_miss_not_allowed=0)
    for pa, k, b in _bounces(e):
        if b["obj"] == -1 and k == 0:
            c["b0_miss"] += 1
        elif b["obj"] == -1 and k == 1 and b["Le"].any():
            c["b1_miss_allowed" if b["allow"] else "b1_miss_not_allowed"] += 1
    return _need(case, variant, c, "b0_miss", "b1_miss_not_allowed" if "+" in variant else "b1_miss_allowed")


def _check_phantom(case, variant, e):
    c = dict(b0_miss_black=0, b0_miss_env=0, b1_miss_env=0)
    for pa, k, b in _bounces(e):
        if b["obj"] == -1:
            if k == 0:
                c["b0_miss_env" if b["Le"].any() else "b0_miss_black"] += 1
            else:
                c["b1_miss_env"] += int(b["Le"].any())
    at_max = e["depth"] == PHANTOM_CAM_DEPTH
    assert (c["b0_miss_env"] == 0) == at_max and (c["b0_miss_black"] == 0) != at_max, c
    return _need(case, variant, c, "b1_miss_env")


def _check_env_is_area(case, variant, e):
    c = {}
    for pa, k, b in _bounces(e):
        if b["nee"] and k == 0:
            a, h = b["nee"]["area"], b["nee"]["hdri"]
            if a["wanted"] and h["wanted"]:
                key = f"area_{'vis' if a['visible'] else 'occ'}_hdri_{'vis' if h['visible'] else 'occ'}"
                c[key] = c.get(key, 0) + 1
    return _need(case, variant, c, "area_vis_hdri_vis", "area_vis_hdri_occ", "area_occ_hdri_vis")


def _check_depth_cut(case, variant, e):
    c = dict(cut_alive=0, ended_by_miss=0)
    for paths in e["paths"]:
        for pa in paths:
            last = pa.bounces[-1]
            c["cut_alive" if (len(pa.bounces) == e["depth"] and last["att"] is not None) else "ended_by_miss"] += 1
    return _need(case, variant, c, "cut_alive", "ended_by_miss")


def _check_edge_on(case, variant, e):
    c = dict(cut=0, cut_mid_columns=0, lit_mid_columns=0, lit_beside=0, dark_beside=0)
    for s, paths in enumerate(e["paths"]):
        for p, pa in enumerate(paths):
            a = pa.bounces[0]["nee"]["area"]
            if pa.margin < 1 or not a["wanted"]:
                continue
            col = p % GW
            assert a["visible"]                      # nothing stands between the wall and the lamp
            if a["cut"]:
                c["cut"] += 1
                c["cut_mid_columns"] += col in (11, 12)
                assert not a["con"].any()
            elif col in (11, 12):
                c["lit_mid_columns"] += 1
            elif col in (10, 13):
                c["lit_beside" if a["con"].min() > 0.05 else "dark_beside"] += 1
    assert c["cut"] == c["cut_mid_columns"] and c["dark_beside"] == 0, c
    return _need(case, variant, c, "cut", "lit_mid_columns", "lit_beside")


def _check_fog(case, variant, e):
    c = _nee_counts(e)
    sc = e["scene"]
    c["iso_then_light"] = 0
    for pa, k, b in _bounces(e):
        if b.get("light_hit") and k >= 2 and b["allow"] and sc.objects[pa.bounces[k - 1]["obj"]]["kind"] == "volume" \
                and sc.objects[pa.bounces[k - 2]["obj"]]["kind"] == "quad":
            c["iso_then_light"] += 1
    # shadow rays the fog alone stops: no quad stands between the wall and the lamp
    return _need(case, variant, c, "b0_occ", "b0_vis", "iso_then_light")


ENV_GATE = {v: (2, 1) for v in ("env", "sky", "bg", "env+light", "sky+light", "bg+light")}

CASES = {c.name: c for c in [
    Case("room", _room, {"d1": (1, 1), "d2": (2, 1), "d3": (3, 1), "d6": (6, 1)}, _check_room, quant8=True, group="room"),
    Case("lights3", _lights3, {"": (2, 1)}, _check_lights3, quant8=True),
    Case("clamp_b1", _clamp_b1, {"": (2, 4)}, _check_clamp),
    Case("sphere_in_list", _sphere_in_list, {"": (2, 2)}, _check_sphere_in_list),
    Case("mirror_chain", _chain, {"mirror": (3, 4)}, _check_chain),
    Case("glass_chain", _chain, {"glass": (4, 4)}, _check_chain),
    Case("checker_light", _checker_light, {"": (2, 1)}, _check_checker),
    Case("env_gate", _env_gate, ENV_GATE, _check_env_gate, group="env", tail=True),
    Case("phantom", _phantom, {"at_max": (PHANTOM_CAM_DEPTH, 1), "below": (PHANTOM_CAM_DEPTH - 1, 1)}, _check_phantom,
         group="env", tail=True),
    Case("env_is_area", _env_is_area, {"": (2, 1)}, _check_env_is_area, quant8=True, group="env"),
    Case("edge_on", _edge_on, {"": (1, 4)}, _check_edge_on),
    Case("depth_cut", _depth_cut, {"d2": (2, 1), "d3": (3, 1)}, _check_depth_cut, group="env", tail=True),
    Case("fog_shadow", _fog_shadow, {"": (3, 4)}, _check_fog, group="fog"),
]}

ROWS = [(n, v) for n, c in CASES.items() for v in c.variants]
TAIL_ROWS = [(n, v) for n, v in ROWS if CASES[n].tail and not CASES[n].scene(v).lights and CASES[n].variants[v][0] > 1]


# ---------------------------------------------------------------------------
# the comparisons, shared by the consumers
# ---------------------------------------------------------------------------
def record_errors(e, ids, s, b, top, t, ray, nee, name, bits="nee"):
    """Bounce b of sample s against the reference: ids, ended paths and the
    NEE bits exact (asserted here); returns the worst errors (ray: absolute,
    over the six coordinates; t: relative) over the compared paths.  bits:
    which expectation the NEE bits are held to: "nee" (the reference's own
    order), "nee_dev" (the oracle's recorder and the device, which cut by
    cosLight before the shadow test) or "nee_lifted" (the device with a
    lifted volume)."""
    ok = e["hit_ok"][s][b]
    want = e["obj"][s][b]
    lut = np.array(list(ids) + [-2, -1], np.int32)          # world index -> hittable id; -1 a miss, -2 ended
    want_top = lut[want]
    top = np.asarray(top)
    bad = np.flatnonzero((top != want_top) & ok)
    assert len(bad) == 0, f"{name} s{s} b{b}: ids differ at pixels {bad[:8]}: {top[bad[:8]]} want {want_top[bad[:8]]}"
    live = ok & (want != -2)
    hit = live & (want >= 0)
    ray_err = float(np.abs(np.asarray(ray, np.float64)[live] - e["ray"][s][b][live]).max()) if live.any() else 0.0
    t_err = float((np.abs(np.asarray(t, np.float64)[hit] - e["t"][s][b][hit]) / e["t"][s][b][hit]).max()) if hit.any() else 0.0
    if nee is not None:
        okn = e["nee_ok"][s][b]
        nee, want_nee = np.asarray(nee), e[bits][s][b]
        bad = np.flatnonzero((nee != want_nee) & okn)
        assert len(bad) == 0, (f"{name} s{s} b{b}: NEE bits ({bits}) differ at pixels {bad[:8]}: {nee[bad[:8]]} "
                               f"want {want_nee[bad[:8]]}")
    return ray_err, t_err


def radiance_error(e, L, rtol=0.0):
    """Worst |error| of the summed radiance over the decided pixels, less rtol times the expected value."""
    ok = e["L_ok"]
    want = e["L"][ok]
    return float((np.abs(np.asarray(L, np.float64).reshape(-1, 3)[ok] - want) - rtol * np.abs(want)).max())
