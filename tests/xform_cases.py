"""The scenes that hold transform.go's five wrappers (Translate, RotateX,
RotateY, RotateZ, Scale) and their chains to tests/path_ref.py: every kind
alone, every ordered pair, chains of one to six with every kind at the
positions the device reads through its second load, inner lists, leaf nodes
and a mesh, a mirror and a glass ball that show the mapped normal, a moving
sphere, a wrapped light, and RotateX / RotateZ siblings under a world tree.
One 24 x 16 frame per row from the grid camera at the origin, seed 3, at most
2 samples, depth at most 3, coordinates within +-4 (the object space of
`scale_1000` reaches 32: path_ref's margins grow with it).  Every row has an
unwrapped back wall and one unwrapped quad light behind the camera, so NEE
runs at every bounce, and is a flat RT_LIST except `rot_bvh`.

Every row asserts on path_ref alone (`expected`) that at most LEFT_OUT_CAP of
its pixel-samples are left out and, for each wrapped object, that it is the
closest hit of at least 12 pixels at bounce 0 and of some ray at bounce 1,
the occluder of a wanted shadow ray, and missed by a shadow ray that passes
through its world bounding box (the box the scene description carries).

Placement.  Except in `wrap_pairs`, an object is written down where it is to
be seen and taken into object space through its chain's own ray maps
(`into_object`), so the frame looks alike whatever the parameters and the
parameters show in the object-space data the device is handed and in the
hit point and normal RotateX / RotateZ report.  `wrap_pairs` keeps one
object-space geometry and one parameter set per kind, so the two orders of a
pair are the same two maps commuted and must differ somewhere.

Two consumers: tests/test_xform_kat.py (path_ref alone, the oracle in both
modes, the production kernels on the host) and tests/test_gpu_xform_kat.py."""
import math

import numpy as np

from tests import path_cases as PC
from tests import path_ref as P
from tests.scene_builder import Builder
from tests.shade_cases import GW

N = PC.N
KINDS = ("translate", "rot_x", "rot_y", "rot_z", "scale")
QUIRK_KINDS = ("rot_x", "rot_z")

A_WALL, A_QUAD, A_BALL, A_TRI, A_DISC = (0.5, 0.25, 0.125), (0.75, 0.75, 0.25), (0.25, 0.5, 0.75), (0.75, 0.125, 0.125), \
    (0.125, 0.75, 0.125)
WALL = ((-4, -4, -3.5), (8, 0, 0), (0, 8, 0))               # faces +z, towards the camera
LAMP = ((-0.75, 1.0, 0.5), (1.5, 0, 0), (0, 1.0, 0))        # behind the camera, no camera ray sees it


def rot(kind, degrees):
    r = math.radians(degrees)
    return (kind, math.sin(r), math.cos(r))


def norm_chain(chain):
    return P.wrapped(chain, [])["chain"]


def point_in(chain, p):
    p, z = P._v(p), np.zeros(3)
    for w in chain:
        p, _ = P.wrap_ray(w, p, z)
    return p


def vector_in(chain, v):
    v, z = P._v(v), np.zeros(3)
    for w in chain:
        _, v = P.wrap_ray(w, z, v)
    return v


def into_object(chain, prim):
    """The primitive `prim`, written down where it is to be seen, in the
    object space of `chain`: points through the chain's map of a ray's origin,
    vectors through its map of a direction.  A sphere's or circle's radius is
    kept: under a Scale it is seen as an ellipsoid or ellipse."""
    ch = norm_chain(chain)
    k = prim["kind"]
    if k == "quad":
        return P.quad(point_in(ch, prim["Q"]), vector_in(ch, prim["u"]), vector_in(ch, prim["v"]), prim["mat"], prim["name"])
    if k == "tri":
        return P.tri(point_in(ch, prim["a"]), point_in(ch, prim["b"]), point_in(ch, prim["c"]), prim["mat"], prim["name"])
    if k == "circle":
        return P.circle(point_in(ch, prim["c"]), vector_in(ch, prim["n"]), prim["r"], prim["mat"], prim["name"])
    return P.sphere(point_in(ch, prim["c"]), prim["r"], prim["mat"], prim["name"], vel=vector_in(ch, prim["vel"]))


def seen(chain, prim, name=None, inner_kind="prim"):
    ob = P.wrapped(chain, into_object(chain, prim), name or prim["name"])
    ob["inner_kind"] = inner_kind
    return ob


def base(objects, extra_lights=()):
    """wall, lamp, then the row's objects; the lights are the lamp and `extra_lights`."""
    obs = [P.quad(*WALL, P.lambertian(A_WALL), "wall"), P.quad(*LAMP, P.light((8, 7, 6)), "lamp")] + list(objects)
    return P.Scene(obs, lights=[1] + [2 + k for k in extra_lights])


# ---------------------------------------------------------------------------
# wrap_each
# ---------------------------------------------------------------------------
EACH = {
    "translate": [("translate", o) for o in ((0.5, -0.25, 0.75), (-1.25, 0.5, -0.5), (0.3, 0.7, 1.1), (-0.6, -0.9, 0.4))],
    "rot_x": [rot("rot_x", a) for a in (20, -35, 50, 110)],
    "rot_y": [rot("rot_y", a) for a in (25, -40, 65, -115)],
    "rot_z": [rot("rot_z", a) for a in (30, -20, 75, 160)],
    "scale": [("scale", f) for f in ((1.3, 0.8, 1.1), (0.7, 1.4, 0.9), (2.0, 0.5, 1.5), (0.6, 0.6, 2.5))],
    "scale_mirror": [("scale", f) for f in ((-1.3, 0.8, 1.1), (0.7, -1.4, 0.9), (2.0, 0.5, -1.5), (-0.6, 0.6, 2.5))],
    # Ry(90), Ry(-90): sin = +-1, cos = math.cos(math.pi / 2) = 6.1e-17, as Ry computes it
    "rot_y_90": [("rot_y", math.sin(s * math.pi / 2), math.cos(s * math.pi / 2)) for s in (1, -1, 1, -1)],
    "rot_x_180": [("rot_x", math.sin(math.pi), math.cos(math.pi))] * 4,
    "scale_1000": [("scale", (8.0, 1.0, 0.125))] * 4,
}
# RotateX / RotateZ by 180 degrees turn P and N by 360 in all: no quirk to show
NO_QUIRK = {("wrap_each", "rot_x_180")}


def four(chains, stacked=False):
    """A quad, a sphere, a triangle and a circle side by side at z = -2.2 (or,
    stacked, one above the other at z = -1.8, each about 1.8 wide), Lambertian, each under its own chain."""
    L = P.lambertian
    out = []
    for k, ch in enumerate(chains):
        if stacked:
            x, y, z, w, h = 0.0, (-0.95, -0.32, 0.32, 0.95)[k], -1.8, 0.9, 0.22
        else:
            x, y, z, w, h = (-1.8, -0.6, 0.6, 1.8)[k], 0.0, -2.2, 0.5, 0.5
        sc = [wr[1] for wr in ch if wr[0] == "scale"]
        f = np.abs(np.prod(np.array(sc, float), axis=0)) if sc else np.ones(3)
        r = 0.22 if stacked else 0.5 / math.sqrt(f[0] * f[1])
        if k == 0:
            pr = P.quad((x - w, y - h, z - 0.1), (2 * w, 0, 0.25), (0, 2 * h, 0.15), L(A_QUAD), "quad")
        elif k == 1:
            pr = P.sphere((x, y, z), r, L(A_BALL), "ball")
        elif k == 2:
            pr = P.tri((x - w, y - h, z - 0.1), (x + w, y - h, z + 0.2), (x, y + h, z), L(A_TRI), "tri")
        else:
            pr = P.circle((x, y, z), (0.2, 0.1, 1.0), r, L(A_DISC), "disc")
        out.append(seen(ch, pr))
    return out


def _wrap_each(variant):
    return base(four([[w] for w in EACH[variant]], stacked=variant == "scale_1000"))


# ---------------------------------------------------------------------------
# wrap_pairs
# ---------------------------------------------------------------------------
PAIR = {"translate": ("translate", (0.3, -0.2, 0.25)), "rot_x": rot("rot_x", 15), "rot_y": rot("rot_y", -18),
        "rot_z": rot("rot_z", 20), "scale": ("scale", (1.25, 0.8, 1.1))}
PAIRS = [f"{a}+{b}" for a in KINDS for b in KINDS]


def _wrap_pairs(variant):
    a, b = variant.split("+")
    ch = [PAIR[a], PAIR[b]]
    q = P.quad((-1.7, -0.6, -2.3), (1.2, 0, 0.25), (0, 1.2, 0.15), P.lambertian(A_QUAD), "quad")
    s = P.sphere((0.8, 0.0, -2.2), 0.6, P.lambertian(A_BALL), "ball")
    obs = []
    for pr in (q, s):
        ob = P.wrapped(ch, pr, pr["name"])
        ob["inner_kind"] = "prim"
        obs.append(ob)
    return base(obs)


# ---------------------------------------------------------------------------
# wrap_long
# ---------------------------------------------------------------------------
LONG = [("translate", (0.4, -0.3, 0.5)), rot("rot_z", 25), rot("rot_y", -30), rot("rot_x", 40), ("scale", (1.25, 0.8, 1.1)),
        ("translate", (-0.35, 0.2, 0.15))]
ALT = {"translate": ("translate", (0.2, 0.45, -0.3)), "rot_x": rot("rot_x", 35), "rot_y": rot("rot_y", 55),
       "rot_z": rot("rot_z", -45), "scale": ("scale", (0.8, 1.3, -1.2))}
LONG_VARIANTS = [f"len{n}" for n in range(1, 7)] + [f"p{p}_{k}" for p in (3, 4, 5) for k in KINDS]


def long_chain(variant):
    if variant.startswith("len"):
        return LONG[:int(variant[3:])]
    p, kind = int(variant[1]), variant[3:]
    return LONG[:p] + [ALT[kind]] + LONG[p + 1:]


def two(ch, inner_kind="prim"):
    q = P.quad((-1.6, -0.6, -2.3), (1.2, 0, 0.25), (0, 1.2, 0.15), P.lambertian(A_QUAD), "quad")
    s = P.sphere((0.9, 0.0, -2.2), 0.55, P.lambertian(A_BALL), "ball")
    return [seen(ch, q), seen(ch, s)]


def _wrap_long(variant):
    return base(two(long_chain(variant)))


# ---------------------------------------------------------------------------
# wrap_inner
# ---------------------------------------------------------------------------
INNER_CHAIN = [("translate", (0.2, -0.1, -2.3)), rot("rot_y", 35), ("scale", (1.2, 0.9, 0.8))]


def box_faces(lo, hi, mat):
    """Builder.box_quads' six faces as path_ref quads, in its order."""
    lo, hi = np.array(lo, float), np.array(hi, float)
    out = []
    for k in range(3):
        for side in (lo, hi):
            Q = lo.copy()
            Q[k] = side[k]
            u, v = np.zeros(3), np.zeros(3)
            u[(k + 1) % 3] = (hi - lo)[(k + 1) % 3]
            v[(k + 2) % 3] = (hi - lo)[(k + 2) % 3]
            out.append(P.quad(Q, u, v, mat, f"face{len(out)}"))
    return out


def octa_mesh(mat):
    """A closed mesh of 32 triangles: an octahedron's faces split in four, the
    new vertices pushed out to the unit sphere, times 0.6."""
    ax = [np.array(v, float) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    faces = [(ax[i], ax[j], ax[k]) for i in (0, 1) for j in (2, 3) for k in (4, 5)]
    tris = []
    for a, b, c in faces:
        ab, bc, ca = ((a + b) / np.linalg.norm(a + b), (b + c) / np.linalg.norm(b + c), (c + a) / np.linalg.norm(c + a))
        tris += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return [P.tri(0.6 * a, 0.6 * b, 0.6 * c, mat, f"t{k}") for k, (a, b, c) in enumerate(tris)]


def _wrap_inner(variant):
    if variant == "mesh":
        ob = P.wrapped(INNER_CHAIN, octa_mesh(P.lambertian(A_TRI)), "mesh")
    else:
        ob = P.wrapped(INNER_CHAIN, box_faces((-0.6, -0.5, -0.4), (0.5, 0.6, 0.5), P.lambertian(A_QUAD)), "box")
    ob["inner_kind"] = variant
    return base([ob])


# ---------------------------------------------------------------------------
# wrap_mats, wrap_moving, wrap_light
# ---------------------------------------------------------------------------
def _wrap_mats(variant):
    mirror = P.quad((-2.0, -0.7, -2.6), (1.5, 0, 0.5), (0, 1.4, 0.3), P.metal((0.75, 0.5, 0.25), 0.0), "mirror")
    glass = P.sphere((1.0, 0.0, -2.2), 0.6, P.dielectric(1.5), "glass")
    return base([seen([rot("rot_x", 12)], mirror), seen([("scale", (1.2, -0.9, 1.1))], glass)])


def _wrap_moving(variant):
    ball = P.sphere((-0.3, 0.0, -2.2), 0.6, P.lambertian(A_BALL), "ball", vel=(0.9, 0.3, 0.0))
    return base([seen([("translate", (0.5, 0.25, -1.0)), rot("rot_y", 40)], ball)])


def _wrap_light(variant):
    panel = P.quad((-1.5, -0.5, -2.4), (1.0, 0, 0.2), (0, 1.0, 0.1), P.light((3, 2, 1)), "panel")
    block = P.quad((0.5, -0.6, -2.3), (1.2, 0, 0.25), (0, 1.2, 0.15), P.lambertian(A_QUAD), "block")
    return base([seen([("translate", (0.4, 0.3, -1.2))], panel), seen([("translate", (-0.3, 0.2, 0.6))], block)], extra_lights=[0])


# ---------------------------------------------------------------------------
# rot_bvh
# ---------------------------------------------------------------------------
def _rot_bvh(variant):
    """Two sibling quads under Translate(RotateX | RotateZ by 30 degrees) below
    one node, the back wall (and the lamp) below the root: node(node(left,
    right), node(wall, lamp)), as tests/test_gpu_rotations.py lays its own out.  A rotated
    quad is seen turned by -30 degrees and boxed turned by +30, so the pair's
    box holds only a part of what Hit sees."""
    w = rot(variant, 30)
    if variant == "rot_x":        # the object 0.6 before the wrapper's origin: seen 0.3 above it, boxed 0.3 below
        tl, tr = (0.0, -0.3, -2.92), (0.4, -0.3, -2.52)
        left = P.quad((-1.6, -0.7, -2.45), (2.0, 0, 0), (0, 1.4, 0.1), P.lambertian(A_QUAD), "left")
        right = P.quad((-0.2, -0.6, -2.02), (1.5, 0, 0), (0, 1.2, 0.05), P.lambertian(A_BALL), "right")
    else:                         # the object 0.9 beside the wrapper's origin: seen 0.45 below it, boxed 0.45 above
        tl, tr = (-0.78, 0.3, -2.4), (-0.38, 0.3, -2.0)
        left = P.quad((-0.8, -0.85, -2.45), (1.6, 0, 0.1), (0, 1.4, 0.1), P.lambertian(A_QUAD), "left")
        right = P.quad((-0.2, -0.75, -2.02), (1.4, 0, 0.05), (0, 1.2, 0.05), P.lambertian(A_BALL), "right")
    sc = base([seen([("translate", tl), w], left), seen([("translate", tr), w], right)])
    sc.tree = P.node(P.node(2, 3), P.node(0, 1))
    return sc


# ---------------------------------------------------------------------------
# a row
# ---------------------------------------------------------------------------
class XCase(PC.Case):
    """path_cases.Case over scenes with wrapped objects, the two more
    primitives and a world tree.  build returns ids (the outermost hittable of
    world object k) and leaves prim_ids[k] (the hittable ids of object k's
    inner primitives, in order) on the case."""

    def __init__(self, name, make, variants, check, group, modes=False, prim=False):
        super().__init__(name, self._scene, variants, check, group=group)
        self.make, self.modes, self.prim = make, modes, prim
        self._g, self._scenes = None, {}

    def _scene(self, variant):
        """The row's scene, once: with boxes[k], the world box of object k, and
        the tree's boxes, all read from the Builder's records."""
        if variant not in self._scenes:
            sc = self.make(variant)
            b, ids, _, nodes = self._hittables(self._g, sc)
            sc.boxes = [list(b.h[i].bbox) for i in ids]
            for nd, hid in nodes:
                nd["box"] = list(b.h[hid].bbox)
            self._scenes[variant] = sc
        return self._scenes[variant]

    def camera(self, g, variant):
        self._g = g
        return super().camera(g, variant)

    def expected(self, g, variant):
        self._g = g
        return super().expected(g, variant)

    @staticmethod
    def _material(g, b, m):
        if m["kind"] in ("lambertian", "light"):
            return b.mat(g.RT_LAMBERTIAN if m["kind"] == "lambertian" else g.RT_DIFFUSE_LIGHT, b.solid(m["tex"][1]))
        if m["kind"] == "metal":
            return b.metal(m["albedo"], m["fuzz"])
        return b.dielectric(m["ior"])

    @classmethod
    def _prim(cls, g, b, pr):
        mat = cls._material(g, b, pr["mat"])
        if pr["kind"] == "quad":
            return b.quad(pr["Q"], pr["u"], pr["v"], mat)
        if pr["kind"] == "tri":
            return b.triangle(pr["a"], pr["b"], pr["c"], mat)
        if pr["kind"] == "circle":
            return b.circle(pr["c"], pr["n"], pr["r"], mat)
        return b.sphere(pr["c"], pr["r"], mat, vel=tuple(pr["vel"]))

    @staticmethod
    def _mesh_tree(b, prims, kids):
        """A binary BVHNode tree over the triangles: halves by the centroid on
        the widest axis (bvh.go:144-159), leaves of at most four as BVHNode{leaf, leaf}."""
        def rec(sel):
            if len(sel) <= 4:
                return b.leaf_node([kids[i] for i in sel])
            cen = np.array([(prims[i]["a"] + prims[i]["b"] + prims[i]["c"]) / 3.0 for i in sel])
            ax = int(np.argmax(cen.max(0) - cen.min(0)))
            order = [sel[i] for i in np.argsort(cen[:, ax], kind="stable")]
            return b.bvh_node(rec(order[:len(order) // 2]), rec(order[len(order) // 2:]))
        return rec(list(range(len(kids))))

    @classmethod
    def _hittables(cls, g, sc):
        b = Builder(g)
        ids, prim_ids = [], []
        for ob in sc.objects:
            if ob["kind"] != "wrapped":
                ids.append(cls._prim(g, b, ob))
                prim_ids.append([ids[-1]])
                continue
            kids = [cls._prim(g, b, pr) for pr in ob["inner"]]
            kind = ob.get("inner_kind", "prim")
            if kind == "prim":
                assert len(kids) == 1
                h = kids[0]
            elif kind == "list":
                h = b.listing(kids)
            elif kind == "leaf":
                h = b.leaf_node(kids)
            else:
                h = cls._mesh_tree(b, ob["inner"], kids)
            for w in reversed(ob["chain"]):
                if w[0] == "translate":
                    h = b.translate(h, tuple(w[1]))
                elif w[0] == "scale":
                    h = b.scale(h, tuple(w[1]))
                else:
                    h = getattr(b, {"rot_x": "rotate_x", "rot_y": "rotate_y", "rot_z": "rotate_z"}[w[0]])(h, w[1], w[2])
            ids.append(h)
            prim_ids.append(kids)
        nodes = []

        def tree(nd):
            if not isinstance(nd, dict):
                return ids[nd]
            hid = b.bvh_node(tree(nd["left"]), tree(nd["right"]))
            nodes.append((nd, hid))
            return hid
        root = tree(sc.tree) if sc.tree is not None else None
        b.lights = [ids[k] for k in sc.lights]
        return b, ids, prim_ids, (nodes if root is not None else [])

    def build(self, g, variant):
        self._g = g
        sc = self._scene(variant)
        b, ids, self.prim_ids, nodes = self._hittables(g, sc)
        root = nodes[-1][1] if nodes else b.listing(ids)
        return b, b.desc(root), self.camera(g, variant), ids

    def group_of(self, variant):
        """The group of rows whose measured fp32 figures hold the variant:
        `stretch` is scale_1000, whose object space reaches 32."""
        return "stretch" if (self.name, variant) == ("wrap_each", "scale_1000") else self.group

    def chains(self, variant):
        return [ob["chain"] for ob in self._scene(variant).objects if ob["kind"] == "wrapped"]

    def quirk(self, variant):
        """Whether the row's chains hold a RotateX / RotateZ that shows: the
        reported hit point is then off the incoming ray."""
        has = any(w[0] in QUIRK_KINDS for ch in self.chains(variant) for w in ch)
        return has and (self.name, variant) not in NO_QUIRK

    def as_written(self, variant):
        """Whether flatten.cpp's RotateX / RotateZ mode holds: fp32 nodes whatever was asked for."""
        return any(w[0] in QUIRK_KINDS for ch in self.chains(variant) for w in ch)

    def has_circle(self, variant):
        return any(pr["kind"] == "circle" for ob in self._scene(variant).objects if ob["kind"] == "wrapped"
                   for pr in ob["inner"])


def shadow_rays(e):
    """(path, bounce, record, origin) of every wanted area shadow ray of the decided paths."""
    for pa, k, b in PC._bounces(e):
        if b["nee"] and b["nee"]["area"]["wanted"]:
            yield pa, k, b["nee"]["area"], b["scatter"][0]


def wrapped_counts(case, variant, e):
    """The four counts every row asserts of each wrapped object."""
    sc = e["scene"]
    c = {}
    rays = list(shadow_rays(e))
    for k, ob in enumerate(sc.objects):
        if ob["kind"] != "wrapped":
            continue
        nm = ob["name"]
        c[f"{nm}_b0"] = sum(1 for pa, kb, b in PC._bounces(e) if kb == 0 and b["obj"] == k)
        c[f"{nm}_b1"] = sum(1 for pa, kb, b in PC._bounces(e) if kb == 1 and b["obj"] == k)
        c[f"{nm}_occludes"] = sum(1 for _, _, a, _ in rays if a["occluder"] == k)
        miss = 0
        for _, _, a, o in rays:
            if a["occluder"] == k:
                continue
            inbox, rb = P.aabb_test(sc.boxes[k], o, a["dir"], 0.001, a["end"])
            if inbox and rb >= 1:
                h, rt, _, _ = P.wrapped_test(o, a["dir"], 0.0, ob, 0.001, a["end"])
                miss += h is None and rt >= 1
        c[f"{nm}_missed_in_box"] = miss
        assert c[f"{nm}_b0"] >= 12, f"{case.name}[{variant}]: {c}"
        assert c[f"{nm}_b1"] >= 1 and c[f"{nm}_occludes"] >= 1 and miss >= 1, f"{case.name}[{variant}]: {c}"
    return c


def _check_plain(case, variant, e):
    return wrapped_counts(case, variant, e)


def _check_inner(case, variant, e):
    c = wrapped_counts(case, variant, e)
    subs = {b["sub"] for pa, k, b in PC._bounces(e) if b["obj"] == 2}
    c["inner_hit"] = len(subs)
    assert len(subs) >= 3, f"{case.name}[{variant}]: inner primitives hit {subs}"
    return c


def _check_mats(case, variant, e):
    c = wrapped_counts(case, variant, e)
    sc = e["scene"]
    c.update(reflected_to_wall=0, refracted_to_wall=0, glass_back_face=0)
    for pa in (pa for paths in e["paths"] for pa in paths if pa.margin >= 1):
        bs = pa.bounces
        for k in range(len(bs) - 1):
            if bs[k]["obj"] < 0:
                break
            nm = sc.objects[bs[k]["obj"]]["name"]
            if nm == "mirror" and bs[k + 1]["obj"] == 0:
                c["reflected_to_wall"] += 1
            if nm == "glass" and bs[k].get("branch") == "refract":
                c["glass_back_face"] += not bs[k]["hit"][2]
                if k + 2 < len(bs) and bs[k + 1]["obj"] == bs[k]["obj"] and bs[k + 1].get("branch") == "refract" \
                        and bs[k + 2]["obj"] == 0:
                    c["refracted_to_wall"] += 1
    return PC._need(case, variant, c, "reflected_to_wall", "refracted_to_wall", "glass_back_face")


def _check_moving(case, variant, e):
    c = wrapped_counts(case, variant, e)
    # the time shows: the ball's hit differs from the one at time 0 somewhere
    sc, moved = e["scene"], 0
    for pa, k, b in PC._bounces(e):
        if k == 0 and b["obj"] == 2:
            h0, _, _, _ = P.wrapped_test(b["o"], b["d"], 0.0, sc.objects[2], 0.001, P.INF)
            moved += h0 is None or abs(h0[0] - b["t"]) > 1e-3 * b["t"]
    c["moved_by_time"] = moved
    return PC._need(case, variant, c, "moved_by_time")


def _check_light(case, variant, e):
    c = PC._nee_counts(e)
    c.update({k: v for k, v in wrapped_counts(case, variant, e).items() if k.startswith("block")})
    for pa, k, b in PC._bounces(e):
        if b["nee"]:
            a = b["nee"]["area"]
            if a["light"] == 1:                               # the wrapped panel: sampleAreaLight takes only *Quad (camera.go:616)
                assert not a["wanted"] and not a["con"].any()
                c["wrapped_chosen"] = c.get("wrapped_chosen", 0) + 1
            elif a["con"].any():
                c["quad_lit"] = c.get("quad_lit", 0) + 1
        if b.get("light_hit"):
            nm = e["scene"].objects[b["obj"]]["name"]
            c[f"b{k}_{nm}"] = c.get(f"b{k}_{nm}", 0) + 1
    assert "b1_light_counted" not in c
    return PC._need(case, variant, c, "wrapped_chosen", "quad_lit", "b0_panel", "b1_panel", "b1_light_dropped")


def _check_bvh(case, variant, e):
    """Camera rays: a brute-force hit of a rotated quad that the tree walk
    never reaches (the pair's box clips it), one it reaches, and the right
    sibling winning over a hit of the left."""
    sc = e["scene"]
    c = dict(clipped=0, reached=0, right_over_left=0)
    for pa, k, b in PC._bounces(e):
        if k != 0:
            continue
        hl, rl, _, _ = P.wrapped_test(b["o"], b["d"], 0.0, sc.objects[2], 0.001, P.INF)
        hr, rr, _, _ = P.wrapped_test(b["o"], b["d"], 0.0, sc.objects[3], 0.001, P.INF)
        if min(rl, rr) < 1 or not (hl or hr):
            continue
        if b["obj"] in (2, 3):
            c["reached"] += 1
            c["right_over_left"] += b["obj"] == 3 and hl is not None
        else:
            c["clipped"] += 1
    for key in c:
        assert c[key] >= 5, f"{case.name}[{variant}]: {c}"
    c.update({k_: v for k_, v in wrapped_counts(case, variant, e).items()})
    return c


CASES = {c.name: c for c in [
    XCase("wrap_each", _wrap_each, {v: (3, 2) for v in EACH}, _check_plain, "chain"),
    XCase("wrap_pairs", _wrap_pairs, {v: (2, 1) for v in PAIRS}, _check_plain, "chain"),
    XCase("wrap_long", _wrap_long, {v: (2, 1) for v in LONG_VARIANTS}, _check_plain, "chain", modes=True),
    XCase("wrap_inner", _wrap_inner, {v: (2, 1) for v in ("list", "leaf", "mesh")}, _check_inner, "tree", modes=True, prim=True),
    XCase("wrap_mats", _wrap_mats, {"": (3, 2)}, _check_mats, "chain"),
    XCase("wrap_moving", _wrap_moving, {"": (2, 2)}, _check_moving, "chain"),
    XCase("wrap_light", _wrap_light, {"": (2, 2)}, _check_light, "chain"),
    XCase("rot_bvh", _rot_bvh, {v: (2, 1) for v in QUIRK_KINDS}, _check_bvh, "tree"),
]}

ROWS = [(n, v) for n, c in CASES.items() for v in c.variants]
MODES = ("quant8", "wide8", "tlas_reference")
MODE_ROWS = [(n, v, m) for n, v in ROWS if CASES[n].modes for m in MODES]


def pair_orders_differ(g):
    """For every unequal pair of kinds, the two orders give a different
    bounce-0 id, t or P somewhere: otherwise the pair pins no order."""
    c = CASES["wrap_pairs"]
    out = {}
    for i, a in enumerate(KINDS):
        for b in KINDS[i + 1:]:
            ea, eb = c.expected(g, f"{a}+{b}"), c.expected(g, f"{b}+{a}")
            worst = 0.0
            for pa, pb in zip(ea["paths"][0], eb["paths"][0]):
                ha, hb = pa.bounces[0], pb.bounces[0]
                if ha["obj"] != hb["obj"]:
                    worst = max(worst, 1.0)
                elif ha["obj"] >= 2:
                    worst = max(worst, abs(ha["t"] - hb["t"]), float(np.abs(ha["hit"][1] - hb["hit"][1]).max()))
            out[(a, b)] = worst
            assert worst > 1e-3, f"wrap_pairs: {a}+{b} and {b}+{a} agree to {worst}"
    return out


def chain_matrix(chain):
    """A: the product of the chain's ray maps of a direction, object <- world."""
    return np.array([vector_in(chain, e) for e in np.eye(3)]).T


def feature_normal(ob, o, d, time=0.0):
    """unit(A^T n_obj) for the ray's closest hit on the wrapped object, n_obj
    the primitive's normal faced against the object-space ray: the true
    normal of the seen surface (the inverse transpose of the object -> world
    map A^-1 is A^T).  None for a miss."""
    h, rt, sub, _ = P.wrapped_test(o, d, time, ob, 0.001, P.INF)
    if h is None:
        return None, rt, sub
    A = chain_matrix(ob["chain"])
    oo, dd = point_in(ob["chain"], o), vector_in(ob["chain"], d)
    hp, _ = P.prim_test(ob["inner"][sub], oo, dd, time, 0.001, P.INF, 1.0)
    n = hp[3]                                                # faced against the object-space ray by SetFaceNormal
    return P.R.unit(A.T @ n), rt, sub


FEATURE_ROWS = [(n, v) for n, v in ROWS if n in ("wrap_each", "wrap_long", "wrap_inner")]


def expected_normals(case, g, variant):
    """Sample 0's camera rays: (want (N, 3), flat, ball): unit(A^T n_obj) for
    the decided pixels whose closest hit is a wrapped object, `flat` those on
    a quad, triangle or circle, `ball` those on a sphere."""
    e = case.expected(g, variant)
    sc = e["scene"]
    want, flat, ball = np.zeros((N, 3)), np.zeros(N, bool), np.zeros(N, bool)
    for p, pa in enumerate(e["paths"][0]):
        b = pa.bounces[0]
        if not e["hit_ok"][0][0][p] or b["obj"] < 0 or sc.objects[b["obj"]]["kind"] != "wrapped":
            continue
        ob = sc.objects[b["obj"]]
        time = P.R.get_ray(case.camera(g, variant), p % GW, p // GW, PC.SEED, 0)[2]
        n, rt, sub = feature_normal(ob, b["o"], b["d"], time)
        assert n is not None and sub == b["sub"]
        want[p] = n
        (ball if ob["inner"][sub]["kind"] == "sphere" else flat)[p] = True
    return want, flat, ball


def ball_normals_f32(case, g, variant, t):
    """The same formula in float32 from a given fp32 t per pixel (the fp32
    oracle's): P = o + t d in object space, n = (P - c(time)) / r faced against
    the ray, unit(A^T n).  (N, 3); rows outside `ball` are 0."""
    F = np.float32
    e = case.expected(g, variant)
    sc = e["scene"]
    _, _, ball = expected_normals(case, g, variant)
    out = np.zeros((N, 3), F)
    for p in (int(x) for x in np.flatnonzero(ball)):
        b = e["paths"][0][p].bounces[0]
        ob = sc.objects[b["obj"]]
        pr = ob["inner"][b["sub"]]
        time = P.R.get_ray(case.camera(g, variant), p % GW, p // GW, PC.SEED, 0)[2]
        o, d = point_in(ob["chain"], b["o"]).astype(F), vector_in(ob["chain"], b["d"]).astype(F)
        c = (pr["c"] + pr["vel"] * time).astype(F)
        n = (o + F(t[p]) * d - c) / F(pr["r"])
        if np.dot(d, n) >= 0:
            n = -n
        w = chain_matrix(ob["chain"]).astype(F).T @ n
        out[p] = w / np.sqrt(np.dot(w, w))
    return out
