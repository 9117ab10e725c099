"""The scenes that hold the traversal stack bound (flatten.cpp stack_needed,
api.cpp device_builds, wave_layout.h spill_cap_for) to what a traversal really
holds: deep hand-built trees in every mode, expected values from
tests/path_ref.py's brute-force float64 closest hit and occlusion over all
primitives, with no tree.  One 24 x 16 frame per row from the grid camera at
the origin, seed 3, one sample, depth 2, at most about 130 primitives.

Construction.  tests/test_gpu_deep_stack.py's chain (a hand-built BVHNode
chain whose subtree is always the child that keeps its siblings pending) with
one change: the members are not quads in one window but concentric spheres,
each link's sphere enclosed by every sphere below it in the chain.

  * A member's box is then entered before its siblings' from either side, so
    the nearest-first traversal descends the whole chain with every sibling
    pending both for camera rays and for the shadow rays that come back from
    the wall (quads at distinct depths order one way only).
  * A sphere does not fill its box: a ray in the `corner band` (outside the
    largest sphere's silhouette, inside the smallest sphere's box) crosses
    every box of the chain and hits nothing.  Such camera rays reach the wall
    with the whole chain's siblings on the stack on the way, and the shadow
    rays from there to the small lamp at the camera's apex cross it again and
    pass; a flat quad fills its box, and no shadow ray could cross a chain of
    them and pass.
  * The radii are 0.636 + 0.010 k / (n - 1) about (0, 0, -1.9): the shells are
    8e-5 or more apart, far more than fp32 resolves, so the closest member is
    unambiguous in float64.  Closest of all is the largest sphere: the bottom
    link in the rows that traverse nearest-first, a link in mid-chain in
    `chain_dfs`, where the order is the reference's (left first).

Rows (variant: what it is there for; the bounds are derived in the rows'
comments below and measured figures are in DESIGN.md §5):

  chain_ref   n4 / n59 / n123: stack_needed 9 (just past the 8-entry ring), 64
              and 128, the largest accepted; n124 is refused (EDGES).  n8: the
              first chain a ray of which holds more than 8 entries (the bound
              has four entries of slack without instances).  p61 / p62: chains
              of pairs of shells, whose 8-wide bound is larger than the 4-wide
              one: 61 pairs take RT_NODES_WIDE8 (126), 62 (129) fall back to
              fp32 nodes.  n12dark: no light, depth 3, for the long-tail
              kernel.  One-word entries, fp32 / quant8 / wide8 nodes.
  chain_dfs   the same chain beside a RotateX sibling: reference order, two
              words per entry; the largest accepted depth (EDGES).
  inst_leaf   at the bottom of a world chain an RT_LIST leaf of five
              instances (Translate over a hand-built BVHNode chain of
              triangles kept by RT_BLAS_REFERENCE): world siblings, pending
              instances, the entry marker and the mesh's siblings at once.
  device_deep a mesh built on the device (RT_BLAS_DEVICE) at the bottom of a
              world chain of 111 shells: triangles whose centroids approach
              the origin in a geometric progression (a radix chain); the
              recomputed stack_needed is 118 + the device tree's need4 = 124.
              GPU only for traversal.
  balanced    64 quads under the SAH builder: must not leave the ring.

Every deep row asserts on path_ref alone that at least 12 camera rays and at
least 12 wanted shadow rays cross every member's box, that of those shadow
rays some are occluded by the deepest link and some pass, and (Case.expected)
that at most 2 % of the pixel-samples are left out."""
import math

import numpy as np

from tests import path_cases as PC
from tests import path_ref as P
from tests import xform_cases as XC
from tests.scene_builder import Builder

N = PC.N
CENTRE = (0.0, 0.0, -1.9)
R_MIN, R_MAX = 0.636, 0.646
A_WALL, A_SHELL, A_TRI, A_FLOOR = (0.5, 0.25, 0.125), (0.25, 0.5, 0.75), (0.75, 0.125, 0.125), (0.75, 0.75, 0.25)
WALL = ((-4, -4, -3.5), (8, 0, 0), (0, 8, 0))                  # faces +z, towards the camera
LAMP = ((-0.05, -0.05, 0.02), (0.1, 0, 0), (0, 0.1, 0))        # at the rays' apex, just behind the camera
LAMP_L = (900, 800, 700)
FLOOR = ((-4, -1.5, 0.5), (8, 0, 0), (0, 0, -4.5))              # seen in the bottom rows: its scattered rays reach the wall behind the shells

# the accepted / refused edges, pinned as exact depths (tests/test_stack_host.py test_edges)
EDGES = dict(chain_ref=dict(accepted=123, refused=124), chain_dfs=dict(accepted=59, refused=60), wide8=dict(taken=61, fallback=62))

K_INST, M_TRIS, W_INST = 5, 12, 20                             # inst_leaf: instances, triangles each, world spheres
S_MIN, S_MAX = 0.70, 0.80                                      # inst_leaf: the triangles' half extents
N_DEVICE, A_DEVICE, R_DEVICE = 19, 0.45, 2.9                    # device_deep: triangles, their half angle (as a slope), the farthest
W_DEVICE = 111                                                 # device_deep: world shells (stack_needed 118 + the device tree's need4)
OFF_DEVICE = (0.5, 0.25, 0.125)                                # exact in fp32
LAMP_DEVICE = ((-0.002, -0.002, 0.002), (0.004, 0, 0), (0, 0.004, 0))   # device_deep: shadow rays must converge as camera rays do


def radii(n, order, r_min=None):
    """The n shells' radii by chain position (0: the top link).  "nested": each
    encloses the one above it, the bottom link the largest.  "perm": a stride
    permutation of the same radii, the largest in mid-chain."""
    r_min = R_MIN if r_min is None else r_min
    r = [r_min + (R_MAX - r_min) * k / max(n - 1, 1) for k in range(n)]
    if order == "nested":
        return r
    s = next(s for s in range(7, 7 + n + 1) if math.gcd(s, n) == 1)
    return [r[(s * (i - n // 2) + n - 1) % n] for i in range(n)]


def shells(n, order, r_min=None):
    return [P.sphere(CENTRE, r, P.lambertian(A_SHELL), f"shell{i}") for i, r in enumerate(radii(n, order, r_min))]


def chain_tree(members, tail):
    """node(node(...node(members[-1], members[-2])..., members[0]) with the
    subtree on the left, then node(chain, tail): world indices."""
    cur = members[-1]
    for m in reversed(members[:-1]):
        cur = P.node(cur, m)
    return P.node(cur, tail)


def base(objects, lamp=True):
    obs = [P.quad(*WALL, P.lambertian(A_WALL), "wall"), P.quad(*FLOOR, P.lambertian(A_FLOOR), "floor")]
    if lamp:
        obs.append(P.quad(*LAMP, P.light(LAMP_L), "lamp"))
    return obs + list(objects), ([2] if lamp else [])


TAIL = P.node(0, P.node(1, 2))                                  # {wall, {floor, lamp}}: what hangs beside every chain


def _chain_ref(variant):
    """n shells, nested.  dark: without the lamp (the long-tail kernel takes
    paths only in scenes without a light)."""
    dark = variant.endswith("dark")
    pairs = variant[0] == "p"
    n = int(variant[1:-4] if dark else variant[1:]) * (2 if pairs else 1)
    obs, lights = base(shells(n, "nested"), lamp=not dark)
    first = len(obs) - n
    sc = P.Scene(obs, lights=lights, sky=dark)
    links = list(range(first, first + n))
    if pairs:                               # every link a node of two shells: the 8-wide collapse opens what the 4-wide keeps
        links = [P.node(links[2 * i], links[2 * i + 1]) for i in range(n // 2)]
    sc.world_tree = chain_tree(links, TAIL if not dark else P.node(0, 1))
    sc.members = list(range(first, first + n))
    sc.deepest = first + n - 1
    return sc


def _chain_dfs(variant):
    """n shells, the largest in mid-chain, beside a small quad under RotateX by
    180 degrees: turned by 360 in all, so its box holds what its Hit sees and
    the tree walk finds what brute force finds, while the scene still
    traverses in the reference's order."""
    n = int(variant[1:])
    tilt = XC.seen([XC.rot("rot_x", 180)], P.quad((1.9, -0.3, -2.0), (0.4, 0, 0), (0, 0.6, 0), P.lambertian(A_TRI), "tilted"))
    obs, lights = base(shells(n, "perm") + [tilt])
    first = len(obs) - n - 1
    sc = P.Scene(obs, lights=lights)
    cur = chain_tree(list(range(first, first + n)), first + n)
    sc.world_tree = P.node(cur, TAIL)
    sc.members = list(range(first, first + n))
    sc.deepest = first + int(np.argmax(radii(n, "perm")))
    return sc


def window(s, mat, name):
    """A triangle that spans the cube CENTRE +- s and fills little of it."""
    c = np.array(CENTRE)
    return P.tri(c + s * np.array((-1.0, -1.0, -1.0)), c + s * np.array((1.0, -1.0, 1.0)), c + s * np.array((-1.0, 1.0, 1.0)), mat, name)


def mesh_instances(k, m):
    """k Translate instances, each over its own chain of m nested triangles; the
    half extents interleave across the instances, so the instances' boxes nest
    as well."""
    out = []
    for j in range(k):
        off = (0.1 * (j + 1), -0.05 * (j + 1), 0.2 * (j + 1))
        ch = [("translate", off)]
        tris = [XC.into_object(ch, window(S_MIN + (S_MAX - S_MIN) * (i * k + j) / (k * m - 1), P.lambertian(A_TRI), f"t{j}_{i}"))
                for i in range(m)]
        ob = P.wrapped(ch, tris, f"mesh{j}")
        ob["inner_kind"] = "tri_chain"
        out.append(ob)
    return out


def _inst_leaf(variant):
    obs, lights = base(shells(W_INST, "nested") + mesh_instances(K_INST, M_TRIS))
    first = len(obs) - W_INST - K_INST
    sc = P.Scene(obs, lights=lights)
    leaf = tuple(range(first + W_INST, first + W_INST + K_INST))           # an RT_LIST of the instances
    sc.world_tree = chain_tree(list(range(first, first + W_INST)) + [leaf], TAIL)
    sc.members = list(range(first, first + W_INST + K_INST))
    sc.deepest = first + W_INST - 1
    return sc


def cone_mesh():
    """N_DEVICE triangles in planes z = -r, r = R_DEVICE 2^(-i / 3), each the
    lower left half of the square of half angle A_DEVICE about the axis: from
    the origin all subtend the same angles, and their centroids lie on one
    line towards the origin in a geometric progression, so successive Morton
    codes differ in ever lower bits and the radix tree is a chain."""
    a = A_DEVICE
    return [P.tri((-a * r, -a * r, -r), (a * r, -a * r, -r), (-a * r, a * r, -r), P.lambertian(A_TRI), f"d{i}")
            for i, r in enumerate(R_DEVICE * 2.0 ** (-k / 3.0) for k in range(N_DEVICE))]


def device_mesh_object_space():
    """(n, 3, 3): the triangles as the instance's mesh holds them."""
    ch = [("translate", OFF_DEVICE)]
    return np.array([[t["a"], t["b"], t["c"]] for t in (XC.into_object(ch, t) for t in cone_mesh())])


def _device_deep(variant):
    """w shells, nested, and at the chain's bottom one Translate instance of
    the cone mesh, whose box (the origin to beyond the shells, wider than
    they) encloses every shell's."""
    w = int(variant[1:])
    ch = [("translate", OFF_DEVICE)]
    ob = P.wrapped(ch, [XC.into_object(ch, t) for t in cone_mesh()], "cone")
    ob["inner_kind"] = "tri_chain"
    # (the shells 4.6e-5 apart: the ring of rays that graze some shell, left out, is narrower; the tiny lamp leaves out a few more)
    obs, lights = base(shells(w, "nested", 0.641) + [ob])
    obs[2] = P.quad(*LAMP_DEVICE, P.light(tuple(625.0 * x for x in LAMP_L)), "lamp")      # the same power from 1 / 625 of the area
    first = len(obs) - w - 1
    sc = P.Scene(obs, lights=lights)
    sc.world_tree = chain_tree(list(range(first, first + w + 1)), TAIL)
    sc.members = list(range(first, first + w + 1))
    sc.deepest = first + w                  # the chain's bottom member is the instance
    return sc


def _balanced(variant):
    """64 small quads in an 8 x 8 grid in front of the wall, a flat list: the
    SAH world builder's tree is balanced."""
    tiles = [P.quad((-1.55 + 0.4 * i, -1.55 + 0.4 * j, -2.6 + 0.05 * ((3 * i + 5 * j) % 8)), (0.3, 0, 0), (0, 0.3, 0),
                    P.lambertian(A_SHELL), f"b{i}{j}") for j in range(8) for i in range(8)]
    obs, lights = base(tiles)
    sc = P.Scene(obs, lights=lights)
    sc.world_tree, sc.members, sc.deepest = None, [], None
    return sc


# ---------------------------------------------------------------------------
# a row
# ---------------------------------------------------------------------------
def member_boxes(sc):
    """The world boxes of the deep structure's members: a shell's own, an
    instance's every triangle (in world space)."""
    out = []
    for k in sc.members:
        ob = sc.objects[k]
        if ob["kind"] == "sphere":
            out.append([x for a in range(3) for x in (ob["c"][a] - ob["r"], ob["c"][a] + ob["r"])])
        else:
            off = ob["chain"][0][1]
            for pr in ob["inner"]:
                pts = np.array([pr["a"], pr["b"], pr["c"]]) + off
                out.append(Builder._pad([x for a in range(3) for x in (pts[:, a].min(), pts[:, a].max())]))
    return out


def crosses(boxes, o, d, tmax):
    return all(P.aabb_test(bx, o, d, 0.001, tmax)[0] for bx in boxes)


class SCase(XC.XCase):
    """xform_cases.XCase whose world tree is only the description's: expected()
    works on the flat list (brute force), build() hands the tree to the
    Builder.  A tree leaf may be a tuple of world indices (an RT_LIST), and an
    instance's inner list a hand-built chain of its triangles."""

    def __init__(self, name, make, variants, check, lower=None):
        super().__init__(name, make, variants, check, "stack", prim=True)
        self.lower = lower

    @staticmethod
    def _tri_chain(b, kids):
        """BVHNode chain over the triangles, the subtree on the left (as
        chain_tree), each triangle a BVHNode{leaf, leaf} of one."""
        cur = b.leaf_node([kids[-1]])
        for k in reversed(kids[:-1]):
            cur = b.bvh_node(cur, b.leaf_node([k]))
        return cur

    def _hittables_tree(self, g, sc):
        b = Builder(g)
        ids, prim_ids = [], []
        for ob in sc.objects:
            if ob["kind"] != "wrapped":
                ids.append(self._prim(g, b, ob))
                prim_ids.append([ids[-1]])
                continue
            kids = [self._prim(g, b, pr) for pr in ob["inner"]]
            h = self._tri_chain(b, kids) if ob.get("inner_kind") == "tri_chain" else kids[0]
            for w in reversed(ob["chain"]):
                if w[0] == "translate":
                    h = b.translate(h, tuple(w[1]))
                else:
                    assert w[0] == "rot_x"
                    h = b.rotate_x(h, w[1], w[2])
            ids.append(h)
            prim_ids.append(kids)

        def tree(nd):
            if isinstance(nd, tuple):
                return b.listing([ids[k] for k in nd])
            if not isinstance(nd, dict):
                return ids[nd]
            return b.bvh_node(tree(nd["left"]), tree(nd["right"]))
        root = tree(sc.world_tree) if sc.world_tree is not None else b.listing(ids)
        b.lights = [ids[k] for k in sc.lights]
        return b, ids, prim_ids, root

    def camera(self, g, variant):
        """The grid camera; a variant outside the table (the edges' refused
        depths, built but never traced) takes depth 2."""
        self._g = g
        if variant in self.variants:
            return super().camera(g, variant)
        return XC.PC.grid_camera(g, D[0])

    def _scene(self, variant):
        if variant not in self._scenes:
            sc = self.make(variant)
            b, ids, _, _ = self._hittables_tree(self._g, sc)
            sc.boxes = [list(b.h[i].bbox) for i in ids]
            self._scenes[variant] = sc
        return self._scenes[variant]

    def build(self, g, variant):
        self._g = g
        sc = self._scene(variant)
        b, ids, self.prim_ids, root = self._hittables_tree(g, sc)
        return b, b.desc(root), self.camera(g, variant), ids


def _check_deep(case, variant, e):
    sc = e["scene"]
    boxes = member_boxes(sc)
    c = dict(cam_cross=0, cam_cross_hit=0, cam_cross_through=0, sh_cross=0, sh_cross_occ_deepest=0, sh_cross_pass=0)
    for pa, k, b in PC._bounces(e):
        if k == 0 and crosses(boxes, b["o"], b["d"], P.INF):
            c["cam_cross"] += 1
            c["cam_cross_hit" if b["obj"] in sc.members else "cam_cross_through"] += 1
    for pa, k, a, o in XC.shadow_rays(e):
        if crosses(boxes, o, a["dir"], a["end"]):
            c["sh_cross"] += 1
            c["sh_cross_pass"] += bool(a["visible"])
            c["sh_cross_occ_deepest"] += a["occluder"] == sc.deepest
    if sc.lights:
        assert c["sh_cross"] >= 12 and c["sh_cross_occ_deepest"] >= 1 and c["sh_cross_pass"] >= 1, f"{case.name}[{variant}]: {c}"
    assert c["cam_cross"] >= 12 and c["cam_cross_hit"] >= 1 and c["cam_cross_through"] >= 1, f"{case.name}[{variant}]: {c}"
    return c


def _check_inst(case, variant, e):
    c = _check_deep(case, variant, e)
    sc = e["scene"]
    c["tri_hits"] = sum(1 for pa, k, b in PC._bounces(e) if b["obj"] >= 0 and sc.objects[b["obj"]]["kind"] == "wrapped")
    c["tri_occludes"] = sum(1 for pa, k, a, o in XC.shadow_rays(e)
                            if a["occluder"] is not None and sc.objects[a["occluder"]]["kind"] == "wrapped")
    assert c["tri_hits"] >= 1, f"{case.name}[{variant}]: {c}"
    return c


def _check_balanced(case, variant, e):
    c = PC._nee_counts(e)
    c["balls_hit"] = len({b["obj"] for pa, k, b in PC._bounces(e) if b["obj"] >= 3})
    assert c["balls_hit"] >= 24, c
    return PC._need(case, variant, c, "b0_vis", "b0_occ")


# Lower bounds of a crossing ray's peak, in words, from the construction, for
# the 4-wide formats (nearest child first; the boxes nest, so the chain's
# subtree is the nearest child at every node).  The chain path's `hanging`
# items are the children of the path's BVH4 nodes that are not themselves on
# the path; however the collapse groups them, a ray that descends to the
# bottom link with every box hit holds all of them but the one it is in.
# Each returns (closest hit, shadow ray).
#   chain_ref n: n shells and at least one item for the wall's subtree hang
#     off the path; in the bottom shell the other n - 1 and that item are
#     pending: n.  A shadow ray ends before the wall and need not hold that
#     item: n - 1.  (pN, a chain of N pairs: at least one item per link.)
#   chain_dfs n: reference order pushes every hit child before it pops the
#     first, two words each: at the bottom the n shells' entries less the one
#     popped, the tilted quad's slot (never culled) and the wall's subtree:
#     2 (n + 1).  Shadow rays do not run in reference order: n - 1 words.
#   inst_leaf: W shells and the wall's subtree hang beside the leaf: W + 1
#     pending while the leaf is processed; the leaf pushes its K instances and
#     pops one (K - 1), entering it pushes the end marker (1), and at the mesh
#     chain's bottom triangle its M - 1 siblings are pending: W + K + M.  A
#     shadow ray that holds the leaf pops the next entry before the leaf is
#     processed (trav_step's postpone), a shell, and need not hold the wall's
#     subtree: W - 1 + K - 1 + 1 + M - 1.
def lower_chain_ref(variant):
    n = int(variant[1:].replace("dark", ""))
    return n, n - 1


def lower_chain_dfs(variant):
    n = int(variant[1:])
    return 2 * (n + 1), n - 1


def lower_inst_leaf(variant):
    return W_INST + K_INST + M_TRIS, W_INST + K_INST + M_TRIS - 2


D = (2, 1)          # depth 2, one sample
CASES = {c.name: c for c in [
    SCase("chain_ref", _chain_ref, {"n4": D, "n8": D, "n59": D, f"n{EDGES['chain_ref']['accepted']}": D, f"p{EDGES['wide8']['taken']}": D,
                                    f"p{EDGES['wide8']['fallback']}": D, "n12dark": (3, 1)}, _check_deep, lower_chain_ref),
    SCase("chain_dfs", _chain_dfs, {f"n{EDGES['chain_dfs']['accepted']}": D}, _check_deep, lower_chain_dfs),
    SCase("inst_leaf", _inst_leaf, {"": D}, _check_inst, lower_inst_leaf),
    SCase("device_deep", _device_deep, {f"w{W_DEVICE}": D}, _check_inst),
    SCase("balanced", _balanced, {"": D}, _check_balanced),
]}

ALL_ROWS = [(n, v) for n, c in CASES.items() for v in c.variants]
ROWS = [(n, v) for n, v in ALL_ROWS if n != "device_deep"]      # device_deep's mesh is built on the device: GPU only
# chain_dfs keeps fp32 nodes whatever is asked for (reference order)
FORMAT_ROWS = [(n, v, f) for n, v in ROWS for f in (("fp32",) if n == "chain_dfs" else ("fp32", "quant8", "wide8"))]
