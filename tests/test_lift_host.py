"""World quads and spheres lifted out of the world BVH, on the host (no GPU).

tests/lift_emu.cpp flattens a description with FlattenOptions::lift_prims on
or off and runs the production closest-hit / any-hit kernels (k_extend,
k_shadow, one lane) followed by what the shading code adds when primitives are
lifted (lifted_prims, shade_path's NEE tests).  Checked here:

  * the flattener: which scenes lift, what a record holds, and that a scene
    that lifts nothing flattens to the same bytes as with the option off;
  * hits: every bounce's closest-hit record (t bits, ids, instance, the
    object's DFS rank) and NEE visibility with lifting on equal those with
    lifting off, and the fp32 oracle's, in every node format and under both
    world builders;
  * exact ties between a lifted quad and a triangle of an instance, another
    lifted quad, and a lifted sphere's tangent point: the oracle's winner;
  * rays within a few ulps of a lifted quad's rim: the same decision on every
    ray (the record's box confirmation; without it some of these differ).

The emulator's stand-alone program runs the same comparison on cornell-lucy's
camera rays under AddressSanitizer + UBSan.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.scene_builder import Builder, pinhole

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")
ASSETS = os.path.join(ROOT, "assets")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

FORMATS = {"fp32": 0, "quant8": 1, "wide8": 2}
TLAS = {"sah": 1, "reference": 0}      # flatten.h BLAS_SAH, BLAS_REFERENCE
PK_SPHERE, PK_QUAD = 1, 2              # dev_layout.h
REC_MAX = 8                            # dev_layout.h kPrimRecMax
SEED, SAMPLES, BOUNCES, RES = 41, (0, 1), 5, 32

f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def _sources(extra):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
            os.path.join(ROOT, "tests", "host_emu")] + extra + [
                os.path.join(ROOT, "tests", "lift_emu.cpp"), os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene",
                f"-Wl,-rpath,{LIB}"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/lift_emu.cpp as a plain shared library (no sanitizer)."""
    t = tmp_path_factory.mktemp("lift_emu")
    so = t / "liblift_emu.so"
    subprocess.run(_sources(["-O2", "-shared", "-fPIC"]) + ["-o", str(so)], check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.lift_emu_flatten.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, i32p, f32p, C.POINTER(C.c_uint64)]
    lib.lift_emu_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, i32p,
                                   f32p, f32p, C.c_int, i32p, i32p, f32p, i32p, i32p, i32p]
    lib.lift_emu_nee.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                 i32p, f32p, f32p, C.c_int, i32p, i32p]
    return lib


def _vp(x):
    return C.cast(x if isinstance(x, C._Pointer) else C.pointer(x), C.c_void_p)


# ------------------------------------------------------------------------ scenes
class Case:
    def __init__(self, name, desc, cam, keep):
        self.name, self.desc, self.cam, self.keep = name, desc, cam, keep


def _mesh_instance(b, at, size, mat):
    """A small two-triangle mesh as a bvh_node tree under a translate: the
    object that stays in the world BVH."""
    t0 = b.triangle((0, 0, 0), (size, 0, 0), (size, size, 0), mat)
    t1 = b.triangle((0, 0, 0), (size, size, 0), (0, size, 0), mat)
    return b.translate(b.bvh_node(t0, t1), list(at))


def cap_scene(g, nquads):
    """A 512 room of `nquads` world quads (six walls, a light, panels inside) and
    one mesh instance, as a world list; the camera looks in from the open side."""
    b = Builder(g)
    white, red = b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.65, 0.05, 0.05))
    R = 512.0
    quads = [b.quad((0, 0, 0), (R, 0, 0), (0, 0, R), white), b.quad((0, R, 0), (R, 0, 0), (0, 0, R), white),
             b.quad((0, 0, 0), (0, R, 0), (0, 0, R), red), b.quad((R, 0, 0), (0, R, 0), (0, 0, R), red),
             b.quad((0, 0, R), (R, 0, 0), (0, R, 0), white)]
    light = b.quad((192, R - 8, 192), (128, 0, 0), (0, 0, 128), b.light((15, 15, 15)))
    quads.append(light)
    k = 0
    while len(quads) < nquads:   # free-standing panels, none touching another
        quads.append(b.quad((64 + 96 * k, 32, 320 + 24 * k), (64, 0, 0), (0, 160, 0), white))
        k += 1
    b.lights = [light]
    inst = _mesh_instance(b, (300.0, 100.0, 200.0), 96.0, white)
    desc = b.desc(b.listing(quads + [inst]))
    o = np.array([256.0, 256.0, -600.0])
    du, dv = np.array([R / RES, 0, 0]), np.array([0, -R / RES, 0])
    p00 = np.array([0.0, R, 0.0]) + 0.5 * (du + dv)
    return Case(f"cap{nquads}", desc, pinhole(g, RES, RES, o, p00, du, dv, max_depth=5), (b, desc))


_cases = {}
NAMED = {"cornell-lucy": dict(lucy_rings=30, lucy_cols=40), "cornell": {}, "hdri-test": {}, "cornell-rotations": {},
         "random": {}}
LIFTS = {"cornell-lucy": 6, "cornell": 0, "hdri-test": 0, "cornell-rotations": 0, "random": 0, "cap8": 8, "cap9": 0}


def case(g, name):
    if name not in _cases:
        if name in NAMED:
            s = g.Scene(name, width=RES, aspect=1.0, **NAMED[name])
            _cases[name] = Case(name, s.desc, s.camera, s)
        else:
            _cases[name] = cap_scene(g, int(name[3:]))
    return _cases[name]


def top_objects(g, desc):
    """(hittable id, kind) of the world's top-level objects in the reference's
    DFS order: position = DFS rank (flatten.cpp collect_top)."""
    d = desc.contents if isinstance(desc, C._Pointer) else desc
    H, ch = d.hittables, d.children
    out = []

    def walk(i):
        h = H[i]
        if h.kind == g.RT_BVH_NODE:
            if h.a == h.b:
                c = H[h.a]
                out.extend((ch[c.a + k], H[ch[c.a + k]].kind) for k in range(c.b)) if c.kind == g.RT_BVH_LEAF \
                    else out.append((h.a, c.kind))
            else:
                walk(h.a)
                walk(h.b)
        elif h.kind in (g.RT_BVH_LEAF, g.RT_LIST):
            out.extend((ch[h.a + k], H[ch[h.a + k]].kind) for k in range(h.b))
        else:
            out.append((i, h.kind))

    walk(d.root)
    return out


# --------------------------------------------------------------------- flattener
def flat(lib, c, tlas, fmt, lift):
    out, recs, boxes = np.zeros(13, np.int32), np.zeros(8 * REC_MAX, np.int32), np.zeros(6 * REC_MAX, np.float32)
    h = C.c_uint64(0)
    rc = lib.lift_emu_flatten(_vp(c.desc), TLAS[tlas], FORMATS[fmt], int(lift), out.ctypes.data_as(i32p),
                              recs.ctypes.data_as(i32p), boxes.ctypes.data_as(f32p), C.byref(h))
    assert rc == 0 and out[0] == 0, f"{c.name}: flatten {out[0]}"
    keys = ("status", "records", "inline_items", "leaf_refs", "format", "dfs_order", "stack_needed", "tlas_depth", "nodes4",
            "refs", "quads", "spheres", "inline_items8")
    info = dict(zip(keys, out.tolist()))
    n = info["records"]
    info["recs"] = [dict(zip(("kind", "idx", "refpos", "rank", "code", "has_box", "hidx", "wref"), r))
                    for r in recs.reshape(REC_MAX, 8)[:n].tolist()]
    info["boxes"] = boxes.reshape(REC_MAX, 6)[:n]
    info["hash"] = h.value
    return info


@pytest.mark.parametrize("tlas", list(TLAS))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_cornell_lucy_lifts_its_six_world_quads(g, emu, fmt, tlas):
    c = case(g, "cornell-lucy")
    tops = top_objects(g, c.desc)
    quads = {i: rank for rank, (i, kind) in enumerate(tops) if kind == g.RT_QUAD}
    assert len(quads) == 6 and len(tops) == 16
    on, off = flat(emu, c, tlas, fmt, True), flat(emu, c, tlas, fmt, False)
    assert on["format"] == off["format"] == FORMATS[fmt]
    assert on["records"] == 6 and (on["inline_items"], on["leaf_refs"], on["inline_items8"]) == (0, 0, 0), on
    assert {r["hidx"]: r["rank"] for r in on["recs"]} == quads, on["recs"]
    H = c.desc.contents.hittables
    for r, box in zip(on["recs"], on["boxes"]):
        assert r["kind"] == PK_QUAD and r["wref"] == r["refpos"] and r["has_box"] == 1, r
        assert r["code"] & 0x80, f"an axis-aligned wall without its axis code: {r}"   # Cornell walls are axis-aligned
        assert (r["code"] & 3) == int(np.argmax(np.abs(np.array(H[r["hidx"]].p[12:15])))), r
        bb = np.array(H[r["hidx"]].bbox[:6])   # the box holds the quad's own bbox
        assert np.all(box[0::2] <= bb[0::2]) and np.all(box[1::2] >= bb[1::2]), (box, bb)
        if tlas == "sah":   # one object per leaf: its own bbox, at most an ulp wider (a reference leaf's box holds all its objects)
            assert np.all(np.abs(box - bb) <= np.spacing(np.abs(bb).astype(np.float32)) + 1e-30), (box, bb)
    # off: nothing lifted, the six quads where they were
    assert off["records"] == 0 and off["inline_items"] + off["leaf_refs"] >= 6, off
    assert off["quads"] == on["quads"] and off["refs"] == on["refs"]
    assert on["stack_needed"] <= off["stack_needed"] and on["nodes4"] <= off["nodes4"]


@pytest.mark.parametrize("tlas", list(TLAS))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", ["cornell", "hdri-test", "cornell-rotations", "random", "cap9"])
def test_scenes_that_lift_nothing_flatten_unchanged(g, emu, name, fmt, tlas):
    """cornell and hdri-test would be left with an empty world, cornell-rotations
    traverses in reference order, random and cap9 are over the cap."""
    c = case(g, name)
    on, off = flat(emu, c, tlas, fmt, True), flat(emu, c, tlas, fmt, False)
    assert on["records"] == 0 and off["records"] == 0
    assert on["hash"] == off["hash"], f"{name}: the flatten output changed with the option"
    assert {k: v for k, v in on.items() if k not in ("recs", "boxes")} == {k: v for k, v in off.items() if k not in ("recs", "boxes")}
    if name == "cornell-rotations":
        assert on["dfs_order"] == 1
    if name == "cap9":
        assert off["inline_items"] + off["leaf_refs"] == 9


@pytest.mark.parametrize("tlas", list(TLAS))
def test_cap_eight_lifts_all_eight(g, emu, tlas):
    c = case(g, "cap8")
    on, off = flat(emu, c, tlas, "fp32", True), flat(emu, c, tlas, "fp32", False)
    assert on["records"] == 8 and (on["inline_items"], on["leaf_refs"]) == (0, 0), on
    assert off["records"] == 0 and off["inline_items"] + off["leaf_refs"] == 8, off
    tops = top_objects(g, c.desc)
    assert {r["hidx"]: r["rank"] for r in on["recs"]} == {i: k for k, (i, kind) in enumerate(tops) if kind == g.RT_QUAD}
    # the world is a list: under the reference builder one leaf at the root, walked with no box test
    assert {r["has_box"] for r in on["recs"]} == ({0} if tlas == "reference" else {1})


# -------------------------------------------------------------------------- hits
_paths = {}


def oracle_paths(O, c):
    if c.name not in _paths:
        recs = []
        for s in SAMPLES:
            rec = O.path_records(c.desc, c.cam, SEED, s, BOUNCES, fp32=True)
            for a in rec:
                a.setflags(write=False)
            recs.append(rec)
        _paths[c.name] = recs
    return _paths[c.name]


def run_paths(lib, c, tlas, fmt, lift, sample, bounce, pix, o, d):
    n = len(pix)
    top, prim, inst, rank = (np.zeros(n, np.int32) for _ in range(4))
    t, info = np.zeros(n, np.float32), np.zeros(2, np.int32)
    rc = lib.lift_emu_paths(_vp(c.desc), _vp(c.cam), TLAS[tlas], FORMATS[fmt], int(lift), SEED, sample, bounce,
                            pix.ctypes.data_as(i32p), o.ctypes.data_as(f32p), d.ctypes.data_as(f32p), n,
                            top.ctypes.data_as(i32p), prim.ctypes.data_as(i32p), t.ctypes.data_as(f32p),
                            inst.ctypes.data_as(i32p), rank.ctypes.data_as(i32p), info.ctypes.data_as(i32p))
    assert rc == 0, f"{c.name}: lift_emu_paths {rc}"
    return dict(top=top, prim=prim, t=t.view(np.uint32), inst=inst, rank=rank), info


def run_nee(lib, c, tlas, fmt, lift, sample, bounce, pix, o, d):
    n = len(pix)
    vis, traced = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = lib.lift_emu_nee(_vp(c.desc), _vp(c.cam), TLAS[tlas], FORMATS[fmt], int(lift), SEED, sample, bounce,
                          c.cam.max_depth - bounce, pix.ctypes.data_as(i32p), o.ctypes.data_as(f32p), d.ctypes.data_as(f32p), n,
                          vis.ctypes.data_as(i32p), traced.ctypes.data_as(i32p))
    assert rc == 0, f"{c.name}: lift_emu_nee {rc}"
    return vis, traced


@pytest.mark.parametrize("tlas", list(TLAS))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", list(LIFTS))
def test_hits_and_shadow_visibility_equal_lifted_and_unlifted(g, O, emu, name, fmt, tlas):
    c = case(g, name)
    rays = 0
    for s, (ot, op, ott, oray, onee) in zip(SAMPLES, oracle_paths(O, c)):
        for b in range(BOUNCES):
            pix = np.flatnonzero(ot[b] != -2).astype(np.int32)
            if len(pix) == 0:
                continue
            o = np.ascontiguousarray(oray[b][pix, 0:3], np.float32)
            d = np.ascontiguousarray(oray[b][pix, 3:6], np.float32)
            on, info = run_paths(emu, c, tlas, fmt, True, s, b, pix, o, d)
            off, _ = run_paths(emu, c, tlas, fmt, False, s, b, pix, o, d)
            assert info[1] == LIFTS[name], f"{name}: {info[1]} primitives lifted"
            for k in on:
                bad = np.flatnonzero(on[k] != off[k])
                assert len(bad) == 0, f"{name} sample {s} bounce {b}: {k} differs on {len(bad)} of {len(pix)} rays, first pixel " \
                                      f"{pix[bad[0]]}: lifted {on[k][bad[0]]} unlifted {off[k][bad[0]]}"
            wt = ott[b][pix].astype(np.float32).view(np.uint32)
            bad = (on["top"] != ot[b][pix]) | (on["prim"] != op[b][pix]) | ((op[b][pix] >= 0) & (on["t"] != wt))
            assert not bad.any(), f"{name} sample {s} bounce {b}: {int(bad.sum())} of {len(pix)} hits differ from the fp32 oracle"
            if c.desc.contents.num_lights if isinstance(c.desc, C._Pointer) else c.desc.num_lights:
                von, ton = run_nee(emu, c, tlas, fmt, True, s, b, pix, o, d)
                voff, toff = run_nee(emu, c, tlas, fmt, False, s, b, pix, o, d)
                assert np.array_equal(von, voff), f"{name} sample {s} bounce {b}: {int(np.sum(von != voff))} visibilities differ"
                assert np.all((ton & ~toff) == 0), "a lifted scene traced a shadow ray the unlifted one did not"
                ov = (onee[b][pix] >> 2) & 3
                assert np.array_equal(von, ov), f"{name} sample {s} bounce {b}: {int(np.sum(von != ov))} visibilities differ " \
                                                f"from the fp32 oracle"
                if LIFTS[name]:
                    rays += int(np.sum(toff != ton))
    if LIFTS[name] and name != "cap8":
        assert rays > 0, "no shadow ray was ever stopped by a lifted primitive: the case pins nothing"


# -------------------------------------------------------------------------- ties
def tie_scene(g, kind):
    """Everything in the plane z = 0, seen straight down -z by rays whose z
    component is exactly -1 (the image plane one unit below the camera), all
    coordinates dyadic: every t is the camera's height, to the bit.
      "tri": a lifted quad coincident with a triangle pair of an instance;
      "quads": two coincident lifted quads (and the instance elsewhere);
      "sphere": a lifted sphere under the plane touching the lifted quad at
      one point, every pixel's ray aimed at it (pixel steps 0)."""
    b = Builder(g)
    white, red, blue = b.lambertian((0.7, 0.7, 0.7)), b.lambertian((0.6, 0.1, 0.1)), b.lambertian((0.1, 0.1, 0.6))
    objs = [b.quad((-4, -4, 0), (8, 0, 0), (0, 8, 0), white)]
    at = (-2.0, -2.0, 0.0) if kind == "tri" else (64.0, 64.0, 0.0)
    if kind == "quads":
        objs.append(b.quad((-2, -2, 0), (4, 0, 0), (0, 4, 0), red))
    if kind == "sphere":
        objs.append(b.sphere((0, 0, -2), 2.0, blue))
    inst = _mesh_instance(b, at, 4.0, red)
    order = [objs[0], inst] + objs[1:]   # the instance between the quads in DFS order
    desc = b.desc(b.listing(order))
    n = 16
    step = 0.0 if kind == "sphere" else 0.5
    du, dv = np.array([step, 0, 0]), np.array([0, step, 0])
    o = np.array([0.0, 0.0, 8.0])
    p00 = np.array([0.0, 0.0, 7.0]) if kind == "sphere" else np.array([-0.5 * n * step, -0.5 * n * step, 7.0]) + 0.5 * (du + dv)
    return Case(f"tie-{kind}", desc, pinhole(g, n, n, o, p00, du, dv, max_depth=2), (b, desc)), objs, inst


@pytest.mark.parametrize("tlas", list(TLAS))
@pytest.mark.parametrize("kind", ["tri", "quads", "sphere"])
def test_exact_ties_go_to_the_oracles_winner(g, O, emu, kind, tlas):
    c, objs, inst = tie_scene(g, kind)
    ot, op, ott, oray, _ = O.path_records(c.desc, c.cam, SEED, 0, 1, fp32=True)
    pix = np.arange(ot.shape[1], dtype=np.int32)
    o = np.ascontiguousarray(oray[0][:, 0:3], np.float32)
    d = np.ascontiguousarray(oray[0][:, 3:6], np.float32)
    assert np.all(d[:, 2] == -1.0)
    on, info = run_paths(emu, c, tlas, "fp32", True, 0, 0, pix, o, d)
    off, _ = run_paths(emu, c, tlas, "fp32", False, 0, 0, pix, o, d)
    assert info[1] == len(objs)
    # the tie is real: rays through the overlap see both objects at t = 8 exactly
    assert np.all(ott[0][ot[0] >= 0] == 8.0)
    second = inst if kind == "tri" else objs[1]
    assert np.any(ot[0] == second) or kind == "sphere", "no ray reached the overlap"
    for k in on:
        assert np.array_equal(on[k], off[k]), f"{kind}: {k} differs between the placements"
    assert np.array_equal(on["top"], ot[0]) and np.array_equal(on["prim"], op[0]), f"{kind}: not the oracle's winner"
    assert np.array_equal(on["t"], ott[0].astype(np.float32).view(np.uint32))
    if kind == "sphere":   # a closed primitive beats an open one at equal t: the quad
        assert np.all(ot[0] == objs[0])


# --------------------------------------------------------------------------- rim
def _step_ulps(x, k):
    out = x.copy()
    for _ in range(abs(int(np.max(np.abs(k))))):
        m = np.abs(k) > 0
        out[m] = np.nextafter(out[m], np.where(k[m] > 0, np.inf, -np.inf).astype(np.float32))
        k = k - np.sign(k)
    return out


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("tlas", list(TLAS))
def test_rim_rays_decide_alike(g, emu, tlas, fmt):
    """Rays aimed at the edges and corners of a lifted wall, every direction
    component moved by up to +-4 ulps.  The wall's box is its own extent in the
    plane and 2e-4 thick, so a ray that reaches the rim at in-plane slope
    |dx / dz| leaves the box 1e-4 |dx / dz| beyond the edge, while the quad
    test places the hit point with an error of about 2^-24 (|dx| + |x|): the
    two disagree where |dz| (1 + |x| / |dx|) exceeds about 1700.  So the
    origins lie straight in front of the targets (|dx| below 1 at |x| up to
    277, a third of them squarely in front: a direction component that is
    nearly 0) at 535 and at 20000 units, on either side of the wall, and the
    wall's corners are exact in fp32 (as a Cornell room's are), so that the
    box's planes are the quad's own edges and not an ulp outside them.  With
    the primitive's test alone about a quarter of these rays hit the wall
    where the unlifted traversal, stopped by the box, goes past it.

    The record's box is the fp32 DNode4 slot box, the box the reference tests:
    with fp32 nodes the two placements decide alike on every ray.  The
    quantised formats' traversal tests a wider box (node_quant.h), so on these
    rays it lets through hits that the fp32 traversal and the oracle do not
    see; a lifted wall does not depend on the node format, and with quant8 /
    wide8 nodes its decisions are asserted equal to the fp32 traversal's."""
    b = Builder(g)
    white = b.lambertian((0.7, 0.7, 0.7))
    Q, u, v = np.array([0.125, 0.25, 555.75]), np.array([277.25, 0, 0]), np.array([0, 311.75, 0])
    wall = b.quad(Q, u, v, white)
    side = b.quad((0.125, 0.25, 0.25), (0, 311.75, 0), (0, 0, 555.5), white)
    inst = _mesh_instance(b, (100.0, 100.0, 300.0), 50.0, white)
    # a reference-builder leaf of both quads (its box is over the two) beside the instance
    desc = b.desc(b.bvh_node(b.leaf_node([wall, side]), inst))
    cam = pinhole(g, 4, 4, (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0))
    c = Case("rim", desc, cam, (b, desc))
    rng = np.random.default_rng(1234)
    n = 6000
    ab = rng.random((n, 2))
    edge = rng.integers(0, 6, n)            # four edges, then corners twice as often as any one edge
    ab[edge == 0, 0], ab[edge == 1, 0], ab[edge == 2, 1], ab[edge == 3, 1] = 0.0, 1.0, 0.0, 1.0
    corner = edge >= 4
    ab[corner] = rng.integers(0, 2, (int(corner.sum()), 2))
    target = (Q + ab[:, :1] * u + ab[:, 1:] * v).astype(np.float32)
    shift = np.where(rng.random((n, 1)) < 1 / 3, 1e-3, 1.0) * (rng.random((n, 3)) - 0.5)
    shift[:, 2] = rng.choice([-535.0, 535.0, -20000.0, 20000.0], n)
    o = (target + shift).astype(np.float32)
    d = _step_ulps((target - o).astype(np.float32), rng.integers(-4, 5, (n, 3)))
    pix = np.zeros(n, np.int32)
    on, info = run_paths(emu, c, tlas, fmt, True, 0, 0, pix, o, d)
    off, _ = run_paths(emu, c, tlas, "fp32", False, 0, 0, pix, o, d)
    assert info[1] == 2 and info[0] == FORMATS[fmt]
    hit = int(np.sum(off["top"] == wall))
    assert 0.2 * n < hit < 0.8 * n, f"the rays do not straddle the rim: {hit} of {n} hit the wall"
    for k in on:
        bad = np.flatnonzero(on[k] != off[k])
        assert len(bad) == 0, f"{k} differs on {len(bad)} of {n} rim rays (first: ray {bad[0]})"


# ---------------------------------------------------------------- under sanitizers
def test_stand_alone_program_under_sanitizers(tmp_path, g):
    exe = tmp_path / "lift_emu"
    subprocess.run(_sources(["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                             "-fno-sanitize-recover=undefined", "-DLIFT_EMU_MAIN"]) + ["-o", str(exe)], check=True, cwd=tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "cornell-lucy", "12", ASSETS, "30", "40"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    rows = [json.loads(x) for x in r.stdout.strip().splitlines()]
    assert len(rows) == 6 and all(x["lifted"] == 6 and x["differ"] == 0 and x["hits"] > 0 for x in rows), rows
    assert [x["format_used"] for x in rows] == [0, 1, 2, 0, 1, 2]
