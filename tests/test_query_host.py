"""Ray queries on the host (no GPU): tests/query_emu.cpp compiles query.hip's
k_query for the host and runs it as 256-lane blocks, one lane at a time.

Replay: the rays of bounces 0-3 of the fp32 oracle's paths (O.path_records)
through the closest-hit kernel with tmin = 0.001, tmax = +inf, over
  * the room of tests/scale_cases.py at scales 1 and 2^10: its picture from
    inside, its axis-parallel fans, views from 64 room sizes away and one from
    inside;
  * two tests/xform_cases.py chains (six wrappers with a RotateX and a
    RotateZ: the reference-order mode; RotateY + Scale);
  * a tests/mesh_cases.py mesh under two instances;
  * cornell-rotations;
with fp32, quant8 and wide8 nodes under both world-BVH builders.  Asserted:
ids and the bits of t equal tests/hits_emu.cpp's hits_emu_run (the production
k_extend) on every scene that accepts, and the fp32 oracle's records on every
live path; the lanes of a block run in ascending and in descending order give
the same bytes; occluded(tmin, +inf) is 1 exactly where the closest hit is one.

Then the closed forms of tests/query_cases.py: interval ends and the any-hit
rule on five parallel quads, the hit record (normal, material, front flag) on a
sphere, a quad and a triangle, a moving sphere at three times, and invalid rays
among valid ones."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_cases as M
from tests import query_cases as Q
from tests import scale_cases as S
from tests import xform_cases as XC
from tests.scene_builder import Builder, pinhole

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

FORMATS = {"fp32": 0, "quant8": 1, "wide8": 2}
TLAS = {"sah": 1, "reference": 0}      # flatten.h BLAS_SAH, BLAS_REFERENCE
BLAS_SAH = 1
SEED, SAMPLE, BOUNCES = 37, 0, 4
BLOCKS = 2                             # fewer blocks than 256-ray chunks: every block loops

f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _build(t, name):
    so = t / f"lib{name}.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", f"{name}.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(so)],
                   check=True, cwd=t)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/query_emu.cpp as a plain shared library (no sanitizer)."""
    lib = _build(tmp_path_factory.mktemp("query_emu"), "query_emu")
    lib.query_emu_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_float, C.c_void_p, C.c_int, C.c_void_p, u8p, i32p]
    return lib


@pytest.fixture(scope="module")
def hits_emu(tmp_path_factory, g):
    """tests/hits_emu.cpp (the production k_extend on the host), as tests/test_scale_host.py builds it."""
    lib = _build(tmp_path_factory.mktemp("hits_emu_q"), "hits_emu")
    lib.hits_emu_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, i32p, i32p, f32p,
                                 i32p]
    return lib


def _vp(x):
    return C.cast(x if isinstance(x, C._Pointer) else C.pointer(x), C.c_void_p)


def run(g, lib, desc, cam, rays, time=0.0, any_hit=False, tlas="sah", fmt="fp32", lift=1, blocks=BLOCKS, descending=False):
    """query_emu_run: (result, info).  The error flag must stay clear."""
    rays = np.ascontiguousarray(rays, g.RAY_DTYPE)
    n = rays.shape[0]
    hits, occ, info = np.zeros(n, g.RAY_HIT_DTYPE), np.zeros(n, np.uint8), np.zeros(6, np.int32)
    rc = lib.query_emu_run(_vp(desc), _vp(cam), TLAS[tlas], BLAS_SAH, FORMATS[fmt], lift, int(any_hit), blocks,
                           int(descending), time, rays.ctypes.data_as(C.c_void_p), n, hits.ctypes.data_as(C.c_void_p),
                           occ.ctypes.data_as(u8p), info.ctypes.data_as(i32p))
    assert rc == 0 and info[4] == 0, f"query_emu_run: {rc}, error flag {info[4]}"
    return (occ if any_hit else hits), info


def any_camera(g):
    return pinhole(g, 4, 4, (0, 0, 0), (0, 0, -1), (0.1, 0, 0), (0, -0.1, 0))


# ------------------------------------------------------------------------ scenes
class Case:
    def __init__(self, name, desc, cams, keep, samples=(SAMPLE,)):
        self.name, self.desc, self.cams, self.keep, self.samples = name, desc, cams, keep, samples


def _room(g, s):
    r = S.room(g, s, 0)
    views = [v for v in r.views if v.kind == "fan"]
    views += [v for v in r.views if v.kind == "far" and v.name.startswith("far64")][:6]
    views += [v for v in r.views if v.kind == "inside"][:1]
    assert len(views) == 10
    return Case(f"room-{S.cell_id(s, 0)}", r.desc, [r.room_camera()] + [v.cam for v in views], r)


def _chain(g, name, variant):
    b, desc, cam, ids = XC.CASES[name].build(g, variant)
    return Case(f"{name}[{variant}]", desc, [cam], (b, desc), samples=(0, 1, 2, 3))   # a small grid camera: more samples


def _mesh(g):
    """tests/mesh_cases.py's 255-triangle grid twice (one BLAS, two instances) over a floor."""
    m = M.grid(255)
    b = Builder(g)
    mat = b.lambertian((0.7, 0.6, 0.5))
    lo, hi = M.bounds(m.tris)
    off = [np.array([0.5, 0.25, 0.125]), np.array([1.75, 0.5, 0.125])]
    wlo, whi = lo + off[0], hi + off[1]
    c, e = 0.5 * (wlo + whi), float(np.max(whi - wlo))
    floor = b.quad([c[0] - 3 * e, c[1] - 3 * e, wlo[2] - 0.25 * e], [6 * e, 0, 0], [0, 6 * e, 0], b.lambertian((0.6, 0.6, 0.6)))
    light = b.quad([c[0] - 0.5 * e, c[1] - 0.5 * e, whi[2] + 6 * e], [e, 0, 0], [0, e, 0], b.light((60, 60, 60)))
    b.lights = [light]
    ids = [b.triangle(t[0], t[1], t[2], mat) for t in m.tris]

    def tree(sel):
        return sel[0] if len(sel) == 1 else b.bvh_node(tree(sel[:len(sel) // 2]), tree(sel[len(sel) // 2:]))
    root = tree(ids)
    desc = b.desc(b.listing([floor, light] + [b.translate(root, list(o)) for o in off]))
    cams = []
    for v in (M.front(wlo, whi), M.side(wlo, whi), M.top(wlo, whi)):
        o, p00, du, dv = M.view_rays(v._replace(res=32))
        cams.append(pinhole(g, 32, 32, o, p00, du, dv, max_depth=5))
    return Case("mesh-two-instances", desc, cams, (b, desc))


def _named(g, name):
    s = g.Scene(name, width=32, aspect=1.0)
    return Case(name, s.desc, [s.camera], s)


MAKERS = {
    "room-s1": lambda g: _room(g, 1.0),
    "room-s2^10": lambda g: _room(g, 2.0 ** 10),
    "chain-len6": lambda g: _chain(g, "wrap_long", "len6"),
    "chain-rot_y+scale": lambda g: _chain(g, "wrap_pairs", "rot_y+scale"),
    "mesh-two-instances": _mesh,
    "cornell-rotations": lambda g: _named(g, "cornell-rotations"),
}
REFERENCE_ORDER = {"chain-len6", "cornell-rotations"}   # RotateX / RotateZ: the kVol variant, fp32 nodes as written
_cases, _paths = {}, {}


def case(g, name):
    if name not in _cases:
        _cases[name] = MAKERS[name](g)
    return _cases[name]


def oracle_rays(g, O, c):
    """Every live path's ray of bounces 0..3 of every camera of the case, with
    the fp32 oracle's record for it; computed once, read-only."""
    if c.name not in _paths:
        o, d, top, prim, t = [], [], [], [], []
        for cam, smp in ((cam, smp) for cam in c.cams for smp in c.samples):
            ot, op, ott, oray, _ = O.path_records(c.desc, cam, SEED, smp, BOUNCES, fp32=True)
            for b in range(BOUNCES):
                live = np.flatnonzero(ot[b] != -2)
                o.append(oray[b][live, 0:3]); d.append(oray[b][live, 3:6])
                top.append(ot[b][live]); prim.append(op[b][live]); t.append(ott[b][live])
        rec = dict(rays=g.make_rays(np.concatenate(o), np.concatenate(d)), top=np.concatenate(top).astype(np.int32),
                   prim=np.concatenate(prim).astype(np.int32), t=np.concatenate(t).astype(np.float32))
        for a in rec.values():
            a.setflags(write=False)
        _paths[c.name] = rec
    return _paths[c.name]


# ------------------------------------------------------------------------ replay
@pytest.mark.parametrize("tlas", list(TLAS))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", list(MAKERS))
def test_replay_equals_k_extend_and_the_fp32_oracle(g, O, emu, hits_emu, name, fmt, tlas):
    c = case(g, name)
    ref = oracle_rays(g, O, c)
    rays, n = ref["rays"], ref["rays"].shape[0]
    assert n > 256 * BLOCKS, f"{name}: {n} rays do not make a block loop"
    h, info = run(g, emu, c.desc, c.cams[0], rays, tlas=tlas, fmt=fmt)
    assert bool(info[5]) == (name in REFERENCE_ORDER), f"{name}: rare-primitive variant {info[5]}"
    assert info[0] == (0 if name in REFERENCE_ORDER else FORMATS[fmt]), f"{name}: node format {info[0]}"
    tb = h["t"].view(np.uint32)
    # the fp32 oracle's records, on every live path
    hit = ref["prim"] >= 0
    assert hit.any() and (name.startswith("room") or (~hit).any() or name == "mesh-two-instances")
    bad = (h["top"] != ref["top"]) | (h["prim"] != ref["prim"]) | (hit & (tb != ref["t"].view(np.uint32)))
    assert not bad.any(), f"{name} {fmt} {tlas}: {int(bad.sum())} of {n} rays differ from the fp32 oracle, first " \
                          f"{int(np.flatnonzero(bad)[0])}: {h[np.flatnonzero(bad)[0]]} vs " \
                          f"{(ref['top'][bad][0], ref['prim'][bad][0], ref['t'][bad][0])}"
    assert np.all(h["t"][~hit] == -1.0) and not h["flags"][~hit].any() and not h["n"][~hit].any()
    assert np.all(h["material"][hit] >= 0) and np.all(h["material"][~hit] == -1)
    nn = np.linalg.norm(h["n"][hit].astype(np.float64), axis=1)
    assert np.all(np.abs(nn - 1.0) < 1e-4), f"{name}: normal lengths {nn.min()} .. {nn.max()}"
    # the production k_extend on the host, where it accepts the scene
    top, prim, t = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    used = C.c_int32(-1)
    o, d = np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])
    rc = hits_emu.hits_emu_run(_vp(c.desc), _vp(c.cams[0]), TLAS[tlas], BLAS_SAH, FORMATS[fmt], o.ctypes.data_as(f32p),
                               d.ctypes.data_as(f32p), n, top.ctypes.data_as(i32p), prim.ctypes.data_as(i32p),
                               t.ctypes.data_as(f32p), C.byref(used))
    assert rc == (3 if name in REFERENCE_ORDER else 0), f"hits_emu_run: {rc}"
    if rc == 0:
        assert used.value == info[0]
        assert np.array_equal(h["top"], top) and np.array_equal(h["prim"], prim) and np.array_equal(tb, t.view(np.uint32))
    # lanes in descending order: the same bytes
    hd, _ = run(g, emu, c.desc, c.cams[0], rays, tlas=tlas, fmt=fmt, descending=True)
    assert hd.tobytes() == h.tobytes(), f"{name}: the lane order shows in the closest hits"
    # one block and many give the same
    h1, _ = run(g, emu, c.desc, c.cams[0], rays[:1100], tlas=tlas, fmt=fmt, blocks=1)
    assert h1.tobytes() == h[:1100].tobytes()
    # any hit over (tmin, +inf) is the closest hit hitting, in both lane orders
    occ, _ = run(g, emu, c.desc, c.cams[0], rays, any_hit=True, tlas=tlas, fmt=fmt)
    assert np.array_equal(occ != 0, hit), f"{name}: {int(np.sum((occ != 0) != hit))} occlusion results differ"
    occ_d, _ = run(g, emu, c.desc, c.cams[0], rays, any_hit=True, tlas=tlas, fmt=fmt, descending=True)
    assert occ_d.tobytes() == occ.tobytes()


def test_lifting_does_not_show(g, O, emu):
    """The room's world quads are lifted out of the BVH by default: the same
    records with them left in it."""
    c = case(g, "mesh-two-instances")
    rays = oracle_rays(g, O, c)["rays"]
    on, i_on = run(g, emu, c.desc, c.cams[0], rays, lift=1)
    off, i_off = run(g, emu, c.desc, c.cams[0], rays, lift=0)
    assert i_on[3] == 2 and i_off[3] == 0, (i_on, i_off)    # the floor and the light
    assert on.tobytes() == off.tobytes()
    o_on, _ = run(g, emu, c.desc, c.cams[0], rays, any_hit=True, lift=1)
    o_off, _ = run(g, emu, c.desc, c.cams[0], rays, any_hit=True, lift=0)
    assert o_on.tobytes() == o_off.tobytes()


def test_volume_scene_is_refused(g, emu):
    b = Builder(g)
    wm = b.lambertian((0.5, 0.5, 0.5))
    fog = b.volume(b.listing(b.box_quads((-1, -1, -3), (1, 1, -2), wm)), 0.5, b.mat(g.RT_ISOTROPIC, b.solid((1, 1, 1))))
    wall = b.quad((-4, -4, -5), (8, 0, 0), (0, 8, 0), wm)
    desc = b.desc(b.listing([fog, wall]))
    rays = g.make_rays([[0, 0, 0]], [[0, 0, -1]])
    hits, occ, info = np.zeros(1, g.RAY_HIT_DTYPE), np.zeros(1, np.uint8), np.zeros(6, np.int32)
    rc = emu.query_emu_run(_vp(desc), _vp(any_camera(g)), 1, 1, 0, 1, 0, 1, 0, 0.0, rays.ctypes.data_as(C.c_void_p), 1,
                           hits.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(u8p), info.ctypes.data_as(i32p))
    assert rc == 2


# ------------------------------------------------------------------ closed forms
@pytest.fixture(params=[("fp32", "sah", 1), ("quant8", "sah", 1), ("wide8", "sah", 1), ("fp32", "reference", 1),
                        ("fp32", "sah", 0)], ids=lambda p: f"{p[0]}-{p[1]}-lift{p[2]}")
def trace(request, g, emu):
    fmt, tlas, lift = request.param
    cam = any_camera(g)

    def f(desc, rays, time, any_hit):
        a, _ = run(g, emu, desc, cam, rays, time=time, any_hit=any_hit, tlas=tlas, fmt=fmt, lift=lift, blocks=1)
        d, _ = run(g, emu, desc, cam, rays, time=time, any_hit=any_hit, tlas=tlas, fmt=fmt, lift=lift, blocks=1, descending=True)
        assert a.tobytes() == d.tobytes()
        return a
    return f


def test_interval_and_any_hit_rule(g, trace):
    Q.check_intervals(g, trace)


def test_hit_record(g, trace):
    Q.check_records(g, trace)


def test_moving_sphere(g, trace):
    Q.check_moving(g, trace)


def test_invalid_rays(g, trace):
    Q.check_invalid(g, trace)
