"""transform.go's wrapper chains against float64, on the CPU: the rows of
tests/xform_cases.py, whose expected values come from tests/path_ref.py's
`wrapped` objects (the five wrappers restated from the Go text, as written),
held against

  * the rows themselves, on path_ref alone: their counts, the 2 % cap, that
    the two orders of every unequal pair of kinds differ, that the list and
    leaf-node variants of `wrap_inner` give identical ids, and that the
    reported hit point lies on the incoming ray for chains without RotateX /
    RotateZ (1e-9) and off it by more than 1e-3 somewhere for chains with
    them (`wrap_each[rot_x_180]` turns P by 360 degrees in all and is held
    to the first);
  * the oracle in both modes: every bounce and the radiance;
  * the production kernels on the host (tests/hits_emu.cpp): the closest hit
    of path_ref's own rays of every bounce (`hits_emu_run_paths`) and the
    frame (`hits_emu_render_opts`), every row in the fp32 node format,
    `wrap_long` and `wrap_inner` also with quant8 and wide8 nodes and the
    reference world builder, the node format taken asserted; `wrap_inner`
    compares the inner primitive hit too;
  * flatten_scene's refusals: a chain of seven and a wrapped plane.

The long-tail kernel takes paths only in scenes without a light; every row
here has one, so no row runs through it.

Tolerances: tests/test_path_kat.py's (ids, ended paths, NEE bits and the
node format exact; the fp64 oracle 1e-12; bounce-0 rays atol 1e-5), with the
fp32 oracle's measured worst error against path_ref per group and bounce in
its MEASURED_FP32 (`chain`, `stretch`, `tree`; the table is in that file's
docstring): the oracle is held to 1.05 x, the host to 4 x."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import path_cases as PC
from tests import xform_cases as XC
from tests.scene_builder import Builder
from tests.test_path_kat import CSRC, LIB, MEASURED_FP32, ROOT, _vp, check_radiance, check_records, f32p, i32p

FORMATS = {"fp32": 0, "quant8": 1, "wide8": 2}
TLAS_REFERENCE, TLAS_SAH = 0, 1
RT_ERR_UNSUPPORTED = -2
ROW_IDS = [f"{n}-{v}" if v else n for n, v in XC.ROWS]


def grp(c, v):
    return types.SimpleNamespace(group=c.group_of(v))


def taken(c, v, mode):
    """The node format the scene takes under `mode`: RotateX / RotateZ scenes
    keep fp32 nodes whatever is asked for (flatten.cpp); wide8 is not taken
    with circles."""
    if c.as_written(v) or mode not in ("quant8", "wide8"):
        return FORMATS["fp32"]
    if mode == "wide8":
        return FORMATS["fp32"] if c.has_circle(v) else FORMATS["wide8"]
    return FORMATS["quant8"]


# ---- on path_ref alone ------------------------------------------------------
def test_rows_are_what_they_claim(g):
    for n, v in XC.ROWS:
        c = XC.CASES[n]
        e = c.expected(g, v)
        print(c.summary(g, v))
        assert e["left_out"] <= PC.LEFT_OUT_CAP * PC.N * e["samples"], (n, v)
    print("wrap_pairs, the two orders apart by", {f"{a}/{b}": round(w, 4) for (a, b), w in XC.pair_orders_differ(g).items()})
    a, b = XC.CASES["wrap_inner"].expected(g, "list"), XC.CASES["wrap_inner"].expected(g, "leaf")
    assert all(np.array_equal(x, y) for x, y in zip(a["obj"], b["obj"]))
    assert [[bn["sub"] for bn in pa.bounces] for pa in a["paths"][0]] == [[bn["sub"] for bn in pa.bounces] for pa in b["paths"][0]]


def test_hit_point_on_or_off_the_ray(g):
    """o + t d of a bounce-0 hit of a wrapped object against the origin of
    the scattered ray (rec.P): the same point (1e-9) unless the chain holds
    a RotateX / RotateZ, and then off it by more than 1e-3 somewhere."""
    for n, v in XC.ROWS:
        c = XC.CASES[n]
        e = c.expected(g, v)
        sc = e["scene"]
        worst = {}
        for pa, k, b in PC._bounces(e):
            if k == 0 and b["obj"] >= 0 and sc.objects[b["obj"]]["kind"] == "wrapped" and "scatter" in b:
                off = float(np.abs(b["o"] + b["d"] * b["t"] - b["scatter"][0]).max())
                q = any(w[0] in XC.QUIRK_KINDS for w in sc.objects[b["obj"]]["chain"]) and (n, v) not in XC.NO_QUIRK
                worst[q] = max(worst.get(q, 0.0), off)
        print(f"{n}[{v}]: rec.P off the ray by {worst}")
        assert worst.get(False, 0.0) <= 1e-9, (n, v, worst)
        assert (True in worst) == c.quirk(v), (n, v)
        if c.quirk(v):
            assert worst[True] > 1e-3, (n, v, worst)


# ---- the oracle, both modes -------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,variant", XC.ROWS, ids=ROW_IDS)
def test_oracle_wrapper_chains(g, O, name, variant, fp32):
    c = XC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    who = "fp32" if fp32 else "fp64"
    b, d, cam, ids = c.build(g, variant)
    what = f"{name}[{variant}] {who} oracle"
    for s in range(e["samples"]):
        top, prim, t, ray, nee = O.path_records(d, cam, PC.SEED, s, e["depth"], fp32=fp32, threads=2)
        for k in range(e["depth"]):
            check_records(what, grp(c, variant), e, ids, s, k, top[k], t[k], ray[k], nee[k], who, bits="nee_dev")
            if c.prim:
                check_prims(what, c, e, s, k, prim[k])
    L = O.render(d, cam, g.make_params(e["samples"], e["depth"], seed=PC.SEED), fp32=fp32, threads=2)
    check_radiance(what, grp(c, variant), e, L, who)


@pytest.mark.parametrize("name,variant", [r for r in XC.FEATURE_ROWS if r[0] != "wrap_inner"],
                         ids=[f"{n}-{v}" for n, v in XC.FEATURE_ROWS if n != "wrap_inner"])
def test_ball_normal_figure(g, O, name, variant):
    """The bar of a wrapped sphere's feature normal (tests/test_gpu_xform_kat.py):
    unit(A^T (P - c) / r) in float32 from the fp32 oracle's t against the
    same in float64, within 1.05 x the group's figure."""
    c = XC.CASES[name]
    b, d, cam, ids = c.build(g, variant)
    want, flat, ball = XC.expected_normals(c, g, variant)
    assert ball.sum() >= 12 and flat.sum() >= 12
    t = O.path_records(d, cam, PC.SEED, 0, 1, fp32=True, threads=2)[2]
    err = float(np.abs(XC.ball_normals_f32(c, g, variant, t[0])[ball] - want[ball]).max())
    bar = 1.05 * MEASURED_FP32[c.group_of(variant)]["n_ball"]
    print(f"{name}[{variant}]: {int(ball.sum())} sphere pixels, float32 normal off by {err:.3g} (bar {bar:.3g})")
    assert err <= bar


def check_prims(what, c, e, s, k, prim):
    """The inner primitive hit, where float64 decides the hit."""
    ok = e["hit_ok"][s][k] & (e["obj"][s][k] >= 0)
    want = np.array([c.prim_ids[bn["obj"]][max(bn["sub"], 0)] if bn["obj"] >= 0 else -1
                     for bn in (pa.bounces[k] if k < len(pa.bounces) else dict(obj=-1) for pa in e["paths"][s])], np.int32)
    bad = np.flatnonzero((np.asarray(prim) != want) & ok)
    assert len(bad) == 0, f"{what} s{s} b{k}: prims differ at pixels {bad[:8]}: {np.asarray(prim)[bad[:8]]} want {want[bad[:8]]}"


# ---- the production kernels on the host -----------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/hits_emu.cpp as a plain shared library (no sanitizer)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    t = tmp_path_factory.mktemp("xform_emu")
    so = t / "libhits_emu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "hits_emu.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(so)],
                   check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.hits_emu_render_opts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, f32p,
                                         C.c_int, i32p]
    lib.hits_emu_run_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int,
                                       i32p, f32p, f32p, C.c_int, i32p, i32p, f32p, i32p]
    lib.hits_emu_flatten_status.argtypes = [C.c_void_p, C.c_int]
    return lib


def emu_paths(lib, d, cam, e, s, k, fmt, tlas):
    """The production closest hit of path_ref's own bounce-k rays, rounded to
    fp32: (top, prim, t) over all pixels (an ended path: -2, as the reference
    has it: it has no ray to trace), and the node format run."""
    want = e["obj"][s][k]
    pix = np.flatnonzero(want != -2).astype(np.int32)
    o = np.ascontiguousarray(e["ray"][s][k][pix, 0:3], np.float32)
    dd = np.ascontiguousarray(e["ray"][s][k][pix, 3:6], np.float32)
    n = len(pix)
    top, prim, t = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    used = C.c_int32(-1)
    rc = lib.hits_emu_run_paths(_vp(d), _vp(cam), tlas, fmt, 1, PC.SEED, s, k, pix.ctypes.data_as(i32p),
                                o.ctypes.data_as(f32p), dd.ctypes.data_as(f32p), n, top.ctypes.data_as(i32p),
                                prim.ctypes.data_as(i32p), t.ctypes.data_as(f32p), C.byref(used))
    assert rc == 0, f"hits_emu_run_paths {rc}"
    full_top, full_prim, full_t = np.full(PC.N, -2, np.int32), np.full(PC.N, -2, np.int32), np.full(PC.N, -1.0)
    full_top[pix], full_prim[pix], full_t[pix] = top, prim, t
    return full_top, full_prim, full_t, used.value


HOST_RUNS = [(n, v, "fp32nodes") for n, v in XC.ROWS] + XC.MODE_ROWS


@pytest.mark.parametrize("name,variant,mode", HOST_RUNS, ids=["-".join(x for x in r if x) for r in HOST_RUNS])
def test_host_wrapper_chains(g, emu, name, variant, mode):
    c = XC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    b, d, cam, ids = c.build(g, variant)
    fmt = FORMATS.get(mode, 0)
    tlas = TLAS_REFERENCE if mode == "tlas_reference" else TLAS_SAH
    what = f"{name}[{variant}] host {mode}"
    for s in range(e["samples"]):
        for k in range(e["depth"]):
            top, prim, t, used = emu_paths(emu, d, cam, e, s, k, fmt, tlas)
            assert used == taken(c, variant, mode), f"{what}: node format {used}"
            # the rays are the reference's own: their error is the rounding to fp32
            check_records(what, grp(c, variant), e, ids, s, k, top, t, e["ray"][s][k].astype(np.float32), None, "device")
            if c.prim:
                check_prims(what, c, e, s, k, prim)
    out = np.zeros((PC.N, 3), np.float32)
    used = C.c_int32(-1)
    rc = emu.hits_emu_render_opts(_vp(d), _vp(cam), fmt, tlas, PC.SEED, 0, e["samples"], e["depth"], out.ctypes.data_as(f32p), 0,
                                  C.byref(used))
    assert rc == 0, f"hits_emu_render_opts {rc}"
    assert used.value == taken(c, variant, mode), f"{what}: node format {used.value}"
    check_radiance(what, grp(c, variant), e, out, "device")


# ---- refusals -------------------------------------------------------------------
def valid_scene(g):
    c = XC.CASES["wrap_long"]
    return c.build(g, "len6")


def chain_of_seven(g):
    b = Builder(g)
    h = b.quad((-0.5, -0.5, -2.0), (1, 0, 0), (0, 1, 0), b.lambertian((0.5, 0.5, 0.5)))
    for k in range(7):
        h = b.translate(h, (0.01 * k, 0.0, 0.0))
    return b, b.desc(b.listing([h]))


def wrapped_plane(g):
    b = Builder(g)
    h = b.translate(b.plane((0, -1, 0), (0, 1, 0), b.lambertian((0.5, 0.5, 0.5))), (0.0, 0.5, 0.0))
    return b, b.desc(b.listing([h]))


@pytest.mark.parametrize("make", [chain_of_seven, wrapped_plane], ids=["chain_of_seven", "wrapped_plane"])
def test_host_refusals(g, emu, make):
    b, d = make(g)
    assert emu.hits_emu_flatten_status(_vp(d), 1) == RT_ERR_UNSUPPORTED
    vb, vd, cam, ids = valid_scene(g)
    assert emu.hits_emu_flatten_status(_vp(vd), 1) == 0
