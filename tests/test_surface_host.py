"""rt_gather_surface's pipeline on the host (no GPU): the production source
kernel k_gather_source<SRC_SURFACE> and the production surface instantiation of
k_shade, compiled through tests/host_emu by tests/surface_emu.cpp and driven
like run_batches' surface mode.

  * the rows of tests/surface_cases.py are what they claim, on
    tests/surface_ref.py alone (their events happen; at most 2 % of their
    point-samples are undecided);
  * a stand-alone program under AddressSanitizer + UBSan, in the three node
    formats: on path_cases' room with six white walls (the walls lifted), the
    grid camera's 24 x 16 rays, samples 0 and 1, depths 1, 2 and 5, hit points
    from the emulated closest hit, rays that meet the lamp, the blocker or the
    small triangle left out and at least 3/4 compared: the surface mode on
    {P, id, n} equals the ray mode on the ray, all bytes, with
    WaveArgs::early_miss 0 and 3; stream 0 holds exactly the valid points and
    bounce 0 leaves exactly the ray mode's survivors and NEE jobs; three samples
    in batches of 1, 2 and 3 give float(the fp64 in-order sum) and `accumulate`
    adds double(previous); with points 0, 63, 64 and the last made invalid the
    other points' bytes are unchanged; a normal scaled by 4 is the same vertex;
    the sanitizers report nothing;
  * every row against surface_ref through the same kernels as a plain library,
    the radiance held to test_path_kat.radiance_bar(group, "device"): a surface
    path is a camera path of the same scene whose first hit is given exactly, so
    the group's bar, measured for full paths, bounds it.

shade_path's NEE block is not duplicated (the surface mode is a compile-time
mode of the one function), so there are no two copies to hold to each other.

Measured worst radiance error per group (host pipeline): room 1.79e-6 (bar
1.21e-5), flat 1.15e-5 (bar 7.48e-5; mid_air, whose clamped sums reach 80),
env 2.21e-6 (bar 5.6e-6), fog 1.55e-6 (bar 2.9e-6)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import surface_cases as SC
from tests.test_path_kat import radiance_bar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
SOURCES = [os.path.join(ROOT, "tests", "surface_emu.cpp"), os.path.join(CSRC, "flatten.cpp")]
COMMON = ["-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "host_emu")]
LINK = ["-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}"]


# ---- the rows, on surface_ref alone -----------------------------------------
def test_reference_rows_are_what_they_claim(g):
    labels = set()
    for row in SC.ROWS:
        e = row.expected(g)
        print(row.summary(g))
        assert e["left_out"] <= SC.PC.LEFT_OUT_CAP * len(e["P"]) * e["samples"], row.label
        assert len(e["P"]) <= SC.GRID_W * SC.GRID_H and e["samples"] <= 5
        labels.add(row.label)
    assert len(labels) == len(SC.ROWS)
    # between them the rows show every event of the vertex
    seen = set()
    for row in SC.ROWS:
        seen |= {k for k, v in row.expected(g)["counts"].items() if v > 0}
    for k in ("area_vis", "area_occ", "cos_cut", "coslight_cut", "area_clamped", "no_area_ray", "hdri_vis", "hdri_occ",
              "area_by_fog", "light_hit_dropped", "no_nee"):
        assert k in seen, k


def test_reference_depth_one_is_the_direct_light_alone(g):
    """max_depth = 1: the vertex's NEE and nothing else; deeper rows add to it."""
    d1, d2 = SC.BY_LABEL["room-d1"].expected(g), SC.BY_LABEL["room-d2"].expected(g)
    assert d1["P"].tobytes() == d2["P"].tobytes()
    for pa, pb in zip(d1["paths"][0], d2["paths"][0]):
        assert len(pa.bounces) == 1
        direct = pa.bounces[0]["nee"]["direct"]
        np.testing.assert_array_equal(pa.L, direct)
        np.testing.assert_array_equal(pb.bounces[0]["nee"]["direct"], direct)
        assert (pb.L >= pa.L).all()


# ---- the stand-alone program under the sanitizers ---------------------------
@pytest.fixture(scope="module")
def emu_exe(tmp_path_factory, g):
    t = tmp_path_factory.mktemp("surface_emu")
    exe = t / "surface_emu"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-DSURFACE_EMU_MAIN"] + COMMON + SOURCES + LINK + ["-o", str(exe)],
                   check=True, cwd=t)
    return str(exe)


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["fp32nodes", "quant8", "wide8"])
def test_surface_mode_equals_the_ray_mode_under_asan(emu_exe, fmt):
    r = subprocess.run([emu_exe, str(fmt)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    print(info)
    assert info["ok"] == 1 and info["overflow"] == 0 and info["format"] == fmt
    assert info["rays"] == 2 * 24 * 16 and 4 * info["compared"] >= 3 * info["rays"]
    assert info["lifted"] == 8 and info["lights"] == 1       # six walls, the lamp and the blocker, tested in k_shade
    assert info["sum"] > 0                                    # the sums compared carry light


# ---- the rows against surface_ref -------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/surface_emu.cpp as a plain shared library (no sanitizer)."""
    t = tmp_path_factory.mktemp("surface_emu_lib")
    so = t / "libsurface_emu.so"
    subprocess.run(["g++", "-O2", "-shared", "-fPIC"] + COMMON + SOURCES + LINK + ["-o", str(so)], check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.surface_emu_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                    C.c_int, f32p, C.c_int, f32p, u32p]
    return lib


def emu_surface(g, lib, d, cam, pts, spp, depth, fmt=0, in_bvh=0, spb=None, sample_offset=0):
    pts = np.ascontiguousarray(pts, g.GATHER_POINT_DTYPE)
    out = np.zeros((len(pts), 3), np.float32)
    count = C.c_uint32(0)
    rc = lib.surface_emu_run(C.cast(C.pointer(d), C.c_void_p), C.cast(C.pointer(cam), C.c_void_p), fmt, in_bvh, SC.SEED,
                             sample_offset, spp, spb or spp, depth, pts.view(np.float32).ctypes.data_as(f32p), len(pts),
                             out.ctypes.data_as(f32p), C.byref(count))
    assert rc == 0, f"surface_emu_run {rc}"
    return out, count.value


HOST_RUNS = ([(r, "fp32nodes") for r in SC.ROWS] + [(r, "quant8") for r in SC.ROWS if r.case.quant8]
             + [(SC.BY_LABEL["fog_shadow"], "in_bvh")])
WORST = {}


@pytest.mark.parametrize("row,mode", HOST_RUNS, ids=[f"{r.label}-{m}" for r, m in HOST_RUNS])
def test_host_pipeline_against_the_reference(g, emu, row, mode):
    e = row.expected(g)
    print(row.summary(g))
    d, cam = row.build(g)
    pts = g.make_gather_points(e["P"], e["N"], ids=e["ids"])
    L, count = emu_surface(g, emu, d, cam, pts, e["samples"], e["depth"], fmt=1 if mode == "quant8" else 0,
                           in_bvh=1 if mode == "in_bvh" else 0)
    assert count == len(pts) * e["samples"]                  # every point is valid: stream 0 holds them all
    atol, _ = radiance_bar(row.group, "device")
    ok = e["L_ok"]
    err = float(np.abs(L.astype(np.float64)[ok] - e["L"][ok]).max())
    WORST[row.group] = max(WORST.get(row.group, 0.0), err)
    print(f"{row.label} host pipeline {mode}: radiance worst |err| {err:.3g} (bar {atol:.3g}); "
          f"worst of group {row.group} so far {WORST[row.group]:.3g}")
    assert err <= atol, f"{row.label} {mode}: radiance off by {err} (bar {atol})"
    # one sample at a time through sample_offset: the same sums up to the fp64 rounding of the total
    if row.label == "sphere_in_list":
        parts = sum(emu_surface(g, emu, d, cam, pts, 1, e["depth"], sample_offset=s)[0].astype(np.float64)
                    for s in range(e["samples"]))
        assert parts.astype(np.float32).tobytes() == L.tobytes()
