"""rt_ray_color's path integral against float64, on the CPU: the ray sets of
tests/ray_color_cases.py (an orthographic grid with a skewed non-unit
direction, a probe's every direction from one point; ids 1000 + 7 k, 2 samples)
over rows of tests/path_cases.py, expected values from tests/path_ref.py's
rayColorInternal on the float32 rays, held against

  * the rows themselves, on path_ref alone: at most 2 % of a row's ray-samples
    left out (measured: room[d3] 4 / 2, fog_shadow 5 / 1, glass_chain 1 / 0,
    mirror_chain 1 / 0 of 768 on ortho / probe, every other row 0), and what
    each row is there for: the probe sets miss at bounce 0 (714 - 718 of 768 on
    the env rows), phantom[at_max] and phantom[below] differ on the probe set
    (mean radiance 0.037 against 1.84: the depth == camera_max_depth rule),
    room averages more than 2.9 bounces;
  * the oracle in both modes.  The oracle is not the code under test and has
    no ray entry point, but it traces any ray through a degenerate camera:
    center = o, pixel00 = o + d, pixel_delta_u = pixel_delta_v = 0, no
    defocus, with the row's background, sky, phantom and max_depth fields, so
    every pixel's ray is (o, d) whatever the jitter, and ray k is read from the
    pixel whose index is its id.  The image is 6370 x 1 (wide enough for id
    1000 + 7 * 767) and each render is the one-pixel bucket at x = id, one
    render per ray.  In float64 o + d and (o + d) - o are exact for these
    rays; in the fp32 mode pixel00 rounds, which is part of the figure below;
  * the production pipeline on the host (tests/ray_color_emu.cpp as a plain
    ctypes library: k_ray_source, then the later-bounce kernels from bounce 0),
    fog_shadow in both volume placements.

Bars.  The fp64 oracle: tests/test_path_kat.py's FP64 bars.  The fp32 oracle:
its measured worst absolute error of the summed radiance against path_ref,
per path_cases group, x 1.05 for the figure's rounding; the host pipeline and
the GPU (tests/test_gpu_ray_color.py): 4 x the figure, the project's margin for
ocml against glibc and for operation order.

  group  rows                                        fp32 oracle, radiance |err|   host pipeline (measured)
  room   room[d3]                                    3.26e-6 (probe)               3.28e-6
  flat   lights3 glass_chain mirror_chain clamp_b1   6.62e-6 (clamp_b1 probe)      6.42e-6
  env    env_gate[env+light] phantom (2)             3.50e-6 (probe)               1.98e-6
  fog    fog_shadow                                  6.39e-7 (ortho)               7.54e-7

The fp64 oracle measures at most 7.1e-15 absolute (clamp_b1, sums near 30) and
nothing past the relative bar."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import path_cases as PC
from tests import ray_color_cases as RC
from tests.test_path_kat import FP64, FP64_ZERO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")

# the fp32 oracle's worst |error| of the summed radiance against path_ref, per group (the table above)
MEASURED_FP32 = {"room": 3.26e-6, "flat": 6.62e-6, "env": 3.50e-6, "fog": 6.39e-7}
ORACLE_WIDTH = int(RC.IDS.max()) + 1

f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
ROW_IDS = [f"{n}-{v}" if v else n for n, v in RC.ROWS]


def radiance_bar(group, who):
    """(atol, rtol) of a row's summed radiance."""
    if who == "fp64":
        return FP64_ZERO, FP64
    return (1.05 if who == "fp32" else 4.0) * MEASURED_FP32[group], 0.0


def check_radiance(what, case, e, L, who):
    atol, rtol = radiance_bar(case.group, who)
    err = PC.radiance_error(e, L)
    print(f"{what}: radiance worst |err| {err:.3g} (bar {atol:.3g})")
    over = PC.radiance_error(e, L, rtol)
    assert over <= atol, f"{what}: radiance off by {err} (past rtol {rtol} by {over}, atol {atol})"


# ---- the rows, on path_ref alone --------------------------------------------
def test_reference_rows_are_what_they_claim():
    e = {(n, v, s): RC.expected(n, v, s) for n, v in RC.ROWS for s in RC.SETS}
    total = RC.N * RC.SAMPLES
    for (n, v, s), x in e.items():
        print(RC.summary(n, v, s))
        assert x["left_out"] <= PC.LEFT_OUT_CAP * total, (n, v, s)
        assert x["left_out"] < 0.007 * total
    for n, v in (("env_gate", "env+light"), ("phantom", "at_max"), ("phantom", "below")):
        assert 714 <= e[(n, v, "probe")]["b0_miss"] <= 718          # the probe looks past the small wall
        assert e[(n, v, "ortho")]["b0_miss"] == 0                   # the grid is all on it
    at_max, below = e[("phantom", "at_max", "probe")], e[("phantom", "below", "probe")]
    assert at_max["depth"] == PC.PHANTOM_CAM_DEPTH == below["depth"] + 1
    assert at_max["L"].mean() / RC.SAMPLES < 0.06 and below["L"].mean() / RC.SAMPLES > 1.5
    for s in RC.SETS:
        assert e[("room", "d3", s)]["bounces"] > 2.9
    # distinct ids, distinct paths: the two samples of a ray differ, and so do neighbours with one origin and direction
    room = e[("room", "d3", "ortho")]
    assert sum(1 for k in range(RC.N) if not np.array_equal(room["paths"][0][k].L, room["paths"][1][k].L)) > RC.N // 2


# ---- the oracle through a degenerate camera ------------------------------------
def oracle_ray_colors(g, O, case, variant, rset, fp32):
    """(N, 3) float64: the oracle's sums for the set's rays, one one-pixel render per ray."""
    e = RC.expected(case.name, variant, rset)
    b, d, cam, ids = case.build(g, variant)
    o, dr = RC.ray_set(rset)
    o, dr = o.astype(np.float64), dr.astype(np.float64)
    cam.image_width, cam.image_height = ORACLE_WIDTH, 1
    cam.defocus_angle = 0.0
    for a in range(3):
        cam.pixel_delta_u[a] = cam.pixel_delta_v[a] = 0.0
    out = np.zeros((RC.N, 3))
    acc = np.zeros((1, ORACLE_WIDTH, 3))
    for k in range(RC.N):
        pid = int(RC.IDS[k])
        for a in range(3):
            cam.center[a] = o[k, a]
            cam.pixel00[a] = o[k, a] + dr[k, a]
            assert cam.pixel00[a] - cam.center[a] == dr[k, a]        # exact in float64
        acc[0, pid] = 0.0
        p = g.make_params(RC.SAMPLES, e["depth"], seed=RC.SEED, buckets=[(pid, 0, 1, 1)])
        O.render(d, cam, p, fp32=fp32, threads=1, accum=acc)
        out[k] = acc[0, pid]
    return out


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,variant", RC.ROWS, ids=ROW_IDS)
def test_oracle_ray_color(g, O, name, variant, fp32):
    case = PC.CASES[name]
    who = "fp32" if fp32 else "fp64"
    for rset in RC.SETS:
        L = oracle_ray_colors(g, O, case, variant, rset, fp32)
        check_radiance(f"{name}[{variant}] {rset} {who} oracle", case, RC.expected(name, variant, rset), L, who)


# ---- the production pipeline on the host -------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/ray_color_emu.cpp as a plain shared library (no sanitizer)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    t = tmp_path_factory.mktemp("ray_color_kat")
    so = t / "libray_color_emu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "ray_color_emu.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(so)],
                   check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.ray_color_emu_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                      C.c_int, f32p, C.c_int, f32p, u32p]
    return lib


def emu_ray_color(g, lib, d, cam, rays, samples, depth, in_bvh=0, spb=0):
    rays = np.ascontiguousarray(rays, g.PATH_RAY_DTYPE)
    out = np.zeros((len(rays), 3), np.float32)
    count = C.c_uint32(0)
    rc = lib.ray_color_emu_run(C.cast(C.pointer(d), C.c_void_p), C.cast(C.pointer(cam), C.c_void_p), 0, in_bvh, RC.SEED, 0,
                               samples, spb or samples, depth, rays.ctypes.data_as(f32p), len(rays), out.ctypes.data_as(f32p),
                               C.byref(count))
    assert rc == 0, f"ray_color_emu_run {rc}"
    return out, count.value


HOST_RUNS = [(n, v, 0) for n, v in RC.ROWS] + [("fog_shadow", "", 1)]


@pytest.mark.parametrize("name,variant,in_bvh", HOST_RUNS, ids=ROW_IDS + ["fog_shadow-in_bvh"])
def test_host_pipeline_ray_color(g, emu, name, variant, in_bvh):
    case = PC.CASES[name]
    b, d, cam, ids = case.build(g, variant)
    for rset in RC.SETS:
        e = RC.expected(name, variant, rset)
        o, dr = RC.ray_set(rset)
        rays = g.make_path_rays(o, dr, RC.IDS)
        L, count = emu_ray_color(g, emu, d, cam, rays, RC.SAMPLES, e["depth"], in_bvh)
        assert count == RC.N * RC.SAMPLES                 # every ray is valid: the whole batch is in the stream
        check_radiance(f"{name}[{variant}] {rset} host pipeline{' in_bvh' if in_bvh else ''}", case, e, L, "device")
        if name == "room":                                # one sample per batch: the same bytes
            assert emu_ray_color(g, emu, d, cam, rays, RC.SAMPLES, e["depth"], in_bvh, spb=1)[0].tobytes() == L.tobytes()
