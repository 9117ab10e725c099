"""The path integral against float64, on the CPU: the rows of
tests/path_cases.py (NEE at every bounce, the light-hit rule, depth, light
selection, the clamp, area-light geometry, shadow rays, the order and weight
of the adds), whose expected values come from tests/path_ref.py, a recursive
float64 restatement of camera.go:443-678 from the Go text alone, held against

  * the rows themselves (their counts, at most 2 % of the pixel-samples left
    out, the recursion against an iterative sum), on path_ref alone;
  * the oracle in both modes: `O.path_records` for every bounce to the row's
    depth (ids, ended paths and the NEE wanted / visible bits exact, rays and
    t within tolerance) and `O.render` for the radiance;
  * the production wavefront pipeline on the host (tests/hits_emu.cpp
    `hits_emu_render`: camera, extend, shade, shadow, NEE apply, accumulate,
    finalize as tests/wave_run.h drives them, a plain ctypes library): the
    radiance of every row in the fp32 node format, of `room`, `lights3` and
    `env_is_area` in quant8 too, and of `fog_shadow` with the volume lifted
    and in the BVH.

Every row prints its depth, samples, the pixel-samples compared and left out
and its counts, and every comparison its worst error (pytest -s).

Tolerances.  Exact: ids, ended paths, the NEE bits.  Which light was chosen
is not in what `path_records`, rt_shadow_visibility or the frame report: it is
held through the bits and the radiance there, and exactly (through the shadow
ray's direction) by test_host_shade_path_nee_records.  The fp64 oracle:
radiance and t 1e-12 relative (radiance 1e-15 where the expected value is 0),
ray coordinates 1e-12 absolute (looser than relative for components below 1;
the accumulated error of five bounces is absolute, measured 1.1e-13; it is how
test_shade_kat holds its rays).  fp32 at bounce 0: rays atol 1e-5, t rtol 2e-6, the project's bars.
Past bounce 0 the bar is the fp32 oracle's measured worst error against
path_ref on the CPU, per group of rows and per bounce: the oracle itself is
held to the figure (x 1.05 for the figure's rounding), the host pipeline and
the GPU (tests/test_gpu_path_kat.py) to 4 x it (ocml against glibc, operation
order).  Radiance is the sum of the row's samples, absolute error.

  group  rows                                       fp32 oracle: rays (abs) at bounce 1..   t (rel) at bounce 1..          radiance
  room   room d1 d2 d3 d6                           9.19e-7 3.78e-6 2.34e-5 2.21e-5 3.99e-5  7.87e-5 1.10e-4 1.10e-4 4.68e-5 7.20e-5  3.02e-6
  flat   lights3 clamp_b1 sphere_in_list edge_on    7.63e-7 1.21e-6 9.91e-7                  1.61e-6 7.26e-7 2.63e-7                  1.87e-5
         mirror_chain glass_chain checker_light
  env    env_gate (6) phantom (2) env_is_area       7.27e-7 4.92e-7                          2.39e-7 5.44e-8                          1.40e-6
         depth_cut d2 d3
  fog    fog_shadow                                 7.45e-7 1.32e-6                          2.71e-7 2.40e-7                          7.26e-7
  chain  xform_cases: wrap_each (less scale_1000)   1.44e-5 1.72e-5                          1.38e-4 1.03e-5                          5.38e-5
         wrap_pairs wrap_long wrap_mats wrap_moving   bounce 0's t: 3.95e-6 (up to six fp32 maps before the primitive's test)
         wrap_light
  stretch wrap_each scale_1000                      4.40e-3 2.46e-4                          1.74e-4 9.92e-5                          5.14e-4
                                                      bounce 0's t: 2.39e-5 (object space reaches 32; the ball's normal is
                                                      (P - c) / 0.22 there, times 8 on the way out)
  tree   wrap_inner (3) rot_bvh (2)                 8.58e-7                                  6.08e-6                                  3.07e-7
  stack  stack_cases: chain_ref chain_dfs inst_leaf    9.46e-7 2.82e-6                          1.93e-5 1.94e-6                          4.43e-6
         balanced                                     (bounce 1's t: `balanced`, a floor ray that meets a tile after t ~ 0.1)
  A wrapped sphere's feature normal, unit(A^T (P - c) / r) in float32 from the fp32 oracle's t: chain 1.43e-5, stretch 4.40e-3.

The room's relative t error is that large because a scattered ray that
starts near a corner hits the next wall after t ~ 0.01, where an absolute
error of 1e-6 is 1e-4 of t.  The host pipeline measures 2.95e-6 (room),
1.94e-5 (flat: clamp_b1, whose sums reach 32), 1.40e-6 (env) and 7.38e-7 (fog)
on the radiance.  The NEE contributions and shadow-ray ends are not visible
one by one through the oracle's recorder or the pipeline.  They are held
through the radiance, and one bounce at a time through the production
shade_path (`hits_emu_shade`) on the reference's own incoming ray of every
bounce, where no error carries over and the one-bounce bars of
test_shade_kat.test_host_area_light_nee hold: directions atol 1e-5, the end
rtol 2e-6, contributions rtol 2e-5 + atol 1e-6, the HDRI contribution the
shading rows' measured `nee` bar.  Measured: directions 5.6e-7, ends 1.04e-6
(room, bounces 0 to 5), HDRI contribution 1.19e-6 (bar 2.1e-6)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import path_cases as PC
from tests.test_shade_kat import BAR as SHADE_BAR
from tests.test_shade_kat import emu_shade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")

RAY_ATOL, T_RTOL = 1e-5, 2e-6              # bounce 0: the project's bars
FP64, FP64_ZERO = 1e-12, 1e-15
# the fp32 oracle against path_ref on the CPU: index 0 is bounce 1
MEASURED_FP32 = {
    "room": dict(ray=[9.19e-7, 3.78e-6, 2.34e-5, 2.21e-5, 3.99e-5], t=[7.87e-5, 1.10e-4, 1.10e-4, 4.68e-5, 7.20e-5], L=3.02e-6),
    "flat": dict(ray=[7.63e-7, 1.21e-6, 9.91e-7], t=[1.61e-6, 7.26e-7, 2.63e-7], L=1.87e-5),
    "env": dict(ray=[7.27e-7, 4.92e-7], t=[2.39e-7, 5.44e-8], L=1.40e-6),
    "fog": dict(ray=[7.45e-7, 1.32e-6], t=[2.71e-7, 2.40e-7], L=7.26e-7),
    # tests/xform_cases.py (tests/test_xform_kat.py); t0: bounce 0's t, where the oracle itself leaves more than T_RTOL;
    # n_ball: a wrapped sphere's feature normal unit(A^T (P - c) / r) in float32 from the fp32 oracle's t
    "chain": dict(ray=[1.44e-5, 1.72e-5], t=[1.38e-4, 1.03e-5], L=5.38e-5, t0=3.95e-6, n_ball=1.43e-5),
    "stretch": dict(ray=[4.40e-3, 2.46e-4], t=[1.74e-4, 9.92e-5], L=5.14e-4, t0=2.39e-5, n_ball=4.40e-3),
    "tree": dict(ray=[8.58e-7], t=[6.08e-6], L=3.07e-7),
    # tests/stack_cases.py (tests/test_stack_host.py)
    "stack": dict(ray=[9.46e-7, 2.82e-6], t=[1.93e-5, 1.94e-6], L=4.43e-6),
}

f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def record_bars(group, bounce, who):
    """(ray atol, t rtol) of bounce `bounce` for `who`: "fp64", "fp32" (the
    fp32 oracle: the measured figure x 1.05) or "device" (4 x the figure)."""
    if who == "fp64":
        return FP64, FP64                  # rays: 1e-12 absolute, as test_shade_kat passes FP64 for its rays' atol
    m = MEASURED_FP32[group]
    k = 1.05 if who == "fp32" else 4.0
    if bounce == 0:                        # t0: a group whose fp32 oracle itself leaves more than T_RTOL on a wrapped hit's t
        return RAY_ATOL, (k * m["t0"] if "t0" in m else T_RTOL)
    return k * m["ray"][bounce - 1], k * m["t"][bounce - 1]


def radiance_bar(group, who):
    """(atol, rtol) of a row's radiance."""
    if who == "fp64":
        return FP64_ZERO, FP64
    return (1.05 if who == "fp32" else 4.0) * MEASURED_FP32[group]["L"], 0.0


def check_radiance(what, case, e, L, who):
    atol, rtol = radiance_bar(case.group, who)
    err = PC.radiance_error(e, L)
    print(f"{what}: radiance worst |err| {err:.3g} (bar {atol:.3g})")
    over = PC.radiance_error(e, L, rtol)
    assert over <= atol, f"{what}: radiance off by {err} (past rtol {rtol} by {over}, atol {atol})"


def check_records(what, case, e, ids, s, b, top, t, ray, nee, who, bits="nee"):
    ray_err, t_err = PC.record_errors(e, ids, s, b, top, t, ray, nee, what, bits=bits)
    ray_bar, t_bar = record_bars(case.group, b, who)
    print(f"{what} s{s} b{b}: ray |err| {ray_err:.3g} (bar {ray_bar:.3g}) t rel {t_err:.3g} (bar {t_bar:.3g})")
    assert ray_err <= ray_bar, f"{what} s{s} b{b}: ray off by {ray_err} (bar {ray_bar})"
    assert t_err <= t_bar, f"{what} s{s} b{b}: t off by {t_err} relative (bar {t_bar})"


# ---- the rows, on path_ref alone --------------------------------------------
def test_reference_rows_are_what_they_claim(g):
    """Every row's counts (the events it is there for happen) and at most 2 %
    of its pixel-samples left out, on path_ref alone: no oracle, no device."""
    for name, v in PC.ROWS:
        c = PC.CASES[name]
        e = c.expected(g, v)
        print(c.summary(g, v))
        assert e["left_out"] <= PC.LEFT_OUT_CAP * PC.N * e["samples"], (name, v)
    for v in ("env", "sky", "bg"):          # the environment is not gated on allow: with and without a light
        assert PC.CASES["env_gate"].expected(g, v + "+light")["counts"]["b1_miss_not_allowed"] > 0
        assert PC.CASES["env_gate"].expected(g, v)["counts"]["b1_miss_allowed"] > 0


def test_reference_recursion_is_the_sum_over_bounces(g):
    """Le + direct + att * indirect, unrolled: a path's radiance is the sum
    over its bounces of beta_b (Le_b + direct_b) with beta_{b+1} = beta_b
    att_b and the clamp inside direct_b, before beta_b; and `room` at depth k
    is that sum cut after bounce k - 1, so L(depth k) - L(depth k - 1) is
    bounce k - 1's term alone, its NEE included."""
    room = PC.CASES["room"]
    deep = room.expected(g, "d6")
    for v in ("d1", "d2", "d3", "d6"):
        e = room.expected(g, v)
        for p, (pa, pd) in enumerate(zip(e["paths"][0], deep["paths"][0])):
            beta, total = np.ones(3), np.zeros(3)
            for b in pd.bounces[:e["depth"]]:
                total = total + beta * (b["Le"] + (b["nee"]["direct"] if b["nee"] else 0.0))
                if b["att"] is not None:
                    beta = beta * b["att"]
            np.testing.assert_allclose(pa.L, total, rtol=1e-13, atol=1e-15, err_msg=f"room[{v}] pixel {p}")
    last = deep["L"] - room.expected(g, "d3")["L"]
    assert (last >= -1e-15).all() and (last > 0).sum() > 300          # bounces 3 to 5 add light almost everywhere


# ---- the oracle, both modes -------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,variant", PC.ROWS, ids=[f"{n}-{v}" if v else n for n, v in PC.ROWS])
def test_oracle_path_integral(g, O, name, variant, fp32):
    c = PC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    who = "fp32" if fp32 else "fp64"
    b, d, cam, ids = c.build(g, variant)
    what = f"{name}[{variant}] {who} oracle"
    if c.records(variant):
        for s in range(e["samples"]):
            top, _, t, ray, nee = O.path_records(d, cam, PC.SEED, s, e["depth"], fp32=fp32, threads=2)
            for k in range(e["depth"]):
                # nee_dev: the oracle's recorder, like the device, applies the cosLight cut before the shadow test
                check_records(what, c, e, ids, s, k, top[k], t[k], ray[k], nee[k], who, bits="nee_dev")
    L = O.render(d, cam, g.make_params(e["samples"], e["depth"], seed=PC.SEED), fp32=fp32, threads=2)
    check_radiance(what, c, e, L, who)


# ---- the production wavefront pipeline on the host ------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/hits_emu.cpp as a plain shared library (no sanitizer)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    t = tmp_path_factory.mktemp("path_emu")
    so = t / "libhits_emu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "hits_emu.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(so)],
                   check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.hits_emu_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, f32p, C.c_int]
    lib.hits_emu_shade.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, i32p,
                                   f32p, f32p, f32p, C.c_int, f32p, i32p, f32p, i32p, f32p, f32p, f32p, f32p, u32p, f32p,
                                   f32p, f32p, f32p, f32p]
    return lib


def _vp(x):
    return C.cast(C.pointer(x), C.c_void_p)


def emu_render(lib, d, cam, spp, depth, fmt=0, in_bvh=0, sample_offset=0):
    out = np.zeros((cam.image_width * cam.image_height, 3), np.float32)
    rc = lib.hits_emu_render(_vp(d), _vp(cam), fmt, PC.SEED, sample_offset, spp, depth, out.ctypes.data_as(f32p), in_bvh)
    assert rc == 0, f"hits_emu_render {rc}"
    return out


HOST_RUNS = ([(n, v, "fp32nodes") for n, v in PC.ROWS] + [(n, v, "quant8") for n, v in PC.ROWS if PC.CASES[n].quant8]
             + [("fog_shadow", "", "in_bvh")] + [(n, v, "tail") for n, v in PC.TAIL_ROWS])


@pytest.mark.parametrize("name,variant,mode", HOST_RUNS, ids=["-".join(x for x in r if x) for r in HOST_RUNS])
def test_host_pipeline_path_integral(g, emu, monkeypatch, name, variant, mode):
    c = PC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    b, d, cam, ids = c.build(g, variant)
    if mode == "tail":                      # wave_run.h: k_tail carries every path on after bounce 0
        monkeypatch.setenv("RTG_EMU_TAIL", "0")
    L = emu_render(emu, d, cam, e["samples"], e["depth"], fmt=1 if mode == "quant8" else 0, in_bvh=1 if mode == "in_bvh" else 0)
    check_radiance(f"{name}[{variant}] host pipeline {mode}", c, e, L, "device")


def test_host_pipeline_sample_offset(g, emu):
    """The row's samples one by one through sample_offset add up to the row's frame."""
    c = PC.CASES["sphere_in_list"]
    e = c.expected(g, "")
    b, d, cam, ids = c.build(g, "")
    L = sum(emu_render(emu, d, cam, 1, e["depth"], sample_offset=s).astype(np.float64) for s in range(e["samples"]))
    check_radiance("sphere_in_list by sample_offset", c, e, L, "device")


# ---- the NEE record of every bounce, one bounce at a time -------------------------
NEE_ROWS = [("room", "d6"), ("lights3", ""), ("clamp_b1", ""), ("sphere_in_list", ""), ("checker_light", ""), ("env_is_area", ""),
            ("edge_on", "")]
CA_RTOL, CA_ATOL = 2e-5, 1e-6               # test_shade_kat.test_host_area_light_nee's bars for a contribution


@pytest.mark.parametrize("name,variant", NEE_ROWS, ids=[f"{n}-{v}" if v else n for n, v in NEE_ROWS])
def test_host_shade_path_nee_records(g, emu, name, variant):
    """What the radiance cannot show one by one: at every bounce of every
    decided path the production shade_path (hits_emu_shade) is given the
    reference's own incoming ray, rounded to fp32, so that no error carries
    over from the bounces before and one bounce's bars hold at every bounce:
    the shadow rays wanted (exact, less those cosLight < 0.001 cuts, which
    the device drops before it queues them; which light was chosen shows in the
    direction, the lights being a unit or more apart), the area ray's
    direction (atol 1e-5), its end dist - 0.001 (rtol 2e-6) and, where the
    reference finds the ray visible, its contribution, clamped and with the
    local attenuation but without the upstream beta (rtol 2e-5, atol 1e-6:
    test_host_area_light_nee's bars); the HDRI ray's direction and
    contribution (test_shade_kat's measured `nee` bar)."""
    c = PC.CASES[name]
    e = c.expected(g, variant)
    b_, d, cam, ids = c.build(g, variant)
    worst = dict(da=0.0, end=0.0, ca=0.0, dh=0.0, ch=0.0)
    compared = 0
    for s in range(e["samples"]):
        for k in range(e["depth"]):
            for allow in (0, 1):
                sel = [p for p, pa in enumerate(e["paths"][s]) if e["nee_ok"][s][k][p] and k < len(pa.bounces)
                       and pa.bounces[k]["nee"] and int(pa.bounces[k]["allow"]) == allow]
                if not sel:
                    continue
                bn = [e["paths"][s][p].bounces[k] for p in sel]
                r = emu_shade(emu, d, cam, k, e["depth"] - k, np.array(sel), np.array([x["o"] for x in bn]),
                              np.array([x["d"] for x in bn]), fmt=0, allow=allow, sample=s)
                area = [x["nee"]["area"] for x in bn]
                want = np.array([a["wanted"] and not a["cut"] for a in area])      # the device cuts before it queues the ray
                assert np.array_equal((r["flags"] & 1) != 0, want), f"{name} s{s} b{k}: area shadow rays wanted"
                vis = np.array([a["visible"] and not a["cut"] for a in area])
                if want.any():
                    worst["da"] = max(worst["da"], np.abs(r["da"][want] - np.array([a["dir"] for a in area])[want]).max())
                    end = np.array([a["end"] for a in area])[want]
                    worst["end"] = max(worst["end"], (np.abs(r["tmax_a"][want] - end) / end).max())
                if vis.any():
                    con = np.array([a["con"] for a in area])[vis]
                    worst["ca"] = max(worst["ca"], (np.abs(r["ca"][vis] - con) - CA_RTOL * np.abs(con)).max())
                if bn[0]["nee"]["hdri"] is not None:
                    hd = [x["nee"]["hdri"] for x in bn]
                    hw = np.array([h["wanted"] for h in hd])
                    assert np.array_equal((r["flags"] & 2) != 0, hw), f"{name} s{s} b{k}: HDRI shadow rays wanted"
                    hv = np.array([h["visible"] for h in hd])
                    if hw.any():
                        worst["dh"] = max(worst["dh"], np.abs(r["dh"][hw] - np.array([h["dir"] for h in hd])[hw]).max())
                    if hv.any():
                        worst["ch"] = max(worst["ch"], np.abs(r["ch"][hv] - np.array([h["con"] for h in hd])[hv]).max())
                compared += len(sel)
    print(f"{name}[{variant}] host shade_path NEE records: {compared} compared, worst {worst}")
    assert compared > 300
    assert worst["da"] <= RAY_ATOL and worst["dh"] <= RAY_ATOL, worst
    assert worst["end"] <= T_RTOL, worst
    assert worst["ca"] <= CA_ATOL, worst
    assert worst["ch"] <= SHADE_BAR["nee"], worst
