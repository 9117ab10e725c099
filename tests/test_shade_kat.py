"""Shading against closed forms, on the CPU: the rows of tests/shade_cases.py
(scattering, textures, environment, lens), whose expected values come from
tests/shade_ref.py, a float64 restatement of the Go text alone, held against

  * the oracle in both modes (`O.path_records` for the rays, `O.render` for
    the radiance), and
  * the production `shade_path` compiled for the host (tests/hits_emu.cpp
    `hits_emu_shade`: k_extend's one-lane closest hit, then shade_path in the
    variant the launcher picks, a plain ctypes library), which is also the
    only place the NEE directions and contributions are visible: `dh`, `ch`
    for the HDRI rows and `da`, `ca`, `tmax_a` for kat_cases.area_light_scene.

Every row prints the pixels compared, the pixels left out and its branch
counts (pytest -s).

Tolerances.  Ray origins and directions atol 1e-5, t rtol 2e-6 (the bars of
tests/test_gpu_kat.py for coordinates of this size); branch choices, ended
paths and image texels exact; the fp64 oracle 1e-12 relative (1e-15 where
the expected value is 0).  Noise values, environment lookups and HDRI NEE
contributions go through sinf / atan2f / asinf / cosf and a 7-octave fp32
sum, so their bar is the fp32 oracle's
measured worst absolute error against shade_ref on the CPU, times 4 (ocml's
and glibc's transcendentals differ in the last ulps) for the
host shade_path and the GPU; the fp32 oracle itself is held to the figure
(x 1.05 for the figure's rounding), so the table stays true:

  group   rows                              fp32 oracle, worst |err|   bar (x 4)
  noise   noise_emit, noise_albedo          2.97e-5                    1.2e-4
  env     env_px / nx / py / rot / f32      2.94e-6 (env_py)           1.2e-5
  nee     env_is, env_is_rot                5.15e-7 (env_is_rot)       2.1e-6

The host shade_path measures 2.97e-5 / 2.93e-6 / 5.15e-7 on the same rows,
the GPU 2.97e-5 / 2.22e-6 / 5.15e-7 (tests/test_gpu_shade_kat.py).  `iso`'s
radiance is the albedo rounded to fp32 once (2^-23 absolute, values < 1).

Two rows sit on an exact tie, where `>` against `>=` (material.go:180) and
`<=` against `<` (hdri.go:306) differ: `glass_tie` (reflectance and draw both
0.25) and `cdf_tie` (xi2 and the CDF entry of a black texel both 0).  Both
numbers are exact in fp32 and fp64, so the tie is decided, not left out; the
(pixel, sample) that draws it was found by a search over samples and is
asserted on the reference."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import kat_cases as K
from tests import shade_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")

MEASURED_FP32 = dict(noise=2.97e-5, env=2.94e-6, nee=5.15e-7)      # the fp32 oracle against shade_ref, CPU
BAR = {k: 4.0 * v for k, v in MEASURED_FP32.items()}
RAY_ATOL, T_RTOL = 1e-5, 2e-6
FP64 = 1e-12
FP64_ZERO = 1e-15

f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
NAMES = list(S.CASES)


def radiance_tol(e, who):
    """(atol, rtol) of a row's radiance for `who`: "fp64" (the fp64 oracle:
    1e-12 relative, 1e-15 for the pixels whose expected value is 0), "fp32"
    (the fp32 oracle: a measured group's figure itself, with 5 % for the
    figure's own rounding) or "device" (the host shade_path and the GPU: 4 x
    that figure)."""
    if who == "fp64":
        return FP64_ZERO, FP64
    m = MEASURED_FP32.get(e.get("group"), 0.0)
    return {"exact": 0.0, "rounded": 2.0 ** -23, "measured": 1.05 * m if who == "fp32" else 4.0 * m}[e["L_kind"]], 0.0


def check_radiance(what, e, variant, L, who):
    atol, rtol = radiance_tol(e, who)
    err = S.radiance_error(e, variant, L)
    print(f"{what}: worst |err| {err:.3g}")
    over = S.radiance_error(e, variant, L, rtol)
    assert over <= atol, f"{what}: radiance off by {err} (past rtol {rtol} by {over}, atol {atol})"


def has_paths(e):
    return any(k in e for k in ("t0", "ray0", "ray1", "ended1"))


def test_reference_rows_are_what_they_claim(g):
    """Every row's own assertions (branch counts, texels reached, seam and
    pole pixels, rejected disk tries, at most 2 % left out), on shade_ref alone."""
    for c in S.CASES.values():
        print(c.summary(g))
    e = S.CASES["glass_back"].expected(g)
    assert e["counts"] == dict(tir=145, reflect=7, refract=232)
    assert S.CASES["metal_f1"].expected(g)["counts"]["absorbed"] == 48
    for name in ("glass_front", "glass_back", "metal_f0", "metal_f03", "metal_f1", "image_quad", "defocus"):
        assert S.CASES[name].expected(g)["left_out"] == 0, name


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_shading_closed_form(g, O, name, fp32):
    c = S.CASES[name]
    e = c.expected(g)
    print(c.summary(g))
    if has_paths(e):
        b, d, cam = c.build(g, c.variants[0])
        top, _, t, ray, _ = O.path_records(d, cam, S.SEED, c.sample, 2, fp32=fp32, threads=2)
        S.check_paths(c, e, (top[0], t[0], ray[0]), (top[1], ray[1]), RAY_ATOL if fp32 else FP64, T_RTOL if fp32 else FP64)
    if "L" in e:
        for v in c.variants:
            b, d, cam = c.build(g, v)
            L = O.render(d, cam, g.make_params(1, e["L_depth"][v], seed=S.SEED, sample_offset=c.sample), fp32=fp32, threads=2)
            check_radiance(f"{name}[{v}] {'fp32' if fp32 else 'fp64'} oracle", e, v, L, "fp32" if fp32 else "fp64")


# ---- the production shade_path on the host ---------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/hits_emu.cpp as a plain shared library (no sanitizer)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    t = tmp_path_factory.mktemp("shade_emu")
    so = t / "libhits_emu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "hits_emu.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(so)],
                   check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.hits_emu_env_format.argtypes = [C.c_void_p, C.c_void_p]
    lib.hits_emu_shade.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, i32p,
                                   f32p, f32p, f32p, C.c_int, f32p, i32p, f32p, i32p, f32p, f32p, f32p, f32p, u32p, f32p,
                                   f32p, f32p, f32p, f32p]
    return lib


def _vp(x):
    return C.cast(C.pointer(x), C.c_void_p)


def emu_shade(lib, d, cam, bounce, dleft, pix, o=None, dr=None, beta=None, fmt=0, allow=1, sample=S.SAMPLE):
    """One bounce of the paths `pix` through hits_emu_shade: a dict of its outputs."""
    n = len(pix)
    pix = np.ascontiguousarray(pix, np.int32)
    beta = np.ones((n, 3), np.float32) if beta is None else np.ascontiguousarray(beta, np.float32)
    f3 = lambda: np.zeros((n, 3), np.float32)    # noqa: E731
    r = dict(ray=np.zeros((n, 6), np.float32), hit=np.zeros(n, np.int32), t=np.zeros(n, np.float32),
             cont=np.zeros(n, np.int32), P=f3(), sd=f3(), nbeta=f3(), Ladd=f3(), flags=np.zeros(n, np.uint32), ca=f3(),
             da=f3(), tmax_a=np.zeros(n, np.float32), ch=f3(), dh=f3())
    if o is not None:
        o, dr = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(dr, np.float32)
    p = lambda a, ty=f32p: a.ctypes.data_as(ty) if a is not None else None    # noqa: E731
    rc = lib.hits_emu_shade(_vp(d), _vp(cam), fmt, S.SEED, sample, bounce, dleft, allow, p(pix, i32p), p(o), p(dr),
                            p(beta), n, p(r["ray"]), p(r["hit"], i32p), p(r["t"]), p(r["cont"], i32p), p(r["P"]),
                            p(r["sd"]), p(r["nbeta"]), p(r["Ladd"]), p(r["flags"], u32p), p(r["ca"]), p(r["da"]),
                            p(r["tmax_a"]), p(r["ch"]), p(r["dh"]))
    assert rc == 0, f"hits_emu_shade {rc}"
    return r


def emu_radiance(lib, d, cam, depth, fmt=0, sample=S.SAMPLE):
    """The frame's radiance as the pipeline adds it up, bounce by bounce: beta
    times the miss colour or emission of bounces 0 and 1, plus the NEE
    contributions of bounce 0 (nothing in these scenes occludes a shadow ray)."""
    n = cam.image_width * cam.image_height
    r0 = emu_shade(lib, d, cam, 0, depth, np.arange(n), fmt=fmt, sample=sample)
    L = r0["Ladd"].astype(np.float64)
    L += np.where((r0["flags"] & 1)[:, None] != 0, r0["ca"], 0) + np.where((r0["flags"] & 2)[:, None] != 0, r0["ch"], 0)
    go = np.flatnonzero(r0["cont"])
    if depth > 1 and len(go):
        r1 = emu_shade(lib, d, cam, 1, depth - 1, go, r0["P"][go], r0["sd"][go], r0["nbeta"][go], fmt=fmt, sample=sample)
        assert not r1["flags"].any()
        L[go] += r1["Ladd"]
    return L, r0


HOST_RUNS = [(n, 0) for n in NAMES] + [(n, 1) for n in NAMES if S.CASES[n].quant8]


@pytest.mark.parametrize("name,fmt", HOST_RUNS, ids=[f"{n}-{'quant8' if f else 'fp32nodes'}" for n, f in HOST_RUNS])
def test_host_shade_path_closed_form(g, emu, name, fmt):
    c = S.CASES[name]
    e = c.expected(g)
    print(c.summary(g))
    if has_paths(e):
        b, d, cam = c.build(g, c.variants[0])
        n = cam.image_width * cam.image_height
        r0 = emu_shade(emu, d, cam, 0, cam.max_depth, np.arange(n), fmt=fmt, sample=c.sample)
        top0 = np.where(r0["hit"] != 0, 0, -1)
        top1 = np.where(r0["cont"] != 0, 0, -2)
        S.check_paths(c, e, (top0, r0["t"], r0["ray"]), (top1, np.concatenate([r0["P"], r0["sd"]], axis=1)),
                      RAY_ATOL, T_RTOL)
    if "L" in e:
        for v in c.variants:
            b, d, cam = c.build(g, v)
            L, r0 = emu_radiance(emu, d, cam, e["L_depth"][v], fmt=fmt, sample=c.sample)
            check_radiance(f"{name}[{v}] host shade_path", e, v, L, "device")
            if "env_rgbe" in e:                          # the texel path the row is there for
                assert emu.hits_emu_env_format(_vp(d), _vp(cam)) == (1 if e["env_rgbe"] else 0), f"{name}: texel path"
            if "nee" in e:                               # the HDRI shadow ray itself: wanted, direction, contribution
                ok, want = e["L_ok"], e["nee"]["traced"]
                assert np.array_equal(((r0["flags"] & 2) != 0)[ok], want[ok]), f"{name}: HDRI rays wanted"
                assert not (r0["flags"] & 1).any(), f"{name}: the light under the floor has cos(theta) <= 0"
                m = ok & want
                np.testing.assert_allclose(r0["dh"][m], e["nee"]["dh"][m], rtol=0, atol=RAY_ATOL)
                assert np.abs(r0["ch"][m] - e["nee"]["ch"][m]).max() <= BAR["nee"]


def test_host_area_light_nee(g, emu):
    """sampleAreaLight's set-up (camera.go:610-678) in shade_path for
    kat_cases.area_light_scene: the shadow ray's direction da = unit(lp - P),
    its end tmax_a = dist - 0.001 (SHADOW_END leaves that alone below 1048)
    and the contribution ca of kat_cases.area_light_expected."""
    b, d, cam = K.area_light_scene(g)
    n = K.AREA_N
    r0 = emu_shade(emu, d, cam, 0, 1, np.arange(n))
    want = K.area_light_expected(spp=1)
    lp = np.zeros((n, 3))
    for pix in range(n):
        li = min(int(K.rnd(K.SEED, pix, 0, 0, K.DOM_NEE, 0) * 2), 1)
        Q, u, v = (np.array(x) for x in K.AREA_LIGHTS[li])
        lp[pix] = Q + K.rnd(K.SEED, pix, 0, 0, K.DOM_NEE, 1) * u + K.rnd(K.SEED, pix, 0, 0, K.DOM_NEE, 2) * v
    dist = np.linalg.norm(lp, axis=1)                       # P is the origin
    assert (r0["flags"] == 1).all() and (r0["hit"] == 1).all()
    np.testing.assert_allclose(r0["P"], 0.0, atol=RAY_ATOL)
    np.testing.assert_allclose(r0["da"], lp / dist[:, None], rtol=0, atol=RAY_ATOL)
    np.testing.assert_allclose(r0["tmax_a"], dist - 0.001, rtol=T_RTOL)
    np.testing.assert_allclose(r0["ca"], want, rtol=2e-5, atol=1e-6)
    assert (want[:, 0] == 20.0).any() and (want[:, 0] < 20.0).any()
