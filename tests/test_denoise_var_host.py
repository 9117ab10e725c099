"""The variance-guided denoiser's kernels on the host (no GPU):
tests/denoise_var_emu.cpp compiles go-raytracing_amd/csrc/denoise_var.hip
through tests/host_emu and runs every block of every kernel with one lane per
block under AddressSanitizer + UBSan, as a child process.  Compared with the
numpy restatement in tests/denoise_var_ref.py (same operation order), and
checked for the exact properties include/rtgpu.h states."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import denoise_ref as R0
from tests import denoise_var_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    t = tmp_path_factory.mktemp("denoise_var_emu")
    exe = t / "denoise_var_emu"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "denoise_var_emu.cpp"),
                    "-o", str(exe)], check=True, cwd=t)
    return str(exe)


def run_emu(emu, tmp, accum, feat, moments, spp, grid=0, **params):
    p = dict(R.DEFAULTS, **params)
    h, w = accum.shape[:2]
    fin, ffeat, fmom, fout, fvar = (tmp / n for n in ("in.f32", "feat.f32", "mom.f32", "out.f32", "var.f32"))
    accum.astype(np.float32).tofile(fin)
    feat.astype(np.float32).tofile(ffeat)
    if moments is not None:
        moments.astype(np.float32).tofile(fmom)
    args = [emu, str(w), str(h), str(spp), str(p["iterations"]), str(p["normal_power_log2"]), str(p["demodulate"]),
            str(p["spatial_below"]), repr(float(p["sigma_lum"])), repr(float(p["sigma_depth"])),
            repr(float(p["albedo_eps"])), str(fin), str(ffeat), str(fmom) if moments is not None else "-",
            str(fout), str(fvar)]
    if grid:
        args.append(str(grid))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return np.fromfile(fout, np.float32).reshape(h, w, 3), np.fromfile(fvar, np.float32).reshape(h, w)


def assert_within_bar(got, ref):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bar = R.BAR * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    worst = float((d / bar).max())
    print(f"colour: max |d| = {d.max():.3e}, worst d/bar = {worst:.3f}")
    assert worst <= 1.0, worst


def assert_var_within_bar(got, ref):
    ref64 = ref.astype(np.float64)
    d = np.abs(got.astype(np.float64) - ref64)
    bar = R.BAR * np.maximum(np.abs(ref64), 1e-3 * ref64.max())
    worst = float((d / bar).max())
    print(f"variance: max |d| = {d.max():.3e}, worst d/bar = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("w,h,grid,spp,params", [
    (40, 24, 0, 4, {}),                                   # step 16 leaves the image on every side; clipped windows
    (131, 67, 1000, 4, {}),                               # odd, no multiple of any tile; grid-stride loops
    (40, 24, 0, 4, dict(iterations=1)),                   # the pass that is both first and last
    (131, 67, 0, 4, dict(demodulate=0, iterations=3)),
    (40, 24, 0, 1, {}),                                   # 1 spp, no moments: the spatial estimate
    (131, 67, 777, 1, dict(iterations=3)),
    (40, 24, 0, 4, dict(spatial_below=5)),                # 4 spp below the threshold: spatial with moments given
])
def test_emulated_kernels_match_reference(emu, tmp_path, w, h, grid, spp, params):
    accum, feat = R.synthetic(w, h, spp=spp, seed=w)
    spatial = spp < dict(R.DEFAULTS, **params)["spatial_below"]
    moments = R.synthetic_moments(accum, spp, seed=h) if spp > 1 else None
    got, var = run_emu(emu, tmp_path, accum, feat, moments, spp, grid=grid, **params)
    ref, rvar = R.denoise_var_ref(accum, feat, moments, spp, **params)
    assert np.isfinite(got).all() and np.isfinite(var).all()
    assert not np.array_equal(got, accum)
    assert (rvar > 0).mean() > 0.5 and (var >= 0).all()
    if spatial and moments is not None:   # the moments are not read in the spatial case
        ref2, rvar2 = R.denoise_var_ref(accum, feat, None, spp, **params)
        assert np.array_equal(ref, ref2) and np.array_equal(rvar, rvar2)
    assert_within_bar(got, ref)
    assert_var_within_bar(var, rvar)


@pytest.mark.parametrize("spp", [1, 4])
def test_zero_iterations_copy_the_input(emu, tmp_path, spp):
    accum, feat = R.synthetic(40, 24, spp=spp, seed=3)
    moments = R.synthetic_moments(accum, spp, seed=4) if spp > 1 else None
    got, var = run_emu(emu, tmp_path, accum, feat, moments, spp, iterations=0)
    assert np.array_equal(got.view(np.uint32), accum.view(np.uint32))
    _, rvar = R.denoise_var_ref(accum, feat, moments, spp, iterations=0)   # out_var: the initial variance
    assert_var_within_bar(var, rvar)


@pytest.mark.parametrize("branch", ["spatial", "moments"])
def test_uncovered_pixels_pass_through_bit_for_bit(emu, tmp_path, branch):
    accum, feat = R.synthetic(131, 67, spp=4, seed=5)
    moments = R.synthetic_moments(accum, 4, seed=6)
    params = dict(spatial_below=5) if branch == "spatial" else {}   # the same 4-spp frame through both branches
    got, var = run_emu(emu, tmp_path, accum, feat, moments, 4, **params)
    through = feat[..., 7] / np.float32(4) < 0.5
    assert 50 < through.sum() < through.size // 2
    assert np.array_equal(got[through].view(np.uint32), accum[through].view(np.uint32))
    assert not np.array_equal(got[~through], accum[~through])
    assert (var[through] == 0).all() and (var[~through] > 0).any()
    # ... and are never neighbours: their radiance and moments do not reach the others
    a2, m2 = accum.copy(), moments.copy()
    a2[through] *= np.float32(7.0)
    m2[through] *= np.float32(5.0)
    got2, var2 = run_emu(emu, tmp_path, a2, feat, m2, 4, **params)
    assert np.array_equal(got2[~through].view(np.uint32), got[~through].view(np.uint32))
    assert np.array_equal(var2.view(np.uint32), var.view(np.uint32))


@pytest.mark.parametrize("spp", [1, 2, 4])
def test_orthogonal_normals_stop_colour_and_variance_exactly(emu, tmp_path, spp):
    """Left half normals +x, right half +y: w_n is exactly 0 across the edge,
    so neither the right half's colours nor its variance can reach the left
    half's output (2 spp: spatial estimate, 4 spp: moments)."""
    a1, feat = R.two_regions(40, 24, spp=spp, right_scale=1.0)
    a2, _ = R.two_regions(40, 24, spp=spp, right_scale=3.0)
    assert np.array_equal(a1[:, :20], a2[:, :20]) and not np.array_equal(a1[:, 20:], a2[:, 20:])
    m1 = R.synthetic_moments(a1, spp, seed=8) if spp > 1 else None
    m2 = R.synthetic_moments(a2, spp, seed=8) if spp > 1 else None
    if spp > 1:
        assert np.array_equal(m1[:, :20], m2[:, :20]) and not np.array_equal(m1[:, 20:], m2[:, 20:])
    o1, v1 = run_emu(emu, tmp_path, a1, feat, m1, spp)
    o2, v2 = run_emu(emu, tmp_path, a2, feat, m2, spp)
    assert np.array_equal(o1[:, :20].view(np.uint32), o2[:, :20].view(np.uint32))
    assert np.array_equal(v1[:, :20].view(np.uint32), v2[:, :20].view(np.uint32))
    assert not np.array_equal(o1[:, 20:], o2[:, 20:]) and not np.array_equal(v1[:, 20:], v2[:, 20:])
    assert not np.array_equal(o1[:, :20], a1[:, :20])   # the left half was filtered


def test_two_runs_give_equal_bits(emu, tmp_path):
    accum, feat = R.synthetic(40, 24, spp=4, seed=9)
    moments = R.synthetic_moments(accum, 4, seed=10)
    o1, v1 = run_emu(emu, tmp_path, accum, feat, moments, 4)
    o2, v2 = run_emu(emu, tmp_path, accum, feat, moments, 4, grid=97)
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32))
    assert np.array_equal(v1.view(np.uint32), v2.view(np.uint32))


def test_firefly_is_pulled_to_its_neighbours(emu, tmp_path):
    """rt_denoise centres its colour weight on the pixel's own value and
    leaves a firefly as it is; the variance-guided weight of a pixel whose
    samples disagree accepts the neighbours."""
    accum, feat, moments, (fy, fx) = R.firefly(40, 24)
    plain = R0.denoise_ref(accum, feat, 4)
    ref, rvar = R.denoise_var_ref(accum, feat, moments, 4)
    got, var = run_emu(emu, tmp_path, accum, feat, moments, 4)
    assert accum[fy, fx, 1] > 100 * np.median(accum[..., 1])
    for out, v in ((ref, rvar), (got, var)):
        assert (out[fy, fx] < plain[fy, fx]).all(), (out[fy, fx], plain[fy, fx])
        assert v[fy, fx] > np.median(v)
    assert_within_bar(got, ref)
    assert_var_within_bar(var, rvar)
