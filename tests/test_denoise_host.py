"""The denoiser's kernels on the host (no GPU): tests/denoise_emu.cpp compiles
go-raytracing_amd/csrc/denoise.hip through tests/host_emu and runs every
block of every pass with one lane per block under AddressSanitizer + UBSan,
as a child process.  Compared with the numpy restatement of the filter in
tests/denoise_ref.py (same tap order), and checked for the exact properties
include/rtgpu.h states."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    t = tmp_path_factory.mktemp("denoise_emu")
    exe = t / "denoise_emu"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "denoise_emu.cpp"),
                    "-o", str(exe)], check=True, cwd=t)
    return str(exe)


def run_emu(emu, tmp, accum, feat, spp, grid=0, **params):
    p = dict(R.DEFAULTS, **params)
    h, w = accum.shape[:2]
    fin, ffeat, fout = tmp / "in.f32", tmp / "feat.f32", tmp / "out.f32"
    accum.astype(np.float32).tofile(fin)
    feat.astype(np.float32).tofile(ffeat)
    args = [emu, str(w), str(h), str(spp), str(p["iterations"]), str(p["normal_power_log2"]), str(p["demodulate"]),
            repr(float(p["sigma_color"])), repr(float(p["sigma_depth"])), repr(float(p["albedo_eps"])),
            str(fin), str(ffeat), str(fout)]
    if grid:
        args.append(str(grid))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return np.fromfile(fout, np.float32).reshape(h, w, 3)


def assert_within_bar(got, ref):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bar = R.BAR * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    worst = float((d / bar).max())
    print(f"max |d| = {d.max():.3e}, worst d/bar = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("w,h,grid,params", [
    (40, 24, 0, {}),                                   # step 16 reaches past the image on every side
    (131, 67, 1000, {}),                               # odd, no multiple of any tile; grid-stride loop
    (131, 67, 0, dict(demodulate=0, iterations=3)),
    (40, 24, 0, dict(iterations=1)),                   # the pass that is both first and last
])
def test_emulated_kernel_matches_reference(emu, tmp_path, w, h, grid, params):
    accum, feat = R.synthetic(w, h, spp=4, seed=w)
    got = run_emu(emu, tmp_path, accum, feat, 4, grid=grid, **params)
    ref = R.denoise_ref(accum, feat, 4, **params)
    assert np.isfinite(got).all()
    assert not np.array_equal(got, accum)
    assert_within_bar(got, ref)


def test_zero_iterations_copy_the_input(emu, tmp_path):
    accum, feat = R.synthetic(40, 24, spp=4, seed=3)
    got = run_emu(emu, tmp_path, accum, feat, 4, iterations=0)
    assert np.array_equal(got.view(np.uint32), accum.view(np.uint32))


def test_uncovered_pixels_pass_through_bit_for_bit(emu, tmp_path):
    accum, feat = R.synthetic(131, 67, spp=4, seed=5)
    got = run_emu(emu, tmp_path, accum, feat, 4)
    through = feat[..., 7] / np.float32(4) < 0.5
    assert 50 < through.sum() < through.size // 2
    assert np.array_equal(got[through].view(np.uint32), accum[through].view(np.uint32))
    assert not np.array_equal(got[~through], accum[~through])


def test_orthogonal_normals_stop_the_filter_exactly(emu, tmp_path):
    """Left half normals +x, right half +y: w_n is exactly 0 across the edge,
    so the right half's colours cannot reach the left half's output."""
    a1, feat = R.two_regions(40, 24, right_scale=1.0)
    a2, _ = R.two_regions(40, 24, right_scale=3.0)
    assert np.array_equal(a1[:, :20], a2[:, :20]) and not np.array_equal(a1[:, 20:], a2[:, 20:])
    o1 = run_emu(emu, tmp_path, a1, feat, 2)
    o2 = run_emu(emu, tmp_path, a2, feat, 2)
    assert np.array_equal(o1[:, :20].view(np.uint32), o2[:, :20].view(np.uint32))
    assert not np.array_equal(o1[:, 20:], o2[:, 20:])
    assert not np.array_equal(o1[:, :20], a1[:, :20])   # the left half was filtered
