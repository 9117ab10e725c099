"""The adaptive-sampling kernels on the host (no GPU): tests/adaptive_emu.cpp
compiles go-raytracing_amd/csrc/adaptive.hip through tests/host_emu and runs
every block of every kernel with one lane per block under AddressSanitizer +
UBSan, as a child process, in the production kernel order
(ad_for_each_kernel).  The list must equal tests/adaptive_ref.py's exactly, and
k_normalize its normalize, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import adaptive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# (w, h, blocks per kernel): fewer blocks than pixels make every block walk several steps
SIZES = [(1, 1, 1), (7, 9, 5), (40, 24, 97), (131, 67, 1000)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    t = tmp_path_factory.mktemp("adaptive_emu")
    exe = t / "adaptive_emu"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "adaptive_emu.cpp"),
                    "-o", str(exe)], check=True, cwd=t)
    return str(exe)


def _run(args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return r.stdout


def emu_select(emu, tmp, mom, counts, max_spp, grid, cur=0, **params):
    p = dict(R.DEFAULTS, **params)
    h, w = counts.shape
    fm, fc, fl = tmp / "mom.f32", tmp / "counts.u32", tmp / "list.u32"
    np.ascontiguousarray(mom, F).tofile(fm)
    np.ascontiguousarray(counts, np.uint32).tofile(fc)
    out = _run([emu, "select", str(w), str(h), str(max_spp), str(cur), str(p["neighbourhood"]),
                repr(float(F(p["rel_error"]))), repr(float(F(p["lum_floor"]))), str(fm), str(fc), str(fl), str(grid)])
    lst = np.fromfile(fl, np.uint32)
    assert int(out.split()[-1]) == lst.size
    return lst


def emu_normalize(emu, tmp, sums, counts, target, grid, alias):
    h, w = counts.shape
    fs, fc, fo = tmp / "sums.f32", tmp / "counts.u32", tmp / "out.f32"
    sums.tofile(fs)
    counts.tofile(fc)
    _run([emu, "normalize", str(w), str(h), str(sums.shape[-1]), str(target), str(fs), str(fc), str(fo), str(grid),
          "1" if alias else "0"])
    return np.fromfile(fo, F).reshape(sums.shape)


@pytest.mark.parametrize("w,h,grid", SIZES)
def test_selection_equals_reference(emu, tmp_path, w, h, grid):
    seen = set()
    for name in R.PATTERNS:
        mom, counts = R.pattern(name, w, h)
        for nb in (0, 1):
            ref = R.select(mom, counts, R.PATTERN_MAX_SPP, neighbourhood=nb)
            got = emu_select(emu, tmp_path, mom, counts, R.PATTERN_MAX_SPP, grid, neighbourhood=nb)
            assert np.array_equal(got, ref), (name, nb, got[:8], ref[:8])
            seen.add((name, nb, ref.size))
    n = w * h
    sizes = {(name, nb): k for name, nb, k in seen}
    assert sizes[("none", 0)] == sizes[("none", 1)] == 0
    assert sizes[("all", 0)] == sizes[("all", 1)] == n
    for name in ("last", "first", "corner", "edge", "interior"):
        assert sizes[(name, 0)] == 1
    # one unconverged pixel keeps its whole neighbourhood inside the image
    assert sizes[("corner", 1)] == min(w, 2) * min(h, 2)
    assert sizes[("interior", 1)] == min(w, 3) * min(h, 3)
    assert sizes[("edge", 1)] == min(w, 2) * min(h, 3)
    if n > 1:
        assert 0 < sizes[("mixed", 0)] < sizes[("mixed", 1)] < n


def test_grid_does_not_change_the_list(emu, tmp_path):
    mom, counts = R.pattern("mixed", 40, 24)
    ref = R.select(mom, counts, R.PATTERN_MAX_SPP)
    for grid in (1, 2, 959, 960, 961, 5000):
        assert np.array_equal(emu_select(emu, tmp_path, mom, counts, R.PATTERN_MAX_SPP, grid), ref), grid


def test_not_in_call_and_finished_pixels_are_never_listed_or_neighbours(emu, tmp_path):
    """counts 0 and counts == max_spp beside unconverged pixels: neither is
    listed, and their moments never keep a neighbour."""
    w, h = 40, 24
    mom, counts = R.pattern("all", w, h)
    counts[:, ::4] = 0
    counts[::3, :] = R.PATTERN_MAX_SPP
    got = emu_select(emu, tmp_path, mom, counts, R.PATTERN_MAX_SPP, 97)
    ref = R.select(mom, counts, R.PATTERN_MAX_SPP)
    assert np.array_equal(got, ref) and 0 < got.size < w * h
    live = (counts.reshape(-1) != 0) & (counts.reshape(-1) < R.PATTERN_MAX_SPP)
    assert live[got].all() and got.size == live.sum()
    # only dead pixels unconverged: nothing is listed, with the dilation too
    mom2, _ = R.pattern("none", w, h)
    mom2[~live.reshape(h, w)] = mom[~live.reshape(h, w)]
    assert emu_select(emu, tmp_path, mom2, counts, R.PATTERN_MAX_SPP, 97).size == 0
    assert R.select(mom2, counts, R.PATTERN_MAX_SPP).size == 0


def test_a_rounds_selection_takes_only_pixels_at_the_current_count(emu, tmp_path):
    """cur > 0 (the rounds of a render): a pixel with fewer samples has left
    the active set and does not return, nor does it keep a neighbour."""
    w, h = 40, 24
    mom, counts = R.pattern("all", w, h)
    counts[:, : w // 2] = 4
    mom[:, : w // 2] = mom[:, : w // 2] / F(2)
    got = emu_select(emu, tmp_path, mom, counts, R.PATTERN_MAX_SPP, 97, cur=8)
    ref = R.select(mom, counts, R.PATTERN_MAX_SPP, cur=8)
    assert np.array_equal(got, ref)
    assert got.size == h * (w - w // 2) and (got % w >= w // 2).all()


@pytest.mark.parametrize("w,h,grid", SIZES)
@pytest.mark.parametrize("alias", [False, True])
def test_normalize_equals_reference(emu, tmp_path, w, h, grid, alias):
    rng = np.random.default_rng(w * 31 + h)
    for ch in (1, 3, 8):
        sums = (rng.random((h, w, ch)) * 40).astype(F)
        counts = rng.integers(0, 65, (h, w)).astype(np.uint32)
        counts.reshape(-1)[0] = 0 if w * h > 1 else 7
        sums[counts == 0] = F(-2.5)
        sums.view(np.uint32)[counts == 0, 0] = 0x7FC00123   # a NaN payload survives a bit copy
        ref = R.normalize(sums, counts, 64)
        got = emu_normalize(emu, tmp_path, sums, counts, 64, grid, alias)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), ch
        assert np.array_equal(got.view(np.uint32)[counts == 0], sums.view(np.uint32)[counts == 0])
        one = counts == 64   # a pixel that took the whole budget keeps its sums
        assert np.array_equal(got[one], sums[one])
