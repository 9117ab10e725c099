"""The radiance-moments / variance-guided denoiser entry points of
include/rtgpu.h: exported, mirrored by ctypes with the C layout, documented
defaults, ABI version unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_render_moments", "rt_render_moments_device", "rt_denoise_variance_default_params", "rt_denoise_variance",
       "rt_denoise_variance_device"]
FIELDS = ["iterations", "normal_power_log2", "demodulate", "spatial_below", "sigma_lum", "sigma_depth", "albedo_eps"]


def test_new_entry_points_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    assert "typedef struct rt_denoise_var_params {" in hdr and "} rt_denoise_var_params;" in hdr
    # the Python layer over them
    for name in ("render_moments", "render_moments_device", "denoise_variance", "denoise_variance_device"):
        assert callable(getattr(g.Context, name))
    assert g.RtDenoiseVarParams and callable(g.denoise_variance_params)


def test_denoise_var_params_mirror_matches_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    offs = ", ".join(f"offsetof(rt_denoise_var_params, {f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtgpu.h"\nint main(void) {\n'
                   f'  printf("{fmt}\\n", sizeof(rt_denoise_var_params), {offs});\n  return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offsets = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(g.RtDenoiseVarParams) == 28
    assert [n for n, _ in g.RtDenoiseVarParams._fields_] == FIELDS
    assert offsets == [getattr(g.RtDenoiseVarParams, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24]


def test_default_params(g):
    dp = g.RtDenoiseVarParams()
    assert g.rtgpu().rt_denoise_variance_default_params(C.byref(dp)) == 0
    assert (dp.iterations, dp.normal_power_log2, dp.demodulate, dp.spatial_below) == (5, 5, 1, 4)
    assert dp.sigma_depth == pytest.approx(0.1) and dp.albedo_eps == pytest.approx(1e-3)
    assert dp.sigma_lum > 0
    assert g.rtgpu().rt_denoise_variance_default_params(None) == -1   # RT_ERR_INVALID
    # sigma_depth / albedo_eps are rt_denoise's
    d0 = g.denoise_params()
    assert (dp.sigma_depth, dp.albedo_eps) == (d0.sigma_depth, d0.albedo_eps)
    # the Python helper: defaults with overrides, unknown names refused
    p = g.denoise_variance_params(iterations=2, sigma_lum=0.5, spatial_below=2)
    assert (p.iterations, p.normal_power_log2, p.spatial_below) == (2, 5, 2) and p.sigma_lum == 0.5
    with pytest.raises(TypeError):
        g.denoise_variance_params(sigma_color=1.0)
    # tests/denoise_var_ref.py restates the same defaults
    from tests import denoise_var_ref as R
    assert set(R.DEFAULTS) == set(FIELDS)
    for k, v in R.DEFAULTS.items():
        assert getattr(dp, k) == pytest.approx(v), k


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
