"""The feature-buffer / denoiser entry points of include/rtgpu.h: exported,
mirrored by ctypes with the C layout, documented defaults, ABI version
unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_render_features", "rt_render_features_device", "rt_denoise_default_params", "rt_denoise",
       "rt_denoise_device"]


def test_new_entry_points_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    assert "typedef struct rt_denoise_params {" in hdr and "} rt_denoise_params;" in hdr
    # the Python layer over them
    for name in ("render_features", "render_features_device", "denoise", "denoise_device"):
        assert callable(getattr(g.Context, name))
    assert g.RtDenoiseParams


def test_denoise_params_mirror_matches_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtgpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(rt_denoise_params), offsetof(rt_denoise_params, sigma_color),\n'
                   '         offsetof(rt_denoise_params, albedo_eps));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_sc, off_eps = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(g.RtDenoiseParams) == 24
    assert off_sc == g.RtDenoiseParams.sigma_color.offset == 12
    assert off_eps == g.RtDenoiseParams.albedo_eps.offset == 20


def test_default_params(g):
    dp = g.RtDenoiseParams()
    assert g.rtgpu().rt_denoise_default_params(C.byref(dp)) == 0
    assert (dp.iterations, dp.normal_power_log2, dp.demodulate) == (5, 5, 1)
    assert dp.sigma_color == pytest.approx(4.0) and dp.sigma_depth == pytest.approx(0.1)
    assert dp.albedo_eps == pytest.approx(1e-3)
    assert g.rtgpu().rt_denoise_default_params(None) == -1   # RT_ERR_INVALID
    # the Python helper: defaults with overrides, unknown names refused
    p = g.denoise_params(iterations=2, sigma_color=0.5)
    assert (p.iterations, p.normal_power_log2) == (2, 5) and p.sigma_color == 0.5
    with pytest.raises(TypeError):
        g.denoise_params(sigma=1.0)
    # tests/denoise_ref.py restates the same defaults
    from tests import denoise_ref as R
    for k, v in R.DEFAULTS.items():
        assert getattr(dp, k) == pytest.approx(v), k


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
