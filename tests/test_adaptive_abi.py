"""The adaptive-sampling entry points of include/rtgpu.h: declared, exported,
mirrored by ctypes with the C layout, documented defaults, refusals that need
no device, ABI version unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_adaptive_default_params", "rt_render_adaptive", "rt_render_adaptive_device", "rt_adaptive_select",
       "rt_normalize_samples", "rt_normalize_samples_device"]
PARAM_FIELDS = ["min_spp", "step_spp", "neighbourhood", "rel_error", "lum_floor"]
STATS_FIELDS = ["kernel_ms", "samples", "rounds", "pixels_at_max"]


def test_new_entry_points_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    for t in ("rt_adaptive_params", "rt_adaptive_stats"):
        assert f"typedef struct {t} {{" in hdr and f"}} {t};" in hdr
    # the header states the rounds, the blocking and the bias
    assert "biased estimator" in hdr and "Both variants block" in hdr
    # the Python layer over them
    for name in ("render_adaptive", "render_adaptive_device", "adaptive_select", "normalize_samples",
                 "normalize_samples_device"):
        assert callable(getattr(g.Context, name))
    assert g.RtAdaptiveParams and g.RtAdaptiveStats and callable(g.adaptive_params)


def test_struct_mirrors_match_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    items = [("rt_adaptive_params", PARAM_FIELDS), ("rt_adaptive_stats", STATS_FIELDS)]
    lines = []
    for t, fields in items:
        offs = ", ".join(f"offsetof({t}, {f})" for f in fields)
        fmt = " ".join(["%zu"] * (len(fields) + 1))
        lines.append(f'  printf("{fmt}\\n", sizeof({t}), {offs});')
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtgpu.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for (t, fields), line, cls in zip(items, out, (g.RtAdaptiveParams, g.RtAdaptiveStats)):
        size, *offsets = map(int, line.split())
        assert size == C.sizeof(cls), t
        assert [n for n, _ in cls._fields_] == fields
        assert offsets == [getattr(cls, f).offset for f in fields], t
    assert C.sizeof(g.RtAdaptiveParams) == 20
    assert [getattr(g.RtAdaptiveParams, f).offset for f in PARAM_FIELDS] == [0, 4, 8, 12, 16]
    assert C.sizeof(g.RtAdaptiveStats) == 24


def test_default_params(g):
    ap = g.RtAdaptiveParams()
    assert g.rtgpu().rt_adaptive_default_params(C.byref(ap)) == 0
    assert (ap.min_spp, ap.step_spp, ap.neighbourhood) == (16, 16, 1)
    assert ap.rel_error == pytest.approx(0.05) and ap.lum_floor == pytest.approx(0.01)
    assert g.rtgpu().rt_adaptive_default_params(None) == -1   # RT_ERR_INVALID
    # the Python helper: defaults with overrides, unknown names refused
    p = g.adaptive_params(min_spp=4, rel_error=0.5, neighbourhood=0)
    assert (p.min_spp, p.step_spp, p.neighbourhood) == (4, 16, 0) and p.rel_error == 0.5
    with pytest.raises(TypeError):
        g.adaptive_params(sigma_lum=1.0)
    # tests/adaptive_ref.py restates the same defaults
    from tests import adaptive_ref as R
    assert list(R.DEFAULTS) == PARAM_FIELDS
    for k, v in R.DEFAULTS.items():
        assert getattr(ap, k) == pytest.approx(v), k
    with pytest.raises(TypeError):
        R.select(None, None, 1, sigma_lum=1.0)


def test_null_arguments_are_refused_without_a_device(g):
    lib = g.rtgpu()
    assert lib.rt_render_adaptive(None, None, None, None, None, None, None, None) == -1
    assert lib.rt_render_adaptive_device(None, None, None, None, None, None, None, None, None) == -1
    assert lib.rt_adaptive_select(None, None, None, 4, 4, 16, None, None, None) == -1
    assert lib.rt_normalize_samples(None, None, 3, None, 4, 4, 16, None) == -1
    assert lib.rt_normalize_samples_device(None, None, 3, None, 4, 4, 16, None, None) == -1


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
