"""The ray-query entry points of include/rtgpu.h: declared, exported, mirrored
by ctypes with the C layout, refusals that need no device, ABI version
unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_trace_rays", "rt_trace_rays_device", "rt_occluded", "rt_occluded_device"]
RAY_FIELDS = ["o", "tmin", "d", "tmax"]
HIT_FIELDS = ["t", "top", "prim", "material", "n", "flags"]


def test_new_entry_points_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    for t in ("rt_ray", "rt_ray_hit"):
        assert f"typedef struct {t} " in hdr and f"}} {t};" in hdr
    assert "RT_HIT_FRONT = 1" in hdr and "RT_HIT_INVALID_RAY = 2" in hdr
    # the header states the interval ends, the refusal of volumes and its follow-up
    assert "t < tmax" in hdr and "tmin <= t" in hdr and "RT_VOLUME" in hdr and "follow-up" in hdr
    # the Python layer over them
    for name in ("trace_rays", "occluded", "trace_rays_device", "occluded_device"):
        assert callable(getattr(g.Context, name))
    assert g.RtRay and g.RtRayHit and (g.RT_HIT_FRONT, g.RT_HIT_INVALID_RAY) == (1, 2)


def test_struct_mirrors_match_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    items = [("rt_ray", RAY_FIELDS), ("rt_ray_hit", HIT_FIELDS)]
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
    for (t, fields), line, cls, dt in zip(items, out, (g.RtRay, g.RtRayHit), (g.RAY_DTYPE, g.RAY_HIT_DTYPE)):
        size, *offsets = map(int, line.split())
        assert size == C.sizeof(cls) == dt.itemsize == 32, t
        assert [n for n, _ in cls._fields_] == fields
        assert offsets == [getattr(cls, f).offset for f in fields], t
        assert offsets == [dt.fields[f][1] for f in fields], t
    assert [getattr(g.RtRay, f).offset for f in RAY_FIELDS] == [0, 12, 16, 28]
    assert [getattr(g.RtRayHit, f).offset for f in HIT_FIELDS] == [0, 4, 8, 12, 16, 28]


def test_make_rays(g):
    r = g.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [0, 1, 0]], tmin=[0.5, 0.25], tmax=7.0)
    assert r.dtype == g.RAY_DTYPE and r.shape == (2,)
    assert r["o"].tolist() == [[1, 2, 3], [4, 5, 6]] and r["d"].tolist() == [[0, 0, 1], [0, 1, 0]]
    assert r["tmin"].tolist() == [0.5, 0.25] and r["tmax"].tolist() == [7.0, 7.0]
    assert np.isinf(g.make_rays(np.zeros((1, 3)), np.ones((1, 3)))["tmax"][0])
    with pytest.raises(ValueError):
        g.make_rays(np.zeros((2, 3)), np.zeros((3, 3)))


def test_null_and_negative_arguments_are_refused_without_a_device(g):
    lib = g.rtgpu()
    ray, hit, occ = g.RtRay(), g.RtRayHit(), C.c_uint8(0)
    assert lib.rt_trace_rays(None, None, 0, 0.0, None) == -1
    assert lib.rt_trace_rays(None, C.byref(ray), 1, 0.0, C.byref(hit)) == -1
    assert lib.rt_trace_rays_device(None, None, 1, 0.0, None, None) == -1
    assert lib.rt_occluded(None, None, 0, 0.0, None) == -1
    assert lib.rt_occluded(None, C.byref(ray), -1, 0.0, C.byref(occ)) == -1
    assert lib.rt_occluded_device(None, None, 1, 0.0, None, None) == -1


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
