"""rt_ray_color's entry points of include/rtgpu.h: declared, exported, mirrored
by ctypes and numpy with the C layout, refusals that need no device, ABI
version unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_ray_color", "rt_ray_color_device"]
RAY_FIELDS = ["o", "id", "d", "reserved"]
PARAM_FIELDS = ["samples", "max_depth", "sample_offset", "seed", "accumulate", "use_sky_gradient", "phantom_hdri",
                "camera_max_depth", "background"]
STAT_FIELDS = ["kernel_ms", "samples", "invalid_rays"]


def test_new_entry_points_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    for t in ("rt_path_ray", "rt_ray_color_params", "rt_ray_color_stats"):
        assert f"typedef struct {t} " in hdr and f"}} {t};" in hdr
    # the header states the defining equality, the key, the invalid-ray rule and what is not offered
    for text in ("bit for bit", "path_key(seed, rays[i].id, sample_offset + s)", "invalid_rays", "per-ray tmin / tmax",
                 "camera_max_depth", "RT_VOLUME"):
        assert text in hdr, text
    for name in ("ray_color", "ray_color_device"):
        assert callable(getattr(g.Context, name))
    assert callable(g.make_path_rays) and callable(g.ray_color_params)


def test_struct_mirrors_match_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    items = [("rt_path_ray", RAY_FIELDS), ("rt_ray_color_params", PARAM_FIELDS), ("rt_ray_color_stats", STAT_FIELDS)]
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
    for (t, fields), line, cls in zip(items, out, (g.RtPathRay, g.RtRayColorParams, g.RtRayColorStats)):
        size, *offsets = map(int, line.split())
        assert size == C.sizeof(cls), t
        assert [n for n, _ in cls._fields_] == fields
        assert offsets == [getattr(cls, f).offset for f in fields], t
    size, *offsets = map(int, out[0].split())
    assert size == g.PATH_RAY_DTYPE.itemsize == 32
    assert offsets == [g.PATH_RAY_DTYPE.fields[f][1] for f in RAY_FIELDS] == [0, 12, 16, 28]
    assert C.sizeof(g.RtRayColorParams) == 56 and g.RtRayColorParams.background.offset == 32
    assert C.sizeof(g.RtRayColorStats) == 24


def test_make_path_rays_and_params(g):
    r = g.make_path_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [0, 1, 0]])
    assert r.dtype == g.PATH_RAY_DTYPE and r.shape == (2,)
    assert r["o"].tolist() == [[1, 2, 3], [4, 5, 6]] and r["d"].tolist() == [[0, 0, 1], [0, 1, 0]]
    assert r["id"].tolist() == [0, 1] and r["reserved"].tolist() == [0, 0]
    assert g.make_path_rays(np.zeros((2, 3)), np.ones((2, 3)), ids=[7, 1 << 31])["id"].tolist() == [7, 1 << 31]
    with pytest.raises(ValueError):
        g.make_path_rays(np.zeros((2, 3)), np.zeros((3, 3)))
    cam = g.RtCameraDesc()
    cam.background[0], cam.background[1], cam.background[2] = 0.25, 0.5, 0.75
    cam.use_sky_gradient, cam.phantom_hdri, cam.max_depth = 1, 1, 9
    p = g.ray_color_params(3, 5, seed=11, sample_offset=2, camera=cam)
    assert (p.samples, p.max_depth, p.sample_offset, p.seed, p.accumulate) == (3, 5, 2, 11, 0)
    assert (p.use_sky_gradient, p.phantom_hdri, p.camera_max_depth, list(p.background)) == (1, 1, 9, [0.25, 0.5, 0.75])
    p = g.ray_color_params(1, 2, camera=cam, background=(1, 2, 3), phantom_hdri=0, accumulate=True)
    assert (p.phantom_hdri, p.accumulate, list(p.background)) == (0, 1, [1.0, 2.0, 3.0])
    with pytest.raises(TypeError):
        g.ray_color_params(1, 2, sky=1)


def test_null_arguments_are_refused_without_a_device(g):
    lib = g.rtgpu()
    ray, p, rgb = g.RtPathRay(), g.ray_color_params(1, 1), (C.c_float * 3)()
    assert lib.rt_ray_color(None, None, 0, None, None, None) == -1
    assert lib.rt_ray_color(None, C.byref(ray), 1, C.byref(p), rgb, None) == -1
    assert lib.rt_ray_color_device(None, None, 1, None, None, None) == -1
    assert lib.rt_ray_color_device(None, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
