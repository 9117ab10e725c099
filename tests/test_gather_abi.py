"""The gather entry points of include/rtgpu.h: declared, exported, mirrored by
ctypes and numpy with the C layout, refusals that need no device, ABI version
unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_gather", "rt_gather_device", "rt_gather_rays"]
POINT_FIELDS = ["p", "id", "n", "reserved"]


def test_new_entry_points_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    for t in ("rt_gather_point", "rt_gather_params"):
        assert f"typedef struct {t} " in hdr and f"}} {t};" in hdr
    assert "RT_GATHER_RAY = 0, RT_GATHER_COSINE = 1, RT_GATHER_SPHERE = 2" in hdr
    # the header lists what is not offered
    for phrase in ("Next-event estimation at the gather point".lower(), "sh projection", "adaptive sampling over points",
                   "per-point source kinds"):
        assert phrase in hdr.lower().replace("\n *", ""), phrase
    for name in ("gather", "gather_device", "gather_rays"):
        assert callable(getattr(g.Context, name))
    assert (g.RT_GATHER_RAY, g.RT_GATHER_COSINE, g.RT_GATHER_SPHERE) == (0, 1, 2)
    # the earlier entry points are still there
    assert hasattr(so, "rt_ray_color") and hasattr(so, "rt_ray_color_device")


def test_struct_mirrors_match_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtgpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_gather_point), offsetof(rt_gather_point, p),\n'
                   '         offsetof(rt_gather_point, id), offsetof(rt_gather_point, n), offsetof(rt_gather_point, reserved));\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(rt_gather_params), offsetof(rt_gather_params, path),\n'
                   '         offsetof(rt_gather_params, source), offsetof(rt_gather_params, reserved));\n'
                   '  printf("%zu %zu\\n", sizeof(rt_path_ray), sizeof(rt_ray_color_params));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    point, params, others = ([int(x) for x in line.split()] for line in out)
    assert point == [32, 0, 12, 16, 28]
    assert params == [64, 0, 56, 60]
    assert others == [32, 56]
    assert C.sizeof(g.RtGatherPoint) == g.GATHER_POINT_DTYPE.itemsize == 32
    assert [n for n, _ in g.RtGatherPoint._fields_] == POINT_FIELDS
    assert [getattr(g.RtGatherPoint, f).offset for f in POINT_FIELDS] == point[1:]
    assert [g.GATHER_POINT_DTYPE.fields[f][1] for f in POINT_FIELDS] == point[1:]
    assert C.sizeof(g.RtGatherParams) == 64
    assert [getattr(g.RtGatherParams, f).offset for f in ("path", "source", "reserved")] == params[1:]
    # rt_path_ray's layout: a point array can be viewed as a ray array
    assert [g.PATH_RAY_DTYPE.fields[f][1] for f in ("o", "id", "d", "reserved")] == point[1:]


def test_make_gather_points_and_params(g):
    pts = g.make_gather_points([[1, 2, 3], [4, 5, 6]], [[0, 0, 2], [0, 1, 0]])
    assert pts.dtype == g.GATHER_POINT_DTYPE and pts.shape == (2,)
    assert pts["p"].tolist() == [[1, 2, 3], [4, 5, 6]] and pts["n"].tolist() == [[0, 0, 2], [0, 1, 0]]
    assert pts["id"].tolist() == [0, 1] and not pts["reserved"].any()
    assert g.make_gather_points(np.zeros((2, 3)), np.ones((2, 3)), ids=[7, 0xFFFFFFFF])["id"].tolist() == [7, 0xFFFFFFFF]
    with pytest.raises(ValueError):
        g.make_gather_points(np.zeros((2, 3)), np.zeros((3, 3)))
    p = g.gather_params(g.RT_GATHER_COSINE, 4, 9, seed=5, sample_offset=2, background=(0.25, 0.5, 0.75))
    assert (p.source, p.reserved, p.path.samples, p.path.max_depth, p.path.seed, p.path.sample_offset) == (1, 0, 4, 9, 5, 2)
    assert list(p.path.background) == [0.25, 0.5, 0.75]


def test_null_arguments_are_refused_without_a_device(g):
    lib = g.rtgpu()
    pt, ray, rgb = g.RtGatherPoint(), g.RtPathRay(), (C.c_float * 3)()
    p = g.gather_params(g.RT_GATHER_COSINE, 1, 2)
    assert lib.rt_gather(None, None, 0, None, None, None) == -1
    assert lib.rt_gather(None, C.byref(pt), 1, C.byref(p), rgb, None) == -1
    assert lib.rt_gather_device(None, None, 1, None, None, None) == -1
    assert lib.rt_gather_device(None, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
    assert lib.rt_gather_rays(None, None, 0, 0, 1, 0, None) == -1
    assert lib.rt_gather_rays(None, C.byref(pt), 1, 0, 1, 0, C.byref(ray)) == -1


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
