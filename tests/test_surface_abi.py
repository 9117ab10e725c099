"""The surface-gather entry points of include/rtgpu.h: declared, exported,
mirrored by ctypes with the C layout, refusals that need no device, ABI version
unchanged, rt_gather still declared with its three sources (no compute calls:
runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_gather_surface", "rt_gather_surface_device"]


def header():
    with open(os.path.join(ROOT, "include", "rtgpu.h")) as f:
        return f.read()


def test_new_entry_points_declared_and_exported(g):
    hdr = header()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    assert "typedef struct rt_gather_surface_params {" in hdr and "} rt_gather_surface_params;" in hdr
    for name in ("gather_surface", "gather_surface_device"):
        assert callable(getattr(g.Context, name))
    assert callable(g.surface_params)
    # the earlier entry points are still there
    for name in ("rt_gather", "rt_gather_device", "rt_gather_rays", "rt_gather_sh", "rt_gather_sh_device", "rt_ray_color"):
        assert hasattr(so, name), name


def test_header_text():
    flat = header().lower().replace("\n *", "")
    # rt_gather keeps its three sources and still says what it does not do, now pointing at the new call
    assert "enum { RT_GATHER_RAY = 0, RT_GATHER_COSINE = 1, RT_GATHER_SPHERE = 2 };" in header()
    assert "next-event estimation at the gather point itself" in flat
    assert "rt_gather_surface, below" in flat
    # the new block: the definition, how it differs from COSINE, the units, what is not offered
    for text in ("---- surface gathers: next-event estimation at the gather point", "solidcolor(1,1,1)", "dom_scatter = 1",
                 "not dom_source", "clamp at 20", "min(dist - 0.001, dist * (1 - 2^-20))", "direct-only bake",
                 "the reference's estimator as written", "rendered radiance of a white lambertian texel",
                 "pi * rgb / samples", "rt_gather_surface({p, r.id, n}, params) equals rt_ray_color(r, params.path)",
                 "rt_opt_early_miss", "unbiased mis at the first vertex", "a probe for the nee records"):
        assert text in flat, text


def test_struct_mirror_matches_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtgpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(rt_gather_surface_params), offsetof(rt_gather_surface_params, path),\n'
                   '         offsetof(rt_gather_surface_params, reserved), sizeof(((rt_gather_surface_params*)0)->reserved));\n'
                   '  printf("%zu %zu\\n", sizeof(rt_gather_params), sizeof(rt_gather_point));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    params, others = ([int(x) for x in line.split()] for line in out)
    assert params == [64, 0, 56, 8]
    assert others == [64, 32]
    assert C.sizeof(g.RtGatherSurfaceParams) == 64
    assert [n for n, _ in g.RtGatherSurfaceParams._fields_] == ["path", "reserved"]
    assert [getattr(g.RtGatherSurfaceParams, f).offset for f in ("path", "reserved")] == params[1:3]
    assert g.RtGatherSurfaceParams.reserved.size == 8


def test_params_helper(g):
    p = g.surface_params(4, 9, seed=5, sample_offset=2, accumulate=True, background=(0.25, 0.5, 0.75))
    assert (list(p.reserved), p.path.samples, p.path.max_depth, p.path.seed, p.path.sample_offset,
            p.path.accumulate) == ([0, 0], 4, 9, 5, 2, 1)
    assert list(p.path.background) == [0.25, 0.5, 0.75]


def test_null_arguments_are_refused_without_a_device(g):
    lib = g.rtgpu()
    pt, rgb = g.RtGatherPoint(), (C.c_float * 3)()
    p = g.surface_params(1, 2)
    assert lib.rt_gather_surface(None, None, 0, None, None, None) == -1
    assert lib.rt_gather_surface(None, C.byref(pt), 1, C.byref(p), rgb, None) == -1
    assert lib.rt_gather_surface_device(None, None, 1, None, None, None) == -1
    assert lib.rt_gather_surface_device(None, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
    assert "#define RT_ABI_VERSION 8" in header()
