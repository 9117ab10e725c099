"""The SH-projection entry points of include/rtgpu.h: declared, exported,
mirrored by ctypes with the C layout, refusals that need no device, ABI version
unchanged (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sh_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_gather_sh", "rt_gather_sh_device"]


def header():
    with open(os.path.join(ROOT, "include", "rtgpu.h")) as f:
        return f.read()


def test_new_entry_points_declared_and_exported(g):
    hdr = header()
    so = C.CDLL(os.path.join(g.LIB_DIR, "librtgpu.so"))
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert hasattr(so, name), name
    assert "typedef struct rt_gather_sh_params " in hdr and "} rt_gather_sh_params;" in hdr
    assert "enum { RT_SH_MAX_BANDS = 3 };" in hdr
    for name in ("gather_sh", "gather_sh_device"):
        assert callable(getattr(g.Context, name))
    assert callable(g.gather_sh_params) and g.RT_SH_MAX_BANDS == 3
    # the earlier entry points are still there
    for name in ("rt_gather", "rt_gather_device", "rt_gather_rays", "rt_ray_color", "rt_ray_color_device"):
        assert hasattr(so, name), name


def test_header_text(g):
    flat = header().lower().replace("\n *", "")
    # the phrases earlier tests pin stay, and the gather block no longer lists the projection as missing
    for phrase in ("next-event estimation at the gather point", "sh projection", "adaptive sampling over points",
                   "per-point source kinds", "per-ray tmin / tmax or time", "feature buffers for rays"):
        assert phrase in flat, phrase
    assert "---- sh projection of a probe" in flat
    assert "sh projection of a probe, moments" not in flat
    # the new block: the basis, the scale, the irradiance formula, what is not offered
    for text in ("0.282095f", "0.488603f*y", "0.488603f*z", "0.488603f*x", "1.092548f*(x*y)", "1.092548f*(y*z)",
                 "0.315392f*(3.0f*(z*z) - 1.0f)", "1.092548f*(x*z)", "0.546274f*(x*x - y*y)", "ramamoorthi",
                 "4 pi / samples", "a_0 = pi, a_1 = 2 pi / 3, a_2 = pi / 4",
                 "bands above 3", "cosine- or otherwise-weighted projection", "irradiance evaluation on the device",
                 "moments per coefficient"):
        assert text in flat, text


def test_struct_mirror_matches_c_header(g, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtgpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(rt_gather_sh_params), offsetof(rt_gather_sh_params, path),\n'
                   '         offsetof(rt_gather_sh_params, bands), offsetof(rt_gather_sh_params, reserved));\n'
                   '  printf("%zu %d\\n", sizeof(rt_gather_params), (int)RT_SH_MAX_BANDS);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    params, others = ([int(x) for x in line.split()] for line in out)
    assert params == [64, 0, 56, 60]
    assert others == [64, 3]
    assert C.sizeof(g.RtGatherShParams) == 64
    assert [n for n, _ in g.RtGatherShParams._fields_] == ["path", "bands", "reserved"]
    assert [getattr(g.RtGatherShParams, f).offset for f in ("path", "bands", "reserved")] == params[1:]


def test_params_helper(g):
    p = g.gather_sh_params(3, 4, 9, seed=5, sample_offset=2, accumulate=True, background=(0.25, 0.5, 0.75))
    assert (p.bands, p.reserved, p.path.samples, p.path.max_depth, p.path.seed, p.path.sample_offset,
            p.path.accumulate) == (3, 0, 4, 9, 5, 2, 1)
    assert list(p.path.background) == [0.25, 0.5, 0.75]


def test_null_arguments_are_refused_without_a_device(g):
    lib = g.rtgpu()
    pt, sh = g.RtGatherPoint(), (C.c_float * 27)()
    p = g.gather_sh_params(3, 1, 2)
    assert lib.rt_gather_sh(None, None, 0, None, None, None) == -1
    assert lib.rt_gather_sh(None, C.byref(pt), 1, C.byref(p), sh, None) == -1
    assert lib.rt_gather_sh_device(None, None, 1, None, None, None) == -1
    assert lib.rt_gather_sh_device(None, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1


def test_abi_version_unchanged(g):
    assert g.rtgpu().rt_abi_version() == 8
    assert "#define RT_ABI_VERSION 8" in header()


def test_restatement_basis_is_orthonormal():
    """The restated basis integrates to the identity over the sphere (float64
    quadrature of the float32 values; the constants carry six digits)."""
    nt, nphi = 400, 800
    ct, wt = np.polynomial.legendre.leggauss(nt)
    phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
    st = np.sqrt(1 - ct * ct)
    d = np.stack([st[:, None] * np.cos(phi)[None], st[:, None] * np.sin(phi)[None], np.repeat(ct[:, None], nphi, 1)], -1)
    Y = SR.basis(d.astype(np.float32), 3).astype(np.float64)
    assert Y.shape == (nt, nphi, 9) and SR.basis(d[0], 2).shape == (nphi, 4)
    w = wt[:, None] * (2 * np.pi / nphi)
    gram = np.einsum("tpi,tpj,tp->ij", Y, Y, np.broadcast_to(w, (nt, nphi)))
    assert np.abs(gram - np.eye(9)).max() < 1e-5
    assert SR.basis(d[:3, :3], 1).tobytes() == SR.basis(d[:3, :3], 3)[..., :1].tobytes()
