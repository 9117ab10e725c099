"""The rows of tests/xform_cases.py (transform.go's wrapper chains; expected
values from tests/path_ref.py, float64 from the Go text alone) through the
GPU, via the C-ABI: the production k_extend's records (rt_extend_hits) and
k_shadow's (rt_shadow_visibility) at every bounce to the row's depth, the
production render at the row's samples, and rt_scene_info's node format.
Every row runs with the default options; wrap_long and wrap_inner with
RT_NODES_QUANT8, RT_NODES_WIDE8 and the reference world builder as well, the
mesh of wrap_inner with each RT_OPT_BLAS_BUILDER setting.  The long-tail
kernel takes paths only in scenes without a light, and every row has one, so
no row runs through it.

Feature normals (rt_render_features) of wrap_each, wrap_long and wrap_inner,
in the same run as the row's default options: unit(A^T n_obj), A the product
of the chain's ray maps, n_obj faced against the object-space ray, in
float64 from the row's data; unit length and facing the ray (1e-5); quads,
triangles and circles 1e-5 absolute, spheres four times the float32 figure of
tests/test_xform_kat.py test_ball_normal_figure.

The two refusals (a chain of seven, a wrapped plane) are raised by upload
with RT_ERR_UNSUPPORTED, and the context renders a valid scene afterwards.

Tolerances: those of tests/test_xform_kat.py for the device (4 x the fp32
oracle's measured error on the CPU; ids, ended paths, NEE bits and the node
format exact).  Frames are 24 x 16, at most 2 samples, depth at most 3."""
import numpy as np
import pytest

from tests import path_cases as PC
from tests import xform_cases as XC
from tests.test_path_kat import MEASURED_FP32, check_radiance, check_records
from tests.test_xform_kat import chain_of_seven, check_prims, grp, taken, valid_scene, wrapped_plane

pytestmark = pytest.mark.gpu

FLAT_NORMAL = 1e-5                           # tests/test_gpu_features.py's bar
RUNS = ([(n, v, "default") for n, v in XC.ROWS] + XC.MODE_ROWS
        + [("wrap_inner", "mesh", f"blas_{b}") for b in ("reference", "sah", "device")])


def check_feature_normals(what, g, ctx, c, variant, cam):
    want, flat, ball = XC.expected_normals(c, g, variant)
    e = c.expected(g, variant)
    f, _ = ctx.render_features(cam, g.make_params(1, 1, seed=PC.SEED))
    f = f.reshape(-1, 8)
    both = flat | ball
    assert (f[both, 7] == 1).all(), f"{what}: a wrapped hit is not covered"
    nrm = f[:, 3:6].astype(np.float64)
    unit = float(np.abs(np.linalg.norm(nrm[both], axis=1) - 1.0).max())
    facing = np.sum(nrm[both] * e["ray"][0][0][both, 3:6], axis=1)
    err_flat = float(np.abs(nrm[flat] - want[flat]).max()) if flat.any() else 0.0
    err_ball = float(np.abs(nrm[ball] - want[ball]).max()) if ball.any() else 0.0
    bar_ball = 4.0 * MEASURED_FP32[c.group_of(variant)].get("n_ball", FLAT_NORMAL / 4.0)
    print(f"{what} feature normals: {int(flat.sum())} flat pixels off by {err_flat:.3g} (bar {FLAT_NORMAL:.3g}), "
          f"{int(ball.sum())} sphere pixels off by {err_ball:.3g} (bar {bar_ball:.3g}), | |n| - 1 | {unit:.3g}")
    assert both.sum() >= 12
    assert unit <= 1e-5 and (facing < 0).all(), f"{what}: unit {unit}, facing {facing.max()}"
    assert err_flat <= FLAT_NORMAL, f"{what}: flat normals off by {err_flat}"
    assert err_ball <= bar_ball, f"{what}: sphere normals off by {err_ball} (bar {bar_ball})"


@pytest.mark.parametrize("name,variant,mode", RUNS, ids=["-".join(x for x in r if x) for r in RUNS])
def test_gpu_wrapper_chains(g, ctx, name, variant, mode):
    c = XC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    what = f"{name}[{variant}] {mode} GPU"
    try:
        ctx.set_node_format(mode if mode in ("quant8", "wide8") else "fp32")
        ctx.set_tlas_builder("reference" if mode == "tlas_reference" else "sah")
        ctx.set_blas_builder(mode[5:] if mode.startswith("blas_") else "sah")
        b, d, cam, ids = c.build(g, variant)
        ctx.upload(d)
        assert ctx.info().node_format == taken(c, variant, mode), f"{what}: node format {ctx.info().node_format}"
        for s in range(e["samples"]):
            for k in range(e["depth"]):
                top, prim, t, ray = ctx.extend_hits(cam, PC.SEED, s, k)
                nee = ctx.shadow_visibility(cam, PC.SEED, s, k)
                check_records(what, grp(c, variant), e, ids, s, k, top, t, ray, nee, "device", bits="nee_dev")
                if c.prim:
                    check_prims(what, c, e, s, k, prim)
        L, _ = ctx.render(cam, g.make_params(e["samples"], e["depth"], seed=PC.SEED))
        check_radiance(what, grp(c, variant), e, L, "device")
        if mode == "default" and (name, variant) in XC.FEATURE_ROWS:
            check_feature_normals(what, g, ctx, c, variant, cam)
    finally:
        ctx.set_node_format("fp32")
        ctx.set_tlas_builder("sah")
        ctx.set_blas_builder("sah")


@pytest.mark.parametrize("make", [chain_of_seven, wrapped_plane], ids=["chain_of_seven", "wrapped_plane"])
def test_gpu_refusals(g, ctx, make):
    b, d = make(g)
    with pytest.raises(g.RTError) as ex:
        ctx.upload(d)
    assert ex.value.code == -2               # RT_ERR_UNSUPPORTED
    c = XC.CASES["wrap_long"]
    e = c.expected(g, "len6")
    vb, vd, cam, ids = valid_scene(g)
    ctx.upload(vd)
    L, _ = ctx.render(cam, g.make_params(e["samples"], e["depth"], seed=PC.SEED))
    check_radiance("wrap_long[len6] after a refusal", grp(c, "len6"), e, L, "device")
