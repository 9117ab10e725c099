"""The rows of tests/stack_cases.py (the traversal stack bound on deep
hand-built trees; expected values from tests/path_ref.py, brute force in
float64) through the GPU, via the C-ABI.  For every row and node format:

  * rt_scene_info's stack_needed and node_format are what the host table says
    (tests/test_stack_host.py FIGURES, from the construction);
  * rt_primary_hits equals the fp32 oracle bit for bit (the rays are the
    same), rt_extend_hits and rt_shadow_visibility at every bounce equal the
    reference (ids, ended paths, NEE bits exact; t and rays within the bars);
  * a render raises no device error (a dropped stack entry is RT_ERR_DEVICE)
    and is within 4 x the measured fp32 error of the reference and within
    test_gpu_parity's fp32 bar of the oracle;
  * rt_count_work's stack_spills is positive where a ray holds more than the
    8-entry LDS ring and 0 for `balanced` and the chain of four.

The exact accepted / refused depths are raised at upload, before any kernel
runs; no test overflows a stack on the GPU.  device_deep: the mesh is built on
the device, stack_needed follows the device tree's need4 (tests/lbvh_ref.py),
and the records equal both the reference and the host-built scene's.

Tolerances: tests/test_stack_host.py's for the device (group `stack`)."""
import numpy as np
import pytest

from tests import lbvh_ref as LR
from tests import mesh_cases as M
from tests import path_cases as PC
from tests import stack_cases as SC
from tests.test_gpu_parity import fp32_bar
from tests.test_path_kat import check_radiance, check_records
from tests.test_stack_host import FIGURES, K_LDS_STACK, K_STACK_MAX, taken
from tests.test_xform_kat import check_prims, grp

pytestmark = pytest.mark.gpu

SPILLS = {("chain_ref", "n4"): False, ("balanced", ""): False}      # the others hold more than the ring


def configure(ctx, name, fmt="fp32", blas=None):
    ctx.set_node_format(fmt)
    ctx.set_tlas_builder("sah" if name == "balanced" else "reference")
    ctx.set_blas_builder(blas or ("sah" if name == "balanced" else "reference"))


def restore(ctx):
    ctx.set_node_format("fp32")
    ctx.set_tlas_builder("sah")
    ctx.set_blas_builder("sah")
    ctx.set_tail(0)


def records(ctx, what, c, variant, e, ids, cam):
    """Every bounce's records against the reference; returns them."""
    out = []
    for k in range(e["depth"]):
        top, prim, t, ray = ctx.extend_hits(cam, PC.SEED, 0, k)
        nee = ctx.shadow_visibility(cam, PC.SEED, 0, k)
        check_records(what, grp(c, variant), e, ids, 0, k, top, t, ray, nee, "device", bits="nee_dev")
        check_prims(what, c, e, 0, k, prim)
        out.append((top, prim, t, nee))
    return out


@pytest.mark.parametrize("name,variant,fmt", SC.FORMAT_ROWS, ids=["-".join(x for x in r if x) for r in SC.FORMAT_ROWS])
def test_gpu_stack_rows(g, O, ctx, name, variant, fmt):
    c = SC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    what = f"{name}[{variant}] {fmt} GPU"
    fig = FIGURES[(name, variant)]
    try:
        configure(ctx, name, fmt)
        b, d, cam, ids = c.build(g, variant)
        ctx.upload(d)
        info = ctx.info()
        used = taken(name, variant, fmt)
        assert info.node_format == used, f"{what}: node format {info.node_format}"
        if fig["bound"] is not None:      # (rt_scene_info reports the 4-wide bound in every format)
            assert info.stack_needed == fig["bound"], f"{what}: stack_needed {info.stack_needed}, the table {fig['bound']}"
        assert 0 < info.stack_needed <= K_STACK_MAX
        # the camera rays are the oracle's: bit for bit
        tg, pg, t_g = ctx.primary_hits(cam, PC.SEED, 0)
        to, po, t_o = O.primary_hits(d, cam, PC.SEED, 0, fp32=True)
        assert np.array_equal(tg, to) and np.array_equal(pg, po), f"{what}: first hits differ from the fp32 oracle's"
        hit = tg >= 0
        assert np.array_equal(t_g[hit], t_o[hit].astype(np.float32)), f"{what}: first-hit t differs from the fp32 oracle's"
        rec = records(ctx, what, c, variant, e, ids, cam)
        assert np.array_equal(rec[0][0], tg) and np.array_equal(rec[0][1], pg) and np.array_equal(rec[0][2][hit], t_g[hit])
        p = g.make_params(e["samples"], e["depth"], seed=PC.SEED)
        L, _ = ctx.render(cam, p)
        ctx.sync()                                              # raises on a device error
        check_radiance(what, grp(c, variant), e, L, "device")
        ref = O.render(d, cam, p, fp32=True, threads=2)
        fp32_bar(what, L, np.asarray(ref).reshape(L.shape), e["samples"])
        spills = ctx.count_work(cam, p)["stack_spills"]
        print(f"{what}: stack_needed {info.stack_needed} stack_spills {spills}")
        if SPILLS.get((name, variant), True):
            assert spills > 0, f"{what}: no ray left the {K_LDS_STACK}-entry ring"
        else:
            assert spills == 0, f"{what}: {spills} pushes beyond the {K_LDS_STACK}-entry ring"
    finally:
        restore(ctx)


def test_gpu_tail_kernel_on_a_deep_stack(g, ctx):
    """chain_ref without a light at depth 12 (stack_needed 16): the long-tail
    kernel taking every path after bounce 0 gives the same bits as the
    per-bounce kernels."""
    c = SC.CASES["chain_ref"]
    e = c.expected(g, "n12dark")
    try:
        configure(ctx, "chain_ref")
        b, d, cam, ids = c.build(g, "n12dark")
        ctx.upload(d)
        assert ctx.info().stack_needed == FIGURES[("chain_ref", "n12dark")]["bound"] > K_LDS_STACK
        p = g.make_params(e["samples"], e["depth"], seed=PC.SEED)
        ctx.set_tail(1)                                         # off: every bounce through the per-bounce kernels
        per_bounce, _ = ctx.render(cam, p)
        ctx.set_tail(1 << 30)                                   # every path left after bounce 0 goes to k_tail
        tail, _ = ctx.render(cam, p)
        ctx.sync()
        assert np.array_equal(per_bounce.view(np.uint32), tail.view(np.uint32))
        check_radiance("chain_ref[n12dark] GPU tail", grp(c, "n12dark"), e, tail, "device")
    finally:
        restore(ctx)


@pytest.mark.parametrize("name,edge", [("chain_ref", "chain_ref"), ("chain_dfs", "chain_dfs")])
def test_gpu_refused_one_link_past_the_bound(g, ctx, name, edge):
    """The first refused depth is RT_ERR_UNSUPPORTED at upload in every node
    format, and the deepest accepted chain (stack_needed 128) uploads right
    after it."""
    c = SC.CASES[name]
    E = SC.EDGES[edge]
    try:
        for fmt in ("fp32", "quant8", "wide8"):
            configure(ctx, name, fmt)
            with pytest.raises(g.RTError) as ex:
                ctx.upload(c.build(g, f"n{E['refused']}")[1])
            assert ex.value.code == -2                           # RT_ERR_UNSUPPORTED (include/rtgpu.h)
            b, d, cam, ids = c.build(g, f"n{E['accepted']}")
            ctx.upload(d)
            assert ctx.info().stack_needed == K_STACK_MAX
            assert (ctx.primary_hits(cam, PC.SEED, 0)[0] >= 0).sum() > PC.N // 3
    finally:
        restore(ctx)


def test_gpu_device_built_mesh_under_a_deep_chain(g, ctx):
    c = SC.CASES["device_deep"]
    variant = f"w{SC.W_DEVICE}"
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    need4 = LR.build(*M.boxes32(M.boxes64(SC.device_mesh_object_space()))).need4
    try:
        b, d, cam, ids = c.build(g, variant)
        configure(ctx, "device_deep", blas="device")
        ctx.upload(d)
        assert ctx.last_build_ms() > 0.0
        dev = ctx.info()
        # the world chain's W + 3 pending items, the instance, its entry marker and the two spare entries: W + 7
        assert dev.stack_needed == SC.W_DEVICE + 7 + need4, f"stack_needed {dev.stack_needed}, the device tree's need4 {need4}"
        assert K_STACK_MAX - 8 <= dev.stack_needed <= K_STACK_MAX
        got = records(ctx, "device_deep device-built", c, variant, e, ids, cam)
        p = g.make_params(e["samples"], e["depth"], seed=PC.SEED)
        L, _ = ctx.render(cam, p)
        ctx.sync()
        check_radiance("device_deep device-built", grp(c, variant), e, L, "device")
        assert ctx.count_work(cam, p)["stack_spills"] > 0
        configure(ctx, "device_deep", blas="sah")
        ctx.upload(d)
        host = ctx.info()
        assert host.stack_needed != dev.stack_needed and host.triangles == dev.triangles
        want = records(ctx, "device_deep host-built", c, variant, e, ids, cam)
        for k, (a, bb) in enumerate(zip(got, want)):
            for x, y, f in zip(a, bb, ("top", "prim", "t", "nee")):
                assert np.array_equal(x, y), f"device_deep b{k}: {f} differs between the device-built and the host-built scene"
    finally:
        restore(ctx)
