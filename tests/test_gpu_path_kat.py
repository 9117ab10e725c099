"""The rows of tests/path_cases.py (the path integral: NEE at every bounce,
the light-hit rule, depth, light selection, the clamp, shadow rays; expected
values from tests/path_ref.py, float64 from the Go text alone) through the
GPU, via the C-ABI: the production k_extend's records (rt_extend_hits) and
k_shadow's (rt_shadow_visibility) at every bounce to the row's depth, and the
production render at the row's samples.  Every row runs with the default
options; room, lights3 and env_is_area with RT_NODES_QUANT8 as well;
fog_shadow under both RT_OPT_VOLUMES settings; the rows without a light also
with RT_OPT_TAIL handing every path to the long-tail kernel after bounce 0.
Frames are 24 x 16, at most 4 samples, depth at most 6.

Tolerances: those of tests/test_path_kat.py (ids, ended paths and NEE bits
exact; bounce 0 rays atol 1e-5, t rtol 2e-6; later bounces and the radiance
four times the fp32 oracle's measured error on the CPU)."""
import pytest

from tests import path_cases as PC
from tests.test_path_kat import check_radiance, check_records

pytestmark = pytest.mark.gpu

RUNS = ([(n, v, "fp32") for n, v in PC.ROWS] + [(n, v, "quant8") for n, v in PC.ROWS if PC.CASES[n].quant8]
        + [("fog_shadow", "", "in_bvh")] + [(n, v, "tail") for n, v in PC.TAIL_ROWS])


@pytest.mark.parametrize("name,variant,mode", RUNS, ids=["-".join(x for x in r if x) for r in RUNS])
def test_gpu_path_integral(g, ctx, name, variant, mode):
    c = PC.CASES[name]
    e = c.expected(g, variant)
    print(c.summary(g, variant))
    what = f"{name}[{variant}] {mode} GPU"
    try:
        ctx.set_node_format("quant8" if mode == "quant8" else "fp32")
        ctx.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_IN_BVH if mode == "in_bvh" else g.RT_VOLUMES_LIFTED)
        ctx.set_tail(1 << 30 if mode == "tail" else 0)      # every path left after bounce 0 goes to k_tail
        b, d, cam, ids = c.build(g, variant)
        ctx.upload(d)
        # the device's traced bits: cut rays never queued; with a lifted volume nor those the fog stops
        bits = "nee_lifted" if name == "fog_shadow" and mode != "in_bvh" else "nee_dev"
        if c.records(variant):
            for s in range(e["samples"]):
                for k in range(e["depth"]):
                    top, _, t, ray = ctx.extend_hits(cam, PC.SEED, s, k)
                    nee = ctx.shadow_visibility(cam, PC.SEED, s, k)
                    check_records(what, c, e, ids, s, k, top, t, ray, nee, "device", bits=bits)
        L, _ = ctx.render(cam, g.make_params(e["samples"], e["depth"], seed=PC.SEED))
        check_radiance(what, c, e, L, "device")
    finally:
        ctx.set_node_format("fp32")
        ctx.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_LIFTED)
        ctx.set_tail(0)
