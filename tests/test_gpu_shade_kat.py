"""The rows of tests/shade_cases.py (scattering, textures, environment, lens:
expected values from tests/shade_ref.py, float64 from the Go text alone)
through the GPU, via the C-ABI: the production k_extend's records
(rt_extend_hits at bounces 0 and 1) for the rays and the ended paths, the
production render at one sample per pixel for the radiance.  Every row runs
with the default options; glass_back, noise_albedo, image_inst and env_is run
with RT_NODES_QUANT8 as well.  A frame is at most 24 x 16 pixels.

Tolerances: those of tests/test_shade_kat.py (rays atol 1e-5, t rtol 2e-6,
branches, ended paths and image texels exact, the noise / env / nee groups
four times the fp32 oracle's measured error on the CPU)."""
import numpy as np
import pytest

from tests import shade_cases as S
from tests.test_shade_kat import RAY_ATOL, T_RTOL, check_radiance, has_paths

pytestmark = pytest.mark.gpu

RUNS = [(n, "fp32") for n in S.CASES] + [(n, "quant8") for n in S.CASES if S.CASES[n].quant8]


@pytest.mark.parametrize("name,nodes", RUNS, ids=[f"{n}-{f}" for n, f in RUNS])
def test_gpu_shading_closed_form(g, ctx, name, nodes):
    c = S.CASES[name]
    e = c.expected(g)
    print(c.summary(g))
    try:
        ctx.set_node_format(nodes)
        if has_paths(e):
            b, d, cam = c.build(g, c.variants[0])
            ctx.upload(d)
            top0, _, t0, ray0 = ctx.extend_hits(cam, S.SEED, c.sample, 0)
            top1, _, _, ray1 = ctx.extend_hits(cam, S.SEED, c.sample, 1)
            S.check_paths(c, e, (top0, t0, ray0), (top1, ray1), RAY_ATOL, T_RTOL)
        if "L" in e:
            for v in c.variants:
                b, d, cam = c.build(g, v)
                ctx.upload(d)
                L, _ = ctx.render(cam, g.make_params(1, e["L_depth"][v], seed=S.SEED, sample_offset=c.sample))
                check_radiance(f"{name}[{v}] {nodes} GPU", e, v, L, "device")
    finally:
        ctx.set_node_format("fp32")
