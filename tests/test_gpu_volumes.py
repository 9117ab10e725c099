"""Volume.Hit across boundary kinds, placements and fallbacks, on the GPU: the
rows of tests/volume_cases.py (tests/test_volume_host.py holds the flattener to
each row's declared placement and runs the same kernels on the host).

Per row, with RT_VOLUMES_LIFTED where the row's volumes are lifted and with
RT_VOLUMES_IN_BVH always:
  * every bounce up to the camera's depth 5 against the fp32 oracle
    (test_gpu_paths.compare_desc_paths): no hit (ids, t bit for bit) and no
    NEE mismatch on any path whose incoming ray is the oracle's, diverged
    paths within test_gpu_paths' 2e-3 share; where the volumes are in the
    world BVH every shadow ray is traced, so the traced flags must equal the
    oracle's too;
  * the radiance of 8 samples within test_gpu_parity.fp32_bar;
  * for the four analytic rows, rt_extend_hits at bounce 0 against the closed
    form (ids exactly, t within volume_cases.T_RTOL on the decided pixels).
box_uv, sphere and vol9 also run with quant8 and wide8 nodes (a scene with a
volume in the world BVH takes fp32 nodes when asked for wide8, and says so).

`disc_capped` / `disc_capped8` (boundaries holding circles) fail without
volume_hit's circle branch."""
import numpy as np
import pytest

from tests import volume_cases as V
from tests.test_gpu_parity import fp32_bar
from tests.test_gpu_paths import IN_BVH, LIFTED, compare_desc_paths

pytestmark = pytest.mark.gpu

MAX_DIVERGED = 2e-3       # test_gpu_paths' share, per bounce
SPP = 8

RUNS = [(n, p, "fp32") for n in V.NAMES for p in (["lifted", "in_bvh"] if n in
        ("box_uv", "box_vu", "sheared", "box_srt", "inside", "leaf2", "vol8") else ["in_bvh"])]
RUNS += [(n, p, f) for n in V.NODE_FORMAT_CASES for f in ("quant8", "wide8")
         for p in (["lifted", "in_bvh"] if n == "box_uv" else ["in_bvh"])]


def test_runs_cover_every_placement(g):
    """The parametrisation above names the lifted rows by hand (pytest needs
    it before a case can be built): it must be what the cases declare."""
    for n in V.NAMES:
        assert [p for m, p, f in RUNS if m == n and f == "fp32"] == V.case(g, n).placements()


@pytest.mark.parametrize("name,place,nodes", RUNS, ids=[f"{n}-{p}-{f}" for n, p, f in RUNS])
def test_volume_paths_radiance_and_closed_form(g, O, ctx, name, place, nodes):
    c = V.case(g, name)
    in_bvh = place == "in_bvh"
    # 8-wide nodes only without a volume in the world BVH
    taken = "fp32" if nodes == "wide8" and in_bvh else nodes
    rows = compare_desc_paths(g, O, c.desc, c.cam, (0,), 0, IN_BVH if in_bvh else LIFTED, nodes, nodes_taken=taken,
                              every_shadow_ray=in_bvh)
    for r in rows:
        print(f"{name} {place} {nodes} bounce {r['bounce']}: alive {r['alive']} compared {r['compared']} diverged "
              f"{r['diverged']} shadow rays {r['shadow_rays']} hit mismatches {r['hit_mismatch']} NEE mismatches "
              f"{r['nee_mismatch']}")
    assert [r["bounce"] for r in rows] == list(range(c.cam.max_depth))
    assert sum(r["shadow_rays"] for r in rows) > 0
    for r in rows:
        assert r["compared"] > 0
        assert r["hit_mismatch"] == 0 and r["nee_mismatch"] == 0, f"{name} {place} {nodes}: {r}"
        assert r["diverged"] <= MAX_DIVERGED * max(r["alive"], 1), f"{name} {place} {nodes}: diverged paths {r}"

    try:
        ctx.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_IN_BVH if in_bvh else g.RT_VOLUMES_LIFTED)
        ctx.set_node_format(nodes)
        ctx.upload(c.desc)
        p = g.make_params(SPP, c.cam.max_depth, seed=V.SEED)
        gpu, _ = ctx.render(c.cam, p)
        fp32_bar(f"volume {name} {place} {nodes}", gpu, O.render(c.desc, c.cam, p, fp32=True, threads=16), SPP)
        if c.analytic:
            top, prim, t, ray = ctx.extend_hits(c.cam, V.SEED, V.SAMPLE, 0)
            o, d = V.camera_rays(O, c)
            assert np.array_equal(ray.astype(np.float64), np.hstack([o, d]))      # the closed form's input rays
            wp, wt, decided = V.expected(c, o, d)
            assert np.array_equal(prim[decided], wp[decided])
            assert np.array_equal(top[decided], wp[decided])                       # world-level objects both
            rel = np.abs(t[decided].astype(np.float64) - wt[decided]) / wt[decided]
            print(f"{name} {place} {nodes}: worst relative t error against the closed form {rel.max():.3e}")
            assert rel.max() <= V.T_RTOL[name]
    finally:
        ctx.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_LIFTED)
        ctx.set_node_format("fp32")
