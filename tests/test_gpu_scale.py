"""First hits, radiance and bounce records across scene scale and ray distance
(tests/scale_cases.py), through the C-ABI.  Marked gpu.

The same cells, views and assertions as tests/test_scale_host.py, on the
device, with fp32, quant8 and wide8 nodes and the SAH and the reference world
BVH, one context per parameter set.  The ids come from rt_extend_first_hits,
the production k_extend in the format's own variant (kQuant, kWide: the
kernel tests/hits_emu.cpp runs on the host), and again from rt_primary_hits,
the probe kernel, which has an fp32 and a quant8 variant and reads a wide8
scene's DNode4 nodes.  Per view
(scale_cases.check_view): ids equal to the fp64 oracle's (the Go arithmetic)
on every interior pixel, at most 2 % of the rays different at all, t equal to
the fp32 oracle's bit for bit wherever the ids agree with it; before that, on
the oracle alone (scale_cases.check_references): at most 25 % silhouette per
view and every primitive reached.

Past the camera ray, where a wall lost to bounce or shadow rays would show
(offset 0, the room camera, 32 x 32):
  * radiance at s = 1, 2^6, 2^10, 64 spp, depth 5, against the fp32 oracle to
    the fp32 bar of tests/test_gpu_parity.py (same paths: mse <= 1e-10), and
    against the fp64 oracle.  s = 1 is held to that file's fp64 bar (mse <=
    1e-4, |relative bias| <= 2e-3).  At 2^6 and 2^10 the fp32 ORACLE alone,
    with every primary id equal to the fp64 oracle's, is outside that bar
    (mse 2.691e-4 / bias -2.02e-2 and mse 7.211e-4 / bias -3.37e-2, measured on
    the CPU), so those scales are held to twice that.  What is
    left there is the reference's absolute ray offset tmin = 0.001: from
    coordinates of about 2^13 half an ulp of a hit point exceeds it and a
    secondary ray can hit the surface it starts on (of 654 shadow rays of
    sample 0, 647 are unoccluded in fp64, 643 in fp32 at 2^6, 642 at 2^10).
    fp32 resolution under the reference's constants, not a culled box;
  * one rt_extend_hits / oracle path_records pass at s = 2^6, bounces 0-4,
    with fp32 and with wide8 nodes (k_extend and k_shadow in both variants),
    with tests/test_gpu_paths.py's machinery and requirement: no id, t or
    shadow-ray mismatch on bit-identical rays.

These two found the second fp32 failure this file pins.  The reference ends an
area light's shadow ray at dist - 0.001 (camera.go:639), which in fp32 rounds
back to dist from dist >= 16384: the closed-interval quad test then took the
light as the occluder of its own shadow ray (372 of 653 shadow rays of sample
0 at 2^6; the fp32 oracle's bias against fp64 was -0.465 at 2^6 and -0.906 at
2^10), and with tmax == t of the light the device, which clips the light's
box to [tmin, tmax] first, and the oracle, which walks a world list, disagreed
at the last ulp on 6 of 2106 shadow rays.  The ray now ends at
min(dist - 0.001, dist * (1 - 2^-20)) on both sides (wavefront.hip,
oracle SHADOW_END): the same value below dist = 1048, at least 8 ulps short
of the light above.
"""
import numpy as np
import pytest

from tests import scale_cases as S
from tests.test_gpu_parity import FP64_BIAS, FP64_MSE, fp32_bar, fp64_bar
from tests.test_gpu_paths import compare_desc_paths

pytestmark = pytest.mark.gpu

CELLS = [(s, k) for s in S.SCALES for k in S.OFFSETS]
CELL_IDS = [S.cell_id(s, k) for s, k in CELLS]
FORMATS = ["fp32", "quant8", "wide8"]
TLAS = ["sah", "reference"]


@pytest.mark.parametrize("tlas", TLAS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("s,k", CELLS, ids=CELL_IDS)
def test_first_hits(g, O, s, k, fmt, tlas):
    room, refs = S.room(g, s, k), S.references(g, O, s, k)
    S.check_references(room, refs)
    c = g.Context(0)
    fails = []
    try:
        c.set_node_format(fmt)
        c.set_tlas_builder(tlas)
        c.upload(room.desc)
        assert c.info().node_format == {"fp32": g.RT_NODES_FP32, "quant8": g.RT_NODES_QUANT8, "wide8": g.RT_NODES_WIDE8}[fmt]
        for r in refs:
            # the production closest-hit kernel (k_extend: the kQuant / kWide variant of the format) and the
            # probe kernel (fp32 or quant8 nodes only: a wide8 scene's DNode4 copy)
            for what, hits in (("k_extend", c.extend_first_hits), ("probe", c.primary_hits)):
                top, prim, t = hits(r.view.cam, S.SEED, S.SAMPLE)
                msg = S.check_view(f"{what} {r.view.name}", r, top, prim, t)
                if msg:
                    fails.append(msg)
        c.sync()   # raises on a device error
    finally:
        c.close()
    assert not fails, f"{S.cell_id(s, k)} {fmt} {tlas}: {len(fails)} of {2 * len(refs)} (kernel, view) pairs fail:\n" + "\n".join(fails)


# s -> (mse, |relative bias|) of the fp32 oracle against the fp64 oracle at these settings, where it exceeds
# the existing bar with every primary id equal (measured on the CPU; the module docstring has the cause)
FP32_ORACLE_VS_FP64 = {2.0 ** 6: (2.691e-4, 2.02e-2), 2.0 ** 10: (7.211e-4, 3.37e-2)}
SPP = 64
RADIANCE_SCALES = [1.0, 2.0 ** 6, 2.0 ** 10]
RADIANCE_IDS = ["s2^0", "s2^6", "s2^10"]

_rendered = {}


def rendered(g, s):
    """(room, camera, params, the GPU's radiance sums) at scale s, rendered once."""
    if s not in _rendered:
        room = S.room(g, s, 0)
        cam = room.room_camera()
        p = g.make_params(SPP, cam.max_depth, seed=5)
        c = g.Context(0)
        try:
            c.upload(room.desc)
            gpu, _ = c.render(cam, p)
            c.sync()
        finally:
            c.close()
        assert np.isfinite(gpu).all() and gpu.sum() > 0
        gpu.setflags(write=False)
        _rendered[s] = (room, cam, p, gpu)
    return _rendered[s]


@pytest.mark.parametrize("s", RADIANCE_SCALES, ids=RADIANCE_IDS)
def test_radiance_vs_fp64_oracle(g, O, s):
    room, cam, p, gpu = rendered(g, s)
    mse_max, bias_max = FP64_MSE, FP64_BIAS
    if s in FP32_ORACLE_VS_FP64:
        mse_max, bias_max = (2.0 * x for x in FP32_ORACLE_VS_FP64[s])
    fp64_bar(f"room {S.cell_id(s, 0)}", gpu, O.render(room.desc, cam, p, fp32=False, threads=16), SPP, mse_max, bias_max)


@pytest.mark.parametrize("s", RADIANCE_SCALES, ids=RADIANCE_IDS)
def test_radiance_vs_fp32_oracle(g, O, s):
    room, cam, p, gpu = rendered(g, s)
    fp32_bar(f"room {S.cell_id(s, 0)}", gpu, O.render(room.desc, cam, p, fp32=True, threads=16), SPP)


_rows = {}
NODES = ["fp32", "wide8"]      # the formats tests/test_gpu_paths.py's machinery takes


def bounce_rows(g, O, nodes):
    if nodes not in _rows:
        room = S.room(g, 2.0 ** 6, 0)
        _rows[nodes] = compare_desc_paths(g, O, room.desc, room.room_camera(), (0,), bounces=5, nodes=nodes)
        for r in _rows[nodes]:
            print(f"room s2^6 {nodes} bounce {r['bounce']}: alive {r['alive']} compared {r['compared']} "
                  f"diverged {r['diverged']} shadow rays {r['shadow_rays']} hit mismatches {r['hit_mismatch']} "
                  f"NEE mismatches {r['nee_mismatch']} first {r['first_bad']}")
    return _rows[nodes]


@pytest.mark.parametrize("nodes", NODES)
def test_bounce_hits(g, O, nodes):
    rows = bounce_rows(g, O, nodes)
    assert [r["bounce"] for r in rows] == [0, 1, 2, 3, 4]
    for r in rows:
        assert r["compared"] > 0
        assert r["hit_mismatch"] == 0, f"bounce {r['bounce']}: {r['hit_mismatch']} hits differ, first {r['first_bad']}"
        assert r["diverged"] <= 2e-3 * max(r["alive"], 1), f"too many diverged paths {r}"


@pytest.mark.parametrize("nodes", NODES)
def test_bounce_shadow_rays(g, O, nodes):
    rows = bounce_rows(g, O, nodes)
    assert sum(r["shadow_rays"] for r in rows) > 1000
    for r in rows:
        assert r["nee_mismatch"] == 0, f"bounce {r['bounce']}: {r['nee_mismatch']} of {r['shadow_rays']} shadow rays differ, first {r['first_bad']}"
