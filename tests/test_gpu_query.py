"""Ray queries (rt_trace_rays / rt_occluded) on the GPU, through the C-ABI.

  * replay: the rays rt_extend_hits reports for bounces 0-3 of one sample,
    traced again with tmin = 0.001, tmax = +inf, give rt_extend_hits' own top,
    prim and the bits of t on every live path: cornell-rotations (the
    reference-order mode), a reduced cornell-lucy (a mesh; its six walls
    lifted out of the BVH), `simple` (static spheres) and the scale room (the
    cap of eight lifted primitives, a sphere among them), under fp32, quant8
    and wide8 nodes, with RT_OPT_LIFT_PRIMS both ways;
  * the closed forms of tests/query_cases.py (interval ends, any-hit rule, hit
    record, moving sphere, invalid rays) through the C-ABI;
  * sizes at which the chunking can go wrong (1, 255, 256, 257; 3 * 256 + 5
    with one block) against one large call;
  * the spill path on the deepest chain of tests/stack_cases.py;
  * the _device variants on a non-default stream, bit-equal to the host ones;
  * the refusals.
`cornell` itself holds a fog volume: it is the scene rt_trace_rays must refuse
(RT_ERR_UNSUPPORTED), so its replay row is the refusal test, and the row that
must really lift is cornell-lucy.

Nothing here provokes a fault: the invalid rays are defined input that the
guard at the ray load turns into misses."""
import numpy as np
import pytest

from tests import path_cases as PC
from tests import query_cases as Q
from tests import scale_cases as S
from tests import stack_cases as SC

pytestmark = pytest.mark.gpu

SEED, SAMPLE, BOUNCES = 29, 0, 4
K_LDS_STACK = 8                        # wavefront.h kLdsStack
LUCY = dict(lucy_rings=30, lucy_cols=40)


def context(g, desc, nodes="fp32", lifted=True, tlas="sah", blas="sah", max_blocks=0):
    c = g.Context(0)
    c.set_lift_prims(lifted)
    c.set_node_format(nodes)
    c.set_tlas_builder(tlas)
    c.set_blas_builder(blas)
    if max_blocks:
        c.set_option(g.RT_OPT_MAX_BLOCKS, max_blocks)
    c.upload(desc)
    return c


def scene(g, name):
    """(desc, camera, keep-alive) of a replay row; frames 32 x 32."""
    if name == "room":
        r = S.room(g, 1.0, 0)
        return r.desc, r.room_camera(32), r
    s = g.Scene(name, width=32, aspect=1.0, **(LUCY if name == "cornell-lucy" else {}))
    return s.desc, s.camera, s


def replay(g, c, cam, what):
    """rt_extend_hits' rays of every bounce through trace_rays: the same ids and t bits.  Returns the rays traced."""
    traced = []
    for k in range(BOUNCES):
        top, prim, t, ray = c.extend_hits(cam, SEED, SAMPLE, k)
        live = np.flatnonzero(top != -2)
        if len(live) == 0:
            continue
        rays = g.make_rays(ray[live, 0:3], ray[live, 3:6], 0.001, float("inf"))
        h = c.trace_rays_raw(rays)
        tb, wb = h["t"].view(np.uint32), t[live].view(np.uint32)
        bad = (h["top"] != top[live]) | (h["prim"] != prim[live]) | (tb != wb)
        assert not bad.any(), f"{what} bounce {k}: {int(bad.sum())} of {len(live)} rays differ from rt_extend_hits, first " \
                              f"pixel {live[np.flatnonzero(bad)[0]]}: {h[np.flatnonzero(bad)[0]]} vs " \
                              f"{(top[live][bad][0], prim[live][bad][0], t[live][bad][0])}"
        hit = prim[live] >= 0
        assert np.array_equal(c.occluded(rays["o"], rays["d"]) != 0, hit), f"{what} bounce {k}: occluded differs from hitting"
        assert not (h["flags"] & Q.INVALID).any()
        traced.append(rays)
    assert len(traced) >= 2, f"{what}: no path went past bounce 0"
    return np.concatenate(traced)


LIFTS = {"cornell-rotations": 0, "cornell-lucy": 6, "simple": None, "room": 8}


@pytest.mark.parametrize("lifted", [True, False], ids=["lifted", "in-bvh"])
@pytest.mark.parametrize("nodes", ["fp32", "quant8", "wide8"])
@pytest.mark.parametrize("name", list(LIFTS))
def test_replay_equals_extend_hits(g, name, nodes, lifted):
    desc, cam, keep = scene(g, name)
    c = context(g, desc, nodes=nodes, lifted=lifted)
    try:
        n = c.lifted_prims()
        if not lifted:
            assert n == 0
        elif LIFTS[name] is not None:
            assert n == LIFTS[name], f"{name}: {n} primitives lifted"
        if name in ("cornell-lucy", "room") and lifted:
            assert n > 0                                  # the row really lifts
        replay(g, c, cam, f"{name} {nodes} {'lifted' if lifted else 'in-bvh'}")
        c.sync()                                          # raises on a device error
    finally:
        c.close()


# ------------------------------------------------------------------ closed forms
@pytest.fixture(params=[("fp32", True), ("quant8", True), ("wide8", True), ("fp32", False)],
                ids=lambda p: f"{p[0]}-{'lifted' if p[1] else 'in-bvh'}")
def trace(request, g):
    nodes, lifted = request.param
    made = []

    def f(desc, rays, time, any_hit):
        if not made or made[-1][0] is not desc:
            for _, c in made:
                c.close()
            made.clear()
            made.append((desc, context(g, desc, nodes=nodes, lifted=lifted)))
        c = made[-1][1]
        rays = np.ascontiguousarray(rays, g.RAY_DTYPE)
        out = c.occluded(rays["o"], rays["d"], rays["tmin"], rays["tmax"], time=time) if any_hit \
            else c.trace_rays_raw(rays, time)
        c.sync()                                          # no error flag was raised
        return out
    yield f
    for _, c in made:
        c.close()


def test_interval_and_any_hit_rule(g, trace):
    Q.check_intervals(g, trace)


def test_hit_record(g, trace):
    Q.check_records(g, trace)


def test_moving_sphere(g, trace):
    Q.check_moving(g, trace)


def test_invalid_rays(g, trace):
    Q.check_invalid(g, trace)


# ------------------------------------------------------------------------ sizes
@pytest.fixture(scope="module")
def lucy_rays(g):
    """cornell-lucy's replay rays and their hits from one large default call."""
    desc, cam, keep = scene(g, "cornell-lucy")
    c = context(g, desc)
    try:
        rays = replay(g, c, cam, "cornell-lucy")
        assert len(rays) > 3 * 256 + 5
        hits, occ = c.trace_rays_raw(rays), c.occluded(rays["o"], rays["d"])
    finally:
        c.close()
    for a in (rays, hits, occ):
        a.setflags(write=False)
    return desc, rays, hits, occ, keep


@pytest.mark.parametrize("n,max_blocks", [(1, 0), (255, 0), (256, 0), (257, 0), (3 * 256 + 5, 1)])
def test_chunk_sizes(g, lucy_rays, n, max_blocks):
    desc, rays, hits, occ, _ = lucy_rays
    c = context(g, desc, max_blocks=max_blocks)
    try:
        for off in (0, 300):                              # from the start and from the middle of the large call
            part = rays[off:off + n]
            assert c.trace_rays_raw(part).tobytes() == hits[off:off + n].tobytes(), f"n {n} at {off}"
            assert c.occluded(part["o"], part["d"]).tobytes() == occ[off:off + n].tobytes(), f"n {n} at {off}"
        assert len(c.trace_rays_raw(rays[:0])) == 0 and len(c.occluded(np.zeros((0, 3)), np.zeros((0, 3)))) == 0   # n == 0: RT_OK
        c.sync()
    finally:
        c.close()


# ------------------------------------------------------------------- spill path
def test_spill_path_on_the_deepest_chain(g):
    """chain_ref at its deepest accepted depth (stack_needed = the kernels'
    largest, far beyond the 8-entry LDS ring): rays that spill agree with
    rt_extend_hits."""
    case = SC.CASES["chain_ref"]
    b, desc, cam, ids = case.build(g, f"n{SC.EDGES['chain_ref']['accepted']}")
    c = context(g, desc, tlas="reference", blas="reference")
    try:
        assert c.info().stack_needed > K_LDS_STACK
        assert c.info().stack_needed == 128
        hit = 0
        for k in range(2):
            top, prim, t, ray = c.extend_hits(cam, PC.SEED, 0, k)
            live = np.flatnonzero(top != -2)
            rays = g.make_rays(ray[live, 0:3], ray[live, 3:6])
            h = c.trace_rays_raw(rays)
            assert np.array_equal(h["top"], top[live]) and np.array_equal(h["prim"], prim[live])
            assert np.array_equal(h["t"].view(np.uint32), t[live].view(np.uint32))
            assert np.array_equal(c.occluded(rays["o"], rays["d"]) != 0, prim[live] >= 0)
            hit += int((prim[live] >= 0).sum())
        assert hit > PC.N // 3
        # the rays do leave the ring: the render's counters over the same camera rays
        assert c.count_work(cam, g.make_params(1, 1, seed=PC.SEED))["stack_spills"] > 0
        c.sync()
    finally:
        c.close()


# -------------------------------------------------------------- device variants
def test_device_variants_on_a_stream(g, lucy_rays):
    import torch
    desc, rays, hits, occ, _ = lucy_rays
    c = context(g, desc)
    try:
        n = len(rays)
        st = torch.cuda.Stream(device=0)
        with torch.cuda.stream(st):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(n, 8).copy()).to("cuda:0", non_blocking=False)
            d_hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
            d_occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            c.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=st.cuda_stream)
            c.occluded_device(d_rays.data_ptr(), n, d_occ.data_ptr(), stream=st.cuda_stream)
            # a second pair on the default stream right behind it: the calls share the context's spill area
            d_hits2 = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
        c.trace_rays_device(d_rays.data_ptr(), n, d_hits2.data_ptr(), stream=torch.cuda.default_stream(0).cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        c.sync()
        assert d_hits.cpu().numpy().tobytes() == hits.tobytes()
        assert d_hits2.cpu().numpy().tobytes() == hits.tobytes()
        assert d_occ.cpu().numpy().tobytes() == occ.tobytes()
    finally:
        c.close()


# --------------------------------------------------------------------- refusals
def test_refusals(g):
    s = g.Scene("cornell", width=32, aspect=1.0)          # holds a fog volume
    o, d = np.zeros((2, 3), np.float32), np.array([[0, 0, -1], [0, 1, 0]], np.float32)
    c = g.Context(0)
    try:
        for call in (lambda: c.trace_rays(o, d), lambda: c.occluded(o, d)):
            with pytest.raises(g.RTError) as ex:
                call()
            assert ex.value.code == -5                    # RT_ERR_NO_SCENE
        c.upload(s.desc)
        assert c.info().volumes > 0
        for call in (lambda: c.trace_rays(o, d), lambda: c.occluded(o, d),
                     lambda: c.trace_rays_device(16, 1, 16), lambda: c.occluded_device(16, 1, 16)):
            with pytest.raises(g.RTError) as ex:
                call()
            assert ex.value.code == -2                    # RT_ERR_UNSUPPORTED
        lib = g.rtgpu()
        ray, hit = g.RtRay(), g.RtRayHit()
        import ctypes as C
        assert lib.rt_trace_rays(c._h, None, 1, 0.0, C.byref(hit)) == -1
        assert lib.rt_trace_rays(c._h, C.byref(ray), -1, 0.0, C.byref(hit)) == -1
        assert lib.rt_occluded(c._h, C.byref(ray), 1, 0.0, None) == -1
    finally:
        c.close()
