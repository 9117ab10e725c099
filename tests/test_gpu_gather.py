"""rt_gather on the GPU, through the C-ABI.

  * the equality that defines it: rt_ray_color over rt_gather_rays(.., s) with
    samples = 1, sample_offset = s is rt_gather with samples = 1,
    sample_offset = s, all bytes, for every source: a reduced cornell-lucy
    (fp32, quant8 and wide8 nodes, walls lifted and in the BVH; surface points
    taken from rt_trace_rays hits), cornell (fog, lifted and in the BVH),
    hdri-nee, and random with the long-tail kernel automatic and off;
  * RT_GATHER_RAY is rt_ray_color on the same bytes;
  * the device probe's rays equal tests/gather_ref.py, all bytes;
  * sums over samples and calls, cuts of the array, schedules, ids, invalid
    points, the _device variant on a stream, the refusals;
  * an open sky in closed form: a hemisphere that cannot reach the scene's one
    sphere gathers exactly samples * background.

Nothing here provokes a fault: the invalid points are defined input that the
guard at the point load turns into zeros."""
import ctypes as C

import numpy as np
import pytest

from tests import gather_ref as GR
from tests.scene_builder import Builder
from tests.test_gather_host import hard_points

pytestmark = pytest.mark.gpu

SEED = 29
LUCY = dict(lucy_rings=30, lucy_cols=40)
N = 3 * 256 + 5
SOURCES = (GR.RAY, GR.COSINE, GR.SPHERE)


def scene(g, name):
    return g.Scene(name, width=32, aspect=1.0, **(LUCY if name == "cornell-lucy" else {}))


def context(g, desc, nodes="fp32", lifted=True, volumes_in_bvh=False, tail=0, **schedule):
    c = g.Context(0)
    c.set_lift_prims(lifted)
    c.set_node_format(nodes)
    c.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_IN_BVH if volumes_in_bvh else g.RT_VOLUMES_LIFTED)
    if schedule:
        c.set_schedule(**schedule)
    c.set_tail(tail)
    c.upload(desc)
    return c


def surface_points(g, c, cam):
    """N points on the surfaces the camera sees (rt_trace_rays hits of sample
    0's camera rays: p = o + t d, n = the hit normal); a miss becomes a fixed
    point inside the box."""
    _, _, _, ray = c.extend_hits(cam, SEED, 0, 0)
    o, d = ray[100:100 + N, 0:3], ray[100:100 + N, 3:6]
    top, prim, t, mat, n, flags = c.trace_rays(o, d)
    hit = top >= 0
    assert hit.sum() > N // 2
    p = (o + t[:, None] * d).astype(np.float32)
    p[~hit] = (278.0, 278.0, 278.0)
    n = n.copy()
    n[~hit] = (0.0, 0.0, 1.0)
    return g.make_gather_points(p, n, ids=np.arange(N) + 1000)


def free_points(g, c, cam):
    """N points a little in front of what the camera rays hit (scenes whose
    volumes rt_trace_rays refuses, or without walls), looking back along the
    ray with normals that are not unit."""
    top, prim, t, ray = c.extend_hits(cam, SEED, 0, 0)
    sl = slice(100, 100 + N)
    o, d, t = ray[sl, 0:3], ray[sl, 3:6], t[sl]
    step = np.where((top[sl] >= 0) & np.isfinite(t), np.float32(0.98) * t, np.float32(1.0)).astype(np.float32)
    return g.make_gather_points(o + step[:, None] * d, -d * (0.5 + 0.25 * (np.arange(N) % 13))[:, None],
                                ids=np.arange(N) + 1000)


def check_defining_equality(g, c, pts, cam, depth, what):
    lit = 0
    for source in SOURCES:
        for s in (0, 1):
            rays = c.gather_rays(pts, source, seed=SEED, sample=s)
            assert rays.tobytes() == GR.rays(pts, source, SEED, s).tobytes(), f"{what}: the probe, source {source} sample {s}"
            want, _ = c.ray_color(rays, 1, depth, seed=SEED, sample_offset=s, camera=cam)
            got, st = c.gather(pts, source, 1, depth, seed=SEED, sample_offset=s, camera=cam)
            assert st.invalid_rays == 0 and st.samples == len(pts)
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
            assert len(bad) == 0, f"{what} source {source} sample {s}: {len(bad)} of {len(pts)} points differ from " \
                                  f"rt_ray_color, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
            assert np.isfinite(got).all()
            lit += int((got > 0).any())
    assert lit == 6, f"{what}: an empty result shows nothing"
    c.sync()                                              # raises on a device error


EQUAL = [
    ("cornell-lucy", dict(nodes="fp32")), ("cornell-lucy", dict(nodes="quant8")), ("cornell-lucy", dict(nodes="wide8")),
    ("cornell-lucy", dict(nodes="fp32", lifted=False)), ("cornell-lucy", dict(nodes="quant8", lifted=False)),
    ("cornell-lucy", dict(nodes="wide8", lifted=False)),
    ("cornell", dict()), ("cornell", dict(volumes_in_bvh=True)), ("hdri-nee", dict()),
    ("random", dict(tail=0)), ("random", dict(tail=1)),
]


@pytest.mark.parametrize("name,opts", EQUAL, ids=[n + "".join(f"-{k}={v}" for k, v in o.items()) for n, o in EQUAL])
def test_gather_equals_ray_color_over_the_probe(g, name, opts):
    s = scene(g, name)
    c = context(g, s.desc, **opts)
    try:
        if name == "cornell":
            assert c.info().volumes > 0
        if name == "cornell-lucy":
            assert (c.lifted_prims() > 0) == opts.get("lifted", True)
            pts = surface_points(g, c, s.camera)
        else:
            pts = free_points(g, c, s.camera)
        check_defining_equality(g, c, pts, s.camera, s.camera.max_depth, f"{name} {opts}")
    finally:
        c.close()


# ------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def lucy(g):
    """The reduced cornell-lucy, N surface points, and their 4-sample COSINE
    sums from one default call."""
    s = scene(g, "cornell-lucy")
    c = context(g, s.desc)
    try:
        pts = surface_points(g, c, s.camera)
        depth = s.camera.max_depth
        rgb, st = c.gather(pts, GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
        assert st.samples == 4 * N and st.invalid_rays == 0
        c.sync()
    finally:
        c.close()
    for a in (pts, rgb):
        a.setflags(write=False)
    assert np.isfinite(rgb).all() and (rgb > 0).any()
    return s, pts, depth, rgb


def test_ray_source_is_ray_color_on_the_same_bytes(g, lucy):
    s, pts, depth, _ = lucy
    c = context(g, s.desc)
    try:
        got, _ = c.gather(pts, GR.RAY, 4, depth, seed=SEED, camera=s.camera)
        want, _ = c.ray_color(pts.view(g.PATH_RAY_DTYPE), 4, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == want.tobytes() and (got > 0).any()
        c.sync()
    finally:
        c.close()


def test_device_probe_equals_the_restatement(g):
    pts = hard_points()
    c = g.Context(0)                                      # no scene uploaded
    try:
        for source in SOURCES:
            for s in (0, 1, 7):
                assert c.gather_rays(pts, source, seed=77, sample=s).tobytes() == GR.rays(pts, source, 77, s).tobytes(), \
                    (source, s)
        assert c.gather_rays(pts[:0], GR.COSINE).shape == (0,)
    finally:
        c.close()


def test_sums_over_samples_and_calls(g, lucy):
    s, pts, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        one = [c.gather(pts, GR.COSINE, 1, depth, seed=SEED, sample_offset=k, camera=s.camera)[0] for k in range(4)]
        tot = np.zeros(rgb4.shape, np.float64)
        for a in one:                                     # fp64, in sample order, rounded once
            tot = tot + a.astype(np.float64)
        assert tot.astype(np.float32).tobytes() == rgb4.tobytes()
        assert all(a.tobytes() != one[0].tobytes() for a in one[1:])      # every sample has its own directions
        first, _ = c.gather(pts, GR.COSINE, 2, depth, seed=SEED, sample_offset=0, camera=s.camera)
        assert first.tobytes() == (one[0].astype(np.float64) + one[1].astype(np.float64)).astype(np.float32).tobytes()
        both, _ = c.gather(pts, GR.COSINE, 2, depth, seed=SEED, sample_offset=2, camera=s.camera, accum=first.copy())
        want = ((one[2].astype(np.float64) + one[3].astype(np.float64)) + first.astype(np.float64)).astype(np.float32)
        assert both.tobytes() == want.tobytes()
        c.sync()
    finally:
        c.close()


@pytest.mark.parametrize("k", range(5), ids=["slots-1", "slots-2n+3", "streams-1", "streams-3", "max-blocks-1"])
def test_cuts_and_schedules(g, lucy, k):
    s, pts, depth, rgb4 = lucy
    sched = [dict(batch_slots=1), dict(batch_slots=2 * N + 3), dict(streams=1), dict(streams=3), dict(max_blocks=1)][k]
    c = context(g, s.desc, **sched)
    try:
        got, _ = c.gather(pts, GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == rgb4.tobytes(), sched
        c.sync()
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_chunk_sizes(g, lucy, n):
    s, pts, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        for off in (0, 300):
            got, _ = c.gather(pts[off:off + n], GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
            assert got.tobytes() == rgb4[off:off + n].tobytes(), f"n {n} at {off}"
        got, st = c.gather(pts[:0], GR.COSINE, 4, depth, seed=SEED, camera=s.camera)       # n == 0: RT_OK
        assert got.shape == (0, 3) and st.samples == 0
        c.sync()
    finally:
        c.close()


def test_ids(g, lucy):
    s, pts, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        perm = np.random.default_rng(5).permutation(N)
        got, _ = c.gather(pts[perm], GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == rgb4[perm].tobytes()      # the id travels with the point; the slot is where it lies
        k = int(np.argmax(rgb4.sum(axis=1)))
        trio = np.repeat(pts[k:k + 1], 3)
        trio["id"][2] = trio["id"][0] + 12345
        got, _ = c.gather(trio, GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
        assert got[0].tobytes() == got[1].tobytes() == rgb4[k].tobytes()      # duplicate ids: the same paths
        assert got[2].tobytes() != got[0].tobytes()
        c.sync()
    finally:
        c.close()


def test_invalid_points(g, lucy):
    s, pts, depth, rgb4 = lucy
    n = 300
    where = [0, 63, 64, 255, 256, n - 1]
    bad = np.array(pts[:n])
    bad["p"][0, 1] = np.nan
    bad["p"][63, 0] = np.inf
    bad["n"][64] = 0.0
    bad["n"][255] = (1e-30, 0.0, 0.0)                     # its fp32 length is 0
    bad["n"][256, 0] = np.nan
    bad["p"][n - 1, 2] = -np.inf
    c = context(g, s.desc)
    try:
        got, st = c.gather(bad, GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 6
        assert not got[where].any()
        keep = np.setdiff1d(np.arange(n), where)
        assert got[keep].tobytes() == rgb4[:n][keep].tobytes()
        assert rgb4[:n][where].any()                      # those points did gather light
        # SPHERE does not read n: only the three bad positions are invalid
        clean, _ = c.gather(pts[:n], GR.SPHERE, 4, depth, seed=SEED, camera=s.camera)
        got, st = c.gather(bad, GR.SPHERE, 4, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 3 and not got[[0, 63, n - 1]].any()
        keep_sphere = np.setdiff1d(np.arange(n), [0, 63, n - 1])
        assert got[keep_sphere].tobytes() == clean[keep_sphere].tobytes()
        # the probe marks them so that rt_ray_color leaves them out too
        rays = c.gather_rays(bad, GR.COSINE, seed=SEED, sample=0)
        assert not rays["d"][where].any() and rays["d"][keep].any(axis=1).all()
        _, st = c.ray_color(rays, 1, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 6
        c.sync()
    finally:
        c.close()


def test_device_variant_on_a_stream(g, lucy):
    import torch
    s, pts, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        p = g.gather_params(GR.COSINE, 4, depth, seed=SEED, camera=s.camera)
        st = torch.cuda.Stream(device=0)
        with torch.cuda.stream(st):
            d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint32).reshape(N, 8).view(np.int32).copy()).to("cuda:0")
            d_rgb = torch.full((N, 3), 7.0, dtype=torch.float32, device="cuda:0")
            d_rgb2 = torch.full((N, 3), 7.0, dtype=torch.float32, device="cuda:0")
            c.gather_device(d_pts.data_ptr(), N, p, d_rgb.data_ptr(), stream=st.cuda_stream)
        # a second call on the default stream right behind it: the calls share the context's batch buffers
        c.gather_device(d_pts.data_ptr(), N, p, d_rgb2.data_ptr(), stream=torch.cuda.default_stream(0).cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        c.sync()
        assert c.last_render_kernel_ms() > 0.0
        assert d_rgb.cpu().numpy().tobytes() == rgb4.tobytes()
        assert d_rgb2.cpu().numpy().tobytes() == rgb4.tobytes()
    finally:
        c.close()


def test_open_sky_in_closed_form(g):
    """One sphere far below the plane y = 0, a constant background and no sky
    gradient: every direction of the cosine hemisphere about (0, 1, 0) has
    d.y >= 0 and leaves the scene, so each sample is exactly float(B) and the
    sum of four equal floats is exact."""
    B = (0.25, 0.5, 0.75)
    b = Builder(g)
    desc = b.desc(b.listing([b.sphere((0, -50, 0), 1.0, b.lambertian((0.5, 0.5, 0.5)))]))
    rng = np.random.default_rng(2)
    p = np.zeros((N, 3), np.float32)
    p[:, 0], p[:, 2] = rng.uniform(-100, 100, N), rng.uniform(-100, 100, N)
    pts = g.make_gather_points(p, np.tile(np.float32([0, 1, 0]), (N, 1)))
    c = g.Context(0)
    try:
        c.upload(desc)
        rgb, st = c.gather(pts, GR.COSINE, 4, 8, seed=SEED, background=B, use_sky_gradient=0)
        assert st.invalid_rays == 0
        assert rgb.tobytes() == np.tile(4 * np.float32(B), (N, 1)).tobytes()
        c.sync()
    finally:
        c.close()


def test_refusals(g):
    s = scene(g, "cornell")
    pts = g.make_gather_points(np.full((2, 3), 278.0), np.array([[0, 0, 1], [0, 1, 0]]))
    lib = g.rtgpu()
    c = g.Context(0)
    try:
        assert c.gather_rays(pts, GR.COSINE, seed=SEED).tobytes() == GR.rays(pts, GR.COSINE, SEED, 0).tobytes()   # before any upload
        with pytest.raises(g.RTError) as ex:
            c.gather(pts, GR.COSINE, 1, 2)
        assert ex.value.code == -5                        # RT_ERR_NO_SCENE
        c.upload(s.desc)
        rgb, _ = c.gather(pts, GR.COSINE, 1, 2, camera=s.camera)
        assert np.isfinite(rgb).all()
        pp = pts.ctypes.data_as(C.POINTER(g.RtGatherPoint))
        op = rgb.ctypes.data_as(C.POINTER(C.c_float))

        def status(n=2, pts_p=pp, rgb_p=op, source=GR.COSINE, reserved=0, **over):
            p = g.gather_params(source, 1, 2)
            p.reserved = reserved
            for k, v in over.items():
                if k == "background":
                    p.path.background[0] = v
                else:
                    setattr(p.path, k, v)
            return lib.rt_gather(c._h, pts_p, n, C.byref(p), rgb_p, None)

        assert status() == 0 and status(n=0) == 0
        assert status(pts_p=None) == -1 and status(rgb_p=None) == -1
        assert lib.rt_gather(c._h, pp, 2, None, op, None) == -1
        assert status(source=3) == -1 and status(source=-1) == -1 and status(reserved=1) == -1
        assert status(n=-1) == -1 and status(n=1 << 31) == -1
        for over in (dict(samples=0), dict(max_depth=0), dict(sample_offset=-1), dict(camera_max_depth=-1),
                     dict(background=float("nan")), dict(background=float("inf"))):
            assert status(**over) == -1, over
        marked = pts.copy()
        marked["reserved"][1] = 1
        assert status(pts_p=marked.ctypes.data_as(C.POINTER(g.RtGatherPoint))) == -1
        out = np.zeros(2, g.PATH_RAY_DTYPE)
        rp = out.ctypes.data_as(C.POINTER(g.RtPathRay))
        assert lib.rt_gather_rays(c._h, pp, 2, GR.COSINE, SEED, 0, rp) == 0
        assert lib.rt_gather_rays(c._h, pp, 2, GR.COSINE, SEED, -1, rp) == -1
        assert lib.rt_gather_rays(c._h, pp, 2, 3, SEED, 0, rp) == -1
        assert lib.rt_gather_rays(c._h, pp, -1, GR.COSINE, SEED, 0, rp) == -1
        assert lib.rt_gather_rays(c._h, None, 2, GR.COSINE, SEED, 0, rp) == -1
        assert lib.rt_gather_rays(c._h, pp, 2, GR.COSINE, SEED, 0, None) == -1
        p = g.gather_params(GR.COSINE, 1, 2)
        assert lib.rt_gather_device(c._h, None, 1, C.byref(p), C.c_void_p(16), None) == -1
        assert lib.rt_gather_device(c._h, C.c_void_p(16), 1, C.byref(p), None, None) == -1
        assert lib.rt_gather_device(c._h, C.c_void_p(16), 0, C.byref(p), C.c_void_p(16), None) == 0
        p.source = 3
        assert lib.rt_gather_device(c._h, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
        p.source, p.reserved = GR.SPHERE, 2
        assert lib.rt_gather_device(c._h, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
        c.sync()
    finally:
        c.close()
