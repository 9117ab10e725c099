"""rt_ray_color on the GPU, through the C-ABI.

  * replay: the rays rt_extend_hits reports at bounce 0 of sample s (GetRay's
    rays), given back with id = pixel, samples = 1, sample_offset = s and the
    camera's background / sky / phantom / depth fields, give the frame
    rt_render writes for that sample, bit for bit: cornell (fog, lifted and
    in the BVH), cornell-smoke, a reduced cornell-lucy (fp32, quant8 and
    wide8 nodes, walls lifted and in the BVH), cornell-rotations, hdri-nee,
    hdri-test at its depth 20, random at its depth 50 with the long-tail
    kernel automatic, off, and taking every path after bounce 0, and the
    bounce overlap;
  * the rows of tests/ray_color_cases.py (ray sets no camera produces) against
    their float64 expectation at the device bar of tests/test_ray_color_kat.py;
  * sums over samples and calls, cuts of the ray array, schedules, ids,
    invalid rays, the _device variant on a stream, the refusals.

Nothing here provokes a fault: the invalid rays are defined input that the
guard at the ray load turns into zeros."""
import ctypes as C

import numpy as np
import pytest

from tests import path_cases as PC
from tests import ray_color_cases as RC
from tests import test_ray_color_kat as RK

pytestmark = pytest.mark.gpu

SEED = 29
LUCY = dict(lucy_rings=30, lucy_cols=40)


def scene(g, name):
    return g.Scene(name, width=32, aspect=1.0, **(LUCY if name == "cornell-lucy" else {}))


def context(g, desc, nodes="fp32", lifted=True, volumes_in_bvh=False, tail=0, overlap=0, **schedule):
    c = g.Context(0)
    c.set_lift_prims(lifted)
    c.set_node_format(nodes)
    c.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_IN_BVH if volumes_in_bvh else g.RT_VOLUMES_LIFTED)
    if schedule:
        c.set_schedule(**schedule)
    c.set_tail(tail)
    c.set_overlap(overlap)
    c.upload(desc)
    return c


def camera_rays(g, c, cam, s, seed=SEED):
    """GetRay's float rays of sample s, as rt_path_ray with id = pixel."""
    top, prim, t, ray = c.extend_hits(cam, seed, s, 0)
    assert (top != -2).all()
    return g.make_path_rays(ray[:, 0:3], ray[:, 3:6])


def replay(g, c, cam, what, depth=None):
    depth = depth or cam.max_depth
    for s in (0, 1):
        rays = camera_rays(g, c, cam, s)
        frame, _ = c.render(cam, g.make_params(1, depth, seed=SEED, sample_offset=s))
        rgb, st = c.ray_color(rays, 1, depth, seed=SEED, sample_offset=s, camera=cam)
        assert st.invalid_rays == 0 and st.samples == len(rays)
        want = frame.reshape(-1, 3)
        bad = np.flatnonzero((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, f"{what} sample {s}: {len(bad)} of {len(rays)} rays differ from rt_render, first pixel " \
                              f"{bad[0]}: {rgb[bad[0]]} vs {want[bad[0]]}"
        assert np.isfinite(rgb).all() and rgb.any(), f"{what}: an empty frame shows nothing"
    c.sync()                                              # raises on a device error


REPLAYS = [
    ("cornell", dict()), ("cornell", dict(volumes_in_bvh=True)), ("cornell-smoke", dict()),
    ("cornell-lucy", dict(nodes="fp32")), ("cornell-lucy", dict(nodes="quant8")), ("cornell-lucy", dict(nodes="wide8")),
    ("cornell-lucy", dict(nodes="fp32", lifted=False)), ("cornell-lucy", dict(nodes="quant8", lifted=False)),
    ("cornell-lucy", dict(nodes="wide8", lifted=False)),
    ("cornell-rotations", dict()), ("hdri-nee", dict()), ("hdri-test", dict()),
    ("random", dict(tail=0)), ("random", dict(tail=1)), ("random", dict(tail=1 << 30)),
    ("cornell-lucy", dict(overlap=2)),
]


@pytest.mark.parametrize("name,opts", REPLAYS, ids=[n + "".join(f"-{k}={v}" for k, v in o.items()) for n, o in REPLAYS])
def test_replay_equals_the_render(g, name, opts):
    s = scene(g, name)
    c = context(g, s.desc, **opts)
    try:
        if name == "cornell":
            assert c.info().volumes > 0                   # the scene every other ray entry point refuses
        if name == "cornell-lucy":
            assert (c.lifted_prims() > 0) == opts.get("lifted", True)
        if name == "hdri-test":
            assert s.camera.max_depth == 20
        if name == "random":
            assert s.camera.max_depth == 50
        replay(g, c, s.camera, f"{name} {opts}")
    finally:
        c.close()


# ------------------------------------------------------------ rays no camera makes
KAT = [(n, v, False) for n, v in RC.ROWS] + [("fog_shadow", "", True)]


@pytest.mark.parametrize("name,variant,in_bvh", KAT, ids=[f"{n}-{v}" if v else n for n, v, _ in KAT[:-1]] + ["fog_shadow-in_bvh"])
def test_ray_sets_against_float64(g, name, variant, in_bvh):
    case = PC.CASES[name]
    b, desc, cam, ids = case.build(g, variant)
    c = context(g, desc, volumes_in_bvh=in_bvh)
    try:
        for rset in RC.SETS:
            e = RC.expected(name, variant, rset)
            print(RC.summary(name, variant, rset))
            o, d = RC.ray_set(rset)
            rgb, _ = c.ray_color(g.make_path_rays(o, d, RC.IDS), RC.SAMPLES, e["depth"], seed=RC.SEED, camera=cam)
            RK.check_radiance(f"{name}[{variant}] {rset} GPU{' in_bvh' if in_bvh else ''}", case, e, rgb, "device")
        c.sync()
    finally:
        c.close()


# ------------------------------------------------------------------------- sums
@pytest.fixture(scope="module")
def lucy(g):
    """The reduced cornell-lucy, n = 3 * 256 + 5 of its camera rays, and their
    4-sample sums from one default call."""
    s = scene(g, "cornell-lucy")
    c = context(g, s.desc)
    try:
        rays = camera_rays(g, c, s.camera, 0)[100:100 + 3 * 256 + 5].copy()
        depth = s.camera.max_depth
        rgb, _ = c.ray_color(rays, 4, depth, seed=SEED, camera=s.camera)
        c.sync()
    finally:
        c.close()
    for a in (rays, rgb):
        a.setflags(write=False)
    assert np.isfinite(rgb).all() and (rgb > 0).any()
    return s, rays, depth, rgb


def test_sums_over_samples_and_calls(g, lucy):
    s, rays, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        one = [c.ray_color(rays, 1, depth, seed=SEED, sample_offset=k, camera=s.camera)[0] for k in range(4)]
        tot = np.zeros(rgb4.shape, np.float64)
        for a in one:                                     # fp64, in sample order, rounded once
            tot = tot + a.astype(np.float64)
        assert tot.astype(np.float32).tobytes() == rgb4.tobytes()
        assert any(a.tobytes() != one[0].tobytes() for a in one[1:])      # the samples differ
        # accumulate: two 2-sample calls; the second adds double(previous) to its own fp64 sum
        first, _ = c.ray_color(rays, 2, depth, seed=SEED, sample_offset=0, camera=s.camera)
        assert first.tobytes() == (one[0].astype(np.float64) + one[1].astype(np.float64)).astype(np.float32).tobytes()
        acc = first.copy()
        both, _ = c.ray_color(rays, 2, depth, seed=SEED, sample_offset=2, camera=s.camera, accum=acc)
        want = ((one[2].astype(np.float64) + one[3].astype(np.float64)) + first.astype(np.float64)).astype(np.float32)
        assert both.tobytes() == want.tobytes()
        c.sync()
    finally:
        c.close()


# ----------------------------------------------------------- cuts and schedules
def _slots_cases(n):
    return [dict(batch_slots=1), dict(batch_slots=2 * n + 3), dict(streams=1), dict(streams=3), dict(max_blocks=1)]


@pytest.mark.parametrize("k", range(5), ids=["slots-below-n", "slots-between-n-and-4n", "streams-1", "streams-3", "max-blocks-1"])
def test_cuts_and_schedules(g, lucy, k):
    s, rays, depth, rgb4 = lucy
    n = len(rays)
    assert n == 3 * 256 + 5
    sched = _slots_cases(n)[k]
    assert k != 1 or n < sched["batch_slots"] < 4 * n
    c = context(g, s.desc, **sched)
    try:
        got, _ = c.ray_color(rays, 4, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == rgb4.tobytes(), sched
        c.sync()
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_chunk_sizes(g, lucy, n):
    s, rays, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        for off in (0, 300):                              # from the start and from the middle of the large call
            got, _ = c.ray_color(rays[off:off + n], 4, depth, seed=SEED, camera=s.camera)
            assert got.tobytes() == rgb4[off:off + n].tobytes(), f"n {n} at {off}"
        got, st = c.ray_color(rays[:0], 4, depth, seed=SEED, camera=s.camera)       # n == 0: RT_OK
        assert got.shape == (0, 3) and st.samples == 0
        c.sync()
    finally:
        c.close()


# -------------------------------------------------------------------------- ids
def test_ids(g, lucy):
    s, rays, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        perm = np.random.default_rng(5).permutation(len(rays))
        got, _ = c.ray_color(rays[perm], 4, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == rgb4[perm].tobytes()      # the id travels with the ray; the slot is where it lies
        # a diffuse first hit: the ray whose 4-sample sum is largest among those that differ between samples
        one = [c.ray_color(rays, 1, depth, seed=SEED, sample_offset=k, camera=s.camera)[0] for k in range(2)]
        k = int(np.argmax(np.abs(one[0] - one[1]).sum(axis=1)))
        trio = np.repeat(rays[k:k + 1], 3)
        trio["id"][2] = trio["id"][0] + 12345
        got, _ = c.ray_color(trio, 4, depth, seed=SEED, camera=s.camera)
        assert got[0].tobytes() == got[1].tobytes() == rgb4[k].tobytes()
        assert got[2].tobytes() != got[0].tobytes()
        c.sync()
    finally:
        c.close()


# ----------------------------------------------------------------- invalid rays
def test_invalid_rays(g, lucy):
    s, rays, depth, rgb4 = lucy
    n = 300
    clean = rgb4[:n]
    bad = np.array(rays[:n])
    where = [0, 63, 64, 255, 256, n - 1]
    bad["o"][0, 1] = np.nan
    bad["o"][63, 0] = np.inf
    bad["d"][64, 2] = -np.inf
    bad["d"][255] = 0.0
    bad["d"][256, 0] = np.nan
    bad["o"][n - 1, 2] = -np.inf
    c = context(g, s.desc)
    try:
        got, st = c.ray_color(bad, 4, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 6
        assert not got[where].any()
        keep = np.setdiff1d(np.arange(n), where)
        assert got[keep].tobytes() == clean[keep].tobytes()
        assert clean[where].any()                          # those rays did carry light
        c.sync()
    finally:
        c.close()


# --------------------------------------------------------------- device variant
def test_device_variant_on_a_stream(g, lucy):
    import torch
    s, rays, depth, rgb4 = lucy
    c = context(g, s.desc)
    try:
        n = len(rays)
        p = g.ray_color_params(4, depth, seed=SEED, camera=s.camera)
        st = torch.cuda.Stream(device=0)
        with torch.cuda.stream(st):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint32).reshape(n, 8).view(np.int32).copy()).to("cuda:0")
            d_rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda:0")
            d_rgb2 = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda:0")
            c.ray_color_device(d_rays.data_ptr(), n, p, d_rgb.data_ptr(), stream=st.cuda_stream)
        # a second call on the default stream right behind it: the calls share the context's batch buffers
        c.ray_color_device(d_rays.data_ptr(), n, p, d_rgb2.data_ptr(), stream=torch.cuda.default_stream(0).cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        c.sync()
        assert c.last_render_kernel_ms() > 0.0
        assert d_rgb.cpu().numpy().tobytes() == rgb4.tobytes()
        assert d_rgb2.cpu().numpy().tobytes() == rgb4.tobytes()
    finally:
        c.close()


# --------------------------------------------------------------------- refusals
def test_refusals(g):
    s = scene(g, "cornell")                               # holds a fog volume
    rays = g.make_path_rays(np.zeros((2, 3)), np.array([[0, 0, -1], [0, 1, 0]]))
    lib = g.rtgpu()
    c = g.Context(0)
    try:
        with pytest.raises(g.RTError) as ex:
            c.ray_color(rays, 1, 2)
        assert ex.value.code == -5                        # RT_ERR_NO_SCENE
        c.upload(s.desc)
        assert c.info().volumes > 0
        rgb, _ = c.ray_color(rays, 1, 2, camera=s.camera)  # cornell is accepted
        assert np.isfinite(rgb).all()

        def status(n=2, rays_p=rays, rgb_p=rgb, **over):
            p = g.ray_color_params(1, 2)
            for k, v in over.items():
                if k == "background":
                    p.background[0] = v
                else:
                    setattr(p, k, v)
            rp = rays_p.ctypes.data_as(C.POINTER(g.RtPathRay)) if rays_p is not None else None
            op = rgb_p.ctypes.data_as(C.POINTER(C.c_float)) if rgb_p is not None else None
            return lib.rt_ray_color(c._h, rp, n, C.byref(p), op, None)

        assert status() == 0
        assert status(n=0) == 0
        assert status(rays_p=None) == -1 and status(rgb_p=None) == -1
        assert lib.rt_ray_color(c._h, rays.ctypes.data_as(C.POINTER(g.RtPathRay)), 2, None,
                                rgb.ctypes.data_as(C.POINTER(C.c_float)), None) == -1
        assert status(n=-1) == -1 and status(n=1 << 31) == -1
        for over in (dict(samples=0), dict(max_depth=0), dict(sample_offset=-1), dict(camera_max_depth=-1),
                     dict(background=float("nan")), dict(background=float("inf"))):
            assert status(**over) == -1, over
        marked = rays.copy()
        marked["reserved"][1] = 1
        assert status(rays_p=marked) == -1
        p = g.ray_color_params(1, 2)
        assert lib.rt_ray_color_device(c._h, None, 1, C.byref(p), C.c_void_p(16), None) == -1
        assert lib.rt_ray_color_device(c._h, C.c_void_p(16), 1, C.byref(p), None, None) == -1
        assert lib.rt_ray_color_device(c._h, C.c_void_p(16), 0, C.byref(p), C.c_void_p(16), None) == 0
        p.samples = 0
        assert lib.rt_ray_color_device(c._h, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
        c.sync()
    finally:
        c.close()
