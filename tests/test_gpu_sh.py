"""rt_gather_sh on the GPU, through the C-ABI.

  * the equality that defines it: for every sample s the rays of
    rt_gather_rays(SPHERE, s), rt_ray_color over them with samples = 1 at that
    offset, projected by tests/sh_ref.py (float32 basis, float64 sum in sample
    order, rounded once) is rt_gather_sh, all bytes: cornell (fog) and a
    reduced cornell-lucy, 4 samples, bands 3;
  * the coefficients of fewer bands are a prefix; sums over samples and calls
    and `accumulate`; cuts of the array, schedules, chunk sizes, ids, invalid
    points, the _device variant on a stream, the refusals;
  * a closed form under the sky gradient: 64 probes that cannot see the
    scene's one tiny sphere, 256 samples each; the pooled means of every
    coefficient against the integrals, at 6 standard errors of each term's own
    variance.

Nothing here provokes a fault: the invalid points are defined input that the
guard at the point load turns into zeros."""
import ctypes as C

import numpy as np
import pytest

from tests import gather_ref as GR
from tests import sh_ref as SR
from tests.scene_builder import Builder
from tests.test_gpu_gather import context, scene

pytestmark = pytest.mark.gpu

SEED = 29
N = 600
SAMPLES = 4


def surface_points(g, c, cam):
    """N points on the surfaces the camera sees (rt_trace_rays hits of sample
    0's camera rays); a miss becomes a fixed point inside the box."""
    _, _, _, ray = c.extend_hits(cam, SEED, 0, 0)
    o, d = ray[100:100 + N, 0:3], ray[100:100 + N, 3:6]
    top, prim, t, mat, n, flags = c.trace_rays(o, d)
    hit = top >= 0
    assert hit.sum() > N // 2
    p = (o + np.float32(0.999) * t[:, None] * d).astype(np.float32)
    p[~hit] = (278.0, 278.0, 278.0)
    n = n.copy()
    n[~hit] = (0.0, 0.0, 1.0)
    return g.make_gather_points(p, n, ids=np.arange(N) + 1000)


def free_points(g, c, cam):
    """N points a little in front of what the camera rays hit (scenes whose
    volumes rt_trace_rays refuses)."""
    top, prim, t, ray = c.extend_hits(cam, SEED, 0, 0)
    sl = slice(100, 100 + N)
    o, d, t = ray[sl, 0:3], ray[sl, 3:6], t[sl]
    step = np.where((top[sl] >= 0) & np.isfinite(t), np.float32(0.98) * t, np.float32(1.0)).astype(np.float32)
    return g.make_gather_points(o + step[:, None] * d, -d, ids=np.arange(N) + 1000)


def per_sample(c, pts, cam, depth, samples, offset=0):
    """([L_s], [d_s]): rt_ray_color with one sample at offset + s over the rays
    of rt_gather_rays(SPHERE, offset + s), and those rays' directions."""
    L, d = [], []
    for s in range(offset, offset + samples):
        rays = c.gather_rays(pts, GR.SPHERE, seed=SEED, sample=s)
        assert rays.tobytes() == GR.rays(pts, GR.SPHERE, SEED, s).tobytes(), f"the probe, sample {s}"
        rgb, _ = c.ray_color(rays, 1, depth, seed=SEED, sample_offset=s, camera=cam)
        L.append(rgb)
        d.append(rays["d"])
    return L, d


def differing(got, want):
    return np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))


@pytest.fixture(scope="module")
def lucy(g):
    """The reduced cornell-lucy, N surface points, their per-sample radiances
    and directions, and the 4-sample bands-3 sums of one default call."""
    s = scene(g, "cornell-lucy")
    c = context(g, s.desc)
    try:
        assert c.lifted_prims() > 0
        pts = surface_points(g, c, s.camera)
        depth = s.camera.max_depth
        L, d = per_sample(c, pts, s.camera, depth, SAMPLES)
        sh, st = c.gather_sh(pts, 3, SAMPLES, depth, seed=SEED, camera=s.camera)
        assert st.samples == SAMPLES * N and st.invalid_rays == 0
        c.sync()
    finally:
        c.close()
    for a in [pts, sh] + L + d:
        a.setflags(write=False)
    assert sh.shape == (N, 9, 3) and np.isfinite(sh).all() and (sh[:, 0] > 0).any()
    return s, pts, depth, sh, L, d


def test_defining_equality_lucy(g, lucy):
    s, pts, depth, sh, L, d = lucy
    want = SR.project(L, d, np.ones(N, bool), 3)
    bad = differing(sh, want)
    assert len(bad) == 0, f"{len(bad)} of {N} points differ, first {bad[0]}: {sh[bad[0]]} vs {want[bad[0]]}"
    assert (np.abs(sh).max(axis=(0, 2)) > 0).all()        # every coefficient carries something


@pytest.mark.parametrize("in_bvh", [False, True], ids=["lifted", "in_bvh"])
def test_defining_equality_cornell_fog(g, in_bvh):
    s = scene(g, "cornell")
    c = context(g, s.desc, volumes_in_bvh=in_bvh)
    try:
        assert c.info().volumes > 0
        pts = free_points(g, c, s.camera)
        depth = s.camera.max_depth
        L, d = per_sample(c, pts, s.camera, depth, SAMPLES)
        got, st = c.gather_sh(pts, 3, SAMPLES, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 0 and st.samples == SAMPLES * N and st.kernel_ms > 0
        want = SR.project(L, d, np.ones(N, bool), 3)
        bad = differing(got, want)
        assert len(bad) == 0, f"{len(bad)} of {N} points differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
        assert np.isfinite(got).all() and (got[:, 0] > 0).any()
        c.sync()                                          # raises on a device error
    finally:
        c.close()


def test_band_prefix(g, lucy):
    s, pts, depth, sh, L, d = lucy
    c = context(g, s.desc)
    try:
        for b in (1, 2):
            got, _ = c.gather_sh(pts, b, SAMPLES, depth, seed=SEED, camera=s.camera)
            assert got.shape == (N, b * b, 3)
            assert got.tobytes() == np.ascontiguousarray(sh[:, :b * b]).tobytes(), f"bands {b}"
        c.sync()
    finally:
        c.close()


def test_sums_over_samples_and_calls(g, lucy):
    """A one-sample call rounds its product to float, so calls do not add up
    to a longer call as rt_gather's do: every call is its own projection of
    the per-sample radiances, and `accumulate` adds double(previous)."""
    s, pts, depth, sh, L, d = lucy
    ok = np.ones(N, bool)
    c = context(g, s.desc)
    try:
        one = [c.gather_sh(pts, 3, 1, depth, seed=SEED, sample_offset=k, camera=s.camera)[0] for k in range(SAMPLES)]
        for k in range(SAMPLES):
            assert one[k].tobytes() == SR.project(L[k:k + 1], d[k:k + 1], ok, 3).tobytes(), k
        assert all(a.tobytes() != one[0].tobytes() for a in one[1:])      # every sample has its own directions
        first, _ = c.gather_sh(pts, 3, 2, depth, seed=SEED, sample_offset=0, camera=s.camera)
        assert first.tobytes() == SR.project(L[:2], d[:2], ok, 3).tobytes()
        both, _ = c.gather_sh(pts, 3, 2, depth, seed=SEED, sample_offset=2, camera=s.camera, accum=first.copy())
        assert both.tobytes() == SR.project(L[2:], d[2:], ok, 3, previous=first).tobytes()
        c.sync()
    finally:
        c.close()


@pytest.mark.parametrize("k", range(5), ids=["slots-1", "slots-2n+3", "streams-1", "streams-3", "max-blocks-1"])
def test_cuts_and_schedules(g, lucy, k):
    s, pts, depth, sh, L, d = lucy
    sched = [dict(batch_slots=1), dict(batch_slots=2 * N + 3), dict(streams=1), dict(streams=3), dict(max_blocks=1)][k]
    c = context(g, s.desc, **sched)
    try:
        got, _ = c.gather_sh(pts, 3, SAMPLES, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == sh.tobytes(), sched
        c.sync()
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_chunk_sizes(g, lucy, n):
    s, pts, depth, sh, L, d = lucy
    c = context(g, s.desc)
    try:
        for off in (0, 300):
            got, _ = c.gather_sh(pts[off:off + n], 3, SAMPLES, depth, seed=SEED, camera=s.camera)
            assert got.tobytes() == sh[off:off + n].tobytes(), f"n {n} at {off}"
        got, st = c.gather_sh(pts[:0], 3, SAMPLES, depth, seed=SEED, camera=s.camera)       # n == 0: RT_OK
        assert got.shape == (0, 9, 3) and st.samples == 0
        c.sync()
    finally:
        c.close()


def test_ids(g, lucy):
    s, pts, depth, sh, L, d = lucy
    c = context(g, s.desc)
    try:
        perm = np.random.default_rng(5).permutation(N)
        got, _ = c.gather_sh(pts[perm], 3, SAMPLES, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == sh[perm].tobytes()        # the id travels with the point; the slot is where it lies
        k = int(np.argmax(sh[:, 0].sum(axis=1)))
        trio = np.repeat(pts[k:k + 1], 3)
        trio["id"][2] = trio["id"][0] + 12345
        got, _ = c.gather_sh(trio, 3, SAMPLES, depth, seed=SEED, camera=s.camera)
        assert got[0].tobytes() == got[1].tobytes() == sh[k].tobytes()        # duplicate ids: the same paths
        assert got[2].tobytes() != got[0].tobytes()
        c.sync()
    finally:
        c.close()


def test_invalid_points(g, lucy):
    s, pts, depth, sh, L, d = lucy
    n = 300
    where = [0, 63, n - 1]
    bad = np.array(pts[:n])
    bad["p"][0, 1] = np.nan
    bad["p"][63, 0] = np.inf
    bad["p"][n - 1, 2] = -np.inf
    bad["n"][64] = 0.0                                    # n is not read: these stay valid
    bad["n"][255, 0] = np.nan
    c = context(g, s.desc)
    try:
        got, st = c.gather_sh(bad, 3, SAMPLES, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 3 and st.samples == SAMPLES * n
        assert not got[where].any()
        keep = np.setdiff1d(np.arange(n), where)
        assert got[keep].tobytes() == sh[:n][keep].tobytes()
        assert sh[:n][where].any()                        # those points did gather light
        # with accumulate an invalid point keeps its previous values
        prev = np.full((n, 9, 3), 0.5, np.float32)
        got, _ = c.gather_sh(bad, 3, SAMPLES, depth, seed=SEED, camera=s.camera, accum=prev.copy())
        assert (got[where] == np.float32(0.5)).all()
        assert got[keep].tobytes() == SR.project([x[:n] for x in L], [x[:n] for x in d], np.ones(n, bool), 3,
                                                 previous=prev)[keep].tobytes()
        c.sync()
    finally:
        c.close()


def test_device_variant_on_a_stream(g, lucy):
    import torch
    s, pts, depth, sh, L, d = lucy
    c = context(g, s.desc)
    try:
        p = g.gather_sh_params(3, SAMPLES, depth, seed=SEED, camera=s.camera)
        st = torch.cuda.Stream(device=0)
        with torch.cuda.stream(st):
            d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint32).reshape(N, 8).view(np.int32).copy()).to("cuda:0")
            d_sh = torch.full((N, 9, 3), 7.0, dtype=torch.float32, device="cuda:0")
            d_sh2 = torch.full((N, 9, 3), 7.0, dtype=torch.float32, device="cuda:0")
            c.gather_sh_device(d_pts.data_ptr(), N, p, d_sh.data_ptr(), stream=st.cuda_stream)
        # a second call on the default stream right behind it: the calls share the context's batch buffers
        c.gather_sh_device(d_pts.data_ptr(), N, p, d_sh2.data_ptr(), stream=torch.cuda.default_stream(0).cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        c.sync()
        assert c.last_render_kernel_ms() > 0.0
        assert d_sh.cpu().numpy().tobytes() == sh.tobytes()
        assert d_sh2.cpu().numpy().tobytes() == sh.tobytes()
    finally:
        c.close()


def test_closed_form_under_the_sky_gradient(g):
    """One Lambertian sphere of radius 1e-3 and 64 probes 1e3 units from it: it
    covers 2.5e-13 of a probe's directions, and rt_trace_rays over the very
    rays of every sample shows that none hits it.  Every sample's radiance is
    then the sky gradient L_c = 1 - 0.5 (y + 1)(1 - col_c), col = (0.5, 0.7, 1):
    the mean of L_c Y_k over the sphere is 0.282095 (1 - 0.5 (1 - col_c)) for
    k = 0, -0.488603 (1 - col_c) / 6 for k = 1 and 0 for the rest.  The pooled
    mean of the 64 x 256 samples is held to 6 standard errors of the term's own
    variance (float64 quadrature over the sphere); blue's coefficient 0 has no
    variance: it is samples * 0.282095 per point to 1e-6 relative (two fp32
    roundings of (1 - a) + a give at most 2e-7)."""
    P, S = 64, 256
    M = P * S
    col = np.array([0.5, 0.7, 1.0])
    b = Builder(g)
    desc = b.desc(b.listing([b.sphere((0, 0, 0), 1e-3, b.lambertian((0.5, 0.5, 0.5)))]))
    u = np.random.default_rng(7).normal(size=(P, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = g.make_gather_points(1e3 * u, np.zeros((P, 3)), ids=np.arange(P) + 17)
    c = g.Context(0)
    try:
        c.upload(desc)
        o = np.concatenate([c.gather_rays(pts, GR.SPHERE, seed=SEED, sample=s) for s in range(S)])
        assert o.shape == (M,) and o["d"].any(axis=1).all()
        top = c.trace_rays(o["o"], o["d"])[0]
        assert (top < 0).all(), "a probe ray hits the sphere"
        sh, st = c.gather_sh(pts, 3, S, 4, seed=SEED, use_sky_gradient=1)
        assert st.invalid_rays == 0 and st.samples == M
        c.sync()
    finally:
        c.close()
    # quadrature: Gauss-Legendre in y (the gradient's axis), uniform in the azimuth
    ny, nphi = 200, 400
    y, wy = np.polynomial.legendre.leggauss(ny)
    phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
    r = np.sqrt(1 - y * y)
    Y = SR.basis(np.stack([r[:, None] * np.sin(phi)[None], np.repeat(y[:, None], nphi, 1), r[:, None] * np.cos(phi)[None]],
                          -1).astype(np.float32), 3).astype(np.float64)          # (ny, nphi, 9)
    w = np.broadcast_to(wy[:, None] / (2.0 * nphi), (ny, nphi))       # of total weight 1: the mean over the sphere
    Lq = 1.0 - 0.5 * (y[:, None, None] + 1.0) * (1.0 - col)[None, None, :]      # (ny, 1, 3)
    term = Lq[:, :, None, :] * Y[:, :, :, None]                         # (ny, nphi, 9, 3)
    mean_q = np.einsum("tpkc,tp->kc", term, w)
    var = np.einsum("tpkc,tp->kc", term * term, w) - mean_q * mean_q
    want = np.zeros((9, 3))
    want[0] = 0.282095 * (1.0 - 0.5 * (1.0 - col))
    want[1] = -0.488603 * (1.0 - col) / 6.0
    assert np.abs(mean_q - want).max() < 1e-6             # the quadrature agrees with the closed form
    got = sh.astype(np.float64).sum(axis=0) / M
    se = np.sqrt(np.maximum(var, 0.0) / M)
    print("pooled means\n", got, "\nclosed form\n", want, "\nin standard errors\n", np.abs(got - want) / np.maximum(se, 1e-300))
    for k in range(9):
        for ch in range(3):
            if k == 0 and ch == 2:
                continue                                  # no variance: held below
            assert se[k, ch] > 1e-4
            assert abs(got[k, ch] - want[k, ch]) <= 6 * se[k, ch], (k, ch, got[k, ch], want[k, ch], se[k, ch])
    assert var[0, 2] < 1e-12
    assert (np.abs(sh[:, 0, 2].astype(np.float64) / (S * 0.282095) - 1.0) <= 1e-6).all()


def test_refusals(g):
    s = scene(g, "cornell")
    pts = g.make_gather_points(np.full((2, 3), 278.0), np.array([[0, 0, 1], [0, 1, 0]]))
    lib = g.rtgpu()
    c = g.Context(0)
    try:
        with pytest.raises(g.RTError) as ex:
            c.gather_sh(pts, 3, 1, 2)
        assert ex.value.code == -5                        # RT_ERR_NO_SCENE
        c.upload(s.desc)
        sh, _ = c.gather_sh(pts, 3, 1, 2, camera=s.camera)
        assert sh.shape == (2, 9, 3) and np.isfinite(sh).all()
        pp = pts.ctypes.data_as(C.POINTER(g.RtGatherPoint))
        op = sh.ctypes.data_as(C.POINTER(C.c_float))

        def status(n=2, pts_p=pp, sh_p=op, bands=3, reserved=0, **over):
            p = g.gather_sh_params(bands, 1, 2)
            p.reserved = reserved
            for k, v in over.items():
                if k == "background":
                    p.path.background[0] = v
                else:
                    setattr(p.path, k, v)
            return lib.rt_gather_sh(c._h, pts_p, n, C.byref(p), sh_p, None)

        assert status() == 0 and status(n=0) == 0 and status(bands=1) == 0 and status(bands=2) == 0
        assert status(pts_p=None) == -1 and status(sh_p=None) == -1
        assert lib.rt_gather_sh(c._h, pp, 2, None, op, None) == -1
        assert status(bands=0) == -1 and status(bands=4) == -1 and status(bands=-1) == -1 and status(reserved=1) == -1
        assert status(n=-1) == -1 and status(n=1 << 31) == -1
        for over in (dict(samples=0), dict(max_depth=0), dict(sample_offset=-1), dict(camera_max_depth=-1),
                     dict(background=float("nan")), dict(background=float("inf"))):
            assert status(**over) == -1, over
        marked = pts.copy()
        marked["reserved"][1] = 1
        assert status(pts_p=marked.ctypes.data_as(C.POINTER(g.RtGatherPoint))) == -1
        p = g.gather_sh_params(3, 1, 2)
        assert lib.rt_gather_sh_device(c._h, None, 1, C.byref(p), C.c_void_p(16), None) == -1
        assert lib.rt_gather_sh_device(c._h, C.c_void_p(16), 1, C.byref(p), None, None) == -1
        assert lib.rt_gather_sh_device(c._h, C.c_void_p(16), 1, None, C.c_void_p(16), None) == -1
        assert lib.rt_gather_sh_device(c._h, C.c_void_p(16), 0, C.byref(p), C.c_void_p(16), None) == 0
        p.bands = 4
        assert lib.rt_gather_sh_device(c._h, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
        p.bands, p.reserved = 3, 2
        assert lib.rt_gather_sh_device(c._h, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
        c.sync()
    finally:
        c.close()
