"""rt_render_moments on the GPU: the frame is rt_render's bit for bit, the
moments are the luminance sums of the per-sample frames in the documented
fp64 operation order, and neither depends on the schedule; buckets,
accumulate, the device variant and the refusals."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 5
F = np.float32


@contextlib.contextmanager
def context(g, scene):
    c = g.Context(0)
    try:
        c.upload(scene.desc)
        yield c
    finally:
        c.close()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ulps(a, b):
    """Distance in float32 steps (both arrays non-negative and finite)."""
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def moments_of(frames, start=None):
    """The numpy-fp64 restatement over per-sample frames f_s (each sample's
    radiance exactly: one fp64 add to 0, one rounding back): per sample
    Y = (0.2126 x + 0.7152 y) + 0.0722 z, m1 += Y, m2 += Y * Y, in sample
    order; `start` = the float32 moments an accumulating call adds to."""
    m1 = np.zeros(frames[0].shape[:2], np.float64)
    m2 = np.zeros(frames[0].shape[:2], np.float64)
    for f in frames:
        L = f.astype(np.float64)
        y = (0.2126 * L[..., 0] + 0.7152 * L[..., 1]) + 0.0722 * L[..., 2]
        m1 = m1 + y
        m2 = m2 + y * y
    if start is not None:
        m1 = m1 + start[..., 0].astype(np.float64)
        m2 = m2 + start[..., 1].astype(np.float64)
    return np.stack([m1, m2], axis=-1).astype(F)


def singles(c, g, cam, n, depth, first=0):
    return [c.render(cam, g.make_params(1, depth, seed=SEED, sample_offset=first + s))[0] for s in range(n)]


def check_against_singles(mom, frames, what, start=None):
    exp = moments_of(frames, start)
    u = ulps(mom, exp)
    print(f"{what}: {int((u > 0).sum())} of {u.size} moments differ from the fp64 restatement, max {int(u.max())} ulp")
    assert u.max() <= 1


@pytest.fixture(scope="module")
def cornell(g):
    return g.Scene("cornell", width=48)


@pytest.fixture(scope="module")
def cornell_runs(g, cornell):
    """The six per-sample frames, the 6-spp frame and its moments render."""
    cam = cornell.camera
    with context(g, cornell) as c:
        f = singles(c, g, cam, 12, 5)
        frame, _ = c.render(cam, g.make_params(6, 5, seed=SEED))
        accum, mom, st = c.render_moments(cam, g.make_params(6, 5, seed=SEED))
        again, _ = c.render(cam, g.make_params(6, 5, seed=SEED))
    assert np.array_equal(bits(frame), bits(again))   # the moments call leaves later renders alone
    return dict(singles=f, frame=frame, accum=accum, mom=mom, stats=st)


def test_precondition_frame_is_the_sum_of_its_samples(cornell_runs):
    r = cornell_runs
    s = np.zeros(r["frame"].shape, np.float64)
    for f in r["singles"][:6]:
        s = s + f.astype(np.float64)
    assert np.array_equal(bits(s.astype(F)), bits(r["frame"]))


def test_frame_bits_and_moments(cornell, cornell_runs):
    r = cornell_runs
    cam = cornell.camera
    assert r["mom"].shape == (cam.image_height, cam.image_width, 2) and r["mom"].dtype == F
    assert np.array_equal(bits(r["accum"]), bits(r["frame"])) and r["frame"].sum() > 0
    assert r["stats"].samples == 6 * cam.image_width * cam.image_height
    check_against_singles(r["mom"], r["singles"][:6], "cornell 48, 6 spp")
    m1, m2 = r["mom"][..., 0], r["mom"][..., 1]
    assert (m2 > 0).mean() >= 1 / 3
    # Cauchy-Schwarz within rounding: m1^2 <= n * m2
    assert (m1.astype(np.float64) ** 2 <= 6 * m2.astype(np.float64) * (1 + 1e-6)).all()


def test_schedule_independent(g, cornell, cornell_runs):
    cam = cornell.camera
    npix = cam.image_width * cam.image_height
    p = g.make_params(6, 5, seed=SEED)
    # wave_layout.h size_batch: at most target / npix samples per batch
    slots = 2 * npix
    max_spb = max(1, min(6, slots // npix))
    assert (6 + max_spb - 1) // max_spb > 1
    with context(g, cornell) as c:
        for streams, sl in ((1, 0), (3, 0), (1, slots), (3, slots)):
            c.set_schedule(sl, 0, 0, streams)
            accum, mom, _ = c.render_moments(cam, p)
            assert np.array_equal(bits(accum), bits(cornell_runs["frame"])), (streams, sl)
            assert np.array_equal(bits(mom), bits(cornell_runs["mom"])), (streams, sl)


def test_buckets_and_accumulate(g, cornell, cornell_runs):
    r = cornell_runs
    cam = cornell.camera
    H, W = cam.image_height, cam.image_width
    tiles = g.generate_buckets(W, H, 16)
    half = [tuple(t) for t in tiles[::2]]
    assert 0 < len(half) < len(tiles)
    inside = np.zeros((H, W), bool)
    for x, y, w, h in half:
        inside[y:y + h, x:x + w] = True
    assert 0 < inside.sum() < inside.size
    with context(g, cornell) as c:
        a0, m0 = np.full((H, W, 3), F(-2.5)), np.full((H, W, 2), F(-7.5))
        a, m, st = c.render_moments(cam, g.make_params(6, 5, seed=SEED, buckets=half), a0, m0)
        assert st.samples == 6 * inside.sum()
        assert np.array_equal(bits(m[inside]), bits(r["mom"][inside]))
        assert np.array_equal(bits(a[inside]), bits(r["frame"][inside]))
        assert (m[~inside] == F(-7.5)).all() and (a[~inside] == F(-2.5)).all()
        # a second call adds samples 6..11 to both arrays (k_finalize's expression)
        a12, m12, _ = c.render_moments(cam, g.make_params(6, 5, seed=SEED, sample_offset=6, accumulate=True),
                                       r["accum"].copy(), r["mom"].copy())
        one12, mom12, _ = c.render_moments(cam, g.make_params(12, 5, seed=SEED))
        plain, _ = c.render(cam, g.make_params(6, 5, seed=SEED, sample_offset=6, accumulate=True), r["frame"].copy())
    assert np.array_equal(bits(a12), bits(plain))
    check_against_singles(m12, r["singles"][6:], "accumulate, samples 6..11", start=r["mom"])
    check_against_singles(mom12, r["singles"], "cornell 48, 12 spp")
    u = ulps(m12, mom12)
    print(f"6 + 6 accumulated against 12 at once: {int((u > 0).sum())} of {u.size} differ, max {int(u.max())} ulp")
    assert u.max() <= 1


def test_tail_kernel_scene(g):
    """`random` has no lights and depth 12 is above 8: k_tail carries the last
    paths, and Lout is read as the tail kernel leaves it."""
    s = g.Scene("random", width=48)
    cam = s.camera
    with context(g, s) as c:
        f = singles(c, g, cam, 4, 12)
        frame, _ = c.render(cam, g.make_params(4, 12, seed=SEED))
        accum, mom, _ = c.render_moments(cam, g.make_params(4, 12, seed=SEED))
        c.set_tail(1)   # RT_OPT_TAIL off: the same moments without the tail kernel
        accum2, mom2, _ = c.render_moments(cam, g.make_params(4, 12, seed=SEED))
    assert np.array_equal(bits(accum), bits(frame)) and np.array_equal(bits(accum2), bits(frame))
    assert np.array_equal(bits(mom), bits(mom2))
    check_against_singles(mom, f, "random 48, 4 spp, depth 12")
    assert (mom[..., 1] > 0).mean() >= 1 / 3


def test_device_variant_equals_host(g, cornell, cornell_runs):
    import torch
    cam = cornell.camera
    H, W = cam.image_height, cam.image_width
    p = g.make_params(6, 5, seed=SEED)
    with context(g, cornell) as c:
        dev = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        mom = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        c.render_moments_device(cam, p, dev.data_ptr(), mom.data_ptr())
        c.sync()
        assert c.last_render_kernel_ms() > 0
        assert np.array_equal(bits(dev.cpu().numpy()), bits(cornell_runs["frame"]))
        assert np.array_equal(bits(mom.cpu().numpy()), bits(cornell_runs["mom"]))


def test_refusals(g, cornell):
    import ctypes as C
    cam = cornell.camera
    p = g.make_params(1, 1)
    c = g.Context(0)
    try:
        with pytest.raises(g.RTError) as e:
            c.render_moments(cam, p)
        assert e.value.code == -5   # RT_ERR_NO_SCENE
        c.upload(cornell.desc)
        accum = np.zeros((cam.image_height, cam.image_width, 3), F)
        rc = g.rtgpu().rt_render_moments(c._h, C.byref(cam), C.byref(p), accum.ctypes.data_as(C.POINTER(C.c_float)),
                                         None, None)
        assert rc == -1             # RT_ERR_INVALID: null moments
        with pytest.raises(g.RTError) as e:
            c.render_moments(cam, g.make_params(0, 1))
        assert e.value.code == -1
    finally:
        c.close()


def test_multi_device_context_is_refused(g, cornell):
    if g.device_count() < 2:
        pytest.skip("needs two visible devices")
    c = g.Context(devices=[0, 1])
    try:
        c.upload(cornell.desc)
        with pytest.raises(g.RTError) as e:
            c.render_moments(cornell.camera, g.make_params(1, 1))
        assert e.value.code == -2   # RT_ERR_UNSUPPORTED
        assert "multi-device" in str(e.value)
    finally:
        c.close()
