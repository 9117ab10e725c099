"""Rays that miss the world box resolved in k_shade (RT_OPT_EARLY_MISS) on the
device: everything a context returns is the same with the option on (2) and
off (1), np.array_equal, on the same context settings.

  * frames: cornell-lucy at width 96 (8 spp, depth 5) and at 37 x 29 (3 spp),
    `cornell` (fog), `random` at depth 50 (it stands on a plane: not eligible,
    both renders take the old path, through the long-tail kernel), the closed
    room, the scene where every ray misses the box and the one where none
    does, an importance-sampled environment (two-ray jobs), and a deep unlit
    scene with the long-tail kernel on (the survivors' part stays off) and off;
  * schedules on cornell-lucy: one, two and three streams, the bounce overlap,
    three batches, and depth 12 (the rays-left probe counts front + back);
  * rt_render_moments and rt_ray_color; rt_shadow_visibility and the path
    probes (probing renders stay on the old path);
  * the instrumented run's counters: the rays k_shade resolved are the rays
    the traversal kernels no longer trace, more than 20 % of each kind.
Small pictures: tests/test_early_host.py pins the schedule ray by ray on the
host; these pin that the device kernels do the same.
"""
import numpy as np
import pytest

from tests import early_cases as EC

pytestmark = pytest.mark.gpu

SEED = 23
OFF, ON = 1, 2
LUCY = dict(lucy_rings=30, lucy_cols=40)


def both(g, desc, setup=None, run=None):
    """run(context) with the option off, then on, on one context."""
    c = g.Context(0)
    try:
        if setup:
            setup(c)
        c.upload(desc)
        out = []
        for mode in (OFF, ON):
            c.set_early_miss(mode)
            out.append(run(c))
        return out
    finally:
        c.close()


def frames_equal(g, desc, cam, spp, depth, setup=None):
    p = g.make_params(spp, depth, seed=SEED)
    off, on = both(g, desc, setup, lambda c: c.render(cam, p)[0].copy())
    assert np.isfinite(on).all() and on.max() > 0
    assert np.array_equal(on, off), f"{int(np.sum(np.any(on != off, axis=2)))} pixels differ"
    return on


# ------------------------------------------------------------------- sizes
def test_cornell_lucy_w96(g):
    s = g.Scene("cornell-lucy", width=96, **LUCY)
    frames_equal(g, s.desc, s.camera, 8, 5)


def test_cornell_lucy_37x29(g):
    s = g.Scene("cornell-lucy", width=EC.W, aspect=EC.W / EC.H, **LUCY)
    frames_equal(g, s.desc, s.camera, EC.SPP, 5)


def test_cornell_fog(g):
    s = g.Scene("cornell", width=64)
    frames_equal(g, s.desc, s.camera, 4, 5)


def test_random_depth_50(g):
    s = g.Scene("random", width=96)
    frames_equal(g, s.desc, s.camera, 4, 50)


@pytest.mark.parametrize("make", [EC.closed_room, EC.all_miss_room, EC.all_pass_room, EC.env_room],
                         ids=["closed-room", "all-miss", "all-pass", "env-room"])
def test_rooms(g, make):
    c = make(g)
    frames_equal(g, c.desc, c.cam, EC.SPP, c.cam.max_depth)


@pytest.mark.parametrize("tail", [0, 1], ids=["tail-auto", "tail-off"])
def test_deep_unlit_scene(g, tail):
    """Depth 12 without lights: with the long-tail kernel allowed the
    survivors' part stays off; with it off the back of the stream is used and
    the rays-left probe counts it."""
    c = EC.unlit_floor(g)
    frames_equal(g, c.desc, c.cam, EC.SPP, 12, setup=lambda x: x.set_tail(tail))


# --------------------------------------------------------------- schedules
@pytest.mark.parametrize("streams", [1, 2, 3])
def test_streams(g, streams):
    s = g.Scene("cornell-lucy", width=96, **LUCY)
    frames_equal(g, s.desc, s.camera, 8, 5, setup=lambda c: c.set_option(g.RT_OPT_STREAMS, streams))


def test_overlap(g):
    s = g.Scene("cornell-lucy", width=96, **LUCY)
    frames_equal(g, s.desc, s.camera, 8, 5, setup=lambda c: c.set_overlap(2))


def test_three_batches(g):
    s = g.Scene("cornell-lucy", width=96, **LUCY)
    npix = s.camera.image_width * s.camera.image_height
    a = frames_equal(g, s.desc, s.camera, 8, 5, setup=lambda c: c.set_schedule(batch_slots=3 * npix, streams=1))
    b = frames_equal(g, s.desc, s.camera, 8, 5, setup=lambda c: c.set_schedule(streams=1))
    assert np.array_equal(a, b)


def test_lit_depth_12(g):
    s = g.Scene("cornell-lucy", width=96, **LUCY)
    frames_equal(g, s.desc, s.camera, 4, 12)


# ------------------------------------------------------ other entry points
def test_moments(g):
    s = g.Scene("cornell-lucy", width=64, **LUCY)
    p = g.make_params(4, 5, seed=SEED)
    off, on = both(g, s.desc, None, lambda c: [np.array(x).copy() for x in c.render_moments(s.camera, p)[:2]])
    assert on[0].max() > 0 and on[1].max() > 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])


def test_ray_color(g):
    s = g.Scene("cornell-lucy", width=48, **LUCY)
    cam = s.camera
    W, H = cam.image_width, cam.image_height
    o = np.array(list(cam.center), np.float64)
    p00, du, dv = (np.array(list(x), np.float64) for x in (cam.pixel00, cam.pixel_delta_u, cam.pixel_delta_v))
    yy, xx = np.mgrid[0:H, 0:W]
    tgt = p00 + xx[..., None] * du + yy[..., None] * dv
    rays = g.make_path_rays(np.broadcast_to(o, (H * W, 3)), (tgt - o).reshape(-1, 3))
    off, on = both(g, s.desc, None, lambda c: c.ray_color(rays, 4, 5, seed=SEED, camera=cam)[0].copy())
    assert on.max() > 0
    assert np.array_equal(on, off)


def test_probes_stay_on_the_old_path(g):
    s = g.Scene("cornell-lucy", width=48, **LUCY)
    cam = s.camera

    def probes(c):
        return [(c.extend_hits(cam, SEED, 0, b), c.shadow_visibility(cam, SEED, 0, b)) for b in range(4)]

    off, on = both(g, s.desc, None, probes)
    traced = 0
    for b, ((hon, non), (hoff, noff)) in enumerate(zip(on, off)):
        for name, x, y in zip(("top", "prim", "t", "ray"), hon, hoff):
            same = np.array_equal(x, y) if x.dtype != np.float32 else np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert same, f"bounce {b}: {name} differs"
        assert np.array_equal(non, noff), f"bounce {b}: NEE words differ"
        traced += int(np.sum(non & 1))
    assert traced > 0


# ---------------------------------------------------------------- counters
def test_counters(g):
    s = g.Scene("cornell-lucy", width=96, **LUCY)
    p = g.make_params(8, 5, seed=SEED)
    off, on = both(g, s.desc, None, lambda c: c.count_work_by_kernel(s.camera, p))
    print("off", {k: (v["rays"], v["shadow_rays"], v["early_rays"], v["early_shadow_rays"]) for k, v in off.items()})
    print("on ", {k: (v["rays"], v["shadow_rays"], v["early_rays"], v["early_shadow_rays"]) for k, v in on.items()})
    assert off["shade"]["early_rays"] == 0 and off["shade"]["early_shadow_rays"] == 0
    early_next, early_nee = on["shade"]["early_rays"], on["shade"]["early_shadow_rays"]
    assert on["extend"]["rays"] + early_next == off["extend"]["rays"]
    assert on["shadow"]["shadow_rays"] + early_nee == off["shadow"]["shadow_rays"]
    assert on["shade"]["rays"] == off["shade"]["rays"]          # every path is shaded either way
    samples = off["extend"]["samples"]
    assert early_next > 0.2 * (off["extend"]["rays"] - samples)
    assert early_nee > 0.2 * off["shadow"]["shadow_rays"]
    # one ray per job here (no environment sampling): the jobs k_shade wrote are the rays k_shadow traced
    assert on["shade"]["shadow_rays"] == on["shadow"]["shadow_rays"]
    assert off["shade"]["shadow_rays"] == off["shadow"]["shadow_rays"]


def test_option_range(g):
    c = g.Context(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(g.RTError):
                c.set_option(g.RT_OPT_EARLY_MISS, bad)
        for ok in (0, 1, 2):
            c.set_option(g.RT_OPT_EARLY_MISS, ok)
    finally:
        c.close()
