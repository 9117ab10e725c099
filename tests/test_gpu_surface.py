"""rt_gather_surface on the GPU, through the C-ABI.

  * the equality that defines it: for a ray r whose closest hit is a white
    Lambertian wall with an axis-aligned normal, with t and n from rt_trace_rays
    and P = fl(o + fl(d t)), rt_gather_surface({P, r.id, n}) is rt_ray_color(r),
    all bytes, at depths 1, 2 and 5 and samples 0 and 1: path_cases' room with
    six white walls, and white-walled lights3, sphere_in_list, env_is_area and
    fog_shadow (both RT_OPT_VOLUMES placements), under the three node formats,
    RT_OPT_LIFT_PRIMS on and off (a small triangle stays in the world BVH so
    that lifting applies), RT_OPT_EARLY_MISS 1 and 2, RT_OPT_OVERLAP 2,
    RT_OPT_STREAMS 1 and 3 and a small RT_OPT_BATCH_SLOTS.  fog_shadow's t comes
    from rt_extend_hits (rt_trace_rays refuses scenes with a volume) and its n
    is the wall's; a ray the fog scatters has the volume as its closest hit and
    is left out like one that meets the lamp;
  * the rows of tests/surface_cases.py against tests/surface_ref.py (float64),
    held to test_path_kat.radiance_bar(group, "device");
  * schedule invariance, one-sample sums, accumulate, the _device form on a
    caller's stream, ids, invalid points, closed forms, refusals, on the reduced
    cornell-lucy of the gather tests.

Nothing here provokes a fault: the invalid points are defined input that the
guard at the point load turns into zeros."""
import ctypes as C

import numpy as np
import pytest

from tests import path_cases as PC
from tests import surface_cases as SC
from tests.scene_builder import Builder
from tests.test_gpu_gather import SEED, scene
from tests.test_path_kat import radiance_bar

pytestmark = pytest.mark.gpu

NP, NS = 300, 3                                # the schedule tests' points and samples


def make_context(g, desc, early=0, overlap=0, nodes="fp32", lifted=True, volumes_in_bvh=False, **schedule):
    c = g.Context(0)
    c.set_lift_prims(lifted)
    c.set_node_format(nodes)
    c.set_option(g.RT_OPT_VOLUMES, g.RT_VOLUMES_IN_BVH if volumes_in_bvh else g.RT_VOLUMES_LIFTED)
    c.set_early_miss(early)
    c.set_overlap(overlap)
    if schedule:
        c.set_schedule(**schedule)
    c.upload(desc)
    return c


# ------------------------------------------------------------- the defining equality
def white_scene(g, name, variant):
    """(desc, camera, wall ids, builder): the white-walled scene plus a small
    white triangle in front of the far wall, so that the world BVH keeps
    something and the world quads can be lifted."""
    case = SC.white(name, variant)
    b, _, cam, ids = case.build(g, variant)
    tri = b.triangle((1.55, -1.4, -2.9), (1.75, -1.4, -2.9), (1.65, -1.25, -2.9), b.lambertian((1, 1, 1)))
    sc = case.scene(variant)
    walls = [ids[k] for k, ob in enumerate(sc.objects) if ob["kind"] == "quad" and ob["mat"]["kind"] == "lambertian"]
    for k in walls:                            # the equality is stated for axis-aligned normals
        n = np.cross(sc.objects[ids.index(k)]["u"], sc.objects[ids.index(k)]["v"])
        assert np.count_nonzero(n) == 1
    return b.desc(b.listing(list(ids) + [tri])), cam, walls, b


# The share of the grid camera's rays that must be compared: 3/4 where only the
# lamps, the blocker and the small triangle take rays away.  fog_shadow's slab
# (density 0.5, 1 unit thick, crossed over 1 to 1.35 units) scatters a ray with
# probability 1 - exp(-0.5 l), 0.39 to 0.49, and such a ray's closest hit is the
# volume: about half of the 384 rays are left (binomial sigma 0.026), held to 1/3.
SHARE, SHARE_FOG = 0.75, 1.0 / 3.0


def check_equality(g, c, cam, walls, depths, what, wall_normal=None):
    n = cam.image_width * cam.image_height
    compared = 0
    lit = False
    for s in (0, 1):
        top_e, _, t_e, ray = c.extend_hits(cam, PC.SEED, s, 0)
        o, d = np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6])
        if wall_normal is None:
            top, _, t, _, nrm, _ = c.trace_rays(o, d)
        else:                                  # a scene with a volume: k_extend's own record, the wall's normal
            top, t, nrm = top_e, t_e, np.tile(np.float32(wall_normal), (n, 1))
        sel = np.flatnonzero(np.isin(top, walls))
        assert len(sel) >= (SHARE if wall_normal is None else SHARE_FOG) * n, f"{what}: only {len(sel)} of {n} rays meet a wall"
        t = t.astype(np.float32)
        P = (o[sel] + (d[sel] * t[sel, None]).astype(np.float32)).astype(np.float32)
        ids = sel.astype(np.uint32)            # the pixel index: the camera ray's key
        pts = g.make_gather_points(P, nrm[sel], ids=ids)
        rays = g.make_path_rays(o[sel], d[sel], ids=ids)
        for depth in depths:
            want, _ = c.ray_color(rays, 1, depth, seed=PC.SEED, sample_offset=s, camera=cam)
            got, st = c.gather_surface(pts, 1, depth, seed=PC.SEED, sample_offset=s, camera=cam)
            assert st.invalid_rays == 0 and st.samples == len(sel)
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
            assert len(bad) == 0, (f"{what} depth {depth} sample {s}: {len(bad)} of {len(sel)} points differ from "
                                   f"rt_ray_color, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}")
            assert np.isfinite(got).all()
            lit = lit or bool((got > 0).any())
            compared += len(sel)
    assert lit, f"{what}: an empty result shows nothing"
    c.sync()                                   # raises on a device error
    return compared


EQUAL = [
    ("room", "d6", dict()), ("room", "d6", dict(nodes="quant8")), ("room", "d6", dict(nodes="wide8")),
    ("room", "d6", dict(lifted=False)), ("room", "d6", dict(nodes="quant8", lifted=False)),
    ("room", "d6", dict(nodes="wide8", lifted=False)),
    ("room", "d6", dict(early=1)), ("room", "d6", dict(early=2)), ("room", "d6", dict(overlap=2)),
    ("room", "d6", dict(streams=1)), ("room", "d6", dict(streams=3)), ("room", "d6", dict(batch_slots=100)),
    ("room", "d6", dict(early=2, overlap=2, streams=3, batch_slots=64)),
    ("lights3", "", dict()), ("lights3", "", dict(nodes="quant8", early=2)), ("lights3", "", dict(lifted=False)),
    ("sphere_in_list", "", dict()), ("sphere_in_list", "", dict(early=1, batch_slots=100)),
    ("env_is_area", "", dict()), ("env_is_area", "", dict(nodes="quant8", early=2, overlap=2)),
    ("env_is_area", "", dict(lifted=False, streams=3)),
    ("fog_shadow", "", dict()), ("fog_shadow", "", dict(volumes_in_bvh=True)),
    ("fog_shadow", "", dict(volumes_in_bvh=True, early=2, batch_slots=100)),
]


@pytest.mark.parametrize("name,variant,opts", EQUAL,
                         ids=[n + "".join(f"-{k}={v}" for k, v in o.items()) for n, _, o in EQUAL])
def test_surface_equals_ray_color_at_the_hit(g, name, variant, opts):
    desc, cam, walls, _keep = white_scene(g, name, variant)
    c = make_context(g, desc, **opts)
    try:
        fog = name == "fog_shadow"
        if fog:
            assert c.info().volumes > 0
        elif opts.get("lifted", True):
            assert c.lifted_prims() > 0
        else:
            assert c.lifted_prims() == 0
        check_equality(g, c, cam, walls, (1, 2, 5), f"{name} {opts}", wall_normal=(0, 0, 1) if fog else None)
    finally:
        c.close()


# ------------------------------------------------------------- the rows against float64
# every row under the defaults; fog_shadow with its volume in the BVH too
ROW_RUNS = [(r, "default") for r in SC.ROWS] + [(SC.BY_LABEL["fog_shadow"], "in_bvh")]


@pytest.mark.parametrize("row,mode", ROW_RUNS, ids=[f"{r.label}-{m}" for r, m in ROW_RUNS])
def test_rows_against_the_reference(g, row, mode):
    e = row.expected(g)
    print(row.summary(g))
    desc, cam = row.build(g)
    c = make_context(g, desc, volumes_in_bvh=mode == "in_bvh")
    try:
        pts = g.make_gather_points(e["P"], e["N"], ids=e["ids"])
        L, st = c.gather_surface(pts, e["samples"], e["depth"], seed=SC.SEED, camera=cam)
        c.sync()
    finally:
        c.close()
    atol, _ = radiance_bar(row.group, "device")
    ok = e["L_ok"]
    err = float(np.abs(L.astype(np.float64)[ok] - e["L"][ok]).max())
    print(f"{row.label} {mode} GPU: radiance worst |err| {err:.3g} (bar {atol:.3g})")
    assert st.invalid_rays == 0
    assert err <= atol, f"{row.label} {mode}: radiance off by {err} (bar {atol})"


# ------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def lucy(g):
    """The reduced cornell-lucy of the gather tests, NP surface points, and
    their NS-sample surface sums from one default call."""
    s = scene(g, "cornell-lucy")
    c = make_context(g, s.desc)
    try:
        _, _, _, ray = c.extend_hits(s.camera, SEED, 0, 0)
        o, d = ray[100:100 + NP, 0:3], ray[100:100 + NP, 3:6]
        top, prim, t, mat, n, flags = c.trace_rays(o, d)
        hit = top >= 0
        assert hit.sum() > NP // 2
        p = (o + t[:, None] * d).astype(np.float32)
        p[~hit] = (278.0, 278.0, 278.0)
        n = n.copy()
        n[~hit] = (0.0, 0.0, 1.0)
        pts = g.make_gather_points(p, n, ids=np.arange(NP) + 1000)
        depth = s.camera.max_depth
        rgb, st = c.gather_surface(pts, NS, depth, seed=SEED, camera=s.camera)
        assert st.samples == NS * NP and st.invalid_rays == 0
        c.sync()
    finally:
        c.close()
    for a in (pts, rgb):
        a.setflags(write=False)
    assert np.isfinite(rgb).all() and (rgb > 0).any()
    return s, pts, depth, rgb


SCHEDULES = [dict(batch_slots=1), dict(batch_slots=2 * NP + 3), dict(streams=1), dict(streams=3), dict(max_blocks=1),
             dict(early=1), dict(early=2), dict(overlap=2), dict(overlap=2, early=2, streams=3, batch_slots=500),
             dict(nodes="quant8"), dict(nodes="wide8"), dict(lifted=False)]


@pytest.mark.parametrize("sched", SCHEDULES, ids=["".join(f"{k}={v} " for k, v in o.items()).strip() for o in SCHEDULES])
def test_schedule_invariance(g, lucy, sched):
    s, pts, depth, rgb = lucy
    c = make_context(g, s.desc, **sched)
    try:
        got, _ = c.gather_surface(pts, NS, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == rgb.tobytes(), sched
        c.sync()
    finally:
        c.close()


def test_sums_over_samples_and_calls(g, lucy):
    s, pts, depth, _ = lucy
    c = make_context(g, s.desc)
    try:
        five, _ = c.gather_surface(pts, 5, depth, seed=SEED, camera=s.camera)
        one = [c.gather_surface(pts, 1, depth, seed=SEED, sample_offset=k, camera=s.camera)[0] for k in range(5)]
        tot = np.zeros(five.shape, np.float64)
        for a in one:                                     # fp64, in sample order, rounded once
            tot = tot + a.astype(np.float64)
        assert tot.astype(np.float32).tobytes() == five.tobytes()
        assert all(a.tobytes() != one[0].tobytes() for a in one[1:])
        first, _ = c.gather_surface(pts, 2, depth, seed=SEED, camera=s.camera)
        both, _ = c.gather_surface(pts, 3, depth, seed=SEED, sample_offset=2, camera=s.camera, accum=first.copy())
        want = (((one[2].astype(np.float64) + one[3].astype(np.float64)) + one[4].astype(np.float64))
                + first.astype(np.float64)).astype(np.float32)
        assert both.tobytes() == want.tobytes()
        c.sync()
    finally:
        c.close()


def test_device_variant_on_a_stream(g, lucy):
    import torch
    s, pts, depth, rgb = lucy
    c = make_context(g, s.desc)
    try:
        p = g.surface_params(NS, depth, seed=SEED, camera=s.camera)
        st = torch.cuda.Stream(device=0)
        with torch.cuda.stream(st):
            d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint32).reshape(NP, 8).view(np.int32).copy()).to("cuda:0")
            d_rgb = torch.full((NP, 3), 7.0, dtype=torch.float32, device="cuda:0")
            d_rgb2 = torch.full((NP, 3), 7.0, dtype=torch.float32, device="cuda:0")
            c.gather_surface_device(d_pts.data_ptr(), NP, p, d_rgb.data_ptr(), stream=st.cuda_stream)
        c.gather_surface_device(d_pts.data_ptr(), NP, p, d_rgb2.data_ptr(), stream=torch.cuda.default_stream(0).cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        c.sync()
        assert c.last_render_kernel_ms() > 0.0
        assert d_rgb.cpu().numpy().tobytes() == rgb.tobytes()
        assert d_rgb2.cpu().numpy().tobytes() == rgb.tobytes()
    finally:
        c.close()


def test_ids(g, lucy):
    s, pts, depth, rgb = lucy
    c = make_context(g, s.desc)
    try:
        perm = np.random.default_rng(5).permutation(NP)
        got, _ = c.gather_surface(pts[perm], NS, depth, seed=SEED, camera=s.camera)
        assert got.tobytes() == rgb[perm].tobytes()       # the id travels with the point; the slot is where it lies
        k = int(np.argmax(rgb.sum(axis=1)))
        trio = np.repeat(pts[k:k + 1], 3)
        trio["id"][2] = trio["id"][0] + 12345
        got, _ = c.gather_surface(trio, NS, depth, seed=SEED, camera=s.camera)
        assert got[0].tobytes() == got[1].tobytes() == rgb[k].tobytes()
        assert got[2].tobytes() != got[0].tobytes()
        c.sync()
    finally:
        c.close()


def test_invalid_points(g, lucy):
    s, pts, depth, rgb = lucy
    n = NP
    where = [0, 63, 64, 255, 256, n - 1]
    bad = np.array(pts[:n])
    bad["p"][0, 1] = np.nan
    bad["p"][63, 0] = np.inf
    bad["n"][64] = 0.0
    bad["n"][255] = (1e-30, 0.0, 0.0)                     # its fp32 length is 0
    bad["n"][256, 0] = np.nan
    bad["p"][n - 1, 2] = -np.inf
    c = make_context(g, s.desc)
    try:
        got, st = c.gather_surface(bad, NS, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 6
        assert not got[where].any()
        keep = np.setdiff1d(np.arange(n), where)
        assert got[keep].tobytes() == rgb[keep].tobytes()
        # a normal that is not unit is the same vertex: unit(n) is what is shaded
        scaled = np.array(pts[:n])
        scaled["n"] *= np.float32(4.0)                    # a power of two: unit(4 n) is unit(n) bit for bit
        got, st = c.gather_surface(scaled, NS, depth, seed=SEED, camera=s.camera)
        assert st.invalid_rays == 0 and got.tobytes() == rgb.tobytes()
        c.sync()
    finally:
        c.close()


def test_closed_forms(g):
    """One far Lambertian quad, no lights, a constant background: points that
    face away from the quad scatter into the open (d.y >= 0 for every direction
    of the hemisphere about +y), so at depth 2 each sample is exactly float(B)
    and at depth 1 nothing is traced and nothing is added."""
    B = (0.25, 0.5, 0.75)
    b = Builder(g)
    desc = b.desc(b.listing([b.quad((-1, -50, -1), (2, 0, 0), (0, 0, 2), b.lambertian((0.5, 0.5, 0.5)))]))
    rng = np.random.default_rng(2)
    n = 3 * 256 + 5
    p = np.zeros((n, 3), np.float32)
    p[:, 0], p[:, 2] = rng.uniform(-100, 100, n), rng.uniform(-100, 100, n)
    pts = g.make_gather_points(p, np.tile(np.float32([0, 3, 0]), (n, 1)))
    c = g.Context(0)
    try:
        c.upload(desc)
        rgb, st = c.gather_surface(pts, 4, 2, seed=SEED, background=B, use_sky_gradient=0)
        assert st.invalid_rays == 0 and st.samples == 4 * n
        assert rgb.tobytes() == np.tile(4 * np.float32(B), (n, 1)).tobytes()
        rgb, _ = c.gather_surface(pts, 4, 1, seed=SEED, background=B, use_sky_gradient=0)
        assert rgb.tobytes() == np.zeros((n, 3), np.float32).tobytes()
        c.sync()
    finally:
        c.close()


def test_refusals(g):
    s = scene(g, "cornell")
    pts = g.make_gather_points(np.full((2, 3), 278.0), np.array([[0, 0, 1], [0, 1, 0]]))
    lib = g.rtgpu()
    c = g.Context(0)
    try:
        with pytest.raises(g.RTError) as ex:
            c.gather_surface(pts, 1, 2)
        assert ex.value.code == -5                        # RT_ERR_NO_SCENE
        c.upload(s.desc)
        rgb, _ = c.gather_surface(pts, 1, 2, camera=s.camera)
        assert np.isfinite(rgb).all()
        pp = pts.ctypes.data_as(C.POINTER(g.RtGatherPoint))
        op = rgb.ctypes.data_as(C.POINTER(C.c_float))

        def status(n=2, pts_p=pp, rgb_p=op, reserved=(0, 0), **over):
            p = g.surface_params(1, 2)
            p.reserved[0], p.reserved[1] = reserved
            for k, v in over.items():
                if k == "background":
                    p.path.background[0] = v
                else:
                    setattr(p.path, k, v)
            return lib.rt_gather_surface(c._h, pts_p, n, C.byref(p), rgb_p, None)

        assert status() == 0 and status(n=0) == 0
        assert status(pts_p=None) == -1 and status(rgb_p=None) == -1
        assert lib.rt_gather_surface(c._h, pp, 2, None, op, None) == -1
        assert lib.rt_gather_surface(None, pp, 2, C.byref(g.surface_params(1, 2)), op, None) == -1
        assert status(reserved=(1, 0)) == -1 and status(reserved=(0, 7)) == -1
        assert status(n=-1) == -1 and status(n=1 << 31) == -1
        for over in (dict(samples=0), dict(max_depth=0), dict(sample_offset=-1), dict(camera_max_depth=-1),
                     dict(background=float("nan")), dict(background=float("inf"))):
            assert status(**over) == -1, over
        marked = pts.copy()
        marked["reserved"][1] = 1
        assert status(pts_p=marked.ctypes.data_as(C.POINTER(g.RtGatherPoint))) == -1
        p = g.surface_params(1, 2)
        assert lib.rt_gather_surface_device(c._h, None, 1, C.byref(p), C.c_void_p(16), None) == -1
        assert lib.rt_gather_surface_device(c._h, C.c_void_p(16), 1, C.byref(p), None, None) == -1
        assert lib.rt_gather_surface_device(c._h, C.c_void_p(16), 1, None, C.c_void_p(16), None) == -1
        assert lib.rt_gather_surface_device(c._h, C.c_void_p(16), 0, C.byref(p), C.c_void_p(16), None) == 0
        assert lib.rt_gather_surface_device(c._h, C.c_void_p(16), -1, C.byref(p), C.c_void_p(16), None) == -1
        p.reserved[1] = 2
        assert lib.rt_gather_surface_device(c._h, C.c_void_p(16), 1, C.byref(p), C.c_void_p(16), None) == -1
        # rt_gather itself is unchanged: the surface gather is no fourth source
        q = g.gather_params(3, 1, 2)
        assert lib.rt_gather(c._h, pp, 2, C.byref(q), op, None) == -1
        c.sync()
    finally:
        c.close()
