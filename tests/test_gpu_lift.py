"""World quads and spheres lifted out of the world BVH (RT_OPT_LIFT_PRIMS) on
the device: everything a context returns is the same with the primitives
tested by the shading kernel (the default) and inside the traversal.

  * frames: cornell-lucy in the three node formats under both world builders,
    hdri-nee (HDRI importance sampling beside an area light), and the
    tests/scale_cases.py room (six walls, a light and a sphere lifted: the cap
    of eight) at scales 1 and 2^6: np.array_equal;
  * the path probe's per-bounce hit records and NEE bits;
  * rt_render_features;
  * one and three streams with lifting on;
  * rt_scene_lifted_prims.
Small pictures (64 wide, 4 spp, depth 5): the host tests
(tests/test_lift_host.py) pin the hits ray by ray; these pin that the device
kernels, their lift variants and the probes do the same.
"""
import numpy as np
import pytest

from tests import scale_cases as S

pytestmark = pytest.mark.gpu

SEED, SPP, DEPTH = 23, 4, 5
LUCY = dict(width=64, lucy_rings=30, lucy_cols=40)


def context(g, desc, lifted, nodes="fp32", tlas="sah", streams=0):
    c = g.Context(0)
    c.set_lift_prims(lifted)
    c.set_node_format(nodes)
    c.set_tlas_builder(tlas)
    if streams:
        c.set_option(g.RT_OPT_STREAMS, streams)
    c.upload(desc)
    return c


def frames(g, desc, cam, spp=SPP, depth=DEPTH, **kw):
    """(frame lifted, frame in-BVH, primitives lifted)."""
    out = []
    for lifted in (True, False):
        c = context(g, desc, lifted, **kw)
        try:
            n = c.lifted_prims()
            assert lifted or n == 0
            out.append(c.render(cam, g.make_params(spp, depth, seed=SEED))[0].copy())
            if lifted:
                count = n
        finally:
            c.close()
    return out[0], out[1], count


def expected_lift(g, desc):
    """The flattener's rule on the description: all the world's quads and
    spheres when there are 1..8 of them, another object stays, and the scene
    holds no RotateX / RotateZ."""
    d = desc.contents
    H, ch = d.hittables, d.children
    if any(H[i].kind in (g.RT_ROTATE_X, g.RT_ROTATE_Z) for i in range(d.num_hittables)):
        return 0
    tops = []

    def walk(i):
        h = H[i]
        if h.kind == g.RT_BVH_NODE and h.a != h.b:
            walk(h.a)
            walk(h.b)
        elif h.kind == g.RT_BVH_NODE:
            walk(h.a)
        elif h.kind in (g.RT_BVH_LEAF, g.RT_LIST):
            tops.extend(H[ch[h.a + k]].kind for k in range(h.b))
        else:
            tops.append(h.kind)

    walk(d.root)
    tops = [k for k in tops if k != g.RT_PLANE]
    prims = sum(k in (g.RT_QUAD, g.RT_SPHERE) for k in tops)
    return prims if 0 < prims <= 8 and len(tops) > prims else 0


@pytest.mark.parametrize("tlas", ["sah", "reference"])
@pytest.mark.parametrize("nodes", ["fp32", "quant8", "wide8"])
def test_cornell_lucy_frames_equal(g, nodes, tlas):
    s = g.Scene("cornell-lucy", **LUCY)
    on, off, n = frames(g, s.desc, s.camera, nodes=nodes, tlas=tlas)
    assert n == 6
    assert np.isfinite(on).all() and on.max() > 0
    assert np.array_equal(on, off), f"{int(np.sum(np.any(on != off, axis=2)))} pixels differ"


def test_hdri_nee_frames_equal(g):
    s = g.Scene("hdri-nee", width=64)
    on, off, n = frames(g, s.desc, s.camera, depth=s.camera.max_depth)
    assert n == expected_lift(g, s.desc), n
    assert np.array_equal(on, off), f"{int(np.sum(np.any(on != off, axis=2)))} pixels differ"


@pytest.mark.parametrize("s", [1.0, 2.0 ** 6], ids=["s2^0", "s2^6"])
def test_scale_room_frames_equal(g, s):
    room = S.room(g, s, 0)
    on, off, n = frames(g, room.desc, room.room_camera(64))
    assert n == 8    # six walls, the light, the sphere: the cap
    assert on.max() > 0
    assert np.array_equal(on, off), f"{int(np.sum(np.any(on != off, axis=2)))} pixels differ"


def test_path_records_equal(g):
    """rt_extend_hits / rt_shadow_visibility at every bounce: ids, t and ray
    bits, and the NEE bits (a ray that a lifted primitive stops is reported as
    traced and occluded, as the traversal reports it)."""
    s = g.Scene("cornell-lucy", **LUCY)
    cam = s.camera
    rec = []
    for lifted in (True, False):
        c = context(g, s.desc, lifted)
        try:
            rec.append([(c.extend_hits(cam, SEED, 0, b), c.shadow_visibility(cam, SEED, 0, b)) for b in range(DEPTH)])
        finally:
            c.close()
    stopped = 0
    for b, ((hon, non), (hoff, noff)) in enumerate(zip(*rec)):
        for name, x, y in zip(("top", "prim", "t", "ray"), hon, hoff):
            same = np.array_equal(x, y) if x.dtype != np.float32 else np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert same, f"bounce {b}: {name} differs"
        assert np.array_equal(non, noff), f"bounce {b}: {int(np.sum(non != noff))} NEE words differ"
        stopped += int(np.sum((non & 1) & ~(non >> 2) & 1))
    assert np.any(rec[0][0][0][0] >= 0) and stopped > 0


def test_features_equal(g):
    s = g.Scene("cornell-lucy", **LUCY)
    out = []
    for lifted in (True, False):
        c = context(g, s.desc, lifted)
        try:
            out.append(c.render_features(s.camera, g.make_params(SPP, 1, seed=SEED))[0].copy())
        finally:
            c.close()
    assert out[0][..., 7].max() > 0
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


def test_streams_equal(g):
    s = g.Scene("cornell-lucy", **LUCY)
    out = []
    for streams in (1, 3):
        c = context(g, s.desc, True, streams=streams)
        try:
            assert c.lifted_prims() == 6
            out.append(c.render(s.camera, g.make_params(SPP, DEPTH, seed=SEED))[0].copy())
        finally:
            c.close()
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("name,kw,want", [("cornell-lucy", LUCY, 6), ("cornell", dict(width=32), 0), ("random", dict(width=32), 0),
                                          ("hdri-test", dict(width=32), 0), ("cornell-rotations", dict(width=32), 0)])
def test_getter(g, ctx, name, kw, want):
    s = g.Scene(name, **kw)
    ctx.upload(s.desc)    # a context's default: lifted
    assert ctx.lifted_prims() == want
