"""RT_BLAS_DEVICE (build.hip) through the C-ABI on the meshes of
tests/mesh_cases.py: the places an LBVH goes wrong, and the ways a scene
composes device-built meshes.  Marked gpu.

Every scene is a world list of a lambertian floor quad, a light quad above it
(shadow rays cross the mesh) and the mesh: a BVHNode tree over triangle()
leaves, split by index (the builder under test ignores the caller's topology;
the triangles' order is the tree's DFS order), inside a translate().

Per mesh, on a device-builder context: the first hits (top id, primitive id,
t) of every view equal the oracle's fp32 mirror bit for bit, and a 2-spp
render at the scene's depth is np.array_equal to a default (SAH) context's.
Every comparison is exact.

Coverage: a ray test sees only the triangles some ray hits first, so for the
grid, planar, collinear, skewed, outlier and large cases the test first
asserts, on the ORACLE's hits, that every triangle of the mesh is the first
hit of at least one ray of the views used (front, side, top and the case's own
views).  Two cases cannot meet that, and tests/test_device_build_host.py is
their cover:
  * duplicate: triangles 64..127 are exact copies of 0..63 and win every tie
    against them (among equal t the closed-interval primitive of the higher
    DFS rank is kept, DESIGN.md §3 "Tie rule"), so the originals are never a
    first hit and every copy is;
  * coincident: 64 nested triangles through one centre line; triangle 0, the
    innermost, is hidden behind its neighbours from every view, the other 63
    are reached.

Node, leaf and stack counts are checked by difference, so the host-built part
of a scene need not be known: two meshes of 1000 triangles (skewed, grid) in
otherwise identical scenes differ in info().nodes, .leaves and .stack_needed
by exactly the reference's (tests/lbvh_ref.py) differences."""
import numpy as np
import pytest

from tests import lbvh_ref as R
from tests import mesh_cases as M
from tests.scene_builder import Builder, pinhole
from tests.test_gpu_parity import fp32_bar

pytestmark = pytest.mark.gpu

OFF = np.array([0.5, 0.25, 0.125])      # exact in fp32: a view from the mesh's origin starts at 0 in its space
SEED, SAMPLE = 21, 1


class Scene:
    """floor + light + meshes [(Mesh, offset)]; `instances`: further offsets
    under which the FIRST mesh's BVH appears again (one BLAS, several instances)."""

    def __init__(self, g, meshes, instances=(), lo=None, hi=None):
        self.g = g
        b = self.b = Builder(g)
        mats = [b.lambertian((0.7, 0.6, 0.5)), b.lambertian((0.2, 0.5, 0.8))]
        wl = [M.bounds(m.tris)[0] + off for m, off in meshes] + [M.bounds(meshes[0][0].tris)[0] + o for o in instances]
        wh = [M.bounds(m.tris)[1] + off for m, off in meshes] + [M.bounds(meshes[0][0].tris)[1] + o for o in instances]
        self.lo = np.min(wl, axis=0) if lo is None else np.asarray(lo, float)
        self.hi = np.max(wh, axis=0) if hi is None else np.asarray(hi, float)
        c, e = 0.5 * (self.lo + self.hi), float(np.max(self.hi - self.lo))
        floor = b.quad([c[0] - 3 * e, c[1] - 3 * e, self.lo[2] - 0.25 * e], [6 * e, 0, 0], [0, 6 * e, 0],
                       b.lambertian((0.6, 0.6, 0.6)))
        light = b.quad([c[0] - 0.5 * e, c[1] - 0.5 * e, self.hi[2] + 6 * e], [e, 0, 0], [0, e, 0], b.light((60, 60, 60)))
        # (the quads keep the Builder's 1e-4 pad, the reference's: at the skewed mesh's scale, 2^20, fp32 does
        # not resolve it, and the slab test keeps the collapsed interval)
        b.lights = [light]
        self.tri_ids, self.tops = [], []
        first_root = None
        for m, off in meshes:
            ids = [b.triangle(t[0], t[1], t[2], mats[k]) for t, k in zip(m.tris, m.mats)]
            root = self._tree(ids)
            first_root = root if first_root is None else first_root
            self.tri_ids.append(np.array(ids))
            self.tops.append(b.translate(root, list(off)))
        for o in instances:
            self.tops.append(b.translate(first_root, list(o)))
        self.desc = b.desc(b.listing([floor, light] + self.tops))

    def _tree(self, ids):
        if len(ids) == 1:
            return ids[0]
        mid = len(ids) // 2
        return self.b.bvh_node(self._tree(ids[:mid]), self._tree(ids[mid:]))

    def cam(self, view, off=(0.0, 0.0, 0.0)):
        o, p00, du, dv = M.view_rays(view)
        off = np.asarray(off, float)
        return pinhole(self.g, view.res, view.res, o + off, p00 + off, du, dv, max_depth=5)

    def std_cams(self):
        return [self.cam(v) for v in (M.front(self.lo, self.hi), M.side(self.lo, self.hi), M.top(self.lo, self.hi))]


def oracle_hits(O, scene, cams):
    return [O.primary_hits(scene.desc, c, SEED, SAMPLE, fp32=True) for c in cams]


def assert_hits(ctx, cams, ref, what):
    for k, (cam, (to, po, t_o)) in enumerate(zip(cams, ref)):
        tg, pg, t_g = ctx.primary_hits(cam, SEED, SAMPLE)
        mism = np.flatnonzero((tg != to) | (pg != po))
        assert mism.size == 0, f"{what} view {k}: {mism.size} first hits differ, first {mism[:5]}"
        hit = tg >= 0
        assert hit.any()
        assert np.array_equal(t_g[hit], t_o[hit].astype(np.float32)), f"{what} view {k}: hit t differs"


def covered(ref, ids):
    seen = np.unique(np.concatenate([po for _, po, _ in ref]))
    return np.isin(ids, seen)


def contexts(g, fmt=None, devices=None):
    dev = g.Context(devices=devices) if devices else g.Context(0)
    dev.set_blas_builder("device")
    if fmt:
        dev.set_node_format(fmt)
    return dev


def assert_radiance_equals_sah(g, scene, dev, cam, what):
    host = g.Context(0)
    try:
        host.upload(scene.desc)
        p = g.make_params(2, cam.max_depth, seed=5)
        a, _ = dev.render(cam, p)
        dev.sync()   # raises on a device error
        b, _ = host.render(cam, p)
        assert np.isfinite(a).all() and a.sum() > 0
        assert np.array_equal(a, b), f"{what}: radiance differs from the SAH-built scene's"
        assert dev.info().triangles == host.info().triangles
    finally:
        host.close()


# name -> (mesh, every triangle must be some ray's first hit)
CASES = {
    **{f"grid{n}": (lambda n=n: M.grid(n), True) for n in (16, 17, 255, 256, 257, 1000)},
    "coincident": (M.coincident, False),
    "planar": (M.planar, True),
    "collinear": (M.collinear, True),
    "skewed": (M.skewed, True),
    "outlier": (M.outlier, True),
    "duplicate": (M.duplicate, False),
    "large": (M.large, True),
}

_made = {}


def made(g, O, name):
    """(scene, cameras, the oracle's hits per camera) of a case, computed once."""
    if name not in _made:
        m = CASES[name][0]()
        s = Scene(g, [(m, OFF)])
        cams = s.std_cams() + [s.cam(v, OFF) for v in m.cams]
        _made[name] = (s, cams, oracle_hits(O, s, cams))
    return _made[name]


@pytest.mark.parametrize("name", list(CASES))
def test_mesh_first_hits_and_radiance(g, O, name):
    s, cams, ref = made(g, O, name)
    cov = covered(ref, s.tri_ids[0])
    print(f"{name}: n {len(cov)}, {len(cams)} views, the oracle's rays reach {cov.mean():.4f} of the triangles")
    if CASES[name][1]:
        assert cov.all(), f"{name}: triangles {np.flatnonzero(~cov)[:10]} are no ray's first hit"
    elif name == "duplicate":
        assert cov[64:].all() and not cov[:64].any()
    else:
        assert cov[1:].all() and not cov[0]
    dev = contexts(g)
    try:
        dev.upload(s.desc)
        assert dev.last_build_ms() > 0.0
        assert_hits(dev, cams, ref, name)
        assert_radiance_equals_sah(g, s, dev, cams[0], name)
    finally:
        dev.close()


def test_counts_by_difference(g):
    """skewed against grid1000, the same floor, light and offset: info()
    differs by the reference's node, leaf and need4 differences (the scenes
    are not RotateX/Z scenes, so a stack entry is one word and stack_needed
    carries need4 as it is; the mesh is the only BLAS with nodes)."""
    infos, refs = [], []
    for make in (M.skewed, lambda: M.grid(1000)):
        m = make()
        refs.append(R.build(*M.boxes32(M.boxes64(m.tris))))
        s = Scene(g, [(m, OFF)], lo=OFF, hi=OFF + 1.5)
        dev, host = contexts(g), g.Context(0)
        try:
            dev.upload(s.desc)
            host.upload(s.desc)
            infos.append(dev.info())
            assert dev.info().triangles == host.info().triangles == 1000
        finally:
            dev.close()
            host.close()
    (a, b), (ra, rb) = infos, refs
    print(f"skewed - grid1000: nodes {ra.nodes - rb.nodes}, leaves {ra.leaves - rb.leaves}, need4 {ra.need4 - rb.need4}")
    assert ra.need4 - rb.need4 >= 20
    assert a.nodes - b.nodes == ra.nodes - rb.nodes
    assert a.leaves - b.leaves == ra.leaves - rb.leaves
    assert a.stack_needed - b.stack_needed == ra.need4 - rb.need4


def composed(g, O, scene, fmt=None, what=""):
    cams = scene.std_cams()
    ref = oracle_hits(O, scene, cams)
    dev = contexts(g, fmt)
    try:
        dev.upload(scene.desc)
        assert_hits(dev, cams, ref, what)
        assert_radiance_equals_sah(g, scene, dev, cams[0], what)
        return dev.info(), dev.last_build_ms(), cams, ref
    finally:
        dev.close()


def test_two_device_built_meshes(g, O):
    """n = 17 and n = 1000 in one world: the second job starts at non-zero
    tri_first, nodes_used and leaves_used."""
    a, b = M.grid(17), M.grid(1000)
    both = Scene(g, [(a, OFF), (b, OFF + [1.5, 0.0, 0.0])])
    info, ms, cams, ref = composed(g, O, both, what="two meshes")
    assert ms > 0.0
    for ids in both.tri_ids:
        assert covered(ref, ids).any()
    # the counts, by difference: the same world with another second mesh of 1000 triangles
    # (the host-built part, the world BVH over four objects, is the same)
    c = M.large(1000)
    other = Scene(g, [(a, OFF), (c, OFF + [1.5, 0.0, 0.0])], lo=both.lo, hi=both.hi)
    rb, rc = (R.build(*M.boxes32(M.boxes64(m.tris))) for m in (b, c))
    dev = contexts(g)
    try:
        dev.upload(other.desc)
        io = dev.info()
    finally:
        dev.close()
    print(f"second mesh: reference nodes {rb.nodes} / {rc.nodes}, leaves {rb.leaves} / {rc.leaves}")
    assert (rb.nodes, rb.leaves) != (rc.nodes, rc.leaves)
    assert info.nodes - io.nodes == rb.nodes - rc.nodes and info.leaves - io.leaves == rb.leaves - rc.leaves
    assert info.triangles == io.triangles == 1017


def test_shared_blas_two_instances(g, O):
    m = M.grid(255)
    one = Scene(g, [(m, OFF)])
    two = Scene(g, [(m, OFF)], instances=[OFF + [1.25, 0.25, 0.0]])
    i2, _, cams, ref = composed(g, O, two, what="shared BLAS")
    tops = np.unique(np.concatenate([to for to, _, _ in ref]))
    assert set(two.tops) <= set(tops.tolist())       # both instances are seen
    dev = contexts(g)
    try:
        dev.upload(one.desc)
        i1 = dev.info()
    finally:
        dev.close()
    assert i2.blases == i1.blases and i2.triangles == i1.triangles == 255 and i2.nodes == i1.nodes
    assert i2.instances == i1.instances + 1


def test_size_threshold(g, O):
    """A mesh of 15 triangles keeps the reference topology (sah_min_prims =
    16): beside a 16-triangle mesh only the latter is built on the device, and
    alone it leaves nothing to build."""
    small, least = M.grid(15), M.grid(16)
    _, ms, _, _ = composed(g, O, Scene(g, [(small, OFF), (least, OFF + [1.5, 0.0, 0.0])]), what="15 beside 16")
    assert ms > 0.0
    _, ms, _, _ = composed(g, O, Scene(g, [(small, OFF)]), what="15 alone")
    assert ms == 0.0


def test_quant8_over_device_built_nodes(g, O):
    s, cams, ref = made(g, O, "grid1000")
    dev = contexts(g, "quant8")
    try:
        dev.upload(s.desc)
        assert dev.info().node_format == g.RT_NODES_QUANT8
        assert_hits(dev, cams, ref, "quant8")
        cam, spp = cams[0], 8
        p = g.make_params(spp, cam.max_depth, seed=77)
        gpu, _ = dev.render(cam, p)
        assert np.isfinite(gpu).all()
        fp32_bar("device build, quant8", gpu, O.render(s.desc, cam, p, fp32=True), spp)
    finally:
        dev.close()


def test_wide8_falls_back_to_fp32_nodes(g, O):
    s, cams, ref = made(g, O, "grid1000")
    dev = contexts(g, "wide8")
    try:
        dev.upload(s.desc)
        assert dev.info().node_format == g.RT_NODES_FP32 and dev.info().nodes8 == 0
        assert_hits(dev, cams, ref, "wide8")
    finally:
        dev.close()


def test_reupload_on_one_context(g, O):
    sa, cams_a, ref_a = made(g, O, "grid257")
    sb, cams_b, ref_b = made(g, O, "skewed")
    dev = contexts(g)
    try:
        dev.upload(sa.desc)
        first = dev.info()
        hits = [dev.primary_hits(c, SEED, SAMPLE) for c in cams_a]
        dev.upload(sb.desc)
        assert_hits(dev, cams_b, ref_b, "second upload")
        dev.upload(sa.desc)
        third = dev.info()
        for name, _ in first._fields_:
            assert getattr(first, name) == getattr(third, name), name
        assert_hits(dev, cams_a, ref_a, "third upload")
        for c, h in zip(cams_a, hits):
            assert all(np.array_equal(x, y) for x, y in zip(dev.primary_hits(c, SEED, SAMPLE), h))
    finally:
        dev.close()


def test_two_devices(g, O):
    """A two-device context, as tests/test_gpu_multidevice.py makes them: the
    device list repeats device 0 where one GPU is visible, so nothing is
    skipped.  Each device builds its own copy (fan_out -> device_builds)."""
    s, cams, ref = made(g, O, "grid1000")
    one, two = contexts(g), contexts(g, devices=[0, 0])
    try:
        assert two.num_devices == 2
        one.upload(s.desc)
        two.upload(s.desc)
        assert two.last_build_ms() > 0.0
        p = g.make_params(2, cams[0].max_depth, seed=5)
        a, _ = one.render(cams[0], p)
        b, _ = two.render(cams[0], p)
        two.sync()
        assert np.array_equal(a, b) and a.sum() > 0
        assert_hits(two, cams, ref, "two devices")
    finally:
        two.close()
        one.close()
