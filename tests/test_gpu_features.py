"""rt_render_features on the GPU: the per-sample albedo / normal / depth /
coverage at the camera ray's closest hit, against the existing probes, the
scene description and the fp32 oracle's rays; the sums' arithmetic; schedule
and node-format independence; no effect on renders."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 37
FP32_OFF = 1e-3   # cap on pixels whose checker cell flips within fp32 of a cell edge
F = np.float32


@contextlib.contextmanager
def context(g, scene, nodes=None, volumes=None):
    c = g.Context(0)
    try:
        if nodes:
            c.set_node_format(nodes)
        if volumes is not None:
            c.set_option(g.RT_OPT_VOLUMES, volumes)
        c.upload(scene.desc)
        yield c
    finally:
        c.close()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def one_sample(c, g, cam, s, seed=SEED):
    f, _ = c.render_features(cam, g.make_params(1, 1, seed=seed, sample_offset=s))
    return f.reshape(-1, 8)


def materials(g, scene):
    """Per material: (kind, solid albedo as float32 or None)."""
    d = scene.desc.contents
    out = []
    for i in range(d.num_materials):
        m = d.materials[i]
        alb = None
        if m.kind in (g.RT_LAMBERTIAN, g.RT_ISOTROPIC, g.RT_DIFFUSE_LIGHT):
            t = d.textures[m.texture]
            if t.kind == g.RT_TEX_SOLID:
                alb = np.array(list(t.albedo), F)
        elif m.kind == g.RT_METAL:
            alb = np.array(list(m.albedo), F)
        elif m.kind == g.RT_DIELECTRIC:
            alb = np.ones(3, F)
        out.append((m.kind, alb))
    return out


def covered_mask(g, scene, top, prim):
    """Pixels whose first hit is a non-emissive material."""
    hs = scene.hittables()
    kinds = np.array([k for k, _ in materials(g, scene)], np.int32)
    hit = top >= 0
    mat = np.where(hit, hs["material"][np.maximum(prim, 0)], 0)
    return hit & (kinds[mat] != g.RT_DIFFUSE_LIGHT), mat


@pytest.mark.parametrize("name,width", [("cornell", 64), ("random", 96)])
def test_depth_and_coverage_match_the_probes(g, O, name, width):
    s = g.Scene(name, width=width)
    cam = s.camera
    with context(g, s) as c:
        for smp in (0, 3):
            f = one_sample(c, g, cam, smp)
            top, prim, t = c.extend_first_hits(cam, SEED, smp)
            cov, _ = covered_mask(g, s, top, prim)
            assert 0.2 < cov.mean()
            assert np.array_equal(f[:, 7], cov.astype(F))
            assert np.array_equal(bits(f[cov, 6]), bits(t[cov]))
            assert not f[~cov].any()
            to, po, t_o = O.primary_hits(s.desc, cam, SEED, smp, fp32=True)
            assert np.array_equal(top, to) and np.array_equal(prim, po)
            assert np.array_equal(bits(f[cov, 6]), bits(t_o[cov].astype(F)))


def expected_normals(g, scene, top, prim, ray, P):
    """(mask, instanced, normals) for the pixels this restatement covers:
    spheres at rest, quads and planes in the world, and quads under cornell's
    Translate(RotateY(box)) chain."""
    hs = scene.hittables()
    n = top.size
    exp = np.zeros((n, 3), np.float64)
    mask = np.zeros(n, bool)
    inst = np.zeros(n, bool)
    rd = ray[:, 3:6]
    for p in np.flatnonzero(top >= 0):
        h = hs[prim[p]]
        d = rd[p]
        if top[p] == prim[p]:
            if h["kind"] == g.RT_SPHERE and not np.any(h["p"][3:6]):
                # from the fp32 hit point, in fp32 like sphere.go:60-62 on the device (the
                # point's own rounding, ~1e-6 of its distance, is part of both sides)
                out = ((P[p].astype(F) - h["p"][0:3].astype(F)) / F(h["p"][6])).astype(np.float64)
            elif h["kind"] == g.RT_QUAD:
                out = h["p"][12:15]
            elif h["kind"] == g.RT_PLANE:
                out = h["p"][3:6]
            else:
                continue
            exp[p] = out if np.dot(d, out) < 0 else -out
            mask[p] = True
        else:
            tr = hs[top[p]]
            if tr["kind"] != g.RT_TRANSLATE or hs[tr["a"]]["kind"] != g.RT_ROTATE_Y or h["kind"] != g.RT_QUAD:
                continue
            sn, cs = hs[tr["a"]]["p"][0], hs[tr["a"]]["p"][1]
            dobj = np.array([cs * d[0] - sn * d[2], d[1], sn * d[0] + cs * d[2]])   # transform.go:131-140
            no = h["p"][12:15]
            no = no if np.dot(dobj, no) < 0 else -no
            exp[p] = [cs * no[0] + sn * no[2], no[1], -sn * no[0] + cs * no[2]]      # transform.go:155-160
            mask[p] = inst[p] = True
    return mask, inst, exp


def test_normals_cornell(g, O):
    s = g.Scene("cornell", width=64)
    cam = s.camera
    with context(g, s) as c:
        f = one_sample(c, g, cam, 0)
        top, prim, _ = c.extend_first_hits(cam, SEED, 0)
    _, _, _, ray, _ = O.path_records(s.desc, cam, SEED, 0, 2, fp32=True)
    cov, _ = covered_mask(g, s, top, prim)
    mask, inst, exp = expected_normals(g, s, top, prim, ray[0], ray[1][:, 0:3])
    mask &= cov
    inst &= cov
    assert mask.sum() > 0.5 * cov.sum() and inst.sum() > 50
    nrm = f[:, 3:6].astype(np.float64)
    err = np.abs(nrm[mask] - exp[mask]).max()
    print(f"cornell normals: {mask.sum()} pixels ({inst.sum()} instanced), max |d| {err:.2e}")
    assert err <= 1e-5
    assert np.abs(np.linalg.norm(nrm[inst], axis=1) - 1.0).max() <= 1e-5
    assert (np.sum(nrm[inst] * ray[0][inst, 3:6], axis=1) < 0).all()
    # the fog (a Volume) reports volume.go:72-76's normal
    hs = s.hittables()
    vol = cov & (hs["kind"][np.maximum(prim, 0)] == g.RT_VOLUME)
    if vol.any():
        assert np.array_equal(f[vol, 3:6], np.tile(np.array([1, 0, 0], F), (vol.sum(), 1)))


def test_normals_spheres(g, O):
    s = g.Scene("random", width=96)
    cam = s.camera
    with context(g, s) as c:
        f = one_sample(c, g, cam, 0)
        top, prim, _ = c.extend_first_hits(cam, SEED, 0)
    otop, _, _, ray, _ = O.path_records(s.desc, cam, SEED, 0, 2, fp32=True)
    cov, mat = covered_mask(g, s, top, prim)
    scattered = cov & (otop[1] != -2)     # P = the scattered ray's origin
    mask, _, exp = expected_normals(g, s, top, prim, ray[0], ray[1][:, 0:3])
    mask &= scattered
    hs = s.hittables()
    spheres = mask & (hs["kind"][np.maximum(prim, 0)] == g.RT_SPHERE)
    assert mask.sum() > 2000 and spheres.sum() > 300   # the ground plane; the spheres that do not move
    err = np.abs(f[mask, 3:6].astype(np.float64) - exp[mask]).max()
    print(f"random normals: {mask.sum()} pixels, max |d| {err:.2e}")
    assert err <= 1e-5


@pytest.fixture(scope="module")
def rotations(g, O):
    """cornell-rotations (RotateX / RotateZ / RotateY / Scale chains): one
    sample's features, the hit ids, the hittables and the camera rays."""
    s = g.Scene("cornell-rotations", width=64)
    cam = s.camera
    with context(g, s) as c:
        f = one_sample(c, g, cam, 0)
        top, prim, _ = c.extend_first_hits(cam, SEED, 0)
    _, _, _, ray, _ = O.path_records(s.desc, cam, SEED, 0, 1, fp32=True)
    return f, top, prim, s.hittables(), ray[0], g


def test_normals_rotations_unit_and_facing(rotations):
    """Every covered pixel's normal is unit within 1e-5 and faces the camera
    ray, spheres and the RotateX / RotateZ chains included (the integrator's
    own normal does neither there: features.hip instance_normal)."""
    f, top, prim, hs, ray, g = rotations
    cov = f[:, 7] == 1
    assert cov.mean() > 0.5
    kind = np.where(prim >= 0, hs["kind"][np.maximum(prim, 0)], 0)
    nrm = f[:, 3:6].astype(np.float64)
    dev = np.abs(np.linalg.norm(nrm, axis=1) - 1.0)
    for k, name in ((g.RT_QUAD, "quad"), (g.RT_TRIANGLE, "triangle"), (g.RT_SPHERE, "sphere")):
        m = cov & (kind == k)
        assert m.sum() > 20
        print(f"cornell-rotations {name}: {m.sum()} pixels, max | |n| - 1 | = {dev[m].max():.2e}")
    away = np.sum(nrm * ray[:, 3:6], axis=1) >= 0
    print(f"cornell-rotations: {(cov & away).sum()} of {cov.sum()} covered pixels with n . rd >= 0")
    assert not (cov & away).any()
    assert dev[cov].max() <= 1e-5


def test_normals_rotations_match_the_chains_geometry(rotations):
    """Flat primitives under a wrapper chain: the feature normal is the
    primitive's own normal, face-forwarded against the ray taken into object
    space (transform.go's ray maps) and brought back by each wrapper's true
    inverse (a rotation's transpose, 1 / factor for Scale, renormalised),
    restated here in float64.  1e-5 absolute, the per-pixel bar for O(1)
    values."""
    f, top, prim, hs, ray, g = rotations
    rot = {g.RT_ROTATE_X: (1, 2), g.RT_ROTATE_Y: (0, 2), g.RT_ROTATE_Z: (0, 1)}   # the plane (i, j) each turns
    worst, n, seen = 0.0, 0, set()
    for p in np.flatnonzero((f[:, 7] == 1) & (top != prim)):
        h = hs[prim[p]]
        if h["kind"] not in (g.RT_QUAD, g.RT_TRIANGLE):
            continue
        chain, i = [], top[p]
        while hs[i]["kind"] in (g.RT_TRANSLATE, g.RT_SCALE, *rot):
            chain.append(hs[i])
            i = hs[i]["a"]
        d = ray[p, 3:6].copy()
        for w in chain:                       # outermost wrapper first: world -> object
            if w["kind"] == g.RT_SCALE:
                d = d * w["p"][3:6]
            elif w["kind"] in rot:            # v_i' = c v_i - s v_j, v_j' = s v_i + c v_j
                a, b = rot[w["kind"]]
                sn, cs = w["p"][0], w["p"][1]
                d[a], d[b] = cs * d[a] - sn * d[b], sn * d[a] + cs * d[b]
        no = h["p"][12:15].copy() if h["kind"] == g.RT_QUAD else h["p"][9:12].copy()
        if np.dot(d, no) >= 0:
            no = -no
        for w in reversed(chain):             # object -> world
            if w["kind"] == g.RT_SCALE:
                no = no * w["p"][3:6]
            elif w["kind"] in rot:
                a, b = rot[w["kind"]]
                sn, cs = w["p"][0], w["p"][1]
                no[a], no[b] = cs * no[a] + sn * no[b], -sn * no[a] + cs * no[b]
        no /= np.linalg.norm(no)
        worst = max(worst, np.abs(f[p, 3:6] - no).max())
        n += 1
        seen |= {int(w["kind"]) for w in chain}
    print(f"cornell-rotations: {n} wrapped flat pixels, max |d| {worst:.2e}")
    assert n > 400 and {g.RT_ROTATE_X, g.RT_ROTATE_Y, g.RT_ROTATE_Z, g.RT_SCALE, g.RT_TRANSLATE} <= seen
    assert worst <= 1e-5


def test_albedo_cornell_is_the_materials_colour(g):
    s = g.Scene("cornell", width=64)
    cam = s.camera
    with context(g, s) as c:
        f = one_sample(c, g, cam, 0)
        top, prim, _ = c.extend_first_hits(cam, SEED, 0)
    cov, mat = covered_mask(g, s, top, prim)
    mats = materials(g, s)
    exp = np.zeros((top.size, 3), F)
    for p in np.flatnonzero(cov):
        assert mats[mat[p]][1] is not None
        exp[p] = mats[mat[p]][1]
    assert len({tuple(v) for v in exp[cov]}) >= 3   # white, red, green (and the fog)
    assert np.array_equal(bits(f[:, 0:3]), bits(exp))


def test_albedo_checker(g, O):
    s = g.Scene("checkered-spheres", width=96)
    cam = s.camera
    with context(g, s) as c:
        f = one_sample(c, g, cam, 0)
        top, prim, _ = c.extend_first_hits(cam, SEED, 0)
    d = s.desc.contents
    cov, mat = covered_mask(g, s, top, prim)
    _, _, _, ray32, _ = O.path_records(s.desc, cam, SEED, 0, 2, fp32=True)
    _, _, _, ray64, _ = O.path_records(s.desc, cam, SEED, 0, 2, fp32=False)

    def cell(P, inv):   # texture.go:47-65 in float32, as tex_value
        q = np.floor(F(inv) * P.astype(F) + F(1e-4)).astype(np.int64)
        return (q.sum(axis=1) % 2) == 0

    exp = np.zeros((top.size, 3), F)
    agree = np.ones(top.size, bool)
    for p in np.flatnonzero(cov):
        m = d.materials[int(mat[p])]
        assert m.kind == g.RT_LAMBERTIAN
        t = d.textures[m.texture]
        assert t.kind == g.RT_TEX_CHECKER
        even = cell(ray32[1][p:p + 1, 0:3], t.inv_scale)[0]
        agree[p] = even == cell(ray64[1][p:p + 1, 0:3], t.inv_scale)[0]
        exp[p] = np.array(list(d.textures[t.even if even else t.odd].albedo), F)
    n = int(cov.sum())
    assert n > 2000
    # the cap holds on the CPU: fp32 and fp64 hit points name the same cell
    assert (~agree[cov]).sum() <= FP32_OFF * n, (~agree[cov]).sum()
    off = np.any(bits(f[cov, 0:3]) != bits(exp[cov]), axis=1).sum()
    print(f"checker albedo: {n} covered pixels, {off} off, fp32/fp64 cell disagreements {(~agree[cov]).sum()}")
    assert off <= FP32_OFF * n
    assert len({tuple(v) for v in f[cov, 0:3]}) == 2


@pytest.mark.parametrize("name", ["earth", "perlin"])
def test_albedo_textured_finite_and_repeatable(g, name):
    s = g.Scene(name, width=96)
    cam = s.camera
    with context(g, s) as c:
        a = one_sample(c, g, cam, 0)
        b = one_sample(c, g, cam, 0)
    assert np.isfinite(a).all() and (a[:, 7] == 1).mean() > 0.2
    assert a[:, 0:3].min() >= 0 and a[:, 0:3].max() <= 1
    assert len(np.unique(a[a[:, 7] == 1, 0])) > 16   # a texture, not one colour
    assert np.array_equal(bits(a), bits(b))


def test_sums_accumulate_and_buckets(g):
    s = g.Scene("cornell", width=64)
    cam = s.camera
    H, W = cam.image_height, cam.image_width
    with context(g, s) as c:
        singles = [one_sample(c, g, cam, k).astype(np.float64) for k in range(6)]
        f4, st = c.render_features(cam, g.make_params(4, 5, seed=SEED))
        assert st.samples == 4 * W * H
        exp4 = (singles[0] + singles[1] + singles[2] + singles[3]).astype(F)
        assert np.array_equal(bits(f4.reshape(-1, 8)), bits(exp4))
        assert not np.array_equal(singles[0][:, 6], singles[1][:, 6])   # jitter, fog: the samples differ
        # accumulate: k_finalize's expression, float(fp64 sum + double(previous))
        f6, _ = c.render_features(cam, g.make_params(2, 0, seed=SEED, sample_offset=4, accumulate=True), f4.copy())
        exp6 = ((singles[4] + singles[5]) + exp4.astype(np.float64)).astype(F)
        assert np.array_equal(bits(f6.reshape(-1, 8)), bits(exp6))
        # one bucket: everything outside it untouched
        buf = np.full((H, W, 8), F(-7.5))
        bk = [(16, 8, 24, 20)]
        fb, st = c.render_features(cam, g.make_params(4, 5, seed=SEED, buckets=bk), buf)
        assert st.samples == 4 * 24 * 20
        inside = np.zeros((H, W), bool)
        inside[8:28, 16:40] = True
        assert np.array_equal(bits(fb[inside]), bits(f4[inside]))
        assert (fb[~inside] == F(-7.5)).all()


def test_schedule_independent(g):
    s = g.Scene("cornell", width=64)
    cam = s.camera
    npix = cam.image_width * cam.image_height
    p = g.make_params(8, 5, seed=SEED)
    frames = []
    with context(g, s) as c:
        for streams in (1, 2, 3):
            for slots in (0, 3 * npix):
                c.set_schedule(slots, 0, 0, streams)
                frames.append(c.render_features(cam, p)[0])
    for k in range(1, len(frames)):
        assert np.array_equal(bits(frames[0]), bits(frames[k])), k
    assert frames[0][..., 7].max() == 8


def test_node_format_and_volume_placement_independent(g):
    s = g.Scene("cornell", width=64)
    cam = s.camera
    p = g.make_params(4, 5, seed=SEED)
    frames = {}
    for nodes in ("fp32", "quant8", "wide8"):
        with context(g, s, nodes=nodes) as c:
            frames[nodes] = c.render_features(cam, p)[0]
    assert np.array_equal(bits(frames["fp32"]), bits(frames["quant8"]))
    assert np.array_equal(bits(frames["fp32"]), bits(frames["wide8"]))
    s = g.Scene("cornell-smoke", width=64)
    cam = s.camera
    vols = []
    for placement in (g.RT_VOLUMES_LIFTED, g.RT_VOLUMES_IN_BVH):
        with context(g, s, volumes=placement) as c:
            vols.append(c.render_features(cam, p)[0])
    assert np.array_equal(bits(vols[0]), bits(vols[1]))
    assert vols[0][..., 7].max() == 4 and len(np.unique(vols[0][..., 3])) > 3   # the smoke's (1, 0, 0) among the normals


def test_renders_unaffected_and_device_variant(g):
    import torch
    s = g.Scene("cornell", width=64)
    cam = s.camera
    H, W = cam.image_height, cam.image_width
    p = g.make_params(4, 5, seed=SEED)
    with context(g, s) as c:
        before, _ = c.render(cam, p)
        host, _ = c.render_features(cam, p)
        after, _ = c.render(cam, p)
        assert np.array_equal(bits(before), bits(after)) and before.sum() > 0
        dev = torch.full((H, W, 8), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        c.render_features_device(cam, p, dev.data_ptr())
        c.sync()
        assert np.array_equal(bits(dev.cpu().numpy()), bits(host))
        again, _ = c.render(cam, p)
        assert np.array_equal(bits(before), bits(again))


def test_refusals(g):
    s = g.Scene("cornell", width=64)
    cam = s.camera
    c = g.Context(0)
    try:
        with pytest.raises(g.RTError) as e:
            c.render_features(cam, g.make_params(1, 1))
        assert e.value.code == -5   # RT_ERR_NO_SCENE
        c.upload(s.desc)
        with pytest.raises(g.RTError) as e:
            c.render_features(cam, g.make_params(0, 1))
        assert e.value.code == -1   # RT_ERR_INVALID
        with pytest.raises(g.RTError) as e:
            c.render_features(cam, g.make_params(1, 1, buckets=[(60, 0, 16, 16)]))
        assert e.value.code == -1
    finally:
        c.close()
