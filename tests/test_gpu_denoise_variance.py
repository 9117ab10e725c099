"""rt_denoise_variance on the GPU against the numpy restatement
(tests/denoise_var_ref.py), its exact properties, and what it is for: a
4-spp frame's fireflies, which rt_denoise leaves alone, are pulled to their
neighbours, so the filtered frame is closer to the converged one."""
import numpy as np
import pytest

from tests import denoise_var_ref as R

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_within_bar(got, ref, what):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bar = R.BAR * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    over = (d > bar).any(axis=-1)
    print(f"{what}: colour max |d| = {d.max():.3e}, worst d/bar = {(d / bar).max():.3f}, pixels over = {over.sum()}")
    assert not over.any()


def assert_var_within_bar(got, ref, what):
    ref64 = ref.astype(np.float64)
    d = np.abs(got.astype(np.float64) - ref64)
    bar = R.BAR * np.maximum(np.abs(ref64), 1e-3 * ref64.max())
    over = d > bar
    print(f"{what}: variance max |d| = {d.max():.3e}, worst d/bar = {(d / bar).max():.3f}, pixels over = {over.sum()}")
    assert not over.any()


def check(ctx, accum, feat, moments, spp, what, **params):
    got, var = ctx.denoise_variance(accum, feat, moments, spp, return_variance=True, **params)
    ref, rvar = R.denoise_var_ref(accum, feat, moments, spp, **params)
    assert np.isfinite(got).all() and np.isfinite(var).all() and not np.array_equal(got, accum)
    assert_within_bar(got, ref, what)
    assert_var_within_bar(var, rvar, what)
    return got, var


@pytest.fixture(scope="module")
def cornell(g):
    return g.Scene("cornell", width=96)


@pytest.fixture(scope="module")
def cornell_frames(g, ctx, cornell):
    """4 spp depth 5 (with moments) and 1 spp depth 3 with their features,
    and the 1024-spp reference of another seed (means)."""
    cam = cornell.camera
    ctx.upload(cornell.desc)
    out = {}
    p4, p1 = g.make_params(4, 5, seed=5), g.make_params(1, 3, seed=5)
    a4, m4, _ = ctx.render_moments(cam, p4)
    out[4] = (a4, ctx.render_features(cam, p4)[0], m4)
    out[1] = (ctx.render(cam, p1)[0], ctx.render_features(cam, p1)[0], None)
    out["ref"] = ctx.render(cam, g.make_params(1024, 5, seed=977))[0] / F(1024)
    return out


@pytest.mark.parametrize("w,h", [(40, 24), (131, 67)])
def test_matches_reference_on_synthetic_images(ctx, w, h):
    accum, feat = R.synthetic(w, h, spp=4, seed=w)
    moments = R.synthetic_moments(accum, 4, seed=h)
    check(ctx, accum, feat, moments, 4, f"synthetic {w}x{h} moments")
    check(ctx, accum, feat, moments, 4, f"synthetic {w}x{h} moments, 1 pass", demodulate=0, iterations=1)
    a1, f1 = R.synthetic(w, h, spp=1, seed=w)
    check(ctx, a1, f1, None, 1, f"synthetic {w}x{h} spatial")
    check(ctx, accum, feat, moments, 4, f"synthetic {w}x{h} spatial at 4 spp", spatial_below=5, iterations=3)


def test_matches_reference_on_a_rendered_frame(ctx, cornell_frames):
    accum, feat, moments = cornell_frames[4]
    check(ctx, accum, feat, moments, 4, "cornell 96 4 spp")
    accum, feat, _ = cornell_frames[1]
    check(ctx, accum, feat, None, 1, "cornell 96 1 spp")


def test_exact_properties(ctx):
    accum, feat = R.synthetic(131, 67, spp=4, seed=5)
    moments = R.synthetic_moments(accum, 4, seed=6)
    o0, v0 = ctx.denoise_variance(accum, feat, moments, 4, return_variance=True, iterations=0)
    assert np.array_equal(bits(o0), bits(accum))
    assert_var_within_bar(v0, R.denoise_var_ref(accum, feat, moments, 4, iterations=0)[1], "initial variance")
    assert np.array_equal(bits(ctx.denoise_variance(accum, feat, moments, 4, iterations=0)), bits(accum))
    got, var = ctx.denoise_variance(accum, feat, moments, 4, return_variance=True)
    through = feat[..., 7] / F(4) < 0.5
    assert through.sum() > 50
    assert np.array_equal(bits(got[through]), bits(accum[through]))
    assert not np.array_equal(got[~through], accum[~through])
    assert (var[through] == 0).all() and (var[~through] > 0).any()
    again, var2 = ctx.denoise_variance(accum, feat, moments, 4, return_variance=True)   # two calls
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(bits(var), bits(var2))
    assert np.array_equal(bits(got), bits(ctx.denoise_variance(accum, feat, moments, 4)))   # without out_var
    # uncovered pixels are never neighbours
    a2, m2 = accum.copy(), moments.copy()
    a2[through] *= F(7.0)
    m2[through] *= F(5.0)
    got2, var3 = ctx.denoise_variance(a2, feat, m2, 4, return_variance=True)
    assert np.array_equal(bits(got2[~through]), bits(got[~through])) and np.array_equal(bits(var3), bits(var))
    for spp in (2, 4):   # spatial estimate, moments
        a1, f2 = R.two_regions(40, 24, spp=spp, right_scale=1.0)
        a2, _ = R.two_regions(40, 24, spp=spp, right_scale=3.0)
        m1, m2 = R.synthetic_moments(a1, spp, seed=8), R.synthetic_moments(a2, spp, seed=8)
        o1, v1 = ctx.denoise_variance(a1, f2, m1, spp, return_variance=True)
        o2, v2 = ctx.denoise_variance(a2, f2, m2, spp, return_variance=True)
        assert np.array_equal(bits(o1[:, :20]), bits(o2[:, :20])) and np.array_equal(bits(v1[:, :20]), bits(v2[:, :20]))
        assert not np.array_equal(o1[:, 20:], o2[:, 20:]) and not np.array_equal(v1[:, 20:], v2[:, 20:])
        assert not np.array_equal(o1[:, :20], a1[:, :20])


def test_zero_coverage_frame_comes_back_unchanged(ctx):
    accum, feat = R.synthetic(40, 24, spp=4, seed=2)
    feat[:] = 0
    got, var = ctx.denoise_variance(accum, feat, R.synthetic_moments(accum, 4, seed=1), 4, return_variance=True)
    assert np.array_equal(bits(got), bits(accum)) and (var == 0).all()


def test_device_variant_equals_host(ctx):
    import torch
    accum, feat = R.synthetic(131, 67, spp=4, seed=9)
    moments = R.synthetic_moments(accum, 4, seed=10)
    host, hvar = ctx.denoise_variance(accum, feat, moments, 4, return_variance=True)
    a, f, m = (torch.from_numpy(x).to("cuda:0") for x in (accum, feat, moments))
    o = torch.zeros_like(a)
    v = torch.full((67, 131), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.denoise_variance_device(a.data_ptr(), f.data_ptr(), m.data_ptr(), 131, 67, 4, o.data_ptr(), v.data_ptr())
    ctx.sync()
    assert np.array_equal(bits(o.cpu().numpy()), bits(host)) and np.array_equal(bits(v.cpu().numpy()), bits(hvar))
    # the spatial case without moments and without out_var
    h1 = ctx.denoise_variance(accum, feat, None, 4, spatial_below=5)
    o.zero_()
    torch.cuda.synchronize()
    ctx.denoise_variance_device(a.data_ptr(), f.data_ptr(), 0, 131, 67, 4, o.data_ptr(), spatial_below=5)
    ctx.sync()
    assert np.array_equal(bits(o.cpu().numpy()), bits(h1))


def test_refusals(g, ctx):
    import ctypes as C
    accum, feat = R.synthetic(40, 24)
    moments = R.synthetic_moments(accum, 4, seed=1)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(spatial_below=1), dict(sigma_lum=0.0)):
        with pytest.raises(g.RTError) as e:
            ctx.denoise_variance(accum, feat, moments, 4, **bad)
        assert e.value.code == -1
    with pytest.raises(g.RTError) as e:
        ctx.denoise_variance(accum, feat, moments, 0)
    assert e.value.code == -1
    with pytest.raises(g.RTError) as e:
        ctx.denoise_variance(accum, feat, None, 4)   # moments NULL while spp >= spatial_below
    assert e.value.code == -1
    # out_var overlapping an input
    dp = g.denoise_variance_params()
    out = np.zeros_like(accum)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    for alias in (accum, feat, moments):
        rc = g.rtgpu().rt_denoise_variance(ctx._h, fp(accum), fp(feat), fp(moments), 40, 24, 4, C.byref(dp), fp(out),
                                           fp(alias))
        assert rc == -1


def test_firefly_is_pulled_to_its_neighbours(ctx):
    accum, feat, moments, (fy, fx) = R.firefly(40, 24)
    plain = ctx.denoise(accum, feat, 4)
    got, var = check(ctx, accum, feat, moments, 4, "firefly")
    assert (got[fy, fx] < plain[fy, fx]).all(), (got[fy, fx], plain[fy, fx])
    assert var[fy, fx] > np.median(var)


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_against_the_converged_frame(ctx, cornell_frames):
    ref = cornell_frames["ref"]
    ratios = {}
    for spp in (4, 1):
        accum, feat, moments = cornell_frames[spp]
        noisy = mse(accum / F(spp), ref)
        den = mse(ctx.denoise(accum, feat, spp) / F(spp), ref)
        dv = mse(ctx.denoise_variance(accum, feat, moments, spp) / F(spp), ref)
        print(f"cornell 96, {spp} spp: mse {noisy:.4e}; rt_denoise {den:.4e} (ratio {den / noisy:.3f}); "
              f"rt_denoise_variance {dv:.4e} (ratio {dv / noisy:.3f})")
        assert dv < noisy
        ratios[spp] = (dv, den)
    # what the filter is for: the 4-spp frame, where the moments exist and fireflies dominate
    assert ratios[4][0] < ratios[4][1]


@pytest.mark.parametrize("name", ["random", "hdri-test"])
def test_quality_reported_for_specular_scenes(g, name):
    """Not asserted: both filters blur reflections the features do not
    describe; the ratios tell users so."""
    s = g.Scene(name, width=96)
    cam = s.camera
    c = g.Context(0)
    try:
        c.upload(s.desc)
        ref = c.render(cam, g.make_params(1024, 5, seed=977))[0] / F(1024)
        p = g.make_params(4, 5, seed=5)
        accum, moments, _ = c.render_moments(cam, p)
        feat = c.render_features(cam, p)[0]
        den = c.denoise(accum, feat, 4)
        dv = c.denoise_variance(accum, feat, moments, 4)
    finally:
        c.close()
    assert np.isfinite(dv).all()
    noisy, d, v = mse(accum / F(4), ref), mse(den / F(4), ref), mse(dv / F(4), ref)
    print(f"{name} 96, 4 spp: mse {noisy:.4e}; rt_denoise ratio {d / noisy:.3f}; rt_denoise_variance ratio {v / noisy:.3f}")
