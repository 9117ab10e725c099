"""rt_denoise on the GPU against the numpy restatement (tests/denoise_ref.py),
its exact properties, and what it is for: a denoised preview pass is closer
to the converged frame than the pass itself."""
import numpy as np
import pytest

from tests import denoise_ref as R

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_within_bar(got, ref, what):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bar = R.BAR * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    over = (d > bar).any(axis=-1)
    print(f"{what}: max |d| = {d.max():.3e}, worst d/bar = {(d / bar).max():.3f}, pixels over = {over.sum()}")
    assert not over.any()


@pytest.fixture(scope="module")
def cornell(g):
    return g.Scene("cornell", width=96)


@pytest.fixture(scope="module")
def cornell_frames(g, ctx, cornell):
    """4 spp depth 5 and 1 spp depth 3 with their features, and the 1024-spp
    reference of another seed (means)."""
    cam = cornell.camera
    ctx.upload(cornell.desc)
    out = {}
    for spp, depth in ((4, 5), (1, 3)):
        p = g.make_params(spp, depth, seed=5)
        out[spp] = (ctx.render(cam, p)[0], ctx.render_features(cam, p)[0])
    out["ref"] = ctx.render(cam, g.make_params(1024, 5, seed=977))[0] / F(1024)
    return out


@pytest.mark.parametrize("w,h", [(40, 24), (131, 67)])
def test_matches_reference_on_synthetic_images(ctx, w, h):
    accum, feat = R.synthetic(w, h, spp=4, seed=w)
    got = ctx.denoise(accum, feat, 4)
    assert np.isfinite(got).all() and not np.array_equal(got, accum)
    assert_within_bar(got, R.denoise_ref(accum, feat, 4), f"synthetic {w}x{h}")
    got = ctx.denoise(accum, feat, 4, demodulate=0, iterations=1)
    assert_within_bar(got, R.denoise_ref(accum, feat, 4, demodulate=0, iterations=1), f"synthetic {w}x{h} 1 pass")


def test_matches_reference_on_a_rendered_frame(ctx, cornell_frames):
    accum, feat = cornell_frames[4]
    got = ctx.denoise(accum, feat, 4)
    assert_within_bar(got, R.denoise_ref(accum, feat, 4), "cornell 96 4 spp")


def test_exact_properties(ctx):
    accum, feat = R.synthetic(131, 67, spp=4, seed=5)
    assert np.array_equal(bits(ctx.denoise(accum, feat, 4, iterations=0)), bits(accum))
    got = ctx.denoise(accum, feat, 4)
    through = feat[..., 7] / F(4) < 0.5
    assert through.sum() > 50
    assert np.array_equal(bits(got[through]), bits(accum[through]))
    assert not np.array_equal(got[~through], accum[~through])
    assert np.array_equal(bits(got), bits(ctx.denoise(accum, feat, 4)))   # two calls
    a1, f2 = R.two_regions(40, 24, right_scale=1.0)
    a2, _ = R.two_regions(40, 24, right_scale=3.0)
    o1, o2 = ctx.denoise(a1, f2, 2), ctx.denoise(a2, f2, 2)
    assert np.array_equal(bits(o1[:, :20]), bits(o2[:, :20]))
    assert not np.array_equal(o1[:, 20:], o2[:, 20:])
    assert not np.array_equal(o1[:, :20], a1[:, :20])


def test_zero_coverage_frame_comes_back_unchanged(ctx):
    accum, feat = R.synthetic(40, 24, spp=4, seed=2)
    feat[:] = 0
    assert np.array_equal(bits(ctx.denoise(accum, feat, 4)), bits(accum))


def test_device_variant_equals_host(ctx):
    import torch
    accum, feat = R.synthetic(131, 67, spp=4, seed=9)
    host = ctx.denoise(accum, feat, 4)
    a, f = torch.from_numpy(accum).to("cuda:0"), torch.from_numpy(feat).to("cuda:0")
    o = torch.zeros_like(a)
    torch.cuda.synchronize()
    ctx.denoise_device(a.data_ptr(), f.data_ptr(), 131, 67, 4, o.data_ptr())
    ctx.sync()
    assert np.array_equal(bits(o.cpu().numpy()), bits(host))


def test_refusals(g, ctx):
    accum, feat = R.synthetic(40, 24)
    for bad in (dict(iterations=9), dict(iterations=-1)):
        with pytest.raises(g.RTError) as e:
            ctx.denoise(accum, feat, 4, **bad)
        assert e.value.code == -1
    with pytest.raises(g.RTError) as e:
        ctx.denoise(accum, feat, 0)
    assert e.value.code == -1


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_denoised_previews_are_closer_to_the_converged_frame(ctx, cornell_frames):
    ref = cornell_frames["ref"]
    for spp in (4, 1):
        accum, feat = cornell_frames[spp]
        noisy = mse(accum / F(spp), ref)
        den = mse(ctx.denoise(accum, feat, spp) / F(spp), ref)
        print(f"cornell 96, {spp} spp: mse {noisy:.4e} -> {den:.4e}, ratio {den / noisy:.3f}")
        assert den < noisy


@pytest.mark.parametrize("name", ["random", "hdri-test"])
def test_quality_reported_for_specular_scenes(g, name):
    """Not asserted: the filter blurs reflections the features do not
    describe; the ratio tells users so."""
    s = g.Scene(name, width=96)
    cam = s.camera
    c = g.Context(0)
    try:
        c.upload(s.desc)
        ref = c.render(cam, g.make_params(1024, 5, seed=977))[0] / F(1024)
        p = g.make_params(4, 5, seed=5)
        accum, feat = c.render(cam, p)[0], c.render_features(cam, p)[0]
        den = c.denoise(accum, feat, 4)
    finally:
        c.close()
    assert np.isfinite(den).all()
    noisy, d = mse(accum / F(4), ref), mse(den / F(4), ref)
    print(f"{name} 96, 4 spp: mse {noisy:.4e} -> {d:.4e}, ratio {d / noisy:.3f}")
