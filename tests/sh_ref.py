"""rt_gather_sh's projection, restated in numpy from the text of
include/rtgpu.h ("SH projection of a probe"), not from the kernel: the real SH
basis of Ramamoorthi & Hanrahan 2001 in float32, one numpy operation per
written operation (so no fused multiply-add), and the float64 sum in sample
order, rounded to float32 once.  Keys, directions and validity come from
tests/gather_ref.py.

    basis(d, bands)                                   -> (..., bands^2) float32
    project(L_per_sample, d_per_sample, valid, bands) -> (n, bands^2, 3) float32
"""
import numpy as np

from tests import gather_ref as GR

F = np.float32


def basis(d, bands):
    """Y_0 .. Y_(bands^2 - 1) at the directions d (..., 3), float32."""
    d = np.asarray(d, F)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = [np.full(x.shape, F(0.282095), F)]
    if bands >= 2:
        Y += [F(0.488603) * y, F(0.488603) * z, F(0.488603) * x]
    if bands >= 3:
        Y += [F(1.092548) * (x * y), F(1.092548) * (y * z), F(0.315392) * (F(3.0) * (z * z) - F(1.0)),
              F(1.092548) * (x * z), F(0.546274) * (x * x - y * y)]
    out = np.stack(Y, axis=-1)
    assert out.dtype == F and out.shape[-1] == bands * bands
    return out


def directions(pts, seed, sample):
    """(d (n, 3) float32, valid (n,)): the SPHERE direction of every point at
    sample index `sample`; zeros where the point is invalid."""
    r = GR.rays(pts, GR.SPHERE, seed, sample)
    return r["d"], GR.valid(np.ascontiguousarray(pts, GR.POINT_DTYPE), GR.SPHERE)


def project(L_per_sample, d_per_sample, valid, bands, previous=None):
    """sh[i, k, c] = float32(sum_s float64(L[s][i, c]) * float64(Y_k(d[s][i]))
    (+ float64(previous[i, k, c]))), the sum in the order of s; an invalid
    point contributes 0 to every coefficient."""
    valid = np.asarray(valid, bool)
    n = valid.shape[0]
    tot = np.zeros((n, bands * bands, 3), np.float64)
    for L, d in zip(L_per_sample, d_per_sample):
        L = np.asarray(L, F).reshape(n, 3)
        Y = basis(np.asarray(d, F).reshape(n, 3), bands)
        term = L.astype(np.float64)[:, None, :] * Y.astype(np.float64)[:, :, None]
        term[~valid] = 0.0
        tot = tot + term
    if previous is not None:
        tot = tot + np.asarray(previous, F).reshape(n, bands * bands, 3).astype(np.float64)
    return tot.astype(F)
