"""Ray sets no camera of ours produces, for rt_ray_color, and their float64
expectation: plain data and tests/path_ref.py's rayColorInternal.

Two sets on the 24 x 16 index grid k = j * 24 + i, id = 1000 + 7 k, 2 samples,
seed 3:

  ortho: o = (-1.8 + 3.6 (i + .5) / 24, 1.3 - 2.6 (j + .5) / 16, 0.5),
         d = (0.1, -0.06, -2): one origin per ray, a skewed direction that is
         not unit;
  probe: o = (0.3, -0.2, -0.5), d = 0.5 (sin th cos ph, cos th, sin th sin ph),
         th = (j + .5) pi / 16, ph = (i + .5) 2 pi / 24: every direction from a point.

over rows of tests/path_cases.py, each at its own depth.  The rays are rounded
to float32 first (what the device is given) and the reference follows those
float32 rays in float64.  Expected value of ray k's sample s:
path_ref.ray_color(scene, (o, d, time), depth, True, (seed, id, s)) with
time = shade_ref.rnd(seed, id, s, 0, DOM_CAMERA, 2), the key's camera-domain
time draw.  A ray-sample whose Path.margin < 1 is left out (at most
path_cases.LEFT_OUT_CAP of a row's, asserted here on the reference alone),
and so is the ray's sum.

Consumers: tests/test_ray_color_kat.py (the oracle through a degenerate
camera, the host pipeline) and tests/test_gpu_ray_color.py (the C-ABI)."""
import numpy as np

from tests import path_cases as PC
from tests import path_ref as P
from tests import shade_ref as R

GW, GH = 24, 16
N = GW * GH
SEED, SAMPLES = 3, 2
IDS = (1000 + 7 * np.arange(N)).astype(np.uint32)

ROWS = [("room", "d3"), ("lights3", ""), ("glass_chain", "glass"), ("mirror_chain", "mirror"), ("env_gate", "env+light"),
        ("phantom", "at_max"), ("phantom", "below"), ("fog_shadow", ""), ("clamp_b1", "")]
SETS = ("ortho", "probe")


def ray_set(name):
    """(o, d): (N, 3) float32 each."""
    k = np.arange(N)
    i, j = (k % GW).astype(np.float64), (k // GW).astype(np.float64)
    if name == "ortho":
        o = np.stack([-1.8 + 3.6 * (i + 0.5) / GW, 1.3 - 2.6 * (j + 0.5) / GH, np.full(N, 0.5)], axis=1)
        d = np.tile(np.array([0.1, -0.06, -2.0]), (N, 1))
    elif name == "probe":
        th, ph = (j + 0.5) * np.pi / GH, (i + 0.5) * 2.0 * np.pi / GW
        o = np.tile(np.array([0.3, -0.2, -0.5]), (N, 1))
        d = 0.5 * np.stack([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)], axis=1)
    else:
        raise KeyError(name)
    return o.astype(np.float32), d.astype(np.float32)


def depth_of(name, variant):
    return PC.CASES[name].variants[variant][0]


def params_of(g, name, variant):
    """The rt_ray_color_params fields rayColorInternal reads, from the row's camera."""
    cam = PC.CASES[name].camera(g, variant)
    return dict(camera=cam)


_EXP = {}


def expected(name, variant, rset):
    """Computed once, read-only: depth; L (N, 3) the sum of the samples; L_ok
    (N) every sample of the ray decided; paths[s][k]; left_out; bounces: the
    mean number of rays per path; b0_miss: ray-samples that miss at bounce 0."""
    key = (name, variant, rset)
    if key in _EXP:
        return _EXP[key]
    sc = PC.CASES[name].scene(variant)
    depth = depth_of(name, variant)
    o32, d32 = ray_set(rset)
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    e = dict(depth=depth, samples=SAMPLES, L=np.zeros((N, 3)), L_ok=np.ones(N, bool), paths=[], scene=sc)
    left = nb = miss = 0
    for s in range(SAMPLES):
        paths = []
        for k in range(N):
            pid = int(IDS[k])
            time = R.rnd(SEED, pid, s, 0, R.DOM_CAMERA, 2)
            pa = P.Path()
            pa.L = P.ray_color(sc, (o[k], d[k], time), depth, True, (SEED, pid, s), pa)
            e["L"][k] += pa.L
            if pa.margin < 1:
                e["L_ok"][k] = False
                left += 1
            nb += len(pa.bounces)
            miss += pa.bounces[0]["obj"] == -1
            paths.append(pa)
        e["paths"].append(paths)
    e["left_out"], e["bounces"], e["b0_miss"] = left, nb / (N * SAMPLES), int(miss)
    assert left <= PC.LEFT_OUT_CAP * N * SAMPLES, f"{name}[{variant}] {rset}: {left} of {N * SAMPLES} ray-samples left out"
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _EXP[key] = e
    return e


def summary(name, variant, rset):
    e = expected(name, variant, rset)
    return (f"{name}[{variant}] {rset} depth {e['depth']}: left_out {e['left_out']} / {N * SAMPLES} "
            f"b0_miss {e['b0_miss']} mean bounces {e['bounces']:.3f} mean radiance {e['L'].mean() / SAMPLES:.4f}")
