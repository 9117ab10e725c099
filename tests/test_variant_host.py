"""CPU checks of the kernel-variant rule and the scene scalars it reads.

wave_variant.h states once which variant of the wavefront kernels a scene
runs (pick_variant) and turns that into template arguments (with_nodes,
with_shading); flatten.cpp scene_scalars derives once every scalar of the
kernels' DScene.  The product and the host emulations of the kernels all go
through them.  tests/variant_probe.cpp (plain g++, no GPU) checks:

* the dispatchers hand the functor constants equal to the runtime fields for
  every variant, reach exactly the 36 + 24 template tuples that exist, and
  never instantiate an 8-wide rare-primitive kernel;
* the rule gives, for every scene x node format x lifting, what the code gave
  before it was gathered in one place (PARENT, recorded from that code);
* scene_scalars refuses lifted primitives in a scene that shades in a variant
  without the lifted-primitive code.
"""
import json
import os
import shutil
import subprocess

import pytest

from tests.test_flatten_host import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")
ASSETS = os.path.join(ROOT, "assets")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# Per scene at width 40, for node format asked 0 / 1 / 2 x lift_prims 0 / 1:
# (node format asked, lift_prims, shade_kind, the rare-primitive (vol) bit,
# node format run, envis, lifted primitive records, shade_kind | SHADE_LIFT),
# as the hand-written rules computed them before wave_variant.h and
# scene_scalars replaced them (the host emulation's scene loader with the
# lifted records patched in, run_variant's and launch_wavefront's expressions).
PARENT = {
    "simple": [
        (0, 0, 1, 0, 0, 0, 0, 1), (0, 1, 1, 0, 0, 0, 0, 1),
        (1, 0, 1, 0, 1, 0, 0, 1), (1, 1, 1, 0, 1, 0, 0, 1),
        (2, 0, 1, 0, 2, 0, 0, 1), (2, 1, 1, 0, 2, 0, 0, 1),
    ],
    "random": [
        (0, 0, 1, 0, 0, 0, 0, 1), (0, 1, 1, 0, 0, 0, 0, 1),
        (1, 0, 1, 0, 1, 0, 0, 1), (1, 1, 1, 0, 1, 0, 0, 1),
        (2, 0, 1, 0, 2, 0, 0, 1), (2, 1, 1, 0, 2, 0, 0, 1),
    ],
    "cornell": [
        (0, 0, 3, 0, 0, 0, 0, 3), (0, 1, 3, 0, 0, 0, 0, 3),
        (1, 0, 3, 0, 1, 0, 0, 3), (1, 1, 3, 0, 1, 0, 0, 3),
        (2, 0, 3, 0, 2, 0, 0, 3), (2, 1, 3, 0, 2, 0, 0, 3),
    ],
    "cornell-smoke": [
        (0, 0, 3, 0, 0, 0, 0, 3), (0, 1, 3, 0, 0, 0, 0, 3),
        (1, 0, 3, 0, 1, 0, 0, 3), (1, 1, 3, 0, 1, 0, 0, 3),
        (2, 0, 3, 0, 2, 0, 0, 3), (2, 1, 3, 0, 2, 0, 0, 3),
    ],
    "cornell-lucy": [
        (0, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 6, 8),
        (1, 0, 0, 0, 1, 0, 0, 0), (1, 1, 0, 0, 1, 0, 6, 8),
        (2, 0, 0, 0, 2, 0, 0, 0), (2, 1, 0, 0, 2, 0, 6, 8),
    ],
    "hdri-test": [
        (0, 0, 1, 0, 0, 0, 0, 1), (0, 1, 1, 0, 0, 0, 0, 1),
        (1, 0, 1, 0, 1, 0, 0, 1), (1, 1, 1, 0, 1, 0, 0, 1),
        (2, 0, 1, 0, 2, 0, 0, 1), (2, 1, 1, 0, 2, 0, 0, 1),
    ],
    "hdri-nee": [
        (0, 0, 1, 0, 0, 1, 0, 1), (0, 1, 1, 0, 0, 1, 0, 1),
        (1, 0, 1, 0, 1, 1, 0, 1), (1, 1, 1, 0, 1, 1, 0, 1),
        (2, 0, 1, 0, 2, 1, 0, 1), (2, 1, 1, 0, 2, 1, 0, 1),
    ],
    "cornell-rotations": [
        (0, 0, 0, 1, 0, 0, 0, 0), (0, 1, 0, 1, 0, 0, 0, 0),
        (1, 0, 0, 1, 0, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0, 0),
        (2, 0, 0, 1, 0, 0, 0, 0), (2, 1, 0, 1, 0, 0, 0, 0),
    ],
    "quads": [
        (0, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 0, 1, 0, 0, 0), (1, 1, 0, 0, 1, 0, 0, 0),
        (2, 0, 0, 0, 2, 0, 0, 0), (2, 1, 0, 0, 2, 0, 0, 0),
    ],
    "primitives": [
        (0, 0, 1, 1, 0, 0, 0, 1), (0, 1, 1, 1, 0, 0, 3, 9),
        (1, 0, 1, 1, 1, 0, 0, 1), (1, 1, 1, 1, 1, 0, 3, 9),
        (2, 0, 1, 1, 0, 0, 0, 1), (2, 1, 1, 1, 0, 0, 3, 9),
    ],
    "perlin": [
        (0, 0, 2, 0, 0, 0, 0, 2), (0, 1, 2, 0, 0, 0, 0, 2),
        (1, 0, 2, 0, 1, 0, 0, 2), (1, 1, 2, 0, 1, 0, 0, 2),
        (2, 0, 2, 0, 2, 0, 0, 2), (2, 1, 2, 0, 2, 0, 0, 2),
    ],
    "earth": [
        (0, 0, 2, 0, 0, 0, 0, 2), (0, 1, 2, 0, 0, 0, 0, 2),
        (1, 0, 2, 0, 1, 0, 0, 2), (1, 1, 2, 0, 1, 0, 0, 2),
        (2, 0, 2, 0, 2, 0, 0, 2), (2, 1, 2, 0, 2, 0, 0, 2),
    ],
    "checkered-spheres": [
        (0, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 0, 1, 0, 0, 0), (1, 1, 0, 0, 1, 0, 0, 0),
        (2, 0, 0, 0, 2, 0, 0, 0), (2, 1, 0, 0, 2, 0, 0, 0),
    ],
    "glossy-metal": [
        (0, 0, 1, 0, 0, 0, 0, 1), (0, 1, 1, 0, 0, 0, 0, 1),
        (1, 0, 1, 0, 1, 0, 0, 1), (1, 1, 1, 0, 1, 0, 0, 1),
        (2, 0, 1, 0, 2, 0, 0, 1), (2, 1, 1, 0, 2, 0, 0, 1),
    ],
    "cornell-glossy": [
        (0, 0, 1, 0, 0, 0, 0, 1), (0, 1, 1, 0, 0, 0, 0, 1),
        (1, 0, 1, 0, 1, 0, 0, 1), (1, 1, 1, 0, 1, 0, 0, 1),
        (2, 0, 1, 0, 2, 0, 0, 1), (2, 1, 1, 0, 2, 0, 0, 1),
    ],
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory, g):
    t = tmp_path_factory.mktemp("variant")
    exe = t / "variant_probe"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "variant_probe.cpp"), os.path.join(CSRC, "flatten.cpp"), "-L", LIB,
                    "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(exe)], check=True, cwd=t)
    return str(exe)


def test_dispatch_round_trip(probe):
    """{vol} x {envis} x {quant, wide, neither} x {the six shades}: the
    constants the functor receives equal the runtime fields (vol && wide
    arrives as W = false); 36 distinct (V, E, S, Q, W) tuples without vol, 24
    with it; an unknown shading kind takes the lean arm."""
    r = subprocess.run([probe, "roundtrip"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout)
    assert info["cases"] == 2 * 2 * 3 * 6 and info["bad"] == 0, info
    assert info["distinct_novol"] == 36 and info["distinct_vol"] == 24, info
    assert info["unknown_arm"] == 0, info   # SHADE_LEAN


def test_parent_table_covers_the_scenes():
    assert list(PARENT) == SCENES
    for rows in PARENT.values():
        assert [(r[0], r[1]) for r in rows] == [(nf, lift) for nf in (0, 1, 2) for lift in (0, 1)]
    assert [r[6] for r in PARENT["cornell-lucy"] if r[1] == 1] == [6, 6, 6]   # as test_lift_host


@pytest.mark.parametrize("name", SCENES)
def test_rule_matches_parent(probe, name):
    """scene_scalars + pick_variant reproduce every cell of PARENT."""
    r = subprocess.run([probe, "scene", name, "40", ASSETS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [json.loads(line) for line in r.stdout.strip().splitlines()]
    got = [(c["nf"], c["lift"], c["shade_kind"], c["vol"], c["format"], c["envis"], c["prim_recs"], c["shade"]) for c in got]
    assert got == PARENT[name]


def test_scene_scalars_refuses_lift_without_variant(probe):
    r = subprocess.run([probe, "badlift"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout)
    assert info["rc"] == info["invalid"] != 0, info
    assert info["err"] == "internal: lifted primitives in a scene without a lift shading variant", info
