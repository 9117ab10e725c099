"""CPU checks of the host flattener and of the device path-tracing source.

* tests/flatten_probe.cpp: every index the kernels dereference (node items,
  leaf ranges, refs, instance -> BLAS, volume boundaries, textures) is in
  range for each scene, and the per-ref arrays (rank, culling box, top
  object) are parallel to `refs`.
* tests/wave_emu.cpp: the production wavefront kernels (wavefront.hip:
  camera, extend, shade, shadow, NEE apply, accumulate) compiled for the
  host, one lane per workgroup, driven batch by batch like run_batches()
  over exactly-sized buffers under AddressSanitizer + UBSan (every stream,
  job and queue index checked), with a 4-entry stack ring (spill path) and a
  non-identity pixel list; compared with the oracle's fp32 mode.  The arrays
  per slot and the spill areas are sized as production sizes them
  (wave_layout.h: no NEE job arrays without lights, spill_cap_for).

The other kernel files have host emulations of their own, built the same way:
tests/denoise_emu.cpp (test_denoise_host.py), tests/denoise_var_emu.cpp
(test_denoise_var_host.py) and tests/build_emu.cpp, the device BVH build's
kernels of build.hip (test_device_build_host.py).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "go-raytracing_amd", "lib")
CSRC = os.path.join(ROOT, "go-raytracing_amd", "csrc")
ASSETS = os.path.join(ROOT, "assets")
SCENES = ["simple", "random", "cornell", "cornell-smoke", "cornell-lucy", "hdri-test", "hdri-nee", "cornell-rotations", "quads",
          "primitives", "perlin", "earth", "checkered-spheres", "glossy-metal", "cornell-glossy"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(tmp, src, out, sanitize=False):
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include")]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                "-I", os.path.join(ROOT, "tests", "host_emu")]
    cmd += [os.path.join(ROOT, "tests", src), os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene",
            f"-Wl,-rpath,{LIB}", "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=tmp)
    return str(out)


@pytest.fixture(scope="module")
def probe(tmp_path_factory, g):
    t = tmp_path_factory.mktemp("probe")
    return _build(t, "flatten_probe.cpp", t / "probe")


@pytest.fixture(scope="module")
def wave(tmp_path_factory, g):
    t = tmp_path_factory.mktemp("wave")
    return _build(t, "wave_emu.cpp", t / "wave", sanitize=True)


def _env():
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:verify_asan_link_order=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    return env


@pytest.mark.parametrize("collapse", ["sah", "greedy"])
@pytest.mark.parametrize("name", SCENES)
def test_flattened_indices_in_range(probe, name, collapse):
    """Every index the kernels dereference is in range and the stack bound
    holds, under both BVH2 -> BVH4 collapses (RTGPU_BVH4_COLLAPSE)."""
    env = dict(os.environ, RTGPU_BVH4_COLLAPSE=collapse)
    r = subprocess.run([probe, name, "64", ASSETS], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout)
    assert info["fails"] == 0, info
    assert 0 < info["stack_needed"] <= 64
    if name in ("cornell-lucy",):
        assert info["culling_boxes"] == info["instances"] == 10   # RotateY/Translate/Scale only


@pytest.mark.parametrize("name,batch", [("simple", 0), ("cornell", 1), ("cornell-smoke", 0), ("cornell-lucy", 1),
                                        ("hdri-nee", 0), ("hdri-test", 1), ("random", 0), ("primitives", 1),
                                        ("perlin", 0), ("earth", 0), ("glossy-metal", 0), ("cornell-glossy", 1),
                                        ("quads", 0), ("checkered-spheres", 0), ("cornell-rotations", 1),
                                        ("cornell+lift", 0), ("cornell-lucy+lift", 1)])
def test_wavefront_kernels_under_asan_match_oracle(wave, O, g, tmp_path, name, batch):
    """NAME+lift: flattened with the world quads / spheres lifted out of the
    world BVH (RTG_EMU_LIFT=1, what contexts do by default; cornell-lucy
    lifts its six walls, cornell shades in the volume variant and lifts
    nothing): with fp32 nodes every ray is decided as in the unlifted scene,
    so the same oracle bar holds."""
    spp, seed, width = 2, 77, 40
    env = _env()
    lifted = 0
    if name.endswith("+lift"):
        name = name[:-len("+lift")]
        env["RTG_EMU_LIFT"] = "1"
        lifted = 6 if name == "cornell-lucy" else 0
    out = tmp_path / f"{name}.f32"
    args = [wave, name, str(width), str(spp), str(seed), ASSETS, str(out)]
    if batch:
        args.append(str(batch))   # one sample per batch: several batches
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["lifted"] == lifted
    if name in ("hdri-test", "hdri-nee"):   # the HDR asset's texels in their 4-B RGBE form (DEnv::rgbe)
        assert json.loads(r.stdout.strip().splitlines()[-1])["rgbe"] == 1
    kw = dict(width=width)
    if name == "cornell-lucy":
        kw.update(lucy_rings=60, lucy_cols=80)
    s = g.Scene(name, **kw)
    cam = s.camera
    ref = O.render(s.desc, cam, g.make_params(spp, cam.max_depth, seed=seed), fp32=True)
    got = np.fromfile(out, np.float32).reshape(ref.shape)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), float(np.abs(got - ref).max())


def test_node_quantiser_is_conservative(tmp_path):
    """RT_NODES_QUANT8 (node_quant.h): on random BVH4 nodes spanning ten
    decades, every child's dequantised box holds its fp32 box with the stated
    margin, unused children are rejected, and the traversal's fp32 quantised
    slab test accepts rays aimed at faces, edges and corners from up to 20
    node magnitudes away (tests/quant_probe.cpp)."""
    exe = tmp_path / "qp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host_emu"),
                    os.path.join(ROOT, "tests", "quant_probe.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout)
    assert info["rays"] == 160000 and info["contain_fail"] == info["unused_fail"] == info["slab_fail"] == 0, info
    # outside the envelope rtgpu.h documents (rays 10^2..10^5 node magnitudes
    # away): how often the quantised test loses a box the fp32 test keeps
    assert info["far_rays"] > 0
    print(f"quant8 vs fp32 boxes, rays 10^2..10^5 node magnitudes away: {info['far_fail']} of "
          f"{info['far_rays']} accepted boxes lost or narrowed")


@pytest.mark.parametrize("name,batch", [("cornell-lucy", 1), ("random", 0), ("cornell-smoke", 0), ("hdri-nee", 0),
                                        ("primitives", 1), ("cornell-rotations", 0)])
def test_wavefront_kernels_quant8_nodes_match_oracle(wave, O, g, tmp_path, name, batch):
    """The same host emulation with the quantised node format
    (RT_NODES_QUANT8; cornell-rotations keeps fp32 nodes): same oracle bar."""
    spp, seed, width = 2, 77, 40
    out = tmp_path / f"{name}.f32"
    args = [wave, name, str(width), str(spp), str(seed), ASSETS, str(out)]
    if batch:
        args.append(str(batch))
    env = _env()
    env["RTG_EMU_QUANT"] = "1"
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    kw = dict(width=width)
    if name == "cornell-lucy":
        kw.update(lucy_rings=60, lucy_cols=80)
    s = g.Scene(name, **kw)
    cam = s.camera
    ref = O.render(s.desc, cam, g.make_params(spp, cam.max_depth, seed=seed), fp32=True)
    got = np.fromfile(out, np.float32).reshape(ref.shape)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), float(np.abs(got - ref).max())


@pytest.mark.parametrize("name,batch,wide", [("cornell-lucy", 1, 1), ("random", 0, 1), ("cornell-smoke", 0, 1),
                                             ("hdri-nee", 0, 1), ("hdri-test", 0, 1), ("simple", 1, 1),
                                             ("cornell", 0, 1), ("quads", 0, 1), ("checkered-spheres", 0, 1),
                                             ("primitives", 1, 0), ("cornell-rotations", 0, 0)])
def test_wavefront_kernels_wide8_nodes_match_oracle(wave, O, g, tmp_path, name, batch, wide):
    """The host emulation with the 8-wide node format (RT_NODES_WIDE8,
    DNode8: octant-ordered children, computed child items, triangle leaves
    as DWTri records, litems for the others); scenes that need the
    rare-primitive traversal (circles: primitives; RotateX/Z) keep BVH4
    nodes (`wide` = which one the emulation ran).  Same oracle bar."""
    spp, seed, width = 2, 77, 40
    out = tmp_path / f"{name}.f32"
    args = [wave, name, str(width), str(spp), str(seed), ASSETS, str(out)]
    if batch:
        args.append(str(batch))
    env = _env()
    env["RTG_EMU_QUANT"] = "2"
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["wide"] == wide and (info["nodes8"] > 0) == bool(wide), info
    kw = dict(width=width)
    if name == "cornell-lucy":
        kw.update(lucy_rings=60, lucy_cols=80)
    s = g.Scene(name, **kw)
    cam = s.camera
    ref = O.render(s.desc, cam, g.make_params(spp, cam.max_depth, seed=seed), fp32=True)
    got = np.fromfile(out, np.float32).reshape(ref.shape)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), float(np.abs(got - ref).max())


@pytest.mark.parametrize("name,tail_after,nodes", [("random", 0, "0"), ("random", 7, "0"), ("hdri-test", 2, "0"),
                                                   ("random", 3, "2"), ("simple", 1, "0")])
def test_tail_kernel_bit_identical(wave, tmp_path, name, tail_after, nodes):
    """The long-tail kernel (k_tail: one lane carries a path through all its
    remaining bounces, trav_step then shade_path) under ASan/UBSan: handed
    the paths left after bounce `tail_after`, the frame equals the one the
    per-bounce kernels render, bit for bit (RT_OPT_TAIL's claim)."""
    spp, seed, width = 2, 5, 48
    outs = {}
    for mode in ("wave", "tail"):
        out = tmp_path / f"{name}_{mode}.f32"
        env = _env()
        env["RTG_EMU_QUANT"] = nodes
        if mode == "tail":
            env["RTG_EMU_TAIL"] = str(tail_after)
        r = subprocess.run([wave, name, str(width), str(spp), str(seed), ASSETS, str(out)], capture_output=True,
                           text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        outs[mode] = np.fromfile(out, np.float32)
    assert outs["wave"].sum() > 0
    assert np.array_equal(outs["wave"], outs["tail"])


@pytest.mark.parametrize("name,batch,nodes", [("cornell-lucy", 1, "0"), ("cornell", 0, "0"), ("hdri-nee", 0, "0"),
                                              ("cornell-smoke", 1, "1"), ("cornell-lucy", 0, "2"),
                                              ("cornell-rotations", 0, "0")])
def test_bounce_overlap_bit_identical(wave, tmp_path, name, batch, nodes):
    """The bounce overlap (RT_OPT_OVERLAP: bounce b's k_shadow / k_nee_apply
    beside bounce b + 1's k_extend) under ASan/UBSan, in the order that
    separates them most (k_extend b + 1 runs to its end first): the NEE
    counters of the two bounces are disjoint parity sets and k_shade resets
    the claim counters, so the frame equals the serial schedule's bit for
    bit, over several batches and every node format."""
    spp, seed, width = 2, 11, 40
    outs = {}
    for mode in ("serial", "overlap"):
        out = tmp_path / f"{name}_{mode}.f32"
        env = _env()
        env["RTG_EMU_QUANT"] = nodes
        env["RTG_EMU_OVERLAP"] = "1" if mode == "overlap" else "0"
        args = [wave, name, str(width), str(spp), str(seed), ASSETS, str(out)]
        if batch:
            args.append(str(batch))
        r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        outs[mode] = np.fromfile(out, np.float32)
    assert outs["serial"].sum() > 0
    assert np.array_equal(outs["serial"], outs["overlap"])


def test_grazing_sliver_ray_documented(tmp_path, g, O):
    """DESIGN.md §5 "Topology and grazing hits": the one C4 camera ray in
    95.9 M path rays (tools/oracle_ray_scan.py) on which the GPU's hit
    differs from the fp32 oracle's, replayed through the production
    k_extend on the host (tests/ray_emu.cpp, the full 280K-triangle mesh).
    The ray grazes a sliver triangle whose Moller-Trumbore test accepts a hit
    outside the triangle's own box; the SAH BLAS's leaf box is missed, so the
    kernel reaches the floor behind it, while the oracle, walking the
    caller's topology, reaches the sliver.  Pinned so that the documented
    class and its cause stay reproducible."""
    exe = tmp_path / "ray_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "ray_emu.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(exe)],
                   check=True)
    ray = "278.0 278.0 -800.0 -1.1796875 -0.32147216796875 10.0\n"
    env = dict(os.environ, RTG_EMU_FULL_LUCY="1")
    r = subprocess.run([str(exe), "cornell-lucy", "1200", ASSETS], input=ray, capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    kind, idx, t = r.stdout.split()[:3]
    assert int(kind) == 2 and float(t) == 135.5   # the floor quad
    s = g.Scene("cornell-lucy", width=1200, aspect=16.0 / 9.0)
    cam = s.camera
    top, prim, tt, rays, _ = O.path_records(s.desc, cam, 1, 27, 1, fp32=True, threads=8)
    p = 441109
    assert np.array_equal(rays[0][p].astype(np.float32), np.array([278.0, 278.0, -800.0, -1.1796875, -0.32147216796875,
                                                                   10.0], np.float32))
    assert prim[0][p] == 512357 and abs(tt[0][p] - 119.65116) < 1e-4   # the sliver triangle, closer
