"""CPU check of the batch layout (go-raytracing_amd/csrc/wave_layout.h).

tests/wave_layout_probe.cpp, built with g++ under AddressSanitizer + UBSan,
sweeps the arithmetic render_wave (api.cpp) launches by: tile counts 1, 2, 3,
5, 64 and a 40x23 image's ragged tiles; 1 to 4 twins with and without the
bounce overlap; lit and dark scenes, feature mode on and off; 1, 3 and 4096
spp; slot targets below and at the pixel count, kMinSlots, kMaxSlots and the
OOM halving sequence.  It asserts that the pixel list is a permutation of the
tiles' pixels, that every twin's slices and every array inside them are
disjoint and inside the sized buffers (binding real buffers where they are
small), that `check` refuses a short buffer and slot counts of 2^31 and
2^32 + 5, the spill capacity, and the knob precedence option > environment >
automatic.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_wave_layout_under_asan(tmp_path):
    exe = tmp_path / "wave_layout_probe"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "wave_layout_probe.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["fails"] == 0 and info["cases"] > 5000, info
