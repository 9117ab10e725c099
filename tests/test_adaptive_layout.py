"""split_list (go-raytracing_amd/csrc/wave_layout.h), how render_wave cuts a
pixel list that is already on the device into the twins' parts:
tests/adaptive_layout_probe.cpp, built with g++ under AddressSanitizer +
UBSan, runs it for n in {0, 1, 2, 3, 255, 256, 257, 2^31 - 1} x 1..3 twins (and
2^32 - 1, 1000003 x 1..kMaxTwins): the parts are contiguous, sum to n, none is
empty unless n < nt, and choose_twins fed the list's length never gives more
twins than pixels."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_split_list_under_asan(tmp_path):
    exe = tmp_path / "adaptive_layout_probe"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"),
                    os.path.join(ROOT, "tests", "adaptive_layout_probe.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["fails"] == 0 and info["cases"] >= 24, info
