"""bench.py's command line: what a plain run does, what --full adds, and the
frame that --dump-outputs writes.

A plain run (`--gpus 1 --steps N --warmup W`) only sets up, warms up, times
the N steps and prints the line; every other leg (live PMC passes, counts and
roofline, the C2/C3/C5 configs, shard balance, the three-pass workload, the
CPU baseline) needs --full, where its --no-* option still drops it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("no_pmc", "no_count", "no_configs", "no_balance", "no_three_pass", "no_cpu_baseline")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_every_extra_leg_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, leg) for leg in LEGS)


def test_full_turns_the_legs_on_and_no_options_still_drop_them(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not any(getattr(a, leg) for leg in LEGS)
    a = _parse(monkeypatch, "--full", "--no-configs", "--no-pmc")
    assert a.no_configs and a.no_pmc
    assert not (a.no_count or a.no_balance or a.no_three_pass or a.no_cpu_baseline)


def test_steps_below_one_is_an_error(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_writes_the_whole_frame(tmp_path):
    H, W = 5, 7
    frame = np.arange(H * W * 3, dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "d"), frame, H, W)
    assert os.listdir(tmp_path / "d") == ["frame.npy"]
    out = np.load(tmp_path / "d" / "frame.npy")
    assert out.dtype == np.float32 and out.shape == (H, W, 3)
    assert np.array_equal(out.ravel(), frame)


def test_dump_of_a_frame_above_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    H, W = 50, 40
    frame = np.random.default_rng(3).random(H * W * 3).astype(np.float32)
    sizes = []
    for name in ("a", "b"):
        d = tmp_path / name
        bench.dump_outputs(str(d), frame, H, W)
        sizes.append(sum(os.path.getsize(d / f) for f in os.listdir(d)))
    assert max(sizes) <= 4000
    px, ids = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "frame_pixels.npy")
    assert px.dtype == np.float32 and ids.dtype == np.float64 and px.shape == (len(ids), 3)
    assert len(ids) > 100 and len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < H * W
    assert np.array_equal(px, frame.reshape(H * W, 3)[ids.astype(np.int64)])
    # the same pixels from run to run
    assert np.array_equal(ids, np.load(tmp_path / "b" / "frame_pixels.npy"))


def _run_and_load(out, *extra):
    """One small bench run that dumps its outputs: (result line, dumped frame)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "320",
                        "--spp", "8", "--dump-outputs", str(out), *extra], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    H, W = line["config"]["height"], line["config"]["width"]
    assert W == 320 and line["value"] == pytest.approx(W * H * 8 / line["ms_per_step"] / 1e3, rel=1e-3)
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3)
    assert np.isfinite(frame).all()
    # the dumped frame is the device buffer the line's checksum was taken from
    assert float(frame.astype(np.float64).sum()) == pytest.approx(line["config"]["frame_sum"], rel=1e-12)
    return line, frame


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_it_timed(tmp_path):
    line, _ = _run_and_load(tmp_path / "dump")
    for key in ("kernels", "work_per_sample", "configs", "shard_balance", "reference_workload"):
        assert key not in line
    assert line["roofline"] is None and line["cpu_baseline"] is None


@pytest.mark.gpu
def test_full_run_dumps_the_timed_frame_not_a_later_legs(tmp_path):
    """The attribution and shard-balance legs render into the same device
    buffer again (the last one an eighth of the frame): the dump must hold
    the last timed step's whole frame, the one `frame_sum` was taken from.
    The three-pass leg (a renderer of its own) runs here too."""
    line, _ = _run_and_load(tmp_path / "dump", "--full", "--no-pmc", "--no-configs", "--no-cpu-baseline")
    assert line["roofline"] is not None and "kernels" in line and "n8" in line["shard_balance"]
    assert "configs" not in line and line["cpu_baseline"] is None
    # the reference's three-pass workload ran too
    assert line["reference_workload"]["three_pass_s"] > 0 and len(line["reference_workload"]["pass_wall_ms"]) == 3
