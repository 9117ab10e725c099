#!/usr/bin/env python3
"""Benchmark: Msamples/s (pixels x spp / s) of the path-tracing hot path.

Workload (`value`, N=1 and every N): CornellBoxLucy (scenes.go:714-817)
overridden to 1200x675, 500 spp, depth 5 — BASELINE.json config C4, the one
its roofline target is quoted on — with the deterministic synthetic
280K-triangle Lucy stand-in (the real mesh is a Git-LFS pointer, SURVEY.md
§0.5).  One step = one full-quality render of the frame (every pixel x every
sample), scene already resident in HBM, output a device float3 accumulation
buffer.

A plain run sets up the scene, warms up, times `--steps` steps, writes the
last step's frame if `--dump-outputs DIR` is given, and prints the result
line.  Everything below that is not the multi-GPU path itself runs only with
`--full` (and each leg can be dropped again with its `--no-*` option).

Also on the same line (`configs`): short timed runs of the other GPU configs
of BASELINE.json at their stated sizes — C2 RandomScene 1200x675x500 spp
(depth 50), C3 CornellBoxScene 600x600x1000 spp (depth 5), C5 HDRITestScene
1920x1080x2000 spp (depth 20) — through the same sharded path.

Multi-GPU (torchrun, one rank per GPU): the 32x32 buckets of the frame are
dealt round-robin to ranks; each rank renders its buckets into a zeroed
full-frame buffer, then one RCCL reduce(sum) to rank 0 combines them (each
pixel has exactly one contributor).  Total work is fixed: strong scaling.
At N=1, `shard_balance` times the 2/4/8-way round-robin shards of the frame
one after another on the one GPU and predicts the N-GPU speed-up from the
slowest shard.

`roofline`: the dominant kernel's algorithmic bytes per launch (instrumented
work counts x the per-unit sizes of DESIGN.md §4, stream bytes included) over
its HIP-event launch time measured on the render stream; `kernels` has the
same for extend / shade / shadow, plus the HBM traffic of the PMC profile
(profiles/pmc_<scene>_<W>x<H>.json, tools/profile_round.sh) as `hbm_frac`.
`cpu_baseline`: the CPU oracle's fp64 restatement of the Go path on every host
core available to the job, on a bounded sample of the same workload (rank 0,
N=1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Algorithmic bytes per unit of work.
BYTES = {
    "node_visits": 128,      # one BVH4 node (DNode4): four 24-B child boxes + four child items; set from the
                             # format the kernels run: 64 (quant8 DNodeQ), 80 (wide8: the five 16-B loads of a DNode8)
    "tri_tests": 36,         # v0, e1, e2 fp32
    "sphere_tests": 32,
    "quad_tests": 64,
    "plane_tests": 32,
    "instance_visits": 112,  # instance entry gather: wrappers 0-2 + BLAS root item and box (SURVEY: 96 B)
    "instance_box_tests": 32,  # world-space instance culling box
    "volume_tests": 64,
    "material_fetches": 32,
    "env_lookups": 48,       # 4 texels x 12 B
}
# Path-stream bytes per unit.
EXTEND_RAY_IO = 48           # ray o, d in (32) + hit record out (16); +16 (throughput word) with volumes;
                             # bounce 0 regenerates the camera ray (hit out only)
SHADE_PATH_IN = 64           # hit, o, d, throughput of a shaded path (bounce 0: the hit only, 16)
SHADE_SURVIVOR_OUT = 48      # o, d, throughput of the next stream
SHADE_END_OUT = 16           # Lout of a sample, zeroed / set at bounce 0 (emission adds later are not counted)
SHADE_JOB_OUT = 52           # NEE job: origin, area dir, info, contribution (+48 with HDRI IS: dir, contribution, throughput)
SHADOW_JOB_IO = 36           # job origin, area dir in, visibility out (+20 with HDRI IS: dir, info)
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec
# ranks deal the 32x32 buckets cut into 16x16 tiles round-robin (finer grain
# than whole buckets: the centre-heavy cost spreads more evenly)
SHARD_TILE = int(os.environ.get("RTGPU_SHARD_TILE", "16"))

# BASELINE.json configs run on the GPU (C1 SimpleScene is the CPU plumbing case).
CONFIGS = {
    "C2": ("random", dict(width=1200, aspect=16.0 / 9.0, spp=500)),   # depth 50 (scenes.go:72-73)
    "C3": ("cornell", dict(width=600, aspect=1.0, spp=1000)),         # depth 5
    "C4": ("cornell-lucy", dict(width=1200, aspect=16.0 / 9.0, spp=500)),
    "C5": ("hdri-test", dict(width=1920, aspect=16.0 / 9.0, spp=2000)),  # depth 20
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--dealing", choices=["static", "dynamic"], default="static",
                    help="N > 1: tiles dealt round-robin (static) or claimed in runs as ranks / devices finish")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", default="cornell-lucy")
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--aspect", type=float, default=16.0 / 9.0)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--depth", type=int, default=0, help="0: scene default")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--nodes", choices=["fp32", "quant8", "wide8"], default="fp32",
                    help="node format (RT_OPT_NODE_FORMAT): BVH4 fp32 / quantised, or 8-wide quantised")
    ap.add_argument("--blas", choices=["sah", "reference", "device"], default="sah",
                    help="mesh BLAS builder: host SAH (default), the caller's topology, or the GPU LBVH "
                         "(build.hip); the world BVH is SAH except for 'reference'")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-count", action="store_true", help="with --full: skip the instrumented count run")
    ap.add_argument("--no-configs", action="store_true", help="with --full: skip the C2/C3/C5 runs")
    ap.add_argument("--no-balance", action="store_true", help="with --full: skip the shard-balance timing")
    ap.add_argument("--no-three-pass", action="store_true",
                    help="with --full: skip the reference's published workload (HDRITestScene 800x450, 3 progressive passes)")
    ap.add_argument("--config-steps", type=int, default=2)
    ap.add_argument("--cpu-spp", type=int, default=48, help="spp of the CPU baseline sample")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0: every host core available to the job")
    ap.add_argument("--no-pmc", action="store_true",
                    help="with --full: skip the live rocprofv3 --pmc passes (traffic then comes from profiles/pmc_*.json)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the other legs: live PMC passes, instrumented counts and "
                         "roofline, the C2/C3/C5 configs, shard balance, the reference's three-pass workload and the "
                         "CPU baseline (each can be dropped again with its --no-* option; without --full none of them "
                         "runs and the --no-* options change nothing)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the frame of the last timed step to DIR/frame.npy (float32, H x W x 3 radiance sums); a "
                         "frame above 64 MB is written as a fixed sample of pixels instead: frame.npy is then n x 3 "
                         "and DIR/frame_pixels.npy holds the n pixel ids (y * W + x, as float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.pmc_child:   # one profiled step of the workload, nothing else
        args.steps, args.warmup = 1, 0
    if args.pmc_child or not args.full:   # a plain run: set up, warm up, time the steps, print the line
        args.no_cpu_baseline = args.no_count = args.no_configs = args.no_balance = args.no_pmc = True
        args.no_three_pass = True
    return args


# Live PMC passes (rank 0, N=1): rocprofv3 --pmc runs of this script's own
# workload (one step) as child processes, started BEFORE this process touches
# the GPU, one counter group per pass, never combined with tracing
# (MI355X_MICROARCH.md, HBM / rocprofv3).  Per-block limits: FETCH_SIZE uses 3
# TCC counters and WRITE_SIZE 2, so they get passes of their own.
PMC_PASSES = [
    ("fetch", ["FETCH_SIZE"]),
    ("write", ["WRITE_SIZE"]),
    ("lat", ["TCC_HIT_sum", "TCC_MISS_sum", "TCP_TCC_READ_REQ_sum", "TCP_TCC_READ_REQ_LATENCY_sum",
             "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VALU", "SQ_THREAD_CYCLES_VALU"]),
]
PMC_FAMILIES = ("k_extend", "k_shade", "k_shadow", "k_nee_apply", "k_accum", "k_finalize")
# Bytes per FETCH_SIZE byte, per kernel family: calibrated on gfx950 by
# tools/fetch_calib.sh (profiles/r06_fetch_calib.json).  Microkernels that miss
# a known number of 128-B lines once each show one 64-B-tallied read request
# per missed line for every access width: whole coalesced lines (128 B read:
# 64.2 / 66.2 FETCH_SIZE bytes per line, factor 1.97), one 16-B row per line,
# and k_extend's node step (7 of a line's 8 rows, both 64-B halves: still one
# request per line, so the L2 fills whole 128-B lines).  On the bench
# workload every production kernel's requests are of that class (0 % 32-B,
# <= 0.03 % 128-B requests; 64.0 FETCH_SIZE bytes per request): x 2 for all.
FETCH_FACTOR = {"extend": 2.0, "shade": 2.0, "shadow": 2.0, "nee_apply": 2.0, "accum": 2.0, "finalize": 2.0}
FETCH_CALIBRATION = "profiles/r06_fetch_calib.json (tools/fetch_calib.sh)"


def pmc_family(name: str):
    for k in PMC_FAMILIES:
        if f"rtg::{k}<" in name or f"rtg::{k}(" in name:
            return k[2:]
    return None


def run_pmc_passes(args) -> dict | None:
    """Per kernel family and launch: HBM-side bytes (FETCH_SIZE x the family's
    calibrated FETCH_FACTOR + WRITE_SIZE, KiB counters), L2 hit rate, average
    L2 read latency, wave wait share and VALU lane utilisation."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    from collections import defaultdict
    if shutil.which("rocprofv3") is None:
        return None
    child = [sys.executable, os.path.abspath(__file__), "--pmc-child", "--scene", args.scene, "--width",
             str(args.width), "--aspect", repr(args.aspect), "--spp", str(args.spp), "--depth", str(args.depth),
             "--seed", str(args.seed), "--nodes", args.nodes, "--blas", args.blas]
    tmp = tempfile.mkdtemp(prefix="rtg_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", RTGPU_STREAMS="1")   # single-stream dispatches (attribution_times)
    vals = defaultdict(lambda: defaultdict(float))
    disp = defaultdict(lambda: defaultdict(set))
    ok = []
    t0 = time.time()
    for name, counters in PMC_PASSES:
        out = os.path.join(tmp, name)
        cmd = ["timeout", "-s", "KILL", "180", "rocprofv3", "--pmc", *counters, "--output-format", "csv", "-d", out,
               "-o", "p", "--", *child]
        print(f"bench: pmc pass {name} ({' '.join(counters)})", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"bench: pmc pass {name} failed rc={r.returncode}: {r.stderr[-400:]}", file=sys.stderr)
            continue
        ok.append(name)
        for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                fam = pmc_family(row.get("Kernel_Name", ""))
                if fam is None:
                    continue
                vals[fam][row["Counter_Name"]] += float(row["Counter_Value"])
                disp[fam][row["Counter_Name"]].add(row.get("Dispatch_Id"))
    shutil.rmtree(tmp, ignore_errors=True)
    if not ok:
        return None
    kern = {}
    for fam, v in vals.items():
        def per(c):
            return v[c] / max(len(disp[fam][c]), 1)
        e = {"dispatches": max((len(s) for s in disp[fam].values()), default=0)}
        if "FETCH_SIZE" in v and "WRITE_SIZE" in v:
            ff = FETCH_FACTOR.get(fam, 2.0)
            fetch, write = per("FETCH_SIZE") * 1024 * ff, per("WRITE_SIZE") * 1024
            # per dispatch, and over the profiled step (one step: with twin
            # streams a kernel's launch is two dispatches, kernel_report)
            e.update(fetch_bytes_per_launch=int(fetch), write_bytes_per_launch=int(write),
                     hbm_bytes_per_launch=int(fetch + write),
                     hbm_bytes_step=int(v["FETCH_SIZE"] * 1024 * ff + v["WRITE_SIZE"] * 1024), fetch_factor=ff)
        h, m = v.get("TCC_HIT_sum", 0.0), v.get("TCC_MISS_sum", 0.0)
        if h + m > 0:
            e["l2_hit"] = round(h / (h + m), 4)
        if v.get("TCP_TCC_READ_REQ_sum"):
            e["l2_read_latency_cycles"] = round(v["TCP_TCC_READ_REQ_LATENCY_sum"] / v["TCP_TCC_READ_REQ_sum"], 1)
        if v.get("SQ_WAVE_CYCLES"):
            e["wave_wait_share"] = round(v.get("SQ_WAIT_ANY", 0.0) / v["SQ_WAVE_CYCLES"], 4)
        if v.get("SQ_ACTIVE_INST_VALU"):
            e["valu_lane_util"] = round(v.get("SQ_THREAD_CYCLES_VALU", 0.0) / (64 * v["SQ_ACTIVE_INST_VALU"]), 4)
        kern[fam] = e
    return {"source": "live rocprofv3 --pmc passes of this workload (one step each): " + ", ".join(ok),
            "seconds": round(time.time() - t0, 1), "kernels": kern}


def host_cores():
    """CPUs this job may use: the affinity mask (what Go's runtime.NumCPU
    reports, main.go:84), capped by a cgroup CPU quota when one is set."""
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        pass
    cores = aff if quota is None else max(1, min(aff, int(quota)))
    return cores, aff, quota


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


class Dist:
    """One process per GPU (RANK/LOCAL_RANK/WORLD_SIZE from torchrun)."""

    def __init__(self):
        import torch
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        # RTGPU_BENCH_BACKEND=gloo (ranks sharing the visible GPUs) rehearses
        # the multi-rank path on a one-GPU box
        self.backend = os.environ.get("RTGPU_BENCH_BACKEND", "nccl")
        ndev = max(torch.cuda.device_count(), 1)
        self.dev_index = local % ndev if self.world > 1 else 0
        torch.cuda.set_device(self.dev_index)
        self.dev = torch.device("cuda", self.dev_index)
        self.dist = None
        if self.world > 1:
            import torch.distributed as dist
            dist.init_process_group(self.backend)
            self.dist = dist

    def store(self):
        """The process group's key-value store (torchrun's TCPStore): its add()
        is atomic across ranks, the shared counter of dynamic dealing."""
        from torch.distributed import distributed_c10d
        return distributed_c10d._get_default_store()

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def max(self, x: float) -> float:
        if self.dist is None:
            return x
        import torch
        t = torch.tensor([x], dtype=torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather(self, vals) -> list:
        """Every rank's list of floats, on every rank (N > 1 diagnostics)."""
        if self.dist is None:
            return [list(vals)]
        import torch
        dev = self.dev if self.backend == "nccl" else "cpu"
        t = torch.tensor(list(vals), dtype=torch.float64, device=dev)
        out = [torch.zeros_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return [[float(x) for x in o.cpu().tolist()] for o in out]

    def sum_int(self, x: int) -> int:
        if self.dist is None:
            return x
        import torch
        t = torch.tensor([x], dtype=torch.int64, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return int(t.item())

    def reduce_frame(self, accum):
        if self.dist is None:
            return
        if self.backend == "nccl":
            self.dist.reduce(accum, dst=0, op=self.dist.ReduceOp.SUM)   # RCCL over xGMI
        else:
            host = accum.cpu()
            self.dist.reduce(host, dst=0, op=self.dist.ReduceOp.SUM)
            if self.rank == 0:
                accum.copy_(host)


def dynamic_runs(add, ntiles: int, world: int, first_pct: int = 50):
    """Runs [start, end) of the tile list this rank claims from a counter
    shared by all ranks (`add(k)`: atomically add k, return the new value):
    api.cpp render_dynamic's rule, bucket_renderer.go:193-213's channel across
    processes.  A run is 1/(2 world) of the tiles left (the first one
    first_pct % of a fair share), at least 1/16 of a fair share; a rank
    claims its next run once its last one is rendered."""
    fair = -(-ntiles // world)
    min_run = max(1, fair // 16)
    first = max(min_run, fair * first_pct // 100)
    runs = 0
    while True:
        left = ntiles - add(0)
        if left <= 0:
            return
        run = first if runs == 0 else max(min_run, -(-left // (2 * world)))
        end = add(run)
        start = end - run
        if start >= ntiles:
            return
        runs += 1
        yield start, min(end, ntiles)


class Workload:
    """One scene resident on this rank's GPU, this rank's bucket shard."""
    _instances = 0   # per process: makes the dynamic-dealing store keys unique per workload

    def __init__(self, g, D: Dist, scene: str, scene_kw: dict, seed: int, blas: str, nodes: str = "fp32",
                 devices=None, dealing: str = "static"):
        import torch
        self.g, self.D = g, D
        t = time.time()
        self.scene = g.Scene(scene, **scene_kw)
        cam = self.cam = self.scene.camera
        self.W, self.H = cam.image_width, cam.image_height
        self.spp, self.depth = cam.samples_per_pixel, cam.max_depth
        # devices: one process driving several GPUs through one multi-device
        # context (rt_ctx_create_multi) instead of torchrun ranks
        self.ctx = g.Context(D.dev_index, devices=devices)
        self.ctx.set_blas_builder(blas)
        self.ctx.set_tlas_builder("reference" if blas == "reference" else "sah")
        if nodes != "fp32":   # fp32 is the default format
            self.ctx.set_node_format(nodes)
        self.ctx.upload(self.scene.desc)
        self.info = self.ctx.info()
        self.dev_build_ms = self.ctx.last_build_ms()
        self.build_s = time.time() - t
        self.seed = seed
        self.buckets = g.generate_buckets(self.W, self.H, 32)
        self.params = g.make_params(self.spp, self.depth, seed=seed,
                                    buckets=g.shard_buckets(self.buckets, D.rank, D.world, SHARD_TILE))
        # dynamic dealing: a multi-device context claims runs itself
        # (RT_DEAL_DYNAMIC); ranks claim runs of the whole tile list through
        # the process group's store, one counter per frame
        self.dealing = dealing
        if devices is not None:
            self.ctx.set_dealing(dealing)
        self.all_tiles = g.split_buckets(self.buckets, SHARD_TILE)
        # static dealing: this rank's share of the tiles
        self.my_tiles = len(g.shard_buckets(self.buckets, D.rank, D.world, SHARD_TILE))
        # the store counters of dynamic dealing live as long as the process
        # group: every workload (the main one, each config scene) and every
        # frame needs keys of its own, or a later workload finds them drained
        Workload._instances += 1
        self.uid = f"{scene}_{self.W}x{self.H}_{Workload._instances}"
        self.frame_no = 0
        self.tiles_rendered = self.my_tiles
        self.reduce_ms = []
        self.accum = torch.zeros(self.H * self.W * 3, dtype=torch.float32, device=D.dev)
        self.stream = torch.cuda.current_stream(D.dev)
        self.kernel_ms, self.kernel_times = [], []

    def step(self, timed: bool = False, kernel_timing: bool = False):
        self.accum.zero_()
        if self.dealing == "dynamic" and self.D.world > 1:
            store = self.D.store()
            key = f"rtgpu_deal_{self.uid}_{self.frame_no}"
            self.frame_no += 1
            self.tiles_rendered = 0
            for a, b in dynamic_runs(lambda k: store.add(key, k), len(self.all_tiles), self.D.world):
                p = self.g.make_params(self.spp, self.depth, seed=self.seed, buckets=self.all_tiles[a:b])
                self.ctx.render_device(self.cam, p, self.accum.data_ptr(), self.stream.cuda_stream)
                self.ctx.sync()   # the next claim follows this rank's progress
                self.tiles_rendered += b - a
        else:
            self.ctx.render_device(self.cam, self.params, self.accum.data_ptr(), self.stream.cuda_stream)
        if timed:
            # blocks until the render kernel has finished; raises on a device error
            self.kernel_ms.append(self.ctx.last_render_kernel_ms())
            if kernel_timing:
                self.kernel_times.append(self.ctx.last_kernel_times())
        if timed and self.D.world > 1:
            # the combine on its own: CUDA events on the render stream (RCCL
            # runs on torch's current stream), a host clock for gloo
            import torch
            if self.D.backend == "nccl":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.stream)
                self.D.reduce_frame(self.accum)
                e1.record(self.stream)
                self.reduce_ms.append((e0, e1))
            else:
                t0 = time.perf_counter()
                self.D.reduce_frame(self.accum)
                self.reduce_ms.append((time.perf_counter() - t0) * 1e3)
        else:
            self.D.reduce_frame(self.accum)

    def reduce_ms_avg(self):
        """Mean ms of the timed steps' frame combine (events: after the sync)."""
        v = [x[0].elapsed_time(x[1]) if isinstance(x, tuple) else x for x in self.reduce_ms]
        return float(sum(v) / len(v)) if v else 0.0

    def check_dealing(self):
        """Dynamic dealing: the ranks' tiles of the last frame must partition
        the tile list (an empty or partial frame must never be reported as a
        throughput)."""
        if self.dealing == "dynamic" and self.D.world > 1:
            total = self.D.sum_int(self.tiles_rendered)
            if total != len(self.all_tiles):
                raise RuntimeError(f"dynamic dealing rendered {total} of {len(self.all_tiles)} tiles")

    def run(self, steps: int, warmup: int, kernel_timing: bool = False) -> float:
        """Barrier + synchronize on both sides of exactly `steps` timed steps;
        returns the slowest rank's elapsed seconds."""
        import torch
        self.ctx.set_kernel_timing(kernel_timing)
        for _ in range(warmup):
            self.step()
        self.ctx.sync()
        self.D.barrier()
        torch.cuda.synchronize(self.D.dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(True, kernel_timing)
        torch.cuda.synchronize(self.D.dev)
        self.D.barrier()
        el = self.D.max(time.perf_counter() - t0)
        self.check_dealing()
        return el

    def frame_sum(self):
        # identical for any rank count: each pixel has one contributor and the
        # RNG is keyed by global pixel id
        return float(self.accum.double().sum().item()) if self.D.rank == 0 else None

    def samples(self) -> int:
        return self.W * self.H * self.spp

    def close(self):
        self.ctx.close()


def attribution_times(w: Workload, steps: int = 2) -> list:
    """Per-kernel launch times for the roofline, from `steps` extra renders of
    the same workload on ONE stream (RT_OPT_STREAMS=1).  The timed steps run
    the default twin streams, whose two halves' kernels share the GPU: a
    kernel's interval there also holds the other twin's kernels, so it says
    nothing about that kernel alone.  The profiles' rocprof kernel trace
    (tools/profile_round.sh) runs the same single-stream attribution."""
    g = w.g
    w.ctx.set_option(g.RT_OPT_STREAMS, 1)
    times = []
    try:
        for _ in range(steps):
            w.accum.zero_()
            w.ctx.render_device(w.cam, w.params, w.accum.data_ptr(), w.stream.cuda_stream)
            w.ctx.last_render_kernel_ms()   # waits for the render
            times.append(w.ctx.last_kernel_times())
    finally:
        w.ctx.set_option(g.RT_OPT_STREAMS, 0)
    return times


def kernel_report(w: Workload, work_k: dict, pmc: dict | None, ktimes: list):
    """Per-kernel algorithmic bytes (work counts x per-unit bytes, stream bytes
    included) and achieved GB/s over the HIP-event launch times; HBM traffic
    and its fraction of peak from the PMC profile when it is for this code."""
    import numpy as np
    ext, sha, shd = work_k["extend"], work_k["shade"], work_k["shadow"]
    info = w.info
    envis = False
    try:
        d = w.scene.desc.contents
        envis = bool(d.environment) and bool(d.environment.contents.use_importance_sampling) and d.num_lights > 0
    except (ValueError, AttributeError):
        pass
    vol = info.volumes > 0
    samples = ext["samples"]
    trav = {k: sum(BYTES[u] * wk[u] for u in BYTES) for k, wk in (("extend", ext), ("shade", sha), ("shadow", shd))}
    alg = {
        "extend": trav["extend"] + (EXTEND_RAY_IO + (16 if vol else 0)) * ext["rays"] - 32 * samples,
        "shade": trav["shade"] + SHADE_PATH_IN * sha["rays"] - 48 * samples + SHADE_SURVIVOR_OUT * (ext["rays"] - samples)
                 + SHADE_END_OUT * samples + (SHADE_JOB_OUT + (48 if envis else 0)) * sha["shadow_rays"],
        "shadow": trav["shadow"] + (SHADOW_JOB_IO + (20 if envis else 0)) * sha["shadow_rays"],
    }
    out = {}
    for k in ("extend", "shade", "shadow"):
        launches = int(np.mean([t[f"{k}_launches"] for t in ktimes]))
        ms_tot = float(np.mean([t[f"{k}_ms"] for t in ktimes]))
        ms_avg = ms_tot / max(launches, 1)
        per_launch = alg[k] / max(launches, 1)
        # requested_GBs: the algorithm's bytes over the launch
        # time.  Most of them are served by L2 / the Infinity Cache (the scene
        # is cache-resident), so this is no HBM figure and may exceed the peak.
        e = {"launches": launches, "twins": int(ktimes[0].get("twins", 1)),
             "ms_total": round(ms_tot, 3), "ms_avg": round(ms_avg, 4),
             "alg_bytes_per_launch": int(per_launch),
             "requested_GBs": round(per_launch / (ms_avg / 1e3) / 1e9, 2) if ms_avg > 0 else None}
        kp = (pmc or {}).get("kernels", {}).get(k)
        if kp and ms_avg > 0 and "hbm_bytes_per_launch" in kp:
            # a launch covers the whole render's work (rt_last_kernel_times
            # joins the two twins' dispatches of one bounce into one launch)
            tb = kp["hbm_bytes_step"] / max(launches, 1) if "hbm_bytes_step" in kp else kp["hbm_bytes_per_launch"]
            e["traffic_bytes_per_launch"] = int(tb)
            e["hbm_GBs"] = round(tb / (ms_avg / 1e3) / 1e9, 2)
            e["hbm_frac"] = round(e["hbm_GBs"] / HBM_PEAK_GBS, 4)
            # share of the algorithmic bytes served without an HBM transfer
            # (negative: more HBM traffic than the algorithm's bytes)
            e["l2_served"] = round(1.0 - tb / per_launch, 4) if per_launch > 0 else None
        for c in ("l2_hit", "l2_read_latency_cycles", "wave_wait_share", "valu_lane_util"):
            if kp and c in kp:
                e[c] = kp[c]
        out[k] = e
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, frame, H: int, W: int) -> None:
    """What the timed path hands its caller after the last timed step: the
    float3 accumulation buffer (per-pixel radiance sums over the spp samples),
    as <out_dir>/frame.npy, float32 [H, W, 3].  A frame above the size limit
    is written as a fixed, seeded sample of its pixels, [n, 3], with their
    pixel ids beside it (frame_pixels.npy, as float64)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    px = np.ascontiguousarray(frame, dtype=np.float32).reshape(H * W, 3)
    per_pixel = 3 * 4 + 8   # the sample's float32 triple and its float64 pixel id
    if px.nbytes <= DUMP_LIMIT_BYTES:
        np.save(os.path.join(out_dir, "frame.npy"), px.reshape(H, W, 3))
        return
    ids = np.sort(np.random.default_rng(0).choice(H * W, size=DUMP_LIMIT_BYTES // per_pixel - 64, replace=False))
    np.save(os.path.join(out_dir, "frame.npy"), px[ids])
    np.save(os.path.join(out_dir, "frame_pixels.npy"), ids.astype(np.float64))


def main():
    args = parse()
    import numpy as np

    # live PMC passes first: the children must run before this process has
    # initialised the GPU (and before it holds the path-slot buffers)
    pmc_live = None
    if (not args.no_pmc and not args.no_count and int(os.environ.get("WORLD_SIZE", "1")) == 1):
        pmc_live = run_pmc_passes(args)
    D = Dist()
    import __graft_entry__ as ge
    g = ge.load_package()

    scene_kw = {}
    if args.width:
        scene_kw["width"] = args.width
    if args.aspect:
        scene_kw["aspect"] = args.aspect
    if args.spp:
        scene_kw["spp"] = args.spp
    if args.depth:
        scene_kw["max_depth"] = args.depth
    # --gpus N without torchrun: one process, one multi-device context over
    # devices 0..N-1 (RTGPU_BENCH_DEVICES=0,0 repeats a device on a one-GPU box)
    devices = None
    if D.world == 1 and args.gpus > 1:
        env_dev = os.environ.get("RTGPU_BENCH_DEVICES")
        devices = [int(x) for x in env_dev.split(",")] if env_dev else list(range(args.gpus))
    w = Workload(g, D, args.scene, scene_kw, args.seed, args.blas, args.nodes, devices, args.dealing)
    W, H, spp, depth = w.W, w.H, w.spp, w.depth
    # bytes a node step reads in the format the kernels run (a scene that
    # does not take the format asked for keeps fp32 BVH4 nodes)
    node_format = {g.RT_NODES_FP32: "fp32", g.RT_NODES_QUANT8: "quant8", g.RT_NODES_WIDE8: "wide8"}[w.info.node_format]
    BYTES["node_visits"] = {"fp32": 128, "quant8": 64, "wide8": 80}[node_format]

    # one HIP event before each extend/shade/shadow launch (and after each
    # shadow launch) on the render stream: per-kernel launch durations
    elapsed = w.run(args.steps, args.warmup, kernel_timing=True)
    value = w.samples() * args.steps / elapsed / 1e6
    ms_per_step = elapsed / args.steps * 1e3
    img_ok = bool(__import__("torch").isfinite(w.accum).all().item()) if D.rank == 0 else True
    frame_sum = w.frame_sum()
    # N > 1: what the driver's scaling line cannot show by itself — each
    # rank's render time and tile count and the combine's own time, so a
    # 1->N curve splits into imbalance, per-render fixed cost and reduce
    rank_diag = None
    if D.world > 1:
        rows = D.gather([float(np.mean(w.kernel_ms)) if w.kernel_ms else 0.0, w.reduce_ms_avg(),
                         float(w.tiles_rendered)])
        rank_diag = {"render_ms": [round(r[0], 3) for r in rows], "reduce_ms": [round(r[1], 3) for r in rows],
                     "tiles": [int(r[2]) for r in rows], "tiles_total": len(w.all_tiles),
                     "note": "per rank, mean over the timed steps: render = device time of the render's kernels "
                             "(rt_last_render_kernel_ms), reduce = the frame combine to rank 0 (events on the "
                             "render stream for RCCL), tiles = 16x16 tiles rendered in the last step"}
    # The timed region ends with the frame in HBM (the C-ABI's device-buffer
    # entry point).  rt_render into host buffers adds one D2H copy of the
    # float3 frame: timed here once, after the timed steps, and reported beside
    # `value` (never as it).
    d2h_ms = None
    if D.rank == 0:
        import torch
        torch.cuda.synchronize(D.dev)
        t_d = time.perf_counter()
        _host = w.accum.cpu()
        d2h_ms = (time.perf_counter() - t_d) * 1e3
        if args.dump_outputs:   # before any later leg renders into the buffer again
            dump_outputs(args.dump_outputs, _host.numpy(), H, W)
        del _host

    roofline = None
    kernels = None
    work = None
    if D.rank == 0 and not args.no_count:
        work_k = w.ctx.count_work_by_kernel(w.cam, w.params)
        work = {k: work_k["extend"][k] + work_k["shadow"][k] + (0 if k in ("rays", "shadow_rays") else
                                                                work_k["shade"][k]) for k in work_k["extend"]}
        pmc, pmc_name, pmc_stale = pmc_live, "live", False
        if pmc is None:   # no live passes: the committed profile, flagged when it is not this frame's
            pmc_name = f"pmc_{args.scene}_{W}x{H}.json"
            pmc_path = os.path.join(ROOT, "profiles", pmc_name)
            pmc_stale = None
            if os.path.exists(pmc_path):
                try:
                    pmc = json.load(open(pmc_path))
                    ref_sum = pmc.get("frame_sum")
                    pmc_stale = ref_sum is None or frame_sum is None or abs(ref_sum - frame_sum) > 1e-9 * abs(frame_sum)
                except (OSError, ValueError):
                    pmc = None
        ktimes = attribution_times(w)
        kernels = kernel_report(w, work_k, pmc, ktimes)
        dom = max(kernels, key=lambda k: kernels[k]["ms_total"])
        kd = kernels[dom]
        # The bound: bytes the dominant kernel moves between L2 and the fabric
        # (FETCH_SIZE x its calibrated factor + WRITE_SIZE per launch; Infinity-Cache hits are
        # counted, so the DRAM share is lower still) over its launch time,
        # against the 8 TB/s HBM peak.  The algorithm's requested bytes
        #  are reported beside it: they exceed what the
        # memory side could deliver because the scene is cache-resident.
        alg_step = sum(kernels[k]["alg_bytes_per_launch"] * kernels[k]["launches"] for k in kernels)
        req_step_GBs = alg_step / (ms_per_step / 1e3) / 1e9
        roofline = {"bound": "hbm", "achieved": kd.get("hbm_GBs"), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": kd.get("hbm_frac"), "traffic": kd.get("traffic_bytes_per_launch"),
                    "measure": f"L2->fabric bytes (FETCH_SIZE x {FETCH_FACTOR.get(dom, 2.0):g}, calibrated in "
                               f"{FETCH_CALIBRATION}, + WRITE_SIZE; includes Infinity-Cache hits) / "
                               "HIP-event launch time, both from single-stream renders of this workload "
                               "(RT_OPT_STREAMS=1: the timed twin-stream steps overlap two halves' kernels)",
                    "kernel": f"k_{dom}", "kernel_ms_avg": kd["ms_avg"], "launches_per_step": kd["launches"],
                    "twin_streams": kd.get("twins"),
                    "alg_bytes_per_launch": kd["alg_bytes_per_launch"], "requested_GBs": kd["requested_GBs"],
                    "l2_served": kd.get("l2_served"),
                    "l2_hit": kd.get("l2_hit"), "l2_read_latency_cycles": kd.get("l2_read_latency_cycles"),
                    "wave_wait_share": kd.get("wave_wait_share"), "valu_lane_util": kd.get("valu_lane_util"),
                    "requested_step_GBs": round(req_step_GBs, 1),
                    "requested_exceeds_peak": bool(req_step_GBs > HBM_PEAK_GBS),
                    "traffic_source": pmc_name if pmc else None, "traffic_stale": pmc_stale,
                    "pipeline_ms_avg": round(float(np.mean(w.kernel_ms)), 3)}
        # the measured stream-read peak on this box: 10 coalesced
        # passes over 4 GiB, 16x the Infinity Cache, through the C-ABI's kernel
        try:
            pk = w.ctx.measure_read_bandwidth(4 << 30, 10)
            roofline["peak_measured"] = round(pk, 1)
            roofline["peak_measured_how"] = "rt_measure_read_bandwidth: coalesced 16-B-per-lane reads, 4 GiB x 10 passes"
            if roofline["achieved"] is not None and pk > 0:
                roofline["frac_of_measured"] = round(roofline["achieved"] / pk, 4)
        except Exception as ex:   # an older library (RTGPU_LIB_DIR A/B builds)
            print(f"bench: no measured read peak ({ex})", file=sys.stderr)
        if roofline["frac"] is not None and roofline["frac"] > 1.0:   # a counter / timing error, not a result
            roofline["error"] = "HBM-side traffic above the peak: the counters or the launch times are wrong"
            print(f"bench: {roofline['error']}", file=sys.stderr)

    balance = None
    if D.world == 1 and devices is None and not args.no_balance:
        import torch

        w.ctx.set_kernel_timing(True)

        def timed_render(params):
            """(host ms around render + sync, device ms of the render kernels,
            summed extend/shade/shadow launch ms)"""
            w.accum.zero_()
            torch.cuda.synchronize(D.dev)
            t0 = time.perf_counter()
            w.ctx.render_device(w.cam, params, w.accum.data_ptr(), w.stream.cuda_stream)
            w.ctx.sync()
            host = (time.perf_counter() - t0) * 1e3
            kt = w.ctx.last_kernel_times()
            return host, w.ctx.last_render_kernel_ms(), kt["extend_ms"] + kt["shade_ms"] + kt["shadow_ms"]

        full = min(timed_render(w.params) for _ in range(2))
        balance = {"full_frame_ms": round(full[0], 2), "full_frame_device_ms": round(full[1], 2),
                   "full_frame_trav_shade_ms": round(full[2], 2)}
        for n in (2, 4, 8):
            runs = []
            for r in range(n):
                p = g.make_params(spp, depth, seed=args.seed, buckets=g.shard_buckets(w.buckets, r, n, SHARD_TILE))
                runs.append(min(timed_render(p) for _ in range(2)))
            shard_ms = [x[0] for x in runs]
            mx, mean = max(shard_ms), float(np.mean(shard_ms))
            balance[f"n{n}"] = {"shard_ms": [round(x, 2) for x in shard_ms], "max_over_mean": round(mx / mean, 4),
                                "predicted_speedup": round(full[0] / mx, 3),
                                "shard_device_ms": [round(x[1], 2) for x in runs],
                                "shard_trav_shade_ms": [round(x[2], 2) for x in runs]}
        balance["note"] = (f"round-robin shards of the 32x32 buckets cut into {SHARD_TILE}x{SHARD_TILE} tiles "
                           "(shard_buckets) timed one after another on this GPU, "
                           "host clock around render + sync; predicted speed-up = full frame / slowest shard, "
                           "excluding the RCCL reduce of the frame")

    configs = None
    if not args.no_configs:
        # the main workload's buffers are released first (path slots are sized
        # from the free HBM)
        main_ctx_closed = True
        w.close()
        configs = {}
        for cid, (scene, kw) in CONFIGS.items():
            if scene == args.scene and kw["width"] == W and kw["spp"] == spp:
                configs[cid] = {"workload": f"{scene} {W}x{H} {spp}spp depth {depth}", "value": round(value, 3),
                                "ms_per_step": round(ms_per_step, 3), "steps": args.steps, "frame_sum": frame_sum}
                continue
            cw = Workload(g, D, scene, kw, args.seed, args.blas, args.nodes, devices, args.dealing)
            el = cw.run(args.config_steps, 1)
            configs[cid] = {"workload": f"{scene} {cw.W}x{cw.H} {cw.spp}spp depth {cw.depth}",
                            "value": round(cw.samples() * args.config_steps / el / 1e6, 3),
                            "ms_per_step": round(el / args.config_steps * 1e3, 3), "steps": args.config_steps,
                            "frame_sum": cw.frame_sum()}
            cw.close()
    else:
        main_ctx_closed = False

    # The reference's only published number: HDRITestScene at
    # its defaults (800x450, 200 spp, depth 20), all three progressive passes
    # of BucketRenderer (bucket_renderer.go:170-191: 1 spp depth 3, 50 spp
    # depth 10, 200 spp depth 20), 30.61 s on 32 CPU workers.  Timed like the
    # reference: the clock starts at renderer construction (:68; here context
    # creation + scene flatten / upload) and covers every pass's render into
    # host buffers, tonemap and framebuffer copy (librtscene rts_renderer, the
    # schedule the Go drop-in runs).
    three = None
    if D.rank == 0 and D.world == 1 and devices is None and not args.no_three_pass:
        s3 = g.Scene("hdri-test")
        r3 = g.BucketRenderer(s3, 32, 0, D.dev_index, seed=args.seed)
        r3.render_all()
        tot_ms, tm = r3.duration_ms(), r3.timings()
        del r3
        cam3 = s3.camera
        ref_s = 30.61
        three = {"workload": f"hdri-test {cam3.image_width}x{cam3.image_height} {cam3.samples_per_pixel}spp depth "
                             f"{cam3.max_depth}, 3 progressive passes",
                 "three_pass_s": round(tot_ms / 1e3, 4), "reference_s": ref_s,
                 "speedup_vs_reference": round(ref_s / (tot_ms / 1e3), 1),
                 "create_ms": round(tm["create_ms"], 2), "pass_wall_ms": [round(x, 2) for x in tm["pass_wall_ms"]],
                 "pass_render_ms": [round(x, 2) for x in tm["pass_render_ms"]],
                 # host-buffer copies, tonemap and launch set-up beyond the device renders
                 "pass_overhead_frac": round(1.0 - sum(tm["pass_render_ms"]) / max(sum(tm["pass_wall_ms"]), 1e-9), 4)}

    cpu = None
    if D.rank == 0 and D.world == 1 and devices is None and not args.no_cpu_baseline:
        from oracle import oracle_py as O
        cores, aff, quota = host_cores()
        threads = args.cpu_threads or cores
        cpu_spp = args.cpu_spp
        # bounded sample: every pixel of the same frame at cpu_spp samples,
        # same scene/BVH/depth, fp64 (the reference's arithmetic)
        cp = g.make_params(cpu_spp, depth, seed=args.seed)
        tc = time.perf_counter()
        O.render(w.scene.desc, w.cam, cp, fp32=False, threads=threads)
        tcpu = time.perf_counter() - tc
        cpu = {"value": round(W * H * cpu_spp / tcpu / 1e6, 4), "unit": "Msamples/s", "cores": threads,
               "kind": "port", "cpu_model": cpu_model(), "affinity_cpus": aff, "cgroup_cpu_quota": quota,
               "sample": f"{args.scene} {W}x{H} x {cpu_spp} spp depth {depth} (fp64 C restatement of the Go path, "
                         f"{threads} threads = every CPU available to the job), {tcpu:.1f} s"}

    if D.rank == 0:
        line = {
            "metric": "Msamples/sec (pixels x SPP / s)",
            "value": round(value, 3),
            "unit": "Msamples/s",
            "n_gpus": D.world if devices is None else len(devices),
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic (deterministic 280K-tri Lucy stand-in; scene geometry per scenes.go)",
            "config": {"workload": f"{args.scene} {W}x{H} {spp}spp depth {depth}", "scene": args.scene,
                       "width": W, "height": H, "spp": spp, "max_depth": depth,
                       "parallelism": (f"tiles-{'rr' if args.dealing == 'static' else 'dyn'}{D.world}" if devices is None
                                       else f"ctx-multi{devices}-{args.dealing}"), "buckets": len(w.buckets), "blas": args.blas, "nodes": node_format,
                       "triangles": w.info.triangles, "bvh_nodes": w.info.nodes, "bvh_nodes8": w.info.nodes8,
                       "scene_build_s": round(w.build_s, 2), "device_bvh_build_ms": round(w.dev_build_ms, 2),
                       "image_finite": img_ok, "frame_sum": frame_sum},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "timed_region": {
                "inside": "every sample of the frame rendered (all bounces, all kernels) into a device float3 "
                          "accumulation buffer" + ("; the RCCL reduce of the frame to rank 0" if D.world > 1 else ""),
                "outside": "scene flatten / upload (resident before the clock starts); the D2H copy of the frame "
                           "that rt_render into host buffers adds (d2h_ms, measured once after the timed steps)",
                "d2h_ms": round(d2h_ms, 3) if d2h_ms is not None else None,
                "value_with_d2h": round(w.samples() / ((ms_per_step + d2h_ms) / 1e3) / 1e6, 3)
                if d2h_ms is not None else None},
        }
        if rank_diag is not None:
            line["ranks"] = rank_diag
        if args.dealing == "dynamic":
            if devices is not None:
                tiles, runs = w.ctx.last_dealing()
                line["dealing"] = {"tiles_per_device": tiles, "runs_per_device": runs}
            elif D.world > 1:
                line["dealing"] = {"rank0_tiles": w.tiles_rendered, "tiles": len(w.all_tiles)}
        if kernels is not None:
            line["kernels"] = kernels
        if work is not None:
            line["work_per_sample"] = {k: round(v / max(work["samples"], 1), 3) for k, v in work.items()
                                       if k != "samples"}
        if configs is not None:
            line["configs"] = configs
        if balance is not None:
            line["shard_balance"] = balance
        if three is not None:
            line["reference_workload"] = three
        print(json.dumps(line), flush=True)
    D.barrier()
    if D.dist is not None:
        D.dist.destroy_process_group()
    if not main_ctx_closed:
        w.close()


if __name__ == "__main__":
    main()
