"""The traversal stack bound on the CPU: the rows of tests/stack_cases.py
(deep hand-built chains in every mode; expected values from tests/path_ref.py,
brute force in float64, no tree) through the flattener and the production
kernels compiled for the host (tests/hits_emu.cpp, tests/wave_run.h).

  * On path_ref alone: every row's counts (rays that cross the whole deep
    structure, shadow rays among them that the deepest link occludes and that
    pass) and at most 2 % of the pixel-samples left out.
  * The oracle in both modes, so the bars below have their origin on record.
  * TStack alone: what is pushed comes back, the error flag is raised by
    exactly the push that exceeds ring + spill_cap, nothing is written past it.
  * The flattener's figures: stack_needed and its terms equal the table
    (FIGURES, worked out from the construction), the sum is the documented
    one, and tlas_need* / blas_need* equal a walk of the flattened DNode4 /
    DNode8 arrays in numpy.
  * The peak: every ray's deepest stack in words, read off a spill area filled
    with a word the traversal never pushes (hits_emu_stack_trace), for closest
    hits (k_extend, the reference-order variant included) and shadow rays
    (k_shadow): peak <= the bound, peak >= the lower bound the construction
    gives (stack_cases: the row's comment), the error flag clear, ids, t and
    visibility the reference's; then again with the product's spill capacity,
    spill_cap_for(bound, ring): the same bits.
  * The whole host pipeline with that capacity (wave_run.h), and once with the
    long-tail kernel taking every path after bounce 0.
  * The accepted / refused edges as exact depths.

Tolerances: tests/test_path_kat.py's (ids, NEE bits, visibility and the node
format exact; bounce-0 t rtol 2e-6; later bounces and the radiance 1.05 x
(oracle) and 4 x (host kernels) the fp32 oracle's measured error, group
`stack` of MEASURED_FP32)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import path_cases as PC
from tests import path_ref as P
from tests import stack_cases as SC
from tests import xform_cases as XC
from tests.test_path_kat import CSRC, LIB, ROOT, _vp, check_radiance, check_records, f32p, i32p, u32p
from tests.test_xform_kat import check_prims, grp

FORMATS = {"fp32": 0, "quant8": 1, "wide8": 2}
REFERENCE, SAH = 0, 1                      # flatten.h BLAS_REFERENCE, BLAS_SAH (both builders' options)
RT_ERR_UNSUPPORTED = -2
K_STACK_MAX, K_LDS_STACK = 128, 8          # wavefront.h
ITEM_SHIFT, ITEM_NODE = 28, 0              # dev_layout.h
ROW_IDS = [f"{n}-{v}" if v else n for n, v in SC.ROWS]

# What the flattener must report, from the construction.  A chain's world tree
# has, hanging off the chain path, its n shells, the wall, the floor and the
# lamp (the quads' node is opened by the collapse): tlas_need4 = n + 3 - 1, and
# stack_needed = tlas_need4 + max_leaf_inst + 1 + blas_need4 + 2 = n + 5 without
# instances.  n12dark has no lamp: 12 + 2 - 1 + 3.  chain_dfs: the RotateX quad
# hangs too and its world leaf counts one instance: 2 (n + 3 + 1 + 1 + 2) less
# the quads' node, which reference order keeps: 2 (n + 5).  inst_leaf: W + 3
# world items and the leaf, K instances, M - 1 mesh siblings: (W + 3) + K + 1 +
# (M - 1) + 2.  A chain of pairs: the 4-wide collapse keeps some pairs as nodes,
# the 8-wide opens them all: 2 n + 3 - 1 + 3 = 2 n + 4 in the 8-wide format.
FIGURES = {
    ("chain_ref", "n4"): dict(bound=9), ("chain_ref", "n8"): dict(bound=13), ("chain_ref", "n59"): dict(bound=64), ("chain_ref", "n123"): dict(bound=128),
    ("chain_ref", "p61"): dict(bound=98, bound8=126), ("chain_ref", "p62"): dict(bound=99, bound8=None),
    ("chain_ref", "n12dark"): dict(bound=16), ("chain_dfs", "n59"): dict(bound=128),
    ("inst_leaf", ""): dict(bound=SC.W_INST + 3 + SC.K_INST + 1 + SC.M_TRIS - 1 + 2),
    ("balanced", ""): dict(bound=16, bound8=25),      # the SAH builders' trees: recorded, not derived
}


def builders(name):
    return (SAH, SAH) if name == "balanced" else (REFERENCE, REFERENCE)


def taken(name, variant, fmt):
    """The node format the row takes: reference order keeps fp32 nodes; the
    8-wide format only up to its own bound (flatten.h kStackMax8)."""
    if name == "chain_dfs":
        return 0
    if fmt == "wide8" and FIGURES[(name, variant)].get("bound8", 0) is None:
        return 0
    return FORMATS[fmt]


@pytest.fixture(scope="module")
def emu(tmp_path_factory, g):
    """tests/hits_emu.cpp as a plain shared library (no sanitizer)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    t = tmp_path_factory.mktemp("stack_emu")
    so = t / "libhits_emu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "host_emu"), os.path.join(ROOT, "tests", "hits_emu.cpp"),
                    os.path.join(CSRC, "flatten.cpp"), "-L", LIB, "-lrtscene", f"-Wl,-rpath,{LIB}", "-o", str(so)],
                   check=True, cwd=t)
    lib = C.CDLL(str(so))
    lib.hits_emu_stack_info.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, u32p, C.c_int, u32p, C.c_int, u32p, C.c_int]
    lib.hits_emu_stack_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p,
                                         f32p, C.c_int, i32p, i32p, f32p, i32p, i32p, i32p]
    lib.hits_emu_stack_unit.argtypes = [C.c_int, C.c_int, C.c_int, u32p, i32p, i32p, i32p]
    lib.hits_emu_render_blas.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, f32p, i32p]
    return lib


# ---- on path_ref alone ------------------------------------------------------
def test_rows_are_what_they_claim(g):
    for n, v in SC.ALL_ROWS:
        c = SC.CASES[n]
        e = c.expected(g, v)
        print(c.summary(g, v))
        assert e["left_out"] <= PC.LEFT_OUT_CAP * PC.N * e["samples"], (n, v)
        assert len(e["scene"].objects) <= 135
    for order in ("nested", "perm"):         # the shells: distinct, 8e-5 or more apart, the largest where the row says
        r = SC.radii(123, order)
        assert len(set(r)) == 123 and np.diff(sorted(r)).min() > 8e-5
    assert np.argmax(SC.radii(59, "perm")) == 59 // 2 and np.argmax(SC.radii(59, "nested")) == 58


# ---- the oracle, both modes -------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,variant", SC.ALL_ROWS, ids=[f"{n}-{v}" if v else n for n, v in SC.ALL_ROWS])
def test_oracle_stack_rows(g, O, name, variant, fp32):
    c = SC.CASES[name]
    e = c.expected(g, variant)
    who = "fp32" if fp32 else "fp64"
    b, d, cam, ids = c.build(g, variant)
    what = f"{name}[{variant}] {who} oracle"
    top, prim, t, ray, nee = O.path_records(d, cam, PC.SEED, 0, e["depth"], fp32=fp32, threads=2)
    for k in range(e["depth"]):
        check_records(what, grp(c, variant), e, ids, 0, k, top[k], t[k], ray[k], nee[k], who, bits="nee_dev")
        check_prims(what, c, e, 0, k, prim[k])
    L = O.render(d, cam, g.make_params(e["samples"], e["depth"], seed=PC.SEED), fp32=fp32, threads=2)
    check_radiance(what, grp(c, variant), e, L, who)


# ---- TStack alone -------------------------------------------------------------
@pytest.mark.parametrize("ring,cap", [(4, 1), (4, 5), (4, 124), (8, 1), (8, 56), (8, 120)])
def test_tstack_push_pop_and_overflow(emu, ring, cap):
    def run(n):
        popped = np.zeros(max(n, 1), np.uint32)
        err, first, past = C.c_int32(-1), C.c_int32(-2), C.c_int32(-1)
        assert emu.hits_emu_stack_unit(ring, cap, n, popped.ctypes.data_as(u32p), C.byref(err), C.byref(first), C.byref(past)) == 0
        return popped[:n], err.value, first.value, past.value
    for n in (1, ring, ring + 1, ring + cap - 1, ring + cap):
        popped, err, first, past = run(n)
        assert np.array_equal(popped, 0x1000 + np.arange(n, dtype=np.uint32)[::-1]), f"ring {ring} cap {cap} n {n}: {popped[:12]}"
        assert (err, first, past) == (0, -1, 0), (ring, cap, n, err, first, past)
    popped, err, first, past = run(ring + cap + 1)
    assert (err, first, past) == (1, ring + cap + 1, 0), (ring, cap, err, first, past)


# ---- the flattener's figures ----------------------------------------------------
def stack_info(emu, d, name, fmt, arrays=False):
    tl, bl = builders(name)
    out = np.zeros(14, np.int32)
    assert emu.hits_emu_stack_info(_vp(d), tl, bl, FORMATS[fmt], out.ctypes.data_as(i32p), None, 0, None, 0, None, 0) == 0
    keys = ("status", "stack_needed", "tlas_need4", "blas_need4", "max_leaf_inst", "dfs_order", "format", "stack_needed8",
            "tlas_need8", "blas_need8", "nodes4", "nodes8", "blas", "bound")
    info = dict(zip(keys, (int(x) for x in out)))
    if arrays and info["status"] == 0:
        n4 = np.zeros((max(info["nodes4"], 1), 5), np.uint32)
        n8 = np.zeros((max(info["nodes8"], 1), 32), np.uint32)
        roots = np.zeros(2 + 2 * info["blas"], np.uint32)
        emu.hits_emu_stack_info(_vp(d), tl, bl, FORMATS[fmt], out.ctypes.data_as(i32p), n4.ctypes.data_as(u32p), len(n4),
                                n8.ctypes.data_as(u32p), len(n8), roots.ctypes.data_as(u32p), len(roots))
        info.update(n4=n4, n8=n8, roots=roots)
    return info


def pending4(n4, item, memo):
    """The most entries a traversal below BVH4 item `item` holds: a node with k
    used slots leaves k - 1 pending while it is in the worst of them."""
    if item >> ITEM_SHIFT != ITEM_NODE:
        return 0
    i = item & ((1 << ITEM_SHIFT) - 1)
    if i not in memo:
        used = [c for c in range(4) if (int(n4[i, 4]) >> c) & 1]
        memo[i] = len(used) - 1 + max(pending4(n4, int(n4[i, c]), memo) for c in used)
    return memo[i]


def pending8(n8, item, memo):
    """The same over DNode8 records (dev_layout.h): word 3 child_base, word 6
    bits 8..15 the internal slots, bits 0..7 the leaf slots; internal child k
    of a node is child_base + its rank among the internal slots."""
    if item >> ITEM_SHIFT != ITEM_NODE:
        return 0
    i = item & ((1 << ITEM_SHIFT) - 1)
    if i not in memo:
        imask, lmask, base = (int(n8[i, 6]) >> 8) & 0xFF, int(n8[i, 6]) & 0xFF, int(n8[i, 3])
        kids = bin(imask).count("1")
        memo[i] = bin(imask | lmask).count("1") - 1 + max([pending8(n8, base + k, memo) for k in range(kids)] + [0])
    return memo[i]


@pytest.mark.parametrize("name,variant", SC.ROWS, ids=ROW_IDS)
def test_flattener_figures(g, emu, name, variant):
    c = SC.CASES[name]
    b, d, cam, ids = c.build(g, variant)
    fig = FIGURES[(name, variant)]
    for fmt in FORMATS:
        i = stack_info(emu, d, name, fmt, arrays=True)
        assert i["status"] == 0 and i["format"] == taken(name, variant, fmt), (fmt, i["status"], i["format"])
        # the documented sum, term by term
        mult = 2 if i["dfs_order"] else 1
        assert i["stack_needed"] == mult * (i["tlas_need4"] + i["max_leaf_inst"] + 1 + i["blas_need4"] + 2), i
        assert i["dfs_order"] == (name == "chain_dfs")
        assert i["max_leaf_inst"] == (SC.K_INST if name == "inst_leaf" else 1 if name in ("chain_dfs", "balanced") else 0), i
        if fig["bound"] is not None:
            assert i["stack_needed"] == fig["bound"], f"{name}[{variant}] {fmt}: stack_needed {i['stack_needed']}, the table {fig['bound']}"
        # the walk of the flattened arrays
        memo = {}
        assert pending4(i["n4"], int(i["roots"][0]), memo) == i["tlas_need4"], f"{name}[{variant}] {fmt}: tlas_need4 {i['tlas_need4']}"
        blas = max([pending4(i["n4"], int(i["roots"][2 + 2 * k]), memo) for k in range(i["blas"])] + [0])
        assert blas == i["blas_need4"], f"{name}[{variant}] {fmt}: blas_need4 {i['blas_need4']}, the walk {blas}"
        if i["format"] == 2:
            memo = {}
            assert pending8(i["n8"], int(i["roots"][1]), memo) == i["tlas_need8"], f"{name}[{variant}]: tlas_need8 {i['tlas_need8']}"
            blas8 = max([pending8(i["n8"], int(i["roots"][3 + 2 * k]), memo) for k in range(i["blas"])] + [0])
            assert blas8 == i["blas_need8"], f"{name}[{variant}]: blas_need8 {i['blas_need8']}, the walk {blas8}"
            assert i["stack_needed8"] == i["tlas_need8"] + i["max_leaf_inst"] + 1 + i["blas_need8"] + 2 <= K_STACK_MAX, i
            assert i["bound"] == max(i["stack_needed"], i["stack_needed8"])
            if fig.get("bound8"):
                assert i["stack_needed8"] == fig["bound8"], f"{name}[{variant}]: stack_needed8 {i['stack_needed8']}"
        else:
            assert i["bound"] == i["stack_needed"]
        print(f"{name}[{variant}] {fmt}: format {i['format']} stack_needed {i['stack_needed']} (tlas {i['tlas_need4']} inst "
              f"{i['max_leaf_inst']} blas {i['blas_need4']}) 8-wide {i['stack_needed8']}")


def test_edges(g, emu):
    """The exact accepted / refused depths: a chain of 123 (stack_needed 128) is
    taken and one of 124 refused, in reference order 59 and 60, and a valid
    scene flattens after a refusal; the chain of 61 pairs takes the 8-wide
    format (its bound there 126) and that of 62 (129) reports fp32 nodes."""
    c = SC.CASES["chain_ref"]
    E = SC.EDGES
    for fmt in FORMATS:
        assert stack_info(emu, c.build(g, f"n{E['chain_ref']['refused']}")[1], "chain_ref", fmt)["status"] == RT_ERR_UNSUPPORTED
        i = stack_info(emu, c.build(g, f"n{E['chain_ref']['accepted']}")[1], "chain_ref", fmt)
        assert (i["status"], i["stack_needed"], i["format"]) == (0, K_STACK_MAX, FORMATS[fmt]), (fmt, i)
    c = SC.CASES["chain_dfs"]
    assert stack_info(emu, c.build(g, f"n{E['chain_dfs']['refused']}")[1], "chain_dfs", "fp32")["status"] == RT_ERR_UNSUPPORTED
    i = stack_info(emu, c.build(g, f"n{E['chain_dfs']['accepted']}")[1], "chain_dfs", "fp32")
    assert (i["status"], i["stack_needed"], i["dfs_order"]) == (0, K_STACK_MAX, 1), i
    c = SC.CASES["chain_ref"]
    a = stack_info(emu, c.build(g, f"p{E['wide8']['taken']}")[1], "chain_ref", "wide8")
    f = stack_info(emu, c.build(g, f"p{E['wide8']['fallback']}")[1], "chain_ref", "wide8")
    assert (a["status"], a["format"], a["stack_needed8"]) == (0, 2, 126), a
    assert (f["status"], f["format"], f["bound"]) == (0, 0, f["stack_needed"]), f


# ---- the peak ---------------------------------------------------------------------
def stack_trace(emu, d, cam, name, fmt, tight, any_hit, bounce, o, dd, tmax=None):
    tl, bl = builders(name)
    n = len(o)
    o, dd = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(dd, np.float32)
    tmax = np.ascontiguousarray(tmax if tmax is not None else np.zeros(n), np.float32)
    top, prim, vis, peak = (np.zeros(n, np.int32) for _ in range(4))
    t, info = np.zeros(n, np.float32), np.zeros(6, np.int32)
    rc = emu.hits_emu_stack_trace(_vp(d), _vp(cam), tl, bl, FORMATS[fmt], int(tight), int(any_hit), bounce, o.ctypes.data_as(f32p),
                                  dd.ctypes.data_as(f32p), tmax.ctypes.data_as(f32p), n, top.ctypes.data_as(i32p),
                                  prim.ctypes.data_as(i32p), t.ctypes.data_as(f32p), vis.ctypes.data_as(i32p),
                                  peak.ctypes.data_as(i32p), info.ctypes.data_as(i32p))
    assert rc == 0, f"hits_emu_stack_trace {rc}"
    return dict(top=top, prim=prim, t=t, vis=vis, peak=peak, format=int(info[0]), bound=int(info[1]), ring=int(info[2]),
                cap=int(info[3]), past=int(info[4]), err=int(info[5]))


def crossing(e):
    """Sample 0: the pixels whose camera ray crosses every member's box, and the
    decided wanted shadow rays (origin, direction, end, visible, crossing)."""
    sc = e["scene"]
    boxes = SC.member_boxes(sc)
    cam = np.array([pa.margin >= 1 and bool(boxes) and SC.crosses(boxes, pa.bounces[0]["o"], pa.bounces[0]["d"], P.INF)
                    for pa in e["paths"][0]])
    sh = [(o, a["dir"], a["end"], a["visible"], bool(boxes) and SC.crosses(boxes, o, a["dir"], a["end"]))
          for pa, k, a, o in XC.shadow_rays(e)]
    return cam, sh


def lower8(n8, root, octant):
    """The 8-wide format's lower bound for a ray of the given octant that hits
    every box, from the flattened DNode8 records and the order trav_step
    documents: the hit children are visited in ascending slot ^ octant, the
    others pushed, so a node leaves pending the used slots that come after the
    slot of the subtree the ray descends into.  Summed down the deepest path
    (at every node the internal child with the largest pending8)."""
    memo, total, item = {}, 0, root
    while item >> ITEM_SHIFT == ITEM_NODE:
        i = item & ((1 << ITEM_SHIFT) - 1)
        imask, lmask, base = (int(n8[i, 6]) >> 8) & 0xFF, int(n8[i, 6]) & 0xFF, int(n8[i, 3])
        slots = [s for s in range(8) if (imask >> s) & 1]
        if not slots:
            break
        k = max(range(len(slots)), key=lambda k: pending8(n8, base + k, memo))
        total += sum(1 for s in range(8) if ((imask | lmask) >> s) & 1 and (s ^ octant) > (slots[k] ^ octant))
        item = base + k
    return total


def octants(d):
    d = np.asarray(d, np.float32).reshape(-1, 3)
    return set(int(x) for x in (np.signbit(d[:, 0]) * 1 + np.signbit(d[:, 1]) * 2 + np.signbit(d[:, 2]) * 4))




@pytest.mark.parametrize("name,variant,fmt", SC.FORMAT_ROWS, ids=["-".join(x for x in r if x) for r in SC.FORMAT_ROWS])
def test_peak_within_the_bound(g, emu, name, variant, fmt):
    c = SC.CASES[name]
    e = c.expected(g, variant)
    b, d, cam, ids = c.build(g, variant)
    what = f"{name}[{variant}] host {fmt}"
    cam_cross, sh = crossing(e)
    # the lower bound by the ray's octant: the 8-wide order is by octant, not by distance, so there it comes from the records
    lower, lower_sh = c.lower(variant) if c.lower else (0, 0)
    low = {o: (lower, lower_sh) for o in range(8)}
    if taken(name, variant, fmt) == 2 and c.lower:
        i8 = stack_info(emu, d, name, fmt, arrays=True)
        low = {o: (lower8(i8["n8"], int(i8["roots"][1]), o),) * 2 for o in range(8)}
    oct_cam = np.array([next(iter(octants(x))) for x in e["ray"][0][0][:, 3:6]])
    oct_sh = np.array([next(iter(octants(x[1]))) for x in sh], int)
    runs = {}
    for tight in (0, 1):
        peaks = []
        for k in range(e["depth"]):
            want = e["obj"][0][k]
            pix = np.flatnonzero(want != -2)
            r = stack_trace(emu, d, cam, name, fmt, tight, False, k, e["ray"][0][k][pix, 0:3], e["ray"][0][k][pix, 3:6])
            assert r["format"] == taken(name, variant, fmt), f"{what}: node format {r['format']}"
            assert (r["err"], r["past"]) == (0, 0), f"{what} b{k} tight {tight}: error flag {r['err']}, words past the capacity {r['past']}"
            assert r["cap"] == (max(1, min(K_STACK_MAX, r["bound"]) - r["ring"]) if tight else K_STACK_MAX)
            top, prim, t = np.full(PC.N, -2, np.int32), np.full(PC.N, -2, np.int32), np.full(PC.N, -1.0)
            top[pix], prim[pix], t[pix] = r["top"], r["prim"], r["t"]
            check_records(what, grp(c, variant), e, ids, 0, k, top, t, e["ray"][0][k].astype(np.float32), None, "device")
            check_prims(what, c, e, 0, k, prim)
            peak = np.zeros(PC.N, np.int32)
            peak[pix] = r["peak"]
            peaks.append(peak)
            runs[(tight, k)] = r
        so, sd, se = (np.array([x[i] for x in sh]) for i in range(3))
        vis, scross = np.array([x[3] for x in sh]), np.array([x[4] for x in sh], bool)
        rs = stack_trace(emu, d, cam, name, fmt, tight, True, 0, so, sd, se)
        assert (rs["err"], rs["past"]) == (0, 0), f"{what} shadow tight {tight}: error flag {rs['err']}, past {rs['past']}"
        bad = np.flatnonzero(rs["vis"] != vis)
        assert len(bad) == 0, f"{what}: shadow visibility differs at rays {bad[:8]}: {rs['vis'][bad[:8]]} want {vis[bad[:8]].astype(int)}"
        runs[(tight, "sh")] = rs
        bound = rs["bound"]
        everything = max(int(np.max(p)) if len(p) else 0 for p in peaks + [rs["peak"]])
        assert everything <= bound, f"{what}: a ray held {everything} words, the bound is {bound}"
        if name == "balanced":
            assert everything <= K_LDS_STACK, f"{what}: a ray held {everything} words, the product's ring is {K_LDS_STACK}"
            continue
        pc, ps = peaks[0][cam_cross], rs["peak"][scross]
        assert cam_cross.sum() >= 12 and scross.sum() >= (12 if e["scene"].lights else 0)
        for o in sorted(set(oct_cam[cam_cross])):      # (a peak inside the ring reads 0: a bound the ring covers cannot be seen)
            got = int(peaks[0][cam_cross & (oct_cam == o)].max())
            assert got >= low[o][0] or low[o][0] <= rs["ring"], f"{what}: the crossing camera rays of octant {o} hold at most {got} words, the construction gives {low[o][0]}"
        for o in sorted(set(oct_sh[scross])):
            got = int(rs["peak"][scross & (oct_sh == o)].max())
            assert got >= low[o][1] or low[o][1] <= rs["ring"], \
                f"{what}: the crossing shadow rays of octant {o} hold at most {got} words, the construction gives {low[o][1]}"
        if taken(name, variant, fmt) == 2 and e["scene"].lights:
            # From the construction alone the 8-wide order gives a bound on a pair of rays: a ray of octant o and one of
            # the opposite octant o ^ 7 visit every node's slots in opposite orders, so the used slots a node leaves
            # pending for the one are those it has already visited for the other, and the two peaks together hold every
            # item that hangs off the path: at least the 4-wide shadow bound.  A camera ray through the corner band and
            # the shadow ray that comes back along it from the wall are such a pair.
            for o in sorted(set(oct_cam[cam_cross]) & set(int(x) ^ 7 for x in oct_sh[scross])):
                pair = int(peaks[0][cam_cross & (oct_cam == o)].max()) + int(rs["peak"][scross & (oct_sh == (o ^ 7))].max())
                assert pair >= lower_sh or lower_sh <= 2 * rs["ring"], \
                    f"{what}: octants {o} and {o ^ 7} hold {pair} words together, the construction gives {lower_sh}"
        if not tight:
            lo_c = max(low[o][0] for o in set(oct_cam[cam_cross]))
            lo_s = max([low[o][1] for o in set(oct_sh[scross])] + [0])
            print(f"{what}: bound {bound} lower {lo_c} / {lo_s} peak closest {pc.max()} shadow {ps.max() if len(ps) else 0} any ray {everything}")
    # the product's capacity changes nothing
    for key in [(0, k) for k in range(e["depth"])] + [(0, "sh")]:
        a, bb = runs[key], runs[(1, key[1])]
        for f in ("top", "prim", "t", "vis", "peak"):
            assert np.array_equal(a[f], bb[f]), f"{what} {key}: {f} differs with the tight spill area"


# ---- the whole pipeline with the product's spill area -------------------------------
def render_tight(emu, d, cam, name, fmt, e):
    tl, bl = builders(name)
    out, info = np.zeros((PC.N, 3), np.float32), np.zeros(3, np.int32)
    rc = emu.hits_emu_render_blas(_vp(d), _vp(cam), FORMATS[fmt], tl, bl, PC.SEED, e["samples"], e["depth"], out.ctypes.data_as(f32p),
                                  info.ctypes.data_as(i32p))
    assert rc == 0, f"hits_emu_render_blas {rc} (6: a kernel flagged an internal error)"
    return out, [int(x) for x in info]


@pytest.mark.parametrize("name,variant,fmt", SC.FORMAT_ROWS, ids=["-".join(x for x in r if x) for r in SC.FORMAT_ROWS])
def test_host_pipeline_with_the_tight_spill_area(g, emu, name, variant, fmt):
    c = SC.CASES[name]
    e = c.expected(g, variant)
    b, d, cam, ids = c.build(g, variant)
    L, (used, bound, cap) = render_tight(emu, d, cam, name, fmt, e)
    assert used == taken(name, variant, fmt) and cap == max(1, min(K_STACK_MAX, bound) - 4)
    check_radiance(f"{name}[{variant}] host pipeline {fmt}, spill capacity {cap}", grp(c, variant), e, L, "device")


def test_host_tail_kernel_on_a_deep_stack(g, emu, monkeypatch):
    """chain_ref without a light at depth 12: k_tail takes every path after
    bounce 0 and gives the per-bounce kernels' frame bit for bit."""
    c = SC.CASES["chain_ref"]
    e = c.expected(g, "n12dark")
    b, d, cam, ids = c.build(g, "n12dark")
    per_bounce, info = render_tight(emu, d, cam, "chain_ref", "fp32", e)
    assert info[1] == FIGURES[("chain_ref", "n12dark")]["bound"] > K_LDS_STACK
    monkeypatch.setenv("RTG_EMU_TAIL", "0")
    tail, _ = render_tight(emu, d, cam, "chain_ref", "fp32", e)
    assert np.array_equal(per_bounce.view(np.uint32), tail.view(np.uint32))
    check_radiance("chain_ref[n12dark] host tail", grp(c, "n12dark"), e, tail, "device")
