"""CPU tests (-m "not gpu") of the coarse depth alignment (gdrnet_amd.refine.depth_offset / depth_align / refine_rgbd): the host restatement
tests/align_host.py -- its key map, its median, and on the host rasterizer's renders the premise (an estimate centimetres off along its ray
gets nothing from the ICP alone) and the purpose (two rounds of the median shift bring it within half of the ICP's distance gate, and the ICP
from there ends where it ends from the fixtures' own starts) -- the checks that raise before any launch, and the exported symbols.

The 10 mm bound is half of icp_refine's dist_gate (0.02 m), which is what the step is for; measured on the fixtures: at most 5 mm in total,
the fixture's own 5 mm start in a hashed direction included, which a shift along the ray cannot remove."""
import os

import numpy as np
import pytest
import torch

import align_host as AH
import icp_host as IH
from gdrnet_amd import cabi, refine, render, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_depth_align_workspace_bytes", "gdrn_depth_offset", "gdrn_depth_align")
CLEAN_BOUND, NOISY_BOUND = 1e-3, 0.1   # degrees and millimetres (tests/test_refine_cpu.py)
ALONG_RAY_BOUND_MM = 10.0               # half of the ICP's dist_gate


def test_the_key_map_is_strictly_monotonic():
    vals = synth.hash_normal(41, "keys", (4000,)).astype(np.float32)
    tiny = np.float32(1e-45)   # the smallest denormal
    fmax = np.finfo(np.float32).max
    edge = np.array([0.0, tiny, -tiny, 3 * tiny, -3 * tiny, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny, fmax, -fmax, 1.0, -1.0,
                     np.nextafter(np.float32(1.0), np.float32(2.0)), np.inf, -np.inf, 1e-40, -1e-40, 0.1, -0.1], dtype=np.float32)
    scaled = (vals[:1000].astype(np.float64) * 1e-41).astype(np.float32)   # hashed denormals
    d = np.unique(np.concatenate([vals, scaled, edge, vals * np.float32(1e30), vals * np.float32(1e-30)]))
    assert d.size > 8000 and (np.abs(d[np.isfinite(d)]) < np.finfo(np.float32).tiny).sum() > 500
    k = AH.key(d)
    assert k.dtype == np.uint32
    assert np.all(k[1:] > k[:-1])   # np.unique sorted the floats ascending (and merged -0.0 into 0.0): the keys ascend strictly
    assert AH.key(np.float32(0.0)) == 0x80000000 and AH.key(-tiny) == 0x7FFFFFFE and AH.key(tiny) == 0x80000001
    assert AH.key(np.float32(-np.inf)) < AH.key(-fmax) and AH.key(fmax) < AH.key(np.float32(np.inf))


def test_the_restated_median_is_numpys_for_odd_and_even_counts_and_for_ties():
    for n in (1, 2, 3, 4, 63, 64, 65, 1000, 1001):
        d = (0.2 * (synth.hash_uniform(42, f"median{n}", (n,)) - 0.5)).astype(np.float32)
        assert AH.median(d) == np.median(d.astype(np.float64)), n
        q = (np.round(d * 64.0) / 64.0).astype(np.float32)   # many ties, exact zeros, both signs
        assert AH.median(q) == np.median(q.astype(np.float64)), n
    assert AH.median(np.full(10, 0.25, np.float32)) == 0.25
    half = np.array([-0.1] * 5 + [0.1] * 5, dtype=np.float32)
    assert AH.median(half) == 0.0 and AH.median(half[:-1]) == np.float64(np.float32(-0.1))
    ren = np.array([[1.0, 1.0, 0.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    sc = np.array([[1.1, 0.0, 1.0, np.nan, np.inf, 1.5]], dtype=np.float32)
    d, mask, covered = AH.pair_differences(ren, sc, 0.2)
    assert covered == 5 and list(mask[0]) == [True, False, False, False, False, False] and d[0] == np.float32(1.1) - np.float32(1.0)
    res = AH.offset(ren, sc, 0.2, min_pairs=2)
    assert res["ok"] == 0 and np.isnan(res["offset"]) and res["pairs"] == 1 and res["covered"] == 5
    t = AH.shift([0.1, -0.2, 0.5], 0.05)
    assert t[2] == 0.5 + 0.05 and abs(t[0] / t[2] - 0.2) < 1e-15 and abs(t[1] / t[2] + 0.4) < 1e-15   # the origin keeps its image


@pytest.mark.parametrize("name,extra_mm,bound", (("sphere", 60.0, CLEAN_BOUND), ("noisy/mixed", -40.0, NOISY_BOUND)))
def test_the_shift_brings_a_start_the_icp_cannot_use_within_its_gate(name, extra_mm, bound):
    inputs = {"sphere": synth.make_refine_inputs("sphere")}
    inputs.update({inp["case"]: inp for inp in synth.make_refine_inputs("noisy")})
    inp, row = inputs[name], 0
    scene = synth.refine_scene(inp, IH.host_gt_depth(inp))[inp["frame"][row]]
    g = int(inp["target"][row])
    R_gt, t_gt = inp["R_gt"][g], inp["t_gt"][g]
    R0, t0 = inp["R0"][row], inp["t0"][row] + 1e-3 * extra_mm * t_gt / t_gt[2]
    ren, K = IH.host_renderer(inp, row), inp["K"][row]
    alone = IH.refine(ren, R0, t0, K, scene)
    assert alone["ok"] == 0 and alone["pairs"] < 64 and np.array_equal(alone["t"], t0) and np.array_equal(alone["R"], R0)   # the premise
    al = AH.align(ren, R0, t0, scene, rounds=2)
    u = t_gt / np.linalg.norm(t_gt)
    along = [1e3 * abs(float((tr["t"] - t_gt) @ u)) for tr in al["trace"]] + [1e3 * abs(float((al["t"] - t_gt) @ u))]
    total = 1e3 * float(np.linalg.norm(al["t"] - t_gt))
    print(f"{name} {extra_mm:+g} mm: along-ray error {along[0]:.2f} -> {along[1]:.2f} -> {along[2]:.2f} mm, total {total:.3f} mm, pairs "
          f"{[tr['pairs'] for tr in al['trace']]}, offsets {[float(tr['offset']) for tr in al['trace']]}")
    assert al["ok"] == 1 and len(al["trace"]) == 2 and all(tr["pairs"] >= 64 for tr in al["trace"])
    assert along[2] < ALONG_RAY_BOUND_MM, along
    res = IH.refine(ren, R0, al["t"], K, scene)
    re, te = IH.pose_errors(res["R"], res["t"], R_gt, t_gt)
    print(f"  the ICP from there: {re:.2e} deg, {te:.2e} mm after {res['iters_done']} steps, pairs {res['pairs']}")
    assert res["ok"] == 1 and re < bound and te < bound, (re, te)


def test_no_cpu_fallback_and_checks_before_any_launch():
    inp = synth.make_refine_inputs("sphere")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    R0, t0, K = (torch.from_numpy(inp[k]) for k in ("R0", "t0", "K"))
    scene = torch.zeros(1, inp["H"], inp["W"])
    ren = torch.zeros(2, inp["H"], inp["W"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.depth_offset(ren, scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.depth_offset(np.zeros((2, 4, 4), np.float32), scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.depth_align(meshes, inp["labels"], R0, t0, K, scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.refine_rgbd(meshes, inp["labels"], R0, t0, K, scene, inp["frame"])
    # the scalar arguments are judged before the device is
    for kw in (dict(gate=0.0), dict(gate=-0.2), dict(gate=float("nan")), dict(min_pairs=0)):
        with pytest.raises(ValueError):
            refine.depth_offset(ren, scene, inp["frame"], **kw)
        with pytest.raises(ValueError):
            refine.depth_align(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], **kw)
    with pytest.raises(ValueError):
        refine.depth_align(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], rounds=-1)
    for kw in (dict(gate=0.0), dict(rounds=-1), dict(align_min_pairs=0), dict(iters=-1), dict(min_pairs=5), dict(dist_gate=0.0), dict(normal_gate=-1.0)):
        with pytest.raises(ValueError):
            refine.refine_rgbd(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], **kw)


def test_entry_points_check_their_arguments_on_the_host():
    """nothing below touches a stream or a device pointer: the pointers are host memory and every call is refused (or has nothing to do)"""
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    zero, one_i = np.zeros(4, dtype=np.int32), np.ones(4, dtype=np.int32)
    p, z = one.ctypes.data, zero.ctypes.data
    ws = lib.gdrn_depth_align_workspace_bytes
    assert ws(0, 4, 4) == 0 and ws(1, 4, 4) == 8 + 4 * 4 + 16 * 4 and ws(2, 37, 53) == 2 * (8 + 3 * 4 + 37 * 53 * 4)
    assert ws(-1, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 4, 0) == -1 and ws(1, 65536, 32768) == -1
    assert ws(64, 4800, 6400) == 64 * (8 + 12 + 4800 * 6400 * 4) > 2 ** 31   # a long long
    off = lib.gdrn_depth_offset
    good = [p, p, z, z, 1, 1, 4, 4, 0.2, 64, p, z, z, z, p]
    for k, bad in ((5, -1), (6, 0), (7, 0), (4, -1), (8, 0.0), (8, -1.0), (8, float("nan")), (9, 0)):
        args = list(good)
        args[k] = bad
        assert off(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 10, 11, 12, 13, 14):   # a NULL pointer, each in turn
        args = list(good)
        args[k] = None
        assert off(*args, None) == -1, k
    assert off(*(good[:14] + [p + 4]), None) == -1                                  # a workspace that is not 8-byte aligned
    assert off(*(good[:4] + [0] + good[5:]), None) == -1                            # frame 0 of no frames
    assert off(*(good[:3] + [one_i.ctypes.data] + good[4:]), None) == -1            # frame 1 of one frame
    assert off(*(good[:5] + [70000] + good[6:]), None) == -2                        # instances beyond a grid dimension
    assert off(None, None, None, None, 0, 0, 4, 4, 0.2, 64, None, None, None, None, None, None) == 0   # N == 0
    al = lib.gdrn_depth_align
    good = [p, z, z, z, z, z, 1, 1, z, z, p, p, p, 1, p, z, z, 1, 4, 4, 0.01, 6.5, 2, 0.2, 64, p, z, z, z, p, p]
    for k, bad in ((13, -1), (18, 0), (19, 0), (17, -1), (22, -1), (24, 0), (23, 0.0), (6, 0), (7, 0), (20, 0.0), (21, 0.005)):
        args = list(good)
        args[k] = bad
        assert al(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 14, 15, 16, 25, 26, 27, 28, 29, 30):
        args = list(good)
        args[k] = None
        assert al(*args, None) == -1, k
    assert al(*(good[:9] + [one_i.ctypes.data] + good[10:]), None) == -1            # label 1 of one class
    assert al(*(good[:16] + [one_i.ctypes.data] + good[17:]), None) == -1           # frame 1 of one frame
    none = [None] * 6 + [1, 1] + [None] * 5 + [0] + [None] * 3 + [1, 4, 4, 0.01, 6.5, 2, 0.2, 64] + [None] * 6
    assert al(*none, None) == 0                                                     # N == 0


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "gdrn_depth_align_workspace_bytes" in cabi._RET_LL and "#define GDRN_ABI_VERSION 5" in header
    from gdrnet_amd import build

    assert "depth_align.hip" in build.SOURCES
    assert callable(refine.depth_offset) and callable(refine.depth_align) and callable(refine.refine_rgbd)
