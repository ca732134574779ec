"""CPU tests (-m "not gpu") of gdrnet_amd.refine: the host restatement of the depth refinement (tests/icp_host.py) on the host rasterizer's
renders -- its own invariants, and the conditions the fixtures of synth.make_refine_inputs must meet before the device is judged on them -- the
checks that raise before any launch, and the exported symbols.

The geometric bounds are properties of the inputs, not tolerances of a kernel: from 5 degrees / 5 mm, ten iterations end within a thousandth of
a degree and of a millimetre on the clean icospheres and within a tenth on the frames rounded to millimetres -- "a tenth of the perturbation or
better".  tests/test_refine_gpu.py holds the device to the same figures."""
import os

import numpy as np
import pytest
import torch

import icp_host as IH
from gdrnet_amd import cabi, refine, render, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_icp_workspace_bytes", "gdrn_icp_accumulate", "gdrn_icp_step", "gdrn_icp_refine")
CLEAN_BOUND, NOISY_BOUND = 1e-3, 0.1   # degrees and millimetres


@pytest.fixture(scope="module")
def loops():
    """the restatement's ten iterations from the 5 degree / 5 mm start of every convergence fixture, run once: name -> (inp, row, scene, result)"""
    out = {}
    scenes = [synth.make_refine_inputs("sphere"), synth.make_refine_inputs("mixed")] + synth.make_refine_inputs("noisy")
    for inp in scenes:
        scene = synth.refine_scene(inp, IH.host_gt_depth(inp))
        row = 0
        assert inp["start_deg"][row] == 5.0 and inp["start_mm"][row] == 5.0 and row in inp["convergent"]
        res = IH.refine(IH.host_renderer(inp, row), inp["R0"][row], inp["t0"][row], inp["K"][row], scene[inp["frame"][row]])
        out[inp["case"]] = (inp, row, scene, res)
    return out


def test_at_the_ground_truth_the_gradient_is_zero_and_the_step_is_the_identity(loops):
    inp, row, scene, _ = loops["sphere"]
    R, t = inp["R_gt"][0], inp["t_gt"][0]
    acc = IH.accumulate(IH.host_renderer(inp, row)(R, t), scene[0], inp["K"][row])
    assert acc["pairs"] > 1000 and not acc["b"].any() and acc["sq"] == 0.0 and not acc["r"].any()   # the render IS the frame: every residual is 0
    sol = IH.solve(acc["A"], acc["b"], acc["pairs"])
    assert sol["ok"] and not sol["xi"].any() and sol["min_pivot"] > 1e-3
    R1, t1, conv = IH.step(R, t, sol["xi"])
    assert np.array_equal(R1, R) and np.array_equal(t1, t) and conv
    res = IH.refine(IH.host_renderer(inp, row), R, t, inp["K"][row], scene[0], iters=3)
    assert res["ok"] == 1 and res["iters_done"] == 1 and res["rms"] == 0.0 and np.array_equal(res["R"], R)   # the stop rule froze it
    np.testing.assert_allclose(acc["A"], acc["A"].T, rtol=0, atol=0)
    assert np.all(np.abs(np.linalg.norm(acc["n"], axis=1) - 1.0) < 1e-15)


def test_flipping_every_normal_changes_nothing(loops):
    inp, row, scene, _ = loops["sphere"]
    ren = IH.host_renderer(inp, row)(inp["R0"][row], inp["t0"][row])
    a, b = IH.accumulate(ren, scene[0], inp["K"][row]), IH.accumulate(ren, scene[0], inp["K"][row], flip_normals=True)
    assert a["pairs"] == b["pairs"] > 1000 and np.array_equal(a["n"], -b["n"]) and a["b"].any()
    for k in ("A", "b", "sq", "A_abs", "b_abs"):
        assert np.array_equal(a[k], b[k]), k   # every term is even in n, sign changes are exact


def test_a_plane_and_an_empty_overlap_are_degenerate():
    inp = synth.make_refine_inputs("degenerate")
    scene = synth.refine_scene(inp, IH.host_gt_depth(inp))
    assert scene.shape == (1, 64, 64) and (scene > 0).all()   # the rectangle fills its frame up to the last row and column
    results = [IH.refine(IH.host_renderer(inp, row), inp["R0"][row], inp["t0"][row], inp["K"][row], scene[0], iters=3) for row in range(3)]
    for row, res in enumerate(results):
        assert res["ok"] == 0 and res["iters_done"] == 0 and len(res["trace"]) == 1, row
        assert np.array_equal(res["R"], inp["R0"][row]) and np.array_equal(res["t"], inp["t0"][row]), row
    plane = results[0]["trace"][0]
    assert plane["acc"]["pairs"] == 62 * 62 and results[0]["rms"] > 1e-4   # every pixel off the border pairs up, and the residual is real
    n = plane["acc"]["n"]
    assert np.all(n == n[0]) and abs(n[0, 2]) == 1.0                       # all normals equal: along the optical axis
    A = plane["acc"]["A"]
    assert A[2, 2] == 0.0 and A[3, 3] == 0.0 and A[4, 4] == 0.0            # the rotation in the plane and the two slides are unobservable
    assert IH.scaled(A)[0] is None
    B = synth.hash_normal(7, "rank5", (5, 6))                              # rank 5 with a positive diagonal: passes the diagonal test, fails on a pivot
    low = IH.solve(B.T @ B, np.ones(6), 100)
    assert IH.scaled(B.T @ B)[0] is not None and low["ok"] is False and abs(low["min_pivot"]) < 1e-12
    for res in results[1:]:                                                # out of the frame | behind the camera: nothing overlaps
        assert res["pairs"] == 0 and np.isnan(res["rms"])
    few = IH.solve(np.eye(6), np.zeros(6), 63)
    assert few["ok"] is False and IH.solve(np.eye(6), np.zeros(6), 64)["ok"] is True


def test_the_fixtures_converge_within_a_tenth_of_their_perturbation_or_better(loops):
    for name, bound in (("sphere", CLEAN_BOUND), ("mixed", CLEAN_BOUND), ("noisy/sphere", NOISY_BOUND), ("noisy/mixed", NOISY_BOUND)):
        inp, row, scene, res = loops[name]
        g = int(inp["target"][row])
        re0, te0 = IH.pose_errors(inp["R0"][row], inp["t0"][row], inp["R_gt"][g], inp["t_gt"][g])
        re, te = IH.pose_errors(res["R"], res["t"], inp["R_gt"][g], inp["t_gt"][g])
        piv = min(tr["sol"]["min_pivot"] for tr in res["trace"])
        cond = max(tr["sol"]["cond"] for tr in res["trace"])
        npairs = [tr["acc"]["pairs"] for tr in res["trace"]]
        print(f"{name}: start {re0:.3f} deg {te0:.3f} mm -> {re:.2e} deg {te:.2e} mm after {res['iters_done']} steps, rms {res['rms']:.2e} m, pairs "
              f"{min(npairs)}..{max(npairs)}, smallest scaled pivot {piv:.2e}, cond {cond:.1e}")
        assert abs(re0 - 5.0) < 1e-9 and abs(te0 - 5.0) < 1e-9
        assert res["ok"] == 1 and res["iters_done"] <= 10
        assert re < bound and te < bound, (name, re, te)
        assert piv > 1e-3 and min(npairs) >= 400                # six orders above the pivot threshold, well above min_pairs = 64
    noisy = loops["noisy/sphere"]
    s = noisy[2][0]
    assert np.array_equal(s, (np.round(s.astype(np.float64) * 1000.0) / 1000.0).astype(np.float32)) and (s > 0).any()   # whole millimetres
    clean = loops["sphere"][2][0]
    ys, xs = np.nonzero(clean > 0)
    third = slice(int(xs.min()), int(xs.min()) + (int(xs.max()) - int(xs.min()) + 1) // 3)
    box = s[int(ys.min()) : int(ys.max()) + 1, third]
    assert np.all(box == box[0, 0]) and abs(float(box[0, 0]) - (float(clean[clean > 0].min()) - 0.05)) < 1e-3   # the occluder, 5 cm in front
    assert loops["noisy/sphere"][3]["pairs"] < loops["sphere"][3]["pairs"]


def test_mixed_holds_what_it_is_meant_to_hold():
    inp = synth.make_refine_inputs("mixed")
    assert list(inp["labels"]) == [2, 0, 1, 1, 0, 2] and list(inp["frame"]) == [0, 0, 0, 1, 1, 0] and inp["num_frames"] == 2
    assert inp["convergent"] == (0, 5) and (inp["H"], inp["W"]) == (120, 160) and inp["H"] % 16 != 0   # a last band of 8 rows
    t = render.MeshTable(inp["vertices"], inp["faces"])
    assert list(t.nfaces) == [12, 2048, 1280]
    sph = synth.make_refine_inputs("sphere")
    assert (sph["H"], sph["W"]) == (96, 128) and list(sph["start_deg"]) == [5.0, 2.0] and len(sph["faces"][0]) == 1280


def test_no_cpu_fallback_and_checks_before_any_launch():
    inp = synth.make_refine_inputs("sphere")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    R0, t0, K = (torch.from_numpy(inp[k]) for k in ("R0", "t0", "K"))
    scene = torch.zeros(1, inp["H"], inp["W"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.icp_refine(meshes, inp["labels"], R0, t0, K, scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.normal_equations(torch.zeros(2, inp["H"], inp["W"]), scene, inp["frame"], K)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.normal_equations(np.zeros((2, 4, 4), np.float32), scene, inp["frame"], K)
    # the scalar arguments are judged before the device is
    for kw in (dict(dist_gate=0.0), dict(dist_gate=-0.02), dict(normal_gate=0.0), dict(normal_gate=float("nan")), dict(iters=-1), dict(min_pairs=5)):
        with pytest.raises(ValueError):
            refine.icp_refine(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], **kw)
    for kw in (dict(dist_gate=0.0), dict(normal_gate=-1.0)):
        with pytest.raises(ValueError):
            refine.normal_equations(torch.zeros(2, inp["H"], inp["W"]), scene, inp["frame"], K, **kw)


def test_entry_points_check_their_arguments_on_the_host():
    """nothing below touches a stream or a device pointer: the pointers are host memory and every call is refused (or has nothing to do)"""
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    zero = np.zeros(4, dtype=np.int32)
    p, z = one.ctypes.data, zero.ctypes.data
    ws = lib.gdrn_icp_workspace_bytes
    assert ws(0, 4, 4) == 0 and ws(1, 16, 4) == 28 * 8 + 3 * 4 and ws(1, 17, 4) == 2 * 28 * 8 + 4 * 4 and ws(5, 120, 160) == 5 * (8 * 28 * 8 + 10 * 4)
    assert ws(-1, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 4, 0) == -1 and ws(1, 65536, 32768) == -1
    assert ws(65535, 16 * 4096, 4) == 65535 * (4096 * 28 * 8 + 4098 * 4) > 2 ** 31   # a long long
    acc = lib.gdrn_icp_accumulate
    good = [p, p, z, z, 1, p, 1, 4, 4, 0.02, 0.01, p, p, p]
    for k, bad in ((6, -1), (7, 0), (8, 0), (4, -1), (9, 0.0), (9, -1.0), (10, 0.0), (9, float("nan"))):
        args = list(good)
        args[k] = bad
        assert acc(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 5, 11, 12, 13):   # a NULL pointer, each in turn
        args = list(good)
        args[k] = None
        assert acc(*args, None) == -1, k
    assert acc(*(good[:13] + [p + 4]), None) == -1                                  # a workspace that is not 8-byte aligned
    assert acc(*(good[:4] + [0] + good[5:]), None) == -1                            # frame 0 of no frames
    one_i = np.ones(4, dtype=np.int32)
    assert acc(*(good[:3] + [one_i.ctypes.data] + good[4:]), None) == -1            # frame 1 of one frame
    assert acc(*(good[:6] + [70000] + good[7:]), None) == -2                        # instances beyond a grid dimension
    assert acc(None, None, None, None, 0, None, 0, 4, 4, 0.02, 0.01, None, None, None, None) == 0   # N == 0
    st = lib.gdrn_icp_step
    assert st(p, z, -1, 64, p, p, z, None) == -1 and st(p, z, 1, 5, p, p, z, None) == -1 and st(None, None, 0, 64, None, None, None, None) == 0
    for k in (0, 1, 4, 5, 6):
        args = [p, z, 1, 64, p, p, z]
        args[k] = None
        assert st(*args, None) == -1, k
    ref = lib.gdrn_icp_refine
    good = [p, z, z, z, z, z, 1, 1, z, z, p, p, p, 1, p, z, z, 1, 4, 4, 0.01, 6.5, 10, 0.02, 0.01, 64, p, z, z, z, p, p]
    for k, bad in ((13, -1), (18, 0), (19, 0), (17, -1), (22, -1), (25, 5), (23, 0.0), (24, 0.0), (6, 0), (7, 0), (20, 0.0), (21, 0.005)):
        args = list(good)
        args[k] = bad
        assert ref(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 14, 15, 16, 26, 27, 28, 29, 30, 31):
        args = list(good)
        args[k] = None
        assert ref(*args, None) == -1, k
    assert ref(*(good[:9] + [one_i.ctypes.data] + good[10:]), None) == -1           # label 1 of one class
    assert ref(*(good[:16] + [one_i.ctypes.data] + good[17:]), None) == -1          # frame 1 of one frame
    none = [None] * 6 + [1, 1] + [None] * 5 + [0] + [None] * 3 + [1, 4, 4, 0.01, 6.5, 10, 0.02, 0.01, 64] + [None] * 6
    assert ref(*none, None) == 0                                                    # N == 0


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "gdrn_icp_workspace_bytes" in cabi._RET_LL and "#define GDRN_ABI_VERSION 5" in header
    assert "GDRN_ICP_RUNNING = 0, GDRN_ICP_CONVERGED = 1, GDRN_ICP_DEGENERATE = 2" in header
    assert (refine.RUNNING, refine.CONVERGED, refine.DEGENERATE) == (0, 1, 2)
    from gdrnet_amd import build

    assert "icp.hip" in build.SOURCES
