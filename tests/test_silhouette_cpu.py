"""CPU tests (-m "not gpu") of the silhouette term of gdrnet_amd.refine: the host restatement tests/sil_host.py against scipy's exact distance
transform, against the reference's edge rule (golden G20) and, on the host rasterizer's renders of synth.make_silhouette_inputs, against
geometry; the checks that raise before any launch, and the exported symbols.

The geometric bounds are properties of the inputs: the contour is pixel-quantised, so the lateral translation ends within one pixel's footprint,
z / fx = 0.6 m / 600 = 1.0 mm, and the rotation within one pixel at the half-length of the plate's long side, atan(1 / 40) = 1.43 degrees.
tests/test_silhouette_gpu.py holds the device to the same figures.

Measured with the restatement (20 iterations, weight 1, gate 8 px), worst over the rows that depth alone leaves untouched:
  "isolated"  lateral 0.414 mm, rotation 0.728 degrees (the issue's prototype: 0.47 mm / 0.73 degrees)
  "occluded"  lateral 0.175 mm, rotation 0.443 degrees (prototype: 0.25 mm / 0.49 degrees)
The cube seen on three faces ends within 1e-6 degrees / mm of the depth-only result."""
import os

import numpy as np
import pytest
import torch

import contour_masks
import icp_host as IH
import sil_host as SH
from gdrnet_amd import cabi, refine, render, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_sil_workspace_bytes", "gdrn_sil_contour_transform", "gdrn_sil_accumulate", "gdrn_icp_step_sil", "gdrn_icp_refine_sil")
LATERAL_MM = 1e3 * 0.6 / 600.0                       # one pixel's footprint at the objects' depth
ROTATION_DEG = float(np.degrees(np.arctan(1.0 / 40.0)))   # one pixel at the half-length (40 px) of the plate's long side
CLEAN_BOUND = 1e-3                                   # degrees and millimetres (tests/test_refine_cpu.py)


@pytest.fixture(scope="module")
def loops():
    """both loops of the restatement from every start of both fixtures, run once: case -> (inp, frames, masks, [depth-only], [with the term])"""
    out = {}
    for case in synth.SILHOUETTE_CASES:
        inp = synth.make_silhouette_inputs(case)
        frames, masks = synth.silhouette_scene(inp, SH.host_gt_depth(inp))
        dep, sil = [], []
        for row in range(len(inp["labels"])):
            g, ren = int(inp["target"][row]), IH.host_renderer(inp, row)
            dep.append(IH.refine(ren, inp["R0"][row], inp["t0"][row], inp["K"][row], frames[g]))
            sil.append(SH.refine(ren, inp["R0"][row], inp["t0"][row], inp["K"][row], frames[g], masks[g]))
        out[case] = (inp, frames, masks, dep, sil)
    return out


def test_the_transform_equals_scipys_exact_distance_transform():
    from scipy.ndimage import distance_transform_edt

    for name, mask in contour_masks.masks().items():
        edge = SH.observed_contour(mask)
        d2, nearest = SH.transform(edge)
        H, W = mask.shape
        if not edge.any():
            assert (d2 == SH.INT32_MAX).all() and (nearest == -1).all(), name
            continue
        idx = distance_transform_edt(~edge, return_distances=False, return_indices=True)
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        want = (idx[0] - y) ** 2 + (idx[1] - x) ** 2
        assert np.array_equal(d2, want), name
        cy, cx = nearest // W, nearest % W       # (scipy breaks ties its own way: only the restatement's own consistency is checked)
        assert edge[cy, cx].all() and np.array_equal((cy - y) ** 2 + (cx - x) ** 2, d2), name
        assert np.array_equal(nearest[edge], (y * W + x)[edge]) and not d2[edge].any(), name


def test_the_observed_contour_is_the_references_get_edge(golden_dir):
    g = np.load(os.path.join(golden_dir, "g20_contours.npz"))
    masks = contour_masks.masks()
    assert sorted(g.files) == sorted("edge/" + k for k in masks) and len(masks) == 6 + 5 * len(contour_masks.RANDOM_SHAPES)
    total = 0
    for name, mask in masks.items():
        edge = SH.observed_contour(mask)       # no depth: the exclusion is this project's own
        assert np.array_equal(edge, g["edge/" + name] != 0), name
        total += int(edge.sum())
    assert total > 5000
    full = np.ones((5, 7), np.uint8)
    assert not SH.observed_contour(full).any()                      # the frame border is no edge
    full[2, 3] = 0
    assert SH.observed_contour(full).sum() == 4


def test_an_occluders_boundary_is_no_contour_and_hidden_pixels_are_no_pairs(loops):
    inp, frames, masks, _, _ = loops["occluded"]
    for g in range(len(masks)):
        plain, kept = SH.observed_contour(masks[g]), SH.observed_contour(masks[g], frames[g])
        assert not (kept & ~plain).any() and 15 < (plain & ~kept).sum() < 80
        ys, xs = np.nonzero(plain & ~kept)
        assert len(set(xs)) == 1 and np.all(frames[g][ys, xs - 1] < frames[g][ys, xs]) and np.all(masks[g][ys, xs - 1] == 0)   # the block's right edge
        row = int(np.nonzero(inp["target"] == g)[0][0])
        ren = IH.host_renderer(inp, row)(inp["R_gt"][g], inp["t_gt"][g])
        hidden_on = SH.rendered_contour(ren, frames[g])
        hidden_off = SH.rendered_contour(ren, ren)
        assert not (hidden_on & ~hidden_off).any() and (hidden_off & ~hidden_on).sum() > 20 and not hidden_on[:, : xs[0]].any()
    iso = loops["isolated"]
    for g in range(4):                          # alone in its frame: the depth rule excludes nothing
        assert np.array_equal(SH.observed_contour(iso[2][g]), SH.observed_contour(iso[2][g], iso[1][g]))


def test_at_the_ground_truth_the_silhouette_residual_is_zero(loops):
    inp, frames, masks, _, _ = loops["isolated"]
    for g in range(4):
        row = 4 * g
        tr = SH.contour_transform(masks[g], frames[g])
        acc = SH.accumulate(frames[g], frames[g], inp["K"][row], tr["d2"], tr["nearest"])
        assert acc["pairs"] == tr["contour"] > 200 and acc["sq"] == 0.0 and not acc["b"].any() and not acc["r"].any()
        np.testing.assert_array_equal(acc["A"], acc["A"].T)
        assert IH.solve(acc["A"], acc["b"], acc["pairs"])["ok"]      # the contour alone sees all six directions
        none = SH.accumulate(frames[g], frames[g], inp["K"][row], tr["d2"] + 2, tr["nearest"], sil_gate=1.0)
        assert none["pairs"] == 0 and not none["A"].any()


def _report(case, inp, dep, sil, rows):
    worst = [0.0, 0.0]
    for row in rows:
        g = int(inp["target"][row])
        re, lat = SH.lateral_errors(sil[row]["R"], sil[row]["t"], inp["R_gt"][g], inp["t_gt"][g])
        _, te = IH.pose_errors(sil[row]["R"], sil[row]["t"], inp["R_gt"][g], inp["t_gt"][g])
        print(f"{case} row {row} (gt {g}) from {inp['start_deg'][row]:g} deg / {inp['start_mm'][row]:.2f} mm: depth-only ok {dep[row]['ok']}; with the term ok "
              f"{sil[row]['ok']} after {sil[row]['iters_done']} steps: {re:.4f} deg, lateral {lat:.4f} mm (|dt| {te:.4f} mm), pairs {sil[row]['pairs']} + "
              f"{sil[row]['sil_pairs']}, sil_rms {sil[row]['sil_rms']:.2e} m")
        worst = [max(worst[0], lat), max(worst[1], re)]
        assert sil[row]["ok"] == 1 and sil[row]["iters_done"] >= 1, (case, row)
        assert lat <= LATERAL_MM and re <= ROTATION_DEG, (case, row, lat, re)
    print(f"{case}: worst lateral {worst[0]:.3f} mm (bound {LATERAL_MM:.2f}), worst rotation {worst[1]:.3f} deg (bound {ROTATION_DEG:.2f})")


def test_flat_faced_objects_stop_sliding_on_isolated(loops):
    inp, _, _, dep, sil = loops["isolated"]
    assert inp["flat"] == tuple(range(12))
    for row in inp["flat"]:                     # the plates and the two-face cube: depth alone finds them degenerate and leaves the pose
        assert dep[row]["ok"] == 0 and dep[row]["iters_done"] == 0, row
        assert np.array_equal(dep[row]["R"], inp["R0"][row]) and np.array_equal(dep[row]["t"], inp["t0"][row]), row
    _report("isolated", inp, dep, sil, inp["flat"])
    for row in range(12, 16):                   # the cube seen on three faces converges already: the term moves it by less than the clean bound
        assert dep[row]["ok"] == 1 and sil[row]["ok"] == 1
        re, te = IH.pose_errors(sil[row]["R"], sil[row]["t"], dep[row]["R"], dep[row]["t"])
        print(f"isolated row {row}: {re:.2e} deg, {te:.2e} mm from the depth-only result")
        assert re < CLEAN_BOUND and te < CLEAN_BOUND, (row, re, te)


def test_flat_faced_objects_stop_sliding_on_occluded(loops):
    inp, _, _, dep, sil = loops["occluded"]
    assert inp["flat"] == tuple(range(10)) and len(inp["labels"]) == 10
    for row in inp["flat"]:
        assert dep[row]["ok"] == 0 and np.array_equal(dep[row]["t"], inp["t0"][row]), row
    _report("occluded", inp, dep, sil, inp["flat"])


def test_the_fixtures_hold_what_they_are_meant_to_hold():
    inp = synth.make_silhouette_inputs("isolated")
    assert (inp["H"], inp["W"]) == (96, 128) and list(inp["gt_labels"]) == [0, 0, 1, 1] and list(inp["frame"]) == [g for g in range(4) for _ in range(4)]
    assert np.array_equal(inp["K"][3], [[600, 0, 63.5], [0, 600, 47.5], [0, 0, 1]]) and np.array_equal(inp["t_gt"][2], [0.004, -0.003, 0.6])
    t = render.MeshTable(inp["vertices"], inp["faces"])
    assert list(t.nfaces) == [24, 12]
    assert np.allclose(inp["start_deg"][:4], [0, 3, 2, 4]) and np.allclose(1e3 * (inp["t0"][3] - inp["t_gt"][0]), [-4, 3, -3])
    assert np.array_equal(inp["R0"][0], inp["R_gt"][0]) and np.array_equal(inp["R_gt"][0], np.eye(3))
    occ = synth.make_silhouette_inputs("occluded")
    assert np.array_equal(occ["R_gt"], inp["R_gt"][1:3]) and occ["occluded"] == (0, 1) and np.allclose(1e3 * (occ["t0"][4] - occ["t_gt"][0]), [4, 2, 1])
    frames, masks = synth.silhouette_scene(occ, SH.host_gt_depth(occ))
    gt = SH.host_gt_depth(occ)
    for g in range(2):
        ys, xs = np.nonzero(gt[g] > 0)
        x1, third = int(xs.min()), (int(xs.max()) - int(xs.min()) + 1) // 3
        block = frames[g] == np.float32(np.float64(gt[g][gt[g] > 0].min()) - synth.REFINE_OCCLUDER)
        by, bx = np.nonzero(block)
        assert (bx.min(), bx.max(), by.min(), by.max()) == (x1 - 6, x1 + third - 1, ys.min() - 6, ys.max() + 6)
        assert np.array_equal(masks[g] != 0, (gt[g] > 0) & ~block) and ((gt[g] > 0) & block).sum() > 0.25 * (gt[g] > 0).sum()
    with pytest.raises(ValueError):
        synth.make_silhouette_inputs("mixed")


def test_no_cpu_fallback_and_checks_before_any_launch():
    inp = synth.make_silhouette_inputs("isolated")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    R0, t0, K = (torch.from_numpy(inp[k]) for k in ("R0", "t0", "K"))
    N, H, W = len(inp["labels"]), inp["H"], inp["W"]
    scene, mask = torch.zeros(4, H, W), torch.zeros(N, H, W, dtype=torch.uint8)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.icp_refine_sil(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], mask)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.contour_transform(mask, scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.contour_transform(mask.numpy(), scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.silhouette_equations(torch.zeros(N, H, W), mask, scene, inp["frame"], K)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.refine_rgbd(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], mask_obs=mask)
    # the scalar arguments are judged before the device is
    for kw in (dict(sil_gate=0.0), dict(sil_gate=float("nan")), dict(sil_weight=-1.0), dict(sil_weight=float("inf")), dict(sil_weight=float("nan")),
               dict(dist_gate=0.0), dict(normal_gate=-1.0), dict(iters=-1), dict(min_pairs=5)):
        with pytest.raises(ValueError):
            refine.icp_refine_sil(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], mask, **kw)
    for kw in (dict(sil_gate=0.0), dict(dist_gate=-0.02)):
        with pytest.raises(ValueError):
            refine.silhouette_equations(torch.zeros(N, H, W), mask, scene, inp["frame"], K, **kw)
    for kw in (dict(sil_gate=-1.0), dict(sil_weight=float("nan"))):
        with pytest.raises(ValueError):
            refine.refine_rgbd(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], mask_obs=mask, **kw)


def test_entry_points_check_their_arguments_on_the_host():
    """nothing below touches a stream or a device pointer: the pointers are host memory and every call is refused (or has nothing to do)"""
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    zero = np.zeros(16, dtype=np.int32)
    one_i = np.ones(4, dtype=np.int32)
    p, z = one.ctypes.data, zero.ctypes.data
    ws = lib.gdrn_sil_workspace_bytes
    icp = lambda n, h, w: (lib.gdrn_icp_workspace_bytes(n, h, w) + 7) // 8 * 8  # noqa: E731
    for n, h, w in ((1, 16, 4), (1, 17, 4), (5, 120, 160), (3, 1, 1)):
        nb = (h + 15) // 16
        assert ws(n, h, w) == n * (nb + 1) * 28 * 8 + icp(n, h, w) + (3 * n * h * w + n * (nb + 4)) * 4 + n * h * w, (n, h, w)
    assert ws(0, 4, 4) == 0 and ws(-1, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 4, 0) == -1 and ws(1, 65536, 32768) == -1
    assert ws(1, 16385, 4) == -2 and ws(1, 4, 16385) == -2 and ws(1, 16384, 16384) > 2 ** 31   # a long long
    tr = lib.gdrn_sil_contour_transform
    good = [p, p, z, z, 1, 1, 4, 4, p, p, p, p]
    for k, bad, status in ((5, -1, -1), (6, 0, -1), (7, 0, -1), (4, -1, -1), (6, 16385, -2), (7, 16385, -2), (5, 70000, -2)):
        args = list(good)
        args[k] = bad
        assert tr(*args, None) == status, (k, bad)
    for k in (0, 1, 2, 3, 8, 9, 10, 11):   # a NULL pointer, each in turn
        args = list(good)
        args[k] = None
        assert tr(*args, None) == -1, k
    assert tr(*(good[:11] + [p + 4]), None) == -1                                   # a workspace that is not 8-byte aligned
    assert tr(*(good[:3] + [one_i.ctypes.data] + good[4:]), None) == -1             # frame 1 of one frame
    assert tr(None, None, None, None, 0, 0, 4, 4, None, None, None, None, None) == 0   # N == 0
    acc = lib.gdrn_sil_accumulate
    good = [p, p, z, z, 1, p, z, z, 1, 4, 4, 8.0, 0.02, p, z, p]
    for k, bad, status in ((8, -1, -1), (9, 0, -1), (10, 0, -1), (4, -1, -1), (11, 0.0, -1), (11, float("nan"), -1), (12, 0.0, -1), (12, -1.0, -1),
                           (9, 16385, -2), (8, 70000, -2)):
        args = list(good)
        args[k] = bad
        assert acc(*args, None) == status, (k, bad)
    for k in (0, 1, 2, 3, 5, 6, 7, 13, 14, 15):
        args = list(good)
        args[k] = None
        assert acc(*args, None) == -1, k
    assert acc(*(good[:15] + [p + 4]), None) == -1
    assert acc(*(good[:3] + [one_i.ctypes.data] + good[4:]), None) == -1
    assert acc(*([None] * 4 + [0] + [None] * 3 + [0, 4, 4, 8.0, 0.02] + [None] * 3), None) == 0
    st = lib.gdrn_icp_step_sil
    good = [p, z, p, z, 1.0, 1, 64, p, p, z]
    for k, bad in ((5, -1), (6, 5), (4, -0.5), (4, float("inf")), (4, float("nan"))):
        args = list(good)
        args[k] = bad
        assert st(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 7, 8, 9):
        args = list(good)
        args[k] = None
        assert st(*args, None) == -1, k
    assert st(None, None, None, None, 1.0, 0, 64, None, None, None, None) == 0
    ref = lib.gdrn_icp_refine_sil
    good = [p, z, z, z, z, z, 1, 1, z, z, p, p, p, 1, p, z, z, 1, p, 4, 4, 0.01, 6.5, 10, 0.02, 0.01, 64, 1.0, 8.0, p, z, z, z, p, z, p, p]
    for k, bad, status in ((13, -1, -1), (19, 0, -1), (20, 0, -1), (17, -1, -1), (23, -1, -1), (26, 5, -1), (24, 0.0, -1), (25, 0.0, -1), (6, 0, -1),
                           (7, 0, -1), (21, 0.0, -1), (22, 0.005, -1), (27, -1.0, -1), (27, float("nan"), -1), (28, 0.0, -1), (19, 16385, -2),
                           (20, 16385, -2), (13, 70000, -2)):
        args = list(good)
        args[k] = bad
        assert ref(*args, None) == status, (k, bad)
    for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 14, 15, 16, 18, 29, 30, 31, 32, 33, 34, 35, 36):
        args = list(good)
        args[k] = None
        assert ref(*args, None) == -1, k
    assert ref(*(good[:9] + [one_i.ctypes.data] + good[10:]), None) == -1           # label 1 of one class
    assert ref(*(good[:16] + [one_i.ctypes.data] + good[17:]), None) == -1          # frame 1 of one frame
    none = [None] * 6 + [1, 1] + [None] * 5 + [0] + [None] * 3 + [1, None, 4, 4, 0.01, 6.5, 10, 0.02, 0.01, 64, 1.0, 8.0] + [None] * 8
    assert ref(*none, None) == 0                                                    # N == 0


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "gdrn_sil_workspace_bytes" in cabi._RET_LL and "#define GDRN_ABI_VERSION 5" in header
    assert "Silhouette term for the depth refinement above (added within ABI 5: new entry points, nothing changed)" in header
    from gdrnet_amd import build

    assert "silhouette.hip" in build.SOURCES and "icp.hip" in build.SOURCES
    doc = refine.__doc__
    assert "icp_refine_sil" in doc and "There is no\nsilhouette term" not in doc
    assert "measured on real data" in refine.icp_refine_sil.__doc__
