"""CPU tests (-m "not gpu") of the hypothesis verification (gdrnet_amd.verify): the exported symbols, the checks that raise before any launch,
and the host restatement tests/verify_host.py against geometry on the host rasterizer's renders -- among the candidates of a ground truth
(itself, the fixtures' starts, shifts along its viewing ray and across it) the ground truth scores strictly highest, with and without the
observed mask, at three values of tau.

The masks: the pixels where a ground truth's own render lies within 1.5 mm of the frame (what a perfect detector would return, occluders cut
out).  Nothing here is tuned: the rule is the header's, and the candidates were fixed before the rule was run on them."""
import os

import numpy as np
import pytest
import torch

import icp_host as IH
import verify_host as VH
from gdrnet_amd import cabi, render, synth, verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_verify_workspace_bytes", "gdrn_verify_maps", "gdrn_verify_score", "gdrn_verify_select", "gdrn_verify_poses")
TAUS = (0.005, 0.01, 0.02)
ALONG_MM = (-8.0, 8.0, -30.0, 30.0)   # along the ground truth's viewing ray: minus is towards the camera
MASK_MM = 1.5


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "gdrn_verify_workspace_bytes" in cabi._RET_LL and "#define GDRN_ABI_VERSION 5" in header
    assert "Hypothesis verification behind the refinement above (added within ABI 5: new entry points, nothing changed)" in header
    from gdrnet_amd import build

    assert "verify.hip" in build.SOURCES
    assert all(callable(getattr(verify, f)) for f in ("verify_maps", "verify_poses", "select_best", "best_of"))


def test_no_cpu_fallback_and_checks_before_any_launch():
    inp = synth.make_refine_inputs("sphere")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    R0, t0, K = (torch.from_numpy(inp[k]) for k in ("R0", "t0", "K"))
    H, W = inp["H"], inp["W"]
    scene, ren = torch.zeros(1, H, W), torch.zeros(2, H, W)
    mask = torch.zeros(2, H, W, dtype=torch.uint8)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        verify.verify_maps(ren, scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        verify.verify_maps(ren, scene, inp["frame"], mask)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        verify.verify_maps(np.zeros((2, 4, 4), np.float32), scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        verify.verify_poses(meshes, inp["labels"], R0, t0, K, scene, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        verify.select_best(torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.int32), [0, 0], 1)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        verify.best_of(meshes, inp["labels"], [(R0, t0)], K, scene, inp["frame"])
    # the scalar arguments are judged before the device is
    bad = (dict(tau=0.0), dict(tau=-0.01), dict(tau=float("nan")), dict(tau=1.0000001), dict(tau=float("inf")), dict(penalty=-1e-9),
           dict(penalty=float("inf")), dict(penalty=float("nan")), dict(min_covered=0), dict(min_covered=-3))
    for kw in bad:
        with pytest.raises(ValueError):
            verify.verify_maps(ren, scene, inp["frame"], **kw)
        with pytest.raises(ValueError):
            verify.verify_poses(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], **kw)
        with pytest.raises(ValueError):
            verify.best_of(meshes, inp["labels"], [(R0, t0)], K, scene, inp["frame"], **kw)
    with pytest.raises(cabi.GdrnHipError):   # tau == 1 and penalty == 0 are allowed: the next check is the device's
        verify.verify_maps(ren, scene, inp["frame"], tau=1.0, penalty=0.0, min_covered=1)
    with pytest.raises(ValueError):
        verify.select_best(torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.int32), [0, 0], -1)
    # so are the mask's dtype, its rank and, without an index, its rows
    for m in (mask.float(), mask.to(torch.int32), mask[0], mask[:, None]):
        with pytest.raises(ValueError, match="mask_obs"):
            verify.verify_maps(ren, scene, inp["frame"], m)
        with pytest.raises(ValueError, match="mask_obs"):
            verify.verify_poses(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], m)
    with pytest.raises(ValueError, match="mask_index"):   # one mask for two candidates
        verify.verify_maps(ren, scene, inp["frame"], mask[:1])
    with pytest.raises(ValueError, match="mask_index"):
        verify.verify_poses(meshes, inp["labels"], R0, t0, K, scene, inp["frame"], torch.zeros(3, H, W, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask_index without mask_obs"):
        verify.verify_maps(ren, scene, inp["frame"], None, [0, 0])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):   # with an index the rows may differ: the next check is the device's
        verify.verify_maps(ren, scene, inp["frame"], mask[:1], [0, 0])


def test_entry_points_check_their_arguments_on_the_host():
    """nothing below touches a stream or a device pointer: the pointers are host memory and every call is refused (or has nothing to do)"""
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    zero, one_i, two_i = np.zeros(4, dtype=np.int32), np.ones(4, dtype=np.int32), np.full(4, 2, dtype=np.int32)
    p, z = one.ctypes.data, zero.ctypes.data
    ws = lib.gdrn_verify_workspace_bytes
    assert ws(0, 4, 4) == 0 and ws(1, 4, 4) == 32 and ws(9, 37, 53) == 9 * 32
    assert ws(-1, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 4, 0) == -1 and ws(1, 65536, 32768) == -1 and ws(1, 46340, 46340) == 32
    maps = lib.gdrn_verify_maps
    #       0  1  2  3  4  5  6  7  8  9 10 11   12   13 14 15
    good = [p, p, z, z, 1, p, z, z, 1, 2, 4, 4, 0.01, z, p, p]
    for k, bad in ((9, -1), (10, 0), (11, 0), (4, -1), (12, 0.0), (12, -0.01), (12, float("nan")), (12, 1.5), (12, float("inf")), (8, 0)):
        args = list(good)
        args[k] = bad
        assert maps(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 13, 14, 15, 6, 7):   # a NULL pointer, each in turn (6, 7: one copy of the mask index without the other)
        args = list(good)
        args[k] = None
        assert maps(*args, None) == -1, k
    assert maps(*(good[:15] + [p + 4]), None) == -1                                  # a workspace that is not 8-byte aligned
    assert maps(*(good[:3] + [one_i.ctypes.data] + good[4:]), None) == -1            # frame 1 of one frame
    assert maps(*(good[:4] + [0] + good[5:]), None) == -1                            # frame 0 of no frames
    assert maps(*(good[:7] + [one_i.ctypes.data] + good[8:]), None) == -1            # mask 1 of one mask
    assert maps(*(good[:7] + [two_i.ctypes.data, 2] + good[9:]), None) == -1         # mask 2 of two masks
    assert maps(*(good[:6] + [None, None, 1] + good[9:]), None) == -1                # no index: one mask for two candidates
    assert maps(*(good[:9] + [70000] + good[10:]), None) == -2                       # candidates beyond a grid dimension
    assert maps(*([None] * 4 + [0] + [None] * 3 + [0, 0, 4, 4, 0.01] + [None] * 3), None) == 0   # N == 0
    score = lib.gdrn_verify_score
    good = [z, p, 2, 1, 0.01, 1.0, 64, p, z]
    for k, bad in ((2, -1), (4, 0.0), (4, 1.5), (4, float("nan")), (5, -1.0), (5, float("inf")), (5, float("nan")), (6, 0), (0, None), (1, None),
                   (7, None), (8, None)):
        args = list(good)
        args[k] = bad
        assert score(*args, None) == -1, (k, bad)
    assert score(None, None, 0, 0, 0.01, 1.0, 64, None, None, None) == 0
    select = lib.gdrn_verify_select
    good = [p, z, z, z, 2, 1, z, p]
    for k, bad in ((4, -1), (5, -1), (0, None), (1, None), (2, None), (3, None), (6, None), (7, None), (7, p + 4), (3, one_i.ctypes.data), (5, 0)):
        args = list(good)
        args[k] = bad
        assert select(*args, None) == -1, (k, bad)
    assert select(None, None, None, None, 0, 0, None, None, None) == 0
    poses = lib.gdrn_verify_poses
    #       0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18 19  20    21  22 23 24 25  26    27  28  29 30 31 32 33 34
    good = [p, z, z, z, z, z, 1, 1, z, z, p, p, p, 1, p, z, z, 1, 4, 4, 0.01, 6.5, p, z, z, 1, 0.01, 1.0, 64, p, z, p, p, z, p]
    for k, bad in ((13, -1), (18, 0), (19, 0), (17, -1), (26, 0.0), (26, 2.0), (27, -1.0), (27, float("inf")), (28, 0), (6, 0), (7, 0), (20, 0.0),
                   (21, 0.005), (25, 0)):
        args = list(good)
        args[k] = bad
        assert poses(*args, None) == -1, (k, bad)
    for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 14, 15, 16, 23, 24, 29, 30, 31, 32, 33, 34):
        args = list(good)
        args[k] = None
        assert poses(*args, None) == -1, k
    assert poses(*(good[:9] + [one_i.ctypes.data] + good[10:]), None) == -1           # label 1 of one class
    assert poses(*(good[:16] + [one_i.ctypes.data] + good[17:]), None) == -1          # frame 1 of one frame
    assert poses(*(good[:24] + [one_i.ctypes.data] + good[25:]), None) == -1          # mask 1 of one mask
    none = [None] * 6 + [1, 1] + [None] * 5 + [0] + [None] * 3 + [1, 4, 4, 0.01, 6.5] + [None] * 3 + [0, 0.01, 1.0, 64] + [None] * 6
    assert poses(*none, None) == 0                                                    # N == 0


def test_the_restated_rules_on_a_row_written_out_by_hand():
    tau = float(np.float32(0.25))
    ren = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, np.nan, 1.0, 1.0]], dtype=np.float32)
    sc = np.array([[1.0, 0.75, 0.5, 1.25, 1.5, 0.0, 1.0, 1.0, np.nan, np.inf]], dtype=np.float32)
    mask = np.array([[1, 1, 1, 0, 1, 1, 1, 0, 0, 0]], dtype=np.uint8)
    c = VH.counts(ren, sc, tau, mask)
    # pixels: inlier e = 0 | inlier e = +tau | occluded | inlier e = -tau | violated | unknown (0) | uncovered | uncovered (NaN) | unknown | unknown
    assert c == dict(covered=8, inlier=3, occluded=1, violated=1, unknown=3, visible=7, mask_px=6, inter=4, sum_q=2 * 262144)
    s, ok = VH.score(c, True, tau, penalty=1.0, min_covered=8)
    assert ok == 1 and s == ((4.0 / 9.0) * (3.0 - 2.0) - 1.0) / 8.0
    assert VH.score(c, False, tau, 0.5, 8) == (((3.0 - 2.0) - 0.5) / 8.0, 1)
    s, ok = VH.score(c, True, tau, 1.0, 9)
    assert ok == 0 and s == -np.inf
    best, val = VH.select(np.array([0.5, -np.inf, 0.75, 0.75, -1.0, np.nan, 2.0]), np.array([1, 0, 1, 1, 1, 1, 0]), np.array([0, 1, 0, 0, 2, 2, 2]), 4)
    assert list(best) == [2, -1, 4, -1] and list(val) == [0.75, -np.inf, -1.0, -np.inf]
    assert VH.key(-0.0) < VH.key(0.0) < VH.key(5e-324) and VH.key(-np.inf) > 0 and VH.key(-1.0) < VH.key(-0.5)


def _along(t, mm):
    """the translation moved so that its depth grows by ``mm`` millimetres and the model origin keeps its image"""
    return t * (1.0 + 1e-3 * mm / t[2])


def _scene_candidates(inp):
    """per ground truth of a scene: dict(g, frame, names, ren [C,H,W], mask [H,W]) with the candidates the issue names, rendered on the host"""
    gt_depth = IH.host_gt_depth(inp)
    frames = synth.refine_scene(inp, gt_depth)
    K_of = {int(g): inp["K"][i] for i, g in enumerate(inp["target"])}
    out = []
    for g, label in enumerate(inp["gt_labels"]):
        K = K_of.get(g, inp["K"][0])
        ren = VH.host_renderer(inp, label, K)
        f = int(inp["gt_frame"][g])
        R_gt, t_gt = inp["R_gt"][g], inp["t_gt"][g]
        cands = [("gt", R_gt, t_gt)]
        for row in np.nonzero(inp["target"] == g)[0]:
            cands.append((f"start {inp['start_deg'][row]:g}/{inp['start_mm'][row]:g}", inp["R0"][row], inp["t0"][row]))
        cands += [(f"ray {mm:+g}", R_gt, _along(t_gt, mm)) for mm in ALONG_MM]
        cands.append(("x +10", R_gt, t_gt + np.array([0.010, 0.0, 0.0])))
        with np.errstate(invalid="ignore"):
            mask = ((gt_depth[g] > 0) & (np.abs(gt_depth[g].astype(np.float64) - frames[f].astype(np.float64)) <= 1e-3 * MASK_MM)).astype(np.uint8)
        out.append(dict(g=g, frame=frames[f], names=[c[0] for c in cands], mask=mask,
                        ren=np.stack([gt_depth[g]] + [ren(R, t) for _, R, t in cands[1:]])))
    return out


@pytest.fixture(scope="module")
def groups():
    """every ground truth of "sphere", "mixed" and both "noisy" scenes with its candidates: list of (scene name, dict of _scene_candidates)"""
    scenes = [synth.make_refine_inputs("sphere"), synth.make_refine_inputs("mixed")] + synth.make_refine_inputs("noisy")
    return [(inp["case"], grp) for inp in scenes for grp in _scene_candidates(inp)]


def _verified(grp, tau, with_mask):
    C = len(grp["names"])
    return VH.verify(grp["ren"], grp["frame"][None], np.zeros(C, int), grp["mask"][None] if with_mask else None,
                     np.zeros(C, int) if with_mask else None, tau=tau)


@pytest.mark.parametrize("with_mask", (False, True))
@pytest.mark.parametrize("tau", TAUS)
def test_the_ground_truth_wins_its_group_on_the_host_rasterizers_renders(groups, tau, with_mask):
    assert len(groups) == 8
    for name, grp in groups:
        res = _verified(grp, tau, with_mask)
        names, s = grp["names"], res["score"]
        order = np.argsort(-s)
        print(f"{name} gt {grp['g']} tau {tau} mask {with_mask}: " + ", ".join(f"{names[k]} {s[k]:.3f}" for k in order[:3]) +
              f" | covered {res['covered'][0]}, occluded {res['occluded'][0]}, mask_px {res['mask_px'][0]}")
        assert res["ok"].all() and names[0] == "gt"
        assert np.all(s[0] > s[1:]), (name, grp["g"], dict(zip(names, s)))                       # strictly the highest
        best, best_score = VH.select(s, res["ok"], np.zeros(len(s), int), 1)
        assert best[0] == 0 and best_score[0] == s[0]
        if "start 2/2" in names and "start 5/5" in names:
            assert s[names.index("start 2/2")] > s[names.index("start 5/5")], (name, grp["g"])
        far = names.index("ray +30")
        assert res["occluded"][far] == res["covered"][far] > 0 and res["inlier"][far] == 0 and s[far] == 0.0 and not np.signbit(s[far])
        near = names.index("ray -30")
        assert res["inlier"][near] <= 2 and s[near] < 0.0, (name, grp["g"], res["inlier"][near], s[near])


def test_identities_hold_on_every_row(groups):
    for tau in TAUS:
        for with_mask in (False, True):
            for name, grp in groups:
                r = _verified(grp, tau, with_mask)
                assert np.array_equal(r["covered"], r["inlier"] + r["occluded"] + r["violated"] + r["unknown"])
                assert np.array_equal(r["visible"], r["covered"] - r["occluded"])
                assert np.all(r["inter"] <= np.minimum(r["visible"], r["mask_px"]))
                assert np.all(r["sum_q"] >= 0) and np.all(r["sum_q"] <= r["inlier"].astype(np.int64) * int(np.floor(tau * 2.0 ** 20)))
                assert np.all(r["score"] <= 1.0) and np.all(r["score"] >= -1.0)
                if not with_mask:
                    assert not r["mask_px"].any() and not r["inter"].any()
