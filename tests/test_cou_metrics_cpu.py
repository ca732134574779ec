"""CPU tests (-m "not gpu") of gdrnet_amd.cou_metrics: the host restatement (tests/cou_host.py) against golden G19 (the reference's
pose_error.cus / cou_mask / cou_bb on the fixture, tests/golden/make_golden_g19.py) by exact equality, the rows the fixture is meant to have, the
checks that raise before any launch, the exported symbols, and CouRecall's bookkeeping."""
import os

import numpy as np
import pytest
import torch

import cou_host as CH
from gdrnet_amd import cabi, cou_metrics as CM, render, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_cou_maps_workspace_bytes", "gdrn_cou_maps", "gdrn_cou_bb")


@pytest.fixture(scope="module")
def g19(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g19_cou_metrics.npz")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_host_cus_equals_the_reference(g19):
    assert int(g19["cus/seed"]) == synth.COU_SEEDS["cus"]
    inp, est, gt = CH.cus_scene()
    err, counts, boxes = CH.cou_maps(est, gt, "depth")
    assert counts.dtype == boxes.dtype == np.int32 and np.array_equal(counts, g19["cus/counts"]) and np.array_equal(boxes, g19["cus/boxes"])
    assert np.array_equal(_bits(err[:, 0]), _bits(g19["cus/cus"]))   # the same integers, the same division and subtraction
    rows = g19["cus/bb_rows"]
    assert np.array_equal(_bits(err[rows, 1]), _bits(g19["cus/cou_bb_proj"][rows]))
    others = np.setdiff1d(np.arange(len(err)), rows)
    assert len(others) == 2 and np.all(err[others, 1] == 1.0) and np.isnan(g19["cus/cou_bb_proj"][others]).all()   # an empty silhouette: 1.0


def test_host_cou_mask_equals_the_reference(g19):
    _, est, gt = CH.cus_scene()
    for as_mask, key in ((lambda d: (d > 0).astype(np.uint8) * 255, "cus/cou_mask_u8"), (lambda d: d > 0, "cus/cou_mask_bool")):
        err, counts, boxes = CH.cou_maps(as_mask(est), as_mask(gt), "mask")
        assert np.array_equal(_bits(err[:, 0]), _bits(g19[key])) and np.array_equal(counts, g19["cus/counts"])
        assert np.array_equal(boxes, g19["cus/boxes"])


def test_host_cou_bb_equals_the_reference(g19):
    pairs = g19["bb/pairs"]
    assert np.array_equal(pairs, np.array(synth.COU_BB_PAIRS, dtype=np.float64)) and len(pairs) == 16
    got = CH.cou_bb(pairs[:, 0], pairs[:, 1])
    assert np.array_equal(_bits(got), _bits(g19["bb/cou_bb"]))
    assert np.array_equal(_bits([CH.iou(a, b) for a, b in pairs]), _bits(g19["bb/iou"]))
    iou = g19["bb/iou"]
    assert iou[0] == 1.0 and not iou[[1, 2, 3, 4, 7, 8, 12]].any() and np.all((iou[[5, 6, 9, 10, 11, 13, 14, 15]] > 0) & (iou[[5, 6, 9, 10, 11, 13, 14, 15]] < 1))
    assert iou[5] == iou[6] and iou[9] == iou[10]
    # the rules the reference's comparisons do not pin: a NaN anywhere gives an IoU of 0
    nan = np.nan
    assert CH.iou([nan, 0, 2, 2], [0, 0, 2, 2]) == 0.0 and CH.iou([0, 0, 2, 2], [0, 0, 2, nan]) == 0.0 and CH.iou([0, 0, 2, 2], [nan, 0, 2, 2]) == 0.0


def test_host_coverage_rules():
    d = np.array([np.nan, -0.0, 0.0, -1.0, np.inf, 1e-45, np.finfo(np.float32).tiny, -np.inf, 1.0, -1e-45], dtype=np.float32)
    neg_nan = np.array([0xFFC00000, 0x7F800001, 0x7F800000, 0x00000001, 0x80000001], dtype=np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(CH.covered(d, "depth"), d > 0) and np.array_equal(CH.covered(neg_nan, "depth"), neg_nan > 0)
    assert list(CH.covered(d, "depth")) == [False, False, False, False, True, True, True, False, True, False]
    m = np.array([0, 1, 2, 128, 255], dtype=np.uint8)
    assert list(CH.covered(m, "mask")) == [False, True, True, True, True] and list(CH.covered(m.astype(bool), "mask")) == [False] + [True] * 4
    err, counts, boxes = CH.cou_maps(np.zeros((2, 3, 5), np.float32), np.zeros((2, 3, 5), np.float32), "depth")
    assert np.all(err == 1.0) and not counts.any() and np.all(boxes == np.array(CH.EMPTY_BOX))


def test_cus_fixture_has_the_rows_it_is_meant_to_have(g19):
    inp, est, gt = CH.cus_scene()
    assert est.shape == gt.shape == (14, 47, 61) and est.dtype == gt.dtype == np.float32 and (47 * 61) % 2 == 1
    assert sorted(set(inp["labels"])) == [0, 1, 2] and not inp["K"][:, 0, 1].any() and not np.array_equal(inp["K"][0], inp["K"][10])
    cus, counts, boxes = g19["cus/cus"], g19["cus/counts"], g19["cus/boxes"]
    assert CH.cus_missing_properties(inp, est, gt, cus, counts, boxes) == []
    r = inp["rows"]
    assert cus[r["exact"]] == 0.0 and cus[r["off_object"]] == 1.0 and counts[r["both_empty"], 1] == 0 and not est[r["est_outside"]].any()
    assert est[r["off_object"]].any() and gt[r["off_object"]].any() and counts[r["off_object"], 0] == 0
    assert boxes[r["cut_left"], 0, 0] == 0 and boxes[r["cut_right"], 0, 2] == 60 and boxes[r["cut_top"], 0, 1] == 0 and boxes[r["cut_bottom"], 0, 3] == 46
    g = cus[list(inp["graded"])]
    assert ((g > 0.25) & (g < 0.5)).sum() >= 2 and ((g > 0.5) & (g < 0.8)).sum() >= 2 and np.all(np.abs(cus - 0.5) > 1e-6)
    assert (cus < CM.CUS_TH).any() and (cus >= CM.CUS_TH).any() and list(g19["cus/bb_rows"]) == [0, 1] + list(range(4, 14))
    stats = {}
    CH.cus_scene(None, stats)
    assert stats["edge_band"] > 1e-6
    t = render.MeshTable(inp["vertices"], inp["faces"])
    assert t.num_classes == 3 and list(t.nfaces) == [12, 1280, 128]


def test_no_cpu_fallback_and_checks_before_any_launch():
    d = torch.zeros(2, 5, 7)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        CM.cou_from_depth(d, d)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        CM.cou_mask(d.to(torch.uint8), d.to(torch.bool))
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        CM.cou_from_depth(d.numpy(), d)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        CM.cou_bb(torch.zeros(3, 4), torch.zeros(3, 4))
    inp = synth.make_cou_inputs("cus")
    poses = [torch.from_numpy(inp[k]) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        CM.cus(render.MeshTable(inp["vertices"], inp["faces"]), inp["labels"], *poses, inp["H"], inp["W"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        CM.CouRecall(inp["obj_names"]).update(torch.zeros(3, dtype=torch.float64), [0, 1, 2])
    with pytest.raises(cabi.GdrnHipError):
        CM.CouRecall(inp["obj_names"]).add_missing(0, 1)
    # dtypes and shapes: judged before the device is
    for bad in (d.double(), d.half(), d.to(torch.uint8), d.to(torch.int32)):
        with pytest.raises(ValueError, match="depth_est is"):
            CM.cou_from_depth(bad, d)
    with pytest.raises(ValueError, match="depth_gt is"):
        CM.cou_from_depth(d, d.to(torch.bool))
    for bad in (d, d.to(torch.int8), d.to(torch.int64)):
        with pytest.raises(ValueError, match="mask_est is"):
            CM.cou_mask(bad, d.to(torch.uint8))
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        CM.cou_from_depth(d[0], d[0])
    with pytest.raises(ValueError, match="differ in shape"):
        CM.cou_from_depth(d, d[:, :, :6])
    with pytest.raises(ValueError, match="differ in shape"):
        CM.cou_mask(d.to(torch.uint8), d[:1].to(torch.bool))
    with pytest.raises(ValueError, match="at least 1"):
        CM.cou_from_depth(d[:, :0], d[:, :0])
    with pytest.raises(ValueError):
        CM.CouRecall([])
    with pytest.raises(ValueError):
        CM.CouRecall(["a"]).add_missing(1, 1, device="cpu")


def test_entry_points_check_their_arguments_on_the_host():
    """nothing below touches a stream or a device pointer: the pointers are host memory and every call is refused (or has nothing to do)"""
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    p = one.ctypes.data
    maps = lib.gdrn_cou_maps
    assert maps(p, p, 2, 1, 4, 4, p, p, p, p, None) == -1 and maps(p, p, -1, 1, 4, 4, p, p, p, p, None) == -1            # the element kind
    assert maps(p, p, 0, -1, 4, 4, p, p, p, p, None) == -1 and maps(p, p, 0, 1, 0, 4, p, p, p, p, None) == -1 and maps(p, p, 1, 1, 4, 0, p, p, p, p, None) == -1
    assert maps(p, p, 0, 1, 65536, 32768, p, p, p, p, None) == -1 and maps(p, p, 1, 1, 46341, 46341, p, p, p, p, None) == -1   # H * W beyond an int
    assert maps(p, p, 0, 0, 65536, 32768, p, p, p, p, None) == -1                                                          # ... also without rows
    assert maps(p, p, 0, 1, 1, 2 ** 31 - 2048, p, p, p, p, None) == -1                                                     # no room for a chunk
    assert maps(p, p, 0, 70000, 32768, 32768, p, p, p, p, None) == -2                                                     # workgroups beyond an int
    for k in range(6):   # a NULL pointer, each in turn
        args = [p, p, 0, 1, 4, 4, p, p, p, p]
        args[(0, 1, 6, 7, 8, 9)[k]] = None
        assert maps(*args, None) == -1
    assert maps(None, None, 0, 0, 4, 4, None, None, None, None, None) == 0 and maps(None, None, 1, 0, 1, 1, None, None, None, None, None) == 0   # N == 0
    bb = lib.gdrn_cou_bb
    assert bb(p, p, -1, p, None) == -1 and bb(None, p, 1, p, None) == -1 and bb(p, None, 1, p, None) == -1 and bb(p, p, 1, None, None) == -1
    assert bb(None, None, 0, None, None) == 0
    ws = lib.gdrn_cou_maps_workspace_bytes
    assert ws(0) == 0 and ws(1) == 40 and ws(14) == 560 and ws(-1) == -1 and ws(2 ** 31 - 1) == 40 * (2 ** 31 - 1) > 2 ** 31   # a long long


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
    assert "gdrn_cou_maps_workspace_bytes" in cabi._RET_LL and "GDRN_COU_DEPTH = 0, GDRN_COU_MASK = 1" in header and "#define GDRN_ABI_VERSION 5" in header
    assert CM.KINDS == {"depth": 0, "mask": 1} and CM.CUS_TH == 0.5
    from gdrnet_amd import build

    assert "cou_metrics.hip" in build.SOURCES


def test_cou_recall_bookkeeping_on_hand_made_errors():
    err = np.array([0.0, 0.49, 0.5, 0.51, 1.0, np.nan, 0.25, np.nextafter(0.5, 0.0)])
    labels = np.array([0, 0, 0, 1, 1, 1, 2, 2])
    ref = CH.recall_counts(err, labels, 4, 0.5, {3: 2, 0: 1})
    assert list(ref["correct"]) == [2, 0, 2, 0] and list(ref["seen"]) == [4, 3, 2, 2]   # an error equal to the threshold is not correct, nor is NaN
    rec = CM.CouRecall(["a", "b", "c", "d"])
    assert rec.th == 0.5 and rec.num_classes == 4
    empty = rec.summarize()
    assert empty["objects"] == {} and np.isnan(empty["all"]) and empty["targets"] == 0 and not rec.counters()["seen"].any()
    # the counters are plain device tensors: hand-fill them where a GPU is absent (update itself runs in the GPU test)
    rec._state = torch.from_numpy(np.stack([ref["correct"], ref["seen"]]))
    rec.add_missing(1, 2)
    with pytest.raises(ValueError):
        rec.add_missing(4, 1)
    with pytest.raises(ValueError):
        rec.add_missing(0, -1)
    got = rec.counters()
    assert list(got["correct"]) == [2, 0, 2, 0] and list(got["seen"]) == [4, 5, 2, 2] and got["seen"].dtype == np.int64
    out = rec.summarize()
    assert out["objects"] == {"a": 0.5, "b": 0.0, "c": 1.0, "d": 0.0} and out["all"] == 4 / 13 and out["targets"] == 13 and out["th"] == 0.5
    assert out["rows"][0] == ["objects", "recall(<0.5)"] and out["rows"][1] == ["a", "50.00"] and out["rows"][-1] == ["all(13)", "30.77"]
    rec.reset()
    assert not rec.counters()["seen"].any() and not rec.counters()["correct"].any()
