"""Plain numpy restatement of the rules of gdrn_cou_maps / gdrn_cou_bb (include/gdrn_hip.h): coverage per element kind, the two counts, the two
boxes with the empty encoding, both errors and the empty cases.  No reference import: this is the project's own host oracle for
gdrnet_amd.cou_metrics, pinned to the reference's pose_error.cus / cou_mask / cou_bb by golden G19 (tests/test_cou_metrics_cpu.py) and shared by
the CPU and the GPU tests."""
import numpy as np

import render_host as RH
from gdrnet_amd import synth

EMPTY_BOX = (0, 0, -1, -1)


def covered(maps, kind):
    """bool array of the covered pixels.  "depth": fp32 > 0 as IEEE compares it, read off the bit pattern (0x00000001 .. 0x7f800000: positive
    subnormals and +inf are covered; +-0, negatives and NaNs are not).  "mask": the byte is non-zero (uint8 or bool storage)."""
    maps = np.ascontiguousarray(maps)
    if kind == "depth":
        assert maps.dtype == np.float32
        return (maps.view(np.uint32) - np.uint32(1)) < np.uint32(0x7F800000)   # (uint32 arithmetic wraps: 0 - 1 = 0xffffffff)
    assert kind == "mask" and maps.dtype in (np.uint8, np.bool_)
    return maps.view(np.uint8) != 0


def box_of(cov):
    """inclusive (x1, y1, x2, y2) of a [H,W] bool map, EMPTY_BOX without a pixel"""
    ys, xs = np.nonzero(cov)
    if len(xs) == 0:
        return EMPTY_BOX
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def iou(a, b):
    """the IoU of two x, y, w, h boxes: corners x + w, y + h; the intersection counts only when both of its sides are > 0; the denominator is
    (area_a + area_b) - area_inter; fp64 throughout, one operation at a time.  A NaN in either box gives 0."""
    a, b = [np.float64(v) for v in a], [np.float64(v) for v in b]
    if any(v != v for v in a + b):
        return 0.0
    brax, bray, brbx, brby = a[0] + a[2], a[1] + a[3], b[0] + b[2], b[1] + b[3]
    tlx, tly = max(a[0], b[0]), max(a[1], b[1])
    brx, bry = min(brax, brbx), min(bray, brby)
    w, h = brx - tlx, bry - tly
    if not (w > 0 and h > 0):
        return 0.0
    area_inter, area_a, area_b = w * h, a[2] * a[3], b[2] * b[3]
    with np.errstate(all="ignore"):
        return float(area_inter / ((area_a + area_b) - area_inter))


def cou_bb(bb_est, bb_gt):
    """[N] fp64: 1 - iou per pair of x, y, w, h boxes"""
    return np.array([1.0 - iou(a, b) for a, b in zip(np.asarray(bb_est), np.asarray(bb_gt))], dtype=np.float64).reshape(-1)


def xywh(box):
    x1, y1, x2, y2 = box
    return [x1, y1, x2 - x1 + 1, y2 - y1 + 1]


def cou_maps(est, gt, kind):
    """(err [N,2] fp64, counts [N,2] int32, boxes [N,2,4] int32) of two [N,H,W] maps, as gdrn_cou_maps writes them"""
    ce, cg = covered(est, kind), covered(gt, kind)
    N = ce.shape[0]
    err, counts, boxes = np.zeros((N, 2), np.float64), np.zeros((N, 2), np.int32), np.zeros((N, 2, 4), np.int32)
    for i in range(N):
        inter, union = int((ce[i] & cg[i]).sum()), int((ce[i] | cg[i]).sum())
        counts[i] = inter, union
        boxes[i, 0], boxes[i, 1] = box_of(ce[i]), box_of(cg[i])
        err[i, 0] = 1.0 - np.float64(inter) / np.float64(union) if union > 0 else 1.0
        empty = boxes[i, 0, 2] < 0 or boxes[i, 1, 2] < 0
        err[i, 1] = 1.0 if empty else 1.0 - iou(xywh(boxes[i, 0].tolist()), xywh(boxes[i, 1].tolist()))
    return err, counts, boxes


def recall_counts(err, labels, num_classes, th, missing=None):
    """per-class (correct [C], seen [C]) under the strict comparison err < th"""
    correct, seen = np.zeros(num_classes, np.int64), np.zeros(num_classes, np.int64)
    for e, c in zip(np.asarray(err), np.asarray(labels)):
        correct[c] += bool(e < th)
        seen[c] += 1
    for c, n in (missing or {}).items():
        seen[c] += n
    return dict(correct=correct, seen=seen)


_scenes = {}


def cus_scene(seed=None, stats=None):
    """(inputs, depth_est, depth_gt [N,H,W] fp32) of synth.make_cou_inputs("cus"), rendered by the host rasterizer; computed once per process
    and seed.  `stats` receives the rasterizer's edge_band over the 2N renders."""
    if seed not in _scenes:
        inp = synth.make_cou_inputs("cus", seed=seed)
        est, gt, band = [], [], np.inf
        for i, c in enumerate(inp["labels"]):
            for out, R, t in ((est, inp["R_est"][i], inp["t_est"][i]), (gt, inp["R_gt"][i], inp["t_gt"][i])):
                s = {}
                out.append(RH.render_one(inp["vertices"][c], inp["faces"][c], R, t, inp["K"][i], inp["H"], inp["W"], inp["near"], inp["far"], s))
                band = min(band, s.get("edge_band", np.inf))
        _scenes[seed] = (inp, np.stack(est), np.stack(gt), band)
    if stats is not None:
        stats["edge_band"] = _scenes[seed][3]
    return _scenes[seed][:3]


def cus_missing_properties(inp, est, gt, cus, counts, boxes):
    """the names of the rows synth.make_cou_inputs("cus") is meant to have and does not, judged on the cus [N], counts [N,2] and boxes [N,2,4]
    handed in (the golden's generator hands in the reference's): an empty list accepts the seed"""
    r, H, W = inp["rows"], inp["H"], inp["W"]
    inter, union = counts[:, 0], counts[:, 1]
    n_est, n_gt = (est > 0).sum((1, 2)), (gt > 0).sum((1, 2))
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)

    i = r["exact"]
    need(np.array_equal(est[i], gt[i]) and inter[i] == union[i] > 50 and cus[i] == 0.0, "exact")
    i = r["off_object"]
    need(n_est[i] > 50 and n_gt[i] > 50 and inter[i] == 0 and cus[i] == 1.0, "off_object")
    i = r["est_outside"]
    need(n_est[i] == 0 and n_gt[i] > 50 and cus[i] == 1.0 and tuple(boxes[i, 0]) == EMPTY_BOX, "est_outside")
    i = r["both_empty"]
    need(union[i] == 0 and cus[i] == 1.0 and tuple(boxes[i, 0]) == tuple(boxes[i, 1]) == EMPTY_BOX, "both_empty")
    for name, k, edge in (("cut_left", 0, 0), ("cut_right", 2, W - 1), ("cut_top", 1, 0), ("cut_bottom", 3, H - 1)):
        i = r[name]
        need(boxes[i, 0, k] == edge and boxes[i, 1, k] != edge and n_est[i] > 20 and 0 < inter[i] < union[i], name)
    g = cus[list(inp["graded"])]
    need(((g > 0.25) & (g < 0.5)).sum() >= 2, "two graded rows in (0.25, 0.5)")
    need(((g > 0.5) & (g < 0.8)).sum() >= 2, "two graded rows in (0.5, 0.8)")
    need(np.all(np.abs(cus - 0.5) > 1e-6), "no cus within 1e-6 of 0.5")
    return bad


def hash_maps(seed, name, shape, kind, coverage=0.3):
    """random maps of `coverage` covered pixels from the repo's hash RNG: depth values in (0.3, 1.3) or 0, mask bytes 1 .. 255 or 0"""
    u, v = synth.hash_uniform(seed, name + "/cov", shape), synth.hash_uniform(seed, name + "/val", shape)
    if kind == "depth":
        return np.where(u < coverage, 0.3 + v, 0.0).astype(np.float32)
    return np.where(u < coverage, 1 + np.floor(255 * v), 0).astype(np.uint8)
