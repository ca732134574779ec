"""The complement-over-union pose errors -- cus, cou_mask, cou_bb, cou_bb_proj -- and their recall on the device (csrc/cou_metrics.hip).

Host-side mirror of the one family of error types of the reference's ``lib/pysixd/scripts/eval_calc_errors.py`` (:34, :418-424) that
``pose_metrics``, ``bop_metrics`` and ``sixd_scores`` leave out:

* ``pose_error.cus``          -- lib/pysixd/pose_error.py:487-531: 1 - |est and gt| / |est or gt| of the silhouettes (depth > 0) of the model
  rendered under the estimated and the ground-truth pose, here ``render.render_depth`` for the whole batch in one call; scored with
  ``correct_th["cus"] = [0.5]`` (eval_calc_scores.py:47)
* ``pose_error.cou_mask``     -- :466-484: the same between a predicted and an annotated mask (``astype(bool)``)
* ``pose_error.cou_bb``       -- :534-542: 1 - ``misc.iou`` of two x, y, w, h boxes
* ``pose_error.cou_bb_proj``  -- :545-589 as it is meant: the shipped function calls ``misc.calc_2d_bbox``, which does not exist; the box is
  ``misc.calc_2d_bbox_xywh(xs, ys, ., ., clip=False)`` = x_min, y_min, x_max - x_min + 1, y_max - y_min + 1, passed through ``misc.iou``

One fused pass reads each map once and gives, per row, the two pixel counts, the two boxes and both errors.  An empty silhouette (where the
reference's box raises ``ValueError``) gives a box error of 1.0, an empty union a ``cus`` of 1.0 as in the reference.  The sphere-projection
shortcut of eval_calc_errors.py:331-335, 419-424 is not applied: it never changes the value (disjoint silhouettes already give 1.0).  One
estimate per ground-truth target is assumed, as in ``bop_metrics``.  Errors stay on the device; ``CouRecall.summarize()`` makes the one
device-to-host copy.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import cabi, devargs, render

CUS_TH = 0.5                    # correct_th["cus"], eval_calc_scores.py:47
KINDS = {"depth": 0, "mask": 1}   # GDRN_COU_DEPTH, GDRN_COU_MASK
WHERE = "the complement-over-union errors"   # (this module in devargs' error sentence)


def _maps(est, gt, dtypes, names):
    """both maps checked -- a tensor of one of ``dtypes``, [N,H,W], equal shapes (ValueError), on the device (``devargs``' sentence) -- and
    contiguous; bool storage is read as bytes"""
    out = []
    for t, what in zip((est, gt), names):
        if not isinstance(t, torch.Tensor):
            raise devargs.no_fallback(what, WHERE)
        if t.dtype not in dtypes:
            raise ValueError(f"{what} is {t.dtype}: {' or '.join(str(d) for d in dtypes)}")
        if t.dim() != 3:
            raise ValueError(f"{what} must be [N, H, W]")
        out.append(t)
    if out[0].shape != out[1].shape:
        raise ValueError(f"{names[0]} {tuple(out[0].shape)} and {names[1]} {tuple(out[1].shape)} differ in shape")
    if min(out[0].shape[1:]) < 1:
        raise ValueError(f"{names[0]}: H and W are at least 1")
    out = [devargs.device_tensor(t, None, None, what, WHERE) for t, what in zip(out, names)]
    if out[0].device != out[1].device:
        raise ValueError(f"{names[0]} is on {out[0].device}, {names[1]} on {out[1].device}")
    return [t.view(torch.uint8) if t.dtype == torch.bool else t for t in out]


def _cou_maps(est, gt, kind, return_parts):
    N, H, W = (int(s) for s in est.shape)
    dev = est.device
    lib = cabi.load()
    err = torch.empty(max(N, 1), 2, dtype=torch.float64, device=dev)[:N]
    counts = torch.empty(max(N, 1), 2, dtype=torch.int32, device=dev)[:N]
    boxes = torch.empty(max(N, 1), 2, 4, dtype=torch.int32, device=dev)[:N]
    ws = devargs.workspace(lib.gdrn_cou_maps_workspace_bytes(N), dev, "cou_maps_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_cou_maps(p(est), p(gt), KINDS[kind], N, H, W, p(err), p(counts), p(boxes), p(ws), devargs.stream(dev)), "cou_maps")
    return (err, counts, boxes) if return_parts else err


def cou_from_depth(depth_est, depth_gt, return_parts=False):
    """``pose_error.cus`` and ``cou_bb_proj`` of N estimates on depth maps that are already rendered: ``depth_est`` / ``depth_gt`` [N,H,W] fp32
    device tensors (the model under the estimated / ground-truth pose); a pixel is covered iff its value is > 0 (NaN, +-0 and negatives are not,
    +inf and subnormals are).  Returns err [N,2] fp64 on the device -- column 0 ``cus``, column 1 ``cou_bb_proj`` (1.0 where a silhouette is
    empty); with ``return_parts`` also counts [N,2] int32 = |intersection|, |union| and boxes [N,2,4] int32 = the inclusive x1, y1, x2, y2 of
    the estimated, then the ground-truth silhouette, (0, 0, -1, -1) for an empty one."""
    est, gt = _maps(depth_est, depth_gt, (torch.float32,), ("depth_est", "depth_gt"))
    return _cou_maps(est, gt, "depth", return_parts)


def cou_mask(mask_est, mask_gt, return_parts=False):
    """``pose_error.cou_mask`` of N mask pairs: ``mask_est`` / ``mask_gt`` [N,H,W] uint8 or bool device tensors, a pixel set iff its byte is
    non-zero.  Returns what ``cou_from_depth`` returns: column 0 ``cou_mask``, column 1 the box error of the two masks."""
    est, gt = _maps(mask_est, mask_gt, (torch.uint8, torch.bool), ("mask_est", "mask_gt"))
    return _cou_maps(est, gt, "mask", return_parts)


def cus(meshes, labels, R_est, t_est, R_gt, t_gt, K, H, W, near=render.NEAR, far=render.FAR, return_parts=False):
    """``pose_error.cus`` (and ``cou_bb_proj``) of N estimates from their poses: the model ``labels[i]`` of the ``render.MeshTable`` ``meshes`` is
    rendered under the estimated and the ground-truth pose -- all 2N instances with ONE ``render_depth`` call -- and scored by
    ``cou_from_depth``.  Poses and K: device tensors, fp32 or fp64.  The silhouettes are the rasterizer's (its rules: include/gdrn_hip.h).
    Nothing is read back."""
    R_est, t_est, K, N = devargs.poses(R_est, t_est, K, WHERE)
    R_gt, t_gt = devargs.device_tensor(R_gt, torch.float64, (-1, 3, 3), "R_gt", WHERE), devargs.device_tensor(t_gt, torch.float64, (-1, 3), "t_gt", WHERE)
    if R_gt.shape[0] != N or t_gt.shape[0] != N:
        raise ValueError("R_est, t_est, R_gt and t_gt need one entry per row")
    dev = R_est.device
    _, lab_host = devargs.index_vector(labels, N, meshes.num_classes, dev, "labels")
    H, W = int(H), int(W)
    if N == 0:
        empty = torch.empty(0, H, W, dtype=torch.float32, device=dev)
        return cou_from_depth(empty, empty, return_parts)
    both = render.render_depth(meshes, np.concatenate([lab_host, lab_host]), torch.cat([R_est, R_gt]), torch.cat([t_est, t_gt]), torch.cat([K, K]),
                               H, W, near, far)
    return cou_from_depth(both[:N], both[N:], return_parts)


def cou_bb(bb_est, bb_gt):
    """``pose_error.cou_bb`` of N box pairs: ``bb_est`` / ``bb_gt`` [N,4] x, y, w, h device tensors of any float / int dtype (widened to fp64).
    Returns [N] fp64 on the device: 1 - ``misc.iou``; a NaN in a box gives an IoU of 0."""
    a, b = devargs.device_tensor(bb_est, torch.float64, None, "bb_est", WHERE), devargs.device_tensor(bb_gt, torch.float64, None, "bb_gt", WHERE)
    if a.dim() != 2 or a.shape[1] != 4 or a.shape != b.shape:
        raise ValueError("bb_est and bb_gt are [N,4] (x, y, w, h)")
    N, dev = int(a.shape[0]), a.device
    err = torch.empty(max(N, 1), dtype=torch.float64, device=dev)[:N]
    p = cabi.ptr
    cabi.check(cabi.load().gdrn_cou_bb(p(a), p(b), N, p(err), devargs.stream(dev)), "cou_bb")
    return err


class CouRecall:
    """The score pass of one complement-over-union error on the device: ``update`` adds a batch of errors ([N] fp64, e.g. ``cus(...)[:, 0]``) to
    per-class counters without reading anything back -- a row is correct iff ``err < th``, the strict comparison of
    ``pose_matching.match_poses`` (a NaN is not correct) -- ``add_missing`` counts ground-truth targets that got no estimate, ``summarize``
    makes the one device-to-host copy."""

    def __init__(self, obj_names, th=CUS_TH):
        self.obj_names, self.th = list(obj_names), float(th)
        if not self.obj_names or not self.th == self.th:
            raise ValueError((obj_names, th))
        self.num_classes = len(self.obj_names)
        self._state = None   # int64 [2, C] on the device: correct, seen

    def _on(self, device):
        if self._state is None:
            self._state = torch.zeros(2, self.num_classes, dtype=torch.int64, device=device)
        elif self._state.device != torch.device(device):
            raise ValueError(f"the counters live on {self._state.device}")
        return self._state

    def update(self, err, labels):
        err = devargs.device_tensor(err, torch.float64, None, "err", "the complement-over-union recall")
        if err.dim() != 1:
            raise ValueError("err is [N]: one error per row (a column of cus / cou_mask / cou_from_depth, or cou_bb)")
        N, dev = int(err.shape[0]), err.device
        lab, _ = devargs.index_vector(labels, N, self.num_classes, dev, "labels")
        state, lab = self._on(dev), lab.long()
        state[0].index_add_(0, lab, (err < self.th).to(torch.int64))
        state[1].index_add_(0, lab, torch.ones_like(lab))

    def add_missing(self, label, count=1, device=None):
        if not 0 <= int(label) < self.num_classes or int(count) < 0:
            raise ValueError((label, count))
        if self._state is None and device is None:
            raise cabi.GdrnHipError("add_missing before the first update needs the device of the counters")
        self._on(device if self._state is None else self._state.device)[1, int(label)] += int(count)

    def counters(self):
        """host copies of the counters (the one device-to-host copy): correct [C], seen [C], int64"""
        host = np.zeros((2, self.num_classes), dtype=np.int64) if self._state is None else self._state.cpu().numpy()
        return dict(correct=host[0].copy(), seen=host[1].copy())

    def summarize(self):
        """recall = correct / targets per object with targets and over all of them ("all": counts summed over the classes), ``rows``: a
        tabulate-ready list"""
        c = self.counters()
        out = {"objects": {n: float(c["correct"][k]) / float(c["seen"][k]) for k, n in enumerate(self.obj_names) if c["seen"][k] > 0}}
        total = int(c["seen"].sum())
        out["all"] = float(c["correct"].sum()) / float(total) if total > 0 else float("nan")
        out["targets"], out["th"] = total, self.th
        rows = [["objects", f"recall(<{self.th:g})"]]
        rows += [[n, f"{100 * out['objects'][n]:.2f}"] for n in sorted(out["objects"])]
        rows.append([f"all({total})", f"{100 * out['all']:.2f}"])
        out["rows"] = rows
        return out

    def reset(self):
        if self._state is not None:
            self._state.zero_()
