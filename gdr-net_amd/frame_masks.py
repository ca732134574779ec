"""Predicted instance masks in the frame (csrc/roi_paste.hip): the link between ``postproc`` and ``refine`` / ``verify`` / ``masks.encode``.

``postproc.get_out_mask`` ends at a [N, 1, res, res] probability map in crop coordinates; ``refine.icp_refine_sil`` / ``refine_rgbd``,
``verify.verify_maps`` / ``verify_poses`` / ``best_of``, ``cou_metrics.cou_mask`` and ``masks.encode`` want [M, H, W] uint8 in frame coordinates
on the device.  ``largest_component`` keeps the largest 8-connected blob of each thresholded map, ``paste_masks`` samples the maps back into the
frames -- bilinearly, with a zero border, at the exact inverse of the ideal crop map of ``get_affine_transform(center, scale, 0, res)``, the
geometry ``RoiCropper`` cropped with -- and ``masks_from_maps`` chains the two behind ``get_out_mask``.  With ``exclusive`` every frame pixel
goes to at most one RoI of its frame: the one with the greatest sampled value, the lowest row among equals.  The arithmetic is stated with the
entry points in ``include/gdrn_hip.h``: a fixed fp64 operation sequence and integer atomics, so the same call gives the same bits.  The
reference has no counterpart on the path.  Nothing of the maps or masks is read back; there is no CPU fallback.

``thr`` (0.5) and ``keep_largest`` are parameters: neither is measured on real data.
"""
import numpy as np
import torch

from . import cabi, devargs, postproc

WHERE = "the mask paste"   # (this module in devargs' error sentence)
MIN_RES, MAX_RES = 2, 64


def _thr(thr):
    thr = float(thr)
    if not 0.0 <= thr < float("inf"):
        raise ValueError(f"thr {thr} must be finite and >= 0")
    return thr


def _map_shape(maps, what):
    """(B, res) of ``maps`` [B, res, res] or [B, 1, res, res]: what can be said about it before the device is looked at"""
    if not isinstance(maps, torch.Tensor):
        raise cabi.GdrnHipError(f"{WHERE} runs on the GPU (no CPU fallback): {what} is not a device tensor")
    shape = tuple(maps.shape)
    if len(shape) == 4 and shape[1] == 1:
        shape = (shape[0], shape[2], shape[3])
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError(f"{what} {tuple(maps.shape)} must be [B, res, res] or [B, 1, res, res]")
    B, res = int(shape[0]), int(shape[1])
    if not MIN_RES <= res <= MAX_RES:
        raise ValueError(f"{what}: res {res} outside [{MIN_RES}, {MAX_RES}]")
    return B, res


def _f64(values, shape, what):
    """host fp64 array of ``shape`` from a sequence, a numpy array or a tensor, the values as given (fp32 widens exactly); a device tensor is
    copied back once, as ``devargs.index_vector`` does for the check of an index vector"""
    host = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
    host = np.ascontiguousarray(host, dtype=np.float64)
    if host.size != int(np.prod(shape)):
        raise ValueError(f"{what}: {host.size} values for {shape}")
    return host.reshape(shape)


def _geometry(bbox_center, scale, B):
    """geom [B, 3] fp64 on the host = cx, cy, scale, checked"""
    c, s = _f64(bbox_center, (B, 2), "bbox_center"), _f64(scale, (B,), "scale")
    if not np.isfinite(c).all():
        raise ValueError("bbox_center must be finite")
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("scale must be finite and > 0")
    return np.ascontiguousarray(np.concatenate([c, s[:, None]], axis=1))


def _frame_size(n, im_H, im_W, what):
    H, W = int(im_H), int(im_W)
    if H < 1 or W < 1:
        raise ValueError(f"frame size {H} x {W}: both sides >= 1")
    if n * H * W >= 2 ** 31:
        raise ValueError(f"{what} * H * W = {n} * {H} * {W} must stay below 2**31")
    return H, W


def _csr(frame_host, F):
    """[F + 1 + B] int32: the offsets of the frames, then the rows of each frame in ascending order"""
    order = np.argsort(frame_host, kind="stable").astype(np.int32)
    offsets = np.zeros(F + 1, dtype=np.int32)
    np.cumsum(np.bincount(frame_host, minlength=F), out=offsets[1:])
    return np.ascontiguousarray(np.concatenate([offsets, order]))


def largest_component(prob, thr=0.5):
    """The largest 8-connected blob of each map: ``prob`` [B, res, res] or [B, 1, res, res] fp32 on the device, 2 <= res <= 64; foreground is
    ``prob > thr``, a non-finite value counting as 0; among components of equal size the one holding the lowest row-major pixel index.  Returns
    a dict of device tensors: filtered (``prob``'s shape, fp32: ``prob`` on the kept component, 0 elsewhere), num_comp [B] and kept_px [B]
    (int32).  One launch, one workgroup per map."""
    thr = _thr(thr)
    B, res = _map_shape(prob, "prob")
    if B * res * res >= 2 ** 31:
        raise ValueError("B * res * res must stay below 2**31")
    p = devargs.device_tensor(prob, torch.float32, None, "prob", WHERE)
    dev = p.device
    out = dict(filtered=torch.empty_like(p), num_comp=torch.empty(B, dtype=torch.int32, device=dev),
               kept_px=torch.empty(B, dtype=torch.int32, device=dev))
    if B > 0:
        cabi.check(cabi.load().gdrn_roi_components(cabi.ptr(p), B, res, thr, cabi.ptr(out["filtered"]), cabi.ptr(out["num_comp"]),
                                                   cabi.ptr(out["kept_px"]), devargs.stream(dev)), "roi_components")
    return out


def paste_masks(maps, bbox_center, scale, im_H, im_W, thr=0.5, frame=None, num_frames=None, exclusive=False):
    """Paste B maps into frame-size masks: ``maps`` [B, res, res] or [B, 1, res, res] fp32 on the device; ``bbox_center`` [B, 2] and ``scale``
    [B] the crop geometry (host sequences, numpy arrays or tensors -- ``RoiCropper``'s batch dict carries them as fp32 device tensors -- taken
    as fp64 from the values as given; a device tensor is copied back once for the check); ``im_H``, ``im_W`` the frame size.  A frame pixel is
    set iff the map, sampled bilinearly with a zero border at the pixel's crop position, exceeds ``thr``.  With ``exclusive`` (needs ``frame``
    [B], the frame of each row, and ``num_frames``, default ``max(frame) + 1``) a pixel claimed by several rows of one frame goes to the greatest
    sampled value, the lowest row among equals.  Returns a dict of device tensors: mask [B, H, W] uint8 (0 / 1), area [B] and bbox [B, 4] int32
    (``masks.stats``' convention), and with ``exclusive`` index [F, H, W] int32, the winning row or -1.  ``mask`` goes unchanged into
    ``icp_refine_sil``, ``refine_rgbd``, ``verify_maps`` / ``verify_poses`` / ``best_of``, ``cou_metrics.cou_mask`` and ``masks.encode``."""
    thr = _thr(thr)
    B, res = _map_shape(maps, "maps")
    H, W = _frame_size(B, im_H, im_W, "B")
    geom_host = _geometry(bbox_center, scale, B)
    F = frame_host = None
    if exclusive:
        if frame is None:
            raise ValueError("exclusive=True needs frame, the frame of each row")
        frame_host = devargs._host_indices(frame, B, None, "frame", False)
        if frame_host.size and frame_host.min() < 0:
            raise ValueError("frame outside [0, num_frames)")
        F = int(num_frames) if num_frames is not None else (int(frame_host.max()) + 1 if B else 0)
        if F < 0 or (frame_host.size and frame_host.max() >= F):
            raise ValueError(f"frame outside [0, {F})")
        _frame_size(F, H, W, "num_frames")
    m = devargs.device_tensor(maps, torch.float32, (B, res, res), "maps", WHERE)
    dev = m.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(mask=torch.empty(B, H, W, dtype=torch.uint8, device=dev), area=torch.empty(B, **i32), bbox=torch.empty(B, 4, **i32))
    if exclusive:
        out["index"] = torch.empty(F, H, W, **i32) if B > 0 else torch.full((F, H, W), -1, **i32)
    if B == 0:
        return out
    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(dev)
    geom = torch.from_numpy(geom_host).to(dev)
    if not exclusive:
        cabi.check(lib.gdrn_roi_paste_masks(p(m), p(geom), geom_host.ctypes.data, B, res, H, W, thr, p(out["mask"]), p(out["area"]),
                                            p(out["bbox"]), st), "roi_paste_masks")
        return out
    csr_host = _csr(frame_host, F)
    csr = torch.from_numpy(csr_host).to(dev)
    cabi.check(lib.gdrn_roi_paste_exclusive(p(m), p(geom), geom_host.ctypes.data, frame_host.ctypes.data, p(csr), csr_host.ctypes.data, B, F, res,
                                            H, W, thr, p(out["index"]), p(out["mask"]), p(out["area"]), p(out["bbox"]), st), "roi_paste_exclusive")
    return out


def masks_from_maps(cfg, out_dict, bbox_center, scale, im_H, im_W, frame=None, num_frames=None, mask_thr=None, keep_largest=True,
                    exclusive=False):
    """The network's mask output as frame masks, the sibling of ``pnp.poses_from_maps`` / ``rigid.poses_from_maps_rgbd``: ``out_dict`` the
    model's eval output (``mask`` [B, 1, res, res]); ``postproc.get_out_mask``, then ``largest_component`` (with ``keep_largest``), then
    ``paste_masks`` on the current stream without a host read of a map.  ``mask_thr`` defaults to ``cfg.MODEL.CDPN.ROT_HEAD.MASK_THR_TEST`` and
    is both the foreground threshold of the blobs and the threshold of the paste.  Returns ``paste_masks``' dict, plus num_comp and kept_px with
    ``keep_largest``."""
    thr = _thr(cfg.MODEL.CDPN.ROT_HEAD.MASK_THR_TEST if mask_thr is None else mask_thr)
    _map_shape(out_dict["mask"], "out_dict['mask']")
    prob = postproc.get_out_mask(cfg, out_dict["mask"])
    extra = {}
    if keep_largest:
        cc = largest_component(prob, thr)
        prob, extra = cc["filtered"], dict(num_comp=cc["num_comp"], kept_px=cc["kept_px"])
    out = paste_masks(prob, bbox_center, scale, im_H, im_W, thr, frame, num_frames, exclusive)
    out.update(extra)
    return out
