"""Scene ground truth on the device: masks, visibility and boxes of every annotated instance from poses (csrc/scene_gt.hip).

Device-side replacement of the BOP toolkit's offline pass whose files every dataset file under core/gdrn_modeling/datasets/ reads from a BOP
folder (lm_pbr.py:143-178): ``mask/*.png``, ``mask_visib/*.png`` and the records of ``scene_gt_info.json`` -- ``bbox_obj``, ``bbox_visib``,
``px_count_all``, ``px_count_valid``, ``px_count_visib``, ``visib_fract``.  The toolkit renders one instance at a time on the host, on a canvas
three times the image, and runs numpy passes over it; here ``render.render_depth`` draws a chunk of instances on the canvas and three pixel
passes do the rest for the whole batch.  ``mask_visib`` becomes the ``segmentation`` of the dataset dicts, ``bbox_visib`` their ``bbox``,
``visib_fract`` is what the loaders' visibility filter thresholds.

Two modes.  With ``depth_scene`` (the frames' depth images in metres) visibility is the toolkit's: the object's surface is compared with the
measured scene, ``visibility._estimate_visib_mask`` (lib/pysixd/visibility.py:29-36) on ``misc.depth_im_to_dist_im_fast`` distances.  Without one
(RGB-only captures, composited synthetic frames) the scene depth is COMPOSED from the frame's own annotated instances -- per pixel the nearest
of them -- so visibility is their mutual occlusion: an instance's own surface is within ``delta`` of itself, another instance less than
``delta`` in front does not hide it, and ``px_count_valid`` equals the mask's pixel count.

What differs from the toolkit: the renderer is this package's rasterizer (integer-pixel rays, inclusive edges, include/gdrn_hip.h), not
OpenGL, so silhouettes can differ from the toolkit's files by boundary pixels; ``bbox_obj`` is the bound of the CANVAS silhouette whenever
``px_count_all > 0`` (a choice of this project: the box of an object that reaches beyond the image is then not clipped, and with ``pad=(0, 0)``
it is the in-image box); an empty box is (0, 0, -1, -1) on the device and [-1, -1, -1, -1] in ``to_scene_gt_info``.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import cabi, devargs, render

VISIB_MODES = {"bop19": 0, "bop18": 1}   # GDRN_VISIB_BOP19, GDRN_VISIB_BOP18
DELTA = 0.015                            # BOP's 15 mm
WHERE = "the scene ground truth"         # (this module in devargs' error sentence)
INFO_KEYS = ("bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract")


def xywh(box):
    """``misc.calc_2d_bbox_xywh`` (lib/pysixd/misc.py:644-654) of inclusive bounds (x1, y1, x2, y2): [x1, y1, x2 - x1 + 1, y2 - y1 + 1]; the empty
    box (0, 0, -1, -1) is written [-1, -1, -1, -1]"""
    x1, y1, x2, y2 = (int(v) for v in box)
    return [-1, -1, -1, -1] if x2 < x1 or y2 < y1 else [x1, y1, x2 - x1 + 1, y2 - y1 + 1]


class SceneGt:
    """The result of ``scene_gt`` / ``scene_gt_from_depth`` for N instances in F frames, device tensors all of them:
    ``mask``, ``mask_visib`` [N,H,W] u8; ``px_count_all``, ``px_count_valid``, ``px_count_visib`` [N] int32; ``bbox_obj``, ``bbox_visib`` [N,4]
    int32, inclusive xyxy in image coordinates (``bbox_obj`` may lie outside the image; empty: (0, 0, -1, -1)); ``visib_fract`` [N] fp64;
    ``depth`` [N,H,W] fp32, the image window of the render (``render.xyz_from_depth`` can follow without a second render); ``depth_scene``
    [F,H,W] fp32, the caller's or the composed one.  ``frame`` [N] and ``num_frames`` are kept on the host."""

    def __init__(self, mask, mask_visib, px_count_all, px_count_valid, px_count_visib, bbox_obj, bbox_visib, visib_fract, depth, depth_scene,
                 frame, num_frames):
        self.mask, self.mask_visib, self.depth, self.depth_scene = mask, mask_visib, depth, depth_scene
        self.px_count_all, self.px_count_valid, self.px_count_visib = px_count_all, px_count_valid, px_count_visib
        self.bbox_obj, self.bbox_visib, self.visib_fract = bbox_obj, bbox_visib, visib_fract
        self.frame = np.asarray(frame, dtype=np.int32).reshape(-1)
        self.num_frames = int(num_frames)

    def __len__(self):
        return int(self.frame.shape[0])

    def to_scene_gt_info(self, frame_ids=None):
        """``{frame_id: [one dict per instance of the frame, in input order]}`` with the keys of ``scene_gt_info.json``, as Python ints and
        floats; boxes as ``misc.calc_2d_bbox_xywh`` writes them, an empty one as [-1, -1, -1, -1].  ``frame_ids`` [F]: the key of each frame
        (default: its index); a frame without instances gets an empty list.  Makes ONE device-to-host copy, of the [N] and [N,4] tensors."""
        N, F = len(self), self.num_frames
        ids = list(range(F)) if frame_ids is None else list(frame_ids)
        if len(ids) != F or len(set(ids)) != F:
            raise ValueError(f"frame_ids: {F} distinct keys, one per frame")
        packed = torch.cat([self.px_count_all.reshape(N, 1), self.px_count_valid.reshape(N, 1), self.px_count_visib.reshape(N, 1),
                            self.bbox_obj.reshape(N, 4), self.bbox_visib.reshape(N, 4),
                            self.visib_fract.reshape(N, 1).contiguous().view(torch.int32)], dim=1)
        host = np.ascontiguousarray(packed.cpu().numpy())   # the one copy
        fract = np.ascontiguousarray(host[:, 11:13]).view(np.float64).reshape(N)
        out = {k: [] for k in ids}
        for i in range(N):
            r = host[i]
            out[ids[int(self.frame[i])]].append(dict(bbox_obj=xywh(r[3:7]), bbox_visib=xywh(r[7:11]), px_count_all=int(r[0]),
                                                     px_count_valid=int(r[1]), px_count_visib=int(r[2]), visib_fract=float(fract[i])))
        return out

    def segmentations(self):
        """the ``segmentation`` entries of the dataset dicts: ``mask_visib`` as compressed COCO RLE, ``[{"size": [H, W], "counts": str}, ...]``"""
        from . import masks

        return masks.encode(self.mask_visib).to_coco()


def _pad(pad, H, W):
    if pad is None:
        return int(W), int(H)
    try:
        px, py = (int(v) for v in pad)
    except (TypeError, ValueError):
        raise ValueError("pad: (px, py), the canvas margin in pixels") from None
    if px < 0 or py < 0:
        raise ValueError("pad: a margin cannot be negative")
    return px, py


def _common(delta, visib_mode):
    if visib_mode not in VISIB_MODES:
        raise ValueError(f"visib_mode {visib_mode!r}: bop19 or bop18")
    delta = float(delta)
    if not delta >= 0.0:
        raise ValueError("delta: a non-negative distance in metres")
    return delta, VISIB_MODES[visib_mode]


def _frames(frame, N, depth_scene, H, W, device):
    """(frame on the device, its host copy, F, depth_scene or None): everything about the frames checked on the host"""
    if depth_scene is not None:
        depth_scene = devargs.device_tensor(depth_scene, torch.float32, None, "depth_scene", WHERE)
        if depth_scene.dim() != 3 or tuple(depth_scene.shape[1:]) != (H, W) or depth_scene.shape[0] < 1:
            raise ValueError(f"depth_scene must be [F, {H}, {W}]")
        F = int(depth_scene.shape[0])
        fr, fr_host = devargs.index_vector(frame, N, F, device, "frame")
    else:
        fr, fr_host = devargs.index_vector(frame, N, None, device, "frame")
        if fr_host.size and fr_host.min() < 0:
            raise ValueError("frame outside [0, F)")
        F = int(fr_host.max()) + 1 if fr_host.size else 0
    return fr, fr_host, F, depth_scene


def csr_of_frames(frame_host, F):
    """(inst_off [F + 1], inst [N]) int32: the instances of frame f are inst[inst_off[f] : inst_off[f + 1]], in input order"""
    frame_host = np.asarray(frame_host, dtype=np.int64).reshape(-1)
    off = np.zeros(F + 1, dtype=np.int32)
    np.cumsum(np.bincount(frame_host, minlength=F), out=off[1:])
    return off, np.argsort(frame_host, kind="stable").astype(np.int32)


class _Out:
    """the output tensors of one call"""

    def __init__(self, N, H, W, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.depth = torch.empty(N, H, W, dtype=torch.float32, device=device)
        self.mask, self.mask_visib = (torch.empty(N, H, W, dtype=torch.uint8, device=device) for _ in range(2))
        self.px_count_all, self.px_count_valid, self.px_count_visib = (torch.empty(N, **i32) for _ in range(3))
        self.bbox_obj, self.bbox_visib = (torch.empty(N, 4, **i32) for _ in range(2))
        self.visib_fract = torch.empty(N, dtype=torch.float64, device=device)

    def canvas_pass(self, lib, canvas, i0, H, W, px, py, device):
        """rows i0 .. i0 + len(canvas) of depth, px_count_all and the running bbox_obj from their canvases"""
        n, p = int(canvas.shape[0]), cabi.ptr
        cabi.check(lib.gdrn_scene_gt_canvas(p(canvas), n, H, W, px, py, p(self.depth[i0:]), p(self.px_count_all[i0:]), p(self.bbox_obj[i0:]),
                                            devargs.stream(device)), "scene_gt_canvas")

    def finish(self, lib, fr, fr_host, F, depth_scene, K, N, H, W, delta, mode, device):
        p = cabi.ptr
        if depth_scene is None:
            off_host, inst_host = csr_of_frames(fr_host, F)
            table = torch.from_numpy(np.concatenate([off_host, inst_host])).to(device)   # one upload
            depth_scene = torch.empty(F, H, W, dtype=torch.float32, device=device)
            cabi.check(lib.gdrn_scene_gt_compose(p(self.depth), p(table), off_host.ctypes.data, p(table[F + 1:]), inst_host.ctypes.data, F, N, H, W,
                                                 p(depth_scene), devargs.stream(device)), "scene_gt_compose")
        cabi.check(lib.gdrn_scene_gt_visibility(p(self.depth), p(depth_scene), p(fr), fr_host.ctypes.data, F, p(K), N, H, W, delta, mode,
                                                p(self.mask), p(self.mask_visib), p(self.px_count_all), p(self.px_count_valid),
                                                p(self.px_count_visib), p(self.bbox_obj), p(self.bbox_visib), p(self.visib_fract),
                                                devargs.stream(device)), "scene_gt_visibility")
        return SceneGt(self.mask, self.mask_visib, self.px_count_all, self.px_count_valid, self.px_count_visib, self.bbox_obj, self.bbox_visib,
                       self.visib_fract, self.depth, depth_scene, fr_host, F)


def _empty(H, W, F, depth_scene, device):
    o = _Out(0, H, W, device)
    scene = depth_scene if depth_scene is not None else torch.zeros(F, H, W, dtype=torch.float32, device=device)
    return SceneGt(o.mask, o.mask_visib, o.px_count_all, o.px_count_valid, o.px_count_visib, o.bbox_obj, o.bbox_visib, o.visib_fract, o.depth,
                   scene, np.zeros(0, np.int32), F)


def scene_gt(meshes, labels, R, t, K, H, W, frame, depth_scene=None, delta=DELTA, visib_mode="bop19", pad=None, near=render.NEAR,
             far=render.FAR, chunk=64):
    """The annotations of N instances in F frames of H x W from their poses: instance i is the mesh ``labels[i]`` of the ``render.MeshTable``
    ``meshes`` under ``R[i]``, ``t[i]`` seen through ``K[i]`` ([3,3]: shared) in frame ``frame[i]`` -- arguments as ``render.render_depth``
    takes them; ``frame`` [N] from the host or the device, range-checked on the host before anything is launched.

    ``depth_scene`` [F,H,W] fp32 device tensor in metres, 0 = no measurement; ``None``: composed from the instances (then F = max(frame) + 1).
    ``delta``: the visibility tolerance in metres.  ``visib_mode`` "bop19" (visible where the scene has no measurement) or "bop18" (not visible
    there).  ``pad`` = (px, py): the canvas margin, default (W, H) -- the toolkit's canvas of three times the image; the instance is rendered at
    (H + 2 py, W + 2 px) with cx + px, cy + py, ``px_count_all`` and ``bbox_obj`` are taken on that canvas and everything else on its central
    window.  (0, 0) gives in-image statistics only.  ``chunk``: how many instances' canvases are alive at once (64 of 480 x 640 at the default
    margin are 708 MB); the results do not depend on it.  Returns a ``SceneGt``; nothing is read back."""
    delta, mode = _common(delta, visib_mode)
    H, W, chunk = int(H), int(W), int(chunk)
    if H < 1 or W < 1:
        raise ValueError("H and W: at least one pixel")
    if chunk < 1:
        raise ValueError("chunk: at least one instance at a time")
    px, py = _pad(pad, H, W)
    R, t, K, N = devargs.poses(R, t, K, WHERE)
    dev = R.device
    lab_host = devargs.index_vector(labels, N, meshes.num_classes, dev, "labels")[1]
    fr, fr_host, F, depth_scene = _frames(frame, N, depth_scene, H, W, dev)
    if N == 0:
        return _empty(H, W, F, depth_scene, dev)
    lib = cabi.load()
    Kc = K.clone()
    Kc[:, 0, 2] += px
    Kc[:, 1, 2] += py
    out = _Out(N, H, W, dev)
    for i0 in range(0, N, chunk):
        i1 = min(i0 + chunk, N)
        canvas = render.render_depth(meshes, lab_host[i0:i1], R[i0:i1], t[i0:i1], Kc[i0:i1], H + 2 * py, W + 2 * px, near, far)
        out.canvas_pass(lib, canvas, i0, H, W, px, py, dev)
    return out.finish(lib, fr, fr_host, F, depth_scene, K, N, H, W, delta, mode, dev)


def scene_gt_from_depth(depth_canvas, K, frame, depth_scene=None, delta=DELTA, visib_mode="bop19", pad=None):
    """``scene_gt`` on canvases that are already rendered: ``depth_canvas`` [N, H + 2 py, W + 2 px] fp32 device tensor (0 = nothing), ``K`` [N,3,3]
    or [3,3] of the IMAGE (the canvas was rendered with cx + px, cy + py), ``pad`` = (px, py) -- default: a canvas of three times the image,
    (W, H).  The other arguments and the result as ``scene_gt``."""
    delta, mode = _common(delta, visib_mode)
    margin = None if pad is None else _pad(pad, 0, 0)
    canvas = devargs.device_tensor(depth_canvas, torch.float32, None, "depth_canvas", WHERE)
    if canvas.dim() != 3:
        raise ValueError("depth_canvas must be [N, H + 2 py, W + 2 px]")
    N, Hc, Wc = (int(s) for s in canvas.shape)
    if margin is None and (Hc % 3 or Wc % 3):
        raise ValueError("a canvas of three times the image has sides that are multiples of 3: pass pad=(px, py)")
    px, py = (Wc // 3, Hc // 3) if margin is None else margin
    H, W = Hc - 2 * py, Wc - 2 * px
    if H < 1 or W < 1:
        raise ValueError(f"a canvas of {Hc} x {Wc} leaves no image inside a margin of ({px}, {py})")
    dev = canvas.device
    K = devargs.device_tensor(K, torch.float64, (-1, 3, 3), "K", WHERE)
    fr, fr_host, F, depth_scene = _frames(frame, N, depth_scene, H, W, dev)
    if N == 0:
        return _empty(H, W, F, depth_scene, dev)
    K = devargs.per_row_K(K, N)
    lib = cabi.load()
    out = _Out(N, H, W, dev)
    out.canvas_pass(lib, canvas, 0, H, W, px, py, dev)
    return out.finish(lib, fr, fr_host, F, depth_scene, K, N, H, W, delta, mode, dev)
