"""Naive numpy restatement of the rules of gdrnet_amd.scene_gt (include/gdrn_hip.h, "Scene ground truth on the device"): the project's own host
oracle, pinned to the reference's visibility, distance and box functions by golden G17 (tests/test_scene_gt_cpu.py).  The canvases come from the
brute-force host rasterizer (render_host.render_one), the distances from bop_host.dist_image; no reference import."""
import numpy as np

import bop_host as BH
import render_host as RH
from gdrnet_amd import synth

EMPTY = (0, 0, -1, -1)
_scenes = {}


def canvas_K(K, px, py):
    Kc = np.array(K, dtype=np.float64, copy=True)
    Kc[..., 0, 2] += px
    Kc[..., 1, 2] += py
    return Kc


def scene(case):
    """(inputs, canvases [N,Hc,Wc] fp32, depth_scene [F,H,W] fp32, the rasterizer's edge_band over the canvases) of a synth.make_scene_gt_inputs
    case, computed once per process."""
    if case not in _scenes:
        inp = synth.make_scene_gt_inputs(case)
        H, W = inp["H"], inp["W"]
        px, py = inp["pad"]
        canv, band = [], np.inf
        for i, c in enumerate(inp["labels"]):
            s = {}
            canv.append(RH.render_one(inp["vertices"][c], inp["faces"][c], inp["R"][i], inp["t"][i], canvas_K(inp["K"][i], px, py), H + 2 * py,
                                      W + 2 * px, inp["near"], inp["far"], s))
            band = min(band, s["edge_band"])
        canv = np.stack(canv)
        _scenes[case] = (inp, canv, synth.scene_gt_depth(inp, window(canv, H, W, px, py)), band)
    return _scenes[case]


def window(canvas, H, W, px, py):
    return np.ascontiguousarray(canvas[..., py : py + H, px : px + W])


def compose(depth, frame, F):
    """per frame and pixel the smallest non-zero depth over the frame's instances, 0 where there is none"""
    N, H, W = depth.shape
    out = np.zeros((F, H, W), dtype=np.float32)
    for i in range(N):
        d, o = depth[i], out[int(frame[i])]
        take = (d != 0) & ((o == 0) | (d < o))
        o[take] = d[take]
    return out


def bounds(mask, ox=0, oy=0):
    ys, xs = np.nonzero(mask)
    return EMPTY if len(xs) == 0 else (int(xs.min()) - ox, int(ys.min()) - oy, int(xs.max()) - ox, int(ys.max()) - oy)


def visible(dist_gt, dist_scene, delta, mode):
    diff = dist_gt.astype(np.float32) - dist_scene.astype(np.float32)
    near = diff <= np.float32(delta)
    if mode == "bop19":
        return ((near | (dist_scene == 0)) & (dist_gt > 0)), diff
    if mode == "bop18":
        return (near & (dist_scene > 0) & (dist_gt > 0)), diff
    raise ValueError(mode)


def scene_gt(canvas, K, frame, F, depth_scene, delta, mode, pad, stats=None):
    """dict of numpy arrays with the fields of gdrnet_amd.scene_gt.SceneGt for canvases [N,Hc,Wc] fp32; depth_scene None: composed.  `stats` receives
    delta_band, the smallest | (f32(dist_gt) - f32(dist_scene)) - delta | over the mask pixels whose scene depth is not 0."""
    px, py = pad
    N, Hc, Wc = canvas.shape
    H, W = Hc - 2 * py, Wc - 2 * px
    depth = window(canvas, H, W, px, py)
    scene_d = compose(depth, frame, F) if depth_scene is None else np.asarray(depth_scene, dtype=np.float32)
    out = dict(depth=depth, depth_scene=scene_d, mask=(depth != 0).astype(np.uint8), mask_visib=np.zeros((N, H, W), np.uint8),
               px_count_all=np.zeros(N, np.int32), px_count_valid=np.zeros(N, np.int32), px_count_visib=np.zeros(N, np.int32),
               bbox_obj=np.zeros((N, 4), np.int32), bbox_visib=np.zeros((N, 4), np.int32), visib_fract=np.zeros(N, np.float64))
    band = np.inf
    for i in range(N):
        Ki = K[i] if np.ndim(K) == 3 else K
        sd = scene_d[int(frame[i])]
        vis, diff = visible(BH.dist_image(depth[i], Ki), BH.dist_image(sd, Ki), delta, mode)
        decided = (depth[i] != 0) & (sd != 0)
        if decided.any():
            band = min(band, float(np.abs(diff[decided].astype(np.float64) - delta).min()))
        out["mask_visib"][i] = vis
        out["px_count_all"][i] = int((canvas[i] != 0).sum())
        out["px_count_valid"][i] = int(((depth[i] != 0) & (sd > 0)).sum())
        out["px_count_visib"][i] = int(vis.sum())
        out["bbox_obj"][i] = bounds(canvas[i] != 0, px, py)
        out["bbox_visib"][i] = bounds(vis)
        out["visib_fract"][i] = np.float64(out["px_count_visib"][i]) / np.float64(out["px_count_all"][i]) if out["px_count_all"][i] > 0 else 0.0
    if stats is not None:
        stats["delta_band"] = band
    return out


def xywh(box):
    x1, y1, x2, y2 = (int(v) for v in box)
    return [-1, -1, -1, -1] if x2 < x1 else [x1, y1, x2 - x1 + 1, y2 - y1 + 1]


_results = {}


def result(case, mode, composed):
    """scene_gt of a fixture case on the host canvases, computed once per process; (fields, delta_band)"""
    key = (case, mode, composed)
    if key not in _results:
        inp, canv, scene_d, _ = scene(case)
        s = {}
        _results[key] = (scene_gt(canv, inp["K"], inp["frame"], inp["num_frames"], None if composed else scene_d, inp["delta"], mode, inp["pad"], s),
                         s["delta_band"])
    return _results[key]
