#!/usr/bin/env python3
"""Generate golden G17 (``g17_scene_gt.npz``) by running the REFERENCE's visibility, distance and box functions on the maps of
``synth.make_scene_gt_inputs`` (rendered by tests/render_host.py: the reference's OpenGL renderer cannot run where this does).

Runs by hand, and only where the reference checkout is present (see make_golden.py); only its outputs are stored, arrays all of them.  Per case
("mixed", "pad0") and instance, as the BOP toolkit's mask and scene_gt_info passes combine them:
  dist_gt / dist_scene     ``misc.depth_im_to_dist_im_fast`` of the instance's image window and of its frame's depth image, with the image's K
  "mask"                   dist_gt > 0, ``np.packbits``
  "<mode>/mask_visib"      ``visibility.estimate_visib_mask_gt(dist_scene, dist_gt, delta, visib_mode=mode)`` for "bop19" and "bop18", packed
  "px_count_all"           the pixels > 0 of ``depth_im_to_dist_im_fast`` of the CANVAS (with cx + px, cy + py)
  "px_count_valid"         ``np.sum(dist_scene[dist_gt > 0] > 0)``
  "<mode>/px_count_visib"  the sum of the visibility mask
  "bbox_obj"               ``misc.calc_2d_bbox_xywh`` of the canvas pixels > 0, moved to image coordinates; [-1, -1, -1, -1] when there are none
  "<mode>/bbox_visib"      the same of the visibility mask
The seed moves on while a pixel centre of a canvas sits within 1e-6 px of a triangle edge or a visibility difference within 1e-5 m of delta (with
the depth images and composed from the instances): the seed that is stored is the one tests/test_scene_gt_cpu.py asserts those margins for.

With ``--workload`` nothing is written: the same functions are timed on this host on the workload of tools/scene_gt_time.py -- 64 instances in 8
frames of 480 x 640, canvases of 1440 x 1920 -- with analytic sphere depth maps in place of the renders (the functions' cost does not depend on
what the maps show).  Rendering is NOT part of that time.

Usage:  python tests/golden/make_golden_g17.py [--workload]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims  # noqa: E402

MODES = ("bop19", "bop18")
EDGE_MARGIN, DELTA_MARGIN = 1e-6, 1e-5


def xywh(misc, mask, W, H, ox=0, oy=0):
    ys, xs = mask.nonzero()
    if len(xs) == 0:
        return np.array([-1, -1, -1, -1], dtype=np.int64)
    return np.array(misc.calc_2d_bbox_xywh(xs - ox, ys - oy, W, H), dtype=np.int64)


def reference_pass(misc, visibility, canvas, Kc, depth, depth_scene, K, delta, pad, modes=MODES):
    """what the toolkit computes for one instance, from the reference's own functions"""
    px, py = pad
    H, W = depth.shape
    dist_canvas = misc.depth_im_to_dist_im_fast(canvas, Kc)
    dist_gt = misc.depth_im_to_dist_im_fast(depth, K)
    dist_scene = misc.depth_im_to_dist_im_fast(depth_scene, K)
    obj = dist_canvas > 0
    out = dict(mask=dist_gt > 0, px_count_all=int(np.sum(obj)), px_count_valid=int(np.sum(dist_scene[dist_gt > 0] > 0)),
               bbox_obj=xywh(misc, obj, W, H, px, py))
    for mode in modes:
        vis = visibility.estimate_visib_mask_gt(dist_scene, dist_gt, delta, visib_mode=mode)
        out[mode] = dict(mask_visib=vis, px_count_visib=int(vis.sum()), bbox_visib=xywh(misc, vis, W, H))
    return out


def sphere_depth(H, W, K, centre, radius):
    """depth of a sphere by ray-sphere intersection, fp32 [H,W], 0 = miss"""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1)
    a, b, c = (d * d).sum(-1), d @ centre, centre @ centre - radius * radius
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        s = (b - np.sqrt(disc)) / a
    return np.where(disc > 0, s, 0.0).astype(np.float32)


def time_workload(misc, visibility, synth):
    N, F, H, W, seed = 64, 8, 480, 640, 7
    K = synth.LM_K.astype(np.float64)
    Kc = K.copy()
    Kc[0, 2] += W
    Kc[1, 2] += H
    u = synth.hash_uniform(seed, "t", (N, 3))
    centres = np.concatenate([0.3 * u[:, :2] - 0.15, 0.6 + 0.8 * u[:, 2:]], axis=1)
    t_pass = 0.0
    scene = np.full((F, H, W), 2.0, dtype=np.float32)
    canv = []
    for i in range(N):
        canv.append(sphere_depth(3 * H, 3 * W, Kc, centres[i], 0.1))
        win = canv[-1][H : 2 * H, W : 2 * W]
        f = i // (N // F)
        scene[f] = np.where((win > 0) & (win < scene[f]), win, scene[f])
    for i in range(N):
        win = np.ascontiguousarray(canv[i][H : 2 * H, W : 2 * W])
        t0 = time.perf_counter()
        reference_pass(misc, visibility, canv[i], Kc, win, scene[i // (N // F)], K, 0.015, (W, H), modes=("bop19",))
        t_pass += time.perf_counter() - t0
    print(f"workload: {N} instances in {F} frames of {H} x {W}, canvases of {3 * H} x {3 * W}: the reference's depth_im_to_dist_im_fast (canvas, "
          f"instance, scene), estimate_visib_mask_gt (bop19), the counts and calc_2d_bbox_xywh (twice) {t_pass:.2f} s on this host, "
          f"{1e3 * t_pass / N:.1f} ms per instance; the renders are not included")


def main():
    install_shims()
    from lib.pysixd import misc, visibility

    import scene_gt_host as SH
    from gdrnet_amd import synth

    if "--workload" in sys.argv:
        time_workload(misc, visibility, synth)
        return
    seed = synth.SCENE_GT_SEED
    while True:
        SH._scenes.clear()
        SH._results.clear()
        synth.SCENE_GT_SEED = seed
        edge = min(SH.scene(case)[3] for case in synth.SCENE_GT_CASES)
        delta = min(SH.result(case, "bop19", comp)[1] for case in synth.SCENE_GT_CASES for comp in (False, True))
        print(f"seed {seed}: edge band {edge:.3e} px, delta band {delta:.3e} m", flush=True)
        if edge >= EDGE_MARGIN and delta > DELTA_MARGIN:
            break
        seed += 1
    g = {"seed": np.array(seed)}
    for case in synth.SCENE_GT_CASES:
        inp, canv, scene_d, _ = SH.scene(case)
        px, py = inp["pad"]
        H, W = inp["H"], inp["W"]
        rows = []
        for i in range(len(inp["labels"])):
            K = inp["K"][i]
            rows.append(reference_pass(misc, visibility, canv[i], SH.canvas_K(K, px, py), SH.window(canv[i], H, W, px, py),
                                       scene_d[inp["frame"][i]], K, inp["delta"], (px, py)))
        g[f"{case}/mask"] = np.packbits(np.stack([r["mask"] for r in rows]))
        for k in ("px_count_all", "px_count_valid"):
            g[f"{case}/{k}"] = np.array([r[k] for r in rows], dtype=np.int64)
        g[f"{case}/bbox_obj"] = np.stack([r["bbox_obj"] for r in rows])
        for mode in MODES:
            g[f"{case}/{mode}/mask_visib"] = np.packbits(np.stack([r[mode]["mask_visib"] for r in rows]))
            g[f"{case}/{mode}/px_count_visib"] = np.array([r[mode]["px_count_visib"] for r in rows], dtype=np.int64)
            g[f"{case}/{mode}/bbox_visib"] = np.stack([r[mode]["bbox_visib"] for r in rows])
        print(f"{case}: px_count_all {g[f'{case}/px_count_all'].tolist()}, px_count_visib (bop19) {g[f'{case}/bop19/px_count_visib'].tolist()}")
    out = os.path.join(HERE, "g17_scene_gt.npz")
    np.savez_compressed(out, **g)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
