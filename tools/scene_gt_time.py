#!/usr/bin/env python3
"""Time gdrnet_amd.scene_gt with HIP events: median of 20 calls after 5 warm-ups.  The workload is 64 instances in 8 frames of 480 x 640, the
20 480-face perturbed icosphere, default margin (canvases of 1440 x 1920, 708 MB for the 64).  Reported:
  scene_gt with depth images             the 64 canvas renders, the canvas pass, the visibility pass
  scene_gt composed                      the same plus the compose pass, no depth images
  scene_gt_from_depth                    the new passes alone on canvases that are already rendered, with the bytes the algorithm needs (every
                                         canvas value read once, the window written and read once, the frames' depth images read once, two masks
                                         written) over the time, and that rate's share of the HBM peak (8.0 TB/s specified, 6.3 TB/s a float4 copy
                                         reaches); then the canvas, compose and visibility entry points each alone, the same way
  scene_gt, pad = (0, 0)                 in-image statistics only: renders of 480 x 640
Reported, not gated: there is no earlier device path to compare with.  The reference's own functions on maps of these sizes are timed on the host
by ``tests/golden/make_golden_g17.py --workload`` where the reference is present (its OpenGL render not included); this tool does not need it.
Usage:  timeout 600 python tools/scene_gt_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import cabi, devargs, render, scene_gt as SG, synth  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12   # bytes / s


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, F, seed, res = torch.device("cuda:0"), 64, 480, 640, 8, 7, []
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R = torch.from_numpy(synth._random_rotations(seed, "R", N)).to(dev)
    t = torch.from_numpy(np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)).to(dev)
    K = torch.from_numpy(np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)).to(dev)
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    meshes = render.MeshTable([v], [f], device=dev)
    labels, frame = np.zeros(N, dtype=np.int64), np.arange(N) // (N // F)
    px, py = W, H
    Hc, Wc = H + 2 * py, W + 2 * px
    Kc = K.clone()
    Kc[:, 0, 2] += px
    Kc[:, 1, 2] += py
    canvas = render.render_depth(meshes, labels, R, t, Kc, Hc, Wc)
    base = SG.scene_gt_from_depth(canvas, K, frame)   # composed: the nearest instance per frame
    # the frames' depth images: that surface in front of a wall at 2 m, +-2 mm of noise
    noise = torch.from_numpy(0.002 * (2.0 * u("noise", F, H, W) - 1.0)).to(dev).float()
    scene = torch.where(base.depth_scene > 0, base.depth_scene, torch.full_like(base.depth_scene, 2.0)) + noise
    shape = dict(N=N, F=F, H=H, W=W, canvas=[Hc, Wc], faces=int(len(f)), covered_fraction=float((base.mask != 0).float().mean()),
                 visible_fraction_mean=float(base.visib_fract.mean()))

    def report(call, fn, nbytes=None, **extra):
        times = timed(fn)[1]
        ms = statistics.median(times)
        row = dict(call=call, gpu_ms_median=ms, gpu_ms_min=min(times), gpu_ms_max=max(times), **extra)
        if nbytes is not None:
            rate = nbytes / (ms * 1e-3)
            row.update(needed_mbytes=nbytes / 1e6, gb_per_s=rate / 1e9, share_of_hbm_spec_peak=rate / HBM_SPEC, share_of_hbm_copy_rate=rate / HBM_COPY)
        res.append(row)
        print(json.dumps(row), flush=True)

    b_canvas = N * Hc * Wc * 4 + N * H * W * 4                       # every canvas value read, the window written
    b_compose = N * H * W * 4 + F * H * W * 4                        # every window read, the frames written
    b_visib = N * H * W * 4 + F * H * W * 4 + 2 * N * H * W          # window and depth images read, two masks written
    report("scene_gt with depth images (64 renders of 1440 x 1920 + passes)", lambda: SG.scene_gt(meshes, labels, R, t, K, H, W, frame, scene), **shape)
    report("scene_gt composed", lambda: SG.scene_gt(meshes, labels, R, t, K, H, W, frame))
    report("render_depth of the 64 canvases alone", lambda: render.render_depth(meshes, labels, R, t, Kc, Hc, Wc))
    report("scene_gt_from_depth with depth images (canvas + visibility passes)", lambda: SG.scene_gt_from_depth(canvas, K, frame, scene),
           b_canvas + b_visib)
    report("scene_gt_from_depth composed (canvas + compose + visibility passes)", lambda: SG.scene_gt_from_depth(canvas, K, frame),
           b_canvas + b_compose + b_visib)
    # the entry points alone, on the tensors of one result
    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(dev)
    g = SG.scene_gt_from_depth(canvas, K, frame, scene)
    fr_host = frame.astype(np.int32)
    fr = torch.from_numpy(fr_host).to(dev)
    off_host, inst_host = SG.csr_of_frames(fr_host, F)
    off, inst = torch.from_numpy(off_host).to(dev), torch.from_numpy(inst_host).to(dev)
    composed = torch.empty_like(scene)
    report("gdrn_scene_gt_canvas alone", lambda: cabi.check(lib.gdrn_scene_gt_canvas(p(canvas), N, H, W, px, py, p(g.depth), p(g.px_count_all),
                                                                                     p(g.bbox_obj), st), "canvas"), b_canvas)
    report("gdrn_scene_gt_compose alone", lambda: cabi.check(lib.gdrn_scene_gt_compose(p(g.depth), p(off), off_host.ctypes.data, p(inst),
                                                                                       inst_host.ctypes.data, F, N, H, W, p(composed), st), "compose"),
           b_compose)
    report("gdrn_scene_gt_visibility alone", lambda: cabi.check(lib.gdrn_scene_gt_visibility(
        p(g.depth), p(scene), p(fr), fr_host.ctypes.data, F, p(K), N, H, W, SG.DELTA, 0, p(g.mask), p(g.mask_visib), p(g.px_count_all),
        p(g.px_count_valid), p(g.px_count_visib), p(g.bbox_obj), p(g.bbox_visib), p(g.visib_fract), st), "visibility"), b_visib)
    report("scene_gt with depth images, pad = (0, 0) (64 renders of 480 x 640 + passes)",
           lambda: SG.scene_gt(meshes, labels, R, t, K, H, W, frame, scene, pad=(0, 0)))
    a, b = SG.scene_gt(meshes, labels, R, t, K, H, W, frame, scene), SG.scene_gt(meshes, labels, R, t, K, H, W, frame, scene, chunk=16)
    assert torch.equal(a.mask_visib, b.mask_visib) and torch.equal(a.bbox_obj, b.bbox_obj) and torch.equal(a.visib_fract, b.visib_fract)
    assert torch.equal(a.mask_visib, g.mask_visib) and torch.equal(composed, base.depth_scene)
    write_json(res)


if __name__ == "__main__":
    main()
