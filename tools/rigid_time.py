#!/usr/bin/env python3
"""Time gdrnet_amd.rigid with HIP events: 64 RoIs of 64 x 64 maps (4096 pixels each, all but the one that anchors the mask's minimum selected) in 8
observed frames of 480 x 640, 100 hypotheses.  The maps are synthesised from known poses: every RoI is a 64 x 64 window of its frame over a smooth
non-planar depth patch, its object coordinates are the back-projected pixels taken into the model frame (fp32, within a 1 mm ball), and 40 % of
them are displaced by 30 .. 120 mm in a random direction.  Four calls, timed INTERLEAVED (one of
each per round, 5 untimed rounds, then the median and range of 20), each behind an untimed 512 MB fill:
  backproject alone            rigid.backproject on the correspondences postproc extracted once
  gdrn_rigid_ransac alone      the entry point on its outputs, every buffer and the workspace allocated once: two launches
  poses_from_maps_rgbd         the chain: gdrn_correspondences, gdrn_backproject_points, gdrn_rigid_ransac on one stream, nothing read back
  pnp.pnp_ransac               the yardstick: the RGB solver on the same correspondences (3 px, 100 hypotheses)
Nothing is gated: the figures go into README.md and INTEGRATION.md.
Usage:  timeout 600 python tools/rigid_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import write_json  # noqa: E402
from gdrnet_amd import cabi, devargs, pnp, postproc, rigid, synth  # noqa: E402
from gdrnet_amd.cfg import lm13_cfg  # noqa: E402

WARMUP, ROUNDS, ITERS = 5, 20, 100
N, M, F, IM_H, IM_W, EXT = 64, 64, 8, 480, 640, 0.4


def workload(seed=11):
    """host arrays: the head's maps, the observed frames, the poses they were made from"""
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    K = synth.LM_K.astype(np.float64)
    Ki = np.linalg.inv(K)
    R = synth._random_rotations(seed, "R", N)
    frame = np.arange(N) // (N // F)
    depth = np.zeros((F, IM_H, IM_W), dtype=np.float32)
    mask = np.ones((N, 1, M, M), dtype=np.float32)
    mask[:, 0, 0, 0] = 0.0   # (the per-RoI min-max normalisation needs a minimum)
    coor = np.zeros((3, N, 1, M, M), dtype=np.float32)
    c2d = np.zeros((N, 2, M, M), dtype=np.float32)
    t = np.zeros((N, 3))
    good = u("out", N, M * M) >= 0.4
    dirs = synth.hash_normal(seed, "dir", (N, M * M, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    rad = u("rad", N, M * M, 1)
    for n in range(N):
        k = n % (N // F)
        x0, y0 = 30 + 150 * (k % 4), 80 + 220 * (k // 4)
        xs, ys = np.meshgrid(np.arange(x0, x0 + M), np.arange(y0, y0 + M))
        z = (0.6 + 0.8 * u("t_z", N)[n]) + 0.02 * np.sin(0.21 * xs + n) * np.cos(0.17 * ys) + 0.0004 * (xs - x0)
        depth[frame[n], y0 : y0 + M, x0 : x0 + M] = z.astype(np.float32)
        zf = depth[frame[n], y0 : y0 + M, x0 : x0 + M].astype(np.float64)
        P = (np.stack([xs, ys, np.ones_like(xs)], axis=-1).reshape(-1, 3) @ Ki.T) * zf.reshape(-1, 1)
        t[n] = P.mean(axis=0)
        X = (P - t[n]) @ R[n]   # R^T (P - t)
        X = X + np.where(good[n][:, None], 0.001 * np.cbrt(rad[n]), 0.03 + 0.09 * rad[n]) * dirs[n]
        for a in range(3):
            coor[a][n, 0] = (X[:, a] / EXT + 0.5).reshape(M, M)
        c2d[n, 0], c2d[n, 1] = xs / IM_W, ys / IM_H
    ext = np.full((N, 3), EXT, dtype=np.float32)
    return dict(mask=mask, coor=coor, c2d=c2d, ext=ext, depth=depth, frame=frame.astype(np.int32), K=K, R=R, t=t, good=good)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, a = "cuda:0", workload()
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    cfg = lm13_cfg()
    # the network's pose: the ground truth 10 degrees / 3 cm off
    ang = np.deg2rad(10.0)
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    out_dict = dict(mask=to(a["mask"]), coor_x=to(a["coor"][0]), coor_y=to(a["coor"][1]), coor_z=to(a["coor"][2]),
                    rot=to((Rz @ a["R"]).astype(np.float32)), trans=to((a["t"] + np.array([0.02, -0.01, 0.02])).astype(np.float32)))
    c2d, ext, scene, K = to(a["c2d"]), to(a["ext"]), to(a["depth"]), to(a["K"])
    im_H, im_W = [IM_H] * N, [IM_W] * N
    frame_host = a["frame"]
    _, _, img, mod, counts = postproc.get_img_model_points_with_coords2d(cfg, out_dict, c2d, ext, im_H, im_W)
    counts_host = counts.cpu().numpy()
    pts = rigid.backproject(img, mod, counts, scene, frame_host, K)
    S = int(img.shape[1])

    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(torch.device(dev))
    R_io = torch.eye(3, dtype=torch.float64, device=dev).repeat(N, 1, 1)
    t_io = torch.zeros(N, 3, dtype=torch.float64, device=dev)
    ok, num = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    rms = torch.empty(N, dtype=torch.float64, device=dev)
    msk = torch.empty(N, S, dtype=torch.uint8, device=dev)
    ws = devargs.workspace(lib.gdrn_rigid_workspace_bytes(N, S, ITERS), dev, "rigid_workspace_bytes")

    def ransac_alone():
        cabi.check(lib.gdrn_rigid_ransac(p(pts["cam_points"]), p(pts["model_points"]), p(pts["counts"]), N, S, 0.02, ITERS, 0, p(R_io), p(t_io), p(ok),
                                         p(num), p(msk), p(rms), p(ws), st), "rigid_ransac")

    calls = [("backproject alone", lambda: rigid.backproject(img, mod, counts, scene, frame_host, K)),
             ("gdrn_rigid_ransac alone", ransac_alone),
             ("poses_from_maps_rgbd", lambda: rigid.poses_from_maps_rgbd(cfg, out_dict, c2d, ext, im_H, im_W, K, scene, frame_host, iters=ITERS)),
             ("pnp.pnp_ransac", lambda: pnp.pnp_ransac(img, mod, counts_host, K, reproj_err=3.0, iters=ITERS, seed=0))]
    times, last = [[] for _ in calls], [None] * len(calls)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for it in range(WARMUP + ROUNDS):
        for k, (_, fn) in enumerate(calls):
            flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = fn()
            e1.record()
            e1.synchronize()
            if it >= WARMUP:
                times[k].append(e0.elapsed_time(e1))
    # what was timed is right: the chain and the raw call agree bit for bit, the poses are the ground truth, the inliers the undisplaced pixels
    chain = last[2]
    assert torch.equal(chain["pose_est"][:, :, :3], R_io) and torch.equal(chain["pose_est"][:, :, 3], t_io) and torch.equal(chain["ok"], ok)
    Rg, tg = R_io.cpu().numpy(), t_io.cpu().numpy()
    dev_gt = [max(float(np.arccos(np.clip(0.5 * (np.trace(Rg[n].T @ a["R"][n]) - 1.0), -1.0, 1.0))), float(np.linalg.norm(tg[n] - a["t"][n]) / np.linalg.norm(a["t"][n])))
              for n in range(N)]
    pn = last[3]
    shape = dict(N=N, maps=f"{M}x{M}", frames=f"{F} x {IM_H}x{IM_W}", hypotheses=ITERS, correspondences_min=int(counts_host.min()),
                 correspondences_max=int(counts_host.max()), with_depth_min=int(pts["counts"].min()), solved=int(ok.sum()),
                 inliers_median=int(num.median()), true_inliers_median=int(np.median(a["good"].sum(axis=1))),
                 deviation_from_truth_median=float(np.median(dev_gt)), deviation_from_truth_max=float(np.max(dev_gt)),
                 rms_mm_median=float(1e3 * rms.median()), pnp_solved=int(pn["ok"].sum()), rounds=ROUNDS)
    res = []
    for (name, _), ts in zip(calls, times):
        row = dict(call=name, gpu_ms_median=statistics.median(ts), gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        res.append(row)
        print(json.dumps(row), flush=True)
    med = [statistics.median(ts) for ts in times]
    verdict = dict(ransac_over_pnp=med[1] / med[3], chain_over_pnp=med[2] / med[3],
                   pairs_per_us_ransac_alone=N * S * ITERS / (med[1] * 1e3))
    print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape, **verdict)


if __name__ == "__main__":
    main()
