#!/usr/bin/env python3
"""Time gdrnet_amd.verify with HIP events.  The workload is that of tools/refine_time.py: 64 instances of the 20 480-face perturbed icosphere,
eight to a frame, in 8 observed frames of 480 x 640 composed from the device's renders of the ground truth by the nearest depth; the observed
mask of an instance is its visible ground truth (its render where it is the nearest surface).  Three candidates per instance: the ground truth,
3 degrees / 5 mm off, and 30 mm behind -- 192 rows.  Four calls, timed INTERLEAVED (one of each per round, 5 untimed rounds, then the median and
range of 20), each behind an untimed 512 MB fill, so that it reads HBM and not what the call before it left in the last-level cache:
  gdrn_verify_maps alone       the counting pass on renders, outputs and a workspace allocated once (needed bytes: N H W (4 + 1), the render and
                               the mask, plus the frame under the covered pixels)
  cou_from_depth               the other pass of this package that streams maps per row, on the same renders against themselves shifted by
                               one candidate (2 N H W 4): the yardstick
  verify_poses                 render, count, score on one stream, no host read
  render_depth                 the same rows rendered once: verify_poses cannot be faster than its render
Per call: ms; for the two streaming passes the needed bytes per second.  Then maps / cou and (verify_poses - render) / render.  Nothing is gated:
the figures go into README.md.
Usage:  timeout 600 python tools/verify_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import write_json  # noqa: E402
from refine_time import workload  # noqa: E402
from gdrnet_amd import cabi, cou_metrics as CM, devargs, render, synth, verify  # noqa: E402

WARMUP, ROUNDS = 5, 20


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, M, H, W, F, seed = "cuda:0", 64, 480, 640, 8, 7
    host = workload(M, F, seed)
    R_gt, t_gt, R0, t0, K = (torch.from_numpy(host[k]).to(dev) for k in ("R_gt", "t_gt", "R0", "t0", "K"))
    det_frame = host["frame"].astype(np.int32)
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    meshes = render.MeshTable([v], [f], device=dev)
    d_gt = render.render_depth(meshes, np.zeros(M, dtype=np.int64), R_gt, t_gt, K, H, W)
    far = torch.where(d_gt > 0, d_gt, torch.full_like(d_gt, float("inf"))).view(F, M // F, H, W).amin(dim=1)
    scene = torch.where(torch.isinf(far), torch.zeros_like(far), far).contiguous()   # the nearest ground-truth surface, 0 where there is none
    masks = ((d_gt > 0) & (d_gt == scene[torch.from_numpy(det_frame).to(dev).long()])).to(torch.uint8).contiguous()   # the visible ground truth
    t_back = t_gt * (1.0 + 0.030 / t_gt[:, 2:3])
    candidates = [(R_gt, t_gt), (R0, t0), (R_gt, t_back)]
    C = len(candidates)
    N = C * M
    R, t, Kn = torch.cat([c[0] for c in candidates]), torch.cat([c[1] for c in candidates]), K.repeat(C, 1, 1)
    labels = np.zeros(N, dtype=np.int64)
    frame_host, det_host = np.tile(det_frame, C), np.tile(np.arange(M, dtype=np.int32), C)
    frame, det = torch.from_numpy(frame_host).to(dev), torch.from_numpy(det_host).to(dev)
    d_ren = render.render_depth(meshes, labels, R, t, Kn, H, W)
    d_other = torch.roll(d_ren, M, dims=0).contiguous()

    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(torch.device(dev))
    o_counts, o_sum = torch.empty(N, 8, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int64, device=dev)
    o_ws = devargs.workspace(lib.gdrn_verify_workspace_bytes(N, H, W), dev, "verify_workspace_bytes")

    def maps():
        cabi.check(lib.gdrn_verify_maps(p(d_ren), p(scene), p(frame), frame_host.ctypes.data, F, p(masks), p(det), det_host.ctypes.data, M, N, H, W,
                                        0.01, p(o_counts), p(o_sum), p(o_ws), st), "verify_maps")

    covered = int((d_ren > 0).sum())
    b_maps, b_cou = N * H * W * 5 + covered * 4, 2 * N * H * W * 4
    calls = [("gdrn_verify_maps alone", maps, b_maps),
             ("cou_from_depth on the same renders", lambda: CM.cou_from_depth(d_ren, d_other), b_cou),
             ("verify_poses", lambda: verify.verify_poses(meshes, labels, R, t, Kn, scene, frame_host, masks, det_host), None),
             ("render_depth", lambda: render.render_depth(meshes, labels, R, t, Kn, H, W), None)]
    times, last = [[] for _ in calls], [None] * len(calls)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for it in range(WARMUP + ROUNDS):
        for k, (_, fn, _) in enumerate(calls):
            flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = fn()
            e1.record()
            e1.synchronize()
            if it >= WARMUP:
                times[k].append(e0.elapsed_time(e1))
    out = last[2]
    ref = verify.verify_maps(d_ren, scene, frame_host, masks, det_host)
    assert torch.equal(o_counts[:, 0].contiguous(), ref["covered"]) and torch.equal(o_sum, ref["sum_q"])
    assert all(torch.equal(out[k].view(torch.int64) if out[k].dtype == torch.float64 else out[k],
                           ref[k].view(torch.int64) if ref[k].dtype == torch.float64 else ref[k]) for k in ref)
    sel = verify.select_best(out["score"], out["ok"], det_host, M)
    score = out["score"].view(C, M)
    shape = dict(N=N, M=M, C=C, H=H, W=W, F=F, faces=int(len(f)), covered_fraction=covered / (N * H * W), rounds=ROUNDS,
                 ground_truth_wins=int(((sel["best"] >= 0) & (sel["best"] < M)).sum()), score_median_per_candidate=[float(score[c].median()) for c in range(C)])
    res = []
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        if nbytes is not None:
            row.update(needed_mbytes=nbytes / 1e6, gb_per_s=nbytes / (ms * 1e-3) / 1e9)
        res.append(row)
        print(json.dumps(row), flush=True)
    med = [statistics.median(ts) for ts in times]
    ratios = [a / b for a, b in zip(times[0], times[1])]   # round by round
    verdict = dict(maps_over_cou=med[0] / med[1], maps_over_cou_min=min(ratios), maps_over_cou_max=max(ratios),
                   passes_over_render=(med[2] - med[3]) / med[3])
    print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape, **verdict)


if __name__ == "__main__":
    main()
