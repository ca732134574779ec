#!/usr/bin/env python3
"""Time gdrnet_amd.cou_metrics with HIP events.  The workload is that of tools/bop_metrics_time.py: 64 estimates at 480 x 640 over the 20 480-face
perturbed icosphere.  Six calls on the same maps, timed INTERLEAVED (one of each per round, 5 untimed rounds, then the median and range of 20),
each behind an untimed 512 MB fill, so that it reads HBM and not what the call before it left in the 256 MB last-level cache:
  cou_from_depth            the fused pass on the 2 x 64 rendered fp32 maps (needed bytes: 2 N H W 4)
  cou_mask                  the same on byte masks (2 N H W)
  torch composition         what a user would write without it for the same counts and boxes: ((e > 0) & (g > 0)).sum((1, 2)),
                            ((e > 0) | (g > 0)).sum((1, 2)) and the four bounds of either map through any / argmax -- no errors, no host loop
  device-to-device copy     a plain copy of the depth maps' bytes (2 N H W 4 read, as many written): the streaming yardstick
  gdrn_cou_maps alone       the entry point on outputs and a workspace allocated once, both element kinds: the three launches without the
                            wrapper's argument checks and four allocations
Per call: ms, the needed bytes per second and that rate as a fraction of the copy's READ rate.  Then, timed the usual way (median of 20 after 5
warm-ups): cus(...) end to end next to render_depth of the same 128 instances alone, and the reduce pass's share of cus.
Gated on one thing only: the fused pass is faster than the torch composition in this run, with non-overlapping min-max ranges over the rounds --
it has no other reason to exist.  Usage:  timeout 300 python tools/cou_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timed, write_json  # noqa: E402
from bop_metrics_time import poses  # noqa: E402
from gdrnet_amd import cabi, cou_metrics as CM, devargs, render, synth  # noqa: E402

WARMUP, ROUNDS = 5, 20


def torch_composition(e, g):
    """counts [N,2] and boxes [N,2,4] of two [N,H,W] maps (> 0 = covered) in plain torch ops; an empty map's box is (0, 0, -1, -1)"""
    ce, cg = e > 0, g > 0
    counts = torch.stack([(ce & cg).sum((1, 2)), (ce | cg).sum((1, 2))], dim=1)
    boxes = []
    for c in (ce, cg):
        cols, rows = c.any(1), c.any(2)                      # [N,W], [N,H]
        W, H = cols.shape[1], rows.shape[1]
        some = cols.any(1)
        x1, y1 = cols.int().argmax(1), rows.int().argmax(1)
        x2, y2 = W - 1 - cols.flip(1).int().argmax(1), H - 1 - rows.flip(1).int().argmax(1)
        zero, minus = torch.zeros_like(x1), torch.full_like(x1, -1)
        boxes.append(torch.stack([torch.where(some, x1, zero), torch.where(some, y1, zero), torch.where(some, x2, minus), torch.where(some, y2, minus)], 1))
    return counts, torch.stack(boxes, dim=1)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, seed = "cuda:0", 64, 480, 640, 7
    host = poses(N, seed)
    P = [torch.from_numpy(host[k]).to(dev) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    meshes = render.MeshTable([v], [f], device=dev)
    labels = np.zeros(N, dtype=np.int64)
    d_est = render.render_depth(meshes, labels, P[0], P[1], P[4], H, W)
    d_gt = render.render_depth(meshes, labels, P[2], P[3], P[4], H, W)
    m_est, m_gt = (d_est > 0).to(torch.uint8) * 255, (d_gt > 0).to(torch.uint8) * 255
    c_est, c_gt = torch.empty_like(d_est), torch.empty_like(d_gt)
    b_depth, b_mask = 2 * N * H * W * 4, 2 * N * H * W

    def copy():
        c_est.copy_(d_est)
        c_gt.copy_(d_gt)

    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(torch.device(dev))
    o_err = torch.empty(N, 2, dtype=torch.float64, device=dev)
    o_counts, o_boxes = torch.empty(N, 2, dtype=torch.int32, device=dev), torch.empty(N, 2, 4, dtype=torch.int32, device=dev)
    o_ws = devargs.workspace(lib.gdrn_cou_maps_workspace_bytes(N), dev, "cou_maps_workspace_bytes")

    def entry(est, gt, kind):
        cabi.check(lib.gdrn_cou_maps(p(est), p(gt), CM.KINDS[kind], N, H, W, p(o_err), p(o_counts), p(o_boxes), p(o_ws), st), "cou_maps")

    calls = [("cou_from_depth", lambda: CM.cou_from_depth(d_est, d_gt, return_parts=True), b_depth),
             ("cou_mask", lambda: CM.cou_mask(m_est, m_gt, return_parts=True), b_mask),
             ("torch composition (counts and boxes only)", lambda: torch_composition(d_est, d_gt), b_depth),
             ("device-to-device copy of the depth maps", copy, b_depth),
             ("gdrn_cou_maps alone, fp32 depth", lambda: entry(d_est, d_gt, "depth"), b_depth),
             ("gdrn_cou_maps alone, byte masks", lambda: entry(m_est, m_gt, "mask"), b_mask)]
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
    (err, counts, boxes), (err_m, counts_m, boxes_m), (t_counts, t_boxes) = last[0], last[1], last[2]
    assert torch.equal(counts.long(), t_counts) and torch.equal(boxes.long(), t_boxes.long()) and torch.equal(counts, counts_m) and torch.equal(boxes, boxes_m)
    assert torch.equal(err, err_m) and torch.equal(c_est, d_est) and torch.equal(o_err, err) and torch.equal(o_boxes, boxes)
    shape = dict(N=N, H=H, W=W, faces=int(len(f)), covered_fraction=float((d_gt > 0).float().mean()), cus_min=float(err[:, 0].min()),
                 cus_max=float(err[:, 0].max()), rounds=ROUNDS)
    copy_rate = b_depth / (statistics.median(times[3]) * 1e-3)
    res = []
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        rate = nbytes / (ms * 1e-3)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts), needed_mbytes=nbytes / 1e6, gb_per_s=rate / 1e9,
                   fraction_of_copy_read_rate=rate / copy_rate)
        res.append(row)
        print(json.dumps(row), flush=True)

    _, t_cus = timed(lambda: CM.cus(meshes, labels, *P, H, W))
    _, t_r = timed(lambda: render.render_depth(meshes, np.concatenate([labels, labels]), torch.cat([P[0], P[2]]), torch.cat([P[1], P[3]]),
                                               torch.cat([P[4], P[4]]), H, W))
    _, t_warm = timed(lambda: CM.cou_from_depth(d_est, d_gt))   # back to back, as inside cus: the maps may still be in the last-level cache
    for name, ts in (("cus (2 x 64 renders + the reduce pass)", t_cus), ("render_depth (128 instances) alone", t_r),
                     ("cou_from_depth back to back (no flush)", t_warm)):
        row = dict(call=name, gpu_ms_median=statistics.median(ts), gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        res.append(row)
        print(json.dumps(row), flush=True)
    share = 1.0 - statistics.median(t_r) / statistics.median(t_cus)
    verdict = dict(reduce_share_of_cus=share, fused_over_torch=statistics.median(times[0]) / statistics.median(times[2]),
                   fused_max_ms=max(times[0]), torch_min_ms=min(times[2]), ranges_do_not_overlap=max(times[0]) < min(times[2]))
    print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape, **verdict)
    assert verdict["ranges_do_not_overlap"], "the fused pass is not clearly ahead of the torch composition: it has no reason to exist"


if __name__ == "__main__":
    main()
