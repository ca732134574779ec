#!/usr/bin/env python3
"""Time the coarse depth alignment of gdrnet_amd.refine with HIP events, on the workload of tools/refine_time.py (64 estimates of the
20 480-face perturbed icosphere, eight to a frame, in 8 observed frames of 480 x 640) with every start moved a further 20 .. 60 mm along its
viewing ray, towards or away from the camera: what the ICP alone returns unchanged.  Four calls, timed INTERLEAVED (one of each per round, 5
untimed rounds, then the median and range of 20), each behind an untimed 512 MB fill:
  depth_align, 2 rounds        the whole loop: 2 x (render, compact, select, shift) on one stream, no host read
  render_depth x 2             the same 64 instances rendered twice at the start poses: the loop cannot be faster than its renders
  gdrn_depth_offset alone      the entry point on renders, outputs and a workspace allocated once
  gdrn_icp_accumulate alone    the yardstick on the same renders: a pass that streams the same maps once
Then the passes' share of the loop, (loop - renders) / renders, and the offset pass in units of the accumulate pass.  Nothing is gated: the
figures go into README.md and INTEGRATION.md.
Usage:  timeout 600 python tools/depth_align_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import write_json  # noqa: E402
from refine_time import workload  # noqa: E402
from gdrnet_amd import cabi, devargs, refine, render, synth  # noqa: E402

WARMUP, ROUNDS, ALIGN_ROUNDS = 5, 20, 2


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, F, seed = "cuda:0", 64, 480, 640, 8, 7
    host = workload(N, F, seed)
    u = synth.hash_uniform(seed, "extra", (N,))
    extra = np.where(synth.hash_uniform(seed, "extra/sign", (N,)) < 0.5, -1.0, 1.0) * (0.02 + 0.04 * u)
    host["t0"] = host["t0"] + extra[:, None] * host["t_gt"] / host["t_gt"][:, 2:3]
    R_gt, t_gt, R0, t0, K = (torch.from_numpy(host[k]).to(dev) for k in ("R_gt", "t_gt", "R0", "t0", "K"))
    frame_host = host["frame"].astype(np.int32)
    frame = torch.from_numpy(frame_host).to(dev)
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    meshes = render.MeshTable([v], [f], device=dev)
    labels = np.zeros(N, dtype=np.int64)
    d_gt = render.render_depth(meshes, labels, R_gt, t_gt, K, H, W)
    far = torch.where(d_gt > 0, d_gt, torch.full_like(d_gt, float("inf"))).view(F, N // F, H, W).amin(dim=1)
    scene = torch.where(torch.isinf(far), torch.zeros_like(far), far).contiguous()   # the nearest ground-truth surface, 0 where there is none
    d_est = render.render_depth(meshes, labels, R0, t0, K, H, W)

    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(torch.device(dev))
    o_sys, o_pairs = torch.empty(N, 28, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    o_ws = devargs.workspace(lib.gdrn_icp_workspace_bytes(N, H, W), dev, "icp_workspace_bytes")
    a_off = torch.empty(N, dtype=torch.float64, device=dev)
    a_pairs, a_cov, a_ok = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    a_ws = devargs.workspace(lib.gdrn_depth_align_workspace_bytes(N, H, W), dev, "depth_align_workspace_bytes")

    def accumulate():
        cabi.check(lib.gdrn_icp_accumulate(p(d_est), p(scene), p(frame), frame_host.ctypes.data, F, p(K), N, H, W, 0.02, 0.01, p(o_sys), p(o_pairs),
                                           p(o_ws), st), "icp_accumulate")

    def offset():
        cabi.check(lib.gdrn_depth_offset(p(d_est), p(scene), p(frame), frame_host.ctypes.data, F, N, H, W, 0.2, 64, p(a_off), p(a_pairs), p(a_cov),
                                         p(a_ok), p(a_ws), st), "depth_offset")

    def renders():
        for _ in range(ALIGN_ROUNDS):
            out = render.render_depth(meshes, labels, R0, t0, K, H, W)
        return out

    b_maps = 2 * N * H * W * 4
    calls = [(f"depth_align, {ALIGN_ROUNDS} rounds", lambda: refine.depth_align(meshes, labels, R0, t0, K, scene, frame_host, rounds=ALIGN_ROUNDS), None),
             (f"render_depth x {ALIGN_ROUNDS}", renders, None),
             ("gdrn_depth_offset alone", offset, b_maps),
             ("gdrn_icp_accumulate alone", accumulate, b_maps)]
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
    out = last[0]
    ref = refine.depth_offset(d_est, scene, frame_host)
    assert torch.equal(a_pairs, ref["pairs"]) and torch.equal(a_off.view(torch.int64), ref["offset"].view(torch.int64))
    ray = t_gt / t_gt.norm(dim=1, keepdim=True)
    along0 = 1e3 * ((t0 - t_gt) * ray).sum(dim=1).abs()
    along = 1e3 * ((out["t"] - t_gt) * ray).sum(dim=1).abs()
    alone = refine.icp_refine(meshes, labels, R0, t0, K, scene, frame_host)
    both = refine.icp_refine(meshes, labels, R0, out["t"], K, scene, frame_host)
    te = 1e3 * (both["t"] - t_gt).norm(dim=1)
    shape = dict(N=N, H=H, W=W, F=F, faces=int(len(f)), rounds_of_align=ALIGN_ROUNDS, covered_fraction=float((d_est > 0).float().mean()),
                 pairs_fraction=float(a_pairs.sum()) / (N * H * W), pairs_median=int(a_pairs.median()), align_ok=int(out["ok"].sum()),
                 along_ray_mm_median_before=float(along0.median()), along_ray_mm_median_after=float(along.median()),
                 along_ray_mm_max_after=float(along.max()), along_ray_over_10_mm_after=int((along > 10.0).sum()), icp_ok_without_align=int(alone["ok"].sum()), icp_ok_after_align=int(both["ok"].sum()),
                 te_mm_median_after_icp=float(te.median()), rounds=ROUNDS)
    res = []
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        if nbytes is not None:
            row.update(needed_mbytes=nbytes / 1e6, gb_per_s=nbytes / (ms * 1e-3) / 1e9)
        res.append(row)
        print(json.dumps(row), flush=True)
    med = [statistics.median(ts) for ts in times]
    verdict = dict(passes_over_renders=(med[0] - med[1]) / med[1], offset_over_accumulate=med[2] / med[3],
                   offset_over_one_render=med[2] / (med[1] / ALIGN_ROUNDS))
    print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape, **verdict)


if __name__ == "__main__":
    main()
