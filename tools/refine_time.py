#!/usr/bin/env python3
"""Time gdrnet_amd.refine with HIP events.  The workload: 64 estimates of the 20 480-face perturbed icosphere (the mesh of
tools/bop_metrics_time.py), eight to a frame, in 8 observed frames of 480 x 640 composed from the device's renders of the ground truth by the
nearest depth; every estimate starts 3 degrees / 5 mm off.  Five calls, timed INTERLEAVED (one of each per round, 5 untimed rounds, then the
median and range of 20), each behind an untimed 512 MB fill, so that it reads HBM and not what the call before it left in the last-level cache:
  icp_refine, 10 iterations    the whole loop: 10 x (render, accumulate, step) on one stream, no host read
  render_depth x 10            the same 64 instances rendered 10 times at the start poses: the yardstick -- the loop cannot be faster than
                               its renders
  gdrn_icp_accumulate alone    the entry point on renders, outputs and a workspace allocated once (needed bytes: 2 N H W 4, the render and
                               the frame under it; the frame is in fact read only where the render is covered)
  gdrn_icp_step alone          the solve-and-update launch on those systems (state reset by a memset inside the timed region)
  cou_from_depth               the other pass of this package that streams two depth maps per row, on the same renders (2 N H W 4)
Per call: ms; for the two streaming passes the needed bytes per second.  Then the passes' share of the loop, (loop - renders) / renders, and
accumulate as a fraction of ONE render.  Nothing is gated: the figures go into README.md and INTEGRATION.md.
Usage:  timeout 600 python tools/refine_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import write_json  # noqa: E402
from gdrnet_amd import cabi, cou_metrics as CM, devargs, refine, render, synth  # noqa: E402

WARMUP, ROUNDS, ITERS = 5, 20, 10


def workload(N, F, seed):
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R_gt = synth._random_rotations(seed, "R_gt", N)
    t_gt = np.concatenate([0.6 * u("t_xy", N, 2) - 0.3, 0.8 + 0.6 * u("t_z", N, 1)], axis=1)
    axis, direction = synth.hash_normal(seed, "axis", (N, 3)), synth.hash_normal(seed, "dir", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    R0 = synth._axis_angle(axis, np.full(N, 3.0)) @ R_gt
    t0 = t_gt + 5e-3 * direction
    K = np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)
    return dict(R_gt=R_gt, t_gt=t_gt, R0=R0, t0=t0, K=K, frame=np.arange(N) // (N // F))


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, F, seed = "cuda:0", 64, 480, 640, 8, 7
    host = workload(N, F, seed)
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
    o_R, o_t, o_state = R0.clone(), t0.clone(), torch.zeros(N, 2, dtype=torch.int32, device=dev)

    def accumulate():
        cabi.check(lib.gdrn_icp_accumulate(p(d_est), p(scene), p(frame), frame_host.ctypes.data, F, p(K), N, H, W, 0.02, 0.01, p(o_sys), p(o_pairs),
                                           p(o_ws), st), "icp_accumulate")

    def step():
        o_state.zero_()
        cabi.check(lib.gdrn_icp_step(p(o_sys), p(o_pairs), N, 64, p(o_R), p(o_t), p(o_state), st), "icp_step")

    def renders():
        for _ in range(ITERS):
            out = render.render_depth(meshes, labels, R0, t0, K, H, W)
        return out

    b_maps = 2 * N * H * W * 4
    calls = [(f"icp_refine, {ITERS} iterations", lambda: refine.icp_refine(meshes, labels, R0, t0, K, scene, frame_host, iters=ITERS), None),
             (f"render_depth x {ITERS}", renders, None),
             ("gdrn_icp_accumulate alone", accumulate, b_maps),
             ("gdrn_icp_step alone", step, None),
             ("cou_from_depth on the same renders", lambda: CM.cou_from_depth(d_est, d_gt), b_maps)]
    accumulate()   # the systems the step call reads
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
    ref = refine.normal_equations(d_est, scene, frame_host, K)
    assert torch.equal(o_pairs, ref["pairs"]) and torch.equal(o_sys[:, 27].contiguous().view(torch.int64), ref["sq"].view(torch.int64))
    dR = out["R"] @ R_gt.transpose(1, 2)
    re = torch.rad2deg(torch.acos(((dR.diagonal(dim1=1, dim2=2).sum(1) - 1.0) * 0.5).clamp(-1.0, 1.0)))
    te = 1e3 * (out["t"] - t_gt).norm(dim=1)
    shape = dict(N=N, H=H, W=W, F=F, faces=int(len(f)), iters=ITERS, covered_fraction=float((d_est > 0).float().mean()),
                 pairs_median=int(o_pairs.median()), ok=int(out["ok"].sum()), re_deg_median=float(re.median()), te_mm_median=float(te.median()),
                 iters_done_median=int(out["iters_done"].median()), rounds=ROUNDS)
    res = []
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        if nbytes is not None:
            row.update(needed_mbytes=nbytes / 1e6, gb_per_s=nbytes / (ms * 1e-3) / 1e9)
        res.append(row)
        print(json.dumps(row), flush=True)
    med = [statistics.median(ts) for ts in times]
    verdict = dict(passes_over_renders=(med[0] - med[1]) / med[1], accumulate_over_one_render=med[2] / (med[1] / ITERS),
                   step_over_one_render=med[3] / (med[1] / ITERS))
    print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape, **verdict)


if __name__ == "__main__":
    main()
