#!/usr/bin/env python3
"""Time the silhouette term of gdrnet_amd.refine with HIP events, on the workload of tools/refine_time.py: 64 estimates of the 20 480-face
perturbed icosphere, eight to a frame, in 8 observed frames of 480 x 640 composed from the device's renders of the ground truth by the nearest
depth; every estimate starts 3 degrees / 5 mm off.  The observed mask of an estimate is the visible part of its ground truth.  Six calls,
timed INTERLEAVED (one of each per round, 5 untimed rounds, then the median and range of 20), each behind an untimed 512 MB fill:
  icp_refine, 10 iterations        the loop without the term: the yardstick (its code is what it was before the term existed)
  icp_refine_sil, 10 iterations    the contour transform once, then 10 x (render, depth accumulate and combine, silhouette accumulate, step)
  render_depth x 10                the same 64 instances rendered 10 times at the start poses: neither loop can be faster than its renders
  gdrn_sil_contour_transform alone on masks, outputs and a workspace allocated once (three launches; paid once per call, not per iteration)
  gdrn_sil_accumulate alone        on the start renders and that transform (needed bytes: N H W 4, the render; the frame, d2 and nearest are
                                   read on the render's contour only)
  gdrn_icp_accumulate alone        the depth term's pass on the same renders (2 N H W 4), for scale
Then what the term adds to the loop, (icp_refine_sil - icp_refine) / icp_refine, the transform's share of that, and the silhouette pass as a
fraction of the depth pass and of ONE render.  With ``--icp-only`` only the first and the third call run: for timing icp_refine with another
build of the library (GDRN_HIP_LIB) on the same box.  Nothing is gated: the figures go into README.md and INTEGRATION.md.
Usage:  timeout 600 python tools/refine_sil_time.py [--icp-only] [--json FILE]"""
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

WARMUP, ROUNDS, ITERS = 5, 20, 10


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    icp_only = "--icp-only" in sys.argv
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
    mask = ((d_gt > 0) & (d_gt == scene[frame.long()])).to(torch.uint8).contiguous()  # the visible part of each ground truth
    d_est = render.render_depth(meshes, labels, R0, t0, K, H, W)

    def renders():
        for _ in range(ITERS):
            out = render.render_depth(meshes, labels, R0, t0, K, H, W)
        return out

    calls = [(f"icp_refine, {ITERS} iterations", lambda: refine.icp_refine(meshes, labels, R0, t0, K, scene, frame_host, iters=ITERS), None),
             (f"render_depth x {ITERS}", renders, None)]
    if not icp_only:
        lib, p, st = cabi.load(), cabi.ptr, devargs.stream(torch.device(dev))
        o_sys, o_pairs = torch.empty(N, 28, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        o_d2, o_near = torch.empty(N, H, W, dtype=torch.int32, device=dev), torch.empty(N, H, W, dtype=torch.int32, device=dev)
        o_contour = torch.empty(N, dtype=torch.int32, device=dev)
        o_ws = devargs.workspace(lib.gdrn_sil_workspace_bytes(N, H, W), dev, "sil_workspace_bytes")
        i_ws = devargs.workspace(lib.gdrn_icp_workspace_bytes(N, H, W), dev, "icp_workspace_bytes")

        def transform():
            cabi.check(lib.gdrn_sil_contour_transform(p(mask), p(scene), p(frame), frame_host.ctypes.data, F, N, H, W, p(o_d2), p(o_near), p(o_contour),
                                                      p(o_ws), st), "sil_contour_transform")

        def sil_accumulate():
            cabi.check(lib.gdrn_sil_accumulate(p(d_est), p(scene), p(frame), frame_host.ctypes.data, F, p(K), p(o_d2), p(o_near), N, H, W, 8.0, 0.02,
                                               p(o_sys), p(o_pairs), p(o_ws), st), "sil_accumulate")

        def icp_accumulate():
            cabi.check(lib.gdrn_icp_accumulate(p(d_est), p(scene), p(frame), frame_host.ctypes.data, F, p(K), N, H, W, 0.02, 0.01, p(o_sys), p(o_pairs),
                                               p(i_ws), st), "icp_accumulate")

        transform()   # the maps the silhouette pass reads
        calls.insert(1, (f"icp_refine_sil, {ITERS} iterations",
                         lambda: refine.icp_refine_sil(meshes, labels, R0, t0, K, scene, frame_host, mask, iters=ITERS), None))
        calls += [("gdrn_sil_contour_transform alone", transform, None), ("gdrn_sil_accumulate alone", sil_accumulate, N * H * W * 4),
                  ("gdrn_icp_accumulate alone", icp_accumulate, 2 * N * H * W * 4)]
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

    def errors(out):
        dR = out["R"] @ R_gt.transpose(1, 2)
        re = torch.rad2deg(torch.acos(((dR.diagonal(dim1=1, dim2=2).sum(1) - 1.0) * 0.5).clamp(-1.0, 1.0)))
        return float(re.median()), float((1e3 * (out["t"] - t_gt).norm(dim=1)).median())

    shape = dict(N=N, H=H, W=W, F=F, faces=int(len(f)), iters=ITERS, rounds=ROUNDS, library=cabi.LIB_PATH, icp_ok=int(last[0]["ok"].sum()))
    shape["icp_re_deg_median"], shape["icp_te_mm_median"] = errors(last[0])
    if not icp_only:
        out = last[1]
        sil_accumulate()
        ref = refine.silhouette_equations(d_est, mask, scene, frame_host, K)
        assert torch.equal(o_pairs, ref["pairs"]) and torch.equal(o_sys[:, 27].contiguous().view(torch.int64), ref["sq"].view(torch.int64))
        shape.update(sil_ok=int(out["ok"].sum()), contour_pixels_median=int(o_contour.median()), sil_pairs_median=int(out["sil_pairs"].median()),
                     pairs_median=int(out["pairs"].median()), mask_fraction=float(mask.float().mean()))
        shape["sil_re_deg_median"], shape["sil_te_mm_median"] = errors(out)
    res = []
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        if nbytes is not None:
            row.update(needed_mbytes=nbytes / 1e6, gb_per_s=nbytes / (ms * 1e-3) / 1e9)
        res.append(row)
        print(json.dumps(row), flush=True)
    med = [statistics.median(ts) for ts in times]
    verdict = {}
    if not icp_only:
        one_render = med[2] / ITERS
        verdict = dict(term_over_icp_refine=(med[1] - med[0]) / med[0], transform_share_of_the_term=med[3] / (med[1] - med[0]),
                       sil_accumulate_over_icp_accumulate=med[4] / med[5], sil_accumulate_over_one_render=med[4] / one_render,
                       transform_over_one_render=med[3] / one_render)
        print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape, **verdict)


if __name__ == "__main__":
    main()
