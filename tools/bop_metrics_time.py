#!/usr/bin/env python3
"""Time gdrnet_amd.bop_metrics with HIP events: median of 20 calls after 5 warm-ups, 64 rows,
  vsd             480 x 640 frames, the 20 480-face perturbed icosphere, 10 taus, step cost: the two renders included (vsd) and on depth maps that are
                  already there (vsd_from_depth), plus vsd_from_depth with the tlinear cost,
  mssd_mspd       16 384 model points x 314 symmetry transformations (a continuous symmetry at BOP's step), and x 1,
and for context the host loop of tests/bop_host.py (numpy, what the toolkit's per-estimate functions do, without their renders) over 8 rows, scaled
to 64.  Reported, not gated: there is no earlier device path to compare with.  Usage:  timeout 600 python tools/bop_metrics_time.py [--json FILE]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_host as BH  # noqa: E402
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import bop_metrics as BM, render, synth  # noqa: E402

HOST_ROWS = 8


def report(res, call, times, **extra):
    row = dict(call=call, gpu_ms_median=statistics.median(times), gpu_ms_min=min(times), gpu_ms_max=max(times), **extra)
    res.append(row)
    return row


def show(row):
    print(json.dumps(row), flush=True)


def poses(N, seed):
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R_gt = synth._random_rotations(seed, "R_gt", N)
    axis = synth.hash_normal(seed, "axis", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    R_est = synth._axis_angle(axis, 0.5 + 10 * u("ang", N)) @ R_gt
    t_gt = np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)
    t_est = t_gt + 0.03 * (u("off", N, 3) - 0.5)
    K = np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)
    return dict(R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, F, seed, res = "cuda:0", 64, 480, 640, 8, 7, []
    host = poses(N, seed)
    P = [torch.from_numpy(host[k]).to(dev) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]

    # ---- VSD ----
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    meshes = render.MeshTable([v], [f], device=dev)
    labels, frame, diam = np.zeros(N, dtype=np.int64), np.arange(N) // (N // F), 0.23
    d_est = render.render_depth(meshes, labels, P[0], P[1], P[4], H, W)
    d_gt = render.render_depth(meshes, labels, P[2], P[3], P[4], H, W)
    # test images: per frame the nearest ground-truth surface in front of a wall at 2 m, +-2 mm of noise
    wall = torch.full((F, H, W), 2.0, dtype=torch.float32, device=dev)
    near = torch.where(d_gt > 0, d_gt, torch.full_like(d_gt, 9.0)).reshape(F, N // F, H, W).amin(dim=1)
    d_test = torch.minimum(wall, near) + torch.from_numpy(0.002 * (2.0 * synth.hash_uniform(seed, "noise", (F, H, W)) - 1.0)).to(dev).float()
    taus = BM.VSD_TAUS
    shape = dict(N=N, H=H, W=W, faces=int(len(f)), taus=len(taus), covered_fraction=float((d_gt != 0).float().mean()))
    err, t_all = timed(lambda: BM.vsd(meshes, labels, *P, d_test, frame, [diam], synth.BOP_VSD_DELTA, taus))
    show(report(res, "vsd (2 x 64 renders + errors)", t_all, **shape))
    _, t_r = timed(lambda: render.render_depth(meshes, np.concatenate([labels, labels]), torch.cat([P[0], P[2]]), torch.cat([P[1], P[3]]),
                                               torch.cat([P[4], P[4]]), H, W))
    show(report(res, "render_depth (128 instances) alone", t_r, **shape))
    (err2, counts), t_v = timed(lambda: BM.vsd_from_depth(d_est, d_gt, d_test, frame, P[4], [diam] * N, synth.BOP_VSD_DELTA, taus, return_counts=True))
    row = report(res, "vsd_from_depth (step)", t_v, mpixel_per_s=N * H * W / statistics.median(t_v) / 1e3, **shape)
    _, t_l = timed(lambda: BM.vsd_from_depth(d_est, d_gt, d_test, frame, P[4], [diam] * N, synth.BOP_VSD_DELTA, taus, cost_type="tlinear"))
    show(report(res, "vsd_from_depth (tlinear)", t_l, **shape))
    assert torch.equal(err, err2)
    he, hg, ht, got, got_counts = d_est[:HOST_ROWS].cpu().numpy(), d_gt[:HOST_ROWS].cpu().numpy(), d_test.cpu().numpy(), err2.cpu().numpy(), counts.cpu().numpy()
    t0 = time.perf_counter()
    ref = [BH.vsd(he[i], hg[i], ht[frame[i]], host["K"][i], synth.BOP_VSD_DELTA, taus, diam) for i in range(HOST_ROWS)]
    row["host_ms_for_64_rows"] = (time.perf_counter() - t0) * 1e3 * N / HOST_ROWS
    row["host_rows_timed"] = HOST_ROWS
    row["count_cells_differing_from_host"] = int(sum((r[1] != got_counts[i]).sum() for i, r in enumerate(ref)))
    row["worst_abs_diff_to_host"] = float(max(np.abs(r[0] - got[i]).max() for i, r in enumerate(ref)))
    show(row)

    # ---- MSSD / MSPD ----
    n = 16384
    pts = [-0.1 + 0.2 * synth.hash_uniform(seed, f"pts{c}", (n, 3)) for c in range(4)]
    cont = BM.symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.01, -0.02, 0.0]}]})
    lab4 = np.arange(N) % 4
    for name, syms in (("314 transformations", [cont] * 4), ("1 transformation", None)):
        table = BM.BopModelTable(pts, [0.2] * 4, syms)
        e, t_m = timed(lambda: BM.mssd_mspd(table, *P, lab4))
        row = report(res, f"mssd_mspd, {n} points x {name}", t_m, N=N, points=n, transformations=int(table.s_max))
        e = e.cpu().numpy()
        S = (np.eye(3)[None], np.zeros((1, 3))) if syms is None else cont
        t0 = time.perf_counter()
        ref = np.array([BH.mssd_mspd(host["R_est"][i], host["t_est"][i], host["R_gt"][i], host["t_gt"][i], host["K"][i], pts[lab4[i]], *S)[:2]
                        for i in range(HOST_ROWS)])
        row["host_ms_for_64_rows"] = (time.perf_counter() - t0) * 1e3 * N / HOST_ROWS
        row["host_rows_timed"] = HOST_ROWS
        row["worst_abs_diff_to_host"] = [float(np.abs(ref[:, k] - e[:HOST_ROWS, k]).max()) for k in (0, 1)]
        show(row)
    write_json(res)


if __name__ == "__main__":
    main()
