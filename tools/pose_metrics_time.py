#!/usr/bin/env python3
"""Time gdrnet_amd.pose_metrics.pose_errors with HIP events: median of 20 calls after 5 warm-ups, N = 64 poses, for
  (a) 16 384 model points, every class symmetric (adi: the O(n^2) nearest-neighbour path),
  (b) 16 384 model points, no class symmetric (add),
  (c) 3 000 model points, every class symmetric,
and, where SciPy is importable, the host loop the evaluator runs for the same rows (one cKDTree build + query per row).
Reported, not gated.  Usage:  timeout 300 python tools/pose_metrics_time.py [--json FILE]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import pose_metrics as PM, synth  # noqa: E402


def inputs(N, n, sym, ncls=4, seed=7):
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    pts = [-0.1 + 0.2 * u(f"pts{c}", n, 3) for c in range(ncls)]
    rz = np.diag([-1.0, -1.0, 1.0])
    table = PM.ModelTable(pts, [0.2] * ncls, [rz[None]] * ncls if sym else None, tuple(range(ncls)) if sym else ())
    R_gt = synth._random_rotations(seed, "R_gt", N)
    axis = synth.hash_normal(seed, "axis", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    R_est = synth._axis_angle(axis, 0.1 + 10 * u("ang", N)) @ R_gt
    t_gt = np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)
    t_est = t_gt + 0.02 * (u("off", N, 3) - 0.5)
    K = np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)
    return table, pts, dict(R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K), np.arange(N) % ncls


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, res = "cuda:0", 64, []
    for name, n, sym in (("n=16384 symmetric (adi)", 16384, True), ("n=16384 non-symmetric (add)", 16384, False), ("n=3000 symmetric (adi)", 3000, True)):
        table, pts, host, labels = inputs(N, n, sym)
        poses = [torch.from_numpy(host[k]).to(dev) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
        out, times = timed(lambda: PM.pose_errors(table, *poses, labels))
        row = dict(shape=name, N=N, gpu_ms_median=statistics.median(times), gpu_ms_min=min(times), gpu_ms_max=max(times))
        try:
            from scipy import spatial

            ad = out["ad"].cpu().numpy()
            rows = range(N) if n <= 4096 else range(8)   # the large shape: 8 rows, scaled
            t0 = time.perf_counter()
            worst = 0.0
            for i in rows:
                p = pts[labels[i]]
                pe, pg = p @ host["R_est"][i].T + host["t_est"][i], p @ host["R_gt"][i].T + host["t_gt"][i]
                ref = spatial.cKDTree(pe).query(pg, k=1)[0].mean() if sym else np.linalg.norm(pe - pg, axis=1).mean()
                worst = max(worst, abs(ref - ad[i]) / ref)
            row["host_ms_for_64_rows"] = (time.perf_counter() - t0) * 1e3 * N / len(rows)
            row["host_rows_timed"], row["worst_rel_diff_to_host"] = len(rows), worst
        except ImportError:
            pass
        res.append(row)
        print(json.dumps(row), flush=True)
    write_json(res)


if __name__ == "__main__":
    main()
