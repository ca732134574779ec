#!/usr/bin/env python3
"""Time gdrnet_amd.pnp.pnp_ransac with HIP events: 64 RoIs x 4096 correspondences (fp32, 40 % outliers, inliers within a 1 px disc) x 100
hypotheses, median of 20 calls after 5 warm-ups, next to the host loop of the test helper on the same data (tests/pnp_host.py: one fp64
Gauss-Newton from the ground truth on the true inlier set + one brute-force inlier test per RoI -- the host does NOT draw or score hypotheses, so
its time is a floor of what a per-RoI host solver costs).  There is no earlier device path to compare with: reported, not gated.
Usage:  timeout 300 python tools/pnp_time.py [--json FILE]"""
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
import pnp_host as H  # noqa: E402
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import pnp, synth  # noqa: E402


def inputs(N=64, S=4096, seed=9):
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R = synth._random_rotations(seed, "R", N)
    t = np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)
    K = np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)
    X = 0.1 * u("X", N, S, 3) - 0.05
    p = (X @ R.transpose(0, 2, 1) + t[:, None]) @ K.transpose(0, 2, 1)
    uv = p[..., :2] / p[..., 2:3]
    good = u("out", N, S) >= 0.4
    ang, rad = 2 * np.pi * u("dir", N, S), u("rad", N, S)
    d = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    uv = uv + np.where(good[..., None], np.sqrt(rad)[..., None], (20.0 + 60.0 * rad)[..., None]) * d
    return dict(img=uv.astype(np.float32), mod=X.astype(np.float32), counts=np.full(N, S, dtype=np.int32), K=K, R=R, t=t, good=good)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, a = "cuda:0", inputs()
    img, mod, cnt, K = (torch.from_numpy(a[k]).to(dev) for k in ("img", "mod", "counts", "K"))
    out, times = timed(lambda: pnp.pnp_ransac(img, mod, cnt, K, reproj_err=3.0, iters=100, seed=0, want_mask=True))
    ok, mask = out["ok"].cpu().numpy(), out["inlier_mask"].cpu().numpy().astype(bool)
    Rg, tg = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    t0 = time.perf_counter()
    worst = 0.0
    for n in range(len(ok)):
        X, uv = a["mod"][n].astype(np.float64), a["img"][n].astype(np.float64)
        R, t, _ = H.gauss_newton(a["K"][n], X[a["good"][n]], uv[a["good"][n]], a["R"][n], a["t"][n])
        H.inliers(a["K"][n], R, t, X, uv, 3.0)
        worst = max(worst, H.rotation_angle(R, Rg[n]), np.linalg.norm(t - tg[n]) / np.linalg.norm(t))
    host_ms = (time.perf_counter() - t0) * 1e3
    row = dict(shape="64 RoIs x 4096 points x 100 hypotheses, fp32 correspondences", gpu_ms_median=statistics.median(times), gpu_ms_min=min(times),
               gpu_ms_max=max(times), host_ms_refine_only=host_ms, solved=int(ok.sum()), masks_equal_truth=bool((mask == a["good"]).all()),
               worst_deviation_from_host=worst)
    print(json.dumps(row), flush=True)
    write_json([row])


if __name__ == "__main__":
    main()
