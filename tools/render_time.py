#!/usr/bin/env python3
"""Time gdrnet_amd.render with HIP events: median of 20 calls after 5 warm-ups of render_depth and of xyz_from_depth, separately, for 64 instances
of a 20 480-face perturbed icosphere (subdivision 5) in 480 x 640 frames under random poses; milliseconds and Mpixel/s (frame pixels of the batch
per second).  Reported, not gated.  Usage:  timeout 300 python tools/render_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import render, synth  # noqa: E402


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, seed = "cuda:0", 64, 480, 640, 7
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    table = render.MeshTable([v], [f], device=dev)
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R = torch.from_numpy(synth._random_rotations(seed, "R", N)).to(dev)
    t = torch.from_numpy(np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)).to(dev)
    K = torch.from_numpy(np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)).to(dev)
    labels = np.zeros(N, dtype=np.int64)
    res = []
    depth, times = timed(lambda: render.render_depth(table, labels, R, t, K, H, W))
    covered = float((depth != 0).float().mean())
    for name, tm in (("render_depth", times), ("xyz_from_depth", timed(lambda: render.xyz_from_depth(depth, R, t, K))[1])):
        ms = statistics.median(tm)
        row = dict(call=name, N=N, faces=int(len(f)), H=H, W=W, covered_fraction=covered, gpu_ms_median=ms, gpu_ms_min=min(tm), gpu_ms_max=max(tm),
                   mpixel_per_s=N * H * W / ms / 1e3)
        res.append(row)
        print(json.dumps(row), flush=True)
    write_json(res)


if __name__ == "__main__":
    main()
