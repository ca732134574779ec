#!/usr/bin/env python3
"""Time gdrnet_amd.model_prep with HIP events: median of 20 calls after 5 warm-ups of each stage alone on uploaded tables, then ``prepare_models``
whole (upload, the three stages, the one read).  The workload is ``synth.make_model_prep_workload()``: 21 objects of 16 008 vertices and one of
259 854 (concentric perturbed icospheres: nothing is read from disk), K = 256 farthest-point-sampling (FPS) points per object.  Reported:
  bounds    one workgroup per object over its vertices;  GB/s over the vertex bytes
  fps       one workgroup per object, all 256 iterations in one launch: the 21 small objects run from registers, the large one from the workspace,
            and the launch lasts as long as the large one;  Mpoint-updates/s over sum(n) * K
  diameter  every vertex pair once, fp64;  Gpair/s
The reference's own code on the same clouds (its compiled FPS extension, ``misc.calc_pts_diameter``) is timed on the host by
``tests/golden/make_golden_g16.py --workload`` where the reference is present; this tool does not need it.
Usage:  timeout 600 python tools/model_prep_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import cabi, devargs, model_prep as MP, synth  # noqa: E402

K = 256


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    lib = cabi.load()
    clouds = synth.make_model_prep_workload()
    models = MP._Models(clouds, 0.0)
    tb = models.on(dev)
    C, n_max = models.num_classes, models.n_max
    npts = models.npts.astype(np.int64)
    ws = devargs.workspace(lib.gdrn_model_prep_workspace_bytes(C, n_max, K), dev, "model_prep_workspace_bytes")
    bounds, max_sq = torch.empty(C, 9, dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)
    idx, xyz = torch.empty(C, K, dtype=torch.int32, device=dev), torch.empty(C, K, 3, dtype=torch.float64, device=dev)
    st, p = devargs.stream(dev), cabi.ptr
    args = (p(tb["pts"]), p(tb["npts"]), models.npts.ctypes.data, C, n_max)
    res = []

    def report(call, fn, **rates):
        times = timed(fn)[1]
        ms = statistics.median(times)
        row = dict(call=call, objects=C, points=int(npts.sum()), n_max=n_max, K=K, gpu_ms_median=ms, gpu_ms_min=min(times), gpu_ms_max=max(times))
        row.update({k: v / ms / 1e6 for k, v in rates.items()})   # (per ms -> per s, in units of 1e9)
        res.append(row)
        print(json.dumps(row), flush=True)

    pairs = float((npts * (npts + 1) // 2).sum())
    report("bounds", lambda: cabi.check(lib.gdrn_model_bounds(*args, p(bounds), st), "model_bounds"), gb_per_s=float(npts.sum()) * 24)
    report("fps, K = 256", lambda: cabi.check(lib.gdrn_model_fps(*args, K, p(idx), p(xyz), p(ws), st), "model_fps"),
           gpoint_updates_per_s=float(npts.sum()) * K)
    report("diameter", lambda: cabi.check(lib.gdrn_model_diameter(*args, p(max_sq), st), "model_diameter"), gpairs_per_s=pairs)
    report("prepare_models, with the upload and the read", lambda: MP.prepare_models(clouds, device=dev))
    report("prepare_models without the diameters", lambda: MP.prepare_models(clouds, diameter=False, device=dev))
    prep = MP.prepare_models(clouds, device=dev)
    assert np.array_equal(prep.fps_indices, idx.cpu().numpy()) and np.array_equal(prep.max_sq_dist, max_sq.cpu().numpy())
    print(json.dumps(dict(diameters=[float(prep.diameters[0]), float(prep.diameters[-1])], first_indices=prep.fps_indices[-1, :4].tolist())), flush=True)
    write_json(res, workspace_bytes=int(ws.numel() * 8))


if __name__ == "__main__":
    main()
