#!/usr/bin/env python3
"""Time gdrnet_amd.sixd_scores with HIP events on the workload of tools/bop_metrics_time.py -- 64 estimates, 16 384 points per class, 314 symmetry
transformations -- against the kernels that already do the same amount of work on the same tables, in the same process, calls interleaved
(A, B, A, B, ...: median of 20 each after 5 warm-ups each):
  ad_errors    against pose_metrics.pose_errors with every class marked symmetric   (the same nearest-neighbour pair count, N n^2)
  sym_errors   against bop_metrics.mssd_mspd                                        (the same posed-and-projected point count, N S n)
The existing kernel's own run-to-run spread (max - min of its 20 calls) is the yardstick for "not slower".  Rates: the adi loop issues 7 fp64 VALU
operations per point pair (3 subtractions, 1 multiplication, 2 fused multiply-adds, 1 minimum; 9 flops), reported against the 39.3e12 fp64 lane
operations/s of an MI355X (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 78.6 Tflop/s counting a fused multiply-add as two); the symmetric walk is
reported in posed-and-projected points per second.  For context the host loop of tests/sixd_host.py over 2 rows, scaled to 64.  Reported, not gated.
Usage:  timeout 600 python tools/sixd_scores_time.py [--json FILE]"""
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
import sixd_host as SH  # noqa: E402
from _timing import write_json  # noqa: E402
from bop_metrics_time import poses  # noqa: E402
from gdrnet_amd import bop_metrics as BM, pose_metrics as PM, sixd_scores as SS, synth  # noqa: E402

HOST_ROWS = 2
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9   # fp64 VALU operations per second of one MI355X


def interleaved(fa, fb, warmup=5, calls=20):
    """(last result of fa, of fb, HIP-event times [ms] of fa, of fb): fa and fb called in turn"""
    ta, tb, out = [], [], [None, None]
    for it in range(warmup + calls):
        for k, (fn, times) in enumerate(((fa, ta), (fb, tb))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[k] = fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times.append(e0.elapsed_time(e1))
    return out[0], out[1], ta, tb


def stats(times):
    return dict(gpu_ms_median=statistics.median(times), gpu_ms_min=min(times), gpu_ms_max=max(times))


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, n, seed, res = "cuda:0", 64, 16384, 7, []
    host = poses(N, seed)
    P = [torch.from_numpy(host[k]).to(dev) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    pts = [-0.1 + 0.2 * synth.hash_uniform(seed, f"pts{c}", (n, 3)) for c in range(4)]
    cont = BM.symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.01, -0.02, 0.0]}]})
    lab4 = np.arange(N) % 4
    table = BM.BopModelTable(pts, [0.2] * 4, [cont] * 4)
    all_sym = PM.ModelTable(pts, [0.2] * 4, None, (0, 1, 2, 3))
    S = int(table.s_max)

    ad, old, t_new, t_old = interleaved(lambda: SS.ad_errors(table, *P[:4], lab4), lambda: PM.pose_errors(all_sym, *P, lab4)["err"])
    assert torch.equal(ad[:, 1], old[:, 0]), "ad_errors' adi and pose_errors' ad of a symmetric class are the same bits"
    pairs = N * n * n
    new, ref = stats(t_new), stats(t_old)
    row = dict(call=f"ad_errors, {n} points (add and adi of every row)", N=N, points=n, **new, existing_call="pose_errors, every class symmetric (adi, re, te, proj)",
               **{f"existing_{k}": v for k, v in ref.items()}, existing_spread_ms=ref["gpu_ms_max"] - ref["gpu_ms_min"],
               slower_by_ms=new["gpu_ms_median"] - ref["gpu_ms_median"], pairs_per_s=pairs / new["gpu_ms_median"] * 1e3,
               fp64_valu_ops_per_s=7 * pairs / new["gpu_ms_median"] * 1e3, fraction_of_fp64_valu_peak=7 * pairs / new["gpu_ms_median"] * 1e3 / PEAK_LANE_OPS,
               existing_fraction_of_fp64_valu_peak=7 * pairs / ref["gpu_ms_median"] * 1e3 / PEAK_LANE_OPS)
    res.append(row)
    print(json.dumps(row), flush=True)

    sym, ms, t_new, t_old = interleaved(lambda: SS.sym_errors(table, *P, lab4), lambda: BM.mssd_mspd(table, *P, lab4))
    new, ref = stats(t_new), stats(t_old)
    row = dict(call=f"sym_errors, {n} points x {S} transformations", N=N, points=n, transformations=S, **new, existing_call="mssd_mspd",
               **{f"existing_{k}": v for k, v in ref.items()}, existing_spread_ms=ref["gpu_ms_max"] - ref["gpu_ms_min"],
               slower_by_ms=new["gpu_ms_median"] - ref["gpu_ms_median"], projected_points_per_s=N * S * n / new["gpu_ms_median"] * 1e3,
               existing_projected_points_per_s=N * S * n / ref["gpu_ms_median"] * 1e3)
    ad, sym = ad.cpu().numpy(), sym.cpu().numpy()
    inp = dict(host, points=pts, syms=[cont] * 4, labels=lab4)
    t0 = time.perf_counter()
    h_ad, h_sym = SH.errors_all(inp, range(HOST_ROWS))
    row["host_ms_for_64_rows"] = (time.perf_counter() - t0) * 1e3 * N / HOST_ROWS
    row["host_rows_timed"] = HOST_ROWS
    row["worst_abs_diff_to_host"] = dict(ad=float(np.abs(h_ad - ad[:HOST_ROWS]).max()), re_te_arp=[float(np.abs(h_sym[:, k] - sym[:HOST_ROWS, k]).max()) for k in range(3)])
    res.append(row)
    print(json.dumps(row), flush=True)

    rec = SS.ScoreRecall(table, ["a", "b", "c", "d"], (0, 1), 640)
    t_ad, t_sym = torch.from_numpy(ad).to(dev), torch.from_numpy(sym).to(dev)
    _, _, t_upd, _ = interleaved(lambda: rec.update(t_ad, t_sym, lab4), lambda: None)
    row = dict(call="ScoreRecall.update", N=N, **stats(t_upd))
    res.append(row)
    print(json.dumps(row), flush=True)
    write_json(res)


if __name__ == "__main__":
    main()
