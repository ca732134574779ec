#!/usr/bin/env python3
"""Generate golden G14 (``g14_bop_metrics.npz``) by running the REFERENCE's BOP pose errors on the fixtures of ``synth.make_bop_metric_inputs``.

Runs only where the reference checkout is present (see make_golden.py); only the inputs' seeds and its outputs are stored.
  "vsd"  per row the reference's own ``pose_error.vsd`` (lib/pysixd/pose_error.py:22-128), cost types step and tlinear, with a stub ``renderer``
         whose ``render_object`` returns the host rasterizer's fp32 depth (tests/render_host.py -- the bits gdrn_render_depth writes), and the three
         integer counts behind it (|union|, |union| - |intersection|, the step cost count per tau) from the reference's
         ``misc.depth_im_to_dist_im_fast`` and ``visibility.estimate_visib_mask_gt`` / ``_est``, chained exactly as ``vsd`` chains them.
  "sym"  per row ``pose_error.mssd`` and ``pose_error.mspd`` with the sets of ``misc.get_symmetry_transformations`` (stored too).
A seed is passed over for the next one -- which must then be recorded in ``synth.BOP_METRIC_SEEDS`` -- while
  (a) a pixel's fp32 visibility difference is within 2^-20 dist of delta (8 fp32 ulps: an fp64 sqrt one ulp off may move the fp32 cast by one),
  (b) a pixel's normalised distance is within 1e-9 of a tau,
  (c) an error, normalised as eval_calc_scores.py:239-250 does, is within 1e-6 (relative) of one of its recall thresholds, or
  (d) a pixel centre of a render is within 1e-6 px of a triangle edge (the G13 rule):
the decisions are then the reference's alone, and no row is left out of any comparison.

Usage:  python tests/golden/make_golden_g14.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims  # noqa: E402

DELTA_BAND, TAU_BAND, TH_BAND, EDGE_BAND = 2.0 ** -20, 1e-9, 1e-6, 1e-6
VSD_THS, MSPD_THS = np.arange(0.05, 0.51, 0.05), np.arange(5, 51, 5)


def clear_of(values, ths, rel=TH_BAND):
    values = np.asarray(values, dtype=np.float64).reshape(-1, 1)
    return bool(np.all(np.abs(values - ths[None, :]) > rel * ths[None, :]))


class HostRenderer:
    """the ``renderer`` argument of pose_error.vsd: ``render_object(obj_id, R, t, fx, fy, cx, cy)["depth"]`` from the host rasterizer"""

    def __init__(self, inp, RH):
        self.inp, self.RH = inp, RH

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        inp = self.inp
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        return {"depth": self.RH.render_one(inp["vertices"][obj_id], inp["faces"][obj_id], R, np.asarray(t).reshape(3), K, inp["H"], inp["W"],
                                            inp["near"], inp["far"])}


def reference_vsd(scene, PE, misc, visibility, RH):
    inp, est, gt, test = scene
    ren = HostRenderer(inp, RH)
    N, T = len(inp["labels"]), len(inp["taus"])
    err = {"step": np.zeros((N, T)), "tlinear": np.zeros((N, T))}
    counts = np.zeros((N, 2 + T), dtype=np.int64)
    for i in range(N):
        c, K, dt = int(inp["labels"][i]), inp["K"][i], test[inp["frame"][i]]
        for cost in err:
            err[cost][i] = PE.vsd(inp["R_est"][i], inp["t_est"][i].reshape(3, 1), inp["R_gt"][i], inp["t_gt"][i].reshape(3, 1), dt, K, inp["delta"],
                                  list(inp["taus"]), True, inp["diameters"][c], ren, c, cost_type=cost)
        # the counts behind the step error, by the reference's own functions on the same renders (pose_error.py:85-107)
        assert np.array_equal(ren.render_object(c, inp["R_gt"][i], inp["t_gt"][i], K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"], gt[i])
        d_test, d_gt, d_est = (misc.depth_im_to_dist_im_fast(d, K) for d in (dt, gt[i], est[i]))
        v_gt = visibility.estimate_visib_mask_gt(d_test, d_gt, inp["delta"], visib_mode="bop19")
        v_est = visibility.estimate_visib_mask_est(d_test, d_est, v_gt, inp["delta"], visib_mode="bop19")
        inter, union = np.logical_and(v_gt, v_est), np.logical_or(v_gt, v_est)
        dists = np.abs(d_gt[inter] - d_est[inter]) / inp["diameters"][c]
        counts[i] = [union.sum(), union.sum() - inter.sum()] + [(dists >= tau).sum() for tau in inp["taus"]]
        if counts[i, 0] > 0:
            assert np.array_equal(err["step"][i], (counts[i, 2:] + counts[i, 1]) / float(counts[i, 0]))
    return err, counts


def main():
    install_shims()
    from lib.pysixd import misc, visibility
    from lib.pysixd import pose_error as PE

    import bop_host as BH
    import render_host as RH
    from gdrnet_amd import synth

    g = {}
    seed = synth.BOP_METRIC_SEEDS["vsd"]
    while True:
        stats = {}
        scene = BH.vsd_scene(seed, stats)
        for cost in ("step", "tlinear"):
            BH.vsd_all(scene, cost, stats)
        err, counts = reference_vsd(scene, PE, misc, visibility, RH)
        ok = stats["delta_band"] > DELTA_BAND and stats["tau_band"] > TAU_BAND and stats["edge_band"] > EDGE_BAND and clear_of(err["step"], VSD_THS)
        if ok:
            break
        print(f"vsd: seed {seed} sits on a decision ({stats}), trying the next one")
        seed += 1
    assert seed == synth.BOP_METRIC_SEEDS["vsd"], f"record seed {seed} for case vsd in synth.BOP_METRIC_SEEDS"
    g["vsd/seed"], g["vsd/err_step"], g["vsd/err_tlinear"], g["vsd/counts"] = np.array(seed), err["step"], err["tlinear"], counts
    print(f"vsd: seed {seed}, bands {stats}\n  union / comp {counts[:, :2].tolist()}\n  step errors\n{np.round(err['step'], 3)}")

    seed = synth.BOP_METRIC_SEEDS["sym"]
    while True:
        inp = synth.make_bop_metric_inputs("sym", seed=seed)
        ref_sets = [misc.get_symmetry_transformations(m, 0.01) for m in inp["model_infos"]]
        N = len(inp["labels"])
        e = np.zeros((N, 2))
        for i in range(N):
            c = int(inp["labels"][i])
            Re, te, Rg, tg = inp["R_est"][i], inp["t_est"][i].reshape(3, 1), inp["R_gt"][i], inp["t_gt"][i].reshape(3, 1)
            e[i] = PE.mssd(Re, te, Rg, tg, inp["points"][c], ref_sets[c]), PE.mspd(Re, te, Rg, tg, inp["K"][i], inp["points"][c], ref_sets[c])
        d = inp["diameters"][inp["labels"]]
        if clear_of(e[:, 0] / d, VSD_THS) and clear_of(e[:, 1] * (640.0 / inp["im_width"]), MSPD_THS):
            break
        print(f"sym: seed {seed} puts an error on a recall threshold, trying the next one")
        seed += 1
    assert seed == synth.BOP_METRIC_SEEDS["sym"], f"record seed {seed} for case sym in synth.BOP_METRIC_SEEDS"
    g["sym/seed"], g["sym/err"] = np.array(seed), e
    for c, s in enumerate(ref_sets):
        g[f"sym/R{c}"], g[f"sym/t{c}"] = np.stack([x["R"] for x in s]), np.stack([np.asarray(x["t"], dtype=np.float64).reshape(3) for x in s])
    print(f"sym: seed {seed}, N = {N}, sets {[len(s) for s in ref_sets]}, mssd / d {np.min(e[:, 0] / d):.3g}..{np.max(e[:, 0] / d):.3g}, "
          f"mspd {e[:, 1].min():.3g}..{e[:, 1].max():.3g}")
    out = os.path.join(HERE, "g14_bop_metrics.npz")
    np.savez_compressed(out, **g)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
