"""Plain numpy restatement of the three BOP pose errors and of the recall counts behind AR, written from their definitions (Hodan et al., "BOP:
Benchmark for 6D Object Pose Estimation", ECCV 2018; the BOP Challenge 2019 MSSD / MSPD) with the reference's number formats: everything fp64, the
visibility difference of VSD on fp32 casts.  No reference import: this is the project's own host oracle for gdrnet_amd.bop_metrics, pinned to the
reference by golden G14 (tests/test_bop_metrics_cpu.py), and the host loop that tools/bop_metrics_time.py times for context."""
import numpy as np

import render_host as RH
from gdrnet_amd import synth

VSD_THS = np.arange(0.05, 0.51, 0.05)
MSSD_THS = np.arange(0.05, 0.51, 0.05)
MSPD_THS = np.arange(5, 51, 5)


def dist_image(depth, K):
    """distance from the camera centre of the surface point behind every pixel, 0 where depth is 0 (the skew term of K is not used)"""
    H, W = depth.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    X, Y = (xs - K[0, 2]) / np.float64(K[0, 0]), (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(X, depth) ** 2 + np.multiply(Y, depth) ** 2 + depth.astype(np.float64) ** 2)


def _visible(d_test, d_model, delta):
    d_diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    return np.logical_and(np.logical_or(d_diff <= delta, d_test == 0), d_model > 0), d_diff


def vsd(depth_est, depth_gt, depth_test, K, delta, taus, diameter, cost_type="step", normalized_by_diameter=True, stats=None):
    """(errors [T], counts [2+T] = |union|, |union| - |intersection|, step cost count per tau) of one estimate.  `stats` (a dict) receives
      delta_band   the smallest | |d_diff - delta| / dist_model | over the pixels whose visibility the comparison decides
      tau_band     the smallest |dists - tau| over the intersection and the taus"""
    d_test, d_gt, d_est = dist_image(depth_test, K), dist_image(depth_gt, K), dist_image(depth_est, K)
    vis_gt, diff_gt = _visible(d_test, d_gt, delta)
    vis_est, diff_est = _visible(d_test, d_est, delta)
    vis_est = np.logical_or(vis_est, np.logical_and(vis_gt, d_est > 0))
    inter, union = np.logical_and(vis_gt, vis_est), np.logical_or(vis_gt, vis_est)
    n_union = int(union.sum())
    comp = n_union - int(inter.sum())
    dists = np.abs(d_gt[inter] - d_est[inter])
    if normalized_by_diameter:
        dists = dists / diameter
    step = [int((dists >= tau).sum()) for tau in taus]
    if stats is not None:
        band = np.inf
        for diff, d_model in ((diff_gt, d_gt), (diff_est, d_est)):
            m = (d_model > 0) & (d_test != 0)
            if m.any():
                band = min(band, float(np.min(np.abs(diff[m].astype(np.float64) - delta) / d_model[m])))
        stats["delta_band"] = band
        stats["tau_band"] = float(min([np.min(np.abs(dists - tau)) for tau in taus])) if len(dists) else np.inf
    if n_union == 0:
        errs = [1.0] * len(taus)
    elif cost_type == "step":
        errs = [(s + comp) / float(n_union) for s in step]
    elif cost_type == "tlinear":
        errs = [(np.sum(np.minimum(dists / tau, 1.0)) + comp) / float(n_union) for tau in taus]
    else:
        raise ValueError(cost_type)
    return np.array(errs, dtype=np.float64), np.array([n_union, comp] + step, dtype=np.int64)


def mssd_mspd(R_est, t_est, R_gt, t_gt, K, pts, sym_R, sym_t):
    """(MSSD, MSPD, index of the transformation with the smallest MSSD) of one estimate"""
    def project(R, t):
        P = K @ np.hstack([R, t.reshape(3, 1)])
        im = P @ np.hstack([pts, np.ones((len(pts), 1))]).T
        return (im[:2] / im[2]).T

    est3, est2 = pts @ R_est.T + t_est, project(R_est, t_est)
    e3, e2 = [], []
    for S, ts in zip(sym_R, sym_t):
        R, t = R_gt @ S, R_gt @ ts + t_gt
        e3.append(np.sqrt(((est3 - (pts @ R.T + t)) ** 2).sum(1)).max())
        e2.append(np.sqrt(((est2 - project(R, t)) ** 2).sum(1)).max())
    return float(min(e3)), float(min(e2)), int(np.argmin(e3))


def recall_counts(vsd_err, ms_err, labels, diameters, im_width, num_classes, missing=None):
    """per-class hit counts under the ten thresholds of each error (strict <): hits_vsd [C,T,10], hits_mssd, hits_mspd [C,10], seen [C]"""
    vsd_err, ms_err, labels = np.asarray(vsd_err), np.asarray(ms_err), np.asarray(labels)
    C, T = num_classes, vsd_err.shape[1]
    out = dict(hits_vsd=np.zeros((C, T, 10), np.int64), hits_mssd=np.zeros((C, 10), np.int64), hits_mspd=np.zeros((C, 10), np.int64),
               seen=np.zeros(C, np.int64))
    factor = 640.0 / float(im_width)
    for i, c in enumerate(labels):
        out["hits_vsd"][c] += vsd_err[i][:, None] < VSD_THS[None, :]
        out["hits_mssd"][c] += ms_err[i, 0] / float(diameters[c]) < MSSD_THS
        out["hits_mspd"][c] += factor * ms_err[i, 1] < MSPD_THS
        out["seen"][c] += 1
    for c, n in (missing or {}).items():
        out["seen"][c] += n
    return out


def average_recall(counts, num_classes):
    """(per class {AR_VSD, AR_MSSD, AR_MSPD, AR} for the classes with targets, the same over all targets): recall = hits / targets per threshold
    (and tau), AR_x the mean of the recalls of x, AR the mean of the three"""
    def ar(hv, hs, hp, n):
        a = dict(AR_VSD=float(np.mean(hv / float(n))), AR_MSSD=float(np.mean(hs / float(n))), AR_MSPD=float(np.mean(hp / float(n))))
        a["AR"] = (a["AR_VSD"] + a["AR_MSSD"] + a["AR_MSPD"]) / 3.0
        return a

    per = {c: ar(counts["hits_vsd"][c], counts["hits_mssd"][c], counts["hits_mspd"][c], counts["seen"][c]) for c in range(num_classes)
           if counts["seen"][c] > 0}
    return per, ar(counts["hits_vsd"].sum(0), counts["hits_mssd"].sum(0), counts["hits_mspd"].sum(0), counts["seen"].sum())


_scenes = {}


def vsd_scene(seed=None, stats=None):
    """(inputs, depth_est, depth_gt [N,H,W], depth_test [F,H,W], all fp32) of synth.make_bop_metric_inputs("vsd"), rendered by the host rasterizer;
    computed once per process and seed.  `stats` receives the rasterizer's edge_band over the 2N renders."""
    if seed not in _scenes:
        inp = synth.make_bop_metric_inputs("vsd", seed=seed)
        est, gt, band = [], [], np.inf
        for i, c in enumerate(inp["labels"]):
            for out, R, t in ((est, inp["R_est"][i], inp["t_est"][i]), (gt, inp["R_gt"][i], inp["t_gt"][i])):
                s = {}
                out.append(RH.render_one(inp["vertices"][c], inp["faces"][c], R, t, inp["K"][i], inp["H"], inp["W"], inp["near"], inp["far"], s))
                band = min(band, s["edge_band"])
        est, gt = np.stack(est), np.stack(gt)
        _scenes[seed] = (inp, est, gt, synth.bop_test_depth(inp, gt), band)
    if stats is not None:
        stats["edge_band"] = _scenes[seed][4]
    return _scenes[seed][:4]


def vsd_all(scene, cost_type="step", stats=None):
    """(err [N,T], counts [N,2+T]) of a vsd_scene; `stats` receives the minima of the bands over the rows"""
    inp, est, gt, test = scene
    errs, counts, bands = [], [], []
    for i in range(len(inp["labels"])):
        s = {}
        e, c = vsd(est[i], gt[i], test[inp["frame"][i]], inp["K"][i], inp["delta"], inp["taus"], inp["diameters"][inp["labels"][i]], cost_type, True, s)
        errs.append(e)
        counts.append(c)
        bands.append(s)
    if stats is not None:
        for k in ("delta_band", "tau_band"):
            stats[k] = min(b[k] for b in bands)
    return np.stack(errs), np.stack(counts)


def mssd_mspd_all(inp):
    """(err [N,2], best transformation [N]) of synth.make_bop_metric_inputs("sym")"""
    ident = (np.eye(3)[None], np.zeros((1, 3)))
    out = []
    for i, c in enumerate(inp["labels"]):
        S = inp["syms"][c] or ident
        out.append(mssd_mspd(inp["R_est"][i], inp["t_est"][i], inp["R_gt"][i], inp["t_gt"][i], inp["K"][i], inp["points"][c], S[0], S[1]))
    return np.array([o[:2] for o in out]), np.array([o[2] for o in out])
