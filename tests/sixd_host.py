"""Plain numpy restatement of the errors, decisions and tables behind the reference's YCB-V scores, written from their definitions (Hinterstoisser et
al., ACCV 2012: ADD / ADD-S; Xiang et al., "PoseCNN", RSS 2018: the 2 cm and 10 cm thresholds; the symmetry-aware minimum over a set of
transformations of the BOP Challenge 2019) with the reference's number format: everything fp64.  No reference import: this is the project's own host
oracle for gdrnet_amd.sixd_scores, pinned to the reference by golden G18 (tests/test_sixd_scores_cpu.py), and the host loop that
tools/sixd_scores_time.py times for context.  Lengths in metres."""
import numpy as np

# (type, thresholds) in the column order of the device counters; AUC* / ABS* / teS thresholds are centimetres, add / adi fractions of the diameter
TYPES = (("AUCadd", list(np.linspace(1, 10, 10))), ("AUCadi", list(np.linspace(1, 10, 10))), ("AUCad", list(np.linspace(1, 10, 10))),
         ("ABSadd", [2]), ("ABSadi", [2]), ("ABSad", [2]), ("add", [0.02, 0.05, 0.1]), ("adi", [0.02, 0.05, 0.1]),
         ("reS", [2, 5, 10]), ("teS", [2, 5, 10]), ("reteS", [2, 5, 10]), ("projS", [2, 5, 10]))
AUC = ("AUCadd", "AUCadi", "AUCad")
NFLAGS = sum(len(t) for _, t in TYPES)
IDENT = (np.eye(3)[None], np.zeros((1, 3)))


def add_adi(R_est, t_est, R_gt, t_gt, pts, chunk=256):
    """(add, adi) of one estimate: the mean distance of corresponding points | from each ground-truth-posed point to the nearest estimate-posed one
    (brute force over all pairs, in chunks of ground-truth points)"""
    pe, pg = pts @ R_est.T + t_est, pts @ R_gt.T + t_gt
    add = float(np.sqrt(((pe - pg) ** 2).sum(1)).mean())
    near = np.empty(len(pts))
    for i in range(0, len(pts), chunk):
        g = pg[i : i + chunk]
        d2 = (g[:, 0:1] - pe[None, :, 0]) ** 2
        d2 += (g[:, 1:2] - pe[None, :, 1]) ** 2
        d2 += (g[:, 2:3] - pe[None, :, 2]) ** 2
        near[i : i + chunk] = np.sqrt(d2.min(axis=1))
    return add, float(near.mean())


def _pixels(pts, R, t, K):
    cam = K @ (R @ pts.T + t.reshape(3, 1))
    return (cam[:2] / cam[2]).T


def sym_errors(R_est, t_est, R_gt, t_gt, K, pts, sym_R, sym_t):
    """(re_sym [deg], te_sym, arp_2d_sym [px]) of one estimate: each the minimum over the transformations (R_gt S, R_gt t_S + t_gt); te_sym is
    the Frobenius norm of M[i][j] = (R_gt t_S)[i] + t_gt[j] - t_est[j], the value the reference's function returns, not a distance"""
    est2 = _pixels(pts, R_est, t_est, K)
    re, te, pr = [], [], []
    for S, ts in zip(sym_R, sym_t):
        R, t = R_gt @ S, R_gt @ ts + t_gt
        tr = min(np.trace(R_est @ R.T), 3.0)
        re.append(np.rad2deg(np.arccos(min(1.0, max(-1.0, 0.5 * (tr - 1.0))))))
        # te_sym as the reference runs it: its t_gt is flattened, its R_gt t_S a column, and their sum broadcasts to 3 x 3 (sixd_scores.sym_errors)
        te.append(np.sqrt((((R_gt @ ts)[:, None] + t_gt[None, :] - t_est[None, :]) ** 2).sum()))
        pr.append(np.sqrt(((est2 - _pixels(pts, R, t, K)) ** 2).sum(1)).mean())
    return float(min(re)), float(min(te)), float(min(pr))


def errors_all(inp, rows=None):
    """(ad [N,2], sym [N,3]) of the rows of a synth.make_sixd_score_inputs-shaped dict (points, syms, labels, poses, K)"""
    rows = range(len(inp["labels"])) if rows is None else rows
    ad, sym = [], []
    for i in rows:
        c = int(inp["labels"][i])
        S = inp["syms"][c] if inp.get("syms") is not None and inp["syms"][c] is not None else IDENT
        K = inp["K"][i] if np.ndim(inp["K"]) == 3 else inp["K"]
        ad.append(add_adi(inp["R_est"][i], inp["t_est"][i], inp["R_gt"][i], inp["t_gt"][i], inp["points"][c]))
        sym.append(sym_errors(inp["R_est"][i], inp["t_est"][i], inp["R_gt"][i], inp["t_gt"][i], K, inp["points"][c], S[0], S[1]))
    return np.array(ad, dtype=np.float64).reshape(-1, 2), np.array(sym, dtype=np.float64).reshape(-1, 3)


def check_errors(ad, sym, ref, what, mm=1000.0):
    """the bounds of tests/test_pose_metrics_gpu.py (add / adi: 1e-9 relative + 1e-12; re: 1e-9 relative from 0.1 degree, 1e-5 degree absolute below) and
    of tests/test_bop_metrics_gpu.py for the symmetric pose walk (a distance in space 1e-13 m, in the image 1e-10 px), on the reference's
    millimetres (``ref`` [N,5] = golden G18's add, adi, re_sym, te_sym, arp_2d_sym) as metres -- or, with ``mm`` = 1, on this
    module's own metres; prints the measured deviations"""
    ref_ad, ref_re, ref_te, ref_pr = ref[:, :2] / mm, ref[:, 2], ref[:, 3] / mm, ref[:, 4]
    d_ad = np.abs(ad - ref_ad)
    d_re, d_te, d_pr = np.abs(sym[:, 0] - ref_re), np.abs(sym[:, 1] - ref_te), np.abs(sym[:, 2] - ref_pr)
    big = ref_re >= 0.1
    print(f"{what}: add / adi worst |got - ref| {d_ad.max():.3e} m, worst relative {np.max(d_ad / np.maximum(ref_ad, 1e-300)):.3e} (bound 1e-9 + 1e-12); "
          f"re_sym worst relative {np.max(d_re[big] / ref_re[big], initial=0.0):.3e} on {int(big.sum())} rows (1e-9), worst absolute {np.max(d_re[~big], initial=0.0):.3e} deg on "
          f"{int((~big).sum())} near-zero rows (1e-5); te_sym worst {d_te.max():.3e} m (1e-13); arp_2d_sym worst {d_pr.max():.3e} px (1e-10)")
    assert ad.shape == (len(ref), 2) and sym.shape == (len(ref), 3) and np.isfinite(ad).all() and np.isfinite(sym).all()
    assert np.all(d_ad <= 1e-9 * ref_ad + 1e-12), what
    assert np.all(d_re[big] <= 1e-9 * ref_re[big]) and np.all(d_re[~big] <= 1e-5), what
    assert np.all(d_te <= 1e-13) and np.all(d_pr <= 1e-10), what


def flags(ad, sym, labels, diameters, sym_classes):
    """[N,51] bool: the strict-< decision of every (type, threshold), in the column order of TYPES"""
    ad, sym, labels = np.asarray(ad).reshape(-1, 2), np.asarray(sym).reshape(-1, 3), np.asarray(labels, dtype=np.int64).reshape(-1)
    d = np.asarray(diameters, dtype=np.float64)[labels]
    is_adi = np.isin(labels, list(sym_classes))
    cm = {"add": ad[:, 0] * 100.0, "adi": ad[:, 1] * 100.0, "ad": np.where(is_adi, ad[:, 1], ad[:, 0]) * 100.0}
    re, te_cm, pr = sym[:, 0], sym[:, 1] * 100.0, sym[:, 2]
    cols = []
    for name, ths in TYPES:
        for th in ths:
            if name[:3] in ("AUC", "ABS"):
                cols.append(cm[name[3:]] < th)
            elif name in ("add", "adi"):
                cols.append(ad[:, 0 if name == "add" else 1] / d < th)
            elif name == "reS":
                cols.append(re < th)
            elif name == "teS":
                cols.append(te_cm < th)
            elif name == "reteS":
                cols.append((re < th) & (te_cm < th))
            else:
                cols.append(pr < th)
    return np.stack(cols, axis=1).reshape(len(labels), NFLAGS)


def recall_counts(ad, sym, labels, diameters, sym_classes, num_classes, missing=None):
    """dict(hits [C,51], seen [C]) int64; `missing`: class -> targets without an estimate"""
    fl, labels = flags(ad, sym, labels, diameters, sym_classes), np.asarray(labels, dtype=np.int64).reshape(-1)
    hits, seen = np.zeros((num_classes, NFLAGS), np.int64), np.zeros(num_classes, np.int64)
    for c in range(num_classes):
        hits[c], seen[c] = fl[labels == c].sum(0), (labels == c).sum()
    for c, n in (missing or {}).items():
        seen[c] += n
    return dict(hits=hits, seen=seen)


def _thr_str(th):
    return str(int(th)) if float(th) == int(th) else f"{th:.3f}"


def tables(obj_names, hits, seen):
    """type -> rows of strings: one row per object with a target, in class order, one column per threshold -- one column, the mean of the ten
    recalls, for an AUC type -- and the row of the means over the objects: always for an AUC type, otherwise for more than one object"""
    out, col = {}, 0
    objs = [c for c in range(len(obj_names)) if seen[c] > 0]
    for name, ths in TYPES:
        rec = [[hits[c][col + k] / float(seen[c]) for k in range(len(ths))] for c in objs]
        col += len(ths)
        if name in AUC:
            rec, head = [[float(np.mean(r))] for r in rec], [f"{name}_{_thr_str(ths[-1])}"]
        else:
            head = [f"{name}_{_thr_str(th)}" for th in ths]
        rows = [["objects"] + head] + [[obj_names[c]] + [f"{100 * r:.2f}" for r in rec[j]] for j, c in enumerate(objs)]
        if len(objs) > 1 or (name in AUC and len(objs) == 1):
            rows.append([f"Avg({len(objs)})"] + [f"{100 * np.mean([r[k] for r in rec]):.2f}" for k in range(len(head))])
        out[name] = rows
    return out


def top_estimates(keys, scores, inst_count=1):
    """indices the toolkit would score: per key the inst_count best scores, the earlier estimate first among equals; keys by first appearance"""
    seen_keys, out = [], []
    for k in keys:
        if k not in seen_keys:
            seen_keys.append(k)
    for k in seen_keys:
        idx = [i for i, kk in enumerate(keys) if kk == k]
        idx.sort(key=lambda i: (-scores[i], i))
        out += idx[:inst_count]
    return out
