#!/usr/bin/env python3
"""Generate golden G18 (``g18_sixd_scores.npz``) by running the REFERENCE's pose errors, matching and recall on the fixture of
``synth.make_sixd_score_inputs``.

Runs only where the reference checkout is present (see make_golden.py); only the input's seed and the reference's outputs are stored.  The
reference works in millimetres: points, translations and the model infos are scaled by 1000 on the way in, and its outputs are stored as it
returns them (mm, degrees, pixels).
  err      per row the reference's own ``pose_error.add``, ``adi``, ``re_sym``, ``te_sym``, ``arp_2d_sym`` (lib/pysixd/pose_error.py:184-234,297-337)
           with the sets of ``misc.get_symmetry_transformations``, called as eval_calc_errors.py:395-448 calls them
  match    per row, type and threshold of eval_pose_results_more.py:64-93 (the 51 columns of ``columns``) whether ``pose_matching.match_poses``
           matches the estimate to its target, on the error lists eval_calc_errors.py builds (mm / 10 where it divides) normalised as
           eval_calc_scores.py:238-250 normalises them
  recall   per object and column ``score.calc_recall`` of the matches over the object's targets (its rows and its targets without an estimate)
A seed is passed over for the next one -- which must then be recorded in ``synth.SIXD_SCORE_SEEDS`` -- while an error, normalised as above, is
within 1e-6 (relative) of one of its thresholds (G14's rule (c)): every decision is then the reference's alone, and no row is left out of any
comparison.

Usage:  python tests/golden/make_golden_g18.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims  # noqa: E402

TH_BAND = 1e-6
AUC_THS = [[th] for th in np.linspace(10 / 10, 10, num=10)]
# (type, correct_th) of eval_pose_results_more.py:64-93 in the column order of the device counters
TYPES = (("AUCadd", AUC_THS), ("AUCadi", AUC_THS), ("AUCad", AUC_THS), ("ABSadd", [[2]]), ("ABSadi", [[2]]), ("ABSad", [[2]]),
         ("add", [[th] for th in [0.02, 0.05, 0.1]]), ("adi", [[th] for th in [0.02, 0.05, 0.1]]), ("reS", [[th] for th in [2, 5, 10]]),
         ("teS", [[th] for th in [2, 5, 10]]), ("reteS", [[2, 2], [5, 5], [10, 10]]), ("projS", [[th] for th in [2, 5, 10]]))
NORMALIZED_BY_DIAMETER = ["ad", "add", "adi", "mssd"]   # eval_calc_scores.py:70


def model_info_mm(info):
    out = {"diameter": 1000.0 * info["diameter"]}
    if "symmetries_discrete" in info:
        out["symmetries_discrete"] = []
        for sym in info["symmetries_discrete"]:
            m = np.reshape(sym, (4, 4)).astype(np.float64)
            m[:3, 3] *= 1000.0
            out["symmetries_discrete"].append(m.ravel().tolist())
    if "symmetries_continuous" in info:
        out["symmetries_continuous"] = [{"axis": s["axis"], "offset": [1000.0 * o for o in s["offset"]]} for s in info["symmetries_continuous"]]
    return out


def error_list(name, e, is_sym_obj):
    """the list eval_calc_errors.py:395-448 stores for an estimate under error type `name`; e = (add, adi, re_sym, te_sym, arp_2d_sym) in mm"""
    add, adi, re_s, te_s, pr_s = e
    if name in ("AUCad", "ABSad"):
        return [(adi if is_sym_obj else add) / 10]
    if name in ("AUCadd", "ABSadd"):
        return [add / 10]
    if name in ("AUCadi", "ABSadi"):
        return [adi / 10]
    return {"add": [add], "adi": [adi], "reS": [re_s], "teS": [te_s / 10], "reteS": [re_s, te_s / 10], "projS": [pr_s]}[name]


def main():
    install_shims()
    from lib.pysixd import misc, pose_matching, score
    from lib.pysixd import pose_error as PE

    from gdrnet_amd import synth

    seed = synth.SIXD_SCORE_SEEDS["sym"]
    while True:
        inp = synth.make_sixd_score_inputs("sym", seed=seed)
        infos = [model_info_mm(m) for m in inp["model_infos"]]
        sets = [misc.get_symmetry_transformations(m, 0.01) for m in infos]
        pts = [1000.0 * p for p in inp["points"]]
        N, C = len(inp["labels"]), len(pts)
        err = np.zeros((N, 5))
        for i in range(N):
            c = int(inp["labels"][i])
            Re, te, Rg, tg = inp["R_est"][i], 1000.0 * inp["t_est"][i].reshape(3, 1), inp["R_gt"][i], 1000.0 * inp["t_gt"][i].reshape(3, 1)
            err[i] = (PE.add(Re, te, Rg, tg, pts[c]), PE.adi(Re, te, Rg, tg, pts[c]), PE.re_sym(Re, Rg, syms=sets[c]),
                      PE.te_sym(te, tg, R_gt=Rg, syms=sets[c]), PE.arp_2d_sym(Re, te, Rg, tg, pts=pts[c], K=inp["K"][i], syms=sets[c]))
        match, columns, clear = [], [], True
        for name, correct_th in TYPES:
            lists = []
            for i in range(N):
                c = int(inp["labels"][i])
                e = error_list(name, err[i], c in inp["sym_classes"])
                if name in NORMALIZED_BY_DIAMETER:
                    e = [x / float(infos[c]["diameter"]) for x in e]
                lists.append(e)
            for th in correct_th:
                columns.append(f"{name}:{'-'.join(str(float(t)) for t in th)}")
                col = []
                for i in range(N):
                    ms = pose_matching.match_poses([{"est_id": 0, "score": 1.0, "errors": {0: lists[i]}}], th, 1, [True])
                    col.append(len(ms) == 1 and ms[0]["gt_id"] == 0)
                    clear = clear and all(abs(x - t) > TH_BAND * t for x, t in zip(lists[i], th))
                match.append(col)
        if clear:
            break
        print(f"sym: seed {seed} puts an error on a threshold, trying the next one")
        seed += 1
    assert seed == synth.SIXD_SCORE_SEEDS["sym"], f"record seed {seed} for case sym in synth.SIXD_SCORE_SEEDS"
    match = np.array(match, dtype=bool).T
    targets = [int((inp["labels"] == c).sum()) + inp["missing"].get(c, 0) for c in range(C)]
    recall = np.array([[score.calc_recall(int(match[inp["labels"] == c, k].sum()), targets[c]) for k in range(match.shape[1])] for c in range(C)])
    g = {"sym/seed": np.array(seed), "sym/err": err, "sym/match": match, "sym/recall": recall, "sym/columns": np.array(columns),
         "sym/targets": np.array(targets)}
    print(f"sym: seed {seed}, N = {N}, sets {[len(s) for s in sets]}, add {err[:, 0].min():.3g}..{err[:, 0].max():.3g} mm, adi "
          f"{err[:, 1].min():.3g}..{err[:, 1].max():.3g} mm, re_sym {err[:, 2].min():.3g}..{err[:, 2].max():.3g} deg, te_sym "
          f"{err[:, 3].min():.3g}..{err[:, 3].max():.3g} mm, arp_2d_sym {err[:, 4].min():.3g}..{err[:, 4].max():.3g} px")
    print("matches per column:", dict(zip(columns, match.sum(0).tolist())))
    out = os.path.join(HERE, "g18_sixd_scores.npz")
    np.savez_compressed(out, **g)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
