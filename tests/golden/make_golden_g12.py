#!/usr/bin/env python3
"""Generate golden G12 (``g12_pose_metrics.npz``) by running the REFERENCE's pose-error functions and evaluator.

Runs only where the reference checkout is present (see make_golden.py); only its outputs are stored.  Per row of
``synth.make_pose_metric_inputs`` the reference's own ``te`` / ``re`` / ``add`` / ``adi`` / ``arp_2d`` (lib/pysixd/pose_error.py) and
``get_closest_rot`` (core/utils/pose_utils.py) are called exactly as ``_eval_predictions`` chains them, and ``_eval_predictions`` itself
(core/gdrn_modeling/gdrn_custom_evaluator.py:493-670) runs on a bare evaluator instance for the recall table (``big_tab``, caught on its way
into ``tabulate``).  A draw in which a reference error sits within 1e-6 (relative) of one of the thresholds, or a table cell within 1e-6 of
a rounding boundary of its two decimals, is discarded for the next seed: the flags and the cells are then decided by the reference alone.

Usage:  python tests/golden/make_golden_g12.py
"""
import os
import sys
import tempfile
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims  # noqa: E402

METRICS = ("ad_2", "ad_5", "ad_10", "rete_2", "rete_5", "rete_10", "re_2", "re_5", "re_10", "te_2", "te_5", "te_10", "proj_2", "proj_5", "proj_10")


def reference_errors(inp, PE, get_closest_rot):
    N = len(inp["labels"])
    err = np.zeros((N, 4))
    for i in range(N):
        c = int(inp["labels"][i])
        Re, te_, Rg, tg, K, pts = inp["R_est"][i], inp["t_est"][i], inp["R_gt"][i], inp["t_gt"][i], inp["K"][i], inp["points"][c]
        if c in inp["sym_classes"]:
            Rs = get_closest_rot(Re, Rg, inp["sym_infos"][c])
            err[i] = PE.adi(Re, te_, Rg, tg, pts=pts), PE.re(Re, Rs), PE.te(te_, tg), PE.arp_2d(Re, te_, Rs, tg, pts=pts, K=K)
        else:
            err[i] = PE.add(Re, te_, Rg, tg, pts=pts), PE.re(Re, Rg), PE.te(te_, tg), PE.arp_2d(Re, te_, Rg, tg, pts=pts, K=K)
    return err


def thresholds_clear(err, inp, rel=1e-6):
    """no error within `rel` of a threshold it is compared with; for case A also: every flag has rows on both sides"""
    d = inp["diameters"][inp["labels"]]
    pairs = [(err[:, 0], f * d) for f in (0.02, 0.05, 0.1)] + [(err[:, 1], np.full(len(d), v)) for v in (2.0, 5.0, 10.0)]
    pairs += [(err[:, 2], np.full(len(d), v)) for v in (0.02, 0.05, 0.1)] + [(err[:, 3], np.full(len(d), v)) for v in (2.0, 5.0, 10.0)]
    return all(np.all(np.abs(e - t) > rel * t) for e, t in pairs)


def flags(err, inp):
    d = inp["diameters"][inp["labels"]]
    ad, re_, te_, pr = err.T
    cols = [ad < 0.02 * d, ad < 0.05 * d, ad < 0.1 * d, (re_ < 2) & (te_ < 0.02), (re_ < 5) & (te_ < 0.05), (re_ < 10) & (te_ < 0.1),
            re_ < 2, re_ < 5, re_ < 10, te_ < 0.02, te_ < 0.05, te_ < 0.1, pr < 2, pr < 5, pr < 10]
    return np.stack(cols, axis=1)


def reference_table(inp, EV):
    """_eval_predictions on a bare instance: rows of big_tab (every cell as a string)"""
    names = inp["obj_names"]
    ev = object.__new__(EV.GDRN_EvaluatorCustom)
    ev.cfg = types.SimpleNamespace(EXP_ID="g12", DATASETS=types.SimpleNamespace(SYM_OBJS=[names[c] for c in inp["sym_classes"]]))
    ev.obj_names, ev.diameters = names, list(inp["diameters"])
    ev.models_3d = [{"pts": p} for p in inp["points"]]
    ev._metadata = types.SimpleNamespace(sym_infos=inp["sym_infos"])
    ev.gts, ev._predictions = OrderedDict(), OrderedDict()
    for c, name in enumerate(names):
        ev.gts[name], ev._predictions[name] = OrderedDict(), OrderedDict()
    for i, c in enumerate(inp["labels"]):
        name, f = names[int(c)], f"{i:06d}"
        ev.gts[name][f] = {"R": inp["R_gt"][i], "t": inp["t_gt"][i], "K": inp["K"][i]}
        ev._predictions[name][f] = {"R": inp["R_est"][i], "t": inp["t_est"][i]}
    for c, cnt in inp["missing"].items():
        for j in range(cnt):
            ev.gts[names[c]][f"missing_{j:03d}"] = {"R": np.eye(3), "t": np.zeros(3), "K": inp["K"][0]}
    ev.get_gts = lambda: None
    ev.dataset_name, ev.use_cache, ev._distributed = "synth", False, False
    ev._logger = types.SimpleNamespace(info=lambda *a, **k: None, warning=lambda *a, **k: None)
    caught = []
    real_tabulate = EV.tabulate

    def catching_tabulate(tab, *a, **k):
        caught.append([[str(x) for x in row] for row in tab])
        return real_tabulate(tab, *a, **k) if callable(real_tabulate) else ""

    EV.tabulate = catching_tabulate
    try:
        with tempfile.TemporaryDirectory() as tmp:
            ev._output_dir = tmp
            ev._eval_predictions()
            assert os.path.exists(os.path.join(tmp, "g12_synth_tab.txt"))
    finally:
        EV.tabulate = real_tabulate
    assert len(caught) == 1
    return caught[0]


def main():
    install_shims()
    import numpy.lib.npyio as npyio

    if not hasattr(npyio, "save"):
        npyio.save = np.save   # (NumPy 2 moved it; the evaluator module's import chain reads it)
    import core.gdrn_modeling.gdrn_custom_evaluator as EV
    from core.utils.pose_utils import get_closest_rot
    from lib.pysixd import pose_error as PE

    from gdrnet_amd import synth

    g = {}
    for case in ("A", "B"):
        seed = synth.POSE_METRIC_SEEDS[case]
        while True:
            inp = synth.make_pose_metric_inputs(case, seed=seed)
            err = reference_errors(inp, PE, get_closest_rot)
            ok = thresholds_clear(err, inp)
            fl = flags(err, inp)
            if case == "A":
                ok = ok and bool(np.all(fl.any(0)) and not np.any(fl.all(0)))
                # the re / te means of the table: not within 1e-6 of a rounding boundary of the two printed decimals
                for col in (1, 2):
                    means = [err[inp["labels"] == c, col].mean() for c in range(len(inp["points"]))]
                    ok = ok and all(abs((100 * m) % 1.0 - 0.5) > 1e-4 for m in means + [np.mean(means)])
            if ok:
                break
            print(f"case {case}: seed {seed} sits on a threshold, trying the next one")
            seed += 1
        assert seed == synth.POSE_METRIC_SEEDS[case], f"record seed {seed} for case {case} in synth.POSE_METRIC_SEEDS"
        g[f"{case}/err"] = err
        g[f"{case}/seed"] = np.array(seed)
        if case == "A":
            rows = reference_table(inp, EV)
            g["A/table"] = np.array(["\t".join(r) for r in rows])
            # the flags the evaluator appended == the flags of the stored errors (the table is their per-class mean)
            names = inp["obj_names"]
            for k, metric in enumerate(METRICS):
                row = rows[1 + k]
                assert row[0] == metric
                for j, name in enumerate(rows[0][1:-1]):
                    c = names.index(name)
                    seen = int((inp["labels"] == c).sum()) + inp["missing"].get(c, 0)
                    assert row[1 + j] == f"{100 * (fl[inp['labels'] == c, k].sum() / seen):.2f}", (metric, name)
            print("\n".join("  ".join(r) for r in rows))
        print(f"case {case}: seed {seed}, N = {len(err)}, ad {err[:, 0].min():.3g}..{err[:, 0].max():.3g}, re {err[:, 1].min():.3g}..{err[:, 1].max():.3g}, "
              f"te {err[:, 2].min():.3g}..{err[:, 2].max():.3g}, proj {err[:, 3].min():.3g}..{err[:, 3].max():.3g}")
    np.savez_compressed(os.path.join(HERE, "g12_pose_metrics.npz"), **g)


if __name__ == "__main__":
    main()
