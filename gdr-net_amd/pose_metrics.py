"""Pose-error metrics and the recall table on the device (csrc/pose_metrics.hip).

Host-side mirror of what the reference's evaluator runs per instance on the CPU right after inference
(``GDRN_EvaluatorCustom._eval_predictions``, core/gdrn_modeling/gdrn_custom_evaluator.py:493-670):

* ``te`` / ``re`` / ``add`` / ``adi`` / ``arp_2d``     -- lib/pysixd/pose_error.py:297-444
* ``get_closest_rot``                                  -- core/utils/pose_utils.py:430-454
* the 15 recall flags and the ``big_tab`` summary      -- gdrn_custom_evaluator.py:593-647

for a whole batch per call, in fp64 like the reference's numpy (adi: an exact brute-force nearest neighbour instead of a KD-tree per
instance).  ``pose_errors`` returns device tensors; ``PoseRecall`` keeps its counters on the device and copies them out once, in
``summarize()``.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import cabi, devargs

ERROR_NAMES = ("ad", "re", "te", "proj")
METRIC_NAMES = ("ad_2", "ad_5", "ad_10", "rete_2", "rete_5", "rete_10", "re_2", "re_5", "re_10", "te_2", "te_5", "te_10",
                "proj_2", "proj_5", "proj_10")   # the evaluator's order (:516-532) = the column order of the kernel's hits
WHERE = "the pose metrics"   # (this module in devargs' error sentence)


class ModelTable(devargs.DeviceTables):
    """Per-class model tables, packed once: ``points`` a list of [n_c,3] arrays, ``diameters`` [C], ``sym_infos`` None or per class None / [K,3,3]
    (a bare 3x3 is one symmetry, as get_closest_rot reshapes it), ``sym_classes`` the class indices scored as symmetric (the role of
    cfg.DATASETS.SYM_OBJS: adi instead of add, closest-rotation search).  ``pad_value`` fills the table rows beyond a class's own points; the
    kernels never read them into a result."""

    TABLES = ("pts", "npts", "diameter", "sym", "nsym", "is_sym")

    def __init__(self, points, diameters, sym_infos=None, sym_classes=(), pad_value=0.0):
        C = len(points)
        if C == 0 or len(diameters) != C or (sym_infos is not None and len(sym_infos) != C):
            raise ValueError("points, diameters and sym_infos need one entry per class")
        self.num_classes = C
        self.pts, self.npts, self.n_max, self.diameter = devargs.pack_points(points, diameters, pad_value, n_min=1)   # (a class may be empty)
        syms = [None] * C if sym_infos is None else [None if s is None else np.asarray(s, dtype=np.float64).reshape(-1, 3, 3) for s in sym_infos]
        self.nsym = np.array([0 if s is None else len(s) for s in syms], dtype=np.int32)
        self.k_max = max(1, int(self.nsym.max()))
        self.sym = np.zeros((C, self.k_max, 3, 3), dtype=np.float64)
        for c, s in enumerate(syms):
            if s is not None:
                self.sym[c, : len(s)] = s
        self.is_sym = np.zeros(C, dtype=np.int32)
        for c in sym_classes:
            if not 0 <= int(c) < C:
                raise ValueError(f"sym_classes: {c} is not a class index below {C}")
            self.is_sym[int(c)] = 1


def _errors(table, R_est, t_est, R_gt, t_gt, K, labels):
    N = int(R_est.shape[0]) if isinstance(R_est, torch.Tensor) else 0
    R_est, R_gt, K = (devargs.device_tensor(m, torch.float64, (-1, 3, 3), what, WHERE) for m, what in ((R_est, "R_est"), (R_gt, "R_gt"), (K, "K")))
    t_est, t_gt = (devargs.device_tensor(v, torch.float64, (-1, 3), what, WHERE) for v, what in ((t_est, "t_est"), (t_gt, "t_gt")))
    dev = R_est.device
    K = devargs.per_row_K(K, N)
    if not (R_gt.shape[0] == t_est.shape[0] == t_gt.shape[0] == N):
        raise ValueError("R_est, t_est, R_gt and t_gt need one entry per row")
    lib = cabi.load()
    lab, lab_host = devargs.index_vector(labels, N, None, dev, "labels")   # (their range: the library refuses a label outside the table)
    tb = table.on(dev)
    err = torch.empty(max(N, 1), 4, dtype=torch.float64, device=dev)[:N]
    ws = devargs.workspace(lib.gdrn_pose_metrics_workspace_bytes(N, table.n_max), dev, "pose_metrics_workspace_bytes")
    st = devargs.stream(dev)
    cabi.check(lib.gdrn_pose_errors(cabi.ptr(R_est), cabi.ptr(t_est), cabi.ptr(R_gt), cabi.ptr(t_gt), cabi.ptr(K), cabi.ptr(lab),
                                    lab_host.ctypes.data, N, cabi.ptr(tb["pts"]), cabi.ptr(tb["npts"]), table.n_max, cabi.ptr(tb["is_sym"]),
                                    cabi.ptr(tb["sym"]), cabi.ptr(tb["nsym"]), table.k_max, table.num_classes, cabi.ptr(err), cabi.ptr(ws), st),
               "pose_errors")
    return err, lab, lab_host


def pose_errors(table, R_est, t_est, R_gt, t_gt, K, labels):
    """ad (add, or adi for the table's symmetric classes), re [deg], te, proj [px] of N poses: a dict of [N] fp64 device tensors plus "err", the
    packed [N,4] in that order.  R_* [N,3,3], t_* [N,3], K [N,3,3] or [3,3]: device tensors, fp32 or fp64; labels [N]: class per row."""
    err, _, _ = _errors(table, R_est, t_est, R_gt, t_gt, K, labels)
    out = {name: err[:, j] for j, name in enumerate(ERROR_NAMES)}
    out["err"] = err
    return out


def format_table(obj_names, hits, seen, re_sum, te_sum, err_cnt):
    """The rows of the evaluator's ``big_tab`` (gdrn_custom_evaluator.py:613-647) from per-class counters (host arrays, one entry per name):
    header ``objects, <sorted names>, Avg(k)``, the 15 recall rows as f"{100 * mean:.2f}", the re / te rows as f"{mean:.2f}"; the classes that
    were never seen are left out, a class without a single prediction reads 0.00 and nan.  Every cell is a string."""
    hits, seen, err_cnt = np.asarray(hits, dtype=np.int64), np.asarray(seen, dtype=np.int64), np.asarray(err_cnt, dtype=np.int64)
    sums = {"re": np.asarray(re_sum, dtype=np.float64), "te": np.asarray(te_sum, dtype=np.float64)}
    order = sorted((name, c) for c, name in enumerate(obj_names) if seen[c] > 0)
    rows = [["objects"] + [name for name, _ in order] + [f"Avg({len(order)})"]]
    for k, metric in enumerate(METRIC_NAMES):
        means = [float(hits[c, k]) / float(seen[c]) for _, c in order]
        line = [metric] + [f"{100 * m:.2f}" for m in means]
        if order:
            line.append(f"{100 * np.mean(means):.2f}")
        rows.append(line)
    for name in ("re", "te"):
        means = [sums[name][c] / float(err_cnt[c]) if err_cnt[c] > 0 else float("nan") for _, c in order]
        line = [name] + [f"{m:.2f}" for m in means]
        if order:
            line.append(f"{np.mean(means):.2f}")
        rows.append(line)
    return rows


class PoseRecall:
    """The evaluator's recall bookkeeping on the device: ``update`` scores a batch of poses and adds their 15 flags and re / te to per-class
    counters without reading anything back, ``add_missing`` counts ground-truth instances that got no prediction (zeros in every recall, nothing
    in the re / te means: gdrn_custom_evaluator.py:552-555), ``summarize`` makes the one device-to-host copy and returns the table rows."""

    def __init__(self, table, obj_names):
        if len(obj_names) != table.num_classes:
            raise ValueError("one name per class of the table")
        self.table, self.obj_names = table, list(obj_names)
        self._state = None

    def _views(self, state):
        C, F = self.table.num_classes, len(METRIC_NAMES)
        return dict(hits=state[: C * F], seen=state[C * F : C * (F + 1)], err_cnt=state[C * (F + 1) : C * (F + 2)],
                    re_sum=state[C * (F + 2) : C * (F + 3)].view(torch.float64), te_sum=state[C * (F + 3) : C * (F + 4)].view(torch.float64))

    def _on(self, device):
        """one flat int64 buffer [hits C*15 | seen C | err_cnt C | re_sum C | te_sum C (fp64 bits)]: one copy brings all of it to the host"""
        if self._state is None:
            self._state = torch.zeros(self.table.num_classes * (len(METRIC_NAMES) + 4), dtype=torch.int64, device=device)
        elif self._state.device != torch.device(device):
            raise ValueError(f"the counters live on {self._state.device}")
        return self._views(self._state)

    def update(self, R_est, t_est, R_gt, t_gt, K, labels):
        err, lab, lab_host = _errors(self.table, R_est, t_est, R_gt, t_gt, K, labels)
        dev = err.device
        v, tb = self._on(dev), self.table.on(dev)
        cabi.check(cabi.load().gdrn_pose_recall_accumulate(cabi.ptr(err), cabi.ptr(lab), lab_host.ctypes.data, err.shape[0], cabi.ptr(tb["diameter"]),
                                                           self.table.num_classes, cabi.ptr(v["hits"]), cabi.ptr(v["seen"]), cabi.ptr(v["re_sum"]),
                                                           cabi.ptr(v["te_sum"]), cabi.ptr(v["err_cnt"]), devargs.stream(dev)),
                   "pose_recall_accumulate")

    def add_missing(self, label, count=1, device=None):
        if not 0 <= int(label) < self.table.num_classes or int(count) < 0:
            raise ValueError((label, count))
        if self._state is None and device is None:
            raise cabi.GdrnHipError("add_missing before the first update needs the device of the counters")
        self._on(device if self._state is None else self._state.device)["seen"][int(label)] += int(count)

    def counters(self):
        """host copies of the counters (the one device-to-host copy): dict of hits [C,15], seen, err_cnt [C] int64, re_sum, te_sum [C] fp64"""
        C = self.table.num_classes
        if self._state is None:
            host = torch.zeros(C * (len(METRIC_NAMES) + 4), dtype=torch.int64)
        else:
            host = self._state.cpu()
        v = {k: t.numpy() for k, t in self._views(host).items()}
        v["hits"] = v["hits"].reshape(C, len(METRIC_NAMES))
        return v

    def summarize(self):
        return format_table(self.obj_names, **self.counters())

    def reset(self):
        if self._state is not None:
            self._state.zero_()
