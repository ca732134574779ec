"""The scores of the reference's YCB-V tables on the device (csrc/sixd_scores.hip): AUC / ABS of add, adi and ad, add / adi by the diameter, and
the symmetry-aware reS / teS / reteS / projS.

Host-side mirror of what the reference gets by writing its estimates to a CSV and running the toolkit on the CPU, one estimate at a time
(``ERROR_TYPES="AUCadd,AUCadi,AUCad,ad,ABSadd,ABSadi,ABSad"`` in every configs/gdrn/ycbv* file; ``load_and_print_val_scores_tab`` defaults to
``["projS", "ad", "reteS"]``, core/gdrn_modeling/test_utils.py:246-248):

* ``pose_error.add`` / ``adi`` of EVERY row             -- lib/pysixd/pose_error.py:297-337 as eval_calc_errors.py:395-406 calls them
* ``pose_error.re_sym`` / ``te_sym`` / ``arp_2d_sym``   -- pose_error.py:184-234 as eval_calc_errors.py:412-448 calls them
* thresholds, normalisation, matching, recall           -- eval_pose_results_more.py:64-93, eval_calc_scores.py:238-250, pose_matching.py:68,
  score.calc_recall
* the tables                                            -- test_utils.summary_scores:182-243

The tables are those of ``bop_metrics.BopModelTable`` (points, diameters, the ``(R, t)`` sets of ``symmetry_transformations``).  Units are metres
(the toolkit's mm / cm thresholds become m).  One estimate per ground-truth target is assumed -- ``select_top_estimates`` makes that true for
detector boxes; the toolkit's estimate-to-target matching is not done -- and the bounding-sphere shortcut of eval_calc_errors.py:340-342,375-380
(``add`` / ``adi`` = inf) is not applied: the errors are the functions' values.  Errors and counters stay on the device; ``ScoreRecall.summarize()``
makes the one device-to-host copy.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import cabi, devargs

WHERE = "the 6D scores"   # (this module in devargs' error sentence)
AUC_THS_CM = np.linspace(1, 10, 10)   # eval_pose_results_more.py:79-82
# (type, header suffix per threshold, first column of the kernel's hits) in the order of eval_pose_results_more.py:64-93 = gdrn_hip.h's columns;
# the suffixes are test_utils.get_thr_str of misc.get_score_signature's "{:.3f}": whole numbers lose their decimals, the others keep three
SCORE_TYPES = (
    ("AUCadd", tuple(str(k) for k in range(1, 11)), 0),
    ("AUCadi", tuple(str(k) for k in range(1, 11)), 10),
    ("AUCad", tuple(str(k) for k in range(1, 11)), 20),
    ("ABSadd", ("2",), 30),
    ("ABSadi", ("2",), 31),
    ("ABSad", ("2",), 32),
    ("add", ("0.020", "0.050", "0.100"), 33),
    ("adi", ("0.020", "0.050", "0.100"), 36),
    ("reS", ("2", "5", "10"), 39),
    ("teS", ("2", "5", "10"), 42),
    ("reteS", ("2", "5", "10"), 45),
    ("projS", ("2", "5", "10"), 48),
)
AUC_TYPES = ("AUCadd", "AUCadi", "AUCad")
NFLAGS = 51          # GDRN_SIXD_NFLAGS
AD_SLAB, AD_TILE, SYM_SLAB = 1024, 512, 8   # GDRN_SIXD_AD_SLAB, GDRN_SIXD_AD_TILE, GDRN_SIXD_SYM_SLAB: where the kernels take another path


def _rows(table, R_est, t_est, R_gt, t_gt, K, labels):
    if K is None:
        R_est, t_est = devargs.device_tensor(R_est, torch.float64, (-1, 3, 3), "R_est", WHERE), devargs.device_tensor(t_est, torch.float64, (-1, 3), "t_est", WHERE)
        N = int(R_est.shape[0])
        if t_est.shape[0] != N:
            raise ValueError("R and t need one entry per row")
    else:
        R_est, t_est, K, N = devargs.poses(R_est, t_est, K, WHERE)
    R_gt, t_gt = devargs.device_tensor(R_gt, torch.float64, (-1, 3, 3), "R_gt", WHERE), devargs.device_tensor(t_gt, torch.float64, (-1, 3), "t_gt", WHERE)
    if R_gt.shape[0] != N or t_gt.shape[0] != N:
        raise ValueError("R_est, t_est, R_gt and t_gt need one entry per row")
    lab, lab_host = devargs.index_vector(labels, N, table.num_classes, R_est.device, "labels")
    return R_est, t_est, R_gt, t_gt, K, lab, lab_host, N


def ad_errors(table, R_est, t_est, R_gt, t_gt, labels):
    """``pose_error.add`` and ``adi`` (lib/pysixd/pose_error.py:297-337) of N estimates, BOTH for every row whatever its class, against the plain
    ground-truth pose as eval_calc_errors.py:395-406 calls them: [N,2] fp64 device tensor, column 0 add, column 1 adi, in the unit of the points.
    adi is the exact brute-force nearest neighbour of ``pose_metrics`` (the reference builds a KD-tree per estimate: the same minimum).  R_* [N,3,3],
    t_* [N,3]: device tensors, fp32 or fp64; labels [N]: class per row of the ``BopModelTable`` ``table``."""
    R_est, t_est, R_gt, t_gt, _, lab, lab_host, N = _rows(table, R_est, t_est, R_gt, t_gt, None, labels)
    dev = R_est.device
    err = torch.empty(max(N, 1), 2, dtype=torch.float64, device=dev)[:N]
    if N == 0:
        return err
    lib = cabi.load()
    tb = table.on(dev)
    ws = devargs.workspace(lib.gdrn_ad_errors_workspace_bytes(N, table.n_max), dev, "ad_errors_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_ad_errors(p(R_est), p(t_est), p(R_gt), p(t_gt), p(lab), lab_host.ctypes.data, N, p(tb["pts"]), p(tb["npts"]), table.n_max,
                                  table.num_classes, p(err), p(ws), devargs.stream(dev)), "ad_errors")
    return err


def sym_errors(table, R_est, t_est, R_gt, t_gt, K, labels):
    """``pose_error.re_sym``, ``te_sym`` and ``arp_2d_sym`` (lib/pysixd/pose_error.py:184-234) of N estimates as eval_calc_errors.py:412-448 calls
    them: [N,3] fp64 device tensor, column 0 re_sym in degrees, column 1 te_sym in the unit of the points, column 2 arp_2d_sym in pixels, each
    the minimum over the symmetry transformations of the class.  R_* [N,3,3], t_* [N,3], K [N,3,3] or [3,3]: device tensors, fp32 or fp64; labels
    [N]: class per row.

    te_sym is the reference's AS IT RUNS: pose_error.py:218 adds the flattened t_gt [3] to the column R_gt t_S [3,1], numpy broadcasts, and the
    function returns the Frobenius norm of M[i][j] = (R_gt t_S)[i] + t_gt[j] - t_est[j] -- sqrt(3) |t_gt - t_est| for a class with the identity
    only, not the distance itself.  The toolkit takes its teS / reteS decisions on that value, so it is what this column holds;
    ``pose_metrics.pose_errors`` has the plain translation error."""
    R_est, t_est, R_gt, t_gt, K, lab, lab_host, N = _rows(table, R_est, t_est, R_gt, t_gt, K, labels)
    dev = R_est.device
    err = torch.empty(max(N, 1), 3, dtype=torch.float64, device=dev)[:N]
    if N == 0:
        return err
    lib = cabi.load()
    tb = table.on(dev)
    ws = devargs.workspace(lib.gdrn_sym_errors_workspace_bytes(N, table.n_max, table.s_max), dev, "sym_errors_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_sym_errors(p(R_est), p(t_est), p(R_gt), p(t_gt), p(K), p(lab), lab_host.ctypes.data, N, p(tb["pts"]), p(tb["npts"]),
                                   table.n_max, p(tb["sym_R"]), p(tb["sym_t"]), p(tb["nsym"]), table.s_max, table.num_classes, p(err), p(ws),
                                   devargs.stream(dev)), "sym_errors")
    return err


def select_top_estimates(target_keys, scores, inst_count=1):
    """The indices of the estimates the toolkit would score (eval_calc_errors.py:281-308, ``n_top = -1``): per target -- one (scene, image, object)
    key -- the ``inst_count`` estimates with the highest score.  ``target_keys``: one hashable key (or row of an integer array) per estimate,
    ``scores`` [n], ``inst_count`` an int or a mapping key -> count (a key it lacks counts 1).  The toolkit sorts with Python's stable ``sorted(...,
    reverse=True)``: among equal scores the estimate that comes first in the input wins.  Returns an int64 array: the targets in the order of
    their first estimate, each target's estimates by descending score.  A target without an estimate contributes nothing here: count it with
    ``add_missing``.  (numpy, no GPU.)"""
    keys = [tuple(np.asarray(k).reshape(-1).tolist()) if isinstance(k, (np.ndarray, list, tuple)) else k for k in target_keys]
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    if len(keys) != len(scores):
        raise ValueError(f"{len(keys)} target keys for {len(scores)} scores")
    groups = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    out = []
    for k, idx in groups.items():
        n_top = int(inst_count.get(k, 1)) if hasattr(inst_count, "get") else int(inst_count)
        if n_top < 0:
            raise ValueError(f"inst_count {n_top} of target {k}")
        out.extend(sorted(idx, key=lambda i: scores[i], reverse=True)[:n_top])
    return np.asarray(out, dtype=np.int64)


def score_tables(obj_names, hits, seen):
    """The tables of ``test_utils.summary_scores`` (core/gdrn_modeling/test_utils.py:182-243) from per-class counters (host arrays: hits [C,51] in
    the column order of gdrn_hip.h, seen [C]): a dict type -> rows, every cell a string.  Header ``["objects", "{type}_{thr}", ...]``, one row per
    object in class order with ``f"{100 * recall:.2f}"`` per threshold, then ``Avg(k)`` -- the mean over the k objects -- when k > 1.  An AUC type
    has ONE column, ``"{type}_10"``: per object the mean of its ten recalls (test_utils.py:238), and always an ``Avg(k)`` row.  Two deliberate
    differences from the reference: classes without a target are left out (it averages a 0.0 in for them), and the AUC table ends in
    ``Avg(k)`` also for k = 1 (its ``[1:-1]`` slice, test_utils.py:236, then drops the only object and prints nan)."""
    hits, seen = np.asarray(hits, dtype=np.int64).reshape(len(obj_names), NFLAGS), np.asarray(seen, dtype=np.int64).reshape(-1)
    order = [c for c in range(len(obj_names)) if seen[c] > 0]
    out = {}
    for name, thr, col in SCORE_TYPES:
        rec = np.array([[hits[c, col + k] / float(seen[c]) for k in range(len(thr))] for c in order], dtype=np.float64).reshape(len(order), len(thr))
        if name in AUC_TYPES:
            rec = rec.mean(axis=1, keepdims=True) if len(order) else rec[:, :1]
            rows = [["objects", f"{name}_{thr[-1]}"]]
        else:
            rows = [["objects"] + [f"{name}_{t}" for t in thr]]
        for j, c in enumerate(order):
            rows.append([obj_names[c]] + [f"{100 * r:.2f}" for r in rec[j]])
        if len(order) > 1 or (name in AUC_TYPES and len(order) == 1):
            rows.append([f"Avg({len(order)})"] + [f"{100 * m:.2f}" for m in rec.mean(axis=0)])
        out[name] = rows
    return out


class ScoreRecall:
    """The toolkit's score pass for these types on the device: ``update`` adds a batch of errors (``ad`` [N,2] from ``ad_errors``, ``sym`` [N,3]
    from ``sym_errors``) to per-class hit counters without reading anything back, ``add_missing`` counts ground-truth targets that got no estimate
    (a miss under every threshold), ``summarize`` makes the one device-to-host copy and returns ``score_tables``' dict.  ``sym_classes``: the class
    indices whose "ad" is adi (the role of dp_model["symmetric_obj_ids"]); the others' is add.  ``im_width``: the test images' width, kept for
    symmetry with ``BopRecall`` -- eval_calc_scores.py:246-250 scales only mspd by 640 / im_width, none of these types, so projS is in the pixels
    of the test image.

    An AUC here is the reference's: the mean of the recalls under the ten thresholds 1 .. 10 cm (test_utils.py:238).  It is NOT YCB-Video's
    area under the continuous accuracy-threshold curve."""

    def __init__(self, table, obj_names, sym_classes, im_width):
        if len(obj_names) != table.num_classes:
            raise ValueError("one name per class of the table")
        self.table, self.obj_names, self.im_width = table, list(obj_names), float(im_width)
        if not self.im_width > 0:
            raise ValueError(f"im_width {im_width}")
        self.ad_is_adi = np.zeros(table.num_classes, dtype=np.int32)
        for c in sym_classes:
            if not 0 <= int(c) < table.num_classes:
                raise ValueError(f"sym_classes: {c} is not a class index below {table.num_classes}")
            self.ad_is_adi[int(c)] = 1
        self._state = None
        self._is_adi_dev = None

    def _views(self, state):
        C = self.table.num_classes
        return dict(hits=state[: C * NFLAGS], seen=state[C * NFLAGS : C * (NFLAGS + 1)])

    def _on(self, device):
        """one flat int64 buffer [hits C*51 | seen C]: one copy brings all of it to the host"""
        if self._state is None:
            self._state = torch.zeros(self.table.num_classes * (NFLAGS + 1), dtype=torch.int64, device=device)
            self._is_adi_dev = torch.from_numpy(self.ad_is_adi).to(device)
        elif self._state.device != torch.device(device):
            raise ValueError(f"the counters live on {self._state.device}")
        return self._views(self._state)

    def update(self, ad, sym, labels):
        ad = devargs.device_tensor(ad, torch.float64, None, "ad", "the 6D score recall")
        sym = devargs.device_tensor(sym, torch.float64, None, "sym", "the 6D score recall")
        N = int(ad.shape[0])
        if tuple(ad.shape) != (N, 2) or tuple(sym.shape) != (N, 3):
            raise ValueError("ad is [N,2], sym [N,3]")
        dev = ad.device
        lab, lab_host = devargs.index_vector(labels, N, self.table.num_classes, dev, "labels")
        v, tb = self._on(dev), self.table.on(dev)
        if N == 0:
            return
        p = cabi.ptr
        cabi.check(cabi.load().gdrn_score_recall_accumulate(p(ad), p(sym), p(lab), lab_host.ctypes.data, N, p(tb["diameter"]), p(self._is_adi_dev),
                                                            self.table.num_classes, p(v["hits"]), p(v["seen"]), devargs.stream(dev)),
                   "score_recall_accumulate")

    def add_missing(self, label, count=1, device=None):
        if not 0 <= int(label) < self.table.num_classes or int(count) < 0:
            raise ValueError((label, count))
        if self._state is None and device is None:
            raise cabi.GdrnHipError("add_missing before the first update needs the device of the counters")
        self._on(device if self._state is None else self._state.device)["seen"][int(label)] += int(count)

    def counters(self):
        """host copies of the counters (the one device-to-host copy): hits [C,51] in the column order of ``SCORE_TYPES``, seen [C], int64"""
        C = self.table.num_classes
        host = torch.zeros(C * (NFLAGS + 1), dtype=torch.int64) if self._state is None else self._state.cpu()
        v = {k: t.numpy() for k, t in self._views(host).items()}
        v["hits"] = v["hits"].reshape(C, NFLAGS)
        return v

    def summarize(self):
        return score_tables(self.obj_names, **self.counters())

    def reset(self):
        if self._state is not None:
            self._state.zero_()
