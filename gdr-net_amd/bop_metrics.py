"""The BOP pose errors -- VSD, MSSD, MSPD -- and average recall on the device (csrc/bop_metrics.hip).

Host-side mirror of what the reference gets by writing its estimates to a CSV and running the BOP toolkit on the CPU
(``GDRN_Evaluator``, core/gdrn_modeling/gdrn_evaluator.py:437-514 -> lib/pysixd/scripts/eval_pose_results_more.py):

* ``pose_error.vsd`` / ``mssd`` / ``mspd``             -- lib/pysixd/pose_error.py:84-179, per estimate (eval_calc_errors.py:344-372), VSD on
  two depth renders of the model, here ``render.render_depth`` for the whole batch in one call
* ``misc.get_symmetry_transformations``                -- lib/pysixd/misc.py:206-254 (host, once per model)
* the recall under ten thresholds per error and AR     -- eval_calc_scores.py:239-250, eval_pose_results_more.py:58-63

Units are metres (BOP's ``delta = 15`` mm is ``0.015``).  One estimate per ground-truth target is assumed -- what GDR-Net produces; the toolkit's
estimate-to-target matching is not done -- and the speed shortcuts of eval_calc_errors.py:328-347,366-367 are not applied: the errors are the
functions' values.  Errors stay on the device; ``BopRecall.summarize()`` makes the one device-to-host copy.  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import cabi, devargs, render

COST_TYPES = {"step": 0, "tlinear": 1}   # GDRN_VSD_STEP, GDRN_VSD_TLINEAR
VSD_TAUS = np.arange(0.05, 0.51, 0.05)   # eval_pose_results_more.py:58
VSD_THS = np.arange(0.05, 0.51, 0.05)    # :60
MSSD_THS = np.arange(0.05, 0.51, 0.05)   # :62
MSPD_THS = np.arange(5, 51, 5).astype(np.float64)   # :63
NTH = 10
MAX_TAUS = 32                            # GDRN_VSD_MAX_TAUS
WHERE = "the BOP errors"                 # (this module in devargs' error sentence)


def _rotation_about(angle, axis):
    """transform.rotation_matrix(angle, axis)[:3, :3] (lib/pysixd/transform.py:319-328), operation for operation."""
    sina, cosa = math.sin(angle), math.cos(angle)
    d = np.array(axis, dtype=np.float64, copy=True).reshape(-1)[:3]
    d /= math.sqrt(np.dot(d, d))
    R = np.diag([cosa, cosa, cosa])
    R += np.outer(d, d) * (1.0 - cosa)
    d *= sina
    R += np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return R


def symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """``misc.get_symmetry_transformations`` (lib/pysixd/misc.py:206-254) restated in numpy: (R [S,3,3], t [S,3]) from a models_info entry with the
    optional keys ``symmetries_discrete`` (flattened 4x4 matrices) and ``symmetries_continuous`` ({"axis", "offset"}).  Without a continuous
    symmetry the identity comes first.  The reference's quirk is kept: the discretised rotations of a continuous symmetry are the steps
    ``range(1, n)`` of n = ceil(pi / max_sym_disc_step) = 315, so a class WITH one gets 314 transformations per discrete one and NOT the identity
    itself.  t is in the unit of the model_info (BOP's files: mm)."""
    disc = [(np.eye(3), np.zeros((3, 1)))]
    for sym in model_info.get("symmetries_discrete", []):
        m = np.reshape(sym, (4, 4)).astype(np.float64)
        disc.append((m[:3, :3], m[:3, 3].reshape(3, 1)))
    cont = []
    for sym in model_info.get("symmetries_continuous", []):
        axis = np.array(sym["axis"])
        offset = np.array(sym["offset"], dtype=np.float64).reshape(3, 1)
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(1, steps):
            R = _rotation_about(i * step, axis)
            cont.append((R, -R.dot(offset) + offset))
    out = []
    for Rd, td in disc:
        if cont:
            for Rc, tc in cont:
                out.append((Rc.dot(Rd), Rc.dot(td) + tc))
        else:
            out.append((Rd, td))
    return np.stack([R for R, _ in out]), np.stack([t.reshape(3) for _, t in out])


class BopModelTable(devargs.DeviceTables):
    """Per-class tables of MSSD / MSPD and the recall, packed once: ``points`` a list of [n_c,3] arrays (metres), ``diameters`` [C], ``syms`` None or
    per class None (the identity only) / ``(R [S,3,3], t [S,3])`` as ``symmetry_transformations`` returns them.  ``pad_value`` / ``sym_pad_value``
    fill the table rows beyond a class's own points / transformations; the kernels never read them into a result."""

    TABLES = ("pts", "npts", "diameter", "sym_R", "sym_t", "nsym")

    def __init__(self, points, diameters, syms=None, pad_value=0.0, sym_pad_value=0.0):
        C = len(points)
        if C == 0 or len(diameters) != C or (syms is not None and len(syms) != C):
            raise ValueError("points, diameters and syms need one entry per class")
        self.num_classes = C
        self.pts, self.npts, self.n_max, self.diameter = devargs.pack_points(points, diameters, pad_value)
        if not self.npts.all():
            raise ValueError("a class without points has no MSSD / MSPD")
        packed = []
        for c in range(C):
            s = None if syms is None else syms[c]
            if s is None:
                packed.append((np.eye(3)[None], np.zeros((1, 3))))
                continue
            R, t = np.asarray(s[0], dtype=np.float64).reshape(-1, 3, 3), np.asarray(s[1], dtype=np.float64).reshape(-1, 3)
            if len(R) == 0 or len(R) != len(t):
                raise ValueError(f"class {c}: a symmetry set is one rotation and one translation per transformation, at least one")
            packed.append((R, t))
        self.nsym = np.array([len(R) for R, _ in packed], dtype=np.int32)
        self.s_max = int(self.nsym.max())
        self.sym_R = np.full((C, self.s_max, 3, 3), float(sym_pad_value), dtype=np.float64)
        self.sym_t = np.full((C, self.s_max, 3), float(sym_pad_value), dtype=np.float64)
        for c, (R, t) in enumerate(packed):
            self.sym_R[c, : len(R)], self.sym_t[c, : len(t)] = R, t


def _f64_vec(v, n, device, what):
    """[n] fp64 device tensor from a list / numpy array / tensor"""
    if isinstance(v, torch.Tensor):
        v = v.detach().to(device=device, dtype=torch.float64).reshape(-1).contiguous()
    else:
        v = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))).to(device)
    if n is not None and v.shape[0] != n:
        raise ValueError(f"{what}: {v.shape[0]} entries for {n} rows")
    return v


def _depth(d, what):
    d = devargs.device_tensor(d, torch.float32, None, what, WHERE)
    if d.dim() != 3:
        raise ValueError(f"{what} must be [n, H, W]")
    return d


def _gt_poses(R_gt, t_gt, N):
    R_gt, t_gt = devargs.device_tensor(R_gt, torch.float64, (-1, 3, 3), "R_gt", WHERE), devargs.device_tensor(t_gt, torch.float64, (-1, 3), "t_gt", WHERE)
    if R_gt.shape[0] != N or t_gt.shape[0] != N:
        raise ValueError("R_est, t_est, R_gt and t_gt need one entry per row")
    return R_gt, t_gt


def vsd_from_depth(depth_est, depth_gt, depth_test, frame, K, diameters, delta, taus=VSD_TAUS, cost_type="step", normalized_by_diameter=True,
                   return_counts=False):
    """``pose_error.vsd`` (lib/pysixd/pose_error.py:84-126, "bop19" visibility) of N estimates on depth maps that are already rendered: ``depth_est``
    / ``depth_gt`` [N,H,W] fp32 device tensors (the model under the estimated / ground-truth pose, 0 = nothing), ``depth_test`` [F,H,W] (the test
    images, 0 = missing), ``frame`` [N] the test image of each row, ``K`` [N,3,3] or [3,3] (the skew term is not read, as in the reference),
    ``diameters`` [N] PER ROW, ``delta`` in the depth maps' unit, ``taus`` [T].  Returns err [N,T] fp64 on the device; with ``return_counts`` also
    counts [N,2+T] int64 = |union|, |union| - |intersection|, the step cost count per tau."""
    if cost_type not in COST_TYPES:
        raise ValueError(f"cost_type {cost_type!r}: step or tlinear")
    depth_est, depth_gt, depth_test = _depth(depth_est, "depth_est"), _depth(depth_gt, "depth_gt"), _depth(depth_test, "depth_test")
    N, H, W = (int(s) for s in depth_est.shape)
    if tuple(depth_gt.shape) != (N, H, W) or tuple(depth_test.shape[1:]) != (H, W):
        raise ValueError("depth_est and depth_gt are [N,H,W], depth_test is [F,H,W]")
    dev = depth_est.device
    F = int(depth_test.shape[0])
    K = devargs.per_row_K(devargs.device_tensor(K, torch.float64, (-1, 3, 3), "K", WHERE), N)
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    diam = _f64_vec(diameters, N, dev, "diameters")
    tau = _f64_vec(taus, None, dev, "taus")
    T = int(tau.shape[0])
    if not 1 <= T <= MAX_TAUS:
        raise ValueError(f"1 to {MAX_TAUS} taus")
    lib = cabi.load()
    err = torch.empty(max(N, 1), T, dtype=torch.float64, device=dev)[:N]
    counts = torch.empty(max(N, 1), 2 + T, dtype=torch.int64, device=dev)[:N]
    ws = devargs.workspace(lib.gdrn_vsd_workspace_bytes(N, H, W, T), dev, "vsd_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_vsd(p(depth_est), p(depth_gt), p(depth_test), p(fr), fr_host.ctypes.data, F, p(K), p(diam), N, H, W, float(delta), p(tau), T,
                            COST_TYPES[cost_type], 1 if normalized_by_diameter else 0, p(err), p(counts), p(ws), devargs.stream(dev)), "vsd")
    return (err, counts) if return_counts else err


def vsd(meshes, labels, R_est, t_est, R_gt, t_gt, K, depth_test, frame, diameters, delta, taus=VSD_TAUS, cost_type="step",
        normalized_by_diameter=True, return_counts=False, near=render.NEAR, far=render.FAR):
    """``pose_error.vsd`` of N estimates from their poses: the model ``labels[i]`` of the ``render.MeshTable`` ``meshes`` is rendered under the
    estimated and the ground-truth pose -- all 2N instances with ONE ``render_depth`` call -- and scored by ``vsd_from_depth`` against
    ``depth_test[frame[i]]``.  ``diameters`` [C] PER CLASS of the mesh table.  Poses and K: device tensors, fp32 or fp64.  Nothing is read back."""
    R_est, t_est, K, N = devargs.poses(R_est, t_est, K, WHERE)
    R_gt, t_gt = _gt_poses(R_gt, t_gt, N)
    depth_test = _depth(depth_test, "depth_test")
    dev = R_est.device
    lab, lab_host = devargs.index_vector(labels, N, meshes.num_classes, dev, "labels")
    diam = _f64_vec(diameters, meshes.num_classes, dev, "diameters")[lab.long()]
    H, W = int(depth_test.shape[1]), int(depth_test.shape[2])
    both = render.render_depth(meshes, np.concatenate([lab_host, lab_host]), torch.cat([R_est, R_gt]), torch.cat([t_est, t_gt]), torch.cat([K, K]),
                               H, W, near, far)
    return vsd_from_depth(both[:N], both[N:], depth_test, frame, K, diam, delta, taus, cost_type, normalized_by_diameter, return_counts)


def mssd_mspd(table, R_est, t_est, R_gt, t_gt, K, labels):
    """``pose_error.mssd`` and ``mspd`` (lib/pysixd/pose_error.py:131-179) of N estimates: [N,2] fp64 device tensor, column 0 MSSD in the unit of the
    points, column 1 MSPD in pixels, each the minimum over the symmetry transformations of the class.  R_* [N,3,3], t_* [N,3], K [N,3,3] or [3,3]:
    device tensors, fp32 or fp64; labels [N]: class per row.  A NaN pose gives NaN."""
    R_est, t_est, K, N = devargs.poses(R_est, t_est, K, WHERE)
    R_gt, t_gt = _gt_poses(R_gt, t_gt, N)
    dev = R_est.device
    lab, lab_host = devargs.index_vector(labels, N, table.num_classes, dev, "labels")
    lib = cabi.load()
    tb = table.on(dev)
    err = torch.empty(max(N, 1), 2, dtype=torch.float64, device=dev)[:N]
    ws = devargs.workspace(lib.gdrn_mssd_mspd_workspace_bytes(N, table.n_max, table.s_max), dev, "mssd_mspd_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_mssd_mspd(p(R_est), p(t_est), p(R_gt), p(t_gt), p(K), p(lab), lab_host.ctypes.data, N, p(tb["pts"]), p(tb["npts"]),
                                  table.n_max, p(tb["sym_R"]), p(tb["sym_t"]), p(tb["nsym"]), table.s_max, table.num_classes, p(err), p(ws),
                                  devargs.stream(dev)), "mssd_mspd")
    return err


def average_recall(obj_names, hits_vsd, hits_mssd, hits_mspd, seen):
    """AR from per-class counters (host arrays): per object with seen > 0 and over all targets ("all": hits and targets summed over the classes,
    as score.calc_localization_scores counts them) -- ``AR_VSD`` = the mean of the T x 10 recalls, ``AR_MSSD`` / ``AR_MSPD`` the mean of the 10,
    ``AR`` the mean of the three, as floats; ``rows``: a tabulate-ready list (header, one row per object sorted by name, the "all" row)."""
    hv, hs, hp = (np.asarray(a, dtype=np.int64) for a in (hits_vsd, hits_mssd, hits_mspd))
    seen = np.asarray(seen, dtype=np.int64)

    def ar(v, s, p, n):
        a = {"AR_VSD": float(np.mean(v / float(n))), "AR_MSSD": float(np.mean(s / float(n))), "AR_MSPD": float(np.mean(p / float(n)))}
        a["AR"] = (a["AR_VSD"] + a["AR_MSSD"] + a["AR_MSPD"]) / 3.0
        return a

    out = {"objects": {name: ar(hv[c], hs[c], hp[c], seen[c]) for c, name in enumerate(obj_names) if seen[c] > 0}}
    total = int(seen.sum())
    keys = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")
    out["all"] = ar(hv.sum(0), hs.sum(0), hp.sum(0), total) if total > 0 else {k: float("nan") for k in keys}
    out["targets"] = total
    rows = [["objects"] + list(keys)]
    for name in sorted(out["objects"]):
        rows.append([name] + [f"{100 * out['objects'][name][k]:.2f}" for k in keys])
    rows.append([f"all({total})"] + [f"{100 * out['all'][k]:.2f}" for k in keys])
    out["rows"] = rows
    return out


class BopRecall:
    """The toolkit's score pass on the device: ``update`` adds a batch of errors (``vsd`` [N,T] from ``vsd`` / ``vsd_from_depth``, ``mssd_mspd`` [N,2])
    to per-class hit counters under the ten thresholds of each error without reading anything back, ``add_missing`` counts ground-truth targets
    that got no estimate (a miss under every threshold), ``summarize`` makes the one device-to-host copy and returns ``average_recall``'s dict.
    ``im_width``: the test images' width (MSPD is scaled by 640 / im_width, eval_calc_scores.py:248)."""

    def __init__(self, table, obj_names, im_width, taus=VSD_TAUS):
        if len(obj_names) != table.num_classes:
            raise ValueError("one name per class of the table")
        self.table, self.obj_names, self.im_width = table, list(obj_names), float(im_width)
        self.T = int(np.asarray(taus).reshape(-1).shape[0])
        if not 1 <= self.T <= MAX_TAUS or not self.im_width > 0:
            raise ValueError((self.T, self.im_width))
        self._state = None
        self._ths = None

    def _views(self, state):
        C, T = self.table.num_classes, self.T
        a, b, c = C * T * NTH, C * T * NTH + C * NTH, C * T * NTH + 2 * C * NTH
        return dict(hits_vsd=state[:a], hits_mssd=state[a:b], hits_mspd=state[b:c], seen=state[c : c + C])

    def _on(self, device):
        """one flat int64 buffer [hits_vsd C*T*10 | hits_mssd C*10 | hits_mspd C*10 | seen C]: one copy brings all of it to the host"""
        if self._state is None:
            C = self.table.num_classes
            self._state = torch.zeros(C * (self.T * NTH + 2 * NTH + 1), dtype=torch.int64, device=device)
            self._ths = torch.from_numpy(np.stack([VSD_THS, MSSD_THS, MSPD_THS]).astype(np.float64)).to(device)
        elif self._state.device != torch.device(device):
            raise ValueError(f"the counters live on {self._state.device}")
        return self._views(self._state)

    def update(self, vsd, mssd_mspd, labels):
        vsd = devargs.device_tensor(vsd, torch.float64, None, "vsd", "the BOP recall")
        mssd_mspd = devargs.device_tensor(mssd_mspd, torch.float64, None, "mssd_mspd", "the BOP recall")
        N = int(vsd.shape[0])
        if vsd.dim() != 2 or vsd.shape[1] != self.T or tuple(mssd_mspd.shape) != (N, 2):
            raise ValueError(f"vsd is [N,{self.T}], mssd_mspd [N,2]")
        dev = vsd.device
        lab, lab_host = devargs.index_vector(labels, N, self.table.num_classes, dev, "labels")
        v, tb = self._on(dev), self.table.on(dev)
        p = cabi.ptr
        cabi.check(cabi.load().gdrn_bop_recall_accumulate(p(vsd), self.T, p(mssd_mspd), p(lab), lab_host.ctypes.data, N, p(tb["diameter"]),
                                                          self.table.num_classes, self.im_width, p(self._ths[0]), p(self._ths[1]), p(self._ths[2]),
                                                          p(v["hits_vsd"]), p(v["hits_mssd"]), p(v["hits_mspd"]), p(v["seen"]),
                                                          devargs.stream(dev)), "bop_recall_accumulate")

    def add_missing(self, label, count=1, device=None):
        if not 0 <= int(label) < self.table.num_classes or int(count) < 0:
            raise ValueError((label, count))
        if self._state is None and device is None:
            raise cabi.GdrnHipError("add_missing before the first update needs the device of the counters")
        self._on(device if self._state is None else self._state.device)["seen"][int(label)] += int(count)

    def counters(self):
        """host copies of the counters (the one device-to-host copy): hits_vsd [C,T,10], hits_mssd, hits_mspd [C,10], seen [C], int64"""
        C = self.table.num_classes
        host = torch.zeros(C * (self.T * NTH + 2 * NTH + 1), dtype=torch.int64) if self._state is None else self._state.cpu()
        v = {k: t.numpy() for k, t in self._views(host).items()}
        v["hits_vsd"] = v["hits_vsd"].reshape(C, self.T, NTH)
        v["hits_mssd"], v["hits_mspd"] = v["hits_mssd"].reshape(C, NTH), v["hits_mspd"].reshape(C, NTH)
        return v

    def summarize(self):
        return average_recall(self.obj_names, **self.counters())

    def reset(self):
        if self._state is not None:
            self._state.zero_()
