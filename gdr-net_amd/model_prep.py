"""Model preparation on the device: the per-object tables the other modules take as constructor arguments, from the vertices of the meshes.

In the reference these tables are files written by offline passes on the host: ``fps_points.pkl`` (tools/lm/1_compute_fps.py and its lmo / ycbv
twins: ``get_fps_and_center``, core/utils/data_utils.py:201-210, nine times per object through the compiled extension core/csrc/fps), the
diameters of ``models_info.json`` (``misc.calc_pts_diameter``, lib/pysixd/misc.py:952-966, an O(n^2) Python loop) and the extents of the per-object
loop in core/gdrn_modeling/data_loader.py:243-276.  ``prepare_models`` computes them for all objects of a dataset in one pass (csrc/model_prep.hip):

    prep = prepare_models([m["pts"] for m in models])
    RoiCropper(cfg, extents=prep.extents, fps_points=prep.fps_points(64))
    ModelTable(points, prep.diameters) / BopModelTable(points, prep.diameters, syms)

What the results are pinned to: the farthest-point-sampling (FPS) indices are the reference's own with ``init_center=True`` -- deterministic fp32
arithmetic with a first-index-wins arg-max -- bit for bit; the diameter is the same fp64 maximum; minimum, maximum and extents are exact; the mean
is an fp64 sum in a fixed order (within n * 2^-52 * max|x| of the exact mean, as numpy's is).  ``init_center=False`` starts from ``rand()`` seeded
with the clock in the reference and cannot be reproduced: it raises ``NotImplementedError``.  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import cabi, devargs

WHERE = "model preparation"
NUM_FPS = (4, 8, 12, 16, 20, 32, 64, 128, 256)   # the entries of the reference's fps_points.pkl


class _Models(devargs.DeviceTables):
    """the packed vertices [C, n_max, 3] fp64 with their counts, uploaded once per device"""

    TABLES = ("pts", "npts")

    def __init__(self, clouds, pad_value):
        self.num_classes = len(clouds)
        self.pts, self.npts, self.n_max, _ = devargs.pack_points(clouds, np.zeros(len(clouds)), pad_value)


class ModelPrep:
    """The tables of C objects as numpy arrays.  ``bounds_min`` / ``bounds_max`` / ``centers`` [C,3] fp64 (the mean of the vertices),
    ``fps_indices`` [C,Kmax] int32, ``fps_xyz`` [C,Kmax,3] fp64 (the fp32-rounded vertices at those indices: ``pts[idxs]`` of the fp32 array the
    reference samples), ``num_fps`` the requested counts, ``max_sq_dist`` [C] fp64 or None (``diameter=False``)."""

    def __init__(self, bounds_min, bounds_max, centers, fps_indices, fps_xyz, num_fps, max_sq_dist=None):
        self.bounds_min = np.asarray(bounds_min, dtype=np.float64).reshape(-1, 3)
        self.bounds_max = np.asarray(bounds_max, dtype=np.float64).reshape(-1, 3)
        self.centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
        C = len(self.centers)
        self.fps_indices = np.asarray(fps_indices, dtype=np.int32).reshape(C, -1)
        self.fps_xyz = np.asarray(fps_xyz, dtype=np.float64).reshape(C, -1, 3)
        self.num_fps = tuple(int(k) for k in num_fps)
        self.max_sq_dist = None if max_sq_dist is None else np.asarray(max_sq_dist, dtype=np.float64).reshape(C)
        if self.bounds_min.shape != (C, 3) or self.bounds_max.shape != (C, 3) or self.fps_xyz.shape[1] != self.fps_indices.shape[1]:
            raise ValueError("one row per object in every table")

    @property
    def num_classes(self):
        return len(self.centers)

    @property
    def extents(self):
        """[C,3] float32: max - min per axis, cast as ``_get_extents`` casts it"""
        return (self.bounds_max - self.bounds_min).astype(np.float32)

    @property
    def diameters(self):
        """[C] fp64: ``math.sqrt`` of the largest squared distance, as ``calc_pts_diameter`` takes it"""
        if self.max_sq_dist is None:
            raise ValueError("prepare_models(..., diameter=False) skipped the diameters")
        return np.array([math.sqrt(v) for v in self.max_sq_dist], dtype=np.float64)

    @property
    def bbox3d_and_center(self):
        """[C,9,3] float32: the eight corners in the order of ``misc.get_bbox3d_and_center``, then the mean"""
        lo, hi = self.bounds_min, self.bounds_max
        pick = lambda x, y, z: np.stack([(hi if x else lo)[:, 0], (hi if y else lo)[:, 1], (hi if z else lo)[:, 2]], axis=1)  # noqa: E731
        rows = [pick(1, 1, 1), pick(0, 1, 1), pick(0, 0, 1), pick(1, 0, 1), pick(1, 1, 0), pick(0, 1, 0), pick(0, 0, 0), pick(1, 0, 0), self.centers]
        return np.stack(rows, axis=1).astype(np.float32)

    def fps_points(self, k, with_center=False):
        """[C,k,3] fp64: the first ``k`` FPS points of every object (the sequence for k is a prefix of the one for any larger k); with
        ``with_center`` [C,k+1,3], the mean appended as ``get_fps_and_center`` appends it"""
        k = int(k)
        if not 1 <= k <= self.fps_xyz.shape[1]:
            raise ValueError(f"{k} FPS points of {self.fps_xyz.shape[1]} computed")
        pts = self.fps_xyz[:, :k]
        return np.concatenate([pts, self.centers[:, None]], axis=1) if with_center else pts.copy()

    def fps_dict(self, obj_ids):
        """``{str(obj_id): {"fps4_and_center": [5,3], ...}}``: the layout of the reference's fps_points.pkl, one entry per requested count"""
        obj_ids = list(obj_ids)
        if len(obj_ids) != self.num_classes:
            raise ValueError("one id per object")
        tabs = {k: self.fps_points(k, with_center=True) for k in self.num_fps}
        return {str(o): {f"fps{k}_and_center": tabs[k][c] for k in self.num_fps} for c, o in enumerate(obj_ids)}


def check_models(points, num_fps=NUM_FPS, init_center=True):
    """the host-side argument checks of ``prepare_models``: ([n_c,3] fp64 arrays, the sorted counts)"""
    if not init_center:
        raise NotImplementedError("init_center=False starts from rand() seeded with the clock in the reference: it cannot be reproduced "
                                  "(only the init_center=True sequence, the one every shipped fps_points.pkl was made with, is computed)")
    num_fps = tuple(int(k) for k in (num_fps if np.ndim(num_fps) else (num_fps,)))
    if not num_fps or min(num_fps) < 1:
        raise ValueError(f"num_fps {num_fps}: every count must be at least 1")
    clouds = []
    for c, p in enumerate(points):
        p = np.asarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"object {c}: vertices of shape {p.shape}, expected [n,3]")
        if p.shape[0] < 1:
            raise ValueError(f"object {c} has no vertices")
        p = np.ascontiguousarray(p, dtype=np.float64)
        with np.errstate(over="ignore"):
            finite = np.isfinite(p.astype(np.float32)).all()
        if not finite:
            raise ValueError(f"object {c}: a vertex is not finite in fp32")
        clouds.append(p)
    if not clouds:
        raise ValueError("no objects")
    if max(len(p) for p in clouds) * 3 >= 2 ** 31:
        raise ValueError("an object with n * 3 >= 2**31 coordinates")
    return clouds, tuple(sorted(set(num_fps)))


def prepare_models(points, num_fps=NUM_FPS, diameter=True, device="cuda", init_center=True, pad_value=0.0, lib=None):
    """``points``: per object an [n_c,3] array of vertices (any float type; list / numpy / tensor).  One upload of the packed vertices, the three
    stages on the current stream (bounds; FPS, one run at the largest of ``num_fps``; the O(n^2) diameter unless ``diameter`` is False) and one
    device-to-host copy of all results: a ``ModelPrep``.  ``pad_value`` fills the packed rows beyond an object's own vertices; the kernels never
    read them.  An empty object, a non-[n,3] array or a count below 1 raises ``ValueError``, a CPU device ``cabi.GdrnHipError``."""
    clouds, num_fps = check_models(points, num_fps, init_center)
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise devargs.no_fallback(f"the target device '{device}'", WHERE)
    device = torch.device("cuda", torch.cuda.current_device()) if device.index is None else device
    lib = lib or cabi.load()
    models = _Models(clouds, pad_value)
    tb = models.on(device)
    C, n_max, K = models.num_classes, models.n_max, num_fps[-1]
    ws = devargs.workspace(lib.gdrn_model_prep_workspace_bytes(C, n_max, K), device, "model_prep_workspace_bytes")
    # one buffer for everything that is read back: [C,9] bounds | [C] largest squared distance | [C,K,3] FPS points | [C,K] int32 indices
    nd = C * (9 + 1 + 3 * K)
    out = torch.zeros(nd + (C * K + 1) // 2, dtype=torch.float64, device=device)
    bounds, max_sq, xyz = out[:C * 9], out[C * 9:C * 10], out[C * 10:nd]
    idx = out[nd:].view(torch.int32)
    st, p = devargs.stream(device), cabi.ptr
    args = (p(tb["pts"]), p(tb["npts"]), models.npts.ctypes.data, C, n_max)
    with torch.cuda.device(device):
        cabi.check(lib.gdrn_model_bounds(*args, p(bounds), st), "model_bounds")
        cabi.check(lib.gdrn_model_fps(*args, K, p(idx), p(xyz), p(ws), st), "model_fps")
        if diameter:
            cabi.check(lib.gdrn_model_diameter(*args, p(max_sq), st), "model_diameter")
    host = out.cpu().numpy()   # the one device-to-host copy
    b = host[:C * 9].reshape(C, 9)
    return ModelPrep(b[:, 0:3], b[:, 3:6], b[:, 6:9], host[nd:].view(np.int32)[:C * K].reshape(C, K), host[C * 10:nd].reshape(C, K, 3), num_fps,
                     host[C * 9:C * 10].copy() if diameter else None)
