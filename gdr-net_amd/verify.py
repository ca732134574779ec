"""Hypothesis verification on the device (csrc/verify.hip): which candidate pose explains the observed depth frame and instance mask best.

The RGB-D chain produces several candidates per detection -- the network's regression, ``pnp.poses_from_maps``, ``rigid.poses_from_maps_rgbd``
with any number of seeds, each of them after ``refine.refine_rgbd`` -- and ``icp_refine``'s rms covers only the pairs that passed its own gates.
Here every candidate is rendered and every pixel its render covers is classed against the observation: *inlier* (within ``tau``), *occluded* (the
observation is nearer), *violated* (the observation is farther: the model claims a surface in measured free space) or *unknown* (no measurement).
The score is the truncated-linear fit of the inliers, scaled by the IoU of the visible render with the observed mask, minus ``penalty`` per
violated pixel, over the covered pixels; ``select_best`` picks the highest score per detection.  The arithmetic is stated with the entry points
in ``include/gdrn_hip.h``: the counts are integers, the score one fixed fp64 operation sequence, so the same call gives the same bits and the rows
of a batch do not influence each other.  The reference is RGB-only and has no counterpart.  Nothing is read back; there is no CPU fallback.

``tau`` (0.01 m), ``penalty`` (1.0) and ``min_covered`` (64 pixels) are parameters: none of them is measured on real data.  ``tau`` must exceed the
depth noise of the sensor and the residual of a good pose and stay below the error that is to be told apart.
"""
import numpy as np
import torch

from . import cabi, devargs, render
from .refine import _Loop, _call, _mask, _renders, _scene

WHERE = "the verification"   # (this module in devargs' error sentence)

COUNTS = ("covered", "inlier", "occluded", "violated", "unknown", "visible", "mask_px", "inter")   # the columns of the library's counts [N][8]
KEYS = COUNTS + ("sum_q", "score", "ok")


def _scalars(tau, penalty, min_covered):
    tau, penalty, min_covered = float(tau), float(penalty), int(min_covered)
    if not 0.0 < tau <= 1.0:
        raise ValueError(f"tau {tau} (metres) must lie in (0, 1]")
    if not 0.0 <= penalty < float("inf"):
        raise ValueError(f"penalty {penalty} must be finite and >= 0")
    if min_covered < 1:
        raise ValueError(f"min_covered {min_covered} must be >= 1")
    return tau, penalty, min_covered


def _mask_meta(mask_obs, mask_index, N):
    """what can be said about the mask arguments before the device is looked at: the dtype, the rank, and the rows of a mask without an index"""
    if mask_obs is None and mask_index is not None:
        raise ValueError("mask_index without mask_obs")
    if not isinstance(mask_obs, torch.Tensor):
        return
    if mask_obs.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask_obs is {mask_obs.dtype}: torch.uint8 or torch.bool (nonzero = object)")
    if mask_obs.dim() != 3:
        raise ValueError(f"mask_obs {tuple(mask_obs.shape)} must be [M, H, W]")
    if mask_index is None and N is not None and mask_obs.shape[0] != N:
        raise ValueError(f"mask_obs {tuple(mask_obs.shape)} has {mask_obs.shape[0]} rows for {N} candidates: one per candidate, or a mask_index")


def _mask_args(mask_obs, mask_index, scene, N):
    """(has_mask, the four mask arguments of the library as a function of ``cabi.ptr``, what must stay alive)"""
    if mask_obs is None:
        return False, lambda p: (None, None, None, 0), ()
    m = _mask(mask_obs, scene, N if mask_index is None else None)
    M = int(m.shape[0])
    if mask_index is None:
        return True, lambda p: (p(m), None, None, M), (m,)
    mi, mi_host = devargs.index_vector(mask_index, N, M, m.device, "mask_index")
    return True, lambda p: (p(m), p(mi), mi_host.ctypes.data, M), (m, mi, mi_host)


def _outputs(N, dev):
    return dict(counts=torch.empty(N, len(COUNTS), dtype=torch.int32, device=dev), sum_q=torch.empty(N, dtype=torch.int64, device=dev),
                score=torch.empty(N, dtype=torch.float64, device=dev), ok=torch.empty(N, dtype=torch.int32, device=dev))


def _result(o):
    out = {k: o["counts"][:, j].contiguous() for j, k in enumerate(COUNTS)}
    out.update(sum_q=o["sum_q"], score=o["score"], ok=o["ok"])
    return out


def verify_maps(depth_ren, depth_scene, frame, mask_obs=None, mask_index=None, tau=0.01, penalty=1.0, min_covered=64):
    """Count and score N candidates on given renders: ``depth_ren`` [N,H,W] fp32 (e.g. ``render.render_depth``'s), ``depth_scene`` [F,H,W] fp32
    (metres; 0, negative or non-finite = no measurement), ``frame`` [N]; ``mask_obs`` [M,H,W] uint8 or bool on the device (nonzero = object)
    with ``mask_index`` [N], the mask of each candidate -- the candidates of one detection share one mask; without ``mask_index``, ``mask_obs``
    must have N rows.  Returns a dict of device tensors [N]: covered, inlier, occluded, violated, unknown, visible, mask_px, inter (int32),
    sum_q (int64), score (fp64; -inf where ok is 0) and ok (int32; 0: fewer than ``min_covered`` covered pixels).  ``tau``, ``penalty`` and
    ``min_covered`` are parameters; their defaults are not measured on real data."""
    tau, penalty, min_covered = _scalars(tau, penalty, min_covered)
    _mask_meta(mask_obs, mask_index, int(depth_ren.shape[0]) if isinstance(depth_ren, torch.Tensor) and depth_ren.dim() == 3 else None)
    ren, scene = _renders(depth_ren, depth_scene)
    N, H, W = (int(s) for s in ren.shape)
    dev, F = ren.device, int(scene.shape[0])
    has_mask, margs, _keep = _mask_args(mask_obs, mask_index, scene, N)
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    o = _outputs(N, dev)
    if N > 0:
        _call(lambda lib: (lib.gdrn_verify_maps, lib.gdrn_verify_workspace_bytes), N, H, W, dev,
              lambda p: (p(ren), p(scene), p(fr), fr_host.ctypes.data, F, *margs(p), N, H, W, tau, p(o["counts"]), p(o["sum_q"])))
        cabi.check(cabi.load().gdrn_verify_score(cabi.ptr(o["counts"]), cabi.ptr(o["sum_q"]), N, int(has_mask), tau, penalty, min_covered,
                                                 cabi.ptr(o["score"]), cabi.ptr(o["ok"]), devargs.stream(dev)), "verify_score")
    return _result(o)


def verify_poses(meshes, labels, R, t, K, depth_scene, frame, mask_obs=None, mask_index=None, tau=0.01, penalty=1.0, min_covered=64,
                 near=render.NEAR, far=render.FAR):
    """``verify_maps`` from poses: ``meshes`` a ``render.MeshTable``, ``labels`` [N], ``R`` [N,3,3], ``t`` [N,3], ``K`` [N,3,3] or [3,3] as
    ``refine.icp_refine`` takes them; the N candidates are rendered (``render.render_depth``'s launch), counted and scored on the current stream
    without a host read.  The same bits as ``render_depth`` followed by ``verify_maps``.  The caller's tensors stay."""
    tau, penalty, min_covered = _scalars(tau, penalty, min_covered)
    _mask_meta(mask_obs, mask_index, R.numel() // 9 if isinstance(R, torch.Tensor) else None)
    c = _Loop(meshes, labels, R, t, K, depth_scene, frame)
    has_mask, margs, _keep = _mask_args(mask_obs, mask_index, c.scene, c.N)
    o = _outputs(c.N, c.dev)
    if c.N > 0:
        c.run(lambda lib: (lib.gdrn_verify_poses, lib.gdrn_verify_workspace_bytes), c.R, c.t, near, far,
              (*margs(cabi.ptr), tau, penalty, min_covered), (o["counts"], o["sum_q"], o["score"], o["ok"]))
    return _result(o)


def select_best(score, ok, group, num_groups):
    """The best row of every group: ``score`` [N] fp64 and ``ok`` [N] int32 on the device (``verify_maps``'), ``group`` [N] with values in
    [0, ``num_groups``).  Per group the row with the highest score among those with ok != 0 (a NaN score is never picked); ties go to the
    lowest row.  Returns a dict of device tensors: best [G] int32 (-1 for a group without such a row) and best_score [G] fp64 (-inf there)."""
    G = int(num_groups)
    if G < 0:
        raise ValueError(f"num_groups {G} must be >= 0")
    score = devargs.device_tensor(score, torch.float64, (-1,), "score", WHERE)
    ok = devargs.device_tensor(ok, torch.int32, (-1,), "ok", WHERE)
    N, dev = int(score.shape[0]), score.device
    if ok.shape[0] != N or ok.device != dev:
        raise ValueError("score and ok need one entry per row on one device")
    gr, gr_host = devargs.index_vector(group, N, G, dev, "group")
    out = dict(best=torch.empty(G, dtype=torch.int32, device=dev), best_score=torch.empty(G, dtype=torch.float64, device=dev))
    if G > 0:
        p = cabi.ptr
        cabi.check(cabi.load().gdrn_verify_select(p(score), p(ok), p(gr), gr_host.ctypes.data, N, G, p(out["best"]), p(out["best_score"]),
                                                  devargs.stream(dev)), "verify_select")
    return out


def best_of(meshes, labels, candidates, K, depth_scene, frame, mask_obs=None, tau=0.01, penalty=1.0, min_covered=64, near=render.NEAR,
            far=render.FAR):
    """Verify C candidate poses for each of M detections and keep the best: ``candidates`` a sequence of C pairs (R [M,3,3], t [M,3]) for the
    same M detections, ``labels``, ``frame`` [M], ``K`` [M,3,3] or [3,3], ``mask_obs`` [M,H,W] the observed mask of each detection (or None).
    The C M rows (candidate-major) go through ``verify_poses`` with the detection as mask index and ``select_best`` with the detection as group.
    Returns a dict of device tensors: R [M,3,3], t [M,3] fp64 (the winner's; candidate 0's where no candidate is ok), which [M] int32 (the
    winning candidate, -1 without one), score [M] fp64 (-inf there), and ``all``: the dict of ``verify_poses`` reshaped to [C,M].  The gather is
    a device operation; nothing is read back.  Without a candidate (C = 0) R and t are NaN, which is -1 and ``all`` is [0,M]."""
    scalars = _scalars(tau, penalty, min_covered)
    cands = list(candidates)
    C = len(cands)
    scene = _scene(depth_scene)
    dev, F = scene.device, int(scene.shape[0])
    if C == 0:
        M = len(devargs.index_vector(frame, None, F, dev, "frame")[1])
        nan = float("nan")
        empty = _result(_outputs(0, dev))
        return dict(R=torch.full((M, 3, 3), nan, dtype=torch.float64, device=dev), t=torch.full((M, 3), nan, dtype=torch.float64, device=dev),
                    which=torch.full((M,), -1, dtype=torch.int32, device=dev),
                    score=torch.full((M,), float("-inf"), dtype=torch.float64, device=dev), all={k: v.reshape(0, M) for k, v in empty.items()})
    rows = [devargs.poses(R, t, K, WHERE) for R, t in cands]
    M = rows[0][3]
    if any(r[3] != M for r in rows):
        raise ValueError("every candidate needs one pose per detection")
    R_all, t_all, K_all = (torch.cat([r[j] for r in rows]) for j in range(3))
    tile = lambda v, bound, what: np.tile(devargs.index_vector(v, M, bound, dev, what)[1], C)  # noqa: E731
    lab, fr, det = tile(labels, meshes.num_classes, "labels"), tile(frame, F, "frame"), np.tile(np.arange(M, dtype=np.int32), C)
    res = verify_poses(meshes, lab, R_all, t_all, K_all, scene, fr, mask_obs, None if mask_obs is None else det, *scalars, near=near, far=far)
    sel = select_best(res["score"], res["ok"], det, M)
    best = sel["best"].to(torch.int64)
    keep = torch.where(best < 0, torch.arange(M, dtype=torch.int64, device=dev), best)   # candidate 0 of the detection: row m
    which = torch.div(sel["best"], max(M, 1), rounding_mode="floor").to(torch.int32)      # (-1 stays -1)
    return dict(R=R_all[keep], t=t_all[keep], which=which, score=sel["best_score"], all={k: v.reshape(C, M) for k, v in res.items()})
