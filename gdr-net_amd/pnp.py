"""Batched PnP-RANSAC and iterative PnP on the device (csrc/pnp.hip) for ``cfg.TEST.USE_PNP``.

Host-side mirror of the step the reference's evaluator runs per RoI on the CPU with OpenCV, between the 2D-3D correspondences
(``gdrnet_amd.postproc``) and the pose metrics (``gdrnet_amd.pose_metrics``):

* ``GDRN_Evaluator.process_pnp_ransac``                 -- core/gdrn_modeling/gdrn_evaluator.py:316-392 -> lib/pysixd/misc.py:145-194
* ``process_net_and_pnp``, ``pnp_type`` "ransac" / "iter"  -- gdrn_evaluator.py:187-307

i.e. ``cfg.TEST.PNP_TYPE = ransac_pnp | net_ransac_pnp | net_iter_pnp``, for a whole batch per call and without a host loop.  All pose arithmetic
is fp64.  This is NOT cv2's algorithm: a fixed hypothesis count instead of the 0.99-confidence early stop, P3P + least-squares refinement instead
of EPnP, a counter-based hash instead of cv2's RNG -- the results are pinned to geometry (known poses) and to an independent fp64 host
computation, not to cv2 output.  There is no CPU fallback.
"""
import torch

from . import cabi, devargs, postproc

WHERE = "PnP"   # (this module in devargs' error sentence)


def _inputs(image_points, model_points, counts, K):
    """contiguous correspondences (fp64 stays fp64, everything else becomes fp32 -- what gdrn_correspondences writes), the counts on both sides
    (checked against the stride on the host, before anything is loaded or launched) and K [N,3,3] fp64"""
    for name, v in (("image_points", image_points), ("model_points", model_points), ("K", K)):
        if not isinstance(v, torch.Tensor):
            raise devargs.no_fallback(name, WHERE)
    img, mod = image_points.detach(), model_points.detach()
    if img.dim() != 3 or mod.dim() != 3 or img.shape[2] != 2 or mod.shape[2] != 3 or img.shape[:2] != mod.shape[:2]:
        raise ValueError(f"image_points [N,S,2] and model_points [N,S,3] expected, got {tuple(img.shape)} and {tuple(mod.shape)}")
    N, S = int(img.shape[0]), int(img.shape[1])
    if N <= 0 or S <= 0:
        raise ValueError("empty batch")
    cnt, host = devargs.index_vector(counts, N, S, img.device, "counts", inclusive=True)
    K = devargs.per_row_K(K.detach().to(torch.float64), N)
    dt = torch.float64 if img.dtype == torch.float64 and mod.dtype == torch.float64 else torch.float32
    # (after the checks that need no device: a bad call fails the same everywhere)
    img, mod = devargs.device_tensor(img, dt, None, "image_points", WHERE), devargs.device_tensor(mod, dt, None, "model_points", WHERE)
    return img, mod, cnt, host, devargs.device_tensor(K, None, None, "K", WHERE), N, S, dt == torch.float64


def _pose0(R0, t0, N, dev):
    """fresh fp64 copies of the caller's initial pose (identity / zero without one): the kernels update them in place"""
    if R0 is None:
        R = torch.eye(3, dtype=torch.float64, device=dev).repeat(N, 1, 1)
    else:
        R = devargs.device_tensor(R0, torch.float64, (-1, 3, 3), "R0", WHERE).clone()
    if t0 is None:
        t = torch.zeros(N, 3, dtype=torch.float64, device=dev)
    else:
        t = devargs.device_tensor(t0, torch.float64, (-1, 3), "t0", WHERE).clone()
    if R.shape[0] != N or t.shape[0] != N:
        raise ValueError(f"R0 / t0 need one entry per RoI ({N})")
    return R, t


def pnp_ransac(image_points, model_points, counts, K, reproj_err=3.0, iters=100, seed=0, R0=None, t0=None, want_mask=False, max_iter=20):
    """RANSAC (``iters`` P3P hypotheses per RoI, gate ``reproj_err`` pixels) + least-squares refinement on the inliers, for N RoIs in one call.
    image_points [N,S,2], model_points [N,S,3] (fp32, or both fp64), counts [N] (only the first counts[n] rows of RoI n are read), K [N,3,3] or
    [3,3]: device tensors.  Returns a dict of device tensors: R [N,3,3], t [N,3] fp64, ok [N] int32 (0: not solvable -- R, t are R0, t0, identity /
    zero without them), num_inliers [N] int32, rms [N] fp64 (inliers' root-mean-square pixel distance, NaN where ok is 0) and, with ``want_mask``,
    inlier_mask [N,S] uint8.  The same (seed, inputs) give the same bits on every call."""
    if int(iters) <= 0 or not float(reproj_err) > 0.0 or int(max_iter) <= 0:
        raise ValueError(f"iters, reproj_err and max_iter must be positive, got {iters}, {reproj_err}, {max_iter}")
    img, mod, cnt, host, K, N, S, f64 = _inputs(image_points, model_points, counts, K)
    dev = img.device
    R, t = _pose0(R0, t0, N, dev)
    lib = cabi.load()
    ok = torch.empty(N, dtype=torch.int32, device=dev)
    num = torch.empty(N, dtype=torch.int32, device=dev)
    rms = torch.empty(N, dtype=torch.float64, device=dev)
    mask = torch.empty(N, S, dtype=torch.uint8, device=dev) if want_mask else None
    ws = devargs.workspace(lib.gdrn_pnp_workspace_bytes(N, S, int(iters)), dev, "pnp_workspace_bytes")
    st = devargs.stream(dev)
    fn = lib.gdrn_pnp_ransac_f64 if f64 else lib.gdrn_pnp_ransac
    cabi.check(fn(cabi.ptr(img), cabi.ptr(mod), cabi.ptr(cnt), host.ctypes.data, cabi.ptr(K), N, S, float(reproj_err), int(iters),
                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_iter), cabi.ptr(R), cabi.ptr(t), cabi.ptr(ok), cabi.ptr(num), cabi.ptr(mask), cabi.ptr(rms),
                  cabi.ptr(ws), st), "pnp_ransac")
    out = dict(R=R, t=t, ok=ok, num_inliers=num, rms=rms)
    if want_mask:
        out["inlier_mask"] = mask
    return out


def pnp_refine(image_points, model_points, counts, K, R0, t0, max_iter=20):
    """Least-squares pose from the caller's (R0, t0) over all valid points of each RoI, no inlier gate (cv2.solvePnP, SOLVEPNP_ITERATIVE with
    useExtrinsicGuess).  Returns a dict of device tensors: R, t, ok (0: fewer than 4 points or a non-finite result -- R, t are R0, t0), rms."""
    if int(max_iter) <= 0:
        raise ValueError(f"max_iter must be positive, got {max_iter}")
    img, mod, cnt, host, K, N, S, f64 = _inputs(image_points, model_points, counts, K)
    dev = img.device
    R, t = _pose0(R0, t0, N, dev)
    lib = cabi.load()
    ok = torch.empty(N, dtype=torch.int32, device=dev)
    rms = torch.empty(N, dtype=torch.float64, device=dev)
    st = devargs.stream(dev)
    fn = lib.gdrn_pnp_refine_f64 if f64 else lib.gdrn_pnp_refine
    cabi.check(fn(cabi.ptr(img), cabi.ptr(mod), cabi.ptr(cnt), host.ctypes.data, cabi.ptr(K), N, S, int(max_iter), cabi.ptr(R), cabi.ptr(t),
                  cabi.ptr(ok), cabi.ptr(rms), None, st), "pnp_refine")
    return dict(R=R, t=t, ok=ok, rms=rms)


PNP_TYPES = ("ransac_pnp", "net_iter_pnp", "net_ransac_pnp")


def poses_from_maps(cfg, out_dict, roi_coord_2d, roi_extents, im_H, im_W, K, pnp_type=None, seed=0):
    """The evaluator's PnP branches for a whole batch: ``postproc.get_img_model_points_with_coords2d`` followed by the solver.  Returns pose_est
    [N,3,4] fp64 on the device.  ``pnp_type`` (default cfg.TEST.PNP_TYPE):

    * ``ransac_pnp``      process_pnp_ransac: 100 hypotheses, 3 px; a RoI with fewer than 4 points (or none solvable) is -100 everywhere (:393-395)
    * ``net_ransac_pnp``  process_net_and_pnp, "ransac": 20 hypotheses, 3 px, from out_dict["rot"] / ["trans"]
    * ``net_iter_pnp``    process_net_and_pnp, "iter": least squares over all points from out_dict["rot"] / ["trans"]

    For the net_* types a RoI with fewer than 4 points keeps the network's pose, and one whose translation moved more than 1 (metre) away from
    the network's keeps the network's translation (:293-296).  Anything else raises NotImplementedError, as ``process`` does."""
    kind = (cfg.TEST.PNP_TYPE if pnp_type is None else pnp_type).lower()
    if kind not in PNP_TYPES:
        raise NotImplementedError(f"unknown pnp type on the MI355X path: {kind}")
    _, _, img, mod, counts = postproc.get_img_model_points_with_coords2d(cfg, out_dict, roi_coord_2d, roi_extents, im_H, im_W)
    N, dev = img.shape[0], img.device
    K = devargs.device_tensor(torch.as_tensor(K), None, None, "K", WHERE)
    if kind == "ransac_pnp":
        res = pnp_ransac(img, mod, counts, K, reproj_err=3.0, iters=100, seed=seed)
        pose = torch.cat([res["R"], res["t"].unsqueeze(2)], dim=2)
        return torch.where(res["ok"].bool().view(N, 1, 1), pose, torch.full_like(pose, -100.0))
    R_net = devargs.device_tensor(out_dict["rot"], torch.float64, (N, 3, 3), "rot", WHERE)
    t_net = devargs.device_tensor(out_dict["trans"], torch.float64, (N, 3), "trans", WHERE)
    if kind == "net_ransac_pnp":
        res = pnp_ransac(img, mod, counts, K, reproj_err=3.0, iters=20, seed=seed, R0=R_net, t0=t_net)
    else:
        res = pnp_refine(img, mod, counts, K, R_net, t_net)
    far = (res["t"] - t_net).norm(dim=1) > 1.0
    t = torch.where(far.view(N, 1), t_net, res["t"])
    return torch.cat([res["R"], t.unsqueeze(2)], dim=2)
