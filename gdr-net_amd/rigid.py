"""Pose from depth and object-coordinate maps on the device (csrc/rigid.hip): batched 3D-3D RANSAC, the RGB-D counterpart of ``cfg.TEST.USE_PNP``.

The network predicts a metric model point for every pixel of the RoI and ``postproc.get_img_model_points_with_coords2d`` extracts them; with a depth
frame each correspondence also has a metric camera point.  From these 3D-3D pairs the pose follows in closed form (Kabsch / Horn) inside a RANSAC:
no render, no iteration, and rotation, lateral position and depth are fixed together -- the start ``refine.depth_align`` / ``refine.icp_refine``
need, which both assume a pose that is already nearly right.

* ``backproject``            -- nearest-pixel depth lookup of every correspondence, valid rows compacted in their input order
* ``rigid_ransac``           -- ``iters`` 3-point hypotheses per RoI, gate ``dist_thr`` metres, refit / re-select / refit on the inliers
* ``rigid_fit``              -- the closed form over all rows, no gate
* ``poses_from_maps_rgbd``   -- the sibling of ``pnp.poses_from_maps``: maps + depth frame -> poses, nothing read back in between

The reference is RGB-only (``WITH_DEPTH=False``) and has no counterpart: the results are pinned to geometry (known poses) and to an independent
fp64 host restatement (tests/rigid_host.py).  All pose arithmetic is fp64, the same call gives the same bits.  There is no CPU fallback.
"""
import torch

from . import cabi, devargs, postproc

WHERE = "the rigid solver"   # (this module in devargs' error sentence)


def _scene(depth_scene):
    """the observed frames, fp32 [F,H,W]: the checks that need no device"""
    if not isinstance(depth_scene, torch.Tensor):
        raise devargs.no_fallback("depth_scene", WHERE)
    if depth_scene.dtype != torch.float32:
        raise ValueError(f"depth_scene is {depth_scene.dtype}: torch.float32 (metres)")
    if depth_scene.dim() != 3 or min(depth_scene.shape) < 1:
        raise ValueError("depth_scene must be [F, H, W] with F, H and W of at least 1")
    return depth_scene.detach()


def _same_device(**tensors):
    """ValueError unless all the given tensors are on one device"""
    names = list(tensors)
    for name in names[1:]:
        if tensors[name].device != tensors[names[0]].device:
            raise ValueError(f"{name} is on {tensors[name].device}, {names[0]} on {tensors[names[0]].device}")


def backproject(image_points, model_points, counts, depth_scene, frame, K):
    """Camera points of 2D-3D correspondences from a depth frame.  image_points [N,S,2] pixels, model_points [N,S,3] (what
    ``postproc.get_img_model_points_with_coords2d`` returns; read as fp32), counts [N] (a device tensor is used as it is: nothing is read back),
    depth_scene [F,H,W] fp32 in metres (0 = no measurement), frame [N] (the frame of each RoI), K [N,3,3] or [3,3].  A row is valid where its
    values are finite and the NEAREST pixel of its (u, v) lies in the frame and holds a finite depth > 0; its camera point is the point of the ray
    through (u, v) itself at that depth.  Returns a dict of device tensors: cam_points, model_points [N,S,3] fp64 with the valid rows first, in
    their input order, and NaN behind them, counts [N] int32."""
    for name, v in (("image_points", image_points), ("model_points", model_points), ("K", K)):
        if not isinstance(v, torch.Tensor):
            raise devargs.no_fallback(name, WHERE)
    img, mod = image_points.detach(), model_points.detach()
    if img.dim() != 3 or mod.dim() != 3 or img.shape[2] != 2 or mod.shape[2] != 3 or img.shape[:2] != mod.shape[:2]:
        raise ValueError(f"image_points [N,S,2] and model_points [N,S,3] expected, got {tuple(img.shape)} and {tuple(mod.shape)}")
    N, S = int(img.shape[0]), int(img.shape[1])
    if N <= 0 or S <= 0:
        raise ValueError("empty batch")
    scene = _scene(depth_scene)
    F, H, W = (int(v) for v in scene.shape)
    K = devargs.per_row_K(K.detach().to(torch.float64), N)
    dev = img.device
    _same_device(image_points=img, model_points=mod, depth_scene=scene, K=K)
    if isinstance(counts, torch.Tensor) and counts.device.type == "cuda":
        _same_device(image_points=img, counts=counts)
    cnt = _counts(counts, N, S, dev)
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    # (after the checks that need no device: a bad call fails the same everywhere)
    img, mod = devargs.device_tensor(img, torch.float32, None, "image_points", WHERE), devargs.device_tensor(mod, torch.float32, None, "model_points", WHERE)
    scene, K = devargs.device_tensor(scene, None, None, "depth_scene", WHERE), devargs.device_tensor(K, None, None, "K", WHERE)
    lib = cabi.load()
    out = dict(cam_points=torch.empty(N, S, 3, dtype=torch.float64, device=dev), model_points=torch.empty(N, S, 3, dtype=torch.float64, device=dev),
               counts=torch.empty(N, dtype=torch.int32, device=dev))
    p = cabi.ptr
    cabi.check(lib.gdrn_backproject_points(p(img), p(mod), p(cnt), p(scene), p(fr), fr_host.ctypes.data, F, H, W, p(K), N, S, p(out["cam_points"]),
                                           p(out["model_points"]), p(out["counts"]), devargs.stream(dev)), "backproject_points")
    return out


def _counts(counts, N, S, dev):
    """counts [N] as an int32 device tensor.  A device tensor is NOT copied back (the kernels clamp it to [0, S]): that is what lets the solver
    chain behind ``backproject``; values from the host are checked here and uploaded."""
    if isinstance(counts, torch.Tensor) and counts.device.type == "cuda":
        c = counts.detach().reshape(-1)
        if c.shape[0] != N:
            raise ValueError(f"counts: {c.shape[0]} entries for {N} rows")
        if c.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
            raise ValueError(f"counts is {c.dtype}: an integer tensor")
        return c.to(torch.int32).contiguous()
    return devargs.index_vector(counts, N, S, dev, "counts", inclusive=True)[0]


def _pairs(cam_points, model_points, counts):
    for name, v in (("cam_points", cam_points), ("model_points", model_points)):
        if not isinstance(v, torch.Tensor):
            raise devargs.no_fallback(name, WHERE)
    cam, mod = cam_points.detach(), model_points.detach()
    if cam.dim() != 3 or cam.shape[2] != 3 or cam.shape != mod.shape:
        raise ValueError(f"cam_points and model_points [N,S,3] expected, got {tuple(cam.shape)} and {tuple(mod.shape)}")
    N, S = int(cam.shape[0]), int(cam.shape[1])
    if N <= 0 or S <= 0:
        raise ValueError("empty batch")
    _same_device(cam_points=cam, model_points=mod)
    if isinstance(counts, torch.Tensor) and counts.device.type == "cuda":
        _same_device(cam_points=cam, counts=counts)
    cnt = _counts(counts, N, S, cam.device)
    # (after the checks that need no device: a bad call fails the same everywhere)
    cam, mod = devargs.device_tensor(cam, torch.float64, None, "cam_points", WHERE), devargs.device_tensor(mod, torch.float64, None, "model_points", WHERE)
    return cam, mod, cnt, N, S


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
    if R.device != dev or t.device != dev:
        raise ValueError(f"R0 / t0 are on {R.device} / {t.device}, the points on {dev}")
    return R, t


def rigid_ransac(cam_points, model_points, counts, dist_thr=0.02, iters=100, seed=0, R0=None, t0=None, want_mask=False):
    """RANSAC (``iters`` 3-point hypotheses per RoI, gate ``dist_thr`` metres -- the default is ``refine``'s ``dist_gate``) + the closed-form fit on
    the inliers, for N RoIs in one call.  cam_points, model_points [N,S,3] (read as fp64), counts [N] (only the first counts[n] rows of RoI n are
    read; a device tensor is not copied back): what ``backproject`` returns.  Returns a dict of device tensors: R [N,3,3], t [N,3] fp64
    (model to camera), ok [N] int32 (0: not solvable -- R, t are R0, t0, identity / zero without them), num_inliers [N] int32, rms [N] fp64
    (root of the inliers' mean squared 3D distance in metres, NaN where ok is 0) and, with ``want_mask``, inlier_mask [N,S] uint8.  The same
    (seed, inputs) give the same bits on every call."""
    if int(iters) <= 0 or not 0.0 < float(dist_thr) < float("inf"):
        raise ValueError(f"iters and dist_thr must be positive, got {iters}, {dist_thr}")
    cam, mod, cnt, N, S = _pairs(cam_points, model_points, counts)
    dev = cam.device
    R, t = _pose0(R0, t0, N, dev)
    lib = cabi.load()
    ok = torch.empty(N, dtype=torch.int32, device=dev)
    num = torch.empty(N, dtype=torch.int32, device=dev)
    rms = torch.empty(N, dtype=torch.float64, device=dev)
    mask = torch.empty(N, S, dtype=torch.uint8, device=dev) if want_mask else None
    ws = devargs.workspace(lib.gdrn_rigid_workspace_bytes(N, S, int(iters)), dev, "rigid_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_rigid_ransac(p(cam), p(mod), p(cnt), N, S, float(dist_thr), int(iters), int(seed) & 0xFFFFFFFFFFFFFFFF, p(R), p(t), p(ok),
                                     p(num), p(mask), p(rms), p(ws), devargs.stream(dev)), "rigid_ransac")
    out = dict(R=R, t=t, ok=ok, num_inliers=num, rms=rms)
    if want_mask:
        out["inlier_mask"] = mask
    return out


def rigid_fit(cam_points, model_points, counts, R0=None, t0=None):
    """The closed-form least-squares pose over all counts[n] rows of each RoI, no inlier gate (the analogue of ``pnp.pnp_refine``; being closed
    form it needs no start: R0, t0 are only what an unsolved RoI hands back).  Returns a dict of device tensors: R, t, ok (0: fewer than 3 rows, a
    degenerate -- collinear -- set or a non-finite row), rms [N] fp64 over all rows (metres)."""
    cam, mod, cnt, N, S = _pairs(cam_points, model_points, counts)
    dev = cam.device
    R, t = _pose0(R0, t0, N, dev)
    lib = cabi.load()
    ok = torch.empty(N, dtype=torch.int32, device=dev)
    rms = torch.empty(N, dtype=torch.float64, device=dev)
    p = cabi.ptr
    cabi.check(lib.gdrn_rigid_fit(p(cam), p(mod), p(cnt), N, S, p(R), p(t), p(ok), p(rms), devargs.stream(dev)), "rigid_fit")
    return dict(R=R, t=t, ok=ok, rms=rms)


def poses_from_maps_rgbd(cfg, out_dict, roi_coord_2d, roi_extents, im_H, im_W, K, depth_scene, frame, dist_thr=0.02, iters=100, seed=0):
    """The RGB-D sibling of ``pnp.poses_from_maps``: ``postproc.get_img_model_points_with_coords2d``, then ``backproject`` into ``depth_scene``
    [F,H,W] (``frame`` [N]: the frame of each RoI), then ``rigid_ransac`` from the network's own pose ``out_dict["rot"]`` / ``["trans"]``; no
    host read between the three.  Returns a dict of device tensors: pose_est [N,3,4] fp64, ok, num_inliers [N] int32, rms [N] fp64.  A RoI that
    cannot be solved -- too few pixels with depth is the usual cause -- keeps the network's pose with ok = 0.  ``refine.icp_refine(meshes, labels,
    pose_est[:, :, :3], pose_est[:, :, 3], K, depth_scene, frame)`` can follow directly."""
    if int(iters) <= 0 or not 0.0 < float(dist_thr) < float("inf"):
        raise ValueError(f"iters and dist_thr must be positive, got {iters}, {dist_thr}")
    scene = _scene(depth_scene)
    mask = out_dict["mask"]
    if not isinstance(mask, torch.Tensor):
        raise devargs.no_fallback("mask", WHERE)
    _same_device(depth_scene=scene, mask=mask)
    N = int(mask.shape[0])
    frame = devargs.index_vector(frame, N, int(scene.shape[0]), "cpu", "frame")[1]   # (checked before anything is launched)
    K = devargs.device_tensor(torch.as_tensor(K), None, None, "K", WHERE)
    R_net = devargs.device_tensor(out_dict["rot"], torch.float64, (N, 3, 3), "rot", WHERE)
    t_net = devargs.device_tensor(out_dict["trans"], torch.float64, (N, 3), "trans", WHERE)
    _, _, img, mod, counts = postproc.get_img_model_points_with_coords2d(cfg, out_dict, roi_coord_2d, roi_extents, im_H, im_W)
    pts = backproject(img, mod, counts, scene, frame, K)
    res = rigid_ransac(pts["cam_points"], pts["model_points"], pts["counts"], dist_thr=dist_thr, iters=iters, seed=seed, R0=R_net, t0=t_net)
    return dict(pose_est=torch.cat([res["R"], res["t"].unsqueeze(2)], dim=2), ok=res["ok"], num_inliers=res["num_inliers"], rms=res["rms"])
