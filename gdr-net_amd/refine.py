"""Depth refinement of estimated poses on the device (csrc/icp.hip): projective point-to-plane ICP against observed depth frames.

The reference is RGB-only (``WITH_DEPTH=False``) and has no counterpart; this is the usual last step of an RGB-D entry between the network's
pose (or ``pnp.poses_from_maps``) and the metric modules.  Per iteration the model is rendered under the current pose (``render.render_depth``'s
launch), every pixel where the render and the observation lie within ``dist_gate`` of each other and the observation has a normal becomes a
pair, and the 6 x 6 point-to-plane normal equations of every estimate are summed and solved; the pose is updated by left multiplication.  The
association is by pixel: it refines estimates that already overlap the object.  There is no silhouette term (flat-faced objects keep their
sliding directions) and there are no robust weights.  The arithmetic is stated with the entry points in ``include/gdrn_hip.h``; all of it is
fp64, sums have a fixed order (the same call gives the same bits; the instances of a batch do not influence each other).  Nothing is read back
inside ``icp_refine``.  There is no CPU fallback.
"""
import torch

from . import cabi, devargs, render

WHERE = "the depth refinement"   # (this module in devargs' error sentence)
RUNNING, CONVERGED, DEGENERATE = 0, 1, 2   # GDRN_ICP_RUNNING, GDRN_ICP_CONVERGED, GDRN_ICP_DEGENERATE


def _scene(depth_scene):
    """the observed frames [F,H,W] fp32, on the device and contiguous"""
    if not isinstance(depth_scene, torch.Tensor) or depth_scene.device.type != "cuda":
        raise devargs.no_fallback("depth_scene", WHERE)
    if depth_scene.dtype != torch.float32:
        raise ValueError(f"depth_scene is {depth_scene.dtype}: torch.float32 (metres)")
    if depth_scene.dim() != 3 or min(depth_scene.shape[1:]) < 1:
        raise ValueError("depth_scene must be [F, H, W] with H and W of at least 1")
    return devargs.device_tensor(depth_scene, None, None, "depth_scene", WHERE)


def _gates(dist_gate, normal_gate):
    dist_gate, normal_gate = float(dist_gate), float(normal_gate)
    if not dist_gate > 0.0 or not normal_gate > 0.0:
        raise ValueError(f"dist_gate {dist_gate} and normal_gate {normal_gate} must be positive")
    return dist_gate, normal_gate


def normal_equations(depth_ren, depth_scene, frame, K, dist_gate=0.02, normal_gate=0.01):
    """One accumulation on given renders: ``depth_ren`` [N,H,W] fp32 (the model under each estimate's pose, e.g. ``render.render_depth``'s),
    ``depth_scene`` [F,H,W] fp32 (metres, 0 = no measurement), ``frame`` [N] (the frame of each estimate), ``K`` [N,3,3] or [3,3].  Returns a
    dict of device tensors: A [N,6,6] fp64 (symmetric, full), b [N,6], sq [N] fp64 and pairs [N] int32."""
    dist_gate, normal_gate = _gates(dist_gate, normal_gate)
    if not isinstance(depth_ren, torch.Tensor) or depth_ren.device.type != "cuda":
        raise devargs.no_fallback("depth_ren", WHERE)
    if depth_ren.dtype != torch.float32 or depth_ren.dim() != 3:
        raise ValueError("depth_ren must be an fp32 [N, H, W] tensor")
    scene = _scene(depth_scene)
    ren = devargs.device_tensor(depth_ren, None, None, "depth_ren", WHERE)
    if ren.shape[1:] != scene.shape[1:]:
        raise ValueError(f"depth_ren {tuple(ren.shape)} and depth_scene {tuple(scene.shape)} differ in H, W")
    if ren.device != scene.device:
        raise ValueError(f"depth_ren is on {ren.device}, depth_scene on {scene.device}")
    N, H, W = (int(s) for s in ren.shape)
    dev = ren.device
    K = devargs.per_row_K(devargs.device_tensor(K, torch.float64, (-1, 3, 3), "K", WHERE), N)
    F = int(scene.shape[0])
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    sys = torch.empty(max(N, 1), 28, dtype=torch.float64, device=dev)[:N]
    pairs = torch.empty(max(N, 1), dtype=torch.int32, device=dev)[:N]
    if N > 0:
        lib = cabi.load()
        ws = devargs.workspace(lib.gdrn_icp_workspace_bytes(N, H, W), dev, "icp_workspace_bytes")
        p = cabi.ptr
        cabi.check(lib.gdrn_icp_accumulate(p(ren), p(scene), p(fr), fr_host.ctypes.data, F, p(K), N, H, W, dist_gate, normal_gate, p(sys), p(pairs),
                                           p(ws), devargs.stream(dev)), "icp_accumulate")
    iu = torch.triu_indices(6, 6, device=dev)
    A = torch.zeros(N, 6, 6, dtype=torch.float64, device=dev)
    A[:, iu[0], iu[1]] = sys[:, :21]   # the packed upper triangle, row by row
    A[:, iu[1], iu[0]] = sys[:, :21]
    return dict(A=A, b=sys[:, 21:27].contiguous(), sq=sys[:, 27].contiguous(), pairs=pairs)


def icp_refine(meshes, labels, R0, t0, K, depth_scene, frame, iters=10, dist_gate=0.02, normal_gate=0.01, min_pairs=64, near=render.NEAR,
               far=render.FAR):
    """Refine N estimates against observed depth: ``meshes`` a ``render.MeshTable``, ``labels`` [N] the mesh of each estimate, ``R0`` [N,3,3],
    ``t0`` [N,3], ``K`` [N,3,3] or [3,3] device tensors (fp32 or fp64; model to camera, metres), ``depth_scene`` [F,H,W] fp32 on the device
    (metres, 0 = no measurement), ``frame`` [N] the frame of each estimate.  ``iters`` iterations of render, accumulate and step run on the
    current stream without a host read.  Returns a dict of device tensors: R [N,3,3] and t [N,3] fp64; ok [N] int32 (0: the instance was found
    degenerate -- fewer than ``min_pairs`` pairs or unobservable directions -- and keeps the pose it had); iters_done [N] int32 (steps applied);
    pairs [N] int32 and rms [N] fp64 (metres; NaN without a pair), those of the residual before the instance's last step."""
    dist_gate, normal_gate = _gates(dist_gate, normal_gate)
    iters, min_pairs = int(iters), int(min_pairs)
    if iters < 0 or min_pairs < 6:
        raise ValueError(f"iters {iters} must be >= 0 and min_pairs {min_pairs} >= 6 (the unknowns of a pose)")
    R, t, K, N = devargs.poses(R0, t0, K, WHERE)
    scene = _scene(depth_scene)
    dev = R.device
    if scene.device != dev:
        raise ValueError(f"R0 is on {dev}, depth_scene on {scene.device}")
    F, H, W = (int(s) for s in scene.shape)
    lab, lab_host = devargs.index_vector(labels, N, meshes.num_classes, dev, "labels")
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    R, t = R.clone(), t.clone()   # in/out for the library; the caller's tensors stay
    out = dict(R=R, t=t, ok=torch.empty(N, dtype=torch.int32, device=dev), iters_done=torch.empty(N, dtype=torch.int32, device=dev),
               pairs=torch.empty(N, dtype=torch.int32, device=dev), rms=torch.empty(N, dtype=torch.float64, device=dev))
    if N == 0:
        return out
    lib = cabi.load()
    tb = meshes.on(dev)
    scratch = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    ws = devargs.workspace(lib.gdrn_icp_workspace_bytes(N, H, W), dev, "icp_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_icp_refine(p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]),
                                   meshes.num_classes, meshes.f_max, p(lab), lab_host.ctypes.data, p(R), p(t), p(K), N, p(scene), p(fr),
                                   fr_host.ctypes.data, F, H, W, float(near), float(far), iters, dist_gate, normal_gate, min_pairs, p(scratch),
                                   p(out["ok"]), p(out["iters_done"]), p(out["pairs"]), p(out["rms"]), p(ws), devargs.stream(dev)), "icp_refine")
    return out
