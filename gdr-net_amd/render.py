"""Batched depth rasterizer and xyz-target generation on the device (csrc/render.hip).

Host-side mirror of the reference's offline pass ``tools/lm/lm_pbr_1_gen_xyz_crop.py``: per annotated instance an OpenGL depth render of the
object's mesh under the ground-truth pose, ``misc.calc_xyz_bp_fast(depth, R, t, K)`` (lib/pysixd/misc.py:288-316) and ``mask2bbox_xyxy``
(lib/utils/mask_utils.py:39-44), pickled as fp16 and pasted back into a frame at training time (core/gdrn_modeling/data_loader.py:460-470).
Here poses, meshes and intrinsics go in and ``xyz_crop`` / ``xyxy`` and the full-object mask come out, for a whole batch per call, ready for
``roi_data.RoiCropper``.  The rasterizer's rules (integer-pixel rays, inclusive edges, no near-plane clipping: a triangle with a vertex in front
of ``near`` is dropped whole) are stated with the entry points in ``include/gdrn_hip.h``.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import cabi, devargs

NEAR, FAR = 0.01, 6.5   # the tool's values (lm_pbr_1_gen_xyz_crop.py:48-49)
WHERE = "the renderer"   # (this module in devargs' error sentence)


class MeshTable(devargs.DeviceTables):
    """Per-class triangle meshes, packed once without padding: ``vertices_list`` a list of [n_c,3] arrays in metres (kept as fp64), ``faces_list`` a
    list of [f_c,3] integer arrays of vertex indices within the class (kept as int32, range-checked here).  ``verts`` / ``faces`` are the
    concatenations, class c owning the rows ``vert_off[c] : vert_off[c] + nverts[c]`` and ``face_off[c] : face_off[c] + nfaces[c]``."""

    TABLES = ("verts", "faces", "vert_off", "nverts", "face_off", "nfaces")

    def __init__(self, vertices_list, faces_list, device=None):
        C = len(vertices_list)
        if C == 0 or len(faces_list) != C:
            raise ValueError("vertices_list and faces_list need one entry per class")
        vs = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in vertices_list]
        fs = []
        for c, f in enumerate(faces_list):
            f = np.asarray(f)
            if f.size and not np.issubdtype(f.dtype, np.integer):
                raise ValueError(f"faces of class {c} are not integers")
            f = f.reshape(-1, 3).astype(np.int64)
            if len(vs[c]) == 0 or len(f) == 0:
                raise ValueError(f"class {c} has no vertices or no faces")
            if f.min() < 0 or f.max() >= len(vs[c]):
                raise ValueError(f"class {c}: face index outside [0, {len(vs[c])})")
            fs.append(f.astype(np.int32))
        self.num_classes = C
        self.nverts = np.array([len(v) for v in vs], dtype=np.int32)
        self.nfaces = np.array([len(f) for f in fs], dtype=np.int32)
        if int(self.nverts.astype(np.int64).sum()) >= 2 ** 31 or int(self.nfaces.astype(np.int64).sum()) >= 2 ** 31:
            raise ValueError("the packed table is indexed with int32 offsets")
        self.vert_off = np.concatenate([[0], np.cumsum(self.nverts)[:-1]]).astype(np.int32)
        self.face_off = np.concatenate([[0], np.cumsum(self.nfaces)[:-1]]).astype(np.int32)
        self.f_max = int(self.nfaces.max())
        self.verts = np.ascontiguousarray(np.concatenate(vs, axis=0))
        self.faces = np.ascontiguousarray(np.concatenate(fs, axis=0))
        if device is not None:
            self.on(device)

    def lib_args(self, device):
        """the eight leading arguments of every library call that draws from the table: the six tables on ``device``, then C and f_max"""
        tb, p = self.on(device), cabi.ptr
        return (p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]), self.num_classes, self.f_max)


def render_depth(table, labels, R, t, K, H, W, near=NEAR, far=FAR):
    """Depth [N,H,W] fp32 (camera-space z in metres, 0 where nothing is drawn) of N instances in one call: instance i is the mesh ``labels[i]`` of
    ``table`` under the pose ``R[i]``, ``t[i]`` (model to camera, metres) seen through ``K[i]`` (upper triangular; [3,3] is shared by all).
    R, t, K: device tensors, fp32 or fp64.  A triangle with a vertex at z < near is dropped whole (no near-plane clipping)."""
    R, t, K, N = devargs.poses(R, t, K, WHERE)
    dev = R.device
    lab, lab_host = devargs.index_vector(labels, N, table.num_classes, dev, "labels")
    mesh = table.lib_args(dev)
    H, W = int(H), int(W)
    depth = torch.empty(max(N, 0), max(H, 0), max(W, 0), dtype=torch.float32, device=dev)
    p = cabi.ptr
    cabi.check(cabi.load().gdrn_render_depth(*mesh, p(lab), lab_host.ctypes.data, p(R), p(t), p(K), N, H, W, float(near), float(far), p(depth),
                                             devargs.stream(dev)), "render_depth")
    return depth


def xyz_from_depth(depth, R, t, K):
    """``calc_xyz_bp_fast`` + ``mask2bbox_xyxy`` for a batch of depth maps [N,H,W] (from ``render_depth`` or the caller's own): a dict of device
    tensors ``xyz`` [N,H,W,3] fp32 = R^T (depth K^-1 [x,y,1] - t) evaluated in fp64, 0 where depth is 0; ``mask`` [N,H,W] u8; ``xyxy`` [N,4] int32,
    the inclusive bounds of the mask; ``visible`` [N] int32.  An empty mask gives xyxy = [0, 0, W-1, H-1] and visible = 0, as the tool writes it."""
    depth = devargs.device_tensor(depth, torch.float32, None, "depth", WHERE)
    if depth.dim() != 3:
        raise ValueError("depth must be [N, H, W]")
    R, t, K, N = devargs.poses(R, t, K, WHERE)
    if depth.shape[0] != N:
        raise ValueError("depth, R, t and K need one entry per instance")
    dev = depth.device
    H, W = int(depth.shape[1]), int(depth.shape[2])
    out = dict(xyz=torch.empty(N, H, W, 3, dtype=torch.float32, device=dev), mask=torch.empty(N, H, W, dtype=torch.uint8, device=dev),
               xyxy=torch.empty(N, 4, dtype=torch.int32, device=dev), visible=torch.empty(N, dtype=torch.int32, device=dev))
    p = cabi.ptr
    cabi.check(cabi.load().gdrn_xyz_from_depth(p(depth), p(R), p(t), p(K), N, H, W, p(out["xyz"]), p(out["mask"]), p(out["xyxy"]), p(out["visible"]),
                                               devargs.stream(dev)), "xyz_from_depth")
    return out


def xyz_targets(table, labels, R, t, K, H, W, near=NEAR, far=FAR):
    """``render_depth`` then ``xyz_from_depth``: a list of N dicts with the keys ``RoiCropper.prepare(..., train=True)`` reads from a RoI --
    ``xyz_crop`` (device fp32 [y2-y1+1, x2-x1+1, 3], the ``[y1:y2+1, x1:x2+1]`` slice of the instance's xyz map, a view) and ``xyxy`` (host
    ints) -- plus ``mask_obj`` (device u8 [H,W], the full-object mask) and ``visible`` (bool).  Costs ONE device-to-host copy per batch, of the
    N x 4 bounds and the N flags: the cropper's task table wants the bounds as host ints.  An instance that is not visible gets the whole frame
    as its box and an all-zero ``xyz_crop``; the reference ignores such instances at training time."""
    depth = render_depth(table, labels, R, t, K, H, W, near, far)
    out = xyz_from_depth(depth, R, t, K)
    host = torch.cat([out["xyxy"], out["visible"][:, None]], dim=1).cpu().numpy()   # the one copy
    res = []
    for i, (x1, y1, x2, y2, vis) in enumerate(host.tolist()):
        res.append(dict(xyz_crop=out["xyz"][i, y1 : y2 + 1, x1 : x2 + 1], xyxy=(x1, y1, x2, y2), mask_obj=out["mask"][i], visible=bool(vis)))
    return res
