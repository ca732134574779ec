"""Deterministic synthetic inputs and weights for the GDR-Net hot path.

Everything here is produced by a repo-owned counter-based integer hash (splitmix64
finaliser) evaluated with numpy, so that the container that generated the golden
fixtures (``tests/golden/make_golden.py``) and the GPU box regenerate *bit-identical*
weights and RoI batches without torch's RNG, datasets or checkpoints.

* ``param_schema()``  -- the reference's state_dict key/shape schema
  (keys from core/gdrn_modeling/models/resnet_backbone.py:17-51,
  cdpn_rot_head_region.py:80-136, conv_pnp_net.py:76-92).
* ``make_state_dict(seed)`` -- Kaiming-scaled deterministic weights (default init
  N(0, 0.001^2) + eval BN gives degenerate activations, SURVEY.md section 7 "hard parts").
* ``make_batch(bs, seed)`` -- a synthetic RoI batch with exactly the keys / dtypes / shapes
  ``batch_data`` emits (core/gdrn_modeling/engine_utils.py:6-60).
"""
import math
from collections import OrderedDict

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _mix64(x):
    """splitmix64 finaliser on a uint64 array (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        x = x.astype(np.uint64)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def _stream_key(seed, name):
    with np.errstate(over="ignore"):
        h = np.uint64(seed) * _GOLD + np.uint64(0x1234567)
        for ch in name.encode():
            h = _mix64(np.array([h ^ np.uint64(ch)], dtype=np.uint64))[0] + _GOLD
    return h


def hash_uniform(seed, name, shape):
    """U[0,1) float64 array of ``shape``; value i depends only on (seed, name, i)."""
    n = int(np.prod(shape)) if len(shape) else 1
    key = _stream_key(seed, name)
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) * _GOLD + key
    h = _mix64(idx)
    u = (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return u.reshape(shape)


def hash_normal(seed, name, shape):
    """N(0,1) float64 array (Box-Muller on two hash streams)."""
    u1 = hash_uniform(seed, name + "/u1", shape)
    u2 = hash_uniform(seed, name + "/u2", shape)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * math.pi * u2)


def hash_randint(seed, name, shape, lo, hi):
    return (lo + np.floor(hash_uniform(seed, name, shape) * (hi - lo))).astype(np.int64)


# ----------------------------------------------------------------------------------------------
# state-dict schema
# ----------------------------------------------------------------------------------------------
RESNET34_LAYERS = (3, 4, 6, 3)
RESNET34_PLANES = (64, 128, 256, 512)
HEAD_CONV_IDX = (3, 6, 10, 13, 17, 20)  # features.N conv 3x3 256->256
HEAD_BN_IDX = (1, 4, 7, 11, 14, 18, 21)
HEAD_UP_BEFORE = (10, 17)  # UpsamplingBilinear2d sits right before these convs (features.9 / .16)
PNP_CONV_IDX = (0, 3, 6)
PNP_GN_IDX = (1, 4, 7)


def param_schema(num_regions=64, pnp_in=69, rot_dim=6):
    """OrderedDict name -> (shape, kind).  kind in conv|convT|bn_w|bn_b|bn_rm|bn_rv|bn_nbt|gn_w|gn_b|fc_w|fc_b|bias."""
    s = OrderedDict()

    def bn(prefix, c):
        s[prefix + ".weight"] = ((c,), "bn_w")
        s[prefix + ".bias"] = ((c,), "bn_b")
        s[prefix + ".running_mean"] = ((c,), "bn_rm")
        s[prefix + ".running_var"] = ((c,), "bn_rv")
        s[prefix + ".num_batches_tracked"] = ((), "bn_nbt")

    s["backbone.conv1.weight"] = ((64, 3, 7, 7), "conv")
    bn("backbone.bn1", 64)
    inpl = 64
    for li, (nb, pl) in enumerate(zip(RESNET34_LAYERS, RESNET34_PLANES), start=1):
        for b in range(nb):
            stride = 2 if (b == 0 and li > 1) else 1
            p = f"backbone.layer{li}.{b}"
            s[p + ".conv1.weight"] = ((pl, inpl, 3, 3), "conv")
            bn(p + ".bn1", pl)
            s[p + ".conv2.weight"] = ((pl, pl, 3, 3), "conv")
            bn(p + ".bn2", pl)
            if stride != 1 or inpl != pl:
                s[p + ".downsample.0.weight"] = ((pl, inpl, 1, 1), "conv")
                bn(p + ".downsample.1", pl)
            inpl = pl
    s["rot_head_net.features.0.weight"] = ((512, 256, 3, 3), "convT")
    bn("rot_head_net.features.1", 256)
    for ci, bi in zip(HEAD_CONV_IDX, HEAD_BN_IDX[1:]):
        s[f"rot_head_net.features.{ci}.weight"] = ((256, 256, 3, 3), "conv")
        bn(f"rot_head_net.features.{bi}", 256)
    out_c = 1 + 3 + (num_regions + 1)
    s["rot_head_net.features.23.weight"] = ((out_c, 256, 1, 1), "conv")
    s["rot_head_net.features.23.bias"] = ((out_c,), "bias")
    cin = pnp_in
    for ci, gi in zip(PNP_CONV_IDX, PNP_GN_IDX):
        s[f"pnp_net.features.{ci}.weight"] = ((128, cin, 3, 3), "conv")
        s[f"pnp_net.features.{gi}.weight"] = ((128,), "gn_w")
        s[f"pnp_net.features.{gi}.bias"] = ((128,), "gn_b")
        cin = 128
    s["pnp_net.fc1.weight"] = ((1024, 128 * 8 * 8), "fc_w")
    s["pnp_net.fc1.bias"] = ((1024,), "fc_b")
    s["pnp_net.fc2.weight"] = ((256, 1024), "fc_w")
    s["pnp_net.fc2.bias"] = ((256,), "fc_b")
    s["pnp_net.fc_r.weight"] = ((rot_dim, 256), "fc_w")
    s["pnp_net.fc_r.bias"] = ((rot_dim,), "fc_b")
    s["pnp_net.fc_t.weight"] = ((3, 256), "fc_w")
    s["pnp_net.fc_t.bias"] = ((3,), "fc_b")
    return s


def conditioned_state_dict(seed=0):
    """make_state_dict with the last BatchNorm weight of every residual block scaled by 0.1 (the usual zero-gamma residual init).  The plain
    synthetic init's BatchNorm-ReLU chain multiplies every perturbation by ~1.2 per layer (x700-1600 over the graph's 43 BatchNorms), so a
    bf16-vs-fp32 comparison on it measures that chaos; with near-identity blocks the amplification is ~x80 and the arithmetic's own error
    is what is left (tests/test_e2e_gpu.py::test_bf16_parity_on_a_conditioned_network, __graft_entry__.smoke)."""
    sd = make_state_dict(seed)
    for k in sd:
        if k.startswith("backbone.layer") and k.endswith("bn2.weight"):
            sd[k] = sd[k] * 0.1
    return sd


def make_state_dict(seed=0, as_torch=True):
    """Deterministic, well-conditioned weights keyed by the reference's state_dict names."""
    sd = OrderedDict()
    for name, (shape, kind) in param_schema().items():
        if kind == "conv":
            fan_in = shape[1] * shape[2] * shape[3]
            v = hash_normal(seed, name, shape) * math.sqrt(2.0 / fan_in)
        elif kind == "convT":
            fan_in = shape[0] * shape[2] * shape[3] / 4.0  # stride 2: 9/4 taps hit per output pixel
            v = hash_normal(seed, name, shape) * math.sqrt(2.0 / fan_in)
        elif kind in ("bn_w", "gn_w"):
            v = 0.5 + hash_uniform(seed, name, shape)
        elif kind in ("bn_b", "gn_b"):
            v = 0.4 * hash_uniform(seed, name, shape) - 0.2
        elif kind == "bn_rm":
            v = np.zeros(shape)
        elif kind == "bn_rv":
            v = np.ones(shape)
        elif kind == "bn_nbt":
            v = np.zeros(shape, dtype=np.int64)
        elif kind == "fc_w":
            v = hash_normal(seed, name, shape) * math.sqrt(1.0 / shape[1])
            if name.endswith("fc_t.weight"):
                v = v * 0.3
        elif kind in ("fc_b", "bias"):
            v = 0.2 * hash_uniform(seed, name, shape) - 0.1
            if name.endswith("fc_t.bias"):
                v = np.array([0.05, -0.03, 1.0])
        else:
            raise KeyError(kind)
        if kind != "bn_nbt":
            v = np.asarray(v, dtype=np.float32)
        sd[name] = v
    if as_torch:
        import torch

        sd = OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
    return sd


# ----------------------------------------------------------------------------------------------
# synthetic RoI batch
# ----------------------------------------------------------------------------------------------
LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)
# ^ LineMOD intrinsics, ref/lm_full.py:106 (dataset constant)
YCBV_K = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]], dtype=np.float32)
# ^ YCB-V intrinsics, ref/ycbv.py:89 (dataset constant)


def _random_rotations(seed, name, n):
    q = hash_normal(seed, name, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack(
        [
            1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y),
        ],
        axis=1,
    ).reshape(n, 3, 3)
    return R


def make_batch(bs, seed=1, num_classes=13, num_points=3000, cam="lm", with_sym=False, as_torch=True, device=None):
    """Synthetic batch with the keys of ``batch_data`` (engine_utils.py:6-60)."""
    K = LM_K if cam == "lm" else YCBV_K
    b = OrderedDict()
    b["roi_img"] = hash_uniform(seed, "roi_img", (bs, 3, 256, 256)).astype(np.float32)
    b["roi_coord_2d"] = hash_uniform(seed, "roi_coord_2d", (bs, 2, 64, 64)).astype(np.float32)
    b["roi_cls"] = hash_randint(seed, "roi_cls", (bs,), 0, num_classes)
    b["roi_cam"] = np.broadcast_to(K, (bs, 3, 3)).copy()
    cx = 100 + 440 * hash_uniform(seed, "cx", (bs,))
    cy = 100 + 280 * hash_uniform(seed, "cy", (bs,))
    b["roi_center"] = np.stack([cx, cy], 1).astype(np.float32)
    wh = 40 + 160 * hash_uniform(seed, "wh", (bs, 2))
    b["roi_wh"] = wh.astype(np.float32)
    scale = 1.5 * wh.max(1)  # data_loader.py:417,423 (DZI_PAD_SCALE * max(bw, bh))
    b["resize_ratio"] = (64.0 / scale).astype(np.float32)
    b["roi_extent"] = (0.05 + 0.25 * hash_uniform(seed, "extent", (bs, 3))).astype(np.float32)
    b["roi_xyz"] = hash_uniform(seed, "roi_xyz", (bs, 3, 64, 64)).astype(np.float32)
    for mk in ("trunc", "visib", "obj"):
        b["roi_mask_" + mk] = (hash_uniform(seed, "mask_" + mk, (bs, 64, 64)) < 0.5).astype(np.float32)
    b["roi_region"] = hash_randint(seed, "roi_region", (bs, 64, 64), 0, 65)
    b["ego_rot"] = _random_rotations(seed, "ego_rot", bs).astype(np.float32)
    t = hash_uniform(seed, "trans", (bs, 3))
    b["trans"] = np.stack([-0.2 + 0.4 * t[:, 0], -0.2 + 0.4 * t[:, 1], 0.5 + t[:, 2]], 1).astype(np.float32)
    tr = hash_uniform(seed, "trans_ratio", (bs, 3))
    b["roi_trans_ratio"] = np.stack([tr[:, 0] - 0.5, tr[:, 1] - 0.5, 0.5 + 1.5 * tr[:, 2]], 1).astype(np.float32)
    b["roi_points"] = (-0.1 + 0.2 * hash_uniform(seed, "roi_points", (bs, num_points, 3))).astype(np.float32)
    sym = [None] * bs
    if with_sym:
        rz = np.diag([-1.0, -1.0, 1.0]).astype(np.float32)  # pi about z
        for i in range(bs):
            if int(b["roi_cls"][i]) % 4 == 0:
                sym[i] = np.stack([np.eye(3, dtype=np.float32), rz])
    if as_torch:
        import torch

        for k in list(b.keys()):
            tt = torch.from_numpy(np.ascontiguousarray(b[k]))
            b[k] = tt.to(device) if device is not None else tt
        sym = [None if s is None else (torch.from_numpy(s).to(device) if device is not None else torch.from_numpy(s)) for s in sym]
    b["sym_info"] = sym
    return b


def model_kwargs(batch, do_loss=True):
    """Map a ``batch_data`` batch to the keyword arguments of ``GDRN.forward`` exactly as
    the reference trainer does (core/gdrn_modeling/engine.py:244-269)."""
    kw = dict(
        roi_classes=batch["roi_cls"],
        roi_cams=batch["roi_cam"],
        roi_whs=batch["roi_wh"],
        roi_centers=batch["roi_center"],
        resize_ratios=batch["resize_ratio"],
        roi_coord_2d=batch.get("roi_coord_2d", None),
        roi_extents=batch.get("roi_extent", None),
        do_loss=do_loss,
    )
    if do_loss:
        kw.update(
            gt_xyz=batch.get("roi_xyz", None),
            gt_xyz_bin=batch.get("roi_xyz_bin", None),
            gt_mask_trunc=batch["roi_mask_trunc"],
            gt_mask_visib=batch["roi_mask_visib"],
            gt_mask_obj=batch["roi_mask_obj"],
            gt_region=batch.get("roi_region", None),
            gt_ego_rot=batch.get("ego_rot", None),
            gt_trans=batch.get("trans", None),
            gt_trans_ratio=batch["roi_trans_ratio"],
            gt_points=batch.get("roi_points", None),
            sym_infos=batch.get("sym_info", None),
        )
    return kw


def make_postproc_inputs(B=3, H=64):
    """Inputs of the inference post-processing golden G7 (dense maps as the network emits them at test time):
    values in [0,1] with exact-0.5 coordinates (de-normalise to 0 -> rejected by the evaluator's |xyz| > 1e-4*extent
    test) and one flat-mask RoI (max == min -> NaN mask after the epsilon-free min-max normalisation -> no points)."""
    u = lambda tag, *shape: hash_uniform(71, tag, shape).astype(np.float32)
    mask = u("mask", B, 1, H, H) * np.float32(1.4) - np.float32(0.2)
    if B > 2:
        mask[2] = 0.25
    cx, cy, cz = u("cx", B, 1, H, H), u("cy", B, 1, H, H), u("cz", B, 1, H, H)
    cx[0, 0, :8] = 0.5
    if B > 1:
        cz[1, 0, :, :5] = 0.5
    coord2d = u("c2d", B, 2, H, H)
    extents = (np.float32(0.05) + np.float32(0.25) * u("ext", B, 3)).astype(np.float32)
    im_hw = np.array([[480, 640], [480, 640], [540, 720], [480, 640]], dtype=np.float32)[np.arange(B) % 4]
    return dict(mask=mask, coor_x=cx, coor_y=cy, coor_z=cz, coord2d=coord2d, extents=extents, im_hw=im_hw)


def make_roi_frames(B=8, seed=5, ncls=13, nfps=64, frame_sizes=((480, 640), (540, 720)), dzi_pad_scale=1.5):
    """Synthetic inputs of the RoI cropper / target builder, numpy on the host:
    a few u8 frames, and per RoI an annotated box with its object-coordinate patch (zeros = background holes),
    visible mask, optional truncation mask, jittered crop centre / size (DZI-like, data_loader.py:417-423), pose
    translation and projected centroid.  Edge cases by construction: RoI 0 hangs over the top-left frame corner,
    RoI 1 has the crop size clamped to max(H, W), RoI 2 is a 1-pixel-wide box, RoI 3 touches the bottom-right corner."""
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    frames = [np.floor(u(f"frame{i}", h, w, 3) * 256).astype(np.uint8) for i, (h, w) in enumerate(frame_sizes)]
    extents = (0.05 + 0.25 * u("ext", ncls, 3)).astype(np.float32)
    fps = ((u("fps", ncls, nfps, 3) - 0.5) * extents[:, None, :].astype(np.float64)).astype(np.float64)
    rois = []
    for n in range(B):
        fi = n % len(frames)
        H, W = frames[fi].shape[:2]
        r = u(f"roi{n}", 12)
        bw, bh = int(20 + r[0] * 160), int(20 + r[1] * 160)
        x1, y1 = int(r[2] * (W - bw - 1)), int(r[3] * (H - bh - 1))
        if n == 0:
            x1, y1 = 0, 0
        if n == 2:
            bw = 1
        if n == 3:
            x1, y1 = W - 1 - bw, H - 1 - bh
        x2, y2 = x1 + bw, y1 + bh
        cls = int(r[4] * ncls)
        xyz = ((u(f"xyz{n}", bh + 1, bw + 1, 3) - 0.5) * extents[cls].astype(np.float64)).astype(np.float32)
        xyz[u(f"hole{n}", bh + 1, bw + 1) < 0.3] = 0  # background inside the box
        seg = np.zeros((H, W), np.uint8)
        seg[y1 : y2 + 1, x1 : x2 + 1] = u(f"seg{n}", bh + 1, bw + 1) < 0.8
        trunc = (u(f"trunc{n}", H, W) < 0.7).astype(np.uint8) if n % 3 == 1 else None
        cx = 0.5 * (x1 + x2) + bw * 0.25 * (2 * r[5] - 1)
        cy = 0.5 * (y1 + y2) + bh * 0.25 * (2 * r[6] - 1)
        scale = max(bw, bh) * (1 + 0.25 * (2 * r[7] - 1)) * dzi_pad_scale
        if n == 1:
            scale = 5000.0
        scale = min(scale, max(H, W)) * 1.0
        rois.append(dict(frame=fi, bbox=np.array([x1, y1, x2, y2], np.float64), xyxy=(x1, y1, x2, y2), xyz_crop=xyz, segmentation=seg,
                         mask_trunc=trunc, bbox_center=np.array([cx, cy]), scale=float(scale), roi_cls=cls,
                         trans=np.array([r[8] * 0.4 - 0.2, r[9] * 0.4 - 0.2, 0.5 + r[10]], np.float32),
                         centroid_2d=np.array([0.5 * (x1 + x2) + 3 * r[11], 0.5 * (y1 + y2) - 2 * r[11]])))
    return dict(frames=frames, rois=rois, extents=extents, fps_points=fps)


AUG_FRAME_SIZES = ((47, 61), (33, 9), (64, 96))
AUG_BANK_SIZES = ((7, 1000), (100, 37), (375, 500), (481, 640))


def make_augment_inputs(seed=15):
    """Synthetic inputs of the frame augmenter (gdrnet_amd.augment), numpy on the host: u8 frames of 47 x 61, 33 x 9 and 64 x 96 with one
    foreground mask each (a noisy blob well inside the frame, so that every cut mode changes it), bank images of 7 x 1000, 100 x 37, 375 x 500 and
    481 x 640 -- between them up- and down-scaling, a zero-padded remainder, tiles cut by the frame edge and a frame narrower than one tile --
    and ``g15_bg``: the ready-made 47 x 61 background golden G15's composites were drawn with (as a bank image it is resized by exactly 1)."""
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    frames = [np.floor(u(f"aug_frame{i}", h, w, 3) * 256).astype(np.uint8) for i, (h, w) in enumerate(AUG_FRAME_SIZES)]
    bank = [np.floor(u(f"aug_bank{i}", h, w, 3) * 256).astype(np.uint8) for i, (h, w) in enumerate(AUG_BANK_SIZES)]
    masks = []
    for i, (h, w) in enumerate(AUG_FRAME_SIZES):
        m = np.zeros((h, w), np.uint8)
        y0, y1, x0, x1 = h // 5, h - h // 4, w // 4, w - w // 5
        m[y0:y1, x0:x1] = (u(f"aug_mask{i}", y1 - y0, x1 - x0) < 0.8) * (1 + i * 100)   # any non-zero value is foreground
        masks.append(m)
    h, w = AUG_FRAME_SIZES[0]
    return dict(frames=frames, masks=masks, bank=bank, g15_bg=np.floor(u("aug_g15_bg", h, w, 3) * 256).astype(np.uint8), seed=seed)


def make_region_inputs(B=4, res=64, nfps=64):
    """Inputs of golden G8 (``xyz_to_region``): cropped object-coordinate maps [B][res][res][3] fp32 with background
    holes, and fps points [B][nfps][3]; batch 1 has a duplicated fps point (argmin tie -> first index) and batch 2
    is all background."""
    u = lambda tag, *shape: hash_uniform(83, tag, shape)  # noqa: E731
    ext = (0.05 + 0.25 * u("ext", B, 3))
    xyz = ((u("xyz", B, res, res, 3) - 0.5) * ext[:, None, None, :]).astype(np.float32)
    xyz[u("hole", B, res, res) < 0.35] = 0
    fps = (u("fps", B, nfps, 3) - 0.5) * ext[:, None, :]
    if B > 1:
        fps[1, 7] = fps[1, 3]
        xyz[1, 0, 0] = fps[1, 3].astype(np.float32)
    if B > 2:
        xyz[2] = 0
    return dict(xyz=xyz, fps_points=fps)


POSE_METRIC_SEEDS = {"A": 91, "B": 92}   # the seeds golden G12 was drawn with (tests/golden/make_golden_g12.py moves on if a draw sits on a threshold)


def _axis_angle(axis, deg):
    """[n,3,3] fp64 rotations about unit `axis` [n,3] by `deg` [n] degrees (Rodrigues)."""
    a = np.deg2rad(deg)[:, None, None]
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    o = np.zeros_like(x)
    Kx = np.stack([o, -z, y, z, o, -x, -y, x, o], axis=1).reshape(-1, 3, 3)
    return np.eye(3)[None] + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)


def make_pose_metric_inputs(case="A", seed=None):
    """Inputs of the pose-error golden G12 (gdrnet_amd.pose_metrics against lib/pysixd/pose_error.py and the evaluator's recall table), fp64.

    case "A": 67 rows cycling through three classes -- 0: 1031 points, non-symmetric; 1: 257 points, symmetric under pi about z and pi about x;
    2: ONE point, symmetric, its single symmetry handed over as a bare 3x3 -- estimates = a rotation of 0.1 .. 20 degrees times the ground truth (times
    one of the class's symmetries on every fourth row of a symmetric class), translation offsets of 0 .. 0.15 m, rows 0 and 4 with the estimate equal
    to the ground truth, rows 7 and 10 (class 1) with R_est = R_gt S_k exactly, and 8 ground-truth instances without a prediction.
    case "B": 3 rows of one symmetric class of 8195 points (one more than a power of two: ragged last slab and last tile)."""
    seed = POSE_METRIC_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    rz, rx = np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0])
    if case == "A":
        N, sizes, diam = 67, (1031, 257, 1), [0.2, 0.3, 0.1]
        sym_infos, sym_classes, names = [None, np.stack([rz, rx]), rz.copy()], (1, 2), ["driller", "ape", "cat"]
        missing = {0: 3, 1: 3, 2: 2}
    elif case == "B":
        N, sizes, diam = 3, (8195,), [0.25]
        sym_infos, sym_classes, names = [rz[None].copy()], (0,), ["eggbox"]
        missing = {}
    else:
        raise ValueError(case)
    points = [-0.1 + 0.2 * u(f"pts{c}", n, 3) for c, n in enumerate(sizes)]
    labels = np.arange(N, dtype=np.int64) % len(sizes)
    R_gt = _random_rotations(seed, "R_gt", N)
    t_gt = np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)
    q = u("quality", N)
    ang = 0.1 * 200.0 ** (0.7 * q + 0.3 * u("q_ang", N))
    off = 0.15 * (0.7 * q + 0.3 * u("q_off", N)) ** 2
    axis = hash_normal(seed, "axis", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    tdir = hash_normal(seed, "tdir", (N, 3))
    tdir /= np.linalg.norm(tdir, axis=1, keepdims=True)
    R_est = _axis_angle(axis, ang) @ R_gt
    t_est = t_gt + off[:, None] * tdir
    for i in range(N):
        s = sym_infos[labels[i]]
        if s is not None and (i // len(sizes)) % 4 == 3:
            s = s.reshape(-1, 3, 3)
            R_est[i] = R_est[i] @ s[(i // (4 * len(sizes))) % len(s)]
    if case == "A":
        for i in (0, 4):
            R_est[i], t_est[i] = R_gt[i], t_gt[i]
        R_est[7], R_est[10] = R_gt[7] @ sym_infos[1][0], R_gt[10] @ sym_infos[1][1]
    K = np.repeat(LM_K.astype(np.float64)[None], N, axis=0)
    return dict(points=points, diameters=np.array(diam), sym_infos=sym_infos, sym_classes=sym_classes, obj_names=names, labels=labels,
                R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K, missing=missing, seed=seed)


PNP_COUNTS = (0, 3, 4, 5, 257, 1025, 4096, 600)   # empty | below minimal | minimal | clean | one past a workgroup stride | one past a scoring tile | full map | coplanar
PNP_SEEDS = {"clean": 131, "noisy": 132}


def make_pnp_inputs(case="clean", seed=None, stride=4096):
    """Inputs of the PnP tests (gdrnet_amd.pnp), fp64: N = 8 RoIs with PNP_COUNTS valid correspondences each in arrays of `stride` rows whose
    padding is NaN; model points in a 0.1 m box (RoI 7: all in one plane), per-RoI K near the LM camera, t_z from 0.3 to 2 m, rotations that
    include the identity (RoI 3) and one 5e-4 rad short of pi (RoI 5).  The RoIs with >= 257 points carry 40 % outliers displaced by 20 .. 80 px;
    the others are outlier-free.  case "clean": the inliers' image points are the exact projections; "noisy": displaced uniformly within a 1 px disc.
    Returns image_points [8,S,2], model_points [8,S,3], counts [8] int32, K [8,3,3], R [8,3,3], t [8,3], inlier [8,S] bool (the true inlier set)."""
    seed = PNP_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    N = len(PNP_COUNTS)
    R = _random_rotations(seed, "R", N)
    R[3] = np.eye(3)
    axis = hash_normal(seed, "axis", (1, 3))
    R[5] = _axis_angle(axis / np.linalg.norm(axis), np.rad2deg(np.array([np.pi - 5e-4])))[0]
    tz = np.array([1.0, 0.7, 0.3, 0.5, 0.8, 1.3, 2.0, 0.6])
    t = np.concatenate([(0.3 * u("t_xy", N, 2) - 0.15) * tz[:, None], tz[:, None]], axis=1)
    K = np.repeat(LM_K.astype(np.float64)[None], N, axis=0)
    K[:, 0, 0] += 4.0 * (u("fx", N) - 0.5)
    K[:, 1, 1] += 4.0 * (u("fy", N) - 0.5)
    K[:, :2, 2] += 6.0 * (u("c", N, 2) - 0.5)
    img = np.full((N, stride, 2), np.nan)
    mod = np.full((N, stride, 3), np.nan)
    inl = np.zeros((N, stride), dtype=bool)
    for n, c in enumerate(PNP_COUNTS):
        if c == 0:
            continue
        X = 0.1 * u(f"X{n}", c, 3) - 0.05
        if n == 7:
            X[:, 2] = 0.3 * X[:, 0] - 0.2 * X[:, 1] + 0.01   # one plane, not through the origin
        p = (X @ R[n].T + t[n]) @ K[n].T
        uv = p[:, :2] / p[:, 2:3]
        good = np.ones(c, dtype=bool)
        if c >= 257:
            good = u(f"out{n}", c) >= 0.4
            good[:4] = True
        ang, rad = 2.0 * math.pi * u(f"dir{n}", c), u(f"rad{n}", c)
        d = np.stack([np.cos(ang), np.sin(ang)], axis=1)
        if case == "noisy":
            uv = uv + np.where(good[:, None], np.sqrt(rad)[:, None] * d, 0.0)
        elif case != "clean":
            raise ValueError(case)
        uv = uv + np.where(good[:, None], 0.0, (20.0 + 60.0 * rad)[:, None] * d)
        img[n, :c], mod[n, :c], inl[n, :c] = uv, X, good
    return dict(image_points=img, model_points=mod, counts=np.array(PNP_COUNTS, dtype=np.int32), K=K, R=R, t=t, inlier=inl, seed=seed)


# ----------------------------------------------------------------------------------------------
# meshes and scenes of the depth rasterizer (gdrnet_amd.render, golden G13)
# ----------------------------------------------------------------------------------------------
def mesh_cube(edge=1.0):
    """axis-aligned cube centred on the origin: ([8,3] fp64 vertices, [12,3] int32 faces)."""
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], dtype=np.float64) * float(edge)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 dtype=np.int32)
    return v, f


def mesh_rectangle(nx, ny, xs=None, ys=None):
    """the rectangle [xs[0], xs[-1]] x [ys[0], ys[-1]] in the plane z = 0 as nx x ny cells of two triangles each (the diagonal from a cell's
    low corner): ([(nx+1)(ny+1),3] fp64 vertices, [2 nx ny,3] int32 faces).  xs / ys: the nx+1 / ny+1 grid coordinates (default: uniform on
    [-0.5, 0.5])."""
    xs = np.linspace(-0.5, 0.5, nx + 1) if xs is None else np.asarray(xs, dtype=np.float64)
    ys = np.linspace(-0.5, 0.5, ny + 1) if ys is None else np.asarray(ys, dtype=np.float64)
    assert xs.shape == (nx + 1,) and ys.shape == (ny + 1,)
    gx, gy = np.meshgrid(xs, ys)
    v = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    j, i = np.meshgrid(np.arange(nx), np.arange(ny))
    p = (i * (nx + 1) + j).ravel()
    f = np.concatenate([np.stack([p, p + 1, p + nx + 2], axis=1), np.stack([p, p + nx + 2, p + nx + 1], axis=1)], axis=0).astype(np.int32)
    return v, f


def mesh_icosphere(subdivisions, radius=1.0, perturb=0.0, seed=0):
    """icosahedron subdivided `subdivisions` times (20 * 4^s faces) on the sphere of `radius`; perturb > 0 scales every vertex radially by
    1 + perturb * (u - 0.5), u hashed per vertex: a non-convex, self-occluding closed surface."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, dtype=np.float64) / math.sqrt(1.0 + g * g) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.stack(v)
    scale = radius * (1.0 + perturb * (hash_uniform(seed, "icosphere/r", (len(v),)) - 0.5)) if perturb else np.full(len(v), float(radius))
    return v * scale[:, None], np.array(f, dtype=np.int32)


RENDER_SEEDS = {"cube": 141, "watertight": 142, "sphere": 143, "mixed": 144, "clip": 145}
# ^ the seeds golden G13 was drawn with (tests/golden/make_golden_g13.py moves on while a pixel centre sits within 1e-6 px of an edge)


def make_render_inputs(case, seed=None):
    """Scenes of the depth rasterizer, fp64: dict(vertices, faces (lists, one entry per class), labels, R, t, K (per instance), H, W, near, far, seed).

    "cube"        one 0.1 m cube, 4 random poses, 48 x 64, K with a skew term
    "watertight"  a fronto-parallel rectangle at z = 2 of 32 x 32 cells whose vertices project exactly onto the integer pixels 0, 2, .., 62, 63 of a
                  64 x 64 frame (power-of-two focal length: every quantity of the rasterizer is exact): every pixel centre lies on an edge or a vertex
    "sphere"      the perturbed icosphere (subdivision 3, 1280 faces), one pose, 96 x 128
    "mixed"       3 classes of 12 / 2048 / 1280 faces (cube, rectangle of 32 x 32 cells, perturbed icosphere), labels [2, 0, 1, 1, 0], 120 x 160
    "clip"        48 x 64: a cube half outside the frame | entirely outside | behind the camera | a strip along the viewing direction whose first
                  cell crosses the near plane | a cube beyond far"""
    seed = RENDER_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    near, far = 0.01, 6.5
    if case == "cube":
        H, W, N = 48, 64, 4
        meshes, labels = [mesh_cube(0.1)], np.zeros(N, dtype=np.int64)
        K = np.array([[70.0, 0.3, 31.7], [0.0, 71.0, 23.4], [0.0, 0.0, 1.0]])
        R = _random_rotations(seed, "R", N)
        t = np.concatenate([0.08 * u("t_xy", N, 2) - 0.04, 0.3 + 0.2 * u("t_z", N, 1)], axis=1)
    elif case == "watertight":
        H, W, N = 64, 64, 1
        px = np.concatenate([np.arange(0, 63, 2), [63]]).astype(np.float64)   # 33 grid lines: pixels 0, 2, .., 62, 63
        K = np.array([[32.0, 0.0, 8.0], [0.0, 32.0, 8.0], [0.0, 0.0, 1.0]])
        meshes, labels = [mesh_rectangle(32, 32, xs=2.0 * (px - 8.0) / 32.0, ys=2.0 * (px - 8.0) / 32.0)], np.zeros(N, dtype=np.int64)
        R, t = np.eye(3)[None].copy(), np.array([[0.0, 0.0, 2.0]])
    elif case == "sphere":
        H, W, N = 96, 128, 1
        meshes, labels = [mesh_icosphere(3, 0.06, 0.35, seed)], np.zeros(N, dtype=np.int64)
        K = np.array([[143.1, 0.0, 63.2], [0.0, 143.4, 47.6], [0.0, 0.0, 1.0]])
        R = _random_rotations(seed, "R", N)
        t = np.concatenate([0.04 * u("t_xy", N, 2) - 0.02, 0.3 + 0.1 * u("t_z", N, 1)], axis=1)
    elif case == "mixed":
        H, W, N = 120, 160, 5
        rv, rf = mesh_rectangle(32, 32)
        meshes = [mesh_cube(0.08), (rv * np.array([0.12, 0.09, 1.0]), rf), mesh_icosphere(3, 0.05, 0.35, seed)]
        labels = np.array([2, 0, 1, 1, 0], dtype=np.int64)
        K = LM_K.astype(np.float64) / 4.0
        K[2, 2] = 1.0
        R = _random_rotations(seed, "R", N)
        t = np.concatenate([0.2 * u("t_xy", N, 2) - 0.1, 0.4 + 0.3 * u("t_z", N, 1)], axis=1)
    elif case == "clip":
        H, W, N = 48, 64, 5
        sv, sf = mesh_rectangle(1, 4)
        meshes = [mesh_cube(0.1), (sv * np.array([0.05, 0.4, 1.0]), sf)]
        labels = np.array([0, 0, 0, 1, 0], dtype=np.int64)
        K = np.array([[70.0, 0.0, 31.7], [0.0, 71.0, 23.4], [0.0, 0.0, 1.0]])
        R = _random_rotations(seed, "R", N)
        t = np.array([[0.0, 0.0, 0.4], [0.9, 0.0, 0.4], [0.0, 0.0, -0.5], [0.0, 0.03, 0.2], [0.0, 0.0, 7.0]]) + 0.004 * (u("t_jit", N, 3) - 0.5)
        t[0, 0] = (W - 1 - K[0, 2]) / K[0, 0] * t[0, 2]   # the cube's centre projects onto the last pixel column
        # the strip: model y runs along the camera's z (from ~0 to ~0.4 m), tilted by about a degree so that no edge is axis-parallel
        axis = hash_normal(seed, "tilt_axis", (1, 3))
        R[3] = _axis_angle(axis / np.linalg.norm(axis), np.array([1.0]))[0] @ np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    else:
        raise ValueError(case)
    return dict(vertices=[m[0] for m in meshes], faces=[m[1] for m in meshes], labels=labels, R=R, t=t, K=np.repeat(K[None], N, axis=0),
                H=H, W=W, near=near, far=far, seed=seed)


# ----------------------------------------------------------------------------------------------
# scenes of the BOP errors (gdrnet_amd.bop_metrics, golden G14)
# ----------------------------------------------------------------------------------------------
BOP_METRIC_SEEDS = {"vsd": 151, "sym": 152}
# ^ the seeds golden G14 was drawn with (tests/golden/make_golden_g14.py moves on while a decision of the reference sits within rounding of its threshold)
BOP_VSD_DELTA = 0.015   # BOP's 15 mm


def make_bop_metric_inputs(case, seed=None):
    """Inputs of the BOP-error golden G14 (gdrnet_amd.bop_metrics against lib/pysixd/pose_error.py vsd / mssd / mspd), fp64, metres.

    "vsd"  12 rows in 3 test frames of 47 x 61 (a ragged last chunk and wave), four per frame, one per quadrant, over three mesh classes -- 0: a
           0.1 m cube, 1: the perturbed icosphere (subdivision 3), 2: a 0.12 x 0.09 m rectangle of 8 x 8 cells -- with a skew-free K per row (frame 2
           has another camera than frames 0 and 1).  Rows: 0 est = gt exactly | 3 est shifted off the object (empty intersection) | 4 est outside the
           frame | 5 gt hidden behind an occluder by more than delta, est with it (empty union) | the others est = gt rotated by 3 .. 25 degrees and
           shifted by up to 6 cm, mostly along the ray.  ``bop_test_depth`` makes the test images from the rows' ground-truth depth maps:
           the nearest surface per frame in front of a background plane, an occluder over the left half of row 1's object and over all of row 5's,
           a block of zero-depth holes over part of row 6's, +-2 mm hash noise.
    "sym"  41 rows cycling through four classes -- 0: 1031 points, 314 transformations (continuous about an axis that misses the origin); 1: 257
           points, 3 (the identity and two discrete ones with a translation part); 2: ONE point, the identity only (syms None); 3: 8195 points, 314
           -- estimates graded as in make_pose_metric_inputs("A") (times one of the class's transformations on every fourth row), rows 0 and 6 with
           est = gt (row 0, class 0: the reference's set of a continuous symmetry leaves the identity out, so its error is one rotation step, not 0),
           rows 5 and 8 with est = gt o S_k exactly for a k > 0, per-row K near the LM camera, 3 targets without an estimate."""
    from .bop_metrics import symmetry_transformations

    seed = BOP_METRIC_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    if case == "vsd":
        H, W, N = 47, 61, 12
        rv, rf = mesh_rectangle(8, 8)
        meshes = [mesh_cube(0.1), mesh_icosphere(3, 0.05, 0.35, seed), (rv * np.array([0.12, 0.09, 1.0]), rf)]
        diam = np.array([0.1 * math.sqrt(3.0), 0.115, 0.15])
        labels = np.arange(N, dtype=np.int64) % 3
        frame = np.arange(N, dtype=np.int64) // 4
        K1 = np.array([[70.0, 0.0, 30.3], [0.0, 71.0, 23.4], [0.0, 0.0, 1.0]])
        K2 = np.array([[64.5, 0.0, 29.1], [0.0, 63.0, 22.2], [0.0, 0.0, 1.0]])
        K = np.stack([K2 if f == 2 else K1 for f in frame])
        R_gt = _random_rotations(seed, "R_gt", N)
        for i in range(N):
            if labels[i] == 2:   # the rectangle: roughly facing the camera
                ax = hash_normal(seed, f"tilt{i}", (1, 3))
                R_gt[i] = _axis_angle(ax / np.linalg.norm(ax), np.array([25.0]))[0]
        z = 0.42 + 0.1 * u("t_z", N)
        centre = np.array([[15.0, 12.0], [45.0, 12.0], [15.0, 35.0], [45.0, 35.0]])[np.arange(N) % 4] + 3.0 * (u("t_px", N, 2) - 0.5)
        t_gt = np.stack([(centre[:, 0] - K[:, 0, 2]) / K[:, 0, 0] * z, (centre[:, 1] - K[:, 1, 2]) / K[:, 1, 1] * z, z], axis=1)
        ang = 3.0 + 22.0 * u("ang", N)
        axis = hash_normal(seed, "axis", (N, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        R_est = _axis_angle(axis, ang) @ R_gt
        dz = np.array([0.0, 0.012, -0.02, 0.0, 0.0, 0.01, 0.03, -0.045, 0.06, -0.008, 0.022, 0.04])
        t_est = t_gt * (1.0 + dz / z)[:, None] + 0.004 * (u("t_jit", N, 3) - 0.5)
        R_est[0], t_est[0] = R_gt[0], t_gt[0]
        R_est[3], t_est[3] = R_gt[3], t_gt[3] - np.array([0.2, 0.0, 0.0])   # (towards the frame's middle: it stays in view)
        t_est[4] = t_gt[4] + np.array([2.0, 0.0, 0.0])
        return dict(vertices=[m[0] for m in meshes], faces=[m[1] for m in meshes], diameters=diam, labels=labels, frame=frame, num_frames=3,
                    R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K, H=H, W=W, near=0.01, far=6.5, delta=BOP_VSD_DELTA,
                    taus=np.arange(0.05, 0.51, 0.05), background=1.5, occluded={1: "left", 5: "all"}, holes_row=6, noise=0.002, seed=seed)
    if case != "sym":
        raise ValueError(case)
    N, sizes, diam = 41, (1031, 257, 1, 8195), [0.2, 0.3, 0.1, 0.25]
    rz, rx = np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0])

    def hom(R, t):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, t
        return m.ravel().tolist()

    model_infos = [
        {"diameter": diam[0], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.01, -0.02, 0.0]}]},
        {"diameter": diam[1], "symmetries_discrete": [hom(rz, [0.01, -0.02, 0.0]), hom(rx, [0.0, 0.015, 0.005])]},
        {"diameter": diam[2]},
        {"diameter": diam[3], "symmetries_continuous": [{"axis": [0.6, 0.0, 0.8], "offset": [0.0, 0.03, 0.01]}]},
    ]
    syms = [symmetry_transformations(m) if len(m) > 1 else None for m in model_infos]
    points = [-0.1 + 0.2 * u(f"pts{c}", n, 3) for c, n in enumerate(sizes)]
    labels = np.arange(N, dtype=np.int64) % len(sizes)
    R_gt = _random_rotations(seed, "R_gt", N)
    t_gt = np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)
    q = u("quality", N)
    ang = 0.1 * 200.0 ** (0.7 * q + 0.3 * u("q_ang", N))
    off = 0.15 * (0.7 * q + 0.3 * u("q_off", N)) ** 2
    axis = hash_normal(seed, "axis", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    tdir = hash_normal(seed, "tdir", (N, 3))
    tdir /= np.linalg.norm(tdir, axis=1, keepdims=True)
    R_est = _axis_angle(axis, ang) @ R_gt
    t_est = t_gt + off[:, None] * tdir
    for i in range(N):
        s = syms[labels[i]]
        if s is not None and (i // len(sizes)) % 4 == 3:   # the estimate lands near another member of the symmetry set
            k = int(u(f"k{i}", 1)[0] * len(s[0]))
            R_est[i], t_est[i] = R_est[i] @ s[0][k], R_est[i] @ s[1][k] + t_est[i]
    for i in (0, 6):
        R_est[i], t_est[i] = R_gt[i], t_gt[i]
    for i, k in ((5, 2), (8, 200)):   # class 1, its last transformation | class 0, deep in the table
        S = syms[labels[i]]
        R_est[i], t_est[i] = R_gt[i] @ S[0][k], R_gt[i] @ S[1][k] + t_gt[i]
    K = np.repeat(LM_K.astype(np.float64)[None], N, axis=0)
    K[:, 0, 0] += 4.0 * (u("fx", N) - 0.5)
    K[:, 1, 1] += 4.0 * (u("fy", N) - 0.5)
    K[:, :2, 2] += 6.0 * (u("c", N, 2) - 0.5)
    return dict(points=points, diameters=np.array(diam), model_infos=model_infos, syms=syms, obj_names=["can", "box", "dot", "bowl"], labels=labels,
                R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K, im_width=640, missing={0: 2, 2: 1}, exact_rows={6: 0, 5: 2, 8: 200}, seed=seed)


def bop_test_depth(inp, depth_gt):
    """The test images [F,H,W] fp32 of a make_bop_metric_inputs("vsd") scene from its rows' ground-truth depth maps ``depth_gt`` [N,H,W] (the host
    rasterizer's or the device's: they hold the same bits): per frame the nearest ground-truth surface, ``background`` where there is none; an
    occluder 0.1 m in front of the left half (row 1) / of all (row 5) of an object's bounding box, grown by 8 pixels all round for "all" so that a
    displaced estimate stays behind it; a 5 x 4 block of zero-depth holes from the centre of row 6's bounding box; then +-``noise`` m of hash noise on
    every valid pixel and one rounding to fp32."""
    depth_gt = np.asarray(depth_gt, dtype=np.float64)
    N, H, W = depth_gt.shape
    out = np.full((inp["num_frames"], H, W), float(inp["background"]))
    for i in range(N):
        f, d = int(inp["frame"][i]), depth_gt[i]
        out[f] = np.where((d > 0) & (d < out[f]), d, out[f])

    def bbox(i):
        ys, xs = np.nonzero(depth_gt[i] > 0)
        return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())

    for i, how in inp["occluded"].items():
        x1, y1, x2, y2 = bbox(i)
        if how == "left":
            x2 = (x1 + x2) // 2
        else:
            x1, y1, x2, y2 = max(x1 - 8, 0), max(y1 - 8, 0), min(x2 + 8, W - 1), min(y2 + 8, H - 1)
        out[int(inp["frame"][i]), y1 : y2 + 1, x1 : x2 + 1] = depth_gt[i][depth_gt[i] > 0].min() - 0.1
    out += inp["noise"] * (2.0 * hash_uniform(inp["seed"], "test_noise", out.shape) - 1.0)
    x1, y1, x2, y2 = bbox(inp["holes_row"])
    cx, cy = (x1 + x2) // 2, (y1 + y2) // 2
    out[int(inp["frame"][inp["holes_row"]]), cy : cy + 4, cx : cx + 5] = 0.0
    return out.astype(np.float32)


# ----------------------------------------------------------------------------------------------
# scenes of the complement-over-union errors (gdrnet_amd.cou_metrics, golden G19)
# ----------------------------------------------------------------------------------------------
COU_SEEDS = {"cus": 211}
# ^ the seed golden G19 was drawn with (tests/golden/make_golden_g19.py moves on while a required row is missing, a pixel centre of a render lies
#   within 1e-6 px of a triangle edge or a cus sits within 1e-6 of the 0.5 threshold)
COU_ROWS = {"exact": 0, "off_object": 1, "est_outside": 2, "both_empty": 3, "cut_left": 4, "cut_right": 5, "cut_top": 6, "cut_bottom": 7}
COU_GRADED = (8, 9, 10, 11, 12, 13)          # est = gt shifted across the image plane by COU_SHIFTS of the object's size, slightly rotated
COU_SHIFTS = (0.17, 0.24, 0.3, 0.44, 0.52, 0.6)
# x, y, w, h pairs for cou_bb: identical | disjoint | touching along a vertical edge (w_inter == 0) | touching along a horizontal edge | touching
# in a corner | contained | containing | zero-area est | zero-area both at one place | partial overlap | the same shifted into negative
# coordinates | fractional overlap | fractional touching | fractional contained | a one-pixel box inside | large coordinates
COU_BB_PAIRS = (
    ((3, 4, 10, 6), (3, 4, 10, 6)), ((0, 0, 5, 5), (20, 30, 4, 4)), ((0, 0, 5, 5), (5, 0, 5, 5)), ((2, 1, 6, 3), (2, 4, 6, 7)),
    ((0, 0, 5, 5), (5, 5, 2, 2)), ((4, 4, 3, 2), (0, 0, 20, 10)), ((0, 0, 20, 10), (4, 4, 3, 2)), ((3, 3, 0, 4), (0, 0, 10, 10)),
    ((5, 5, 0, 0), (5, 5, 0, 0)), ((0, 0, 10, 10), (5, 7, 10, 10)), ((-8, -9, 10, 10), (-3, -2, 10, 10)), ((0.5, 0.25, 3.75, 2.5), (1.125, 1.0, 4.3, 2.2)),
    ((0.1, 0.2, 0.7, 0.3), (0.8, 0.2, 0.9, 0.3)), ((1.3, 1.7, 0.9, 1.1), (0.2, 0.4, 7.7, 5.9)), ((7, 3, 1, 1), (5, 2, 6, 4)),
    ((100000, 200000, 3000, 1000), (101000, 200500, 3000, 1000)),
)


def make_cou_inputs(case, seed=None):
    """Inputs of the complement-over-union golden G19 (gdrnet_amd.cou_metrics against lib/pysixd/pose_error.py cus / cou_mask / cou_bb), fp64, metres.

    "cus"  14 rows in frames of 47 x 61 (H * W = 2867 is odd: a row's slice of the batch starts at any alignment) over the three mesh classes of
           make_bop_metric_inputs("vsd") -- 0: a 0.1 m cube, 1: the perturbed icosphere, 2: a 0.12 x 0.09 m rectangle -- with a skew-free K per
           row (rows 10 and up have another camera).  Rows (COU_ROWS): 0 est = gt exactly | 1 est shifted off the object, both in view
           (intersection 0) | 2 est outside the frame | 3 gt outside the frame and est behind the near plane (union 0) | 4 .. 7 the est
           silhouette cut by the left, right, top, bottom frame edge | COU_GRADED: est = gt rotated by 2 .. 8 degrees and shifted across the
           image plane by COU_SHIFTS of the object's apparent size, so that cus falls on both sides of its 0.5 threshold."""
    if case != "cus":
        raise ValueError(case)
    seed = COU_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    H, W, N = 47, 61, 14
    rv, rf = mesh_rectangle(8, 8)
    meshes = [mesh_cube(0.1), mesh_icosphere(3, 0.05, 0.35, seed), (rv * np.array([0.12, 0.09, 1.0]), rf)]
    size = np.array([0.1, 0.1, 0.09])               # the extent a shift is measured in, per class
    labels = np.arange(N, dtype=np.int64) % 3
    K1 = np.array([[70.0, 0.0, 30.3], [0.0, 71.0, 23.4], [0.0, 0.0, 1.0]])
    K2 = np.array([[64.5, 0.0, 29.1], [0.0, 63.0, 22.2], [0.0, 0.0, 1.0]])
    K = np.stack([K2 if i >= 10 else K1 for i in range(N)])
    R_gt = _random_rotations(seed, "R_gt", N)
    for i in range(N):
        if labels[i] == 2:   # the rectangle: roughly facing the camera
            ax = hash_normal(seed, f"tilt{i}", (1, 3))
            R_gt[i] = _axis_angle(ax / np.linalg.norm(ax), np.array([25.0]))[0]
    z = 0.42 + 0.1 * u("t_z", N)
    centre = np.array([30.0, 23.0]) + 6.0 * (u("t_px", N, 2) - 0.5)

    def at(i, px):   # the translation that puts the model origin of row i on pixel px at depth z[i]
        return np.array([(px[0] - K[i, 0, 2]) / K[i, 0, 0] * z[i], (px[1] - K[i, 1, 2]) / K[i, 1, 1] * z[i], z[i]])

    t_gt = np.stack([at(i, centre[i]) for i in range(N)])
    ang = 2.0 + 6.0 * u("ang", N)
    axis = hash_normal(seed, "axis", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    R_est = _axis_angle(axis, ang) @ R_gt
    t_est = t_gt + 0.004 * (u("t_jit", N, 3) - 0.5)
    r = COU_ROWS
    R_est[r["exact"]], t_est[r["exact"]] = R_gt[r["exact"]], t_gt[r["exact"]]
    i = r["off_object"]
    t_gt[i], t_est[i] = at(i, (14.0, 22.0)), at(i, (46.0, 25.0))
    t_est[r["est_outside"]] = t_gt[r["est_outside"]] + np.array([2.0, 0.0, 0.0])
    i = r["both_empty"]
    t_gt[i], t_est[i] = t_gt[i] + np.array([0.0, -2.0, 0.0]), t_gt[i] * np.array([1.0, 1.0, -1.0])
    for name, px, inward in (("cut_left", (2.0, 20.0), (10.0, 1.0)), ("cut_right", (58.5, 27.0), (-10.0, -1.0)), ("cut_top", (25.0, 1.5), (1.0, 14.0)),
                             ("cut_bottom", (35.0, 44.5), (-1.0, -10.0))):
        i = r[name]
        jit = u(f"cut_{name}", 2) - 0.5
        t_est[i] = at(i, np.array(px) + jit)
        t_gt[i] = at(i, np.array(px) + jit + np.array(inward))
    for i, s in zip(COU_GRADED, COU_SHIFTS):
        th = 2.0 * np.pi * u(f"dir{i}", 1)[0]
        t_est[i] = t_gt[i] + s * size[labels[i]] * np.array([np.cos(th), np.sin(th), 0.0])
    return dict(vertices=[m[0] for m in meshes], faces=[m[1] for m in meshes], labels=labels, obj_names=["cube", "blob", "card"], R_est=R_est,
                t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K, H=H, W=W, near=0.01, far=6.5, rows=dict(COU_ROWS), graded=COU_GRADED,
                bb_pairs=np.array(COU_BB_PAIRS, dtype=np.float64), seed=seed)


# ----------------------------------------------------------------------------------------------
# estimates and depth frames of the depth refinement (gdrnet_amd.refine)
# ----------------------------------------------------------------------------------------------
REFINE_SEEDS = {"sphere": 231, "mixed": 232, "noisy": 233, "degenerate": 234}
REFINE_CASES = tuple(REFINE_SEEDS)
REFINE_OCCLUDER = 0.05   # metres in front of the object's nearest point


def _refine_starts(seed, R_gt, t_gt, target, deg, mm):
    """the ground truth `target[k]` turned by deg[k] degrees about a hashed axis through the model origin and moved by mm[k] millimetres along a
    hashed direction"""
    n = len(target)
    axis, direction = hash_normal(seed, "start/axis", (n, 3)), hash_normal(seed, "start/dir", (n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    R0 = _axis_angle(axis, np.asarray(deg, dtype=np.float64)) @ R_gt[target]
    t0 = t_gt[target] + 1e-3 * np.asarray(mm, dtype=np.float64)[:, None] * direction
    return R0, t0


def make_refine_inputs(case, seed=None):
    """Inputs of the depth refinement (gdrnet_amd.refine), fp64, metres, built from make_render_inputs' meshes and ground-truth poses.  The depth
    frames are not in here: ``refine_scene(inp, depth_gt)`` composes them from renders of the ground truth (the device's or the host's).

    "sphere"      the 96 x 128 scene of make_render_inputs("sphere"); two estimates of its one pose: 5 degrees / 5 mm and 2 degrees / 2 mm off
    "mixed"       the 120 x 160 scene of make_render_inputs("mixed") (icosphere, cube, rectangle, rectangle, cube); ground truths {0, 1, 2} in frame
                  0, {3, 4} in frame 1; one estimate per ground truth, 5 / 5 off (even rows) or 2 / 2 off (odd rows), and a second estimate of the
                  icosphere, 2 / 2 off (row 5).  ``convergent`` = the rows of the icosphere: a cube seen on two faces slides along their common
                  edge under point-to-plane ICP, and a rectangle leaves three directions unobservable
    "noisy"       a LIST of two inputs: "sphere", and the icosphere of "mixed" alone in its frame, each with the frame rounded to whole
                  millimetres (a BOP depth PNG) behind an occluder REFINE_OCCLUDER in front of the left third of the object's box
    "degenerate"  the fronto-parallel rectangle of make_render_inputs("watertight"), which fills its 64 x 64 frame up to the last row and column:
                  all normals are equal.  Row 0: 0.2 degrees / 2 mm off (within the distance gate everywhere); row 1: moved out of the frame; row 2: behind the camera

    Keys: vertices, faces (per class), gt_labels, R_gt, t_gt, gt_frame [G]; labels, target (its ground truth), R0, t0, K, frame, start_deg,
    start_mm [N]; num_frames, H, W, near, far, round_mm, occluded (ground truths behind an occluder), convergent (rows), seed."""
    if case not in REFINE_SEEDS:
        raise ValueError(case)
    seed = REFINE_SEEDS[case] if seed is None else seed
    if case == "noisy":
        parts = []
        for k, base in enumerate(("sphere", "mixed")):
            inp = make_refine_inputs(base, seed + 1000 * k)
            keep = [i for i, g in enumerate(inp["target"]) if g == 0]   # the icosphere's rows
            for key in ("labels", "target", "R0", "t0", "K", "frame", "start_deg", "start_mm"):
                inp[key] = inp[key][keep]
            for key in ("gt_labels", "R_gt", "t_gt", "gt_frame"):
                inp[key] = inp[key][:1]
            inp.update(num_frames=1, round_mm=True, occluded=(0,), convergent=tuple(range(len(keep))), case="noisy/" + base)
            parts.append(inp)
        return parts
    base = make_render_inputs({"sphere": "sphere", "mixed": "mixed", "degenerate": "watertight"}[case])
    R_gt, t_gt, gt_labels = base["R"], base["t"], np.asarray(base["labels"], dtype=np.int64)
    if case == "sphere":
        target, deg, mm, gt_frame = [0, 0], [5.0, 2.0], [5.0, 2.0], [0]
        convergent = (0, 1)
    elif case == "mixed":
        target, deg, mm, gt_frame = [0, 1, 2, 3, 4, 0], [5.0, 2.0, 5.0, 2.0, 5.0, 2.0], [5.0, 2.0, 5.0, 2.0, 5.0, 2.0], [0, 0, 0, 1, 1]
        convergent = (0, 5)
    else:
        target, deg, mm, gt_frame = [0, 0, 0], [0.2, 0.0, 0.0], [2.0, 0.0, 0.0], [0]
        convergent = ()
    target, gt_frame = np.array(target, dtype=np.int64), np.array(gt_frame, dtype=np.int64)
    R0, t0 = _refine_starts(seed, R_gt, t_gt, target, deg, mm)
    if case == "degenerate":
        t0[1] = t_gt[0] + np.array([50.0, 0.0, 0.0])
        t0[2] = t_gt[0] * np.array([1.0, 1.0, -1.0])
    return dict(vertices=base["vertices"], faces=base["faces"], gt_labels=gt_labels, R_gt=R_gt, t_gt=t_gt, gt_frame=gt_frame,
                labels=gt_labels[target], target=target, R0=R0, t0=t0, K=base["K"][target], frame=gt_frame[target],
                start_deg=np.array(deg), start_mm=np.array(mm), num_frames=int(gt_frame.max()) + 1, H=base["H"], W=base["W"], near=base["near"],
                far=base["far"], round_mm=False, occluded=(), convergent=convergent, seed=seed, case=case)


def refine_scene(inp, depth_gt):
    """The observed frames [F,H,W] fp32 of a make_refine_inputs scene from the depth maps ``depth_gt`` [G,H,W] of its ground truths (the host
    rasterizer's or the device's): per frame the nearest ground-truth surface, 0 (no measurement) where there is none; for a ground truth in
    ``occluded`` a block REFINE_OCCLUDER in front of its nearest point over the left third of its bounding box; with ``round_mm`` every depth
    rounded to whole millimetres; one rounding to fp32."""
    depth_gt = np.asarray(depth_gt, dtype=np.float64)
    G, H, W = depth_gt.shape
    out = np.full((inp["num_frames"], H, W), np.inf)
    for g in range(G):
        f, d = int(inp["gt_frame"][g]), depth_gt[g]
        out[f] = np.where((d > 0) & (d < out[f]), d, out[f])
    out[np.isinf(out)] = 0.0
    for g in inp["occluded"]:
        ys, xs = np.nonzero(depth_gt[g] > 0)
        x1, x2 = int(xs.min()), int(xs.max())
        out[int(inp["gt_frame"][g]), int(ys.min()) : int(ys.max()) + 1, x1 : x1 + (x2 - x1 + 1) // 3] = depth_gt[g][depth_gt[g] > 0].min() - REFINE_OCCLUDER
    if inp["round_mm"]:
        out = np.round(out * 1000.0) / 1000.0
    return out.astype(np.float32)


# ----------------------------------------------------------------------------------------------
# flat-faced objects for the silhouette term of the depth refinement (gdrnet_amd.refine.icp_refine_sil)
# ----------------------------------------------------------------------------------------------
SILHOUETTE_CASES = ("isolated", "occluded")
SILHOUETTE_GROW = 6   # pixels the occluder reaches beyond the object's box
SILHOUETTE_STARTS = (((0.0, 0.0, 1.0), 0.0, (3.0, 0.0, 0.0)), ((0.0, 0.0, 1.0), 3.0, (2.0, -2.0, 0.0)), ((1.0, 1.0, 0.2), 2.0, (2.0, 1.0, 2.0)),
                     ((0.2, 1.0, 0.5), 4.0, (-4.0, 3.0, -3.0)))
SILHOUETTE_EXTRA_START = ((1.0, 0.2, 0.1), 3.0, (4.0, 2.0, 1.0))   # "occluded" only


def make_silhouette_inputs(case):
    """Inputs of the silhouette term (gdrnet_amd.refine.icp_refine_sil), fp64, metres: flat-faced objects alone in 96 x 128 frames at 0.6 m under
    K = [[600, 0, 63.5], [0, 600, 47.5], [0, 0, 1]] (a pixel's footprint is 1 mm), one ground truth per frame.  The frames and masks are not in
    here: ``silhouette_scene(inp, depth_gt)`` composes them from renders of the ground truth.

    "isolated"  ground truths 0: an 80 x 60 mm plate, fronto-parallel; 1: the plate tilted; 2: a 50 mm cube seen on two faces; 3: the cube seen
                on three.  Four starts each (rows 4 g .. 4 g + 3), 0-4 degrees and 3-6 mm off.  Depth alone leaves 0 - 2 degenerate
    "occluded"  ground truths 1 and 2 of "isolated", each behind a block REFINE_OCCLUDER in front of its nearest point over the left third of its
                box, grown by SILHOUETTE_GROW pixels; five starts each

    Keys: those of make_refine_inputs, and ``flat`` (the rows whose ground truth depth alone cannot refine)."""
    if case not in SILHOUETTE_CASES:
        raise ValueError(case)
    H, W = 96, 128
    K = np.array([[600.0, 0.0, 63.5], [0.0, 600.0, 47.5], [0.0, 0.0, 1.0]])
    rot = lambda axis, deg: _axis_angle(np.array([axis], dtype=np.float64) / np.linalg.norm(axis), np.array([float(deg)]))[0]  # noqa: E731
    vertices, faces = zip(mesh_rectangle(4, 3, xs=np.linspace(-0.04, 0.04, 5), ys=np.linspace(-0.03, 0.03, 4)), mesh_cube(0.05))
    R_gt = np.stack([np.eye(3), rot([1, 0.3, 0], 25) @ rot([0, 0, 1], 17), rot([0, 1, 0], 40), rot([1, 0, 0], 30) @ rot([0, 1, 0], 40)])
    gt_labels = np.array([0, 0, 1, 1], dtype=np.int64)
    starts = list(SILHOUETTE_STARTS)
    flat_gt = (0, 1, 2)
    if case == "occluded":
        R_gt, gt_labels, starts, flat_gt = R_gt[1:3], gt_labels[1:3], starts + [SILHOUETTE_EXTRA_START], (0, 1)
    G, S = len(gt_labels), len(starts)
    t_gt = np.array([[0.004, -0.003, 0.6]]).repeat(G, axis=0)
    target = np.repeat(np.arange(G), S)
    turn = np.stack([rot(a, d) for a, d, _ in starts])
    move = 1e-3 * np.array([m for _, _, m in starts])
    k = np.tile(np.arange(S), G)
    return dict(vertices=list(vertices), faces=list(faces), gt_labels=gt_labels, R_gt=R_gt, t_gt=t_gt, gt_frame=np.arange(G), labels=gt_labels[target],
                target=target, R0=turn[k] @ R_gt[target], t0=t_gt[target] + move[k], K=K[None].repeat(G * S, axis=0), frame=target.copy(),
                start_deg=np.array([d for _, d, _ in starts])[k], start_mm=np.linalg.norm(move, axis=1)[k] * 1e3, num_frames=G, H=H, W=W,
                near=0.01, far=6.5, occluded=tuple(range(G)) if case == "occluded" else (),
                flat=tuple(int(r) for r in np.nonzero(np.isin(target, flat_gt))[0]), case=case)


def silhouette_scene(inp, depth_gt):
    """(frames [F,H,W] fp32, masks [G,H,W] uint8) of a make_silhouette_inputs scene from the depth maps ``depth_gt`` [G,H,W] of its ground
    truths: the frame of an object is its render, its mask the render > 0; for a ground truth in ``occluded`` a block REFINE_OCCLUDER in front of
    its nearest point covers the left third of its box, grown by SILHOUETTE_GROW pixels on the three outer sides, and the mask is the visible part."""
    depth_gt = np.asarray(depth_gt, dtype=np.float32)
    frames, masks = depth_gt.copy(), (depth_gt > 0).astype(np.uint8)
    H, W = depth_gt.shape[1:]
    for g in inp["occluded"]:
        ys, xs = np.nonzero(depth_gt[g] > 0)
        x1, x2, g6 = int(xs.min()), int(xs.max()), SILHOUETTE_GROW
        box = (slice(max(int(ys.min()) - g6, 0), min(int(ys.max()) + 1 + g6, H)), slice(max(x1 - g6, 0), x1 + (x2 - x1 + 1) // 3))
        frames[g][box] = np.float32(np.float64(depth_gt[g][depth_gt[g] > 0].min()) - REFINE_OCCLUDER)
        masks[g][box] = 0
    return frames, masks


# ----------------------------------------------------------------------------------------------
# estimates of the YCB-V score tables (gdrnet_amd.sixd_scores, golden G18)
# ----------------------------------------------------------------------------------------------
SIXD_SCORE_SEEDS = {"sym": 191}
# ^ the seed golden G18 was drawn with (tests/golden/make_golden_g18.py moves on while an error of the reference, normalised as its score script
#   normalises it, sits within 1e-6 relative of one of its thresholds)
SIXD_SYM_CLASSES = (0, 1)   # the classes whose "ad" is adi (the fixture's dp_model["symmetric_obj_ids"]); classes 2 (the single point) and 3 (8195 points) take add


def make_sixd_score_inputs(case="sym", seed=None):
    """Inputs of the score golden G18 (gdrnet_amd.sixd_scores against lib/pysixd/pose_error.py add / adi / re_sym / te_sym / arp_2d_sym and the
    toolkit's matching and recall), fp64, metres: the rows of ``make_bop_metric_inputs("sym")`` drawn with this fixture's own seed -- 41 estimates
    graded from exact to far over four classes (1031 points x 314 transformations | 257 x 3 with translation parts | ONE point, identity only |
    8195 x 314), rows 0 and 6 with est = gt, rows 5 and 8 with est = gt o S_k, every fourth estimate of a symmetric class near another member of
    its set, 3 targets without an estimate -- plus ``sym_classes``, the classes scored with adi under "ad"."""
    if case != "sym":
        raise ValueError(case)
    inp = make_bop_metric_inputs("sym", seed=SIXD_SCORE_SEEDS[case] if seed is None else seed)
    inp["sym_classes"] = SIXD_SYM_CLASSES
    return inp


# ----------------------------------------------------------------------------------------------
# vertex clouds of the model preparation (gdrnet_amd.model_prep, golden G16)
# ----------------------------------------------------------------------------------------------
MODEL_PREP_SEED = 161
MODEL_PREP_CASES = ("rand1000", "rand1029", "rand8209", "rand70000", "sphere642", "grid125", "repeat20", "single")
MODEL_PREP_BOX = np.array([0.12, 0.08, 0.2])   # metres: the size of an LM object


def make_model_prep_inputs(case):
    """[n,3] fp64 vertices of one object of golden G16 (the reference's FPS, diameter and box on them); deterministic, nothing is read.

    "rand<n>"    n points uniform in a 0.12 x 0.08 x 0.2 m box (fp64 values that fp32 does not hold: the rounding is part of the case)
    "sphere642"  the perturbed icosphere (subdivision 3) of 0.05 m radius
    "grid125"    the 5 x 5 x 5 grid of spacing 0.25: exact ties throughout, and its centre point sits exactly on the centre of the box
    "repeat20"   5 distinct points, 4 times over: any K above 5 is beyond the number of distinct points
    "single"     one point"""
    u = lambda tag, *shape: hash_uniform(MODEL_PREP_SEED, f"{case}/{tag}", shape)  # noqa: E731
    if case.startswith("rand"):
        return (u("p", int(case[4:]), 3) - 0.5) * MODEL_PREP_BOX
    if case == "sphere642":
        return mesh_icosphere(3, 0.05, 0.35, MODEL_PREP_SEED)[0]
    if case == "grid125":
        g = np.arange(5, dtype=np.float64) * 0.25 - 0.5
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    if case == "repeat20":
        return np.tile((u("p", 5, 3) - 0.5) * MODEL_PREP_BOX, (4, 1))
    if case == "single":
        return (u("p", 1, 3) - 0.5) * MODEL_PREP_BOX
    raise ValueError(case)


def model_prep_shells(subdivisions, seed=MODEL_PREP_SEED):
    """one cloud from concentric perturbed icospheres (``mesh_icosphere`` with perturb 0.35), shell j of radius 0.05 (1 - 0.1 j) m and its own seed:
    a scanned object's vertex count without a file -- 10 * 4^s + 2 vertices per shell of subdivision s"""
    return np.concatenate([mesh_icosphere(s, 0.05 * (1.0 - 0.1 * j), 0.35, seed + j)[0] for j, s in enumerate(subdivisions)], axis=0)


def make_model_prep_workload():
    """the clouds tools/model_prep_time.py times: 21 objects of 16 008 vertices (shells of subdivision 5, 4, 4, 3) and one of 259 854 (7, 6, 6, 5,
    4, 3, 3), the sizes of a dataset of CAD models with one scanned mesh among them"""
    return [model_prep_shells((5, 4, 4, 3), MODEL_PREP_SEED + 10 * c) for c in range(21)] + [model_prep_shells((7, 6, 6, 5, 4, 3, 3), MODEL_PREP_SEED + 500)]


# ----------------------------------------------------------------------------------------------
# scenes of the scene ground truth (gdrnet_amd.scene_gt, golden G17)
# ----------------------------------------------------------------------------------------------
SCENE_GT_SEED = 171
# ^ the seed golden G17 was drawn with (tests/golden/make_golden_g17.py moves on while a pixel centre sits within 1e-6 px of an edge or a visibility
#   difference within 1e-5 m of delta)
SCENE_GT_CASES = ("mixed", "pad0")
# (instance, what it is there for): tests/test_scene_gt_cpu.py asserts each on the host results
SCENE_GT_KINDS = {"inside": 0, "truncated": 1, "outside_image": 2, "outside_canvas": 3, "partly_hidden": 4, "hider": 5, "fully_hidden": 6,
                  "cover": 7, "pair": (8, 9), "occluded_left": 10, "single": 11}


def make_scene_gt_inputs(case, seed=None):
    """Scenes of golden G17, fp64, metres: dict(vertices, faces (one entry per class), labels, frame, num_frames, R, t, K (of the image, per
    instance), H, W, pad, near, far, delta, background, occluded, holes_row, noise, seed).

    "mixed"  12 instances in 3 frames of 47 x 61 (a ragged last chunk and wave) with pad = (61, 47): a canvas of 141 x 183.  Classes -- 0: a 0.1 m
             cube, 1: the perturbed icosphere (subdivision 3), 2: a 0.12 x 0.09 m rectangle of 8 x 8 cells.  Frame 0 (instances 0-5): 0 fully
             inside the image and unoccluded | 1 truncated by the right and bottom border | 2 wholly left of the image, inside the canvas |
             3 outside the canvas | 4 a rectangle partly hidden by 5, a sphere 0.15 m in front of it.  Frame 1 (6-10): 6 a sphere fully hidden
             behind the cube 7 | 8 and 9 two parallel rectangles 8 mm apart along the viewing direction (closer than delta: both visible) |
             10 a cube whose left half ``scene_gt_depth`` puts behind an occluder.  Frame 2 (another camera): 11 alone.
    "pad0"   the same scene with pad = (0, 0): in-image statistics only."""
    if case not in SCENE_GT_CASES:
        raise ValueError(case)
    seed = SCENE_GT_SEED if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    H, W, N = 47, 61, 12
    rv, rf = mesh_rectangle(8, 8)
    meshes = [mesh_cube(0.1), mesh_icosphere(3, 0.05, 0.35, seed), (rv * np.array([0.12, 0.09, 1.0]), rf)]
    labels = np.array([1, 0, 1, 0, 2, 1, 1, 0, 2, 2, 0, 1], dtype=np.int64)
    frame = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2], dtype=np.int64)
    K1 = np.array([[70.0, 0.0, 30.3], [0.0, 71.0, 23.4], [0.0, 0.0, 1.0]])
    K2 = np.array([[64.5, 0.0, 29.1], [0.0, 63.0, 22.2], [0.0, 0.0, 1.0]])
    K = np.stack([K2 if f == 2 else K1 for f in frame])
    R = _random_rotations(seed, "R", N)
    for i in range(N):
        if labels[i] == 2:   # the rectangles: roughly facing the camera
            ax = hash_normal(seed, f"tilt{i}", (1, 3))
            R[i] = _axis_angle(ax / np.linalg.norm(ax), np.array([25.0]))[0]
    R[9] = R[8]
    #                  0           1           2            3             4           5           6           7           8           9          10          11
    centre = np.array([[14., 13.], [58., 38.], [-25., 20.], [400., 20.], [35., 14.], [41., 14.], [15., 15.], [15., 15.], [42., 13.], [43., 13.], [42., 35.], [30., 22.]])
    z = np.array([0.50, 0.45, 0.50, 0.50, 0.55, 0.40, 0.70, 0.40, 0.500, 0.508, 0.50, 0.45])
    jit = u("t_px", N, 2) - 0.5
    jit[9] = jit[8]
    jit[7] = jit[6]
    centre = centre + jit
    z = z + 0.01 * np.repeat(u("t_z", N // 2), 2)   # (pairs share their offset: 4 / 5, 6 / 7 and 8 / 9 keep their distance)
    t = np.stack([(centre[:, 0] - K[:, 0, 2]) / K[:, 0, 0] * z, (centre[:, 1] - K[:, 1, 2]) / K[:, 1, 1] * z, z], axis=1)
    return dict(vertices=[m[0] for m in meshes], faces=[m[1] for m in meshes], labels=labels, frame=frame, num_frames=3, R=R, t=t, K=K, H=H, W=W,
                pad=(W, H) if case == "mixed" else (0, 0), near=0.01, far=6.5, delta=0.015, background=1.5, occluded={10: "left"}, holes_row=8,
                noise=0.002, seed=seed)


def scene_gt_depth(inp, depth):
    """The frames' depth images [F,H,W] fp32 of a make_scene_gt_inputs scene from its instances' image-window depths ``depth`` [N,H,W], made as
    ``bop_test_depth`` makes the test images of VSD: the nearest surface per frame in front of a background plane, an occluder 0.1 m in front of
    the left half of instance 10, a 5 x 4 block of zero holes from the centre of instance 8's box, +-2 mm of hash noise."""
    return bop_test_depth(inp, depth)


# ----------------------------------------------------------------------------------------------
# scenes of the shaded renderer (gdrnet_amd.shade; the oracle is tests/shade_host.py, no golden)
# ----------------------------------------------------------------------------------------------
SHADE_SEEDS = {"cube": RENDER_SEEDS["cube"], "sphere": RENDER_SEEDS["sphere"], "watertight": RENDER_SEEDS["watertight"], "scene": 181}
# ^ cube, sphere and watertight reuse the geometry (and so the accepted seeds) of make_render_inputs; tests/test_shade_cpu.py asserts for all four
#   that no pixel centre sits within 1e-6 px of an edge without being exactly on it
SHADE_CASES = ("cube", "sphere", "watertight", "scene")
SHADE_PHONG = (0.4, 0.8, 0.3)         # gdrnet_amd.shade.PHONG / LIGHT (kept apart: this module imports nothing of the package)
SHADE_LIGHT = (0.4, -0.4, -0.4)
SHADE_SCENE_KINDS = {"sphere_in_front": 0, "tie_first": 1, "rectangle_behind": 2, "tie_second": 3, "truncated": 4, "outside": 5, "behind_camera": 6}


def make_shade_inputs(case, seed=None):
    """Scenes of the shaded renderer, fp64, metres: dict(vertices, faces, colors (one entry per class; floats in [0, 1] or u8), labels, frame,
    num_frames, R, t, K (per instance), H, W, near, far, light [F,3], phong [F,3], background [F,H,W,3] u8, seed).

    "cube"        the cube scene of make_render_inputs: 48 x 64, 4 poses, one per frame, skewed K; a distinct colour per vertex, large triangles
    "sphere"      the perturbed icosphere (1280 faces), 96 x 128, the same pose in 3 frames: the default light and weights | a light behind the
                  object (the diffuse clamp) | weights that saturate (the clamp at 1)
    "watertight"  the exact rectangle scene, 64 x 64: every pixel centre on an edge or a vertex, exact depth ties between faces; u8 colours
    "scene"       47 x 61 (a ragged last wave), 3 frames, 7 instances in mixed input order (SHADE_SCENE_KINDS).  Frame 0: a sphere in front of
                  a rectangle, a cube truncated by the right and bottom border.  Frame 1: two coincident rectangles of different colour (two
                  classes with the same geometry: an exact tie between instances), a cube outside the frame, a sphere behind the camera.
                  Frame 2: no instance."""
    if case not in SHADE_CASES:
        raise ValueError(case)
    seed = SHADE_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    if case != "scene":
        inp = make_render_inputs(case, seed)
        v, H, W = inp["vertices"][0], inp["H"], inp["W"]
    if case == "cube":
        F = 4
        frame = np.arange(4, dtype=np.int64)
        colors = [0.15 + 0.6 * (v / 0.1 + 0.5) + 0.1 * u("col", 8, 3)]   # the corners of a colour cube, jittered: all distinct, far apart
        light, phong = np.tile(SHADE_LIGHT, (F, 1)), np.tile(SHADE_PHONG, (F, 1))
        inp = dict(inp, faces=[inp["faces"][0][:, ::-1].copy()])   # mesh_cube winds clockwise seen from outside: reversed, the normals point outward
    elif case == "sphere":
        F = 3
        inp = dict(inp, labels=np.zeros(F, dtype=np.int64), R=np.repeat(inp["R"], F, axis=0), t=np.repeat(inp["t"], F, axis=0),
                   K=np.repeat(inp["K"], F, axis=0))
        frame = np.arange(F, dtype=np.int64)
        colors = [0.2 + 0.7 * u("col", len(v), 3)]
        light = np.stack([np.array(SHADE_LIGHT), inp["t"][0] + np.array([0.05, -0.03, 0.5]), np.array(SHADE_LIGHT)])
        phong = np.array([SHADE_PHONG, SHADE_PHONG, (1.5, 2.0, 1.0)])
    elif case == "watertight":
        F = 1
        frame = np.zeros(1, dtype=np.int64)
        colors = [np.floor(256.0 * u("col", len(v), 3)).astype(np.uint8)]
        light, phong = np.array([SHADE_LIGHT]), np.array([SHADE_PHONG])
    else:
        H, W, F, N = 47, 61, 3, 7
        rv, rf = mesh_rectangle(8, 8)
        rv = rv * np.array([0.12, 0.09, 1.0])
        sv, sf = mesh_icosphere(3, 0.05, 0.35, seed)
        cv, cf = mesh_cube(0.1)
        cf = cf[:, ::-1].copy()   # (outward normals, as in "cube")
        meshes = [(sv, sf), (rv, rf), (rv.copy(), rf.copy()), (cv, cf)]
        colors = [0.2 + 0.7 * u("col0", len(sv), 3), np.floor(40 + 200.0 * u("col1", len(rv), 3)).astype(np.uint8),
                  np.clip(np.array([0.9, 0.2, 0.1]) + 0.1 * (u("col2", len(rv), 3) - 0.5), 0.0, 1.0), 0.15 + 0.6 * (cv / 0.1 + 0.5) + 0.1 * u("col3", 8, 3)]
        labels = np.array([0, 1, 1, 2, 3, 3, 0], dtype=np.int64)
        frame = np.array([0, 1, 0, 1, 0, 1, 1], dtype=np.int64)
        K1 = np.array([[70.0, 0.0, 30.3], [0.0, 71.0, 23.4], [0.0, 0.0, 1.0]])
        R = _random_rotations(seed, "R", N)
        for i in (1, 2):   # the rectangles: roughly facing the camera, their normal (the winding's +z) turned towards it
            ax = hash_normal(seed, f"tilt{i}", (1, 3))
            R[i] = _axis_angle(ax / np.linalg.norm(ax), np.array([25.0]))[0] @ np.diag([1.0, -1.0, -1.0])
        R[3] = R[1]
        #                    0           1           2           3           4           5            6
        centre = np.array([[20., 20.], [36., 24.], [29., 23.], [36., 24.], [58., 38.], [400., 20.], [30., 22.]])
        z = np.array([0.40, 0.50, 0.55, 0.50, 0.45, 0.50, -0.50]) + 0.01 * u("t_z", 1)[0]
        centre = centre + (u("t_px", N, 2) - 0.5)
        centre[3] = centre[1]
        K = np.repeat(K1[None], N, axis=0)
        t = np.stack([(centre[:, 0] - K[:, 0, 2]) / K[:, 0, 0] * z, (centre[:, 1] - K[:, 1, 2]) / K[:, 1, 1] * z, z], axis=1)
        inp = dict(vertices=[m[0] for m in meshes], faces=[m[1] for m in meshes], labels=labels, R=R, t=t, K=K, H=H, W=W, near=0.01, far=6.5)
        light = np.array([SHADE_LIGHT, (-0.3, -0.2, -0.1), (0.0, 0.0, 0.0)])
        phong = np.array([SHADE_PHONG, (0.5, 0.7, 0.4), SHADE_PHONG])
    background = np.floor(256.0 * u("background", F, H, W, 3)).astype(np.uint8)
    return dict(vertices=inp["vertices"], faces=inp["faces"], colors=colors, labels=inp["labels"], frame=frame, num_frames=F, R=inp["R"], t=inp["t"],
                K=inp["K"], H=H, W=W, near=inp["near"], far=inp["far"], light=light, phong=phong, background=background, seed=seed)


# ----------------------------------------------------------------------------------------------
# scenes of the textured / flat-shaded renderer (gdrnet_amd.shade.render_frames_bop; the oracle is tests/tex_host.py, no golden)
# ----------------------------------------------------------------------------------------------
TEX_CASES = ("quad", "cube", "sphere", "scene")
TEX_SEEDS = {"quad": 201, "cube": SHADE_SEEDS["cube"], "sphere": SHADE_SEEDS["sphere"], "scene": SHADE_SEEDS["scene"]}
# ^ cube, sphere and scene reuse the geometry of make_shade_inputs; tests/test_shade_tex_cpu.py asserts for every case how many covered pixels sit
#   within 1e-9 of a texel boundary (none on "sphere")
TEX_QUAD_ORIGIN = (10, 13)   # the frame pixel (x, y) that shows texel (0, 0) of "quad"


def _texture(seed, tag, h, w):
    return np.floor(256.0 * hash_uniform(seed, tag, (h, w, 3))).astype(np.uint8)


def _sphere_uv(v):
    """longitude / latitude of the vertex directions as UV coordinates in [0, 1]; the triangles across the seam span the whole texture"""
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.stack([0.5 + np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi), 0.5 + np.arcsin(np.clip(d[:, 2], -1.0, 1.0)) / np.pi], axis=1)


def make_tex_inputs(case, seed=None):
    """Scenes of the textured renderer: the dict of make_shade_inputs without ``phong``, with ``colors`` entries that may be None (a class drawn
    gray), and with ``uvs`` (per class [n_c,2] fp64 or None), ``textures`` (per class [h,w,3] u8 in file row order or None), ``ambient`` [F].

    "quad"    32 x 32: a fronto-parallel rectangle at z = 2 whose 8 x 8 pixels [10, 18) x [13, 21) show the 8 x 8 texels of a random texture, one
              each: power-of-two focal length and dyadic coordinates, so that u w = x - 10 + 0.5 and v h = 20 - y + 0.5 exactly; ambient 1
    "cube"    the 4 cube poses of make_shade_inputs, a 5 x 7 texture, UV coordinates from -0.5 to 1.5 (clamp-to-edge), large slanted triangles
    "sphere"  the 1280-face icosphere with a 16 x 16 texture in 3 frames: light at the origin, ambient 0.5 | a light behind the object | ambient 0.9
    "scene"   the 47 x 61 scene of make_shade_inputs (3 frames, 7 instances, SHADE_SCENE_KINDS): a textured sphere (6 x 9 texels) in front of a
              vertex-coloured rectangle; the cube cut by the border has neither colours nor a texture (gray); of the two coincident rectangles
              the first in input order has a 1 x 1 texture, the second vertex colours; frame 2 is empty"""
    if case not in TEX_CASES:
        raise ValueError(case)
    seed = TEX_SEEDS[case] if seed is None else seed
    u = lambda tag, *shape: hash_uniform(seed, tag, shape)  # noqa: E731
    if case == "quad":
        H = W = 32
        x0, y0 = TEX_QUAD_ORIGIN
        K = np.array([[32.0, 0.0, 12.0], [0.0, 32.0, 12.0], [0.0, 0.0, 1.0]])
        xs, ys = (np.array([x0 - 0.5, x0 + 7.5]) - 12.0) / 16.0, (np.array([y0 - 0.5, y0 + 7.5]) - 12.0) / 16.0   # (z / f = 1 / 16)
        v, f = mesh_rectangle(1, 1, xs=xs, ys=ys)
        inp = dict(vertices=[v], faces=[f], colors=[0.2 + 0.7 * u("col", 4, 3)], labels=np.zeros(1, dtype=np.int64), frame=np.zeros(1, dtype=np.int64),
                   num_frames=1, R=np.eye(3)[None].copy(), t=np.array([[0.0, 0.0, 2.0]]), K=K[None].copy(), H=H, W=W, near=0.01, far=6.5,
                   light=np.zeros((1, 3)), background=np.floor(256.0 * u("background", 1, H, W, 3)).astype(np.uint8), seed=seed)
        uvs = [np.stack([(v[:, 0] - xs[0]) / (xs[1] - xs[0]), (ys[1] - v[:, 1]) / (ys[1] - ys[0])], axis=1)]   # v = 1 along the top edge
        textures, ambient = [_texture(seed, "tex", 8, 8)], np.ones(1)
    else:
        inp = make_shade_inputs(case, seed)
        del inp["phong"]
        F = inp["num_frames"]
        inp["light"] = np.zeros((F, 3))
        ambient = np.full(F, 0.5)
    if case == "cube":
        uv = -0.5 + 2.0 * u("uv", 8, 2)
        uv[0], uv[7] = (-0.5, -0.5), (1.5, 1.5)
        uvs, textures = [uv], [_texture(seed, "tex", 5, 7)]
    elif case == "sphere":
        uvs, textures = [_sphere_uv(inp["vertices"][0])], [_texture(seed, "tex", 16, 16)]
        inp["light"][1] = inp["t"][1] + np.array([0.05, -0.03, 0.5])
        ambient[2] = 0.9
    elif case == "scene":
        inp["labels"] = np.array([0, 2, 1, 1, 3, 3, 0], dtype=np.int64)   # tie_first: class 2 (textured), tie_second: class 1; the same geometry
        rv = inp["vertices"][2]
        uvs = [_sphere_uv(inp["vertices"][0]), None, (rv[:, :2] - rv[:, :2].min(axis=0)) / np.ptp(rv[:, :2], axis=0), None]
        textures = [_texture(seed, "tex0", 6, 9), None, _texture(seed, "tex2", 1, 1), None]
        inp["colors"] = inp["colors"][:3] + [None]
        inp["light"][1] = (-0.3, -0.2, -0.1)
        ambient[1] = 0.3
    return dict(inp, uvs=uvs, textures=textures, ambient=ambient)
