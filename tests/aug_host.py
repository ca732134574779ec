"""Host restatement (numpy) of the frame augmenter's arithmetic, stage by stage as include/gdrn_hip.h specifies it: the oracle of
gdrnet_amd.augment's kernels.  Written on its own (vectorised over the frame, point ops applied one after the other to the image rather than
through a composed table) so that it shares no code with the product module.  The cut and the composite are pinned to the reference's
``replace_bg`` by golden G15, the crop / scale / size of the background to its ``get_bg_image``; the 8-bit bilinear rule, CoarseDropout,
GaussianBlur and the point ops restate OpenCV 4 / imgaug 0.4 as published (neither library is in the image: parity with them is unpinned)."""
import numpy as np


def bg_geometry(bg_h, bg_w, H, W):
    """(ch, cw, s, oh, ow): get_bg_image's crop, resize_short_edge's scale, cv2.resize's output size clamped to the frame"""
    ratio = float(H) / float(W)
    frame_wide, bg_wide = ratio < 1, float(bg_h) / float(bg_w) < 1
    ch, cw = bg_h, bg_w
    if frame_wide == bg_wide:
        if bg_h >= bg_w:
            new = int(np.ceil(bg_w * ratio))
            if new < bg_h:
                ch = new
        else:
            new = int(np.ceil(bg_h / ratio))
            if new < bg_w:
                cw = new
    elif bg_h >= bg_w:
        ch = len(range(bg_h)[0 : int(np.ceil(bg_w * ratio))])
    else:
        cw = len(range(bg_w)[0 : int(np.ceil(bg_h / ratio))])
    target, max_size = min(H, W), max(H, W)
    s = float(target) / float(min(ch, cw))
    if np.round(s * max(ch, cw)) > max_size:
        s = float(max_size) / float(max(ch, cw))
    oh, ow = int(np.rint(ch * s)), int(np.rint(cw * s))
    return ch, cw, s, min(oh, H), min(ow, W)


def _taps(n_dst, inv, n_src):
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * inv - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= n_src - 1
    s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    w1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s, np.minimum(s + 1, n_src - 1), w0, w1


def background(bank_img, H, W):
    """the H x W x 3 background of a frame from one bank image: crop, 8-bit fixed-point bilinear resize, zero remainder"""
    ch, cw, s, oh, ow = bg_geometry(bank_img.shape[0], bank_img.shape[1], H, W)
    crop = bank_img[:ch, :cw].astype(np.int32)
    inv = 1.0 / s
    sx, sx1, a0, a1 = _taps(ow, inv, cw)
    sy, sy1, b0, b1 = _taps(oh, inv, ch)
    rows = crop[:, sx] * a0[None, :, None] + crop[:, sx1] * a1[None, :, None]   # [ch][ow][3] int32
    S0, S1 = rows[sy], rows[sy1]
    val = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    out = np.zeros((H, W, 3), np.uint8)
    out[:oh, :ow] = np.minimum(val, 255).astype(np.uint8)
    return out


def truncate_mask(mask, mode, u):
    """replace_bg's TRUNCATE_FG cut of a bool mask; an empty mask stays empty (the reference raises there)"""
    m = mask.astype(bool).copy()
    if not m.any():
        return m
    rows, cols = np.nonzero(m)
    r_min, r_max, c_min, c_max = rows.min(), rows.max(), cols.min(), cols.max()
    c_h, c_w = 0.5 * (r_min + r_max), 0.5 * (c_min + c_max)
    if mode == 0:
        m[: int(r_min + (c_h - r_min) * u), :] = False
    elif mode == 1:
        m[int(c_h + (r_max - c_h) * u) :, :] = False
    elif mode == 2:
        m[:, : int(c_min + (c_w - c_min) * u)] = False
    elif mode == 3:
        m[:, int(c_w + (c_max - c_w) * u) :] = False
    return m


def composite(frame, mask_trunc, bg):
    out = frame.copy()
    out[~mask_trunc] = bg[~mask_trunc]
    return out


def coarse_dropout(img, keep):
    H, W = img.shape[:2]
    gh, gw = keep.shape
    cy = np.minimum(np.floor(np.arange(H, dtype=np.float64) * gh / H).astype(np.int64), gh - 1)
    cx = np.minimum(np.floor(np.arange(W, dtype=np.float64) * gw / W).astype(np.int64), gw - 1)
    return img * np.asarray(keep, bool)[cy][:, cx][:, :, None].astype(np.uint8)


def gaussian_weights(sigma):
    ksize = max(int(3.3 * sigma), 5)
    if ksize % 2 == 0:
        ksize += 1
    r = ksize // 2
    w = np.array([np.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(-r, r + 1)], dtype=np.float64)
    return r, (w / w.sum()).astype(np.float32)


def gaussian_blur(img, sigma):
    if sigma < 1e-3:
        return img
    r, w = gaussian_weights(sigma)
    H, W = img.shape[:2]
    if H <= r or W <= r:
        raise ValueError("frame side <= blur radius")
    p = np.pad(img.astype(np.float32), ((r, r), (r, r), (0, 0)), mode="reflect")   # reflect-101
    acc = w[0] * p[:, 0:W]
    for k in range(1, 2 * r + 1):
        acc = acc + w[k] * p[:, k : k + W]            # fp32 products and sums, left to right
    out = w[0] * acc[0:H]
    for k in range(1, 2 * r + 1):
        out = out + w[k] * acc[k : k + H]             # top to bottom
    assert acc.dtype == np.float32 and out.dtype == np.float32
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def point_op(img, name, vals):
    out = img.copy()
    for c in range(3):
        ch = img[:, :, c]
        if name == "Add":
            out[:, :, c] = np.clip(ch.astype(np.int64) + int(vals[c]), 0, 255)
        elif name == "Multiply":
            out[:, :, c] = np.clip(ch.astype(np.float32) * np.float32(vals[c]), 0, 255).astype(np.uint8)
        elif name == "LinearContrast":
            v = np.float32(127) + np.float32(vals[c]) * (ch.astype(np.float32) - np.float32(127))
            assert v.dtype == np.float32
            out[:, :, c] = np.clip(v, 0, 255).astype(np.uint8)
        elif name == "Invert":
            if vals[c]:
                out[:, :, c] = 255 - ch
        else:
            raise ValueError(name)
    return out


def augment_frame(frame, mask, bank, plan, i):
    """frame i of an AugPlan on the host: (image, mask_trunc or None)"""
    img, trunc = frame, None
    if plan.replace_bg[i]:
        trunc = truncate_mask(mask != 0, plan.trunc_mode[i], plan.trunc_u[i])
        img = composite(frame, trunc, background(bank[plan.bg_index[i]], *frame.shape[:2]))
    if plan.color[i]:
        if plan.dropout[i] is not None:
            img = coarse_dropout(img, plan.dropout[i])
        if plan.blur_sigma[i] is not None:
            img = gaussian_blur(img, plan.blur_sigma[i])
        for name, vals in plan.point_ops[i]:
            img = point_op(img, name, vals)
    return img, (None if trunc is None else trunc.astype(np.uint8))
