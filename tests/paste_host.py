"""Host restatement (numpy, fp64) of the three entry points of csrc/roi_paste.hip, written from the text of include/gdrn_hip.h: the operation
sequence of p, the exclusivity rule, the area / box convention, and the largest 8-connected component by a flood fill of its own.  numpy's
elementwise fp64 products and sums are IEEE operations without contraction, so the device (contraction off) gives the same bits."""
import numpy as np


def clean(map_):
    """fp32 map as fp64 with every non-finite value 0"""
    m = np.asarray(map_, dtype=np.float32)
    return np.where(np.isfinite(m), m, np.float32(0)).astype(np.float64)


def sample(map_, cx, cy, scale, H, W):
    """(p [H, W] fp64, inside [H, W] bool): the header's p of every frame pixel; outside the RoI's square p is 0 and nothing is read"""
    m = clean(map_)
    res = m.shape[0]
    pad = np.zeros((res + 2, res + 2), dtype=np.float64)   # a tap outside the map is 0
    pad[1:-1, 1:-1] = m
    cx, cy, scale = np.float64(cx), np.float64(cy), np.float64(scale)
    with np.errstate(all="ignore"):
        k = np.float64(res) / scale
        u = (np.arange(W, dtype=np.float64) - cx) * k + np.float64(0.5 * res)
        v = (np.arange(H, dtype=np.float64) - cy) * k + np.float64(0.5 * res)
        in_u, in_v = (u > -1.0) & (u < res), (v > -1.0) & (v < res)   # False for a NaN
        u, v = np.where(in_u, u, 0.0), np.where(in_v, v, 0.0)
        u0, v0 = np.floor(u), np.floor(v)
        fu, fv = (u - u0)[None, :], (v - v0)[:, None]
        iu, iv = u0.astype(np.int64)[None, :] + 1, v0.astype(np.int64)[:, None] + 1
        m00, m01, m10, m11 = pad[iv, iu], pad[iv, iu + 1], pad[iv + 1, iu], pad[iv + 1, iu + 1]
        a = m00 * (1.0 - fu) + m01 * fu
        b = m10 * (1.0 - fu) + m11 * fu
        p = a * (1.0 - fv) + b * fv
    inside = in_v[:, None] & in_u[None, :]
    return np.where(inside, p, 0.0), inside


def stats(mask):
    """(area, [x1, y1, x2, y2]) of one mask: bottom-right inclusive; empty: 0 and the whole frame"""
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return 0, [0, 0, W - 1, H - 1]
    return len(ys), [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def _with_stats(mask):
    st = [stats(m) for m in mask]
    return dict(mask=mask, area=np.array([s[0] for s in st], dtype=np.int32), bbox=np.array([s[1] for s in st], dtype=np.int32).reshape(-1, 4))


def paste(maps, geom, H, W, thr):
    """dict(mask [B, H, W] uint8, area [B] int32, bbox [B, 4] int32); geom [B, 3] = cx, cy, scale; thr as the fp32 the library receives"""
    thr = np.float64(np.float32(thr))
    mask = np.zeros((len(maps), H, W), dtype=np.uint8)
    for n, (m, (cx, cy, s)) in enumerate(zip(maps, geom)):
        p, inside = sample(m, cx, cy, s, H, W)
        mask[n] = inside & (p > thr)
    return _with_stats(mask)


def paste_exclusive(maps, geom, frame, F, H, W, thr):
    """paste with every frame pixel given to the row of its frame with the greatest p above thr, the lowest row among equals; adds index [F, H, W]"""
    thr = np.float64(np.float32(thr))
    B = len(maps)
    index = np.full((F, H, W), -1, dtype=np.int32)
    best = np.zeros((F, H, W), dtype=np.float64)
    for n in range(B):   # ascending rows: strictly greater replaces
        f = int(frame[n])
        p, inside = sample(maps[n], *geom[n], H, W)
        take = inside & (p > thr) & ((index[f] < 0) | (p > best[f]))
        index[f][take] = n
        best[f][take] = p[take]
    mask = np.stack([(index[int(frame[n])] == n) for n in range(B)]).astype(np.uint8) if B else np.zeros((0, H, W), np.uint8)
    out = _with_stats(mask)
    out["index"] = index
    return out


def label(fg):
    """8-connected components of a boolean map by flood fill in row-major order: (labels int32 with -1 for background and 0, 1, ... in the
    order of each component's lowest row-major pixel index, sizes)"""
    res_y, res_x = fg.shape
    lab = np.full(fg.shape, -1, dtype=np.int32)
    sizes = []
    for y in range(res_y):
        for x in range(res_x):
            if not fg[y, x] or lab[y, x] >= 0:
                continue
            c = len(sizes)
            lab[y, x] = c
            stack, size = [(y, x)], 0
            while stack:
                yy, xx = stack.pop()
                size += 1
                for ny in range(max(yy - 1, 0), min(yy + 2, res_y)):
                    for nx in range(max(xx - 1, 0), min(xx + 2, res_x)):
                        if fg[ny, nx] and lab[ny, nx] < 0:
                            lab[ny, nx] = c
                            stack.append((ny, nx))
            sizes.append(size)
    return lab, np.array(sizes, dtype=np.int64)


def components(prob, thr):
    """dict(filtered, num_comp, kept_px) of prob [B, res, res] fp32: the most pixels, then the lowest row-major pixel index"""
    prob = np.asarray(prob, dtype=np.float32)
    thr = np.float32(thr)
    filtered = np.zeros_like(prob)
    num_comp, kept_px = np.zeros(len(prob), dtype=np.int32), np.zeros(len(prob), dtype=np.int32)
    for b, m in enumerate(prob):
        fg = np.where(np.isfinite(m), m, np.float32(0)) > thr
        lab, sizes = label(fg)
        num_comp[b] = len(sizes)
        if len(sizes):
            keep = int(np.argmax(sizes))   # the first of the largest: components are numbered by their lowest pixel index
            kept_px[b] = sizes[keep]
            filtered[b] = np.where(lab == keep, m, np.float32(0))
    return dict(filtered=filtered, num_comp=num_comp, kept_px=kept_px)


# ---------------------------------------------------------------------------------------------------------------------
# the shapes the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
FRAME_H, FRAME_W = 40, 56   # neither side a multiple of 16: vector tails and row ends
# (cx, cy, scale): inside | off the top-left | off the bottom-right | the identity scale | a 7x minification | wholly outside | a 2x magnification
GEOMS = ((20.3, 17.9, 37.7), (3.2, 5.1, 50.0), (55.0, 39.0, 21.0), (28.0, 20.0, 64.0), (30.5, 10.25, 9.0), (-40.0, -40.0, 20.0), (28.0, 20.0, 128.0))


def smooth_map(seed, tag, res=64, passes=3):
    """a predicted-like map: hashed noise under ``passes`` 5 x 5 box filters, stretched to [0, 1], fp32"""
    from gdrnet_amd import synth

    m = synth.hash_uniform(seed, tag, (res, res))
    for _ in range(passes):
        p = np.pad(m, 2, mode="edge")
        m = sum(p[dy:dy + res, dx:dx + res] for dy in range(5) for dx in range(5)) / 25.0
    return ((m - m.min()) / (m.max() - m.min())).astype(np.float32)


def geometry_maps(seed=83):
    """one map per geometry of GEOMS [7, 64, 64] fp32, each different"""
    return np.stack([smooth_map(seed, f"map{n}") for n in range(len(GEOMS))])
