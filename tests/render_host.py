"""Brute-force fp64 numpy rasterizer with the rules of gdrn_render_depth (include/gdrn_hip.h): every pixel against every triangle, no
acceleration structure.  This project's own oracle for gdrnet_amd.render; also measures how far the scene is from a coverage decision that
rounding could flip (the acceptance condition of the fixtures' seeds).

Rules: pixel (x, y) is sampled on d = K^-1 [x, y, 1] (integer coordinates); vertex indices of a face sorted ascending, edge normals on ascending
pairs; covered when d.(a x b), d.(b x c), d.(c x a) are all >= 0 or all <= 0; z = (n.a) / (n.d), n = (b - a) x (c - a); a triangle with a vertex at
z < near is dropped whole, as is a degenerate one; fragments with n.d == 0, z > far or a non-positive / non-finite fp32 depth are dropped; the
nearest fragment wins after the one rounding to fp32; 0 where nothing is drawn."""
import numpy as np

CHUNK = 64   # triangles per vectorised step


def pixel_rays(K, H, W):
    """(dx, dy) [H*W] of d = K^-1 [x, y, 1] for the upper-triangular K (third component 1), the operation order of the kernel."""
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dy = (y - cy) / fy
    dx = ((x - sk * dy) - cx) / fx
    return dx.ravel(), dy.ravel()


def render_one(verts, faces, R, t, K, H, W, near=0.01, far=6.5, stats=None):
    """depth [H,W] fp32 of one mesh under one pose.  `stats` (a dict) receives
      edge_band       the smallest |m| in pixels over all (pixel, kept triangle), m = the signed distance of the pixel centre to the triangle's
                      nearest edge line on the covered side: the pixel is covered iff m >= 0
      edge_band_off   the same over the pairs with m != 0 (scenes that put pixel centres exactly on edges on purpose)
      near_far_band   the smallest relative distance of a vertex depth to near, or of a covered fragment's depth to near or far"""
    verts, faces = np.asarray(verts, dtype=np.float64), np.sort(np.asarray(faces, dtype=np.int64), axis=1)
    vc = verts @ np.asarray(R, dtype=np.float64).T + np.asarray(t, dtype=np.float64)
    a, b, c = vc[faces[:, 0]], vc[faces[:, 1]], vc[faces[:, 2]]
    n = np.cross(b - a, c - a)
    keep = (a[:, 2] >= near) & (b[:, 2] >= near) & (c[:, 2] >= near) & np.any(n != 0, axis=1)
    a, b, c, n = a[keep], b[keep], c[keep], n[keep]
    E = np.stack([np.cross(a, b), np.cross(b, c), -np.cross(a, c)], axis=1)   # [T,3 edges,3]: a x b, b x c, c x a = -(a x c)
    na = np.einsum("ij,ij->i", n, a)
    dx, dy = pixel_rays(K, H, W)
    D = np.stack([dx, dy, np.ones_like(dx)], axis=0)   # [3, HW]
    fx, sk, fy = K[0, 0], K[0, 1], K[1, 1]
    best = np.full(H * W, np.inf, dtype=np.float32)
    band, band_off, nf_band = np.inf, np.inf, np.inf
    if stats is not None and len(faces):
        zs = vc[np.unique(faces)][:, 2]
        nf_band = float(np.min(np.abs(zs - near) / near))
    for s in range(0, len(a), CHUNK):
        Ec, nc, nac = E[s : s + CHUNK], n[s : s + CHUNK], na[s : s + CHUNK]
        w = np.einsum("tek,kp->tep", Ec, D)   # [T,3,HW]
        inside = np.all(w >= 0, axis=1) | np.all(w <= 0, axis=1)
        if stats is not None:
            gx, gy = Ec[:, :, 0] / fx, (Ec[:, :, 1] - sk * Ec[:, :, 0] / fx) / fy   # gradient of w over the pixel grid
            with np.errstate(divide="ignore", invalid="ignore"):
                dist = w / np.hypot(gx, gy)[:, :, None]
            dist = np.where(np.isnan(dist), 0.0, dist)
            m = np.abs(np.maximum(dist.min(axis=1), (-dist).min(axis=1)))   # either orientation counts
            band = min(band, float(m.min()))
            if np.any(m != 0):
                band_off = min(band_off, float(m[m != 0].min()))
        ti, pi = np.nonzero(inside)
        if len(ti) == 0:
            continue
        den = nc[ti, 0] * dx[pi] + (nc[ti, 1] * dy[pi] + nc[ti, 2])
        ok = den != 0
        ti, pi, den = ti[ok], pi[ok], den[ok]
        z = nac[ti] / den
        if stats is not None and len(z):
            pos = z > 0
            if np.any(pos):
                nf_band = min(nf_band, float(np.min(np.abs(z[pos] - far) / far)), float(np.min(np.abs(z[pos] - near) / near)))
        ok = ~(z > far)
        with np.errstate(over="ignore"):
            zf = z.astype(np.float32)
        ok &= (zf > 0) & np.isfinite(zf)
        np.minimum.at(best, pi[ok], zf[ok])
    if stats is not None:
        stats.update(edge_band=band, edge_band_off=band_off, near_far_band=nf_band)
    best[np.isinf(best)] = 0.0
    return best.reshape(H, W)


def render_depth(inp, stats=None):
    """depth [N,H,W] fp32 of a synth.make_render_inputs scene; `stats` receives the minima over the instances."""
    out, acc = [], []
    for i, c in enumerate(inp["labels"]):
        s = {} if stats is not None else None
        out.append(render_one(inp["vertices"][c], inp["faces"][c], inp["R"][i], inp["t"][i], inp["K"][i], inp["H"], inp["W"], inp["near"], inp["far"], s))
        acc.append(s)
    if stats is not None:
        for k in ("edge_band", "edge_band_off", "near_far_band"):
            stats[k] = min(s[k] for s in acc)
    return np.stack(out)


def xyz_from_depth(depth, R, t, K):
    """calc_xyz_bp_fast + mask2bbox_xyxy for one depth map, written from their definitions (R^T (depth K^-1 [x, y, 1] - t) times the mask
    depth != 0; inclusive bounds of the mask, the whole frame when it is empty): (xyz [H,W,3] fp64, mask [H,W] bool, xyxy, visible)."""
    H, W = depth.shape
    dx, dy = pixel_rays(K, H, W)
    z = depth.astype(np.float64).ravel()
    P = np.stack([z * dx, z * dy, z], axis=1) - np.asarray(t, dtype=np.float64)
    mask = depth != 0
    xyz = (P @ np.asarray(R, dtype=np.float64)).reshape(H, W, 3) * mask[:, :, None]
    if not mask.any():
        return xyz, mask, [0, 0, W - 1, H - 1], 0
    ys, xs = np.nonzero(mask)
    return xyz, mask, [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())], 1


def cube_depth_analytic(edge, R, t, K, H, W):
    """the depth of an axis-aligned cube of `edge` centred on the model origin by fp64 ray-box slab intersection in model space: an oracle that
    shares nothing with the triangle rasterizer.  (depth [H,W] fp64 with 0 = miss; the camera is outside the cube.)"""
    dx, dy = pixel_rays(K, H, W)
    d = np.stack([dx, dy, np.ones_like(dx)], axis=1) @ R   # R^T d per pixel
    o = -(np.asarray(t, dtype=np.float64) @ R)             # camera centre in model coordinates
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-0.5 * edge - o) / d, (0.5 * edge - o) / d
    lo, hi = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
    hit = (lo <= hi) & (lo > 0)
    return np.where(hit, lo, 0.0).reshape(H, W), (hi - lo).reshape(H, W)
