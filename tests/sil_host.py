"""Plain numpy fp64 restatement of the silhouette term of the depth refinement (gdrnet_amd.refine.icp_refine_sil, include/gdrn_hip.h
"Silhouette term"): the observed contour, its distance transform by brute force, the rendered contour, the point-to-ray system and the loop
with the combined step.  Written from the header's text; the solve and the update are icp_host's.  The renders are an argument (a callable
for the loop), so the same code serves the device's renders and the host rasterizer's.

Like icp_host.accumulate, the accumulation also returns the sums of the absolute values of every sum's terms."""
import numpy as np

import icp_host as IH
import render_host as RH

INT32_MAX = 2 ** 31 - 1


def _shifted(a, fill):
    """the four in-frame 4-neighbours of every pixel of a [H,W]: (left, right, up, down), `fill` beyond the frame"""
    H, W = a.shape
    p = np.full((H + 2, W + 2), fill, dtype=a.dtype)
    p[1:-1, 1:-1] = a
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def observed_contour(mask, depth_scene=None):
    """[H,W] bool: mask pixels with an in-frame 4-neighbour outside the mask (the frame border is no edge); with ``depth_scene`` [H,W] fp32 (the
    instance's frame), without those where such a neighbour holds a nearer observed depth"""
    m = np.asarray(mask) != 0
    inside = _shifted(np.ones(m.shape, bool), False)
    nb_m = _shifted(m, True)
    out = np.zeros(m.shape, bool)
    occ = np.zeros(m.shape, bool)
    zs = None if depth_scene is None else np.asarray(depth_scene)
    if zs is not None:
        assert zs.dtype == np.float32 and zs.shape == m.shape
        nb_z = _shifted(zs, np.float32(0))
    for k in range(4):
        q_out = inside[k] & ~nb_m[k]
        out |= q_out
        if zs is not None:
            with np.errstate(invalid="ignore"):
                occ |= q_out & (nb_z[k] > 0) & (zs > 0) & (nb_z[k] < zs)
    return m & out & ~occ


def transform(contour):
    """(d2 [H,W] int32, nearest [H,W] int32) of a contour [H,W] bool by brute force over its pixels in ascending linear index"""
    H, W = contour.shape
    cy, cx = np.nonzero(contour)   # row-major: ascending cy * W + cx
    if len(cy) == 0:
        return np.full((H, W), INT32_MAX, np.int32), np.full((H, W), -1, np.int32)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    d = (cx[None, None, :] - x[:, :, None]) ** 2 + (cy[None, None, :] - y[:, :, None]) ** 2
    k = d.argmin(axis=2)           # the first of the minimisers
    return np.take_along_axis(d, k[:, :, None], axis=2)[:, :, 0].astype(np.int32), (cy[k] * W + cx[k]).astype(np.int32)


def contour_transform(mask, depth_scene):
    """dict(d2, nearest, contour (the count), edge [H,W] bool) of one instance"""
    edge = observed_contour(mask, depth_scene)
    d2, nearest = transform(edge)
    return dict(d2=d2, nearest=nearest, contour=int(edge.sum()), edge=edge)


def rendered_contour(depth_ren, depth_scene, dist_gate=0.02):
    """[H,W] bool: covered pixels of the render with an uncovered in-frame 4-neighbour that are not hidden behind a nearer observation"""
    zr_f, zs_f = np.asarray(depth_ren), np.asarray(depth_scene)
    assert zr_f.dtype == np.float32 and zs_f.dtype == np.float32 and zr_f.shape == zs_f.shape
    with np.errstate(invalid="ignore"):
        cov = zr_f > 0
        inside, nb = _shifted(np.ones(cov.shape, bool), False), _shifted(cov, True)
        edge = np.zeros(cov.shape, bool)
        for k in range(4):
            edge |= inside[k] & ~nb[k]
        zr, zs = zr_f.astype(np.float64), zs_f.astype(np.float64)
        hidden = (zs_f > 0) & (zs < zr - dist_gate)
    return cov & edge & ~hidden


def accumulate(depth_ren, depth_scene, K, d2, nearest, sil_gate=8.0, dist_gate=0.02):
    """One instance: depth_ren, depth_scene [H,W] fp32, K [3,3], d2 / nearest [H,W] int32 of its mask.  Returns dict(A [6,6], b [6], sq, pairs,
    A_abs, b_abs (the sums of the terms' absolute values; sq's terms are squares), mask [H,W] (the pair pixels), r [pairs,2])."""
    H, W = np.asarray(depth_ren).shape
    pair = rendered_contour(depth_ren, depth_scene, dist_gate) & (nearest >= 0) & (d2.astype(np.float64) <= sil_gate * sil_gate)
    A, b = np.zeros((6, 6)), np.zeros(6)
    if not pair.any():
        return dict(A=A, b=b, sq=0.0, pairs=0, A_abs=A.copy(), b_abs=b.copy(), mask=pair, r=np.zeros((0, 2)))
    dx, dy = (v.reshape(H, W) for v in RH.pixel_rays(np.asarray(K, dtype=np.float64), H, W))
    c = nearest[pair].astype(np.int64)
    z = np.asarray(depth_ren)[pair].astype(np.float64)
    ddx, ddy, gx, gy = dx[pair], dy[pair], dx.ravel()[c], dy.ravel()[c]
    P = np.stack([z * ddx, z * ddy, z], axis=1)
    one, zero = np.ones_like(z), np.zeros_like(z)
    cross = lambda p, n: np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],  # noqa: E731
                                   p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
    n1, n2 = np.stack([one, zero, -gx], axis=1), np.stack([zero, one, -gy], axis=1)
    J = np.stack([np.concatenate([cross(P, n1), n1], axis=1), np.concatenate([cross(P, n2), n2], axis=1)], axis=1)   # [pairs, 2, 6]
    r = np.stack([z * (ddx - gx), z * (ddy - gy)], axis=1)                                                            # [pairs, 2]
    JJ, Jr = J[:, :, :, None] * J[:, :, None, :], J * r[:, :, None]
    return dict(A=JJ.sum(axis=(0, 1)), b=Jr.sum(axis=(0, 1)), sq=float((r * r).sum()), pairs=int(pair.sum()), A_abs=np.abs(JJ).sum(axis=(0, 1)),
                b_abs=np.abs(Jr).sum(axis=(0, 1)), mask=pair, r=r)


def combine(dep, sil, weight=1.0):
    """(A, b, pairs) of the combined step: entry by entry depth + weight * silhouette, the pair counts added"""
    return dep["A"] + weight * sil["A"], dep["b"] + weight * sil["b"], dep["pairs"] + sil["pairs"]


def refine(render, R0, t0, K, depth_scene, mask, iters=20, sil_weight=1.0, sil_gate=8.0, dist_gate=0.02, normal_gate=0.01, min_pairs=64):
    """The loop for one instance: ``render(R, t)`` -> [H,W] fp32, depth_scene [H,W] its frame, mask [H,W] its observed mask.  Returns dict(R, t,
    ok, iters_done, pairs, rms, sil_pairs, sil_rms, trace): trace[k] = both systems and the solve of iteration k with the pose they were
    accumulated at."""
    R, t = np.array(R0, dtype=np.float64), np.array(t0, dtype=np.float64)
    out = dict(ok=1, iters_done=0, pairs=0, rms=np.nan, sil_pairs=0, sil_rms=np.nan, trace=[])
    if iters > 0:
        tr = contour_transform(mask, depth_scene)
    for _ in range(iters):
        ren = render(R, t)
        dep = IH.accumulate(ren, depth_scene, K, dist_gate, normal_gate)
        sil = accumulate(ren, depth_scene, K, tr["d2"], tr["nearest"], sil_gate, dist_gate)
        A, b, n = combine(dep, sil, sil_weight)
        sol = IH.solve(A, b, n, min_pairs)
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update(pairs=dep["pairs"], rms=float(np.sqrt(np.float64(dep["sq"]) / np.float64(dep["pairs"]))), sil_pairs=sil["pairs"],
                       sil_rms=float(np.sqrt(np.float64(sil["sq"]) / np.float64(sil["pairs"]))))
        out["trace"].append(dict(R=R.copy(), t=t.copy(), dep=dep, sil=sil, A=A, b=b, pairs=n, sol=sol))
        if not sol["ok"]:
            out["ok"] = 0
            break
        R, t, conv = IH.step(R, t, sol["xi"])
        out["iters_done"] += 1
        if conv:
            break
    out.update(R=R, t=t)
    return out


def lateral_errors(R, t, R_gt, t_gt):
    """(rotation error in degrees, lateral translation error in millimetres: the x and y components of t - t_gt)"""
    re, _ = IH.pose_errors(R, t, R_gt, t_gt)
    return re, float(1e3 * np.linalg.norm((np.asarray(t) - np.asarray(t_gt))[:2]))


def host_gt_depth(inp):
    """depth [G,H,W] fp32 of the ground truths of a synth.make_silhouette_inputs scene by the host rasterizer"""
    return np.stack([RH.render_one(inp["vertices"][int(c)], inp["faces"][int(c)], inp["R_gt"][g], inp["t_gt"][g], inp["K"][0], inp["H"], inp["W"],
                                   inp["near"], inp["far"]) for g, c in enumerate(inp["gt_labels"])])
