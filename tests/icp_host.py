"""Plain numpy fp64 restatement of the depth refinement (gdrnet_amd.refine, include/gdrn_hip.h "Depth refinement"): the accumulation of the
point-to-plane normal equations, the solve-and-update step and the loop.  Written from the header's text, vectorised over the pixels of a frame;
the renders are an argument (a callable for the loop), so the same code serves the device's renders and the host rasterizer's.

Besides the sums it returns the sum of the absolute values of every sum's terms (the scale of the rounding error of a sum in any order) and the
2-norm condition number of the Jacobi-scaled matrix (the amplification of that error by the solve)."""
import numpy as np

import render_host as RH

PIVOT_MIN, STEP_TOL, SMALL_ANGLE = 1e-9, 1e-10, 1e-12


def accumulate(depth_ren, depth_scene, K, dist_gate=0.02, normal_gate=0.01, flip_normals=False):
    """One instance: depth_ren, depth_scene [H,W] fp32 (the instance's render and ITS frame), K [3,3].  Returns dict(A [6,6], b [6], sq, pairs,
    A_abs, b_abs, sq_abs (the sums of the terms' absolute values; sq's terms are squares), mask [H,W] (the pairs), n [pairs,3], r [pairs])."""
    zr_f, zs_f = np.asarray(depth_ren), np.asarray(depth_scene)
    assert zr_f.dtype == np.float32 and zs_f.dtype == np.float32 and zr_f.shape == zs_f.shape
    H, W = zr_f.shape
    zr, zs = zr_f.astype(np.float64), zs_f.astype(np.float64)
    dx, dy = (v.reshape(H, W) for v in RH.pixel_rays(np.asarray(K, dtype=np.float64), H, W))
    A, b = np.zeros((6, 6)), np.zeros(6)
    empty = dict(A=A, b=b, sq=0.0, pairs=0, A_abs=A.copy(), b_abs=b.copy(), sq_abs=0.0, mask=np.zeros((H, W), bool), n=np.zeros((0, 3)), r=np.zeros(0))
    if H < 3 or W < 3:
        return empty
    c = (slice(1, H - 1), slice(1, W - 1))                       # the pixels that are not on the border
    lf, rt = (slice(1, H - 1), slice(0, W - 2)), (slice(1, H - 1), slice(2, W))
    up, dn = (slice(0, H - 2), slice(1, W - 1)), (slice(2, H), slice(1, W - 1))
    with np.errstate(invalid="ignore"):
        ok = (zr[c] > 0) & (zs[c] > 0)
        for nb in (lf, rt, up, dn):
            ok &= (zs[nb] > 0) & (np.abs(zs[nb] - zs[c]) <= normal_gate)
        ok &= np.abs(zs[c] - zr[c]) <= dist_gate
        q = lambda s: (zs[s] * dx[s], zs[s] * dy[s], zs[s])  # noqa: E731
        (rx, ry, rz), (lx, ly, lz), (wx, wy, wz), (ux, uy, uz) = q(rt), q(lf), q(dn), q(up)
        a = (rx - lx, ry - ly, rz - lz)
        bb = (wx - ux, wy - uy, wz - uz)
        cr = (a[1] * bb[2] - a[2] * bb[1], a[2] * bb[0] - a[0] * bb[2], a[0] * bb[1] - a[1] * bb[0])
        ln = np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
        ok &= ln > 0
    mask = np.zeros((H, W), bool)
    mask[c] = ok
    if not ok.any():
        return empty
    ln = ln[ok]
    n = np.stack([cr[0][ok] / ln, cr[1][ok] / ln, cr[2][ok] / ln], axis=1)
    if flip_normals:
        n = -n
    ddx, ddy, z_r, z_s = dx[c][ok], dy[c][ok], zr[c][ok], zs[c][ok]
    r = (z_r - z_s) * ((n[:, 0] * ddx + n[:, 1] * ddy) + n[:, 2])     # n . (p - q), p - q = (depth_ren - depth_scene) d
    p = np.stack([z_r * ddx, z_r * ddy, z_r], axis=1)
    pn = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
    J = np.concatenate([pn, n], axis=1)
    JJ, Jr = J[:, :, None] * J[:, None, :], J * r[:, None]
    return dict(A=JJ.sum(axis=0), b=Jr.sum(axis=0), sq=float((r * r).sum()), pairs=int(ok.sum()), A_abs=np.abs(JJ).sum(axis=0),
                b_abs=np.abs(Jr).sum(axis=0), sq_abs=float((r * r).sum()), mask=mask, n=n, r=r)


def scaled(A):
    """(S A S, S) with S = diag(A_ii^-1/2); None where a diagonal entry is not > 0"""
    d = np.diag(A)
    if not np.all(d > 0):
        return None, None
    s = 1.0 / np.sqrt(d)
    return A * s[:, None] * s[None, :], s


def pivots(M):
    """the pivots of the Cholesky factorisation of M (the remainder of each diagonal entry before its square root), stopping at the first
    one that is not positive"""
    L, out = np.zeros((6, 6)), []
    for r in range(6):
        for c in range(r + 1):
            v = M[r, c] - L[r, :c] @ L[c, :c]
            if r == c:
                out.append(v)
                if not v > 0:
                    return np.array(out)
                L[r, r] = np.sqrt(v)
            else:
                L[r, c] = v / L[c, c]
    return np.array(out)


def solve(A, b, pairs, min_pairs=64):
    """dict(ok, xi [6] (zeros when degenerate), cond (2-norm condition number of S A S, inf when degenerate), min_pivot)"""
    bad = dict(ok=False, xi=np.zeros(6), cond=np.inf, min_pivot=0.0)
    if pairs < min_pairs:
        return bad
    M, s = scaled(A)
    if M is None:
        return bad
    pv = pivots(M)
    if len(pv) < 6 or not np.all(pv >= PIVOT_MIN):
        return dict(bad, min_pivot=float(pv.min()))
    xi = s * np.linalg.solve(M, -(s * b))
    if not np.all(np.isfinite(xi)):
        return bad
    return dict(ok=True, xi=xi, cond=float(np.linalg.cond(M, 2)), min_pivot=float(pv.min()))


def exp_so3(w):
    th = float(np.linalg.norm(w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < SMALL_ANGLE:
        return np.eye(3) + Wx
    return np.eye(3) + (np.sin(th) / th) * Wx + (2.0 * np.sin(0.5 * th) ** 2 / (th * th)) * (Wx @ Wx)


def log_so3(E):
    """the rotation vector of a rotation matrix close to the identity (angles well below pi)"""
    v = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])   # sin(th) axis
    s = float(np.linalg.norm(v))
    if s < 1e-8:
        return v * (1.0 + s * s / 6.0)
    return v * (np.arcsin(min(s, 1.0)) / s)


def step(R, t, xi):
    """(R', t', converged) of an accepted step"""
    E = exp_so3(xi[:3])
    conv = np.linalg.norm(xi[:3]) < STEP_TOL and np.linalg.norm(xi[3:]) < STEP_TOL * np.linalg.norm(t)
    return E @ R, E @ t + xi[3:], bool(conv)


def refine(render, R0, t0, K, depth_scene, iters=10, dist_gate=0.02, normal_gate=0.01, min_pairs=64):
    """The loop for one instance: ``render(R, t)`` -> [H,W] fp32, depth_scene [H,W] its frame.  Returns dict(R, t, ok, iters_done, pairs, rms,
    trace): trace[k] = the system and the solve of iteration k with the pose it was accumulated at."""
    R, t = np.array(R0, dtype=np.float64), np.array(t0, dtype=np.float64)
    out = dict(ok=1, iters_done=0, pairs=0, rms=np.nan, trace=[])
    for _ in range(iters):
        acc = accumulate(render(R, t), depth_scene, K, dist_gate, normal_gate)
        sol = solve(acc["A"], acc["b"], acc["pairs"], min_pairs)
        out["pairs"] = acc["pairs"]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["rms"] = float(np.sqrt(np.float64(acc["sq"]) / np.float64(acc["pairs"])))
        out["trace"].append(dict(R=R.copy(), t=t.copy(), acc=acc, sol=sol))
        if not sol["ok"]:
            out["ok"] = 0
            break
        R, t, conv = step(R, t, sol["xi"])
        out["iters_done"] += 1
        if conv:
            break
    out.update(R=R, t=t)
    return out


def pose_errors(R, t, R_gt, t_gt):
    """(rotation error in degrees, translation error in millimetres)"""
    c = 0.5 * (np.trace(R @ R_gt.T) - 1.0)
    s = 0.5 * np.linalg.norm(np.array([(R @ R_gt.T)[2, 1] - (R @ R_gt.T)[1, 2], (R @ R_gt.T)[0, 2] - (R @ R_gt.T)[2, 0], (R @ R_gt.T)[1, 0] - (R @ R_gt.T)[0, 1]]))
    return float(np.degrees(np.arctan2(s, c))), float(1e3 * np.linalg.norm(np.asarray(t) - np.asarray(t_gt)))


def host_renderer(inp, row):
    """render(R, t) of row `row` of a synth.make_refine_inputs scene by the host rasterizer"""
    c = int(inp["labels"][row])
    return lambda R, t: RH.render_one(inp["vertices"][c], inp["faces"][c], R, t, inp["K"][row], inp["H"], inp["W"], inp["near"], inp["far"])


def host_gt_depth(inp):
    """depth [G,H,W] fp32 of the ground truths of a synth.make_refine_inputs scene by the host rasterizer"""
    K_of = {int(g): inp["K"][i] for i, g in enumerate(inp["target"])}
    return np.stack([RH.render_one(inp["vertices"][int(c)], inp["faces"][int(c)], inp["R_gt"][g], inp["t_gt"][g], K_of.get(g, inp["K"][0]),
                                   inp["H"], inp["W"], inp["near"], inp["far"]) for g, c in enumerate(inp["gt_labels"])])
