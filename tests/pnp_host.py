"""Independent fp64 numpy yardstick of the PnP tests: the pinhole projection, a plain Gauss-Newton on the reprojection cost and a brute-force
inlier test, written from the definition of the cost (sum over the points of |proj(K (R X + t)) - uv|^2, pixels) -- not from the kernels: the
rotation is updated on the RIGHT (R <- R exp([w]x)), the Jacobian comes from the chain rule on R X + t, the system is solved by numpy.  No scipy."""
import numpy as np


def project(K, R, t, X):
    """[n,2] pixel positions and [n] depths of the model points X [n,3]"""
    p = (X @ R.T + t) @ K.T
    return p[:, :2] / p[:, 2:3], p[:, 2]


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def expm_so3(w):
    th = np.linalg.norm(w)
    W = _skew(w)
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / th ** 2 * W @ W


def rotation_angle(Ra, Rb):
    """angle [rad] of Ra^T Rb, from the skew part and the trace (accurate near 0, where arccos of the trace is not)"""
    D = Ra.T @ Rb
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


def gauss_newton(K, X, uv, R0, t0, iters=50, tol=1e-13):
    """minimiser of the reprojection cost over the given points from the given start: (R, t, rms [px])"""
    R, t = R0.copy(), t0.copy()
    for _ in range(iters):
        Xc = X @ R.T + t
        p = Xc @ K.T
        proj = p[:, :2] / p[:, 2:3]
        r = (proj - uv).reshape(-1)
        # d proj / d Xc, rows (K_a - proj_a K_2) / p_2
        G = (K[None, :2, :] - proj[:, :, None] * K[None, 2:3, :]) / p[:, 2, None, None]          # [n,2,3]
        # R exp([w]x) X = R X + R (w x X) = R X - R [X]x w
        dXc_dw = np.stack([-R @ _skew(x) for x in X])                                             # [n,3,3]
        J = np.concatenate([G @ dXc_dw, G], axis=2).reshape(-1, 6)
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        R = R @ expm_so3(d[:3])
        t = t + d[3:]
        if max(np.linalg.norm(d[:3]), np.linalg.norm(d[3:]) / np.linalg.norm(t)) < tol:
            break
    uvp, _ = project(K, R, t, X)
    return R, t, float(np.sqrt(np.mean(np.sum((uvp - uv) ** 2, axis=1))))


def jacobian(K, R, t, X):
    """[2n,6] derivative of the stacked projections in (rotation vector applied on the right [rad], translation [m]) at (R, t)"""
    p = (X @ R.T + t) @ K.T
    proj = p[:, :2] / p[:, 2:3]
    G = (K[None, :2, :] - proj[:, :, None] * K[None, 2:3, :]) / p[:, 2, None, None]
    dXc_dw = np.stack([-R @ _skew(x) for x in X])
    return np.concatenate([G @ dXc_dw, G], axis=2).reshape(-1, 6)


def inliers(K, R, t, X, uv, thr):
    """brute force: in front of the camera and closer than thr pixels"""
    uvp, z = project(K, R, t, X)
    return (z > 0) & (np.sum((uvp - uv) ** 2, axis=1) < thr * thr)


def perturbed(R, t, deg=5.0, rel=0.05, k=0):
    """a start `deg` degrees and `rel` |t| away from (R, t), deterministic in k"""
    axis = np.array([[1.0, 2.0, -1.5], [-2.0, 0.5, 1.0], [0.3, -1.0, 2.0]])[k % 3]
    axis /= np.linalg.norm(axis)
    off = np.array([[0.6, -0.5, 0.62], [-0.4, 0.7, -0.59], [0.5, 0.5, 0.707]])[k % 3]
    return expm_so3(np.deg2rad(deg) * axis) @ R, t + rel * np.linalg.norm(t) * off / np.linalg.norm(off)
