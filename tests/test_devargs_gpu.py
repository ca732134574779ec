"""GPU tests of the argument forms the pose-geometry modules accept through gdrnet_amd.devargs: fp32 poses or the same values as fp64, K as one
[3,3] or its [N,3,3] expansion, labels / frames / counts as a list, a numpy int64 array, a CPU tensor or a device int32 tensor are the SAME call --
every output bit for bit (no tolerance: the forms differ on the host side only).  One test per module, at the smallest shapes that reach every
kernel of the entry point; what the entry points compute is pinned elsewhere (the modules' own GPU tests against their goldens)."""
import numpy as np
import pytest
import torch

from gdrnet_amd import bop_metrics as BM, pnp, pose_metrics as PM, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _index_forms(values):
    """the four forms of an index vector"""
    v = np.asarray(values, dtype=np.int64)
    return [v.tolist(), v, torch.from_numpy(v), torch.from_numpy(v).to(DEV).to(torch.int32)]


def _same_bits(a, b):
    """bit for bit, NaN payloads included (torch.equal on the raw bytes)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _all_same(results):
    """every result (a tensor, or a dict / tuple of tensors) equals the first one"""
    def flat(r):
        return [r[k] for k in sorted(r)] if isinstance(r, dict) else list(r) if isinstance(r, (tuple, list)) else [r]

    first = flat(results[0])
    return len(results) > 1 and all(len(flat(r)) == len(first) and all(_same_bits(x, y) for x, y in zip(flat(r), first)) for r in results[1:])


@pytest.fixture(scope="module")
def scene():
    """N = 3 poses whose values are fp32 numbers (so the fp32 and the fp64 form hold the same values), two point clouds of 5 and 7 points"""
    rng = np.random.default_rng(5)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    R_gt = f32([_rot(0.3, -0.2, 0.5), _rot(-0.4, 0.1, 1.2), _rot(0.05, 0.6, -0.7)])
    R_est = f32([_rot(0.32, -0.18, 0.52), _rot(-0.4, 0.1, 1.2 + np.pi), _rot(0.0, 0.65, -0.7)])
    t_gt = f32([[0.02, -0.01, 0.5], [-0.03, 0.02, 0.6], [0.0, 0.01, 0.45]])
    t_est = f32(t_gt + [[0.004, 0.0, -0.01], [0.0, 0.002, 0.005], [-0.003, 0.001, 0.0]])
    K = f32([[20.0, 0.0, 7.5], [0.0, 21.0, 8.25], [0.0, 0.0, 1.0]])   # a 16 x 16 frame
    points = [0.1 * rng.random((5, 3)) - 0.05, 0.1 * rng.random((7, 3)) - 0.05]
    return dict(R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K, points=points, diameters=[0.15, 0.17], labels=[0, 1, 1])


def _pose_forms(s, n=3):
    """(R_est, t_est, R_gt, t_gt, K) four ways: fp64 and fp32 with K [n,3,3], fp64 and fp32 with the one K [3,3]"""
    keys = ("R_est", "t_est", "R_gt", "t_gt")
    K_n = np.repeat(s["K"][None], n, axis=0)
    return [[_dev(s[k][:n], torch.float64) for k in keys] + [_dev(K_n, torch.float64)],
            [_dev(s[k][:n], torch.float32) for k in keys] + [_dev(K_n, torch.float32)],
            [_dev(s[k][:n], torch.float64) for k in keys] + [_dev(s["K"], torch.float64)],
            [_dev(s[k][:n], torch.float32) for k in keys] + [_dev(s["K"], torch.float32)]]


def test_pose_errors_argument_forms_are_one_call(scene):
    rz = np.diag([-1.0, -1.0, 1.0])
    table = PM.ModelTable(scene["points"], scene["diameters"], [None, rz[None]], sym_classes=(1,))
    poses = _pose_forms(scene)
    res = [PM.pose_errors(table, *p, scene["labels"])["err"] for p in poses]
    res += [PM.pose_errors(table, *poses[0], lab)["err"] for lab in _index_forms(scene["labels"])]
    assert res[0].shape == (3, 4) and bool(torch.isfinite(res[0]).all()) and bool((res[0][:, 0] > 0).all())
    assert _all_same(res)


def test_mssd_mspd_argument_forms_are_one_call(scene):
    syms = [None, (np.stack([np.eye(3), np.diag([-1.0, -1.0, 1.0])]), np.array([[0.0, 0.0, 0.0], [0.001, -0.002, 0.0]]))]
    table = BM.BopModelTable(scene["points"], scene["diameters"], syms)
    poses = _pose_forms(scene)
    res = [BM.mssd_mspd(table, *p, scene["labels"]) for p in poses]
    res += [BM.mssd_mspd(table, *poses[0], lab) for lab in _index_forms(scene["labels"])]
    assert res[0].shape == (3, 2) and bool(torch.isfinite(res[0]).all()) and bool((res[0] > 0).all())
    assert _all_same(res)


@pytest.fixture(scope="module")
def tetrahedron():
    # (12 px across at these poses: faces with a screen box above and below the rasterizer's 64-pixel switch between its two walks)
    verts = np.array([[0.15, 0.15, 0.15], [-0.15, -0.15, 0.15], [-0.15, 0.15, -0.15], [0.15, -0.15, -0.15]])
    return render.MeshTable([verts], [np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])])


def test_render_and_xyz_argument_forms_are_one_call(scene, tetrahedron):
    def call(p, labels):
        R, t, K = p[2], p[3], p[4]
        depth = render.render_depth(tetrahedron, labels, R, t, K, 16, 16)
        return dict(render.xyz_from_depth(depth, R, t, K), depth=depth)

    poses = _pose_forms(scene, n=2)
    res = [call(p, [0, 0]) for p in poses] + [call(poses[0], lab) for lab in _index_forms([0, 0])]
    assert res[0]["depth"].shape == (2, 16, 16) and bool((res[0]["visible"] == 1).all()) and 4 < int(res[0]["mask"].sum()) < 2 * 256
    assert _all_same(res)


def test_vsd_from_depth_argument_forms_are_one_call(scene, tetrahedron):
    p = _pose_forms(scene, n=2)
    d_est = render.render_depth(tetrahedron, [0, 0], p[0][0], p[0][1], p[0][4], 16, 16)
    d_gt = render.render_depth(tetrahedron, [0, 0], p[0][2], p[0][3], p[0][4], 16, 16)
    d_test = torch.where(d_gt[:1] > 0, d_gt[:1] + 0.002, torch.full_like(d_gt[:1], 0.9))   # F = 1

    def call(K, frame):
        return BM.vsd_from_depth(d_est, d_gt, d_test, frame, K, [0.15, 0.15], 0.015, taus=[0.05, 0.3], cost_type="tlinear", return_counts=True)

    res = [call(q[4], [0, 0]) for q in p] + [call(p[0][4], fr) for fr in _index_forms([0, 0])]
    err, counts = res[0]
    assert err.shape == (2, 2) and counts.shape == (2, 4) and bool((counts[:, 0] > 0).all()) and bool(torch.isfinite(err).all())
    assert _all_same(res)


def test_pnp_argument_forms_are_one_call(scene):
    rng = np.random.default_rng(11)
    N, S, K = 2, 8, synth.LM_K.astype(np.float64)   # (fp32 values)
    X = 0.1 * rng.random((N, S, 3)) - 0.05
    R, t = scene["R_gt"][:N].astype(np.float64), scene["t_gt"][:N].astype(np.float64)
    cam = (X @ R.transpose(0, 2, 1) + t[:, None]) @ K.T
    img, mod = _dev(cam[..., :2] / cam[..., 2:3], torch.float32), _dev(X, torch.float32)
    K_forms = [_dev(np.repeat(K[None], N, axis=0), torch.float64), _dev(np.repeat(K[None], N, axis=0), torch.float32), _dev(K, torch.float64),
               _dev(K, torch.float32)]
    counts = _index_forms([8, 5])
    ransac = [pnp.pnp_ransac(img, mod, counts[0], k, iters=4, seed=3, want_mask=True) for k in K_forms]
    ransac += [pnp.pnp_ransac(img, mod, c, K_forms[0], iters=4, seed=3, want_mask=True) for c in counts]
    assert bool(ransac[0]["ok"].any()) and ransac[0]["inlier_mask"].shape == (N, S)
    assert _all_same(ransac)
    R0, t0 = np.asarray([_rot(0.32, -0.18, 0.52), _rot(-0.38, 0.12, 1.18)], dtype=np.float32), scene["t_est"][:N]   # fp32 values near the truth
    refine = [pnp.pnp_refine(img, mod, counts[0], k, _dev(R0, dt), _dev(t0, dt)) for k in K_forms for dt in (torch.float64, torch.float32)]
    refine += [pnp.pnp_refine(img, mod, c, K_forms[0], _dev(R0, torch.float64), _dev(t0, torch.float64)) for c in counts]
    assert bool(refine[0]["ok"].all()) and refine[0]["R"].dtype == torch.float64
    assert _all_same(refine)
