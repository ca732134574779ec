"""GPU tests (-m gpu) of the pose from depth and object-coordinate maps (gdrnet_amd.rigid, csrc/rigid.hip) against known poses and the independent
fp64 host restatement tests/rigid_host.py.  The reference is RGB-only and has no counterpart: the feature is pinned to geometry.

Fixture: rigid_host.make_rigid_inputs -- 8 RoIs in one call (0, 2, 3, 5 collinear, 257, 513, 4096 and 600 coplanar pairs in rows of 4096, NaN padding,
40 % outliers 30 .. 120 mm off on the RoIs with >= 257 pairs), gate 10 mm, 100 hypotheses, seed 0: 9 mm of margin on the inlier side and 20 mm on
the outlier side, so the recovered inlier set is the true one whatever the last bits of the solver.

Bounds (deviation = max(rotation angle [rad], |dt| / |t|)).  Noise-free: 1e-10 against the ground truth -- a closed form in fp64 whose host
restatement is off by 5.5e-15 at worst, while one fp32 step anywhere gives at least 1e-8.  Bounded noise (inliers within a 1 mm ball): 1e-10
against rigid_host.kabsch on the true inlier set -- the same closed-form minimum, no iteration tolerance involved; rms to 1e-9 relative.  From a
render: 1e-5 -- fp32 depth at up to 2 m is off by at most 1.2e-7 m, a coherent worst case on a 5 cm radius is 2.4e-6 rad, the bound four times that."""
import numpy as np
import pytest
import torch

import rigid_host as H
from gdrnet_amd import refine, render, rigid, synth
from gdrnet_amd.cfg import lm13_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK = [0, 0, 1, 0, 1, 1, 1, 1]
SOLVED = (2, 4, 5, 6, 7)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _start(N):
    """the R0 / t0 handed in: recognisable values the unsolved RoIs must hand back bit for bit"""
    R0 = torch.eye(3, dtype=torch.float64).repeat(N, 1, 1) * 0.5 + 0.125
    t0 = torch.arange(3 * N, dtype=torch.float64).reshape(N, 3) + 0.25
    return R0.to(DEV), t0.to(DEV)


def _run(dev, **kw):
    R0, t0 = _start(8)
    args = dict(dist_thr=H.DIST_THR, iters=H.ITERS, seed=H.SEED, R0=R0, t0=t0, want_mask=True)
    args.update(kw)
    return _np(rigid.rigid_ransac(dev["cam_points"], dev["model_points"], dev["counts"], **args))


def _bits_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


@pytest.fixture(scope="module")
def clean():
    inp = H.make_rigid_inputs("clean")
    dev = {k: _dev(inp[k]) for k in ("cam_points", "model_points", "counts")}
    return inp, dev, _run(dev)


@pytest.fixture(scope="module")
def noisy():
    inp = H.make_rigid_inputs("noisy")
    dev = {k: _dev(inp[k]) for k in ("cam_points", "model_points", "counts")}
    ref = {}
    for n in SOLVED:   # the host yardstick, once: the closed form on the true inlier set
        m = inp["inlier"][n]
        ref[n] = H.fit(inp["cam_points"][n][m], inp["model_points"][n][m])
    return inp, dev, _run(dev), ref


def _check_unsolved(out, rows):
    R0, t0 = (x.cpu().numpy() for x in _start(8))
    for n in rows:   # the caller's values, bit for bit
        assert np.array_equal(out["R"][n], R0[n]) and np.array_equal(out["t"][n], t0[n]), n
        assert out["num_inliers"][n] == 0 and not out["inlier_mask"][n].any() and np.isnan(out["rms"][n]), n


def _check_clean(inp, out, bound=1e-10, rows=SOLVED):
    worst = 0.0
    for n in rows:
        assert out["ok"][n] == 1, n
        worst = max(worst, H.deviation(out["R"][n], out["t"][n], inp["R"][n], inp["t"][n]))
        assert np.array_equal(out["inlier_mask"][n].astype(bool), inp["inlier"][n]), n
        assert abs(np.linalg.det(out["R"][n]) - 1.0) < 1e-12
    print(f"worst deviation from the ground truth: {worst:.3e} (bound {bound:.0e}); worst rms {np.nanmax(out['rms']):.3e} m")
    assert np.array_equal(out["num_inliers"], out["inlier_mask"].sum(axis=1))
    assert worst <= bound
    return worst


def test_noise_free_recovery(clean):
    """bound 1e-10 against the ground truth; measured on an MI355X: 5.6e-16 (worst rms 2.6e-16 m)"""
    inp, _, out = clean
    assert list(out["ok"]) == OK, out["ok"]
    _check_unsolved(out, (0, 1, 3))
    _check_clean(inp, out)
    assert np.nanmax(out["rms"]) < 1e-12 and np.isfinite(out["R"]).all() and np.isfinite(out["t"]).all()


def test_bounded_noise_matches_the_host_closed_form(noisy):
    """bounds 1e-10 against rigid_host.kabsch on the true inlier set and 1e-9 relative on rms; measured on an MI355X: 5.5e-15 and 1.8e-15"""
    inp, _, out, ref = noisy
    assert list(out["ok"]) == OK, out["ok"]
    _check_unsolved(out, (0, 1, 3))
    worst = worst_rms = 0.0
    for n in SOLVED:
        ok, R_ref, t_ref, rms_ref = ref[n]
        assert ok == 1
        worst = max(worst, H.deviation(out["R"][n], out["t"][n], R_ref, t_ref))
        worst_rms = max(worst_rms, abs(out["rms"][n] - rms_ref) / rms_ref)
        assert np.array_equal(out["inlier_mask"][n].astype(bool), inp["inlier"][n]), n
    print(f"worst deviation from the host closed form: {worst:.3e} (bound 1e-10); worst relative rms difference {worst_rms:.3e} (bound 1e-9)")
    assert np.array_equal(out["num_inliers"], out["inlier_mask"].sum(axis=1))
    assert worst <= 1e-10 and worst_rms <= 1e-9


def test_rigid_fit_matches_the_host(noisy):
    """rigid_fit over all rows of the true-inlier subsets (the outlier-free RoIs whole): 1e-10 against the host, rms 1e-9 relative"""
    inp, _, _, _ = noisy
    cam, mod = np.full_like(inp["cam_points"], np.nan), np.full_like(inp["model_points"], np.nan)
    counts = inp["inlier"].sum(axis=1).astype(np.int32)
    for n in range(8):
        cam[n, : counts[n]], mod[n, : counts[n]] = inp["cam_points"][n][inp["inlier"][n]], inp["model_points"][n][inp["inlier"][n]]
    assert list(counts[:4]) == [0, 2, 3, 5] and counts[4] < 257 and counts[6] < 4096
    R0, t0 = _start(8)
    out = _np(rigid.rigid_fit(_dev(cam), _dev(mod), _dev(counts), R0, t0))
    assert list(out["ok"]) == OK, out["ok"]
    for n in (0, 1, 3):   # empty, below the minimum, collinear
        assert np.array_equal(out["R"][n], R0[n].cpu().numpy()) and np.array_equal(out["t"][n], t0[n].cpu().numpy()) and np.isnan(out["rms"][n])
    worst = worst_rms = 0.0
    for n in SOLVED:
        ok, R_ref, t_ref, rms_ref = H.fit(cam[n, : counts[n]], mod[n, : counts[n]])
        assert ok == 1
        worst = max(worst, H.deviation(out["R"][n], out["t"][n], R_ref, t_ref))
        worst_rms = max(worst_rms, abs(out["rms"][n] - rms_ref) / rms_ref)
    print(f"rigid_fit against the host closed form: {worst:.3e} (bound 1e-10); relative rms difference {worst_rms:.3e} (bound 1e-9)")
    assert worst <= 1e-10 and worst_rms <= 1e-9


def test_chunk_edges_and_determinism(clean, noisy):
    inp, dev, out0, _ = noisy
    out = _run(dev, iters=257)   # a second chunk of one hypothesis, against the host restatement of the whole loop
    assert list(out["ok"]) == OK
    worst = 0.0
    for n, c in enumerate(inp["counts"]):
        r = H.ransac(inp["cam_points"][n, :c], inp["model_points"][n, :c], H.DIST_THR, 257, H.SEED, n)
        assert r["ok"] == out["ok"][n] and np.array_equal(out["inlier_mask"][n, :c].astype(bool), r["mask"]) and not out["inlier_mask"][n, c:].any()
        if r["ok"]:
            worst = max(worst, H.deviation(out["R"][n], out["t"][n], r["R"], r["t"]))
    print(f"iters = 257 against the host RANSAC: {worst:.3e} (bound 1e-10)")
    assert worst <= 1e-10
    cinp, cdev, _ = clean
    one = _run(cdev, iters=1)   # one hypothesis: may miss on the outlier RoIs, not on the minimal one
    assert one["ok"][2] == 1 and list(one["ok"][[0, 1, 3]]) == [0, 0, 0]
    assert H.deviation(one["R"][2], one["t"][2], cinp["R"][2], cinp["t"][2]) <= 1e-10
    assert _bits_equal(out0, _run(dev))   # the same call: the same bits in every output
    pad = {k: v.clone() for k, v in dev.items()}
    for k in ("cam_points", "model_points"):   # what lies behind counts[n] is never read into a result
        pad[k] = torch.where(torch.isnan(pad[k]), torch.full_like(pad[k], 1e30), pad[k])
    assert not torch.isnan(pad["cam_points"]).any()
    assert _bits_equal(out0, _run(pad))
    R0, t0 = _start(8)
    fit0 = _np(rigid.rigid_fit(dev["cam_points"], dev["model_points"], dev["counts"], R0, t0))
    assert _bits_equal(fit0, _np(rigid.rigid_fit(pad["cam_points"], pad["model_points"], pad["counts"], R0, t0)))


def test_backproject_against_the_host():
    """2 frames of 48 x 64 (H != W), 4 RoIs of 300 rows (more than one 256-row pass): counts_out and the order of the surviving rows equal the
    host's exactly, camera points to 1e-12 relative (the inverse of K may differ in its last bits), NaN padding, model points widened exactly"""
    Hh, W, S, N = 48, 64, 300, 4
    u = lambda tag, *shape: synth.hash_uniform(51, tag, shape)  # noqa: E731
    depth = (0.3 + 1.7 * u("depth", 2, Hh, W)).astype(np.float32)
    depth[u("holes", 2, Hh, W) < 0.2] = 0.0
    depth[0, 5, 7], depth[0, 6, 7], depth[1, 40, 60] = np.nan, -0.5, np.inf
    depth[0, 0, 0], depth[0, Hh - 1, W - 1], depth[0, 0, W - 1], depth[0, Hh - 1, 0] = 0.9, 1.1, 1.2, 1.3
    img = np.stack([-2.0 + (W + 4.0) * u("u", N, S), -2.0 + (Hh + 4.0) * u("v", N, S)], axis=2).astype(np.float32)
    edge = [(-0.5, 3.0), (W - 0.5, 3.0), (3.0, -0.5), (3.0, Hh - 0.5), (-0.5, -0.5), (W - 0.5, Hh - 0.5),   # exact .5 boundaries
            (W - 0.5 - 2.0 ** -17, Hh - 0.5 - 2.0 ** -18), (-0.5 - 2.0 ** -24, 3.0),                         # ... and one fp32 step inside / outside
            (-1.0, 5.0), (float(W), 5.0), (5.0, -1.0), (5.0, float(Hh)),                                      # one pixel outside each border
            (7.0, 5.0), (7.0, 6.0), (7.25, 4.75), (np.nan, 5.0), (5.0, np.nan), (0.0, 0.0), (W - 1.0, Hh - 1.0), (W - 1.0, 0.0), (0.0, Hh - 1.0)]
    img[0, 10 : 10 + len(edge)] = np.array(edge, dtype=np.float32)
    img[0, 270 : 270 + len(edge)] = np.array(edge, dtype=np.float32)   # the same rows in the second pass
    mod = (0.1 * u("X", N, S, 3) - 0.05).astype(np.float32)
    mod[0, 40, 1], mod[1, 3, 2] = np.nan, np.inf
    counts = np.array([S, 130, 0, S], dtype=np.int32)
    frame = np.array([0, 1, 1, 0], dtype=np.int32)
    K = np.repeat(np.array([[70.0, 0.3, 31.5], [0.0, 65.0, 23.0], [0.0, 0.0, 1.0]])[None], N, axis=0)
    K[1, 0, 0], K[1, 1, 2] = 80.0, 25.5
    K[3, 2] = 0.0   # singular: every row of RoI 3 is invalid
    out = _np(rigid.backproject(_dev(img), _dev(mod), _dev(counts), _dev(depth), frame, _dev(K)))
    worst = 0.0
    for n in range(N):
        cam_h, mod_h, k = H.backproject(img[n], mod[n], counts[n], depth[frame[n]], K[n])
        assert out["counts"][n] == k, (n, out["counts"][n], k)
        assert np.array_equal(out["model_points"][n], mod_h, equal_nan=True), n   # the survivors, in order, widened exactly; NaN behind them
        assert np.isnan(out["cam_points"][n, k:]).all() and np.isfinite(out["cam_points"][n, :k]).all()
        if k:
            worst = max(worst, float((np.abs(out["cam_points"][n, :k] - cam_h[:k]) / np.abs(cam_h[:k]).max(axis=1, keepdims=True)).max()))
            assert np.array_equal(out["cam_points"][n, :k, 2], cam_h[:k, 2])   # z is the depth itself
    print(f"camera points against the host: {worst:.3e} relative (bound 1e-12); counts_out {out['counts']}")
    assert 100 < out["counts"][0] < S and 40 < out["counts"][1] < 130 and out["counts"][2] == 0 and out["counts"][3] == 0
    assert worst <= 1e-12
    with pytest.raises(ValueError):
        rigid.backproject(_dev(img), _dev(mod), _dev(counts), _dev(depth), [0, 1, 2, 0], _dev(K))


FX, IM_H, IM_W = 160.0, 96, 128


@pytest.fixture(scope="module")
def scene():
    """a 0.1 m cube and a perturbed icosphere at 0.5 .. 0.8 m, each in its own 96 x 128 frame; a third, empty frame.  A band of each frame is
    overwritten by an occluding plane 6 cm in front of the object's nearest point, a block of the object's pixels is set to 0."""
    meshes = render.MeshTable([synth.mesh_cube(0.1)[0], synth.mesh_icosphere(2, 0.05, 0.3, 3)[0]],
                              [synth.mesh_cube(0.1)[1], synth.mesh_icosphere(2, 0.05, 0.3, 3)[1]], device=DEV)
    labels = np.array([0, 1])
    R = synth._random_rotations(61, "R", 2)
    t = np.array([[0.03, -0.02, 0.5], [-0.05, 0.03, 0.8]])
    K = np.array([[FX, 0.0, 64.0], [0.0, FX, 48.0], [0.0, 0.0, 1.0]])
    Rd, td, Kd = _dev(R), _dev(t), _dev(K)
    depth = render.render_depth(meshes, labels, Rd, td, Kd, IM_H, IM_W)
    xyz = render.xyz_from_depth(depth, Rd, td, Kd)
    dn, xn, mn = depth.cpu().numpy(), xyz["xyz"].cpu().numpy(), xyz["mask"].cpu().numpy().astype(bool)
    obs = np.zeros((3, IM_H, IM_W), dtype=np.float32)
    obs[:2] = dn
    band, block = np.zeros((2, IM_H, IM_W), dtype=bool), np.zeros((2, IM_H, IM_W), dtype=bool)
    for n in range(2):
        ys, xs = np.nonzero(mn[n])
        x0, x1, y0, y1 = xs.min(), xs.max() + 1, ys.min(), ys.max() + 1
        w, h = x1 - x0, y1 - y0
        band[n, :, x0 + w // 5 : x0 + 2 * w // 5] = True
        block[n, y0 + h // 2 : y0 + h // 2 + h // 6, x0 + 3 * w // 5 : x0 + 4 * w // 5] = True
        obs[n][band[n]] = dn[n][mn[n]].min() - 0.06
        obs[n][block[n]] = 0.0
    return dict(meshes=meshes, labels=labels, R=R, t=t, K=K, depth=dn, xyz=xn, mask=mn, obs=obs, band=band, block=block)


def test_pose_from_a_render(scene):
    """rendered depth + xyz_from_depth object coordinates, an occluder and a hole: counts_out = covered - hole, inliers = the unoccluded pixels,
    deviation <= 1e-5 from the ground truth; measured on an MI355X: 2.2e-9 (rms 1.5e-9 m); through the maps of poses_from_maps_rgbd 1.4e-8"""
    s, S = scene, 4096
    img, mod = np.full((2, S, 2), np.nan, dtype=np.float32), np.full((2, S, 3), np.nan, dtype=np.float32)
    counts, truth, kept = np.zeros(2, dtype=np.int32), [], []
    for n in range(2):
        ys, xs = np.nonzero(s["mask"][n])   # row-major
        c = len(ys)
        assert 200 < c <= S
        img[n, :c, 0], img[n, :c, 1], mod[n, :c], counts[n] = xs, ys, s["xyz"][n, ys, xs], c
        keep = ~s["block"][n, ys, xs]
        kept.append(keep)
        truth.append(~s["band"][n, ys, xs][keep])
        assert 0 < (~keep).sum() and 0 < (~truth[n]).sum() < truth[n].sum()
    pts = rigid.backproject(_dev(img), _dev(mod), _dev(counts), _dev(s["obs"]), [0, 1], _dev(s["K"]))
    out = _np(rigid.rigid_ransac(pts["cam_points"], pts["model_points"], pts["counts"], want_mask=True))
    cnt = pts["counts"].cpu().numpy()
    worst = 0.0
    for n in range(2):
        assert cnt[n] == kept[n].sum(), (n, cnt[n], kept[n].sum(), counts[n])
        assert np.array_equal(pts["model_points"][n, : cnt[n]].cpu().numpy(), mod[n, : counts[n]][kept[n]].astype(np.float64))
        assert out["ok"][n] == 1 and np.array_equal(out["inlier_mask"][n, : cnt[n]].astype(bool), truth[n]) and out["num_inliers"][n] == truth[n].sum(), n
        worst = max(worst, H.deviation(out["R"][n], out["t"][n], s["R"][n], s["t"][n]))
    print(f"pose from a render: deviation {worst:.3e} (bound 1e-5); rms {out['rms']} m; inliers {out['num_inliers']} of {cnt}")
    assert worst <= 1e-5


def test_poses_from_maps_rgbd(scene):
    """maps in the head's normalisation cut from the render as 64 x 64 RoIs, the ground truth perturbed by 10 degrees / 3 cm as the network's pose:
    the solved RoIs within the bound of the render test, the RoI whose frame holds no depth hands the network's pose back bit for bit, ok = 0;
    refine.icp_refine takes the result as it is"""
    s, N, M = scene, 3, 64
    src = [0, 1, 0]   # RoI 2: the cube again, looked up in the empty frame
    frame = np.array([0, 1, 2])
    ext = np.array([[0.1, 0.1, 0.1], [0.13, 0.13, 0.13], [0.1, 0.1, 0.1]], dtype=np.float32)
    mask, coor, c2d = np.zeros((N, 1, M, M), dtype=np.float32), np.full((3, N, 1, M, M), 0.5, dtype=np.float32), np.zeros((N, 2, M, M), dtype=np.float32)
    for n in range(N):
        ys, xs = np.nonzero(s["mask"][src[n]])
        x0 = int(np.clip((xs.min() + xs.max()) // 2 - M // 2, 0, IM_W - M))
        y0 = int(np.clip((ys.min() + ys.max()) // 2 - M // 2, 0, IM_H - M))
        assert xs.min() >= x0 and xs.max() < x0 + M and ys.min() >= y0 and ys.max() < y0 + M   # the object lies inside its RoI
        mask[n, 0] = s["mask"][src[n], y0 : y0 + M, x0 : x0 + M]
        for a in range(3):
            coor[a][n, 0] = s["xyz"][src[n], y0 : y0 + M, x0 : x0 + M, a] / ext[n, a] + np.float32(0.5)
        c2d[n, 0] = (np.arange(x0, x0 + M, dtype=np.float32) / np.float32(IM_W))[None, :]
        c2d[n, 1] = (np.arange(y0, y0 + M, dtype=np.float32) / np.float32(IM_H))[:, None]
    assert np.abs(s["xyz"][0]).max() < 0.05 * 1.0001 and np.abs(s["xyz"][1]).max() < 0.065
    R_gt, t_gt = s["R"][src], s["t"][src]
    ang = np.deg2rad(10.0)
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    R_net = (Rz @ R_gt).astype(np.float32)
    t_net = (t_gt + np.array([0.02, -0.01, 0.02])).astype(np.float32)   # 3 cm
    out_dict = dict(mask=_dev(mask), coor_x=_dev(coor[0]), coor_y=_dev(coor[1]), coor_z=_dev(coor[2]), rot=_dev(R_net), trans=_dev(t_net))
    K, obs = _dev(s["K"]), _dev(s["obs"])
    res = rigid.poses_from_maps_rgbd(lm13_cfg(), out_dict, _dev(c2d), _dev(ext), [IM_H] * N, [IM_W] * N, K, obs, frame)
    pose, ok = res["pose_est"].cpu().numpy(), res["ok"].cpu().numpy()
    assert pose.shape == (N, 3, 4) and pose.dtype == np.float64 and list(ok) == [1, 1, 0]
    assert np.array_equal(pose[2, :, :3], R_net[2].astype(np.float64)) and np.array_equal(pose[2, :, 3], t_net[2].astype(np.float64))
    assert res["num_inliers"][2] == 0 and torch.isnan(res["rms"][2])
    worst = max(H.deviation(pose[n, :, :3], pose[n, :, 3], R_gt[n], t_gt[n]) for n in (0, 1))
    print(f"poses_from_maps_rgbd: deviation {worst:.3e} (bound 1e-5); inliers {res['num_inliers'].cpu().numpy()}, rms {res['rms'].cpu().numpy()}")
    assert worst <= 1e-5
    icp = refine.icp_refine(s["meshes"], s["labels"], res["pose_est"][:2, :, :3], res["pose_est"][:2, :, 3], K, obs, frame[:2], iters=2)
    assert icp["R"].shape == (2, 3, 3) and bool(torch.isfinite(icp["t"]).all())
