"""CPU tests (-m "not gpu") of gdrnet_amd.rigid: the host restatement the GPU tests are judged by (tests/rigid_host.py) recovers the fixture's poses
and inlier sets, its draw rule and degeneracy rule hold on hand-made cases, the wrappers refuse bad calls before anything is loaded or launched,
and there is no CPU fallback."""
import numpy as np
import pytest
import torch

import rigid_host as H
from gdrnet_amd import cabi, rigid
from gdrnet_amd.cfg import lm13_cfg

OK = [0, 0, 1, 0, 1, 1, 1, 1]


def _solve_all(a):
    return [H.ransac(a["cam_points"][n, :c], a["model_points"][n, :c], H.DIST_THR, H.ITERS, H.SEED, n) for n, c in enumerate(a["counts"])]


def test_fixture_is_deterministic_and_has_the_edge_rois():
    a, b = H.make_rigid_inputs("clean"), H.make_rigid_inputs("clean")
    for k in ("cam_points", "model_points", "counts", "R", "t", "inlier"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
    assert tuple(a["counts"]) == (0, 2, 3, 5, 257, 513, 4096, 600) and a["cam_points"].shape == (8, 4096, 3) and a["cam_points"].dtype == np.float64
    for case in ("clean", "noisy"):
        a = H.make_rigid_inputs(case)
        for n, c in enumerate(a["counts"]):
            assert np.isnan(a["cam_points"][n, c:]).all() and np.isnan(a["model_points"][n, c:]).all() and not a["inlier"][n, c:].any()
            assert np.isfinite(a["cam_points"][n, :c]).all() and np.abs(a["model_points"][n, :c]).max(initial=0.0) <= 0.1
            d = np.linalg.norm(a["model_points"][n, :c] @ a["R"][n].T + a["t"][n] - a["cam_points"][n, :c], axis=1)
            m = a["inlier"][n, :c]
            assert (d[m] <= (1e-3 + 1e-12 if case == "noisy" else 1e-15)).all()
            if c >= 257:   # 40 % outliers, 30 .. 120 mm off, never in the first 3 rows
                assert 0.3 < 1.0 - m.mean() < 0.5 and m[:3].all()
                assert d[~m].min() >= 0.03 - 1e-12 and d[~m].max() <= 0.12 + 1e-12
            else:
                assert m.all()
        assert np.array_equal(a["R"][3], np.eye(3)) and 0.3 <= a["t"][:, 2].min() and a["t"][:, 2].max() <= 2.0
        X3, X7 = a["model_points"][3, :5], a["model_points"][7, :600]
        assert np.linalg.matrix_rank(X3 - X3.mean(0), tol=1e-12) == 1 and np.linalg.matrix_rank(X7 - X7.mean(0), tol=1e-9) == 2


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_host_ransac_recovers_the_clean_fixture(seed):
    """the yardstick before the GPU is judged by it: ok pattern, the winner already counts the true set, final mask = truth, deviation <= 1e-12"""
    a = H.make_rigid_inputs("clean", seed)
    res = _solve_all(a)
    assert [r["ok"] for r in res] == OK
    worst = 0.0
    for n, (r, c) in enumerate(zip(res, a["counts"])):
        if not r["ok"]:
            assert r["num_inliers"] == 0 and not r["mask"].any() and np.isnan(r["rms"])
            continue
        truth = a["inlier"][n, :c]
        assert np.array_equal(r["mask"], truth) and r["num_inliers"] == truth.sum() and r["winner_count"] == truth.sum(), n
        assert abs(np.linalg.det(r["R"]) - 1.0) < 1e-12 and r["rms"] < 1e-12
        worst = max(worst, H.deviation(r["R"], r["t"], a["R"][n], a["t"][n]))
    print(f"worst deviation of the host RANSAC from the ground truth, seed {seed}: {worst:.3e} (bound 1e-12)")
    assert worst <= 1e-12


def test_host_ransac_on_the_noisy_fixture_finds_the_true_inliers():
    a = H.make_rigid_inputs("noisy")
    res = _solve_all(a)
    assert [r["ok"] for r in res] == OK
    for n, (r, c) in enumerate(zip(res, a["counts"])):
        if r["ok"]:
            truth = a["inlier"][n, :c]
            assert np.array_equal(r["mask"], truth), n
            R, t, ok = H.kabsch(a["model_points"][n, :c][truth], a["cam_points"][n, :c][truth])
            assert ok and H.deviation(r["R"], r["t"], R, t) <= 1e-12   # the closed-form minimum on that set: reached, not approached
            assert 0.0 < r["rms"] <= 1e-3


def test_draw_rule_against_hand_computed_indices():
    # mix64(0) = 0: the draw with an all-zero key is index 0 whatever the count
    assert H.mix64(0) == 0 and H.draw(0, 0, 0, 0, 4096) == 0
    # n = 1 alone: key = 0xBF58476D1CE4E5B9, worked through the three steps of the finaliser by hand
    x = 0xBF58476D1CE4E5B9
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    x ^= x >> 31
    assert H.draw(0, 1, 0, 0, 1000) == ((x >> 32) * 1000) >> 32
    # values recorded from the shared device / host header (csrc/ransac_draw.h compiled for the host)
    assert H.draw(0, 3, 7, 2, 257) == 68 and H.draw(12345, 7, 99, 63, 600) == 386 and H.draw(2 ** 64 - 1, 1, 1, 1, 3) == 1
    for count in (3, 5, 4096):
        for h in range(50):
            idx = H.sample3(0, 2, h, count)
            assert idx is not None and len(set(idx)) == 3 and all(0 <= i < count for i in idx)
            drawn = [H.draw(0, 2, h, d, count) for d in range(H.MAX_DRAWS)]
            first = list(dict.fromkeys(drawn))[:3]   # the first three distinct values, in order
            assert idx == first
    assert H.sample3(0, 0, 0, 2) is None   # two rows cannot give three distinct indices: dropped after 64 draws


def test_kabsch_is_proper_on_a_reflected_set_and_exact_on_a_rotated_one():
    X = 0.1 * H.synth.hash_uniform(5, "X", (40, 3)) - 0.05
    R0 = H.synth._random_rotations(5, "R", 1)[0]
    t0 = np.array([0.1, -0.2, 0.9])
    R, t, ok = H.kabsch(X, X @ R0.T + t0)
    assert ok and H.deviation(R, t, R0, t0) < 1e-14
    M = R0 @ np.diag([1.0, 1.0, -1.0])   # a reflection: the optimum over O(3) is improper
    R, t, ok = H.kabsch(X, X @ M.T + t0)
    assert ok and abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    # ... and it is the best proper rotation: no nearby rotation does better
    cost = lambda Rr: (H.residual2(Rr, (X @ M.T + t0).mean(0) - Rr @ X.mean(0), X, X @ M.T + t0)).sum()  # noqa: E731
    for k in range(6):
        w = 1e-3 * np.eye(3)[k % 3] * (1 if k < 3 else -1)
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Rn = (np.eye(3) + Wx + 0.5 * Wx @ Wx) @ R
        U, _, Vt = np.linalg.svd(Rn)
        assert cost(U @ Vt) >= cost(R)


def test_degeneracy_rule_on_collinear_and_coplanar_sets():
    R0 = H.synth._random_rotations(6, "R", 1)[0]
    t0 = np.array([0.0, 0.1, 0.5])
    s = np.array([[-1.0], [-0.3], [0.2], [0.7], [1.0]])
    line = np.array([0.01, 0.02, -0.03]) + s * np.array([0.03, -0.02, 0.05])
    assert not H.kabsch(line, line @ R0.T + t0)[2]                       # collinear: no unique rotation
    assert not H.kabsch(line[:3], line[:3] @ R0.T + t0)[2]
    assert not H.kabsch(line[[0, 0, 4]], line[[0, 0, 4]] @ R0.T + t0)[2]   # a repeated point
    bent = line.copy()
    bent[2, 0] += 1e-12                                                   # off the line by less than the rule resolves
    assert not H.kabsch(bent, bent @ R0.T + t0)[2]
    bent[2, 0] += 1e-3                                                    # ... and by more
    assert H.kabsch(bent, bent @ R0.T + t0)[2]
    plane = 0.1 * H.synth.hash_uniform(6, "P", (30, 3)) - 0.05
    plane[:, 2] = 0.3 * plane[:, 0] - 0.2 * plane[:, 1] + 0.01
    R, t, ok = H.kabsch(plane, plane @ R0.T + t0)                         # coplanar: rank 2 is still unique
    assert ok and H.deviation(R, t, R0, t0) < 1e-13
    R, t, ok = H.kabsch(plane[:3], plane[:3] @ R0.T + t0)                 # the minimal sample is always coplanar
    assert ok and H.deviation(R, t, R0, t0) < 1e-12
    assert not H.kabsch(plane[:2], plane[:2])[2]                          # fewer than 3 pairs


def test_host_backproject_rules():
    depth = np.full((4, 6), 2.0, dtype=np.float32)
    depth[1, 2], depth[2, 2], depth[3, 2], depth[0, 2] = 0.0, np.nan, -1.0, np.inf
    K = np.array([[100.0, 0.0, 3.0], [0.0, 50.0, 2.0], [0.0, 0.0, 1.0]])
    img = np.array([[0.0, 0.0], [2.0, 1.0], [5.49, 3.49], [5.5, 0.0], [-0.5, 0.0], [-0.51, 0.0], [1.5, 0.5], [np.nan, 1.0], [2.0, 2.0], [2.0, 3.0],
                    [2.0, 0.0], [4.0, 3.0]], dtype=np.float32)
    mod = np.arange(36, dtype=np.float32).reshape(12, 3)
    cam, mo, k = H.backproject(img, mod, 11, depth, K)
    # rows: 0 ok | 1 zero depth | 2 ok (rounds to the last pixel) | 3 one past the right border | 4 ok (-0.5 rounds to 0) | 5 outside | 6 ok, pixel (2, 1)
    # is the zero -> invalid | 7 NaN | 8 NaN depth | 9 negative depth | 10 inf depth | 11 beyond counts
    assert k == 3 and np.array_equal(mo[:3], mod[[0, 2, 4]].astype(np.float64)) and np.isnan(cam[3:]).all() and np.isnan(mo[3:]).all()
    assert np.allclose(cam[0], [(0 - 3) / 100 * 2, (0 - 2) / 50 * 2, 2.0], rtol=1e-14)
    assert np.allclose(cam[1], [(np.float32(5.49) - 3) / 100 * 2, (np.float32(3.49) - 2) / 50 * 2, 2.0], rtol=1e-14)   # the ray of (u, v) itself, not of the pixel centre
    assert H.backproject(img, mod, 11, depth, np.zeros((3, 3)))[2] == 0   # singular K: nothing is valid


def test_wrappers_reject_bad_calls_before_loading_anything(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded for a call that is refused")

    monkeypatch.setattr(cabi, "load", no_load)
    a = H.make_rigid_inputs("clean")
    cam, mod = (torch.from_numpy(a[k][:, :16].copy()) for k in ("cam_points", "model_points"))
    cnt = np.minimum(a["counts"], 16)
    R0, t0 = torch.from_numpy(a["R"]), torch.from_numpy(a["t"])
    img = torch.zeros(8, 16, 2)
    depth = torch.ones(2, 48, 64)
    frame = np.zeros(8, dtype=np.int64)
    K = torch.eye(3, dtype=torch.float64)
    with pytest.raises(cabi.GdrnHipError):   # CPU tensors: no fallback
        rigid.rigid_ransac(cam, mod, cnt)
    with pytest.raises(cabi.GdrnHipError):
        rigid.rigid_fit(cam, mod, cnt, R0, t0)
    with pytest.raises(cabi.GdrnHipError):
        rigid.rigid_ransac(cam.numpy(), mod.numpy(), cnt)
    with pytest.raises(cabi.GdrnHipError):
        rigid.backproject(img, mod.float(), cnt, depth, frame, K)
    for bad in (dict(dist_thr=0.0), dict(dist_thr=-1.0), dict(dist_thr=float("nan")), dict(iters=0), dict(iters=-3)):   # non-positive gate / count
        with pytest.raises(ValueError):
            rigid.rigid_ransac(cam, mod, cnt, **bad)
        with pytest.raises(ValueError):
            rigid.poses_from_maps_rgbd(lm13_cfg(), {}, None, None, 480, 640, K, depth, frame, **bad)
    with pytest.raises(ValueError):          # mismatched shapes
        rigid.rigid_ransac(cam, mod[:7], cnt)
    with pytest.raises(ValueError):
        rigid.rigid_ransac(cam, mod[:, :, :2], cnt)
    with pytest.raises(ValueError):
        rigid.rigid_fit(cam, mod, cnt[:7])
    with pytest.raises(ValueError):          # a count above the stride
        rigid.rigid_ransac(cam, mod, a["counts"])
    with pytest.raises(ValueError):
        rigid.backproject(img, mod[:7].float(), cnt, depth, frame, K)
    with pytest.raises(ValueError):
        rigid.backproject(img[:, :, :1], mod.float(), cnt, depth, frame, K)
    with pytest.raises(ValueError):
        rigid.backproject(img, mod.float(), cnt, depth, frame, K.repeat(5, 1, 1))
    with pytest.raises(ValueError):          # a frame outside [0, F)
        rigid.backproject(img, mod.float(), cnt, depth, frame + 2, K)
    with pytest.raises(ValueError):
        rigid.backproject(img, mod.float(), cnt, depth, frame[:3], K)
    for bad_depth in (depth.double(), depth[0], depth[:, :, :0], depth.to(torch.float16)):   # depth_scene that is not fp32 [F,H,W]
        with pytest.raises(ValueError):
            rigid.backproject(img, mod.float(), cnt, bad_depth, frame, K)
        with pytest.raises(ValueError):
            rigid.poses_from_maps_rgbd(lm13_cfg(), {}, None, None, 480, 640, K, bad_depth, frame)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")  # noqa: E731
    with pytest.raises(ValueError):          # tensors on different devices
        rigid.rigid_ransac(cam, meta(mod), cnt)
    with pytest.raises(ValueError):
        rigid.backproject(img, mod.float(), cnt, meta(depth), frame, K)
    with pytest.raises(ValueError):
        rigid.backproject(meta(img), mod.float(), cnt, depth, frame, K)
    with pytest.raises(ValueError):
        rigid.poses_from_maps_rgbd(lm13_cfg(), dict(mask=meta(torch.zeros(8, 1, 64, 64))), None, None, 480, 640, K, depth, frame)


def test_workspace_query_and_abi_symbols():
    for name in ("gdrn_backproject_points", "gdrn_rigid_workspace_bytes", "gdrn_rigid_ransac", "gdrn_rigid_fit"):
        assert name in cabi.EXPORTS
    lib = cabi.load()
    ws = lib.gdrn_rigid_workspace_bytes
    assert ws(1, 1, 1) > 0 and ws(8, 4096, 100) >= 8 * 4096 + 8 * 12 * 8
    assert ws(0, 4096, 100) == -1 and ws(8, 0, 100) == -1 and ws(8, 4096, 0) == -1
    assert ws(1 << 20, 1 << 12, 100) > 2 ** 31   # a long long
    assert lib.gdrn_version() == 5
