"""CPU tests (-m "not gpu") of gdrnet_amd.pnp: the host yardstick of the GPU tests (tests/pnp_host.py) recovers known poses, the wrappers refuse bad
calls before anything is loaded or launched, and there is no CPU fallback."""
import numpy as np
import pytest
import torch

import pnp_host as H
from gdrnet_amd import cabi, pnp, synth
from gdrnet_amd.cfg import lm13_cfg


def test_fixture_is_deterministic_and_has_the_edge_rois():
    a, b = synth.make_pnp_inputs("clean"), synth.make_pnp_inputs("clean")
    for k in ("image_points", "model_points", "counts", "K", "R", "t", "inlier"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
    assert tuple(a["counts"]) == (0, 3, 4, 5, 257, 1025, 4096, 600) and a["image_points"].shape == (8, 4096, 2) and a["image_points"].dtype == np.float64
    for n, c in enumerate(a["counts"]):
        assert np.isnan(a["image_points"][n, c:]).all() and np.isnan(a["model_points"][n, c:]).all() and not a["inlier"][n, c:].any()
        assert np.isfinite(a["image_points"][n, :c]).all()
        if c >= 257:   # 40 % outliers, at least 20 px off
            frac = 1.0 - a["inlier"][n, :c].mean()
            assert 0.3 < frac < 0.5
            uv, _ = H.project(a["K"][n], a["R"][n], a["t"][n], a["model_points"][n, :c])
            d = np.linalg.norm(uv - a["image_points"][n, :c], axis=1)
            assert d[~a["inlier"][n, :c]].min() >= 20.0 - 1e-9 and d[a["inlier"][n, :c]].max() < 1e-9
        else:
            assert a["inlier"][n, :c].all()
    assert np.array_equal(a["R"][3], np.eye(3)) and abs(H.rotation_angle(np.eye(3), a["R"][5]) - (np.pi - 5e-4)) < 1e-9
    assert 0.3 <= a["t"][:, 2].min() and a["t"][:, 2].max() <= 2.0
    X7 = a["model_points"][7, :600]
    assert np.linalg.matrix_rank(X7 - X7.mean(0), tol=1e-9) == 2
    noisy = synth.make_pnp_inputs("noisy")
    for n, c in enumerate(noisy["counts"]):
        uv, _ = H.project(noisy["K"][n], noisy["R"][n], noisy["t"][n], noisy["model_points"][n, :c])
        d = np.linalg.norm(uv - noisy["image_points"][n, :c], axis=1)
        m = noisy["inlier"][n, :c]
        assert (d[m] <= 1.0 + 1e-9).all() and (c < 4 or d[m].max() > 0.5) and (d[~m] >= 19.0).all()


def test_host_gauss_newton_recovers_the_ground_truth():
    """the yardstick before the GPU is judged by it: from 5 degrees / 5 % off, on the true inliers of every solvable RoI, to 1e-9"""
    a = synth.make_pnp_inputs("clean")
    worst = 0.0
    for n, c in enumerate(a["counts"]):
        if c < 4:
            continue
        m = a["inlier"][n, :c]
        R0, t0 = H.perturbed(a["R"][n], a["t"][n], k=n)
        assert abs(np.rad2deg(H.rotation_angle(R0, a["R"][n])) - 5.0) < 1e-6
        R, t, rms = H.gauss_newton(a["K"][n], a["model_points"][n, :c][m], a["image_points"][n, :c][m], R0, t0)
        dr, dt = H.rotation_angle(R, a["R"][n]), np.linalg.norm(t - a["t"][n]) / np.linalg.norm(a["t"][n])
        worst = max(worst, dr, dt)
        assert dr < 1e-9 and dt < 1e-9 and rms < 1e-9, (n, dr, dt, rms)
        assert np.array_equal(H.inliers(a["K"][n], R, t, a["model_points"][n, :c], a["image_points"][n, :c], 3.0), m)
    print(f"worst deviation of the host Gauss-Newton from the ground truth: {worst:.3e} (bound 1e-9)")


def test_wrappers_reject_bad_calls_before_loading_anything(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded for a call that is refused")

    monkeypatch.setattr(cabi, "load", no_load)
    a = synth.make_pnp_inputs("clean")
    img, mod, K = (torch.from_numpy(a[k][:, :16].copy()) for k in ("image_points", "model_points")), None, torch.from_numpy(a["K"])
    img, mod = img
    cnt = np.minimum(a["counts"], 16)
    R0, t0 = torch.from_numpy(a["R"]), torch.from_numpy(a["t"])
    with pytest.raises(cabi.GdrnHipError):   # CPU tensors: no fallback
        pnp.pnp_ransac(img, mod, cnt, K)
    with pytest.raises(cabi.GdrnHipError):
        pnp.pnp_refine(img, mod, cnt, K, R0, t0)
    with pytest.raises(cabi.GdrnHipError):
        pnp.pnp_ransac(img.numpy(), mod.numpy(), cnt, K)
    with pytest.raises(ValueError):          # mismatched N
        pnp.pnp_ransac(img, mod[:7], cnt, K)
    with pytest.raises(ValueError):
        pnp.pnp_ransac(img, mod, cnt[:7], K)
    with pytest.raises(ValueError):
        pnp.pnp_refine(img, mod, cnt, K[:5], R0, t0)
    with pytest.raises(ValueError):          # iters = 0
        pnp.pnp_ransac(img, mod, cnt, K, iters=0)
    with pytest.raises(ValueError):
        pnp.pnp_ransac(img, mod, cnt, K, reproj_err=0.0)
    with pytest.raises(ValueError):
        pnp.pnp_refine(img, mod, cnt, K, R0, t0, max_iter=0)
    with pytest.raises(ValueError):          # a count above the stride
        pnp.pnp_ransac(img, mod, a["counts"], K)
    with pytest.raises(ValueError):
        pnp.pnp_refine(img, mod, -cnt - 1, K, R0, t0)


def test_poses_from_maps_rejects_an_unknown_pnp_type():
    cfg = lm13_cfg()
    assert cfg.TEST.PNP_TYPE == "ransac_pnp"
    with pytest.raises(NotImplementedError):
        pnp.poses_from_maps(cfg, {}, None, None, 480, 640, None, pnp_type="net_ransac_pnp_rot")
    cfg.TEST.PNP_TYPE = "epnp"
    with pytest.raises(NotImplementedError):
        pnp.poses_from_maps(cfg, {}, None, None, 480, 640, None)


def test_workspace_query_and_abi_symbols():
    lib = cabi.load()
    ws = lib.gdrn_pnp_workspace_bytes
    assert ws(1, 1, 1) > 0 and ws(8, 4096, 100) >= 8 * 4096 + 8 * 12 * 8
    assert ws(0, 4096, 100) == -1 and ws(8, 0, 100) == -1 and ws(8, 4096, 0) == -1
    assert ws(1 << 20, 1 << 12, 100) > 2 ** 31   # a long long
    for name in ("gdrn_pnp_ransac", "gdrn_pnp_refine", "gdrn_pnp_workspace_bytes"):
        assert name in cabi.EXPORTS and hasattr(lib, name)
