"""Pins tests/pose_host.py (the fp64 yardstick of pose_loss_kernel, tests/test_pose_loss_gpu.py) without a GPU: it reproduces the reference's
golden pose decodes (g3) and pose losses (g4) at the tolerances of tests/test_oracle_golden.py, its autograd rows equal central differences of
its own fp64 losses, its gradient is finite and continuous on the optical axis, every seeded input of the GPU module has signs that fp32
evaluation cannot flip, and the comparison the GPU module applies rejects a reference with one forward-mode partial dropped or one wave's sign
sum negated."""
import os

import numpy as np
import pytest
import torch

import pose_host as R
from gdrnet_amd import synth
from oracle import gdrn_oracle as O


def from_batch(pb, fc9, npts, centers=None, with_sym=False):
    N = fc9.shape[0]
    fc = np.zeros((N, 64), dtype=np.float32)
    fc[:, :9] = fc9
    n = lambda k: pb[k].numpy()
    a = dict(fc=fc, cams=n("roi_cam"), centers=n("roi_center") if centers is None else centers, whs=n("roi_wh"), ratios=n("resize_ratio"),
             extents=n("roi_extent"), gt_rot=n("ego_rot"), gt_trans=n("trans"), gt_trans_ratio=n("roi_trans_ratio"), points=n("roi_points")[:, :npts])
    if with_sym:
        K = max(1, max(0 if s is None else s.shape[0] for s in pb["sym_info"]))
        a["sym"], a["sym_count"] = np.full((N, K, 3, 3), np.nan, dtype=np.float32), np.zeros(N, dtype=np.int32)
        for i, s in enumerate(pb["sym_info"]):
            if s is not None:
                a["sym"][i, :s.shape[0]], a["sym_count"][i] = s.numpy(), s.shape[0]
    return a


def test_reproduces_the_golden_decodes_g3(golden_dir):
    g = np.load(os.path.join(golden_dir, "g3_pose.npz"))
    N = g["rot6d"].shape[0]
    a = from_batch(synth.make_batch(N, seed=21), np.concatenate([g["rot6d"], g["t_"]], 1), 64, centers=g["center"])
    for dtype in (torch.float64, torch.float32):
        r, t = R.reference(a, dtype), R.decode_test(a, dtype)
        np.testing.assert_allclose(r["trans"], g["trans_train"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(r["rot"], g["rot_train"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(t["rot"], g["rot_test"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(t["trans"], g["trans_test"], rtol=1e-6, atol=1e-7)
        assert np.abs(r["rot_allo"] - g["R_allo"]).max() < 1e-6


def test_reproduces_the_golden_pose_losses_g4(golden_dir):
    g = np.load(os.path.join(golden_dir, "g4_loss.npz"))
    B = 4
    batch = synth.make_batch(B, seed=7, num_classes=21, cam="ycbv", with_sym=True)
    mk = lambda name, shape, s=1.0: (synth.hash_normal(11, name, shape) * s).astype(np.float32)
    fc9 = np.concatenate([mk("r6", (B, 6)), mk("t", (B, 3), 0.3) + np.array([0.0, 0.0, 1.0], dtype=np.float32)], 1)
    for tag, sym in (("nosym", False), ("sym", True)):
        a = from_batch(batch, fc9, batch["roi_points"].shape[1], with_sym=sym)
        for dtype in (torch.float64, torch.float32):
            r = R.reference(a, dtype)
            names = list(g[f"normal/{tag}/names"])
            want = dict(zip(names, g[f"normal/{tag}/values"]))
            for k, nm in enumerate(("loss_PM_R", "loss_centroid", "loss_z")):
                np.testing.assert_allclose(r["losses"][k], want[nm], rtol=1e-5, atol=1e-7, err_msg=f"{tag} {nm}")
            np.testing.assert_allclose(r["rows"].sum(0), r["losses"], rtol=1e-6 if dtype == torch.float32 else 1e-13)
        if sym:
            assert (a["sym_count"] > 0).any()       # (the golden batch does carry symmetries)


def test_internal_identities():
    """dfc[0] = S . J (the kernel's contraction), S = the four wave parts, rows 1 and 2 of dfc are the signs over 2 N and N, zeros behind entry 9"""
    a = R.generic(64, 700)
    r = R.reference(a)
    N = 5
    np.testing.assert_allclose(np.einsum("nab,nabk->nk", r["S"], r["J"].reshape(N, 3, 3, 9)), r["dfc"][0][:, :9], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r["S_wave"].sum(0), r["S"], rtol=1e-12, atol=1e-15)
    sg = np.sign(R.f64(a["fc"])[:, 6:9] - R.f64(a["gt_trans_ratio"]))
    want = np.zeros((2, N, 64))
    want[0, :, 6:8], want[1, :, 8] = sg[:, :2] / (2 * N), sg[:, 2] / N
    assert np.array_equal(r["dfc"][1:], want) and not r["dfc"][0][:, 9:].any()
    np.testing.assert_allclose(r["vis"][:, 1], np.linalg.norm(R.f64(a["gt_trans"]) - r["trans"], axis=1), rtol=1e-14)


def test_autograd_rows_equal_central_differences():
    a = R.generic(12, 63, N=2)
    r = R.reference(a)
    b = dict(a)
    h = 1e-6
    for n in range(2):
        for k in range(9):
            L = []
            for s in (+1, -1):
                fc = R.f64(a["fc"]).copy()
                fc[n, k] += s * h
                b["fc"] = fc
                L.append(R.reference(b)["losses"])
            num = (L[0] - L[1]) / (2 * h)
            # second-order term of the central difference (h^2 times a third derivative of O(10)) and the fp64 noise of the losses over 2 h
            np.testing.assert_allclose(r["dfc"][:, n, k], num, rtol=1e-6, atol=1e-9, err_msg=f"RoI {n} input {k}")


@pytest.mark.parametrize("z", R.AXIS_Z)
def test_on_axis_gradient_is_finite_and_continuous(z):
    a = R.optical_axis(z, R.ORIGIN_K)
    keep = {k: (v[:1].copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    out = []
    for off in (0.0, 1e-9):
        b = dict(keep)
        b["centers"] = R.f64(keep["cams"])[:, :2, 2] + off
        out.append(R.reference(b))
    g0, g1 = out[0]["dfc"][0], out[1]["dfc"][0]
    assert np.isfinite(g0).all() and np.isfinite(out[0]["rot"]).all() and np.abs(g0).max() > 0
    assert np.abs(g0 - g1).max() <= 1e-5 * np.abs(g0).max()
    assert np.abs(out[0]["rot"] - out[1]["rot"]).max() <= 1e-9
    # and in fp32 on the axis itself (what e32 is taken from)
    assert np.isfinite(R.reference(keep, torch.float32)["dfc"]).all()


CASES = R.seeded_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_no_seeded_input_has_a_sign_that_rounding_decides(name):
    a = CASES[name]
    r64, r32 = R.both(a)
    for v in r64.values():
        assert np.isfinite(v).all() or v is r64["margin_deg"]
    unc = R.sign_uncertain(a, r64, r32)
    assert len(unc) == 0, f"{name}: {len(unc)} (RoI, point, axis) elements within rounding of 0, first {unc[:4].tolist()}"
    if name == "symmetry":
        assert tuple(r64["chosen_idx"]) == R.SYM_CHOICE == tuple(r32["chosen_idx"])
        assert (r64["margin_deg"][1:] >= 1.0).all(), r64["margin_deg"]
        assert (r64["vis"][1:3, 0] > 80.0).all() and abs(r64["vis"][3, 0] - 10.0) < 1e-3   # (against the UNsymmetrised gt)


def test_the_exact_match_case_is_sign_uncertain_on_purpose():
    a = dict(R.exact_match_first())
    a["gt_rot"] = R.f32(R.reference(a, torch.float32)["rot"])
    r64, r32 = R.both(a)
    assert len(R.sign_uncertain(a, r64, r32)) > 0.9 * r64["d"].size
    assert r32["losses"][0] == 0.0 and not r32["dfc"][0].any()      # (the oracle at the kernel's precision: abs has gradient 0 at 0)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_fc_tail_replay_equals_torch_fp32(splits, kind):
    t = R.fc_tail_inputs(splits, kind=kind)
    ref = R.fc_tail(t["ws"], t["bias"], t["w_rt"], t["b_rt"], kind)
    v = torch.zeros(3, 256)
    for sp in range(splits):
        v = v + torch.from_numpy(t["ws"][sp])
    v = torch.nn.functional.leaky_relu(v + torch.from_numpy(t["bias"]), 0.1)
    want = v.to(torch.float16 if kind == "fp16" else torch.bfloat16).float().numpy()
    assert np.array_equal(ref["f2"].view(np.int32), want.view(np.int32))
    assert (ref["pre"][:, :16] == 0).all() and (ref["pre"] < 0).sum() > 100 and (ref["pre"] > 0).sum() > 100
    assert np.array_equal(R.round16(t["w_rt"], kind), t["w_rt"])
    fc32 = (torch.from_numpy(ref["f2"]) @ torch.from_numpy(t["w_rt"]).T + torch.from_numpy(t["b_rt"])).numpy()
    assert (np.abs(fc32 - ref["fc"]) <= 0.5 * ref["fc_bound"]).all()       # an independent fp32 evaluation sits inside half the bound


# ------------------------------------------------------------------------------------------------ teeth
def test_comparison_rejects_a_dropped_partial_and_a_negated_wave_sum():
    """what the GPU module's generic case would see if the kernel lost one lane's partial of one rotation entry, or one wave's sign sums came in
    with the wrong sign: the reference's own dfc[0] rebuilt from S and J with that defect must fail check_decode()"""
    a = CASES["generic fs64 npts700"]
    r64, r32 = R.both(a)
    N = 5
    J = r64["J"].reshape(N, 3, 3, 9)
    clean = np.einsum("nab,nabk->nk", r64["S"], J)
    ok, e32, worst = R.check_decode(clean, r64, r32, "dfc0")
    assert ok and worst < 1e-12
    ok32, _, w32 = R.check_decode(r32["dfc"][0][:, :9], r64, r32, "dfc0")
    assert ok32 and abs(w32 - e32) < 1e-15
    rejected = 0
    for k in range(9):            # lane k loses its largest partial (RoI 0)
        ab = int(np.abs(r64["S"][0].reshape(9) * J[0].reshape(9, 9)[:, k]).argmax())
        bad = clean.copy()
        bad[0, k] -= r64["S"][0].reshape(9)[ab] * J[0].reshape(9, 9)[ab, k]
        rejected += not R.check_decode(bad, r64, r32, "dfc0")[0]
    assert rejected >= 6, rejected     # (t_ lanes 6..8 reach R only through the allo -> ego turn: their partials may be below the row's bound)
    lane, ab = 2, int(np.abs(r64["S"][0].reshape(9) * J[0].reshape(9, 9)[:, 2]).argmax())
    bad = clean.copy()
    bad[0, lane] -= r64["S"][0].reshape(9)[ab] * J[0].reshape(9, 9)[ab, lane]
    assert not R.check_decode(bad, r64, r32, "dfc0")[0]
    for v in range(4):
        S = r64["S"] - 2.0 * r64["S_wave"][v]
        assert not R.check_decode(np.einsum("nab,nabk->nk", S, J), r64, r32, "dfc0")[0], f"wave {v}"
    nan = clean.copy()
    nan[3, 4] = np.nan
    assert not R.check_decode(nan, r64, r32, "dfc0")[0]
