"""GPU tests (-m gpu) of the batched PnP-RANSAC / iterative PnP (gdrnet_amd.pnp, csrc/pnp.hip) against known poses and the independent fp64 host
yardstick tests/pnp_host.py.  cv2's own result depends on its RNG and on EPnP and cannot be pinned without OpenCV: the feature is pinned to
geometry instead.

Fixture: synth.make_pnp_inputs -- 8 RoIs in one call (0, 3, 4, 5, 257, 1025, 4096 and 600 coplanar points in rows of 4096, NaN padding, 40 % outliers
>= 20 px off on the RoIs with >= 257 points), handed over in fp64 (as cv2 accepts them) so that the "clean" projections are exact.

Bounds.  Noise-free: 1e-8 on the rotation angle [rad] and on |dt| / |t| against the ground truth -- 100 x the 1e-10 stop tolerance of a quadratically
converging iteration; an fp32 step anywhere would miss it by orders of magnitude.  Bounded noise (inliers within a 1 px disc): 1e-7 against the host
Gauss-Newton on the true inlier set -- the same minimum reached by two iterations that each stop at 1e-10, with slack for linear convergence at
a non-zero residual; rms to 1e-9 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import pnp_host as H
from gdrnet_amd import cabi, pnp, synth
from gdrnet_amd.cfg import lm13_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOLVABLE = (2, 3, 4, 5, 6, 7)
KEYS = ("R", "t", "ok", "num_inliers", "rms", "inlier_mask")


def _upload(inp):
    return {k: torch.from_numpy(inp[k]).to(DEV) for k in ("image_points", "model_points", "counts", "K")}


def _start(N):
    """the R0 / t0 handed in: recognisable values the unsolved RoIs must hand back bit for bit"""
    R0 = torch.eye(3, dtype=torch.float64).repeat(N, 1, 1) * 0.5 + 0.125
    t0 = torch.arange(3 * N, dtype=torch.float64).reshape(N, 3) + 0.25
    return R0.to(DEV), t0.to(DEV)


def _run(dev, **kw):
    R0, t0 = _start(8)
    args = dict(reproj_err=3.0, iters=100, seed=0, R0=R0, t0=t0, want_mask=True)
    args.update(kw)
    out = pnp.pnp_ransac(dev["image_points"], dev["model_points"], dev["counts"], dev["K"], **args)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def clean():
    inp = synth.make_pnp_inputs("clean")
    dev = _upload(inp)
    return inp, dev, _run(dev)


@pytest.fixture(scope="module")
def noisy():
    inp = synth.make_pnp_inputs("noisy")
    dev = _upload(inp)
    ref = {}
    for n in SOLVABLE:   # the host yardstick, once: Gauss-Newton on the true inlier set from the ground truth
        c, m = inp["counts"][n], inp["inlier"][n]
        ref[n] = H.gauss_newton(inp["K"][n], inp["model_points"][n][m], inp["image_points"][n][m], inp["R"][n], inp["t"][n])
    return inp, dev, _run(dev), ref


def _deviation(R, t, R_ref, t_ref):
    return max(H.rotation_angle(R, R_ref), np.linalg.norm(t - t_ref) / np.linalg.norm(t_ref))


def _check_clean(inp, out, bound=1e-8):
    R0, t0 = (x.cpu().numpy() for x in _start(8))
    assert list(out["ok"]) == [0, 0, 1, 1, 1, 1, 1, 1], out["ok"]
    for n in (0, 1):   # not solvable: the caller's values, bit for bit
        assert np.array_equal(out["R"][n], R0[n]) and np.array_equal(out["t"][n], t0[n])
        assert out["num_inliers"][n] == 0 and not out["inlier_mask"][n].any() and np.isnan(out["rms"][n])
    worst = 0.0
    for n in SOLVABLE:
        worst = max(worst, _deviation(out["R"][n], out["t"][n], inp["R"][n], inp["t"][n]))
        assert np.array_equal(out["inlier_mask"][n].astype(bool), inp["inlier"][n]), n
    print(f"worst deviation from the ground truth: {worst:.3e} (bound {bound:.0e}); worst rms {np.nanmax(out['rms']):.3e} px")
    assert np.array_equal(out["num_inliers"], out["inlier_mask"].sum(axis=1))
    assert worst <= bound
    assert np.isfinite(out["R"]).all() and np.isfinite(out["t"]).all()
    return worst


def test_noise_free_recovery(clean):
    """bound 1e-8 against the ground truth (a host replay of the kernels' arithmetic: 2e-14; not yet measured on an MI355X)"""
    inp, _, out = clean
    _check_clean(inp, out)
    assert np.nanmax(out["rms"]) < 1e-8


def test_bounded_noise_matches_the_host_least_squares(noisy):
    """bounds 1e-7 against the host Gauss-Newton and 1e-9 relative on rms (not yet measured on an MI355X)"""
    inp, _, out, ref = noisy
    assert list(out["ok"]) == [0, 0, 1, 1, 1, 1, 1, 1], out["ok"]
    worst = worst_rms = 0.0
    for n in SOLVABLE:
        R_ref, t_ref, rms_ref = ref[n]
        worst = max(worst, _deviation(out["R"][n], out["t"][n], R_ref, t_ref))
        worst_rms = max(worst_rms, abs(out["rms"][n] - rms_ref) / rms_ref)
        assert np.array_equal(out["inlier_mask"][n].astype(bool), inp["inlier"][n]), n
    print(f"worst deviation from the host Gauss-Newton: {worst:.3e} (bound 1e-7); worst relative rms difference {worst_rms:.3e} (bound 1e-9)")
    assert np.array_equal(out["num_inliers"], out["inlier_mask"].sum(axis=1))
    assert worst <= 1e-7 and worst_rms <= 1e-9


def test_reproducibility_and_seeds(clean, noisy):
    inp, dev, out0, ref = noisy
    again = _run(dev)
    for k in KEYS:   # the same seed: the same bits in every output
        assert np.array_equal(out0[k].view(np.uint8), again[k].view(np.uint8)), k
    for seed in (1, 2):   # other samples, the same optimum
        o = _run(dev, seed=seed)
        assert list(o["ok"]) == list(out0["ok"])
        worst = max(_deviation(o["R"][n], o["t"][n], out0["R"][n], out0["t"][n]) for n in SOLVABLE)
        print(f"seed {seed} against seed 0: {worst:.3e} (bound 1e-7)")
        assert worst <= 1e-7
    cinp, cdev, _ = clean
    one = _run(cdev, iters=1)   # one hypothesis: may miss on the outlier RoIs, not on the clean minimal ones
    assert one["ok"][2] == 1 and one["ok"][3] == 1 and one["ok"][0] == 0 and one["ok"][1] == 0
    for n in (2, 3):
        assert _deviation(one["R"][n], one["t"][n], cinp["R"][n], cinp["t"][n]) <= 1e-8
    _check_clean(cinp, _run(cdev, iters=300))   # more hypotheses than threads


def test_fp32_correspondences_are_widened_exactly(noisy):
    """what gdrn_correspondences writes (fp32) gives the same bits as its exactly widened fp64 copy: same samples, same counts, same sums"""
    inp, dev, _, _ = noisy
    i32, m32 = dev["image_points"].float(), dev["model_points"].float()
    R0, t0 = _start(8)
    a = pnp.pnp_ransac(i32, m32, dev["counts"], dev["K"], R0=R0, t0=t0, want_mask=True)
    b = pnp.pnp_ransac(i32.double(), m32.double(), dev["counts"], dev["K"], R0=R0, t0=t0, want_mask=True)
    assert list(a["ok"].cpu()) == [0, 0, 1, 1, 1, 1, 1, 1]
    for k in KEYS:
        assert np.array_equal(a[k].cpu().numpy().view(np.uint8), b[k].cpu().numpy().view(np.uint8)), k
    ra = pnp.pnp_refine(i32[:4], m32[:4], dev["counts"][:4], dev["K"][:4], a["R"][:4], a["t"][:4])
    rb = pnp.pnp_refine(i32[:4].double(), m32[:4].double(), dev["counts"][:4], dev["K"][:4], a["R"][:4], a["t"][:4])
    for k in ("R", "t", "ok", "rms"):
        assert np.array_equal(ra[k].cpu().numpy().view(np.uint8), rb[k].cpu().numpy().view(np.uint8)), k


def test_refine_from_a_guess(clean):
    """pnp_refine on the outlier-free RoIs from 5 degrees / 5 % off reaches the host Gauss-Newton's result (bound 1e-8)"""
    inp, dev, _ = clean
    rows = [1, 2, 3]   # 3 (not solvable), 4 and 5 points
    R0 = np.stack([H.perturbed(inp["R"][n], inp["t"][n], k=n)[0] for n in rows])
    t0 = np.stack([H.perturbed(inp["R"][n], inp["t"][n], k=n)[1] for n in rows])
    sel = torch.tensor(rows, device=DEV)
    out = pnp.pnp_refine(dev["image_points"][sel], dev["model_points"][sel], dev["counts"][sel], dev["K"][sel], torch.from_numpy(R0).to(DEV),
                         torch.from_numpy(t0).to(DEV))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert list(out["ok"]) == [0, 1, 1]
    assert np.array_equal(out["R"][0], R0[0]) and np.array_equal(out["t"][0], t0[0]) and np.isnan(out["rms"][0])
    worst = 0.0
    for j, n in enumerate(rows[1:], start=1):
        c = inp["counts"][n]
        R_ref, t_ref, _ = H.gauss_newton(inp["K"][n], inp["model_points"][n, :c], inp["image_points"][n, :c], R0[j], t0[j])
        worst = max(worst, _deviation(out["R"][j], out["t"][j], R_ref, t_ref))
        assert out["rms"][j] < 1e-8
    print(f"pnp_refine against the host Gauss-Newton: {worst:.3e} (bound 1e-8)")
    assert worst <= 1e-8


def _maps_case():
    """N = 3 RoIs of 64x64 maps whose roi_coord_2d is the projection of the per-pixel model point; RoI 1's mask leaves 3 pixels above threshold"""
    src = synth.make_pnp_inputs("clean")
    rows, N, S, im_H, im_W = (4, 5, 6), 3, 64, 480, 640
    u = lambda tag, *shape: synth.hash_uniform(77, tag, shape).astype(np.float32)  # noqa: E731
    coor = [np.float32(0.05) + np.float32(0.9) * u(f"c{a}", N, 1, S, S) for a in range(3)]
    mask = u("mask", N, 1, S, S)
    mask[1] = 0.0
    mask[1, 0, 10, 20] = mask[1, 0, 30, 31] = mask[1, 0, 63, 63] = 1.0
    ext = (np.float32(0.08) + np.float32(0.04) * u("ext", N, 3)).astype(np.float32)
    # the model point of a pixel, in the reference's fp32 operation order; its projection in fp64, normalised and stored in fp32
    X = np.stack([(coor[a][:, 0] - np.float32(0.5)) * ext[:, a, None, None] for a in range(3)], axis=-1)   # [N,S,S,3] fp32
    R, t, K = src["R"][list(rows)], src["t"][list(rows)], src["K"][list(rows)]
    c2d = np.zeros((N, 2, S, S), dtype=np.float32)
    for n in range(N):
        uv, _ = H.project(K[n], R[n], t[n], X[n].reshape(-1, 3).astype(np.float64))
        c2d[n, 0] = (uv[:, 0] / im_W).reshape(S, S).astype(np.float32)
        c2d[n, 1] = (uv[:, 1] / im_H).reshape(S, S).astype(np.float32)
    return dict(coor=coor, mask=mask, ext=ext, X=X, R=R, t=t, K=K, c2d=c2d, im_H=im_H, im_W=im_W)


def test_poses_from_maps_end_to_end():
    """the three evaluator branches on synthetic maps.  Bound on the good RoIs: test 1's 1e-8 widened by the fp32 storage of the pixel coordinates
    alone -- each stored coordinate went through two fp32 roundings (u / im_W, then * im_W), relative 2^-24 each, so it is off by at most
    e = 2^-23 max|coordinate| pixels; a residual perturbation of norm <= e sqrt(2 n) moves the least-squares pose by at most e sqrt(2 n) / sigma_min(J)
    (J: the Jacobian of the n projections at the ground truth, rad and metres).  The model points are bit-equal to the ones the projection used."""
    from gdrnet_amd import postproc

    m = _maps_case()
    cfg = lm13_cfg()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    out_dict = dict(mask=dev(m["mask"]), coor_x=dev(m["coor"][0]), coor_y=dev(m["coor"][1]), coor_z=dev(m["coor"][2]))
    args = (dev(m["c2d"]), dev(m["ext"]), [m["im_H"]] * 3, [m["im_W"]] * 3)
    _, _, img, mod, counts = postproc.get_img_model_points_with_coords2d(cfg, out_dict, *args)
    counts = counts.cpu().numpy()
    assert counts[1] == 3 and counts[0] > 1000 and counts[2] > 1000
    bounds = {}
    for n in (0, 2):
        X = mod[n, : counts[n]].cpu().numpy()
        sel = m["mask"][n, 0].reshape(-1) > 0.5   # (min-max normalisation of a map that spans [~0, ~1) moves no pixel across 0.5 here: checked below)
        Xall = m["X"][n].reshape(-1, 3)
        keep = sel & (np.abs(Xall) > np.float32(0.0001) * m["ext"][n]).all(axis=1)
        if keep.sum() == counts[n]:
            assert np.array_equal(X, Xall[keep])   # bit-equal model points: the only fp32 effect left is the pixel coordinates'
        uv = img[n, : counts[n]].cpu().numpy().astype(np.float64)
        e = 2.0 ** -23 * np.abs(uv).max()
        exact, _ = H.project(m["K"][n], m["R"][n], m["t"][n], X.astype(np.float64))
        assert np.abs(exact - uv).max() <= e, (np.abs(exact - uv).max(), e)
        smin = np.linalg.svd(H.jacobian(m["K"][n], m["R"][n], m["t"][n], X.astype(np.float64)), compute_uv=False)[-1]
        bounds[n] = 1e-8 + e * np.sqrt(2.0 * counts[n]) / smin
    K = dev(m["K"])
    pose = pnp.poses_from_maps(cfg, out_dict, *args, K, pnp_type="ransac_pnp").cpu().numpy()
    assert pose.shape == (3, 3, 4) and pose.dtype == np.float64
    assert np.all(pose[1] == -100.0)
    for n in (0, 2):
        d = max(H.rotation_angle(pose[n, :, :3], m["R"][n]), np.linalg.norm(pose[n, :, 3] - m["t"][n]))   # (|t| >= 0.8: the absolute error bounds the relative one)
        print(f"ransac_pnp RoI {n}: deviation {d:.3e}, bound {bounds[n]:.3e}")
        assert d <= bounds[n]
    # the network's pose: RoI 0 a fair guess, RoI 1 anything, RoI 2 a translation 1.5 m from where the correspondences put it
    R_net = np.stack([H.perturbed(m["R"][n], m["t"][n], k=n)[0] for n in range(3)])
    t_net = np.stack([H.perturbed(m["R"][n], m["t"][n], k=n)[1] for n in range(3)])
    t_net[2] = m["t"][2] + np.array([0.0, 0.0, 1.5])
    out_dict.update(rot=dev(R_net.astype(np.float32)), trans=dev(t_net.astype(np.float32)))
    R32, t32 = R_net.astype(np.float32).astype(np.float64), t_net.astype(np.float32).astype(np.float64)
    cfg.TEST.PNP_TYPE = "net_iter_pnp"
    for kind in (None, "net_ransac_pnp"):
        pose = pnp.poses_from_maps(cfg, out_dict, *args, K, pnp_type=kind).cpu().numpy()
        assert np.array_equal(pose[1, :, :3], R32[1]) and np.array_equal(pose[1, :, 3], t32[1])   # thin RoI: the network pose
        assert np.array_equal(pose[2, :, 3], t32[2])                                               # moved more than 1 m: the network translation
        assert H.rotation_angle(pose[2, :, :3], m["R"][2]) <= bounds[2]                            # ... with the solver's rotation
        d = max(H.rotation_angle(pose[0, :, :3], m["R"][0]), np.linalg.norm(pose[0, :, 3] - m["t"][0]))
        print(f"{kind or cfg.TEST.PNP_TYPE} RoI 0: deviation {d:.3e}, bound {bounds[0]:.3e}")
        assert d <= bounds[0]


def test_abi_argument_errors_return_before_any_launch(clean):
    inp, dev, out = clean
    lib, N, S = cabi.load(), 8, 4096
    img, mod = dev["image_points"].float().contiguous(), dev["model_points"].float().contiguous()
    cnt, K = dev["counts"], dev["K"]
    host = (C.c_int * N)(*[int(c) for c in inp["counts"]])
    bad_host = (C.c_int * N)(*([int(c) for c in inp["counts"][:7]] + [S + 1]))
    R0, t0 = _start(N)
    R, t = R0.clone(), t0.clone()
    ok = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    num = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    rms = torch.full((N,), -7.0, dtype=torch.float64, device=DEV)
    mask = torch.full((N, S), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(lib.gdrn_pnp_workspace_bytes(N, S, 100), dtype=torch.uint8, device=DEV)
    p = cabi.ptr

    def ransac(img_=p(img), iters=100, host_=host, thr=3.0, n=N, stride=S, R_=p(R)):
        return lib.gdrn_pnp_ransac(img_, p(mod), p(cnt), host_, p(K), n, stride, thr, iters, 0, 20, R_, p(t), p(ok), p(num), p(mask), p(rms), p(ws), None)

    def refine(mod_=p(mod), host_=host, n=N, it=20):
        return lib.gdrn_pnp_refine(p(img), mod_, p(cnt), host_, p(K), n, S, it, p(R), p(t), p(ok), p(rms), None, None)

    assert ransac(img_=None) == -1 and ransac(iters=0) == -1 and ransac(host_=bad_host) == -1 and ransac(host_=None) == -1
    assert ransac(thr=0.0) == -1 and ransac(n=0) == -1 and ransac(stride=0) == -1 and ransac(R_=None) == -1
    assert refine(mod_=None) == -1 and refine(host_=bad_host) == -1 and refine(n=0) == -1 and refine(it=0) == -1
    torch.cuda.synchronize()
    assert torch.equal(R, R0) and torch.equal(t, t0) and bool((ok == -7).all()) and bool((num == -7).all()) and bool((rms == -7.0).all())
    assert bool((mask == 9).all())   # nothing ran
    with pytest.raises(ValueError):
        pnp.pnp_ransac(img, mod, [0, 3, 4, 5, 257, 1025, 4097, 600], K)
    # the valid call through the raw fp32 entry point computes what the wrapper does on the same fp32 data
    assert ransac() == 0
    torch.cuda.synchronize()
    want = pnp.pnp_ransac(img, mod, cnt, K, R0=R0, t0=t0, want_mask=True)
    assert torch.equal(R, want["R"]) and torch.equal(t, want["t"]) and torch.equal(ok, want["ok"]) and torch.equal(num, want["num_inliers"])
    assert torch.equal(mask, want["inlier_mask"]) and list(ok.cpu()) == [0, 0, 1, 1, 1, 1, 1, 1]
