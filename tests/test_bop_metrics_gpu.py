"""GPU tests of the BOP pose errors and the recall counts (csrc/bop_metrics.hip through gdrnet_amd.bop_metrics) against golden G14: the reference's
own pose_error.vsd / mssd / mspd on the fixtures of synth.make_bop_metric_inputs (tests/golden/make_golden_g14.py).

Bounds.  VSD, step cost: the three integer counts are equal for every row and tau -- the fixtures' seeds keep every visibility difference 8 fp32 ulps
and every pixel distance 1e-9 off its threshold, so the reference's decisions are not a matter of rounding -- and the error is one fp64 division of
the same two integers: 4 * 2^-52 relative.  tlinear: (n_inter + 4) * 2^-52 relative, the bound of a sum of n_inter non-negative fp64 terms taken in
another order than numpy's, plus the division.  MSSD: 1e-13 m absolute -- posed coordinates are <= 1.5 m and carry about 4 roundings of 2^-53
relative on either side (~7e-16 each), a tenfold margin on top.  MSPD: 1e-10 px -- pixel coordinates <= 700 after a division by z >= 0.3.  The
measured deviations are printed (and recorded in DESIGN.md section 7)."""
import os

import numpy as np
import pytest
import torch

import bop_host as BH
from gdrnet_amd import bop_metrics as BM
from gdrnet_amd import render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def g14(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g14_bop_metrics.npz")))


@pytest.fixture(scope="module")
def sym():
    inp = synth.make_bop_metric_inputs("sym")
    return inp, BM.BopModelTable(inp["points"], inp["diameters"], inp["syms"])


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _vsd_host_depths(cost_type, rows=slice(None), test=None, **kw):
    inp, est, gt, dt = BH.vsd_scene()
    diam = inp["diameters"][inp["labels"]]
    err, counts = BM.vsd_from_depth(_dev(est[rows]), _dev(gt[rows]), _dev(dt if test is None else test), inp["frame"][rows], _dev(inp["K"][rows]),
                                    diam[rows], inp["delta"], inp["taus"], cost_type=cost_type, return_counts=True, **kw)
    torch.cuda.synchronize()
    assert err.dtype == torch.float64 and counts.dtype == torch.int64
    return err.cpu().numpy(), counts.cpu().numpy()


def _check_vsd(err, counts, g14, cost_type, what):
    ref, ref_counts = g14[f"vsd/err_{cost_type}"], g14["vsd/counts"]
    n_inter = (ref_counts[:, 0] - ref_counts[:, 1])[:, None]
    rel = np.abs(err - ref) / np.maximum(ref, 1e-300)
    print(f"{what} ({cost_type}): counts differ in {int((counts != ref_counts).sum())} cells, worst error deviation {rel.max() / EPS:.2f} x 2^-52, "
          f"worst / bound {np.max(rel / ((n_inter + 4) * EPS)):.3g} (tlinear bound)")
    assert err.shape == ref.shape == (12, 10) and np.array_equal(counts, ref_counts), what
    bound = 4 * EPS if cost_type == "step" else (n_inter + 4) * EPS
    assert np.all(np.abs(err - ref) <= bound * ref), what
    assert np.all(err[ref_counts[:, 0] == 0] == 1.0)


def test_vsd_from_host_depths_step(g14):
    _check_vsd(*_vsd_host_depths("step"), g14, "step", "vsd_from_depth")


def test_vsd_from_host_depths_tlinear(g14):
    _check_vsd(*_vsd_host_depths("tlinear"), g14, "tlinear", "vsd_from_depth")


def _vsd_device_render(cost_type, dtype=torch.float64, through_fp32=False):
    inp = synth.make_bop_metric_inputs("vsd")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    poses = [_dev(inp[k].astype(np.float32).astype(np.float64) if through_fp32 else inp[k], dtype) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    _, _, _, dt = BH.vsd_scene()
    err, counts = BM.vsd(meshes, inp["labels"], *poses, _dev(dt), inp["frame"], inp["diameters"], inp["delta"], inp["taus"], cost_type=cost_type,
                         return_counts=True)
    torch.cuda.synchronize()
    return err.cpu().numpy(), counts.cpu().numpy()


def test_vsd_with_the_device_render(g14):
    inp, est, gt, _ = BH.vsd_scene()
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    for host, R, t in ((est, "R_est", "t_est"), (gt, "R_gt", "t_gt")):   # the device depth is the host rasterizer's, bit for bit, on these seeds
        d = render.render_depth(meshes, inp["labels"], _dev(inp[R]), _dev(inp[t]), _dev(inp["K"]), inp["H"], inp["W"], inp["near"], inp["far"])
        assert np.array_equal(d.cpu().numpy().view(np.uint32), host.view(np.uint32)), R
    for cost in ("step", "tlinear"):
        _check_vsd(*_vsd_device_render(cost), g14, cost, "vsd")


def _mssd_mspd(inp, table, rows=slice(None), dtype=torch.float64, **over):
    poses = [_dev(over.get(k, inp[k])[rows], dtype) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    e = BM.mssd_mspd(table, *poses, inp["labels"][rows])
    torch.cuda.synchronize()
    assert e.dtype == torch.float64 and e.shape == (len(inp["labels"][rows]), 2)
    return e.cpu().numpy()


def test_mssd_mspd_against_the_reference(g14, sym):
    inp, table = sym
    got, ref = _mssd_mspd(inp, table), g14["sym/err"]
    d3, d2 = np.abs(got[:, 0] - ref[:, 0]), np.abs(got[:, 1] - ref[:, 1])
    print(f"mssd: worst deviation {d3.max():.3g} m (bound 1e-13), mspd: {d2.max():.3g} px (bound 1e-10); exact-symmetry rows "
          f"{[(i, float(got[i, 0]), float(got[i, 1])) for i in inp['exact_rows']]}")
    assert np.all(d3 <= 1e-13) and np.all(d2 <= 1e-10)
    for i in inp["exact_rows"]:   # est = gt o S_k: the same absolute bounds around 0
        assert got[i, 0] <= 1e-13 and got[i, 1] <= 1e-10
    assert got[6, 0] == 0.0 and got[6, 1] == 0.0   # est = gt, identity only: the same operations on both sides


def test_padding_never_enters_a_result(g14, sym):
    inp, table = sym
    clean = _mssd_mspd(inp, table)
    padded = BM.BopModelTable(inp["points"], inp["diameters"], inp["syms"], pad_value=1e3, sym_pad_value=np.nan)
    assert np.all(padded.pts[2, 1:] == 1e3) and np.isnan(padded.sym_R[1, 3:]).all() and not table.pts[2, 1:].any()
    assert np.array_equal(clean.view(np.uint64), _mssd_mspd(inp, padded).view(np.uint64))
    # VSD: a test frame no row refers to, and the model depths of rows that are not part of the call, are never read into a result
    _, est, gt, dt = BH.vsd_scene()
    for cost in ("step", "tlinear"):
        err, counts = _vsd_host_depths(cost)
        nan_frame = np.concatenate([dt, np.full((1,) + dt.shape[1:], np.nan, dtype=np.float32)])
        err2, counts2 = _vsd_host_depths(cost, test=nan_frame)
        assert np.array_equal(err.view(np.uint64), err2.view(np.uint64)) and np.array_equal(counts, counts2)
        dt3 = dt.copy()
        dt3[2] = np.nan   # frame 2 belongs to rows 8 .. 11 only
        err3, counts3 = _vsd_host_depths(cost, rows=slice(0, 8), test=dt3)
        assert np.array_equal(err[:8].view(np.uint64), err3.view(np.uint64)) and np.array_equal(counts[:8], counts3)


def test_repeated_calls_are_bit_identical_and_the_batch_split_does_not_matter(sym):
    inp, table = sym
    a = _mssd_mspd(inp, table)
    assert np.array_equal(a.view(np.uint64), _mssd_mspd(inp, table).view(np.uint64))
    halves = np.concatenate([_mssd_mspd(inp, table, slice(0, 20)), _mssd_mspd(inp, table, slice(20, 40))])
    assert np.array_equal(a[:40].view(np.uint64), halves.view(np.uint64))
    for cost in ("step", "tlinear"):
        err, counts = _vsd_host_depths(cost)
        err2, counts2 = _vsd_host_depths(cost)
        assert np.array_equal(err.view(np.uint64), err2.view(np.uint64)) and np.array_equal(counts, counts2)
        parts = [_vsd_host_depths(cost, rows=r) for r in (slice(0, 6), slice(6, 12))]
        assert np.array_equal(err.view(np.uint64), np.concatenate([p[0] for p in parts]).view(np.uint64))
        assert np.array_equal(counts, np.concatenate([p[1] for p in parts]))


def test_fp32_poses_are_accepted_and_nan_poses_give_nan(g14, sym):
    inp, table = sym
    as32 = {k: inp[k].astype(np.float32).astype(np.float64) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")}
    wide = _mssd_mspd(inp, table, **as32)
    assert np.array_equal(wide.view(np.uint64), _mssd_mspd(inp, table, dtype=torch.float32).view(np.uint64))   # fp32 -> fp64 widens exactly
    err32, counts32 = _vsd_device_render("step", torch.float32)
    err64, counts64 = _vsd_device_render("step", torch.float64, through_fp32=True)
    assert err32.shape == (12, 10) and np.array_equal(err32.view(np.uint64), err64.view(np.uint64)) and np.array_equal(counts32, counts64)
    bad = inp["R_est"].copy()
    bad[3, 1, 1] = np.nan
    bad[8] = np.nan
    got, clean = _mssd_mspd(inp, table, R_est=bad), _mssd_mspd(inp, table)
    assert np.isnan(got[[3, 8]]).all()
    keep = np.ones(len(got), dtype=bool)
    keep[[3, 8]] = False
    assert np.array_equal(got[keep].view(np.uint64), clean[keep].view(np.uint64))


def test_recall_counts_and_average_recall(g14, sym):
    inp, table = sym
    N = 36
    vsd_err = np.tile(g14["vsd/err_step"], (3, 1))   # the 12 VSD rows three times over, next to the first 36 MSSD / MSPD rows
    ms_err, labels = g14["sym/err"][:N], inp["labels"][:N]
    rec = BM.BopRecall(table, inp["obj_names"], inp["im_width"])
    rec.update(_dev(vsd_err[:20]), _dev(ms_err[:20]), labels[:20])
    rec.update(_dev(vsd_err[20:]), _dev(ms_err[20:]), _dev(labels[20:]))   # labels from the device as well
    for c, n in inp["missing"].items():
        rec.add_missing(c, n)
    got = rec.counters()
    ref = BH.recall_counts(vsd_err, ms_err, labels, inp["diameters"], inp["im_width"], 4, inp["missing"])
    for k in ("hits_vsd", "hits_mssd", "hits_mspd", "seen"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), k
    assert list(got["seen"]) == [11, 9, 10, 9] and got["hits_vsd"].shape == (4, 10, 10)
    assert 0 < got["hits_mssd"].sum() < 10 * N and 0 < got["hits_mspd"].sum() < 10 * N and 0 < got["hits_vsd"].sum() < 100 * N
    out = rec.summarize()
    per, total = BH.average_recall(ref, 4)
    for c, name in enumerate(inp["obj_names"]):
        for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
            assert abs(out["objects"][name][k] - per[c][k]) <= 1e-15
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert abs(out["all"][k] - total[k]) <= 1e-15 and 0.0 < out["all"][k] < 1.0
    assert out["targets"] == N + 3 and len(out["rows"]) == 6 and out["rows"][-1][0] == f"all({N + 3})"
    rec.reset()
    assert not rec.counters()["seen"].any()
