"""CPU tests (-m "not gpu") of gdrnet_amd.bop_metrics: the host oracle (tests/bop_host.py) and the numpy restatement of
misc.get_symmetry_transformations against golden G14 (the reference's pose_error.vsd / mssd / mspd on the fixtures), table packing, the checks
that raise before any launch, the exported symbols, and the properties the fixtures are meant to have."""
import os

import numpy as np
import pytest
import torch

import bop_host as BH
from gdrnet_amd import bop_metrics as BM
from gdrnet_amd import cabi, render, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_vsd_workspace_bytes", "gdrn_vsd", "gdrn_mssd_mspd_workspace_bytes", "gdrn_mssd_mspd", "gdrn_bop_recall_accumulate")


@pytest.fixture(scope="module")
def g14(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g14_bop_metrics.npz")))


@pytest.fixture(scope="module")
def sym_inp():
    return synth.make_bop_metric_inputs("sym")


def test_host_vsd_equals_the_reference(g14):
    assert int(g14["vsd/seed"]) == synth.BOP_METRIC_SEEDS["vsd"]
    scene = BH.vsd_scene()
    err, counts = BH.vsd_all(scene, "step")
    assert np.array_equal(counts, g14["vsd/counts"])
    assert np.array_equal(err, g14["vsd/err_step"])   # the same integers, the same division
    err_t, counts_t = BH.vsd_all(scene, "tlinear")
    assert np.array_equal(counts_t, counts)
    n_inter = (counts[:, 0] - counts[:, 1])[:, None]
    assert np.all(np.abs(err_t - g14["vsd/err_tlinear"]) <= (n_inter + 4) * 2.0 ** -52 * g14["vsd/err_tlinear"])


def test_host_mssd_mspd_equal_the_reference(g14, sym_inp):
    assert int(g14["sym/seed"]) == synth.BOP_METRIC_SEEDS["sym"]
    err, _ = BH.mssd_mspd_all(sym_inp)
    assert err.shape == g14["sym/err"].shape == (41, 2)
    assert np.all(np.abs(err[:, 0] - g14["sym/err"][:, 0]) <= 1e-13) and np.all(np.abs(err[:, 1] - g14["sym/err"][:, 1]) <= 1e-10)


def test_symmetry_transformations_equal_the_reference(g14, sym_inp):
    for c, info in enumerate(sym_inp["model_infos"]):
        R, t = BM.symmetry_transformations(info, 0.01)
        assert R.shape == g14[f"sym/R{c}"].shape and t.shape == g14[f"sym/t{c}"].shape == (len(R), 3)
        assert np.all(np.abs(R - g14[f"sym/R{c}"]) <= 1e-15) and np.all(np.abs(t - g14[f"sym/t{c}"]) <= 1e-15)
    sizes = [len(BM.symmetry_transformations(m)[0]) for m in sym_inp["model_infos"]]
    assert sizes == [314, 3, 1, 314]
    R, _ = BM.symmetry_transformations(sym_inp["model_infos"][0])
    assert not any(np.array_equal(r, np.eye(3)) for r in R)   # the reference's quirk: range(1, n) leaves the identity out
    R1, t1 = BM.symmetry_transformations(sym_inp["model_infos"][1])
    assert np.array_equal(R1[0], np.eye(3)) and not t1[0].any() and t1[1:].any()
    both = dict(sym_inp["model_infos"][0], symmetries_discrete=sym_inp["model_infos"][1]["symmetries_discrete"])
    assert len(BM.symmetry_transformations(both)[0]) == 3 * 314
    assert len(BM.symmetry_transformations(sym_inp["model_infos"][0], 0.1)[0]) == 31


def test_table_packing(sym_inp):
    t = BM.BopModelTable(sym_inp["points"], sym_inp["diameters"], sym_inp["syms"], pad_value=7.0, sym_pad_value=np.nan)
    assert t.num_classes == 4 and t.n_max == 8195 and t.s_max == 314 and list(t.npts) == [1031, 257, 1, 8195] and list(t.nsym) == [314, 3, 1, 314]
    assert t.pts.shape == (4, 8195, 3) and t.sym_R.shape == (4, 314, 3, 3) and t.sym_t.shape == (4, 314, 3)
    assert t.pts.dtype == t.sym_R.dtype == t.sym_t.dtype == t.diameter.dtype == np.float64 and t.npts.dtype == t.nsym.dtype == np.int32
    for c, p in enumerate(sym_inp["points"]):
        assert np.array_equal(t.pts[c, : len(p)], p) and np.all(t.pts[c, len(p):] == 7.0)
    assert np.array_equal(t.sym_R[1, :3], sym_inp["syms"][1][0]) and np.array_equal(t.sym_t[1, :3], sym_inp["syms"][1][1])
    assert np.isnan(t.sym_R[1, 3:]).all() and np.isnan(t.sym_t[2, 1:]).all()
    assert np.array_equal(t.sym_R[2, 0], np.eye(3)) and not t.sym_t[2, 0].any()   # None: the identity only
    plain = BM.BopModelTable(sym_inp["points"][:2], sym_inp["diameters"][:2])
    assert plain.s_max == 1 and list(plain.nsym) == [1, 1] and np.array_equal(plain.sym_R[1, 0], np.eye(3))
    with pytest.raises(ValueError):
        BM.BopModelTable(sym_inp["points"], sym_inp["diameters"][:3])
    with pytest.raises(ValueError):
        BM.BopModelTable(sym_inp["points"], sym_inp["diameters"], sym_inp["syms"][:2])
    with pytest.raises(ValueError):
        BM.BopModelTable([np.zeros((0, 3))], [0.1])
    with pytest.raises(ValueError):
        BM.BopModelTable([np.zeros((2, 3))], [0.1], [(np.zeros((0, 3, 3)), np.zeros((0, 3)))])
    with pytest.raises(ValueError):
        BM.BopRecall(t, ["a", "b"], 640)
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(ValueError):
            t.check_labels(bad)
    assert t.check_labels(torch.tensor([3, 0])).dtype == np.int32


def test_no_cpu_fallback_and_checks_before_any_launch(sym_inp):
    t = BM.BopModelTable(sym_inp["points"], sym_inp["diameters"], sym_inp["syms"])
    poses = [torch.from_numpy(sym_inp[k]) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    with pytest.raises(cabi.GdrnHipError):
        BM.mssd_mspd(t, *poses, sym_inp["labels"])
    d = torch.zeros(2, 5, 7)
    with pytest.raises(cabi.GdrnHipError):
        BM.vsd_from_depth(d, d, d, [0, 0], poses[4][:2], [0.1, 0.1], 0.015)
    with pytest.raises(ValueError):
        BM.vsd_from_depth(d, d, d, [0, 0], poses[4][:2], [0.1, 0.1], 0.015, cost_type="linear")
    with pytest.raises(cabi.GdrnHipError):
        BM.BopRecall(t, sym_inp["obj_names"], 640).update(torch.zeros(3, 10), torch.zeros(3, 2), [0, 1, 2])
    with pytest.raises(cabi.GdrnHipError):
        BM.BopRecall(t, sym_inp["obj_names"], 640).add_missing(0, 1)
    # the C entry points themselves: a label / frame outside its range is refused on the host copy, before a stream or a device pointer is touched
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    p = one.ctypes.data
    for frames, F in (([0, 3], 3), ([-1, 0], 3), ([0, 0], 0)):
        fr = np.array(frames, dtype=np.int32)
        assert lib.gdrn_vsd(p, p, p, p, fr.ctypes.data, F, p, p, 2, 5, 7, 0.015, p, 10, 0, 1, p, p, p, None) == -1
    fr = np.zeros(2, dtype=np.int32)
    assert lib.gdrn_vsd(p, p, p, p, fr.ctypes.data, 1, p, p, 2, 5, 7, 0.015, p, 10, 2, 1, p, p, p, None) == -1    # cost type
    assert lib.gdrn_vsd(p, p, p, p, fr.ctypes.data, 1, p, p, 2, 5, 7, 0.015, p, 33, 0, 1, p, p, p, None) == -2    # more taus than GDRN_VSD_MAX_TAUS
    assert lib.gdrn_vsd(None, p, p, p, fr.ctypes.data, 1, p, p, 2, 5, 7, 0.015, p, 10, 0, 1, p, p, p, None) == -1
    for labels in ([0, 4], [-1, 0]):
        lab = np.array(labels, dtype=np.int32)
        assert lib.gdrn_mssd_mspd(p, p, p, p, p, p, lab.ctypes.data, 2, p, p, 8, p, p, p, 3, 4, p, p, None) == -1
        assert lib.gdrn_bop_recall_accumulate(p, 10, p, p, lab.ctypes.data, 2, p, 4, 640.0, p, p, p, p, p, p, p, None) == -1
    lab = np.zeros(2, dtype=np.int32)
    assert lib.gdrn_mssd_mspd(p, p, p, p, p, p, lab.ctypes.data, 2, p, p, 8, p, p, p, 0, 4, p, p, None) == -1
    assert lib.gdrn_bop_recall_accumulate(p, 10, p, p, lab.ctypes.data, 2, p, 4, 0.0, p, p, p, p, p, p, p, None) == -1
    assert lib.gdrn_bop_recall_accumulate(p, 33, p, p, lab.ctypes.data, 2, p, 4, 640.0, p, p, p, p, p, p, p, None) == -2


def test_workspace_queries():
    lib = cabi.load()
    v, m = lib.gdrn_vsd_workspace_bytes, lib.gdrn_mssd_mspd_workspace_bytes
    assert v(12, 47, 61, 10) == 12 * 2 * 10 * 8 and v(1, 1, 1, 1) == 8 and v(64, 480, 640, 10) == 64 * 150 * 10 * 8
    assert v(0, 4, 4, 1) == -1 and v(1, 0, 4, 1) == -1 and v(1, 4, 4, 0) == -1 and v(1, 4, 4, 33) == -2 and v(70000, 4, 4, 1) == -2
    assert m(1, 1, 1) == (5 + 2) * 8 and m(41, 8195, 314) == 41 * (5 * 8195 + 2 * 40) * 8
    assert m(0, 1, 1) == -1 and m(1, 0, 1) == -1 and m(1, 1, 0) == -1
    assert m(65535, 1 << 20, 314) > 2 ** 31   # a long long, not an int


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and hasattr(lib, name) and f" {name}(" in header
    assert "GDRN_VSD_MAX_TAUS 32" in header and "GDRN_BOP_NTH 10" in header and BM.MAX_TAUS == 32 and BM.NTH == 10
    assert np.array_equal(BM.VSD_THS, np.arange(0.05, 0.51, 0.05)) and np.array_equal(BM.MSPD_THS, np.arange(5, 51, 5)) and len(BM.VSD_TAUS) == 10


def test_vsd_fixture_has_the_rows_it_is_meant_to_have(g14):
    inp, est, gt, test = BH.vsd_scene()
    assert est.shape == gt.shape == (12, 47, 61) and test.shape == (3, 47, 61) and est.dtype == gt.dtype == test.dtype == np.float32
    assert (47 * 61) % 2048 != 0 and (47 * 61) % 64 != 0 and not inp["K"][:, 0, 1].any()
    assert sorted(set(inp["labels"])) == [0, 1, 2] and list(inp["frame"]) == [0] * 4 + [1] * 4 + [2] * 4
    assert not np.array_equal(inp["K"][0], inp["K"][8]) and np.array_equal(inp["K"][0], inp["K"][1])
    err, counts = g14["vsd/err_step"], g14["vsd/counts"]
    union, comp = counts[:, 0], counts[:, 1]
    assert np.array_equal(inp["R_est"][0], inp["R_gt"][0]) and np.array_equal(est[0], gt[0]) and union[0] > 100 and not err[0].any()
    assert union[3] > 0 and comp[3] == union[3] and np.all(err[3] == 1.0) and (est[3] != 0).any()    # off the object: empty intersection
    assert not est[4].any() and gt[4].any() and comp[4] == union[4] > 0                               # outside the frame
    assert union[5] == 0 and gt[5].any() and est[5].any() and np.all(err[5] == 1.0)                   # both hidden: empty union
    d5 = test[1][gt[5] > 0].astype(np.float64) - gt[5][gt[5] > 0]
    assert np.all(d5 < -inp["delta"] - 0.05)
    graded = [i for i in range(12) if np.all((err[i] > 0) & (err[i] < 1)) and len(set(err[i])) >= 5]
    assert len(graded) >= 5
    assert (test[1] == 0).sum() == 20 and ((test[1] == 0) & (gt[6] > 0)).sum() >= 10                  # the holes lie on row 6's object
    x = test[0][(gt[1] > 0)].astype(np.float64) - gt[1][gt[1] > 0]
    assert (x < -0.05).any() and (np.abs(x) < 0.0021).any()                                           # row 1: partly behind the occluder
    for th in BM.VSD_THS:
        assert (err < th).any() and (err >= th).any()


def test_sym_fixture_has_the_rows_it_is_meant_to_have(g14, sym_inp):
    inp, err = sym_inp, g14["sym/err"]
    assert [len(p) for p in inp["points"]] == [1031, 257, 1, 8195] and inp["syms"][2] is None and len(inp["labels"]) == 41
    assert np.abs(inp["syms"][1][1][1:]).max() > 0.01 and np.abs(inp["syms"][0][1]).max() > 0.01     # translation parts
    _, best = BH.mssd_mspd_all(inp)
    assert (best > 0).sum() >= 5 and best[5] == 2 and best[8] == 200
    for i in (5, 6, 8):
        assert err[i, 0] <= 1e-13 and err[i, 1] <= 1e-10
    assert np.array_equal(inp["R_est"][6], inp["R_gt"][6]) and err[6, 0] == 0.0 and err[6, 1] == 0.0
    # row 0, est = gt in a class with a continuous symmetry: the reference's set has no identity, the nearest member is one step away
    assert np.array_equal(inp["R_est"][0], inp["R_gt"][0]) and best[0] in (0, 313) and 1e-4 < err[0, 0] < 0.01
    e3, e2 = err[:, 0] / inp["diameters"][inp["labels"]], err[:, 1] * 640.0 / inp["im_width"]
    for th3, th2 in zip(BM.MSSD_THS, BM.MSPD_THS):
        assert (e3 < th3).any() and (e3 >= th3).any() and (e2 < th2).any() and (e2 >= th2).any()


def test_average_recall_on_hand_filled_counters():
    hv = np.zeros((3, 2, 10), dtype=np.int64)
    hs, hp = np.zeros((3, 10), dtype=np.int64), np.zeros((3, 10), dtype=np.int64)
    hv[0], hs[0], hp[0] = 4, 2, 1          # "pear": 4 targets
    hv[1, 0], hs[1, :5], hp[1] = 1, 2, 2   # "apple": 2 targets
    out = BM.average_recall(["pear", "apple", "never"], hv, hs, hp, [4, 2, 0])
    assert out["objects"]["pear"] == {"AR_VSD": 1.0, "AR_MSSD": 0.5, "AR_MSPD": 0.25, "AR": (1.0 + 0.5 + 0.25) / 3.0}
    assert out["objects"]["apple"] == {"AR_VSD": 0.25, "AR_MSSD": 0.5, "AR_MSPD": 1.0, "AR": (0.25 + 0.5 + 1.0) / 3.0}
    assert "never" not in out["objects"] and out["targets"] == 6
    assert out["all"]["AR_VSD"] == pytest.approx((4 * 20 + 10) / 6.0 / 20.0, abs=1e-15) and out["all"]["AR_MSPD"] == 0.5
    assert out["rows"][0] == ["objects", "AR_VSD", "AR_MSSD", "AR_MSPD", "AR"] and out["rows"][1][:3] == ["apple", "25.00", "50.00"]
    assert out["rows"][-1][0] == "all(6)" and all(isinstance(c, str) for r in out["rows"] for c in r)
    empty = BM.average_recall(["a"], hv[:1] * 0, hs[:1] * 0, hp[:1] * 0, [0])
    assert empty["objects"] == {} and np.isnan(empty["all"]["AR"]) and empty["targets"] == 0
    per, total = BH.average_recall(dict(hits_vsd=hv, hits_mssd=hs, hits_mspd=hp, seen=np.array([4, 2, 0])), 3)
    assert per[0] == out["objects"]["pear"] and per[1] == out["objects"]["apple"] and total == out["all"]


def test_mesh_table_serves_the_vsd_scene():
    inp = synth.make_bop_metric_inputs("vsd")
    t = render.MeshTable(inp["vertices"], inp["faces"])
    assert t.num_classes == 3 and list(t.nfaces) == [12, 1280, 128] and len(inp["diameters"]) == 3
