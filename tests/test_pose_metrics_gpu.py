"""GPU tests (-m gpu) of the on-device pose-error metrics (gdrnet_amd.pose_metrics, csrc/pose_metrics.hip) against golden G12: the reference's
own te / re / add / adi / arp_2d / get_closest_rot per row and its evaluator's recall table (tests/golden/make_golden_g12.py).

Bounds.  ad, te, proj: both sides are fp64 and differ in summation / dot-product order over <= 8195 terms (~1e-13): relative 1e-9 plus 1e-12
absolute for the exact-zero rows -- four digits of slack, and any fp32 step would miss it by five.  re: relative 1e-9 where the reference
value is >= 0.1 degree; on the near-zero rows (estimate = ground truth, or = ground truth times a symmetry) arccos at 1 turns a few ulps of
the trace into ~sqrt(2 k 1.1e-16) rad ~ 1e-6 degree: absolute 1e-5 degree there."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gdrnet_amd import cabi, pose_metrics as PM, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_pose_metrics.npz"))


def _case(case, g12, pad_value=0.0):
    assert int(g12[f"{case}/seed"]) == synth.POSE_METRIC_SEEDS[case]
    inp = synth.make_pose_metric_inputs(case)
    table = PM.ModelTable(inp["points"], inp["diameters"], inp["sym_infos"], inp["sym_classes"], pad_value=pad_value)
    poses = [torch.from_numpy(inp[k]).to(DEV) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    return inp, table, poses


@pytest.fixture(scope="module")
def case_a(g12):
    inp, table, poses = _case("A", g12)
    out = PM.pose_errors(table, *poses, inp["labels"])
    return inp, table, poses, out["err"].cpu().numpy()


@pytest.fixture(scope="module")
def case_b(g12):
    inp, table, poses = _case("B", g12)
    out = PM.pose_errors(table, *poses, inp["labels"])
    return inp, table, poses, out["err"].cpu().numpy()


def _check_against_golden(got, ref, rows=slice(None), cols=(0, 1, 2, 3)):
    got, ref = got[rows], ref[rows]
    for j, name in enumerate(PM.ERROR_NAMES):
        if j not in cols:
            continue
        diff = np.abs(got[:, j] - ref[:, j])
        if name == "re":
            big = ref[:, j] >= 0.1
            rel = (diff[big] / ref[big, j]).max() if big.any() else 0.0
            small = diff[~big].max() if (~big).any() else 0.0
            print(f"{name}: worst relative error {rel:.3e} on {int(big.sum())} rows (bound 1e-9), worst absolute error {small:.3e} deg on "
                  f"{int((~big).sum())} near-zero rows (bound 1e-5)")
            assert rel <= 1e-9 and small <= 1e-5, (name, rel, small)
        else:
            excess = (diff - (1e-9 * np.abs(ref[:, j]) + 1e-12)).max()
            print(f"{name}: worst |got - ref| {diff.max():.3e}, worst relative {np.max(diff / np.maximum(np.abs(ref[:, j]), 1e-300)):.3e} "
                  f"(bound 1e-9 relative + 1e-12)")
            assert excess <= 0.0, (name, int(np.argmax(diff)), diff.max())
    assert np.isfinite(got).all()


@pytest.mark.parametrize("case", ["A", "B"])
def test_errors_match_the_reference(case, g12, case_a, case_b):
    inp, _, _, got = case_a if case == "A" else case_b
    ref = g12[f"{case}/err"]
    assert got.shape == ref.shape == (len(inp["labels"]), 4) and got.dtype == np.float64
    _check_against_golden(got, ref)
    if case == "A":   # the exact rows: estimate = ground truth -> zero ad / te / proj, as the reference
        assert np.all(ref[[0, 4]][:, [0, 2, 3]] == 0) and np.all(got[[0, 4]][:, [0, 2, 3]] == 0)


def test_named_outputs_are_the_columns_and_fp32_poses_widen(case_b):
    inp, table, poses, got = case_b
    out = PM.pose_errors(table, *poses, torch.from_numpy(inp["labels"]))
    for j, name in enumerate(PM.ERROR_NAMES):
        assert out[name].shape == (3,) and out[name].dtype == torch.float64 and out[name].device.type == "cuda"
        assert torch.equal(out[name], out["err"][:, j])
    assert np.array_equal(out["err"].cpu().numpy(), got)
    # fp32 estimates: the same as handing over their exactly widened fp64 values
    r32, t32 = poses[0].float(), poses[1].float()
    a = PM.pose_errors(table, r32, t32, *poses[2:], inp["labels"])["err"]
    b = PM.pose_errors(table, r32.double(), t32.double(), *poses[2:], inp["labels"])["err"]
    assert torch.equal(a, b)


def test_padding_is_inert(g12, case_a):
    """class 2 has ONE point in a table padded to 1031 rows: whatever the padding holds, its rows' ad and proj are the same bits"""
    inp, table, poses, got0 = case_a
    assert table.pts.shape == (3, 1031, 3) and table.npts[2] == 1 and np.all(table.pts[2, 1:] == 0)
    _, table_p, _ = _case("A", g12, pad_value=1e3)
    assert np.all(table_p.pts[2, 1:] == 1e3) and np.all(table_p.pts[1, 257:] == 1e3)
    got1 = PM.pose_errors(table_p, *poses, inp["labels"])["err"].cpu().numpy()
    rows = inp["labels"] == 2
    assert rows.sum() == 22
    assert np.array_equal(got0[rows][:, [0, 3]], got1[rows][:, [0, 3]])
    assert np.array_equal(got0, got1)   # ... and every other row's too (class 1 is padded as well)
    _check_against_golden(got1, g12["A/err"], rows=rows, cols=(0, 3))


def test_two_calls_give_the_same_bits(case_b):
    inp, table, poses, got = case_b
    again = PM.pose_errors(table, *poses, inp["labels"])["err"].cpu().numpy()
    assert np.array_equal(got.view(np.int64), again.view(np.int64))


def _golden_flags(err, inp):
    d = inp["diameters"][inp["labels"]]
    ad, re_, te_, pr = err.T
    return np.stack([ad < 0.02 * d, ad < 0.05 * d, ad < 0.1 * d, (re_ < 2) & (te_ < 0.02), (re_ < 5) & (te_ < 0.05), (re_ < 10) & (te_ < 0.1),
                     re_ < 2, re_ < 5, re_ < 10, te_ < 0.02, te_ < 0.05, te_ < 0.1, pr < 2, pr < 5, pr < 10], axis=1)


def test_recall_table_equals_the_reference_evaluators(g12, case_a):
    inp, table, poses, _ = case_a
    want_rows = [str(r).split("\t") for r in g12["A/table"]]
    fl = _golden_flags(g12["A/err"], inp)
    want_hits = np.stack([fl[inp["labels"] == c].sum(0) for c in range(3)])
    rec = PM.PoseRecall(table, inp["obj_names"])
    for _ in range(2):
        lo = 0
        for n in (20, 40, 7):
            assert rec.update(*[p[lo:lo + n] for p in poses], inp["labels"][lo:lo + n]) is None
            lo += n
        assert lo == 67
        for c, cnt in inp["missing"].items():
            rec.add_missing(c, cnt)
        cnt = rec.counters()
        assert np.array_equal(cnt["hits"], want_hits), (cnt["hits"], want_hits)
        assert np.array_equal(cnt["err_cnt"], [23, 22, 22]) and np.array_equal(cnt["seen"], [26, 25, 24])
        rows = rec.summarize()
        print("\n".join("  ".join(r) for r in rows))
        assert rows == want_rows
        rec.reset()
        assert not rec.counters()["hits"].any() and not rec.counters()["seen"].any() and not rec.counters()["re_sum"].any()


def test_abi_argument_checks_return_before_any_launch(case_b):
    inp, table, poses, got = case_b
    lib, tb, N = cabi.load(), table.on(DEV), 3
    lab = torch.zeros(N, dtype=torch.int32, device=DEV)
    ok_host, bad_host = (C.c_int * N)(0, 0, 0), (C.c_int * N)(0, 1, 0)   # one class: label 1 >= C
    err = torch.full((N, 4), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(lib.gdrn_pose_metrics_workspace_bytes(N, table.n_max) // 8, dtype=torch.float64, device=DEV)
    p = cabi.ptr

    def call(pts=p(tb["pts"]), n=N, host=ok_host, npts=p(tb["npts"])):
        return lib.gdrn_pose_errors(p(poses[0]), p(poses[1]), p(poses[2]), p(poses[3]), p(poses[4]), p(lab), host, n, pts, npts, table.n_max,
                                    p(tb["is_sym"]), p(tb["sym"]), p(tb["nsym"]), table.k_max, 1, p(err), p(ws), None)

    assert call(pts=None) == -1 and call(npts=None) == -1 and call(n=0) == -1 and call(host=bad_host) == -1 and call(host=None) == -1
    torch.cuda.synchronize()
    assert bool((err == -7.0).all())   # nothing ran
    state = torch.zeros(19, dtype=torch.int64, device=DEV)
    f = state[17:].view(torch.float64)

    def acc(e=p(err), n=N, host=ok_host):
        return lib.gdrn_pose_recall_accumulate(e, p(lab), host, n, p(tb["diameter"]), 1, p(state[:15]), p(state[15:16]), p(f[:1]), p(f[1:]),
                                               p(state[16:17]), None)

    assert acc(e=None) == -1 and acc(n=0) == -1 and acc(host=bad_host) == -1
    torch.cuda.synchronize()
    assert not state.any()
    with pytest.raises(cabi.GdrnHipError):
        PM.pose_errors(table, *poses, [0, 1, 0])
    # and the valid call through the same raw entry point computes what the wrapper did
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(err.cpu().numpy(), got)
