"""GPU tests of the YCB-V score errors and recall counts (csrc/sixd_scores.hip through gdrnet_amd.sixd_scores) against golden G18: the reference's own
pose_error.add / adi / re_sym / te_sym / arp_2d_sym, pose_matching.match_poses and score.calc_recall on the fixture of
synth.make_sixd_score_inputs (tests/golden/make_golden_g18.py).

Bounds (sixd_host.check_errors): the ones the existing tests hold for the same quantities against the reference.  add / adi: 1e-9 relative + 1e-12
m, re_sym: 1e-9 relative from 0.1 degree and 1e-5 degree absolute below (tests/test_pose_metrics_gpu.py: fp64 on both sides, another summation
order over <= 8195 terms; arccos next to 1).  te_sym 1e-13 m, arp_2d_sym 1e-10 px (tests/test_bop_metrics_gpu.py, the symmetric pose walk: posed
coordinates <= 1.5 m and pixel coordinates <= 700 with a handful of roundings of 2^-53 relative each; a mean of such distances is no further off
than its terms).  The host restatement's own distance to the reference, measured on the CPU (tests/test_sixd_scores_cpu.py prints it): add / adi
1.4e-14 relative, re_sym 0, te_sym 3.0e-16 m, arp_2d_sym 7.1e-14 px.  Hit counters and recalls: exact.  The measured deviations are printed.

te_sym is the reference's function AS IT RUNS (a broadcast makes it the Frobenius norm of a 3 x 3 matrix, see sixd_scores.sym_errors): with the
identity only it is sqrt(3) times the plain te of pose_metrics, and that is what the consistency test below holds it to."""
import os

import numpy as np
import pytest
import torch

import sixd_host as SH
from gdrnet_amd import bop_metrics as BM
from gdrnet_amd import pose_metrics as PM
from gdrnet_amd import sixd_scores as SS
from gdrnet_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSES = ("R_est", "t_est", "R_gt", "t_gt", "K")


@pytest.fixture(scope="module")
def g18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g18_sixd_scores.npz")))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _errors(inp, table, rows=slice(None)):
    """(ad [n,2], sym [n,3]) device tensors of the rows"""
    P = [_dev(inp[k][rows]) for k in POSES]
    ad, sym = SS.ad_errors(table, *P[:4], inp["labels"][rows]), SS.sym_errors(table, *P, inp["labels"][rows])
    n = len(inp["labels"][rows])
    assert ad.dtype == sym.dtype == torch.float64 and tuple(ad.shape) == (n, 2) and tuple(sym.shape) == (n, 3) and ad.device.type == "cuda"
    return ad, sym


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def fix(g18):
    assert int(g18["sym/seed"]) == synth.SIXD_SCORE_SEEDS["sym"]
    inp = synth.make_sixd_score_inputs()
    table = BM.BopModelTable(inp["points"], inp["diameters"], inp["syms"])
    ad, sym = _errors(inp, table)
    torch.cuda.synchronize()
    return inp, table, ad, sym


def test_errors_against_the_reference(g18, fix):
    inp, _, ad, sym = fix
    ad, sym = ad.cpu().numpy(), sym.cpu().numpy()
    SH.check_errors(ad, sym, g18["sym/err"], "device")
    assert not ad[6].any() and not sym[6, 1:].any() and sym[6, 0] <= 1e-5   # est = gt, identity only: the same operations on both sides
    assert ad[0, 0] == 0.0 and ad[0, 1] == 0.0                              # est = gt: every point is its own nearest neighbour, at distance 0
    for i in (5, 8):                                                        # est = gt o S_k
        assert sym[i, 0] <= 1e-5 and sym[i, 2] <= 1e-10


def _recall(inp, table, ad, sym, splits):
    rec = SS.ScoreRecall(table, inp["obj_names"], inp["sym_classes"], inp["im_width"])
    lo = 0
    for k, n in enumerate(splits):
        lab = inp["labels"][lo:lo + n]
        assert rec.update(ad[lo:lo + n], sym[lo:lo + n], _dev(lab) if k % 2 else lab) is None   # labels from the host and from the device
        lo += n
    assert lo == len(inp["labels"])
    for c, n in inp["missing"].items():
        rec.add_missing(c, n)
    return rec


def test_hit_counters_recalls_and_tables(g18, fix):
    inp, table, ad, sym = fix
    rec = _recall(inp, table, ad, sym, (41,))
    cnt = rec.counters()
    want_hits = np.stack([g18["sym/match"][inp["labels"] == c].sum(0) for c in range(4)])
    assert cnt["hits"].dtype == np.int64 and np.array_equal(cnt["hits"], want_hits) and np.array_equal(cnt["seen"], g18["sym/targets"])
    assert np.array_equal(cnt["hits"] / cnt["seen"][:, None].astype(np.float64), g18["sym/recall"])
    tabs = rec.summarize()
    assert tabs == SH.tables(inp["obj_names"], want_hits, g18["sym/targets"])
    assert tabs["AUCad"][0] == ["objects", "AUCad_10"] and tabs["AUCad"][-1][0] == "Avg(4)" and [r[0] for r in tabs["reteS"][1:-1]] == inp["obj_names"]
    print("\n".join("  ".join(r) for name in ("AUCadd", "AUCadi", "AUCad", "ABSad", "reteS", "projS") for r in tabs[name]))
    # update in pieces (one of them a single row, one empty) adds up to the same counters
    parts = _recall(inp, table, ad, sym, (20, 1, 0, 13, 7)).counters()
    assert np.array_equal(parts["hits"], cnt["hits"]) and np.array_equal(parts["seen"], cnt["seen"])
    rec.reset()
    assert not rec.counters()["hits"].any() and not rec.counters()["seen"].any()


# points per class: 1 | one below, at and above the LDS tile of the adi loop | one below, at and above the point slab | two slabs and one point;
# transformations per class: 1 | one below, at and above the symmetry slab | 1 | two slabs | two slabs and one | 314
EDGE_POINTS = (1, SS.AD_TILE - 1, SS.AD_TILE, SS.AD_TILE + 1, SS.AD_SLAB - 1, SS.AD_SLAB, SS.AD_SLAB + 1, 2 * SS.AD_SLAB + 1, 5)
EDGE_SYMS = (1, SS.SYM_SLAB - 1, SS.SYM_SLAB, SS.SYM_SLAB + 1, 1, 2 * SS.SYM_SLAB, 2 * SS.SYM_SLAB + 1, 314, 2)


def _edge_inputs(N=67, seed=1801):
    """N rows cycling through the first eight classes of EDGE_POINTS / EDGE_SYMS (the ninth has no row), estimates 0 .. 12 degrees and 0 .. 4 cm off"""
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    C = len(EDGE_POINTS)
    points = [-0.1 + 0.2 * u(f"pts{c}", n, 3) for c, n in enumerate(EDGE_POINTS)]
    syms = []
    for c, s in enumerate(EDGE_SYMS):
        if s == 1:
            syms.append(None)
            continue
        axis = synth.hash_normal(seed, f"sax{c}", (1, 3))
        R = synth._axis_angle(np.repeat(axis / np.linalg.norm(axis), s, axis=0), 360.0 * np.arange(s) / s)
        syms.append((R, 0.02 * (u(f"st{c}", s, 3) - 0.5)))
    labels = np.arange(N, dtype=np.int64) % (C - 1)
    R_gt = synth._random_rotations(seed, "R_gt", N)
    axis = synth.hash_normal(seed, "axis", (N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    t_gt = np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)
    K = np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)
    K[:, :2, 2] += 6.0 * (u("c", N, 2) - 0.5)
    return dict(points=points, diameters=np.full(C, 0.2), syms=syms, labels=labels, R_gt=R_gt, t_gt=t_gt, K=K,
                R_est=synth._axis_angle(axis, 12.0 * u("ang", N) ** 2) @ R_gt, t_est=t_gt + 0.04 * u("off", N, 1) * (u("dir", N, 3) - 0.5),
                obj_names=[f"o{c}" for c in range(C)], sym_classes=(1, 2, 5, 7), im_width=640, missing={})


@pytest.fixture(scope="module")
def edge():
    inp = _edge_inputs()
    table = BM.BopModelTable(inp["points"], inp["diameters"], inp["syms"])
    assert table.n_max == 2 * SS.AD_SLAB + 1 and table.s_max == 314 and len(inp["labels"]) % 64 != 0 and 8 not in inp["labels"]
    ad, sym = _errors(inp, table)
    torch.cuda.synchronize()
    return inp, table, ad, sym, SH.errors_all(inp)


def test_edge_shapes_against_the_host_restatement(edge):
    inp, table, ad, sym, (host_ad, host_sym) = edge
    SH.check_errors(ad.cpu().numpy(), sym.cpu().numpy(), np.concatenate([host_ad, host_sym], axis=1), "edge shapes", mm=1.0)
    # N = 1 (every class in turn): the same bits as the row had in the batch -- a row's result does not depend on the other rows of the call
    for i in range(8):
        a1, s1 = _errors(inp, table, slice(i, i + 1))
        assert np.array_equal(_bits(a1), _bits(ad[i:i + 1])) and np.array_equal(_bits(s1), _bits(sym[i:i + 1])), i
    # N = 0: empty results, nothing launched, counters untouched
    a0, s0 = _errors(inp, table, slice(0, 0))
    assert tuple(a0.shape) == (0, 2) and tuple(s0.shape) == (0, 3)
    # the recall kernel on these rows (a ragged last wave, a class without a row): the counters are the decisions on the DEVICE's errors, exactly
    rec = _recall(inp, table, ad, sym, (67,))
    rec.update(a0, s0, [])
    want = SH.recall_counts(ad.cpu().numpy(), sym.cpu().numpy(), inp["labels"], inp["diameters"], inp["sym_classes"], 9)
    got = rec.counters()
    assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["seen"], want["seen"]) and got["seen"][8] == 0 and got["seen"].sum() == 67
    assert 0 < got["hits"].sum() < 51 * 67
    tabs = rec.summarize()
    assert tabs == SH.tables(inp["obj_names"], want["hits"], want["seen"]) and tabs["AUCadd"][-1][0] == "Avg(8)" and len(tabs["add"]) == 10


def test_padding_never_enters_a_result(fix, edge):
    for inp, table, ad, sym in (fix, edge[:4]):
        padded = BM.BopModelTable(inp["points"], inp["diameters"], inp["syms"], pad_value=np.nan, sym_pad_value=np.nan)
        assert np.isnan(padded.pts[0, len(inp["points"][0]):]).all() and np.isnan(padded.sym_R).any() and not np.isnan(table.pts).any()
        ad_p, sym_p = _errors(inp, padded)
        assert np.array_equal(_bits(ad), _bits(ad_p)) and np.array_equal(_bits(sym), _bits(sym_p))


def test_consistent_with_the_pose_metrics(fix):
    """ad_errors against pose_errors' "ad", bit for bit (the same tile loop, the same sums in the same order); sym_errors with identity-only sets
    against the plain re (bit for bit: R_gt times the identity is R_gt), proj (another formulation of the projection and another summation order:
    within the bound of the reference comparison) and te (te_sym as the reference runs it is sqrt(3) te with the identity only: 1e-13 m)"""
    inp, table, ad, _ = fix
    P = [_dev(inp[k]) for k in POSES]
    for sym_classes in ((0, 1, 3), (2,)):   # every class takes either branch once
        plain = PM.ModelTable(inp["points"], inp["diameters"], None, sym_classes)
        ref = PM.pose_errors(plain, *P, inp["labels"])["err"]
        rows = _dev(np.isin(inp["labels"], sym_classes))
        assert np.array_equal(_bits(ad[rows, 1]), _bits(ref[rows, 0])) and np.array_equal(_bits(ad[~rows, 0]), _bits(ref[~rows, 0]))
    ident = BM.BopModelTable(inp["points"], inp["diameters"], None)
    sym = SS.sym_errors(ident, *P, inp["labels"]).cpu().numpy()
    ref = ref.cpu().numpy()
    assert np.array_equal(sym[:, 0].view(np.uint64), ref[:, 1].view(np.uint64))
    d_te, d_pr = np.abs(sym[:, 1] - np.sqrt(3.0) * ref[:, 2]), np.abs(sym[:, 2] - ref[:, 3])
    print(f"identity-only sets: |te_sym - sqrt(3) te| worst {d_te.max():.3e} m (1e-13), |arp_2d_sym - proj| worst {d_pr.max():.3e} px (1e-10)")
    assert np.all(d_te <= 1e-13) and np.all(d_pr <= 1e-10)


def test_two_runs_give_the_same_bits_and_the_batch_split_does_not_matter(fix):
    inp, table, ad, sym = fix
    ad2, sym2 = _errors(inp, table)
    assert np.array_equal(_bits(ad), _bits(ad2)) and np.array_equal(_bits(sym), _bits(sym2))
    halves = [_errors(inp, table, r) for r in (slice(0, 20), slice(20, 41))]
    assert np.array_equal(_bits(ad), np.concatenate([_bits(h[0]) for h in halves]))
    assert np.array_equal(_bits(sym), np.concatenate([_bits(h[1]) for h in halves]))
    # fp32 poses: the same as handing over their exactly widened fp64 values
    P32 = [_dev(inp[k]).float() for k in POSES]
    a32, a64 = SS.ad_errors(table, *P32[:4], inp["labels"]), SS.ad_errors(table, *[p.double() for p in P32[:4]], inp["labels"])
    s32, s64 = SS.sym_errors(table, *P32, inp["labels"]), SS.sym_errors(table, *[p.double() for p in P32], inp["labels"])
    assert np.array_equal(_bits(a32), _bits(a64)) and np.array_equal(_bits(s32), _bits(s64))
