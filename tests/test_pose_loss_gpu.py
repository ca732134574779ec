"""Per-element tests (-m gpu) of pose_loss_kernel (csrc/pose_loss.hip) through gdrn_pose_loss against the fp64 autograd reference of
tests/pose_host.py (pinned on the CPU by tests/test_pose_host_cpu.py): the decode (train and test mode), the closest symmetric target, the
three pose losses (atomics and per-RoI rows), all three planes of dL/dfc, the weighted 16-bit gradient and the fc tail, at N <= 8 and
npts <= 700, every output pre-filled with NaN inside a guarded buffer.

Bounds (derived in tests/pose_host.py; no number from the kernel enters one): rot, trans and dfc[0] within 8 e32 + 16 * 2^-24 of the fp64
reference relative to the RoI row's largest magnitude, e32 the distance of the same oracle run in fp32; loss rows within the fp32 summation
bound; f2_out bit-exact, fc_w within the 256-term dot-product bound; signs, zeros and sentinels exact.  Every case prints a line
`pose-e32 <case> <output> e32 <e32> kernel <err> ratio <err / e32>`.

The 16-bit format is a property of the library build: this module tests libgdrn_hip.so; tests/test_pose_loss_fp16_gpu.py executes the
format-dependent cases of the same source on libgdrn_hip_f16.so."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_host as R
from gdrnet_amd import cabi
from gdrnet_amd.cabi import F32, PoseParams, check, ptr

pytestmark = pytest.mark.gpu

BF16 = globals().get("__HALF__", cabi.BF16)       # the 16-bit dtype code under test
IS_F16 = BF16 == cabi.F16
HT = torch.float16 if IS_F16 else torch.bfloat16
KIND = "fp16" if IS_F16 else "bf16"
ERR_ARG = -1
GENERIC = [(64, 257)] if IS_F16 else [(fs, npts) for fs in R.GENERIC_FS for npts in R.GENERIC_NPTS]   # (the decode does not depend on the format)


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hiputil

    cabi.load(BF16)
    return hiputil


_REF = {}


def refs(name, a):
    """(fp64 reference, fp32 oracle) of a seeded case, computed once"""
    if name not in _REF:
        _REF[name] = R.both(a)
    return _REF[name]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(x, y):
    return torch.equal(bits(x), bits(y))


class Launch:
    """one gdrn_pose_loss call on the arrays of `a`: every output a NaN-filled Guarded buffer.  rows / comb (= gw [3]) / tail (= the dict of
    pose_host.fc_tail_inputs) switch the ABI 5 outputs on; `over` overrides struct fields by name (None drops a pointer)."""

    OUTS = ("rot", "trans", "losses", "dfc", "vis", "loss_rows", "dfc_comb", "f2_out", "fc_w")

    def __init__(self, H, a, train=1, rows=False, comb=None, tail=None, fc_dev=None, over=None):
        lib = cabi.load(BF16)
        N, fs = a["fc"].shape
        npts = a["points"].shape[1]
        self.N, self.fs = N, fs
        dev = {k: H.f32_dev(v) for k, v in a.items() if k != "sym_count"}
        if fc_dev is not None:
            dev["fc"] = fc_dev
        G = H.Guarded
        self.o = dict(rot=G((N, 9), torch.float32), trans=G((N, 3), torch.float32), losses=G((3,), torch.float32), dfc=G((3, N, fs), torch.float32),
                      vis=G((N, 2), torch.float32), loss_rows=G((N, 4), torch.float32), dfc_comb=G((N, fs), HT), f2_out=G((N, 256), HT),
                      fc_w=G((N, fs), torch.float32))
        pp = PoseParams()
        pp.fc, pp.fs, pp.cams, pp.centers, pp.whs, pp.ratios, pp.extents = ptr(dev["fc"]), fs, ptr(dev["cams"]), ptr(dev["centers"]), ptr(dev["whs"]), ptr(dev["ratios"]), ptr(dev["extents"])
        pp.gt_rot, pp.gt_trans, pp.gt_trans_ratio, pp.points, pp.npts = ptr(dev["gt_rot"]), ptr(dev["gt_trans"]), ptr(dev["gt_trans_ratio"]), ptr(dev["points"]), npts
        if a.get("sym") is not None:
            dev["sym_count"] = torch.from_numpy(np.ascontiguousarray(a["sym_count"], dtype=np.int32)).to(H.DEV)
            pp.sym, pp.sym_count, pp.Kmax = ptr(dev["sym"]), ptr(dev["sym_count"]), a["sym"].shape[1]
        pp.N, pp.train = N, train
        pp.rot, pp.trans, pp.losses, pp.dfc, pp.vis = (ptr(self.o[k].t) for k in ("rot", "trans", "losses", "dfc", "vis"))
        if rows:
            pp.loss_rows = ptr(self.o["loss_rows"].t)
        if comb is not None:
            dev["gw"] = H.f32_dev(comb)
            pp.gw, pp.dfc_comb = ptr(dev["gw"]), ptr(self.o["dfc_comb"].t)
        if tail is not None:
            dev["ws"], dev["bias"], dev["b_rt"] = H.f32_dev(tail["ws"]), H.f32_dev(tail["bias"]), H.f32_dev(tail["b_rt"])
            dev["w_rt"] = H.to_dev(tail["w_rt"], BF16)
            pp.fc2_ws, pp.fc2_bias, pp.fc2_splits, pp.f2_out = ptr(dev["ws"]), ptr(dev["bias"]), tail["ws"].shape[0], ptr(self.o["f2_out"].t)
            pp.w_rt, pp.b_rt, pp.fc_w = ptr(dev["w_rt"]), ptr(dev["b_rt"]), ptr(self.o["fc_w"].t)
        for k, v in (over or {}).items():
            setattr(pp, k, v)
        self.dev = dev
        self.rc = lib.gdrn_pose_loss(C.byref(pp), H.stream())
        torch.cuda.synchronize()
        self.h = {k: self.o[k].host(k) for k in self.OUTS}

    def t(self, k):
        return self.o[k].t

    def untouched(self, *keys):
        return all(np.isnan(self.h[k]).all() for k in (keys or self.OUTS))


def report(name, key, e32, worst):
    print(f"pose-e32 {name} {key} e32 {e32:.3e} kernel {worst:.3e} ratio {worst / e32 if e32 > 0 else float('inf'):.2f}")


def check_decoded(name, got, r64, r32, key):
    ok, e32, worst = R.check_decode(got, r64, r32, key)
    report(name, key, e32, worst)
    assert ok, f"{name} {key}: error {worst:.3e} of the row maximum, bound 8 * {e32:.3e} + 16 * 2^-24 = {R.decode_bound(e32):.3e}"
    return R.decode_bound(e32) * R.rowmax(r64, key)[:, 0]


def check_train(H, name, a, L, totals=True):
    """every output of a train-mode launch (atomics mode, separate dfc planes) against the reference"""
    r64, r32 = refs(name, a)
    N, fs = L.N, L.fs
    assert L.rc == 0, L.rc
    dR = check_decoded(name, L.h["rot"], r64, r32, "rot")
    dt = check_decoded(name, L.h["trans"], r64, r32, "trans")
    check_decoded(name, L.h["dfc"][0][:, :9], r64, r32, "dfc0")
    H.assert_within(L.h["vis"], r64["vis"], R.vis_bound(a, r64, dR, dt), f"{name} vis")
    if totals:
        H.assert_within(L.h["losses"], r64["losses"], R.totals_bound(a, r64, r32), f"{name} loss totals")
    H.assert_same(L.h["dfc"][0][:, 9:], np.zeros((N, fs - 9)), f"{name} dfc[0] entries 9..fs-1")
    H.assert_same(L.h["dfc"][1:], R.f64(R.f32(r64["dfc"][1:])), f"{name} dfc[1], dfc[2]: sign / (2 N), sign / N, exact zeros")
    assert L.untouched("loss_rows", "dfc_comb", "f2_out", "fc_w")
    return r64, r32


# ---------------------------------------------------------------------------------------------- generic
@pytest.mark.parametrize("fs,npts", GENERIC)
def test_generic_every_output(H, fs, npts):
    """N = 5; fs = 9 (no zero entry), 12, 64, 256 (every thread writes); npts = 1 (three waves without a point), 63, 65, 256 (one full trip), 257
    (a remainder of one), 700 (a third trip)"""
    name = f"generic fs{fs} npts{npts}"
    a = R.generic(fs, npts)
    check_train(H, name, a, Launch(H, a))


@pytest.mark.parametrize("N", [1, 8])
def test_generic_one_and_eight_rois(H, N):
    a = R.generic(64, 257, N)
    check_train(H, f"generic N{N}", a, Launch(H, a))


# ---------------------------------------------------------------------------------------------- optical axis
@pytest.mark.parametrize("cam", ["lm", "origin"])
@pytest.mark.parametrize("z", R.AXIS_Z)
def test_optical_axis_train_and_test_mode(H, z, cam):
    """the object 0, 1e-5, 1e-3, 0.1, 1, 30 px off the optical axis (RoI 6: on it, with an axis-aligned rot6d whose allocentric matrix is exact)"""
    name = f"axis z{z} {cam}"
    a = R.optical_axis(z, R.LM_K if cam == "lm" else R.ORIGIN_K)
    check_train(H, name, a, Launch(H, a))
    T = Launch(H, a, train=0)
    assert T.rc == 0 and T.untouched("losses", "dfc", "loss_rows")
    t64, t32 = R.decode_test(a, torch.float64), R.decode_test(a, torch.float32)
    check_decoded(name + " test-mode", T.h["rot"], t64, t32, "rot")
    check_decoded(name + " test-mode", T.h["trans"], t64, t32, "trans")
    on_axis = np.flatnonzero((a["centers"] == a["cams"][:, :2, 2]).all(1))
    assert 0 in on_axis and R.AXIS_EXACT_ROI in on_axis
    # the identity branch (`if angle > 0` not taken): rot IS the allocentric matrix -- known exactly for the axis-aligned rot6d
    # (for the generic rot6d of RoI 0 the fp64 reference takes the branch too: held to its allocentric matrix by the bound above)
    H.assert_same(T.h["rot"][R.AXIS_EXACT_ROI].reshape(3, 3), R.AXIS_EXACT_ALLO, f"{name} test mode on the axis: rot != allocentric matrix")
    assert np.array_equal(t64["rot"][on_axis], t64["rot_allo"][on_axis])


# ---------------------------------------------------------------------------------------------- degenerate rot6d, sign edges
def test_degenerate_rot6d_forward_and_gradient(H):
    a = R.degenerate_rot6d()
    L = Launch(H, a)
    r64, _ = check_train(H, "degenerate", a, L)
    assert not np.isnan(L.h["dfc"]).any() and not np.isnan(L.h["rot"]).any()
    assert not r64["rot"][0].any() and not L.h["rot"][0].any()                       # a1 = 0: every column vanishes, exactly
    for n in (1, 2):                                                                 # a2 || a1: the columns y and z vanish (the allo -> ego turn mixes rows only)
        assert not L.h["rot"][n].reshape(3, 3)[:, 1:].any() and L.h["rot"][n].any()


@pytest.mark.parametrize("k", [6, 7, 8])
def test_sign_of_zero_in_the_regression_rows(H, k):
    """fc[k] bit-equal to its target: that unit gradient entry is exactly 0, the other two +-1 / (2 N), +-1 / N"""
    a = R.sign_edges(k)
    L = Launch(H, a)
    check_train(H, f"sign fc{k}", a, L)
    N = 3
    mag = {6: np.float32(1) / np.float32(2 * N), 7: np.float32(1) / np.float32(2 * N), 8: np.float32(1) / np.float32(N)}
    for j in (6, 7, 8):
        got = L.h["dfc"][1 if j < 8 else 2][:, j]
        if j == k:
            assert (got == 0).all(), got
        else:
            sg = np.sign(R.f64(a["fc"][:, j]) - R.f64(a["gt_trans_ratio"][:, j - 6]))
            assert (sg != 0).all() and np.array_equal(got, sg * float(mag[j])), (j, got)


def test_exact_match_has_zero_loss_and_zero_gradient(H):
    """prediction bit-equal to the chosen target (the returned rot fed back as gt_rot): d = w e - w g must be exactly 0 for every point, the
    reference's |.| has gradient 0 there: loss_PM_R == 0 and dfc[0] == 0.  Measured on an MI355X on this case (generic launch: loss 0.758, max
    |dfc[0]| 6.8e-2): with d = fma(w, e, -(w g)) and e, g contracted in two different orders loss 1.16e-8, max |dfc[0]| 3.0e-3 -- signs of rounding
    residues; with only the two products kept apart 3.4e-9 and 1.4e-3; with e and g as the same fma chain as well 0 and 0.  The test prints both
    launches' figures."""
    a = dict(R.exact_match_first())
    L1 = Launch(H, a)
    check_train(H, "exact first", a, L1)
    a["gt_rot"] = R.f32(L1.h["rot"]).reshape(-1, 3, 3)
    L2 = Launch(H, a)
    assert L2.rc == 0 and same_bits(L1.t("rot"), L2.t("rot"))
    print(f"exact match: loss_PM_R {L2.h['losses'][0]!r} max |dfc[0]| {np.abs(L2.h['dfc'][0]).max()!r} (first launch: loss {L1.h['losses'][0]!r}, max |dfc[0]| {np.abs(L1.h['dfc'][0]).max()!r})")
    assert L2.h["losses"][0] == 0.0, L2.h["losses"]
    H.assert_same(L2.h["dfc"][0], np.zeros_like(L2.h["dfc"][0]), "exact match dfc[0]")


# ---------------------------------------------------------------------------------------------- symmetry
def test_closest_symmetric_target(H):
    """sym_count = {0, 1, 3 = Kmax, 2}, NaN in the unused slots: two RoIs closest to a non-identity symmetry, one with symmetries closest to its
    plain gt; vis[:, 0] is the error against the unsymmetrised gt"""
    a = R.symmetry()
    r64, _ = check_train(H, "symmetry", a, Launch(H, a))
    assert tuple(r64["chosen_idx"]) == R.SYM_CHOICE and (r64["margin_deg"][1:] >= 1.0).all()


# ---------------------------------------------------------------------------------------------- row mode
def test_loss_rows_per_roi_and_run_to_run(H):
    name = "generic fs64 npts700"
    a = R.generic(64, 700)
    r64, r32 = refs(name, a)
    L1, L2 = Launch(H, a, rows=True), Launch(H, a, rows=True)
    assert L1.rc == 0 and L2.rc == 0
    H.assert_within(L1.h["loss_rows"][:, :3], r64["rows"], R.rows_bound(a, r64, r32), "loss rows")
    assert np.isnan(L1.h["loss_rows"][:, 3]).all() and L1.untouched("losses")
    for k in ("rot", "trans", "dfc", "vis"):
        assert same_bits(L1.t(k), L2.t(k)), k
    assert same_bits(L1.t("loss_rows")[:, :3], L2.t("loss_rows")[:, :3])
    A = Launch(H, a)                         # atomics mode: N fp32 adds in any order of the same rows
    rows = L1.h["loss_rows"][:, :3]
    H.assert_within(A.h["losses"], rows.sum(0), (5 - 1) * R.EPS32 * np.abs(rows).sum(0), "atomics totals against the sum of the rows")
    assert same_bits(A.t("dfc"), L1.t("dfc"))


# ---------------------------------------------------------------------------------------------- the weighted 16-bit gradient
def ulp16(x):
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -14.0) - 10.0) if IS_F16 else 2.0 ** (e - 7.0)


def test_dfc_comb_is_the_weighted_sum_at_the_storage_width(H):
    lib = cabi.load(BF16)
    name = "generic fs64 npts257"
    a = R.generic(64, 257)
    gw = R.f32([0.7, 1.3, -0.55])
    P = Launch(H, a)
    check_train(H, name, a, P)
    Cb = Launch(H, a, comb=gw)
    assert Cb.rc == 0 and Cb.untouched("dfc")        # (`dfc` is not written when dfc_comb is)
    d = R.f32(P.h["dfc"])
    want32 = ((gw[0] * d[0]).astype(np.float32) + (gw[1] * d[1]).astype(np.float32)).astype(np.float32)
    want32 = (want32 + (gw[2] * d[2]).astype(np.float32)).astype(np.float32)
    want = R.f64(R.round16(want32, KIND))
    H.assert_within(Cb.h["dfc_comb"], want, ulp16(want), "dfc_comb against round16(gw0 d0 + gw1 d1 + gw2 d2)", exact=(want == 0))
    # the separate path: dfc -> gdrn_combine3 -> cast, bit for bit
    comb32, comb16 = H.Guarded((5, 64), torch.float32), H.Guarded((5, 64), HT)
    check(lib.gdrn_combine3(ptr(P.t("dfc")), ptr(Cb.dev["gw"]), ptr(comb32.t), 5 * 64, H.stream()), "combine3")
    check(lib.gdrn_cast_from_f32(ptr(comb32.t), ptr(comb16.t), 5 * 64, BF16, H.stream()), "cast")
    comb16.host()
    assert same_bits(comb16.t, Cb.t("dfc_comb"))
    for k in ("rot", "trans", "vis"):
        assert same_bits(P.t(k), Cb.t(k)), k


# ---------------------------------------------------------------------------------------------- the fc tail
@pytest.mark.parametrize("splits", [1, 3])
def test_fc_tail_in_the_same_launch(H, splits):
    N, fs = 3, 64
    a = R.make_inputs(7100 + splits, N, fs, 65)
    tail = R.fc_tail_inputs(splits, N, fs, KIND)
    ref = R.fc_tail(tail["ws"], tail["bias"], tail["w_rt"], tail["b_rt"], KIND)
    assert (ref["pre"] == 0).any() and (ref["pre"] < 0).any() and (ref["pre"] > 0).any()
    nan_fc = H.nans((N, fs))                           # `fc` is not read with the tail
    L = Launch(H, a, rows=True, tail=tail, fc_dev=nan_fc)
    assert L.rc == 0
    H.assert_same(R.f32(L.h["f2_out"]).view(np.int32), ref["f2"].view(np.int32), "f2_out bits")
    H.assert_within(L.h["fc_w"][:, :9], ref["fc"], ref["fc_bound"], "fc_w")
    assert np.isnan(L.h["fc_w"][:, 9:]).all()
    assert not np.isnan(L.h["rot"]).any() and not np.isnan(L.h["dfc"][:, :, :9]).any()
    # the same launch without the tail, fed the nine outputs it wrote
    L2 = Launch(H, a, rows=True, fc_dev=L.t("fc_w"))
    assert L2.rc == 0 and L2.untouched("f2_out", "fc_w")
    for k in ("rot", "trans", "vis", "dfc"):
        assert same_bits(L.t(k), L2.t(k)), k
    assert same_bits(L.t("loss_rows")[:, :3], L2.t("loss_rows")[:, :3])


# ---------------------------------------------------------------------------------------------- test mode, rejections
def test_test_mode_leaves_the_train_outputs_alone(H):
    a = R.generic(64, 65)
    for rows in (False, True):
        L = Launch(H, a, train=0, rows=rows)
        assert L.rc == 0 and not np.isnan(L.h["rot"]).any() and not np.isnan(L.h["trans"]).any()
        assert L.untouched("losses", "dfc", "loss_rows", "dfc_comb"), {k: L.h[k] for k in ("losses", "loss_rows")}


def test_rejected_arguments_leave_every_output_untouched(H):
    a = R.generic(64, 65)
    a12 = R.generic(12, 65)
    gw = R.f32([1.0, 1.0, 1.0])
    tail = R.fc_tail_inputs(1, 5, 64, KIND)
    sym = dict(a, sym=np.full((5, 1, 3, 3), np.nan, dtype=np.float32), sym_count=np.zeros(5, dtype=np.int32))
    cases = {"fs = 8": (a12, {}, dict(fs=8)), "fs = 257": (a12, {}, dict(fs=257)), "N = 0": (a, {}, dict(N=0)),
             "train without points": (a, {}, dict(points=None)), "train with npts = 0": (a, {}, dict(npts=0)),
             "dfc_comb without gw": (a, dict(comb=gw), dict(gw=None)), "fc2_ws without its bias": (a, dict(tail=tail), dict(fc2_bias=None)),
             "sym with Kmax = 0": (sym, {}, dict(Kmax=0)), "sym with Kmax = -1": (sym, {}, dict(Kmax=-1))}
    for what, (arr, kw, over) in cases.items():
        L = Launch(H, arr, over=over, **kw)
        assert L.rc == ERR_ARG, (what, L.rc)
        assert L.untouched(), what
    assert Launch(H, sym).rc == 0
