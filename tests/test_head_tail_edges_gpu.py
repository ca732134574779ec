"""Per-element tests (-m gpu) of the head-tail, map-loss and fused head-conv kernels of csrc/head_tail.hip and csrc/head_conv.hip at their launch edges, against the
fp64 yardstick of tests/head_host.py (pinned on the CPU by tests/test_head_host_cpu.py):

  (a) the 64-region kernels head_tail_fwd64<T, LOSS> / head_tail_bwd64 through gdrn_head_tail_fwd, gdrn_head_tail_loss_fwd (atomics and partial
      rows) and gdrn_head_tail_bwd, up to M = 65583 pixels (a second grid-stride pass of 47 pixels);
  (b) the generic kernels head_tail_fwd / map_loss_fwd / head_tail_bwd at nreg in {1, 5, 16, 17, 32, 63} and at 64 regions on 69-wide rows, up
      to M = 32800 (past the 2048-workgroup cap of map_loss_fwd_kernel), plus gdrn_map_loss_fwd on its own;
  (c) the fused kernels head_conv_tail64<T, LOSS> and head_out_dgrad64 (16-bit only) with idle waves, ngroups % 4 != 0, a RoI change inside a
      workgroup and a second, prefetched group per wave; the shapes they refuse;
  (d) the row-stride checks of gdrn_head_tail_bwd and gdrn_map_loss_fwd;
  the three finalizers behind every loss run.

Every output is a NaN-filled hiputil.Guarded buffer (partial rows: one NaN guard row), every comparison goes through hiputil.assert_within /
assert_same, columns a kernel must not read hold a large finite value.  The seeded rows (head_host.make_inputs) hold near-one-hot rows with a
spread of 60, all-equal rows, offsets of +80, entries of -80, targets 0 / 1 / nreg - 1 / nreg, masked-out pixels and exact L1 ties.  Bounds are
derived in tests/head_host.py; no number from a kernel enters one.  Every numeric check prints a line
`head-e32 <case> <output> e32 <e32> kernel <err> ratio <err / bound>`.

The 16-bit format is a property of the library build: this module tests libgdrn_hip.so; tests/test_head_tail_edges_fp16_gpu.py executes the
format-dependent cases of the same source on libgdrn_hip_f16.so."""

import numpy as np
import pytest
import torch

import head_host as R
import norm_host as NH
from gdrnet_amd import cabi
from gdrnet_amd.cabi import F32, check, ptr

pytestmark = pytest.mark.gpu

BF16 = globals().get("__HALF__", cabi.BF16)       # the 16-bit dtype code under test
IS_F16 = BF16 == cabi.F16
HT = torch.float16 if IS_F16 else torch.bfloat16
KIND = "fp16" if IS_F16 else "bf16"
DTS = [BF16] if IS_F16 else [F32, BF16]           # (the fp32 cases do not depend on the 16-bit format)
ERR_ARG, ERR_SHAPE = -1, -2
PREZ, ROWS = cabi.PREZEROED, cabi.ACC_ROWS
MASKED = (1, 16, True)                            # the all-masked batch: den clamps to 1, the cross entropy is 16 ln(nreg + 1)


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hiputil

    cabi.load(BF16)
    return hiputil


def kind_of(dt):
    return "fp32" if dt == F32 else KIND


def tt(dt):
    return torch.float32 if dt == F32 else HT


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.int64))


def same_bits(x, y):
    torch.cuda.synchronize()
    return torch.equal(bits(x), bits(y))


def report(case, output, e32, got, ref, bnd):
    got, ref, bnd = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.broadcast_to(np.asarray(bnd, dtype=np.float64), np.shape(ref))
    err = np.abs(got - ref)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    print(f"head-e32 {case} {output} e32 {e32:.3e} kernel {float(err.max()) if err.size else 0.0:.3e} ratio {ratio:.3f}")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- device copies of a case
class Dev:
    """the device arrays of a head_host.Case; head rows of stride hs whose columns >= nreg + 5 hold zeros or (poison) 1e30"""

    def __init__(self, H, c):
        a = self.a = c.a
        self.H, self.c = H, c
        self.N, self.HW, self.M, self.nreg, self.C = a["N"], a["HW"], a["M"], a["nreg"], a["nreg"] + 5
        self.coord2d, self.extents, self.gt_xyz = H.f32_dev(a["coord2d"]), H.f32_dev(a["extents"]), H.f32_dev(a["gt_xyz"])
        self.mvis, self.mtr, self.gw = H.f32_dev(a["mvis"]), H.f32_dev(a["mtr"]), H.f32_dev(a["gw"])
        self.greg = torch.from_numpy(a["gt_region"]).to(H.DEV)
        self._heads = {}

    def head(self, hs, poison=False):
        if (hs, poison) not in self._heads:
            h = np.full((self.M, hs), 1e30 if poison else 0.0, dtype=np.float32)
            h[:, :self.C] = self.a["head"][:, :self.C]
            self._heads[(hs, poison)] = self.H.f32_dev(h)
        return self._heads[(hs, poison)]

    def d_pnp(self, pcs, dt, poison=False):
        """channels 3, 4 (loaded, never used) and the pad hold zeros, or the poison value"""
        d = np.full((self.M, pcs), R.POISON[kind_of(dt)] if poison else 0.0)
        d[:, :3], d[:, 5:self.C] = self.a["d_pnp"][:, :3], self.a["d_pnp"][:, 5:self.C]
        return self.H.to_dev(NH.store(d, kind_of(dt)), dt)


_DEV = {}


def dev_case(H, N, HW, nreg, dt, masked=False):
    key = (N, HW, nreg, kind_of(dt), masked)
    if key not in _DEV:
        _DEV[key] = Dev(H, R.case(*key))
    return _DEV[key]


# ---------------------------------------------------------------------------------------------- launches
def fwd(H, d, dt, hs, pcs, flags=0, poison=False, loss=None):
    """loss: None = gdrn_head_tail_fwd; "atomics" / "rows" = gdrn_head_tail_loss_fwd.  Returns (pnp Guarded, acc Guarded | None, nrows)"""
    lib = cabi.load(BF16)
    pnp = H.Guarded((d.M, pcs), tt(dt))
    hd = d.head(hs, poison)
    if loss is None:
        check(lib.gdrn_head_tail_fwd(ptr(hd), hs, ptr(d.coord2d), ptr(d.extents), ptr(pnp.t), pcs, d.N, d.HW, d.nreg, dt | flags, H.stream()), "head_tail_fwd")
        return pnp, None, 0
    nrows = int(lib.gdrn_head_tail_loss_rows(d.N, d.HW, d.nreg, hs, pcs)) if loss == "rows" else 0
    acc = H.Guarded((1 + nrows, 8), torch.float64)
    check(lib.gdrn_head_tail_loss_fwd(ptr(hd), hs, ptr(d.coord2d), ptr(d.extents), ptr(pnp.t), pcs, ptr(d.gt_xyz), ptr(d.mvis), ptr(d.mtr), ptr(d.greg),
                                      ptr(acc.t), d.N, d.HW, d.nreg, dt | flags | (ROWS if loss == "rows" else 0), H.stream()), "head_tail_loss_fwd")
    return pnp, acc, nrows


def bwd(H, d, dt, hs, pnp_t, dpnp_t, pcs, acc_t, dcs, flags=0, poison=False):
    lib = cabi.load(BF16)
    dh = H.Guarded((d.M, dcs), tt(dt))
    check(lib.gdrn_head_tail_bwd(ptr(d.head(hs, poison)), hs, ptr(pnp_t), ptr(dpnp_t), pcs, ptr(d.extents), ptr(d.gt_xyz), ptr(d.mvis), ptr(d.mtr), ptr(d.greg),
                                 ptr(acc_t), ptr(d.gw), ptr(dh.t), dcs, d.N, d.HW, d.nreg, dt | flags, H.stream()), "head_tail_bwd")
    return dh


def finalize(H, d, acc, nrows):
    """the five map losses out of the finalizer that fits (atomics: gdrn_map_loss_finalize; rows: gdrn_map_loss_finalize_rows, then once more
    through gdrn_loss_finalize with pose rows and weights).  Returns (losses [8] host, totals [8] host)"""
    lib = cabi.load(BF16)
    ls = H.Guarded((8,), torch.float32)
    if nrows == 0:
        check(lib.gdrn_map_loss_finalize(ptr(acc.t), d.N, d.HW, ptr(ls.t), H.stream()), "map_loss_finalize")
        return ls.host("losses"), acc.host("acc")[0]
    check(lib.gdrn_map_loss_finalize_rows(ptr(acc.t), nrows, d.N, d.HW, ptr(ls.t), H.stream()), "map_loss_finalize_rows")
    l1, a1 = ls.host("losses"), acc.host("acc")
    assert not np.isnan(a1[:1 + nrows, :6]).any(), "a partial row was not written"
    rg = np.random.default_rng(5)
    pose, w = R.f32(rg.random((d.N, 4))), R.f32(0.5 + rg.random(8))
    pose_d, w_d = H.f32_dev(pose), H.f32_dev(w)
    ls2, wt = H.Guarded((8,), torch.float32), H.Guarded((8,), torch.float32)
    check(lib.gdrn_loss_finalize(ptr(acc.t), nrows, d.N, d.HW, ptr(pose_d), ptr(ls2.t), ptr(w_d), ptr(wt.t), H.stream()), "loss_finalize")
    l2, w2 = ls2.host("losses"), wt.host("weighted")
    H.assert_same(l2[:5], l1[:5], "gdrn_loss_finalize against gdrn_map_loss_finalize_rows")
    want = np.zeros(3, dtype=np.float32)
    for n in range(d.N):
        want = (want + pose[n, :3]).astype(np.float32)            # fp32, RoI order
    H.assert_same(l2[5:], want.astype(np.float64), "pose losses from the per-RoI rows")
    H.assert_same(w2, (l2.astype(np.float32) * w).astype(np.float64), "weighted losses")
    H.assert_same(acc.host("acc")[0], a1[0], "totals of the second finalize")
    return l1, a1[0]


# ---------------------------------------------------------------------------------------------- checks
def check_pnp(H, name, c, got, kind, pcs, prez, fast):
    C = c.nreg + 5
    b, e32 = R.tail_bound(c.p64, c.p32, c.mag_xyz, kind)
    ref = c.p64.copy()
    ref[:, 3:5] = NH.store(ref[:, 3:5], kind)                     # bit-exact copies of coord2d
    exact = np.zeros(ref.shape, dtype=bool)
    exact[:, 3:5] = True
    report(name, "pnp.xyz", 0.0, got[:, :3], ref[:, :3], b[:, :3])
    report(name, "pnp.softmax", e32, got[:, 5:C], ref[:, 5:], b[:, 5:])
    H.assert_within(got[:, :C], ref, b, f"{name} pnp", exact=exact)
    if c.nreg == 1:
        H.assert_same(got[:, 5], np.ones(c.M), f"{name}: a softmax over one class")
    kept = ((72 if fast else C) if prez else pcs)                 # GDRN_PREZEROED: the pad behind the last written group is the caller's
    H.assert_same(got[:, C:kept], np.zeros((c.M, kept - C)), f"{name} pnp pad")
    assert np.isnan(got[:, kept:]).all(), f"{name}: pad channels written under GDRN_PREZEROED"


def check_totals(H, name, c, tot8, ls, carry):
    tb, e32 = R.totals_bound(c.t64, c.t32, c.a_ce, carry)
    for k, out in enumerate(("sum.x", "sum.y", "sum.z", "sum.mask", "sum.ce")):
        report(name, out, e32 if k == 4 else 0.0, tot8[k], c.tot[k], tb[k])
    H.assert_within(tot8[:6], c.tot, tb, f"{name} totals", exact=np.arange(6) == 5)
    H.assert_same(tot8[6:], np.zeros(2), f"{name} acc[6..7]")
    lb = R.losses_bound(tb, c.tot, c.M)
    report(name, "losses", e32, ls[:5], c.losses, lb)
    H.assert_within(ls[:5], c.losses, lb, f"{name} losses")
    assert np.isnan(ls[5:]).all(), f"{name}: losses[5..7] written without pose rows"


def check_bwd(H, name, c, got, refs, kind, with_dpnp, dcs, prez, fast):
    C = c.nreg + 5
    r64, r32 = refs
    bb, e32 = R.tail_bwd_bound(r64, r32, kind, with_dpnp)
    a = c.a
    ex = R.tail_bwd_exact(a["head"], a["gt_xyz"], a["mvis"], a["mtr"], a["gw"], c.den, c.HW, kind)
    ref = r64["d"].copy()
    exact = np.zeros(ref.shape, dtype=bool)
    ref[:, 0], exact[:, 0] = ex[:, 0], True                       # a sign times a constant
    if not with_dpnp:
        ref[:, 1:4], exact[:, 1:4] = ex[:, 1:], True
        exact[a["mvis"] == 0, 4:] = True                          # a masked pixel's cross-entropy gradient is exactly 0
    tag = "d_head" if with_dpnp else "d_head.loss-only"
    report(name, tag + ".classes", e32, got[:, 4:C], ref[:, 4:], bb[:, 4:])
    if with_dpnp:
        report(name, tag + ".xyz", 0.0, got[:, 1:4], ref[:, 1:4], bb[:, 1:4])
    H.assert_within(got[:, :C], ref, bb, f"{name} {tag}", exact=exact)
    kept = ((72 if fast else C) if prez else dcs)
    H.assert_same(got[:, C:kept], np.zeros((c.M, kept - C)), f"{name} d_head pad")
    assert np.isnan(got[:, kept:]).all(), f"{name}: d_head pad channels written under GDRN_PREZEROED"


_BWD_REF = {}


def bwd_refs(c, key, pnp_host):
    """fp64 / fp32 replays from the stored tail, once per case and kernel path; a later stride set must have produced the same tail"""
    if key not in _BWD_REF:
        C = c.nreg + 5
        _BWD_REF[key] = (pnp_host[:, :C].copy(), (c.bwd(pnp_host, True), c.bwd(pnp_host, True, np.float32)), (c.bwd(None, False), c.bwd(None, False, np.float32)))
    return _BWD_REF[key]


def tail_roundtrip(H, name, N, HW, nreg, dt, hs, pcs, dcs, prez, masked=False):
    """every check of (a) / (b) at one stride set"""
    lib = cabi.load(BF16)
    d = dev_case(H, N, HW, nreg, dt, masked)
    c, kind, M, C = d.c, kind_of(dt), N * HW, nreg + 5
    ok64 = lambda s1, s2: nreg == 64 and s1 >= 72 and s1 % 4 == 0 and s2 >= 72 and s2 % 4 == 0    # the library's fast-path condition
    fast, fast_b0 = ok64(hs, pcs), ok64(hs, dcs)                  # forward; backward without d_pnp_in (pcs is not used then)
    fast_b = fast_b0 and fast                                     # backward with d_pnp_in
    flags = PREZ if prez else 0
    cap = 4096 if fast else 2048
    name = f"{name} {kind} N{N} HW{HW}{' masked' if masked else ''} nreg{nreg} hs{hs} pcs{pcs} dcs{dcs}{' prez' if prez else ''}"
    # forward: eval entry point, then the train entry point with atomics and with partial rows (twice)
    pnp, _, _ = fwd(H, d, dt, hs, pcs, flags)
    got = pnp.host("pnp")
    check_pnp(H, name, c, got, kind, pcs, prez, fast)
    pnp_a, acc_a, _ = fwd(H, d, dt, hs, pcs, flags, loss="atomics")
    assert same_bits(pnp_a.buf, pnp.buf), f"{name}: the train entry point writes another tail"
    carry = cdiv(M, 16 * min(cdiv(M, 16), cap))
    ls, tot = finalize(H, d, acc_a, 0)
    check_totals(H, name + " atomics", c, tot, ls, carry)
    nr = int(lib.gdrn_head_tail_loss_rows(N, HW, nreg, hs, pcs))
    assert nr == min(cdiv(M, 16), cap), (name, nr)
    runs = []
    for rep in range(2):
        pnp_r, acc_r, nrows = fwd(H, d, dt, hs, pcs, flags, loss="rows")
        assert nrows == nr and same_bits(pnp_r.buf, pnp.buf)
        ls_r, tot_r = finalize(H, d, acc_r, nrows)
        runs.append((ls_r, tot_r, acc_r))
    check_totals(H, name + " rows", c, runs[0][1], runs[0][0], carry)
    H.assert_same(runs[1][1], runs[0][1], f"{name}: partial-row totals of two runs")
    H.assert_same(runs[1][0][:5], runs[0][0][:5], f"{name}: losses of two runs")
    if masked:
        assert c.den == 1.0 and abs(c.tot[4] - 16 * np.log(nreg + 1.0)) < 1e-12
    # head columns behind the row poisoned: nothing may change
    pnp_p, acc_p, _ = fwd(H, d, dt, hs, pcs, flags, poison=True, loss="rows")
    assert same_bits(pnp_p.buf, pnp.buf), f"{name}: the tail reads head columns >= {C}"
    assert same_bits(acc_p.t[1:], runs[0][2].t[1:]), f"{name}: the loss sums read head columns >= {C}"
    if not fast:                                                  # gdrn_map_loss_fwd on its own (always the generic kernel, atomics)
        acc_m = H.Guarded((1, 8), torch.float64)
        check(lib.gdrn_map_loss_fwd(ptr(d.head(hs)), hs, ptr(d.gt_xyz), ptr(d.mvis), ptr(d.mtr), ptr(d.greg), N, HW, nreg, ptr(acc_m.t), H.stream()), "map_loss_fwd")
        ls_m, tot_m = finalize(H, d, acc_m, 0)
        check_totals(H, name + " map_loss_fwd", c, tot_m, ls_m, carry)
    # backward: from the tail the kernel stored, with and without d_pnp; poisoned d_pnp channels 3, 4 and pad; poisoned head columns
    first, with_refs, loss_refs = bwd_refs(c, (id(c), fast), got)
    H.assert_same(got[:, :C], first, f"{name}: the tail depends on the strides")
    acc8 = acc_a.t[0]
    dh = bwd(H, d, dt, hs, pnp.t, d.d_pnp(pcs, dt), pcs, acc8, dcs, flags)
    check_bwd(H, name, c, dh.host("d_head"), with_refs, kind, True, dcs, prez, fast_b)
    dh_p = bwd(H, d, dt, hs, pnp.t, d.d_pnp(pcs, dt, poison=True), pcs, acc8, dcs, flags, poison=True)
    assert same_bits(dh_p.buf, dh.buf), f"{name}: d_head depends on d_pnp channels 3, 4, a pad column, or head columns >= {C}"
    dh0 = bwd(H, d, dt, hs, None, None, pcs, acc8, dcs, flags)
    check_bwd(H, name, c, dh0.host("d_head"), loss_refs, kind, False, dcs, prez, fast_b0)
    dh1 = bwd(H, d, dt, hs, pnp.t, None, pcs, runs[0][2].t[0], dcs, flags)    # pnp_in without d_pnp_in is not read; totals from the rows run
    assert same_bits(dh1.buf, dh0.buf)


# ---------------------------------------------------------------------------------------------- (a) the 64-region kernels
STRIDES_ALL = [(hs, pcs, dcs, pz) for hs in (72, 76) for pcs in (72, 76, 128) for dcs in (72, 76, 128) for pz in (False, True)]
STRIDES_BIG = [(72, 72, 72, False), (76, 128, 76, True), (72, 76, 128, True)]      # every value of every stride once at the large shapes
FAST = [(N, HW, False) for (N, HW) in R.FAST_SHAPES] + [MASKED]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,HW,masked", FAST)
def test_fast_path_every_output_per_element(H, dt, N, HW, masked):
    for (hs, pcs, dcs, pz) in (STRIDES_ALL if N * HW <= 32 else STRIDES_BIG):
        tail_roundtrip(H, "fast", N, HW, 64, dt, hs, pcs, dcs, pz, masked)


# ---------------------------------------------------------------------------------------------- (b) the generic kernels
GENERIC = [(N, HW, False) for (N, HW) in R.GENERIC_SHAPES] + [MASKED]
GENERIC_NREG = ([17, 64] if IS_F16 else R.GENERIC_NREG + [64])   # 64: hs = pcs = dcs = 69, the unaligned rows that fall off the fast path


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nreg", GENERIC_NREG)
@pytest.mark.parametrize("N,HW,masked", GENERIC)
def test_generic_path_every_output_per_element(H, dt, nreg, N, HW, masked):
    C = nreg + 5
    sets = [(C, C, C, False), (C, C, C, True), (C + 3, C + 4, C + 2, False), (C + 3, C + 4, C + 18, True)]
    if nreg == 64:
        sets = [(69, 69, 69, False), (69, 69, 69, True), (72, 70, 69, False), (71, 72, 73, True), (72, 72, 70, False)]   # each one fails ht64_ok somewhere
    if N * HW > 4096:
        sets = sets[::2] if nreg != 64 else sets[:2]
    for (hs, pcs, dcs, pz) in sets:
        tail_roundtrip(H, "generic", N, HW, nreg, dt, hs, pcs, dcs, pz, masked)


# ---------------------------------------------------------------------------------------------- (c) the fused kernels (16-bit only)
FUSED_STRIDES = [dict(x_cs=256, w_rows=69, hs=72, pcs=72), dict(x_cs=264, w_rows=128, hs=76, pcs=128), dict(x_cs=256, w_rows=128, hs=72, pcs=128)]


def fused_inputs(H, N, HW, x_cs, w_rows):
    M = N * HW
    x, w, bias = R.conv_inputs(R.seed_of(N, HW, 64) + 1, M, KIND, x_cs, w_rows)
    return x, w, bias, H.to_dev(x, BF16), H.to_dev(w, BF16), H.f32_dev(bias)


@pytest.mark.parametrize("N,HW", R.FUSED_SHAPES)
def test_fused_conv_tail_per_element(H, N, HW):
    lib, st = cabi.load(BF16), H.stream()
    M, ng = N * HW, N * HW // 16
    d = dev_case(H, N, HW, 64, BF16)
    a = d.a
    for s in (FUSED_STRIDES if M <= 4096 else FUSED_STRIDES[1:2]):
        x_cs, w_rows, hs, pcs = s["x_cs"], s["w_rows"], s["hs"], s["pcs"]
        name = f"fused {KIND} N{N} HW{HW} x_cs{x_cs} w_rows{w_rows} hs{hs} pcs{pcs}"
        x, w, bias, xd, wd, bd = fused_inputs(H, N, HW, x_cs, w_rows)
        head, pnp = H.Guarded((M, hs), torch.float32), H.Guarded((M, pcs), HT)
        check(lib.gdrn_head_conv_tail_fwd(ptr(xd), x_cs, ptr(wd), w_rows, ptr(bd), ptr(d.coord2d), ptr(d.extents), ptr(head.t), hs, ptr(pnp.t), pcs, N, HW, 64, BF16, st),
              "head_conv_tail_fwd")
        lg, got = head.host("logits"), pnp.host("pnp")
        y, _, yb = R.conv_logits(x, w, bias)
        report(name, "logits", 0.0, lg[:, :69], y, yb)
        H.assert_within(lg[:, :69], y, yb, f"{name} logits")
        H.assert_same(lg[:, 69:72], np.zeros((M, 3)), f"{name} logit columns 69..71")
        assert np.isnan(lg[:, 72:]).all() and np.isnan(got[:, 72:]).all(), f"{name}: columns >= 72 are the caller's"
        # the tail and the loss sums against the fp64 tail of the logits the kernel itself wrote: the GEMM's rounding stays out of their bounds
        lg32 = R.f32(lg[:, :69])
        p64, p32 = (R.tail(lg32, a["coord2d"], a["extents"], 64, dt) for dt in (np.float64, np.float32))
        b, e32 = R.tail_bound(p64, p32, R.tail_mag(lg32, a["extents"], HW), KIND)
        ref = p64.copy()
        ref[:, 3:5] = NH.store(ref[:, 3:5], KIND)
        exact = np.zeros(ref.shape, dtype=bool)
        exact[:, 3:5] = True
        report(name, "fused.pnp.softmax", e32, got[:, 5:69], ref[:, 5:], b[:, 5:])
        H.assert_within(got[:, :69], ref, b, f"{name} pnp", exact=exact)
        H.assert_same(got[:, 69:72], np.zeros((M, 3)), f"{name} pnp channels 69..71")
        pnp2 = H.Guarded((M, pcs), HT)
        check(lib.gdrn_head_conv_tail_fwd(ptr(xd), x_cs, ptr(wd), w_rows, ptr(bd), ptr(d.coord2d), ptr(d.extents), None, hs, ptr(pnp2.t), pcs, N, HW, 64, BF16, st),
              "head_conv_tail_fwd (no logits)")
        assert same_bits(pnp2.buf, pnp.buf), f"{name}: head = NULL changes the tail"
        # train variant: the same logits and tail, the six sums as one partial row per workgroup
        nrows = int(lib.gdrn_head_conv_tail_loss_rows(N, HW))
        assert nrows == min(cdiv(ng, 4), 1024)
        tot64, t64, a_ce = R.map_sums(lg32, a["gt_xyz"], a["mvis"], a["mtr"], a["gt_region"], 64)
        _, t32, _ = R.map_sums(lg32, a["gt_xyz"], a["mvis"], a["mtr"], a["gt_region"], 64, np.float32)
        tb, e32c = R.totals_bound(t64, t32, a_ce, 4 * cdiv(ng, 4 * nrows))
        runs = []
        for rep in range(2):
            head3, pnp3, acc = H.Guarded((M, hs), torch.float32), H.Guarded((M, pcs), HT), H.Guarded((1 + nrows, 8), torch.float64)
            check(lib.gdrn_head_conv_tail_loss_fwd(ptr(xd), x_cs, ptr(wd), w_rows, ptr(bd), ptr(d.coord2d), ptr(d.extents), ptr(head3.t), hs, ptr(pnp3.t), pcs,
                                                   ptr(d.gt_xyz), ptr(d.mvis), ptr(d.mtr), ptr(d.greg), ptr(acc.t), N, HW, 64, BF16, st), "head_conv_tail_loss_fwd")
            assert same_bits(head3.buf, head.buf) and same_bits(pnp3.buf, pnp.buf), f"{name}: the train variant writes other logits or another tail"
            ls = H.Guarded((8,), torch.float32)
            check(lib.gdrn_map_loss_finalize_rows(ptr(acc.t), nrows, N, HW, ptr(ls.t), st), "map_loss_finalize_rows")
            ah = acc.host("acc")
            assert not np.isnan(ah[:, :6]).any(), f"{name}: a partial row was not written"
            runs.append((ah[0], ls.host("losses")))
        for k, out in enumerate(("sum.x", "sum.y", "sum.z", "sum.mask", "sum.ce")):
            report(name, "fused." + out, e32c if k == 4 else 0.0, runs[0][0][k], tot64[k], tb[k])
        H.assert_within(runs[0][0][:6], tot64, tb, f"{name} totals", exact=np.arange(6) == 5)
        H.assert_same(runs[0][0][6:], np.zeros(2), f"{name} acc[6..7]")
        H.assert_within(runs[0][1][:5], R.losses(tot64, M), R.losses_bound(tb, tot64, M), f"{name} losses")
        H.assert_same(runs[1][0], runs[0][0], f"{name}: totals of two runs")
        H.assert_same(runs[1][1][:5], runs[0][1][:5], f"{name}: losses of two runs")


DGRAD_STRIDES = [dict(dy_cs=96, wd_cs=96, raw_cs=256, dx_cs=256), dict(dy_cs=128, wd_cs=96, raw_cs=264, dx_cs=264), dict(dy_cs=96, wd_cs=128, raw_cs=256, dx_cs=264)]


@pytest.mark.parametrize("N,HW", R.DGRAD_SHAPES)
def test_fused_out_dgrad_per_element(H, N, HW):
    lib, st = cabi.load(BF16), H.stream()
    M, ng = N * HW, N * HW // 16
    nrows = int(lib.gdrn_head_out_dgrad_rows(N, HW))
    assert nrows == min(cdiv(ng, 4), 512)
    for s in (DGRAD_STRIDES if M <= 4096 else DGRAD_STRIDES[1:2]):
        dy_cs, wd_cs, raw_cs, dx_cs = s["dy_cs"], s["wd_cs"], s["raw_cs"], s["dx_cs"]
        name = f"dgrad {KIND} N{N} HW{HW} dy_cs{dy_cs} wd_cs{wd_cs} raw_cs{raw_cs} dx_cs{dx_cs}"
        i = R.dgrad_inputs(R.seed_of(N, HW, 64), M, KIND, dy_cs, wd_cs, raw_cs)
        r = R.out_dgrad(i["dy"], i["wd"], i["raw"], i["mean"], i["invstd"], i["scale"], i["shift"], terms=2 * cdiv(ng, 4 * nrows))
        dev = {k: (H.to_dev(v, BF16) if k in ("dy", "wd", "raw") else H.f32_dev(v)) for k, v in i.items()}
        dx, rows = H.Guarded((M, dx_cs), HT), H.rows_buf(nrows, 256)
        check(lib.gdrn_head_out_dgrad(ptr(dev["dy"]), dy_cs, ptr(dev["wd"]), wd_cs, ptr(dev["raw"]), raw_cs, ptr(dev["mean"]), ptr(dev["invstd"]), ptr(dev["scale"]),
                                      ptr(dev["shift"]), ptr(dx.t), dx_cs, ptr(rows), N, HW, BF16, st), "head_out_dgrad")
        got = dx.host("dx")
        assert np.isnan(got[:, 256:]).all(), f"{name}: dx columns >= 256 are the caller's"
        ok = ~r["marginal"]                                       # (mask argument within rounding of 0: either outcome is right)
        assert r["marginal"].mean() <= 1e-3
        g = np.where(ok, got[:, :256], r["g"])
        b = R.dx_bound(r, KIND)
        report(name, "dx", 0.0, g, r["g"], b)
        H.assert_within(g, r["g"], b, f"{name} dx", exact=ok & ~r["keep"])
        sums = H.rows_total(rows, nrows)
        report(name, "bn-sum1", 0.0, sums[0], r["s1"], r["b1"])
        report(name, "bn-sum2", 0.0, sums[1], r["s2"], r["b2"])
        H.assert_within(sums[0], r["s1"], r["b1"], f"{name} sum of the masked gradient")
        H.assert_within(sums[1], r["s2"], r["b2"], f"{name} sum of the masked gradient times xhat")


def test_fused_kernels_refuse_what_they_cannot_run(H):
    lib, st = cabi.load(BF16), H.stream()
    N, HW = 2, 48
    M = N * HW
    dd = dev_case(H, 3, 80, 64, BF16)                             # M = 240 pixels of inputs: the two-RoI calls of 96 pixels stay inside them
    x, w, bias, xd, wd, bd = fused_inputs(H, 3, 80, 264, 128)
    out = lambda: (H.Guarded((240, 76), torch.float32), H.Guarded((240, 128), HT), H.Guarded((1 + 64, 8), torch.float64))

    def conv(N=N, HW=HW, x_cs=264, nreg=64, dt=BF16, w_rows=128, hs=76, pcs=128, loss=False, head=True):
        hd, pnp, acc = out()
        if loss:
            rc = lib.gdrn_head_conv_tail_loss_fwd(ptr(xd), x_cs, ptr(wd), w_rows, ptr(bd), ptr(dd.coord2d), ptr(dd.extents), ptr(hd.t) if head else None, hs, ptr(pnp.t),
                                                  pcs, ptr(dd.gt_xyz), ptr(dd.mvis), ptr(dd.mtr), ptr(dd.greg), ptr(acc.t), N, HW, nreg, dt, st)
        else:
            rc = lib.gdrn_head_conv_tail_fwd(ptr(xd), x_cs, ptr(wd), w_rows, ptr(bd), ptr(dd.coord2d), ptr(dd.extents), ptr(hd.t) if head else None, hs, ptr(pnp.t), pcs,
                                             N, HW, nreg, dt, st)
        untouched = all(np.isnan(o.host()).all() for o in (hd, pnp, acc))
        return rc, untouched

    for loss in (False, True):
        assert conv(loss=loss)[0] == 0                            # the call the refusals below are variations of
        assert conv(N=2, HW=24, loss=loss) == (ERR_SHAPE, True)   # HW % 16 != 0 (M % 16 == 0)
        assert conv(nreg=63, loss=loss) == (ERR_SHAPE, True)
        assert conv(x_cs=260, loss=loss) == (ERR_SHAPE, True)     # x_cs % 8 != 0
        assert conv(N=1 << 17, HW=64, loss=loss) == (ERR_SHAPE, True)   # M * x_cs = 2^23 * 264 >= 2^31
        assert conv(dt=F32, loss=loss) == (ERR_SHAPE, True)
        assert conv(w_rows=68, loss=loss) == (ERR_SHAPE, True)
    assert conv(loss=True, head=False) == (ERR_ARG, True)         # the backward pass reads the logits
    i = R.dgrad_inputs(3, 240, KIND, 128, 128, 264)
    dev = {k: (H.to_dev(v, BF16) if k in ("dy", "wd", "raw") else H.f32_dev(v)) for k, v in i.items()}

    def dgrad(N=N, HW=HW, dy_cs=128, wd_cs=128, raw_cs=264, dx_cs=264, dt=BF16):
        dx, rows = H.Guarded((240, 264), HT), H.rows_buf(64, 256)
        rc = lib.gdrn_head_out_dgrad(ptr(dev["dy"]), dy_cs, ptr(dev["wd"]), wd_cs, ptr(dev["raw"]), raw_cs, ptr(dev["mean"]), ptr(dev["invstd"]), ptr(dev["scale"]),
                                     ptr(dev["shift"]), ptr(dx.t), dx_cs, ptr(rows), N, HW, dt, st)
        torch.cuda.synchronize()
        return rc, bool(np.isnan(dx.host()).all() and torch.isnan(rows).all())

    assert dgrad()[0] == 0
    assert dgrad(N=1, HW=24) == (ERR_SHAPE, True)                 # M % 16 != 0
    assert dgrad(dy_cs=100) == (ERR_SHAPE, True)                  # a stride that is no multiple of 8
    assert dgrad(wd_cs=88) == (ERR_SHAPE, True)                   # fewer than 96 columns
    assert dgrad(N=1 << 17, HW=64) == (ERR_SHAPE, True)           # M * 264 >= 2^31
    assert dgrad(dt=F32) == (ERR_SHAPE, True)
    assert lib.gdrn_head_out_dgrad_rows(1, 24) == ERR_ARG and lib.gdrn_head_conv_tail_loss_rows(1, 24) == ERR_ARG


# ---------------------------------------------------------------------------------------------- (d) the row-stride checks
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nreg", [17, 64])
def test_short_rows_are_refused_with_every_output_untouched(H, dt, nreg):
    """gdrn_head_tail_bwd reads h[4 + nreg] and, with d_pnp_in, pnp[4 + nreg]; gdrn_map_loss_fwd reads h[4 + nreg]: a stride below nreg + 5 makes them
    read the next pixel's values and, in the last row, past the buffer.  Every buffer here is allocated at the FULL row stride, so a library
    without the check would stay inside its allocations."""
    lib, st = cabi.load(BF16), H.stream()
    N, HW, C = 1, 17, nreg + 5
    full = 72 if nreg == 64 else C + 3
    d = dev_case(H, N, HW, nreg, dt)
    M = d.M
    pnp, acc, _ = fwd(H, d, dt, full, full, loss="atomics")
    dpn = d.d_pnp(full, dt)

    def call(hs, pcs, dcs, with_dpnp):
        dh = H.Guarded((M, full), tt(dt))
        rc = lib.gdrn_head_tail_bwd(ptr(d.head(full)), hs, ptr(pnp.t), ptr(dpn) if with_dpnp else None, pcs, ptr(d.extents), ptr(d.gt_xyz), ptr(d.mvis), ptr(d.mtr),
                                    ptr(d.greg), ptr(acc.t), ptr(d.gw), ptr(dh.t), dcs, N, HW, nreg, dt, st)
        return rc, bool(np.isnan(dh.host("d_head")).all())

    assert call(full, full, full, True)[0] == 0 and call(C, C, C, False)[0] == 0
    assert call(C - 1, full, full, True) == (ERR_ARG, True)       # hs < nreg + 5
    assert call(C - 1, full, full, False) == (ERR_ARG, True)
    assert call(full, C - 1, full, True) == (ERR_ARG, True)       # pcs < nreg + 5 with d_pnp_in given
    assert call(full, C - 1, full, False)[0] == 0                 # ... without it pcs is not used
    assert call(full, full, C - 1, True) == (ERR_ARG, True)       # (dcs: checked before this change as well)
    for hs, want in ((C - 1, ERR_ARG), (4, ERR_ARG), (C, 0)):
        acc2 = H.Guarded((1, 8), torch.float64)
        rc = lib.gdrn_map_loss_fwd(ptr(d.head(full)), hs, ptr(d.gt_xyz), ptr(d.mvis), ptr(d.mtr), ptr(d.greg), N, HW, nreg, ptr(acc2.t), st)
        assert rc == want and bool(np.isnan(acc2.host("acc")).all()) == (want != 0), (hs, rc)
