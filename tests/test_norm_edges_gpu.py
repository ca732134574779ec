"""Per-element tests (-m gpu) of the normalisation / pooling / resampling kernels of csrc/norm.hip and the casts of csrc/pack.hip at the edges
of their launch geometry, through the C ABI, against the fp64 numpy references of tests/norm_host.py (pinned on the CPU by
tests/test_norm_host_cpu.py).

Regime (a): small edge shapes (H != W, odd sizes, one pixel, sizes around every switch between two code paths), real-valued data, every element
held to   |got - ref| <= u_T |ref| + (1 + u_T) k 2^-24 A   with k and A derived next to each reference (no device figure enters a bound);
discrete outputs (tap codes, masks, zero patterns, elements that must be exactly dy) compared exactly.  Per-channel constants include negative
and zero BatchNorm scales and a shift that empties a pool window.  Outputs are pre-filled with NaN inside buffers with a guard row behind them.

Regime (b): every element exactly once at the launch-geometry switches (more than 1024 reduce workgroups, more rows per workgroup than the
floor, the 4096-workgroup cap of the grid-stride kernels and their second loop trip): small-integer operands and power-of-two constants make
every product and sum exact in any order, the expectation is plain torch fp32 on the CPU and the comparison is torch.equal.

The 16-bit format is a property of the library build: this module tests libgdrn_hip.so (bf16 and fp32);
tests/test_norm_edges_fp16_gpu.py executes the same source on libgdrn_hip_f16.so (regime (b) once, here)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_host as R
from gdrnet_amd import cabi
from gdrnet_amd.cabi import F32, check, ptr

pytestmark = pytest.mark.gpu

BF16 = globals().get("__HALF__", cabi.BF16)       # the 16-bit dtype code under test ("BF16" reads "the build's half" below)
IS_F16 = BF16 == cabi.F16
HT = torch.float16 if IS_F16 else torch.bfloat16
DTS = [BF16] if IS_F16 else [F32, BF16]            # (the fp32 kernels are tested once, out of the bf16 library)
LEFT_OUT = 1e-5                                     # largest share of a case's elements / windows that may be left out of an exact comparison


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hiputil

    cabi.load(BF16)
    return hiputil


def f32c(seed, C_, lo=-0.5, hi=0.5):
    return (lo + (hi - lo) * np.random.default_rng(seed).random(C_)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- (a) bilinear pair
def bn_apply_any_c(H, lib, xd, sc, sh, out, npix, C_, dt):
    """gdrn_bn_apply (ReLU); channel counts whose vector count does not divide 256 (C = 24) go through it in 8-channel slabs: the same kernel and
    arithmetic per element"""
    if 256 % (C_ // R.vec(H.KIND[dt])) == 0:
        check(lib.gdrn_bn_apply(ptr(xd), ptr(sc), ptr(sh), None, ptr(out), npix, C_, 1, dt, H.stream()), "bn_apply")
        return
    x2, o2 = xd.view(npix, C_), out.view(npix, C_)
    for c0 in range(0, C_, 8):
        xs, scs, shs = x2[:, c0:c0 + 8].contiguous(), sc[c0:c0 + 8].contiguous(), sh[c0:c0 + 8].contiguous()
        os_ = torch.full_like(xs, float("nan"))
        check(lib.gdrn_bn_apply(ptr(xs), ptr(scs), ptr(shs), None, ptr(os_), npix, 8, 1, dt, H.stream()), "bn_apply")
        torch.cuda.synchronize()
        o2[:, c0:c0 + 8] = os_


def run_upsample(H, dt, N, Hh, W, C_, seed=70, parts=("fwd", "bwd")):
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    u, k, td = R.U[kind], R.k_bilinear(Hh, W), H.tdt(dt)
    x = R.operand(seed, (N, Hh, W, C_), kind, 1.5)
    dy = R.operand(seed + 1, (N, 2 * Hh, 2 * W, C_), kind)
    xd, dyd = H.to_dev(x, dt), H.to_dev(dy, dt)
    tag = f"{kind} N{N} {Hh}x{W} C{C_}"
    scale, shift = R.channel_consts(seed + 2, C_)
    sc, sh = H.f32_dev(scale), H.f32_dev(shift)
    if "fwd" in parts:
        run_upsample_fwd(H, lib, dt, N, Hh, W, C_, x, xd, scale, shift, sc, sh, k, tag)
    if "bwd" in parts:
        return run_upsample_bwd(H, lib, dt, N, Hh, W, C_, x, xd, dy, dyd, scale, shift, sc, sh, k, seed, tag)


def run_upsample_fwd(H, lib, dt, N, Hh, W, C_, x, xd, scale, shift, sc, sh, k, tag):
    st, u, td = H.stream(), R.U[H.KIND[dt]], H.tdt(dt)
    # plain forward
    y = H.Guarded((N, 2 * Hh, 2 * W, C_), td)
    check(lib.gdrn_upsample2x_fwd(ptr(xd), ptr(y.t), N, Hh, W, C_, dt, st), "upsample_fwd")
    ref = R.upsample2x(x)
    H.assert_within(y.host(), ref, R.bound(ref, R.upsample_mag(x), k, u), f"upsample2x_fwd {tag}")
    # BatchNorm + ReLU form: bn_apply (held to its own reference) then the plain form, bit for bit; and against the reference on that activation
    act = H.Guarded((N, Hh, W, C_), td)
    bn_apply_any_c(H, lib, xd, sc, sh, act.t, N * Hh * W, C_, dt)
    aref = R.bn_apply(x, scale, shift, None, True)
    acth = act.host()
    H.assert_within(acth, aref, R.bound(aref, R.bn_apply_mag(x, scale, shift), R.K_BN_APPLY, u), f"bn_apply(relu) {tag}", exact=(aref == 0))
    two = H.Guarded((N, 2 * Hh, 2 * W, C_), td)
    one = H.Guarded((N, 2 * Hh, 2 * W, C_), td)
    check(lib.gdrn_upsample2x_fwd(ptr(act.t), ptr(two.t), N, Hh, W, C_, dt, st), "upsample_fwd")
    check(lib.gdrn_bn_relu_upsample2x_fwd(ptr(xd), ptr(sc), ptr(sh), ptr(one.t), N, Hh, W, C_, dt, st), "bn_relu_upsample_fwd")
    oneh = one.host()
    ref2 = R.upsample2x(acth)
    H.assert_within(oneh, ref2, R.bound(ref2, R.upsample_mag(acth), k, u), f"bn_relu_upsample2x_fwd {tag}")
    assert torch.equal(one.t, two.t), f"fused BN+ReLU upsampling differs from bn_apply + upsample2x_fwd {tag}"
    two.host()


def run_upsample_bwd(H, lib, dt, N, Hh, W, C_, x, xd, dy, dyd, scale, shift, sc, sh, k, seed, tag):
    st, u, td = H.stream(), R.U[H.KIND[dt]], H.tdt(dt)
    dx = H.Guarded((N, Hh, W, C_), td)
    check(lib.gdrn_upsample2x_bwd(ptr(dyd), ptr(dx.t), N, Hh, W, C_, dt, st), "upsample_bwd")
    dref = R.upsample2x_adjoint(dy)
    H.assert_within(dx.host(), dref, R.bound(dref, R.upsample_mag(dy, 4.0), k, u), f"upsample2x_bwd {tag}")
    # ... with the BatchNorm-backward sums
    mean, invstd = f32c(seed + 3, C_), f32c(seed + 4, C_, 0.5, 1.5)
    md, isd = H.f32_dev(mean), H.f32_dev(invstd)
    npix, tpr = N * Hh * W, C_ // R.vec(H.KIND[dt])
    if 256 % tpr:
        assert lib.gdrn_upsample2x_bwd_bnsums(ptr(dyd), ptr(dx.t), ptr(xd), ptr(md), ptr(isd), ptr(sc), ptr(sh), N, Hh, W, C_, ptr(md), dt, st) == -2
        return
    nrows = lib.gdrn_bn_bwd_reduce_rows(npix, C_, dt)
    rows = H.rows_buf(nrows, C_)
    dx2 = H.Guarded((N, Hh, W, C_), td)
    check(lib.gdrn_upsample2x_bwd_bnsums(ptr(dyd), ptr(dx2.t), ptr(xd), ptr(md), ptr(isd), ptr(sc), ptr(sh), N, Hh, W, C_, ptr(rows), dt, st), "bnsums")
    d2 = dx2.host()
    H.assert_within(d2, dref, R.bound(dref, R.upsample_mag(dy, 4.0), k, u), f"upsample2x_bwd_bnsums dx {tag}")
    assert torch.equal(dx2.t, dx.t), f"bnsums dx differs from upsample2x_bwd {tag}"
    check_bn_sums(H, rows, nrows, d2, None, x, scale, shift, mean, invstd, npix, C_, dt, f"bnsums rows {tag}")
    return nrows


def check_bn_sums(H, rows, nrows, g_stored, ymask, x, msc, msh, mean, invstd, npix, C_, dt, what):
    """partial rows summed in fp64 against the reference sums of the masked stored gradient: k_sum(terms a thread walks)"""
    tot = H.rows_total(rows, nrows)
    g, _ = R.bn_mask(g_stored, ymask, x, msc, msh)
    s1, s2 = R.bn_bwd_sums(g, x, mean, invstd)
    m1, m2 = R.bn_bwd_sums_mag(g, x, mean, invstd)
    rpp = 256 // (C_ // R.vec(H.KIND[dt]))
    k = R.k_sum(-(-(-(-npix // nrows)) // rpp))    # ceil(ceil(npix / workgroups) / row lanes): rows a thread walks
    H.assert_within(tot[0], s1, k * R.EPS32 * m1, what + " sum g")
    H.assert_within(tot[1], s2, k * R.EPS32 * m2, what + " sum g*xhat")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C_", R.UP_C)
@pytest.mark.parametrize("hw", R.UP_HW)
def test_upsample_pair_per_element(H, dt, C_, hw):
    """gdrn_upsample2x_fwd / gdrn_bn_relu_upsample2x_fwd / gdrn_upsample2x_bwd / gdrn_upsample2x_bwd_bnsums, H != W: C = 8 and 256 take the row
    kernel, C = 24 (3 or 6 channel vectors) the generic one -- in both BatchNorm+ReLU forms too"""
    for N in (1, 2):
        run_upsample(H, dt, N, hw[0], hw[1], C_)


@pytest.mark.parametrize("dt", DTS)
def test_upsample_both_sides_of_the_lds_switch(H, dt):
    """C = 256: two source rows of W pixels are 64 KiB of LDS at W = 64 (16-bit) / 32 (fp32): the row kernel; one pixel more: the generic kernel"""
    for (Hh, W) in R.UP_LDS_SWITCH[H.KIND[dt]]:
        assert (2 * W * 256 * (4 if dt == F32 else 2) > 65536) == (W % 2 == 1)
        run_upsample(H, dt, 1, Hh, W, 256, seed=170)


# ---------------------------------------------------------------------------------------------- (a) stem pool
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C_", R.POOL_C)
@pytest.mark.parametrize("hw", R.POOL_HW)
def test_pool_per_element_and_tap_codes(H, dt, C_, hw):
    """gdrn_bn_relu_maxpool_fwd: y per element, the tap code ky*3 + kx of the FIRST tap in scan order that attains the maximum exactly (negative
    and zero scales, an all-zero window, integer levels with many positive ties); gdrn_maxpool_bwd: g exactly 0 / exactly dy where at most one
    window points at the pixel, bounded elsewhere; with rows: the same g bit for bit and the row totals"""
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    u, td = R.U[kind], H.tdt(dt)
    Hh, W = hw
    for N in (1, 3):
        for integer in (False, True):
            tag = f"{kind} N{N} {Hh}x{W} C{C_} {'integer' if integer else 'real'}"
            x, scale, shift = R.pool_inputs(1000 + Hh * 37 + W, N, Hh, W, C_, kind, integer)
            dy = R.operand(1001 + Hh, (N, Hh // 2, W // 2, C_), kind)
            xd, dyd, sc, sh = H.to_dev(x, dt), H.to_dev(dy, dt), H.f32_dev(scale), H.f32_dev(shift)
            y = H.Guarded((N, Hh // 2, W // 2, C_), td)
            idx = H.Guarded((N, Hh // 2, W // 2, C_), torch.uint8)
            check(lib.gdrn_bn_relu_maxpool_fwd(ptr(xd), ptr(sc), ptr(sh), ptr(y.t), ptr(idx.t), N, Hh, W, C_, dt, st), "pool_fwd")
            yref, code = R.bn_relu_maxpool(x, scale, shift)
            H.assert_within(y.host(), yref, R.bound(yref, R.bn_relu_maxpool_mag(x, scale, shift), R.K_POOL, u), f"pool y {tag}", exact=(yref == 0))
            gap, mag = R.pool_top2_gap(x, scale, shift)
            amb = (gap > 0) & (gap <= 2.0 ** -22 * mag)          # two distinct candidates within rounding of each other: no rule to hold it to
            assert amb.mean() <= LEFT_OUT
            idxh = idx.host()
            H.assert_same(np.where(amb, code, idxh), code, f"pool tap codes {tag}")
            # backward on the reference's tap codes
            codd = torch.from_numpy(code).to(H.DEV)
            g = H.Guarded((N, Hh, W, C_), td)
            check(lib.gdrn_maxpool_bwd(ptr(dyd), ptr(codd), ptr(xd), ptr(sc), ptr(sh), ptr(g.t), N, Hh, W, C_, None, None, None, dt, st), "pool_bwd")
            gref = R.maxpool_bwd(dy, code, x, scale, shift)
            gmag = R.maxpool_bwd(dy, code, x, scale, shift, mag=True)
            cnt = R.maxpool_bwd(np.ones_like(dy), code, x, scale, shift)
            left = R.affine_sign_margin(x, scale, shift)      # sign of x*scale + shift within fp32 rounding of 0 (contracted or not)
            assert left.mean() <= LEFT_OUT
            gh = np.where(left, gref, g.host())
            H.assert_within(gh, gref, R.bound(gref, gmag, R.K_POOL_BWD, u), f"pool g {tag}", exact=(cnt <= 1))
            mean, invstd = f32c(1002, C_), f32c(1003, C_, 0.5, 1.5)
            md, isd = H.f32_dev(mean), H.f32_dev(invstd)
            cvn = C_ // R.vec(H.KIND[dt])
            nrows = lib.gdrn_maxpool_bwd_rows(N, Hh, W, C_, dt)
            rows = H.rows_buf(max(nrows, 1), C_)
            g2 = H.Guarded((N, Hh, W, C_), td)
            rc = lib.gdrn_maxpool_bwd(ptr(dyd), ptr(codd), ptr(xd), ptr(sc), ptr(sh), ptr(g2.t), N, Hh, W, C_, ptr(md), ptr(isd), ptr(rows), dt, st)
            if cvn > 64:
                assert rc == -2        # a thread would change its channel vector between grid-stride trips (fp32 C = 512)
                continue
            check(rc, "pool_bwd(rows)")
            g2.host()
            assert torch.equal(g2.t, g.t)
            tot = H.rows_total(rows, nrows)
            gs = H.to_host(g.t)                                # the stored (rounded) gradient is what the sums see
            s1, s2 = R.bn_bwd_sums(gs, x, mean, invstd)
            m1, m2 = R.bn_bwd_sums_mag(gs, x, mean, invstd)
            k = R.k_sum(-(-(N * Hh * W * cvn) // (nrows * 256)))   # grid-stride trips of a thread
            H.assert_within(tot[0], s1, k * R.EPS32 * m1, f"pool rows sum g {tag}")
            H.assert_within(tot[1], s2, k * R.EPS32 * m2, f"pool rows sum g*xhat {tag}")


# ---------------------------------------------------------------------------------------------- (a) BatchNorm
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C_", R.BN_C)
def test_bn_apply_reduce_bwd_apply_per_element(H, dt, C_):
    """gdrn_bn_apply (with / without residual and ReLU), gdrn_bn_bwd_reduce and gdrn_bn_bwd_apply under every mask combination (stored, affine,
    both, neither; with and without g_out) at npix = 1, one short of the row lanes, 433, 1283.  The masks are exact: g_out is exactly 0 or dy."""
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    u, td = R.U[kind], H.tdt(dt)
    for npix in R.bn_npix(C_, kind):
        tag = f"{kind} npix{npix} C{C_}"
        x = R.operand(2000 + npix, (npix, C_), kind, 2.0, 0.5)
        scale, shift = R.channel_consts(2001 + npix, C_)
        res, dy = R.operand(2002 + npix, (npix, C_), kind), R.operand(2003 + npix, (npix, C_), kind)
        xd, resd, dyd, sc, sh = H.to_dev(x, dt), H.to_dev(res, dt), H.to_dev(dy, dt), H.f32_dev(scale), H.f32_dev(shift)
        ymask = None
        for with_res in (False, True):
            for relu in (0, 1):
                y = H.Guarded((npix, C_), td)
                check(lib.gdrn_bn_apply(ptr(xd), ptr(sc), ptr(sh), ptr(resd) if with_res else None, ptr(y.t), npix, C_, relu, dt, st), "bn_apply")
                r = res if with_res else None
                ref = R.bn_apply(x, scale, shift, r, bool(relu))
                H.assert_within(y.host(), ref, R.bound(ref, R.bn_apply_mag(x, scale, shift, r), R.K_BN_APPLY, u), f"bn_apply res={with_res} relu={relu} {tag}")
                if with_res and relu:
                    ymask = y          # the stored activation of BN + residual + ReLU: the mask source of the backward
        ymh = ymask.host()
        mean, invstd = f32c(2004, C_), f32c(2005, C_, 0.5, 1.5)
        a, b, c = (np.random.default_rng(2006 + i).standard_normal(C_).astype(np.float32) for i in range(3))
        md, isd, ad, bd, cd = (H.f32_dev(v) for v in (mean, invstd, a, b, c))
        nrows = lib.gdrn_bn_bwd_reduce_rows(npix, C_, dt)
        assert 1 <= nrows <= 1024
        for stored in (False, True):
            for affine in (False, True):
                ym_p, ym_h = (ptr(ymask.t), ymh) if stored else (None, None)
                ms_p, mh_p, msc, msh = (ptr(sc), ptr(sh), scale, shift) if affine else (None, None, None, None)
                g, _ = R.bn_mask(dy, ym_h, x, msc, msh)
                rows = H.rows_buf(nrows, C_)
                check(lib.gdrn_bn_bwd_reduce(ptr(dyd), ym_p, ptr(xd), ptr(md), ptr(isd), ms_p, mh_p, npix, C_, ptr(rows), dt, st), "bn_bwd_reduce")
                check_bn_sums(H, rows, nrows, dy, ym_h, x, msc, msh, mean, invstd, npix, C_, dt, f"bn_bwd_reduce stored={stored} affine={affine} {tag}")
                dref = R.bn_bwd_apply(g, x, a, b, c)
                for with_gout in (False, True):
                    dx, gout = H.Guarded((npix, C_), td), H.Guarded((npix, C_), td)
                    check(lib.gdrn_bn_bwd_apply(ptr(dyd), ym_p, ptr(xd), ptr(ad), ptr(bd), ptr(cd), ms_p, mh_p, npix, C_, ptr(dx.t),
                                                ptr(gout.t) if with_gout else None, dt, st), "bn_bwd_apply")
                    H.assert_within(dx.host(), dref, R.bound(dref, R.bn_bwd_apply_mag(g, x, a, b, c), R.K_BN_BWD_APPLY, u),
                                    f"bn_bwd_apply dx stored={stored} affine={affine} {tag}")
                    if with_gout:
                        H.assert_same(gout.host(), g, f"bn_bwd_apply g_out (exactly 0 or dy) stored={stored} affine={affine} {tag}")
                    else:
                        torch.cuda.synchronize()
                        assert bool(torch.isnan(gout.buf).all())


@pytest.mark.parametrize("C_", [8, 512])
@pytest.mark.parametrize("nrows", [1, 255, 257, 1024])
def test_bn_coef_and_finalize_from_the_devices_own_rows(H, nrows, C_):
    """gdrn_bn_bwd_coef / gdrn_bn_finalize (fp64 totals of fp32 partial rows, one launch, 256 rows per pass: 1, 255, 257, 1024 rows) against fp64
    from the same rows; count = 1 (the unbiased-variance guard); running statistics NULL and not"""
    lib, st = cabi.load(BF16), H.stream()
    u32 = R.U["fp32"]
    rg = np.random.default_rng(3000 + nrows)
    rows = rg.standard_normal((nrows, 2, C_)).astype(np.float32)
    gamma, mean, invstd = f32c(3001, C_, 0.5, 1.5), f32c(3002, C_), f32c(3003, C_, 0.5, 1.5)
    gamma[1::4] *= -1.0
    rd, gd, md, isd = (H.f32_dev(v) for v in (rows, gamma, mean, invstd))
    npix = 1283
    s = R.f64(rows).sum(0)
    for with_grads in (True, False):
        o = [H.Guarded((C_,), torch.float32) for _ in range(5)]
        check(lib.gdrn_bn_bwd_coef(ptr(rd), nrows, C_, npix, ptr(gd), ptr(md), ptr(isd), ptr(o[0].t), ptr(o[1].t), ptr(o[2].t),
                                   ptr(o[3].t) if with_grads else None, ptr(o[4].t) if with_grads else None, st), "bn_bwd_coef")
        a, b, c, dgamma, dbeta = R.bn_bwd_coef(s[0], s[1], npix, gamma, mean, invstd)
        ma, mb, mc = R.bn_bwd_coef_mag(s[0], s[1], npix, gamma, mean, invstd)
        for got, ref, mag, nm in ((o[0], a, ma, "a"), (o[1], b, mb, "b"), (o[2], c, mc, "c")):
            H.assert_within(got.host(), ref, R.bound(ref, mag, R.K_COEF, u32), f"bn_bwd_coef {nm} rows{nrows} C{C_}")
        if with_grads:   # (float) of the fp64 total: one rounding (and the fp64 total's own order, far below it)
            H.assert_within(o[3].host(), dgamma, 1.01 * u32 * np.abs(dgamma), f"bn_bwd_coef dgamma rows{nrows} C{C_}")
            H.assert_within(o[4].host(), dbeta, 1.01 * u32 * np.abs(dbeta), f"bn_bwd_coef dbeta rows{nrows} C{C_}")
        else:
            torch.cuda.synchronize()
            assert bool(torch.isnan(o[3].buf).all() and torch.isnan(o[4].buf).all())
    # finalize: rows of (sum x, sum x^2) of 8 values each; and one row with count = 1
    beta = f32c(3004, C_)
    bd = H.f32_dev(beta)
    for rows_n, count in ((nrows, 8 * nrows), (1, 1)):
        xs = rg.standard_normal((rows_n, count // rows_n, C_)) * 1.5 + 0.3
        part = np.stack([xs.sum(1), (xs * xs).sum(1)], axis=1).astype(np.float32)
        pd = H.f32_dev(part)
        tot = R.f64(part).sum(0)
        for running in (True, False):
            rm0, rv0 = f32c(3005, C_), f32c(3006, C_, 0.5, 1.5)
            rmd, rvd = H.f32_dev(rm0), H.f32_dev(rv0)
            nbt = torch.full((), 41, dtype=torch.int64, device=H.DEV)
            o = [H.Guarded((C_,), torch.float32) for _ in range(4)]
            check(lib.gdrn_bn_finalize(ptr(pd), rows_n, C_, float(count), ptr(gd), ptr(bd), ptr(rmd) if running else None, ptr(rvd) if running else None,
                                       ptr(nbt) if running else None, 0.1, 1e-5, ptr(o[0].t), ptr(o[1].t), ptr(o[2].t), ptr(o[3].t), None, st), "bn_finalize")
            fin = R.bn_finalize(tot[0], tot[1], count, gamma, beta, 1e-5, rm0 if running else None, rv0 if running else None, 0.1)
            tag = f"rows{rows_n} count{count} C{C_} running={running}"
            # mean = (float) of an fp64 quotient: one rounding.  invstd: the fp64 difference s2/n - m^2 cancels (relative 2^-53 n |s2/n| / (var + eps),
            # far below 2^-24 for these rows), then one rounding
            H.assert_within(o[0].host(), fin["mean"], 1.01 * u32 * np.abs(fin["mean"]), f"bn_finalize mean {tag}")
            H.assert_within(o[1].host(), fin["invstd"], 1.01 * u32 * np.abs(fin["invstd"]), f"bn_finalize invstd {tag}")
            H.assert_within(o[2].host(), fin["scale"], R.bound(fin["scale"], np.abs(fin["scale"]), R.K_FINALIZE, u32), f"bn_finalize scale {tag}")
            H.assert_within(o[3].host(), fin["shift"], R.bound(fin["shift"], fin["shift_mag"], R.K_FINALIZE, u32), f"bn_finalize shift {tag}")
            if running:
                H.assert_within(H.to_host(rmd), fin["running_mean"], R.bound(fin["running_mean"], fin["running_mean_mag"], R.K_FINALIZE, u32), f"running_mean {tag}")
                H.assert_within(H.to_host(rvd), fin["running_var"], R.bound(fin["running_var"], fin["running_var_mag"], R.K_FINALIZE, u32), f"running_var {tag}")
                assert int(nbt) == 42
            if count == 1:
                assert np.all(fin["var"] < 1e-4)   # (the guard: var * count / (count - 1) is not formed)


# ---------------------------------------------------------------------------------------------- (a) GroupNorm + ReLU
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", R.GN_SLAB32 + R.GN_WHOLE)
def test_groupnorm_relu_per_element(H, dt, case):
    """gdrn_gn_relu_fwd / gdrn_gn_relu_bwd: the 32-channel slab path with HW around the register-cached form's limit (a last pass cut short by
    r < HW) and the whole-C slabs ((64, 1): <= 64 channels with the pc tree; (128, 2), (256, 1), (512, 4): > 64 without; (64, 2) has 32 channels
    per group and takes the 32-channel slab); mean_rstd to 1 ulp of fp32; dgamma / dbeta with GDRN_PREZEROED
    on a zeroed buffer and without it on a buffer of NaN"""
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    u, td = R.U[kind], H.tdt(dt)
    C_, G, HW = case
    cpg, V = C_ // G, R.vec(H.KIND[dt])
    CS = R.gn_slab(C_, G, V)
    rpp = 256 // (CS // V)
    for N in (1, 3):
        tag = f"{kind} N{N} HW{HW} C{C_} G{G} (slab {CS}, {rpp} row lanes)"
        x = R.operand(4000 + HW, (N, HW, C_), kind, 1.5, 0.3)
        dy = R.operand(4001 + HW, (N, HW, C_), kind)
        gam, bet = f32c(4002, C_, 0.5, 1.5), f32c(4003, C_)
        gam[1::4] *= -1.0
        xd, dyd, gd, bd = H.to_dev(x, dt), H.to_dev(dy, dt), H.f32_dev(gam), H.f32_dev(bet)
        y, mr = H.Guarded((N, HW, C_), td), H.Guarded((N, G, 2), torch.float32)
        check(lib.gdrn_gn_relu_fwd(ptr(xd), ptr(gd), ptr(bd), ptr(y.t), ptr(mr.t), N, HW, C_, G, 1e-5, dt, st), "gn_fwd")
        yref, mean, rstd = R.gn_relu_fwd(x, gam, bet, G, 1e-5)
        mrh = mr.host()
        ulp = lambda v: R.f64(np.spacing(np.abs(v).astype(np.float32)))
        worst = max(float((np.abs(mrh[..., 0] - mean) / ulp(mean)).max()), float((np.abs(mrh[..., 1] - rstd) / ulp(rstd)).max()))
        print(f"gn mean_rstd {tag}: worst {worst:.2f} ulp")
        H.assert_within(mrh[..., 0], mean, ulp(mean), f"gn mean {tag}")
        H.assert_within(mrh[..., 1], rstd, ulp(rstd), f"gn rstd {tag}")
        yh = y.host()
        H.assert_within(yh, yref, R.bound(yref, R.gn_relu_fwd_mag(x, gam, bet, mean, rstd, G), R.K_GN_FWD, u), f"gn y {tag}")
        # backward from the device's own stored y and mean_rstd
        dref, dgam, dbet = R.gn_relu_bwd(dy, yh, x, gam, mrh[..., 0], mrh[..., 1], G)
        dmag, gmag, bmag = R.gn_relu_bwd(dy, yh, x, gam, mrh[..., 0], mrh[..., 1], G, mag=True)
        shA, shB = R.gn_relu_bwd_shares(dy, yh, x, gam, mrh[..., 0], mrh[..., 1], G)
        for prezeroed in (True, False):
            dx = H.Guarded((N, HW, C_), td)
            dg = H.Guarded((C_,), torch.float32)
            db = H.Guarded((C_,), torch.float32)
            if prezeroed:
                dg.t.zero_()
                db.t.zero_()
            check(lib.gdrn_gn_relu_bwd(ptr(dyd), ptr(y.t), ptr(xd), ptr(gd), ptr(mr.t), ptr(dx.t), ptr(dg.t), ptr(db.t), N, HW, C_, G,
                                       dt | (cabi.PREZEROED if prezeroed else 0), st), "gn_bwd")
            H.assert_within(dx.host(), dref, R.gn_dx_bound(dref, dmag, shA, shB, HW, rpp, cpg, u), f"gn dx {tag}")
            H.assert_within(dg.host(), dgam, R.k_gn_dgamma(HW, rpp, N) * R.EPS32 * gmag, f"gn dgamma prezeroed={prezeroed} {tag}")
            H.assert_within(db.host(), dbet, R.k_gn_dbeta(HW, rpp, N) * R.EPS32 * bmag, f"gn dbeta prezeroed={prezeroed} {tag}")


# ---------------------------------------------------------------------------------------------- (a) LeakyReLU backward, bias gradient, layout
@pytest.mark.parametrize("dt", DTS)
def test_leaky_bwd_zero_signs_and_subnormals(H, dt):
    """n = 8 (one vector of the 16-bit type): y = +0, -0 (not > 0: the slope), the smallest subnormal of the storage type of either sign (> 0: exactly dy)"""
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    tiny = {"fp32": 2.0 ** -149, "bf16": 2.0 ** -133, "fp16": 2.0 ** -24}[kind]
    for n, seed in ((8, 5000), (8 * 37, 5001)):
        y = R.operand(seed, (n,), kind)
        y[:8] = [0.0, -0.0, tiny, -tiny, 1.0, -1.0, 3.0e4, -3.0e4]
        dy = R.operand(seed + 1, (n,), kind, 3.0)
        yd, dyd = H.to_dev(y, dt), H.to_dev(dy, dt)
        assert float(yd[2]) == tiny and math.copysign(1.0, float(yd[1])) == -1.0    # (the operands reached the device as meant)
        dx = H.Guarded((n,), H.tdt(dt))
        check(lib.gdrn_leaky_bwd(ptr(dyd), ptr(yd), ptr(dx.t), n, dt, st), "leaky_bwd")
        ref = R.leaky_bwd(dy, y)
        H.assert_within(dx.host(), ref, R.bound(ref, R.SLOPE * np.abs(dy) * (y <= 0), R.K_LEAKY, R.U[kind]), f"leaky_bwd {kind} n{n}", exact=(y > 0))


@pytest.mark.parametrize("dt", DTS)
def test_bias_grad_single_row_partial_columns_and_widest_stride(H, dt):
    """gdrn_bias_grad: rows = 1 (the sum IS the row: exact), C below the stride (69 of 128, 1 of 8), stride 1024 (the widest: all 256 threads on one
    row in fp32); with GDRN_PREZEROED on a zeroed buffer and without it on a buffer of NaN; nothing behind db[C] is written"""
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    V = R.vec(H.KIND[dt])
    for cs, C_, rows in ((8, 8, 1), (128, 69, 1), (8, 1, 1), (1024, 1024, 1), (1024, 1024, 37), (1024, 1000, 37)):
        d = R.operand(5100 + cs + rows, (rows, cs), kind)
        dd = H.to_dev(d, dt)
        ref = R.col_sums(d, C_)
        rpp = 256 // (cs // V)
        k = R.k_bias(rows, rpp)
        assert rows == 1 or k <= R.k_sum(min(16, -(-rows // rpp)))
        for prezeroed in (True, False):
            db = H.Guarded((C_,), torch.float32)
            if prezeroed:
                db.t.zero_()
            check(lib.gdrn_bias_grad(ptr(dd), cs, rows, C_, ptr(db.t), dt | (cabi.PREZEROED if prezeroed else 0), st), "bias_grad")
            bnd = 0.0 if rows == 1 else k * R.EPS32 * np.abs(d[:, :C_]).sum(0)
            H.assert_within(db.host(), ref, bnd, f"bias_grad {kind} cs{cs} C{C_} rows{rows} prezeroed={prezeroed}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("HW", [1, 49])
def test_nhwc_to_nchw_channel_window(H, dt, HW):
    """gdrn_nhwc_to_nchw_f32: a channel window [c0, c0 + C) of a wider pixel stride -> NCHW fp32, exact"""
    lib, st, kind = cabi.load(BF16), H.stream(), H.KIND[dt]
    N, cs, c0, C_ = 3, 16, 3, 5
    src = R.operand(5200 + HW, (N, HW, cs), kind)
    sd = H.to_dev(src, dt)
    dst = H.Guarded((N, C_, HW), torch.float32)
    check(lib.gdrn_nhwc_to_nchw_f32(ptr(sd), cs, c0, C_, ptr(dst.t), N, HW, dt, st), "nhwc_to_nchw")
    H.assert_same(dst.host(), np.transpose(src[:, :, c0:c0 + C_], (0, 2, 1)), f"nhwc_to_nchw {kind} HW{HW}")
    assert lib.gdrn_nhwc_to_nchw_f32(ptr(sd), cs, 12, C_, ptr(dst.t), N, HW, dt, st) == -1    # window past the stride


# ---------------------------------------------------------------------------------------------- the casts (pack_bf2 / f2bf of common.h)
def cast_inputs():
    """fp32 bit patterns around every rounding decision of the build's 16-bit format: for every 16-bit pattern h and its successor the fp32
    midpoint and its two fp32 neighbours (ties to even, carries into the exponent, the overflow edge, the subnormal range), +-0, +-inf, +-max
    finite, fp32 subnormals, NaNs"""
    if IS_F16:
        h = np.arange(0, 0x7C00, dtype=np.uint16)
        a = h.view(np.float16).astype(np.float32)
        b = np.append(a[1:], np.float32(65536.0))            # the successor of the largest finite half: where it would be (the overflow edge)
        mid = ((a.astype(np.float64) + b.astype(np.float64)) / 2).astype(np.float32)      # exact: 12 significant bits
        pos = np.concatenate([np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(np.inf))])
        bits = np.concatenate([pos, -pos]).view(np.uint32)
    else:
        h = np.arange(0, 0x10000, dtype=np.uint32) << 16        # every upper half, signs, inf and NaN patterns included
        bits = np.concatenate([h | 0x7FFF, h | 0x8000, h | 0x8001]).astype(np.uint32)
        assert bits.size == 196608
    extra = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                      0x00400000, 0x00012345, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF800001, 0x7FFFFFFF, 0x477FE000, 0x477FEFFF,
                      0x477FF000, 0x33800000, 0x33000000, 0x33000001, 0x32FFFFFF], dtype=np.uint32)
    sub = np.random.default_rng(5300).integers(1, 0x00800000, 4096).astype(np.uint32)     # fp32 subnormals of either sign
    return np.concatenate([bits, extra, sub, sub | 0x80000000]).astype(np.uint32)


def test_cast_from_f32_rounds_to_nearest_even_at_every_tie(H):
    """gdrn_cast_from_f32: the bit pattern of torch's CPU conversion (round to nearest even; NaN compared as NaN-ness)"""
    lib, st = cabi.load(BF16), H.stream()
    bits = cast_inputs()
    src = torch.from_numpy(bits.view(np.float32).copy())
    want = src.to(HT).view(torch.int16).numpy().view(np.uint16)
    dst = H.Guarded((bits.size,), HT)
    check(lib.gdrn_cast_from_f32(ptr(src.to(H.DEV)), ptr(dst.t), bits.size, BF16, st), "cast_from_f32")
    dst.host()
    got = dst.t.view(torch.int16).cpu().numpy().view(np.uint16)
    nan = np.isnan(src.numpy())
    assert np.array_equal(np.isnan(dst.t.float().cpu().numpy()), nan)
    fb = bits.astype(np.int64)
    idx = np.flatnonzero((got != want) & ~nan)
    assert idx.size == 0, "fp32 -> 16-bit differs from round-to-nearest-even at " + ", ".join(f"{fb[i]:#010x}: got {got[i]:#06x} want {want[i]:#06x}" for i in idx[:8])
    # fp32 destination: a copy, bit for bit
    d32 = H.Guarded((bits.size,), torch.float32)
    check(lib.gdrn_cast_from_f32(ptr(src.to(H.DEV)), ptr(d32.t), bits.size, F32, st), "cast_from_f32(f32)")
    d32.host()
    assert np.array_equal(d32.t.view(torch.int32).cpu().numpy()[~nan], src.view(torch.int32).numpy()[~nan])


def test_cast_to_f32_is_exact_over_all_patterns(H):
    lib, st = cabi.load(BF16), H.stream()
    pat = torch.from_numpy(np.arange(0x10000, dtype=np.uint16).view(np.int16).copy()).view(HT)
    want = pat.float()
    dst = H.Guarded((0x10000,), torch.float32)
    check(lib.gdrn_cast_to_f32(ptr(pat.to(H.DEV)), ptr(dst.t), 0x10000, BF16, st), "cast_to_f32")
    dst.host()
    got = dst.t.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    H.assert_same(got.view(torch.int32).numpy()[~nan.numpy()], want.view(torch.int32).numpy()[~nan.numpy()], "cast_to_f32 bit patterns")


# ---------------------------------------------------------------------------------------------- (b) every element once at the geometry switches
if not IS_F16:   # (one storage type per case is enough: the fp16 twin does not repeat this regime)
    def ints(seed, shape, lo, hi):
        return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32))

    def consts(seed, C_):
        return {k: torch.from_numpy(v) for k, v in R.pow2_consts(seed, C_).items()}

    @pytest.mark.parametrize("C_,dt,npix", [(512, F32, 8463), (512, BF16, 16411), (64, BF16, 132300)])
    def test_exact_bn_bwd_reduce_above_1024_workgroups(H, C_, dt, npix):
        """bwd_reduce_grid re-grids (npix > 4096 row passes): every pixel exactly once into exactly one of <= 1024 partial rows"""
        lib, st = cabi.load(BF16), H.stream()
        rpp = 256 // (C_ // R.vec(H.KIND[dt]))
        nrows = lib.gdrn_bn_bwd_reduce_rows(npix, C_, dt)
        assert npix > 4096 * rpp and nrows <= 1024
        print(f"bn_bwd_reduce C{C_} {H.KIND[dt]} npix{npix}: {nrows} workgroups, {rpp} row lanes, >= {-(-npix // nrows)} rows per workgroup")
        dy, x, k = ints(6000, (npix, C_), -2, 2), ints(6001, (npix, C_), -3, 3), consts(6002, C_)
        g = torch.where(x * k["scale"] + k["shift"] > 0, dy, torch.zeros(()))
        want = torch.stack([g.sum(0), (g * (x - k["mean"]) * k["invstd"]).sum(0)])
        assert float(want.abs().max()) < 2 ** 23
        dev = {n: v.to(H.DEV) for n, v in k.items()}
        dyd, xd = dy.to(H.DEV).to(H.tdt(dt)), x.to(H.DEV).to(H.tdt(dt))
        rows = H.rows_buf(nrows, C_)
        check(lib.gdrn_bn_bwd_reduce(ptr(dyd), None, ptr(xd), ptr(dev["mean"]), ptr(dev["invstd"]), ptr(dev["scale"]), ptr(dev["shift"]), npix, C_, ptr(rows), dt, st), "bn_bwd_reduce")
        tot = H.rows_total(rows, nrows)
        H.assert_same(tot, want.double().numpy(), "channel totals (exact integers and halves)")

    def test_exact_and_bounded_upsample_bwd_bnsums_above_1024_workgroups(H):
        """the same switch in gdrn_upsample2x_bwd_bnsums (fp32: 4 row lanes at C = 256, 16637 pixels; the 16-bit type's 8 row lanes would stay below
        it).  The bilinear weights are not dyadic, so nothing here is exact in any order: dx per element and the fp64 totals of the partial rows
        are held to the regime (a) bounds"""
        npix = 131 * 127
        assert npix > 4096 * (256 // (256 // 4))
        nrows = run_upsample(H, F32, 1, 131, 127, 256, seed=6100, parts=("bwd",))
        print(f"upsample2x_bwd_bnsums C256 fp32 npix{npix}: {nrows} workgroups")
        assert nrows <= 1024 and -(-npix // nrows) > 16

    @pytest.mark.parametrize("dt,npix", [(F32, 16411), (BF16, 32801)])
    def test_exact_bn_apply_and_bwd_apply_above_the_rows_floor(H, dt, npix):
        """ew_rows leaves its 4-rows-per-thread floor (npix > 8192 row passes, C = 512): every element bit for bit"""
        lib, st, C_ = cabi.load(BF16), H.stream(), 512
        rpp = 256 // (C_ // R.vec(H.KIND[dt]))
        rpb = -(-(-(-npix // 2048)) // rpp) * rpp     # ew_rows: ceil(npix / 2048) rounded up to whole passes of the row lanes, at least 4 passes
        assert npix > 8192 * rpp and rpb > 4 * rpp
        print(f"bn_apply / bn_bwd_apply C512 {H.KIND[dt]} npix{npix}: {rpp} row lanes, {rpb} rows per workgroup (floor {4 * rpp})")
        td = H.tdt(dt)
        x, res, dy, k = ints(6200, (npix, C_), -3, 3), ints(6201, (npix, C_), -3, 3), ints(6202, (npix, C_), -2, 2), consts(6203, C_)
        dev = {n: v.to(H.DEV) for n, v in k.items()}
        xd, resd, dyd = (v.to(H.DEV).to(td) for v in (x, res, dy))
        y = H.Guarded((npix, C_), td)
        check(lib.gdrn_bn_apply(ptr(xd), ptr(dev["scale"]), ptr(dev["shift"]), ptr(resd), ptr(y.t), npix, C_, 1, dt, st), "bn_apply")
        y.host()
        want = F.relu(x * k["scale"] + k["shift"] + res)
        assert torch.equal(y.t.cpu(), want.to(td)) and torch.equal(want.to(td).float(), want)
        # backward apply: a = scale, b = invstd, c = shift of the constants; stored + affine mask; g_out
        dx, gout = H.Guarded((npix, C_), td), H.Guarded((npix, C_), td)
        check(lib.gdrn_bn_bwd_apply(ptr(dyd), ptr(y.t), ptr(xd), ptr(dev["scale"]), ptr(dev["invstd"]), ptr(dev["shift"]), ptr(dev["scale"]), ptr(dev["shift"]),
                                    npix, C_, ptr(dx.t), ptr(gout.t), dt, st), "bn_bwd_apply")
        dx.host(), gout.host()
        g = torch.where((want > 0) & (x * k["scale"] + k["shift"] > 0), dy, torch.zeros(()))
        wdx = k["scale"] * g + (k["invstd"] * x + k["shift"])
        assert torch.equal(wdx.to(td).float(), wdx)
        assert torch.equal(gout.t.cpu(), g.to(td)) and torch.equal(dx.t.cpu(), wdx.to(td))

    @pytest.mark.parametrize("dt,C_", [(BF16, 512), (F32, 256)])
    def test_exact_pool_second_grid_stride_trip(H, dt, C_):
        """ew_grid caps at 4096 workgroups: the pool forward (1.13 M vectors) and backward (4.5 M) take a second and a fifth grid-stride trip; with rows,
        64 channel vectors (the row reduction without a shuffle level): a thread must keep its channel vector over the trips.  y, idx, g bit for
        bit, the row totals exactly the integers"""
        lib, st = cabi.load(BF16), H.stream()
        N, Hh, W = 2, 184, 192
        td, cvn = H.tdt(dt), C_ // R.vec(H.KIND[dt])
        assert cvn == 64 and N * (Hh // 2) * (W // 2) * cvn > 4096 * 256
        nrows = lib.gdrn_maxpool_bwd_rows(N, Hh, W, C_, dt)
        print(f"pool C{C_} {H.KIND[dt]}: forward {N * Hh * W * cvn // 4} vectors, backward {N * Hh * W * cvn} vectors on {nrows} workgroups")
        assert nrows == 4096
        x, dy, k = ints(6300, (N, C_, Hh, W), -3, 3), ints(6301, (N, C_, Hh // 2, W // 2), -2, 2), consts(6302, C_)
        cv = lambda v: v.view(1, -1, 1, 1)
        t = (x * cv(k["scale"]) + cv(k["shift"])).requires_grad_(True)
        yw, ind = F.max_pool2d(F.relu(t), 3, 2, 1, return_indices=True)
        yw.backward(dy)
        oy, ox = torch.arange(Hh // 2).view(1, 1, -1, 1), torch.arange(W // 2).view(1, 1, 1, -1)
        code = ((ind // W - (2 * oy - 1)) * 3 + (ind % W - (2 * ox - 1))).to(torch.uint8)
        to_nhwc = lambda v: v.detach().permute(0, 2, 3, 1).contiguous()
        xd, dyd = to_nhwc(x).to(H.DEV).to(td), to_nhwc(dy).to(H.DEV).to(td)
        dev = {n: v.to(H.DEV) for n, v in k.items()}
        y, idx = H.Guarded((N, Hh // 2, W // 2, C_), td), H.Guarded((N, Hh // 2, W // 2, C_), torch.uint8)
        check(lib.gdrn_bn_relu_maxpool_fwd(ptr(xd), ptr(dev["scale"]), ptr(dev["shift"]), ptr(y.t), ptr(idx.t), N, Hh, W, C_, dt, st), "pool_fwd")
        y.host(), idx.host()
        assert torch.equal(y.t.cpu().float(), to_nhwc(yw))
        assert torch.equal(idx.t.cpu(), to_nhwc(code))
        g, rows = H.Guarded((N, Hh, W, C_), td), H.rows_buf(nrows, C_)
        check(lib.gdrn_maxpool_bwd(ptr(dyd), ptr(idx.t), ptr(xd), ptr(dev["scale"]), ptr(dev["shift"]), ptr(g.t), N, Hh, W, C_, ptr(dev["mean"]), ptr(dev["invstd"]),
                                   ptr(rows), dt, st), "pool_bwd(rows)")
        g.host()
        gw = to_nhwc(t.grad)
        assert torch.equal(g.t.cpu().float(), gw)
        xw = to_nhwc(x)
        want = torch.stack([gw.sum((0, 1, 2)), (gw * (xw - k["mean"]) * k["invstd"]).sum((0, 1, 2))])
        assert float(want.abs().max()) < 2 ** 23
        H.assert_same(H.rows_total(rows, nrows), want.double().numpy(), "pool row totals")

    def test_bounded_generic_upsample_second_grid_stride_trip(H):
        """the generic forward kernel (C = 24: three channel vectors) past the 4096-workgroup cap: 2 x 420 x 420 x 3 = 1,058,400 vectors"""
        assert 2 * 420 * 420 * 3 > 4096 * 256
        run_upsample(H, BF16, 2, 210, 210, 24, seed=6400, parts=("fwd",))

    def test_bounded_upsample_bwd_second_grid_stride_trip(H):
        """gdrn_upsample2x_bwd past the cap: 2 x 129 x 129 x 32 = 1,065,024 vectors"""
        assert 2 * 129 * 129 * 32 > 4096 * 256
        run_upsample(H, BF16, 2, 129, 129, 256, seed=6500, parts=("bwd",))

    def test_exact_leaky_and_casts_second_grid_stride_trip(H):
        """ew_grid's cap in gdrn_leaky_bwd (1,048,579 vectors) and the casts (1,048,583 elements, one per thread): the last 3 / 7 come in a second trip"""
        lib, st = cabi.load(BF16), H.stream()
        n = 8 * 1048579
        y, dy = ints(6600, (n,), -3, 3), ints(6601, (n,), -2, 2)
        dx = H.Guarded((n,), HT)
        yd, dyd = y.to(H.DEV).to(HT), dy.to(H.DEV).to(HT)
        check(lib.gdrn_leaky_bwd(ptr(dyd), ptr(yd), ptr(dx.t), n, BF16, st), "leaky_bwd")
        dx.host()
        assert torch.equal(dx.t.cpu(), torch.where(y > 0, dy, torch.tensor(0.1) * dy).to(HT))
        n = 1048583
        src = torch.from_numpy(np.random.default_rng(6602).standard_normal(n).astype(np.float32))
        sd = src.to(H.DEV)
        d16, back = H.Guarded((n,), HT), H.Guarded((n,), torch.float32)
        check(lib.gdrn_cast_from_f32(ptr(sd), ptr(d16.t), n, BF16, st), "cast_from_f32")
        check(lib.gdrn_cast_to_f32(ptr(d16.t), ptr(back.t), n, BF16, st), "cast_to_f32")
        d16.host(), back.host()
        assert torch.equal(d16.t.cpu(), src.to(HT)) and torch.equal(back.t.cpu(), src.to(HT).float())

    def test_exact_bias_grad_regrid(H):
        """gdrn_bias_grad re-grids above 1024 workgroups (rows > 16384 row passes): cs = C = 1024, 32771 rows, every column total the exact integer"""
        lib, st = cabi.load(BF16), H.stream()
        cs, rows = 1024, 32771
        assert rows > 16384 * (256 // (cs // 8))
        d = ints(6700, (rows, cs), -2, 2)
        dd = d.to(H.DEV).to(HT)
        db = H.Guarded((cs,), torch.float32)
        check(lib.gdrn_bias_grad(ptr(dd), cs, rows, cs, ptr(db.t), BF16, st), "bias_grad")
        H.assert_same(db.host(), d.sum(0).double().numpy(), "bias_grad column totals")
