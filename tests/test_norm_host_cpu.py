"""Pins the fp64 numpy references of tests/norm_host.py (the yardstick of tests/test_norm_edges_gpu.py) without a GPU:
each one equals torch autograd in fp64 on the CPU to 1e-12 relative; the bilinear pair is an adjoint pair; torch's own fp32 CPU evaluation of
each operation stays within HALF the derived per-element bound on the same operands (a guard against a wrong derivation of k / A -- the bounds
are derived, not measured on the device); and the seeded inputs of the GPU cases leave no element in the sets that may be left out of the exact
comparisons (ReLU signs within fp32 rounding of 0, pool windows whose two best distinct candidates are within rounding of each other)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_host as R

KINDS = ["fp32", "bf16", "fp16"]
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(R.f64(a)))


def nchw(a):
    return t64(a).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def relmax(a, b):
    a, b = R.f64(a), R.f64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def half_bound_ratio(got32, ref, A, k):
    """max over the elements of |fp32 evaluation - ref| / (half the fp32 bound); elements with a zero bound must be exact"""
    b = 0.5 * R.bound(ref, A, k, R.U["fp32"])
    err = np.abs(R.f64(got32) - ref)
    assert np.all(err[b == 0] == 0)
    return float((err[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0


def test_store_is_torchs_rounding():
    a = np.random.default_rng(0).standard_normal(20000).astype(np.float32) * np.float32(37.0)
    a[:6] = [1.00390625, 1.01171875, 0.0, -0.0, 65504.0, 3.0e-5]   # bf16 ties to even (down, up), zeros, fp16 max, an fp16 subnormal
    for kind in KINDS:
        assert np.array_equal(R.store(a, kind), torch.from_numpy(a).to(TD[kind]).double().numpy()), kind


# ---------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("npix", [1, 3, 433])
def test_bn_references_equal_autograd(C, npix):
    x = t64(R.operand(1, (npix, C), "bf16", 2.0, 0.5)).requires_grad_(True)
    res = t64(R.operand(2, (npix, C), "bf16"))
    dy = t64(R.operand(3, (npix, C), "bf16"))
    scale, shift = R.channel_consts(4, C)
    for relu in (False, True):
        for rs in (None, res):
            y = x * t64(scale) + t64(shift) + (0 if rs is None else rs)
            y = F.relu(y) if relu else y
            assert relmax(R.bn_apply(x.detach().numpy(), scale, shift, None if rs is None else rs.numpy(), relu), y.detach().numpy()) < 1e-12
    # training-mode BatchNorm -> ReLU backward through the sums, the coefficients and the apply pass (both mask kinds describe the same mask)
    gam = t64(np.float32(0.5) + np.random.default_rng(5).random(C).astype(np.float32)).requires_grad_(True)
    bet = t64(np.random.default_rng(6).random(C).astype(np.float32) - np.float32(0.5)).requires_grad_(True)
    if npix > 1:
        eps = float(np.float32(1e-5))
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        yt = F.relu(F.batch_norm(x, rm, rv, gam, bet, True, float(np.float32(0.1)), eps))
        yt.backward(dy)
        xn = x.detach().numpy()
        fin = R.bn_finalize(xn.sum(0), (xn * xn).sum(0), npix, gam.detach().numpy(), bet.detach().numpy(), eps, np.zeros(C), np.ones(C), 0.1)
        assert relmax(fin["running_mean"], rm.numpy()) < 1e-12 and relmax(fin["running_var"], rv.numpy()) < 1e-12
        assert relmax(R.bn_apply(xn, fin["scale"], fin["shift"], None, True), yt.detach().numpy()) < 1e-12
        for kw in (dict(ymask=yt.detach().numpy()), dict(x=xn, msc=fin["scale"], msh=fin["shift"])):
            g, keep = R.bn_mask(dy.numpy(), **kw)
            assert np.array_equal(keep, yt.detach().numpy() > 0)
            s1, s2 = R.bn_bwd_sums(g, xn, fin["mean"], fin["invstd"])
            a, b, c, dgamma, dbeta = R.bn_bwd_coef(s1, s2, npix, gam.detach().numpy(), fin["mean"], fin["invstd"])
            assert relmax(R.bn_bwd_apply(g, xn, a, b, c), x.grad.numpy()) < 1e-12
            assert relmax(dgamma, gam.grad.numpy()) < 1e-12 and relmax(dbeta, bet.grad.numpy()) < 1e-12
    # count = 1: the unbiased-variance guard leaves the variance as it is
    fin1 = R.bn_finalize(np.ones(C), np.ones(C), 1, np.ones(C), np.zeros(C), 1e-5, np.zeros(C), np.ones(C), 0.1)
    assert np.all(fin1["var"] == 0) and np.allclose(fin1["running_var"], 0.9, rtol=1e-7)


# ---------------------------------------------------------------------------------------------- pool
def torch_pool(x, scale, shift, dy=None):
    z = (nchw(x) * t64(scale).view(1, -1, 1, 1) + t64(shift).view(1, -1, 1, 1)).requires_grad_(True)
    y, ind = F.max_pool2d(F.relu(z), 3, 2, 1, return_indices=True)
    W = x.shape[2]
    Ho, Wo = y.shape[2:]
    iy, ix = ind // W, ind % W
    oy, ox = torch.arange(Ho).view(1, 1, -1, 1), torch.arange(Wo).view(1, 1, 1, -1)
    code = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))
    g = None
    if dy is not None:
        y.backward(nchw(dy))
        g = nhwc(z.grad)
    return nhwc(y), nhwc(code).astype(np.uint8), g


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("hw", R.POOL_HW)
def test_pool_reference_equals_autograd_and_torchs_indices(hw, integer):
    for N, C in ((1, 8), (3, 64)):
        x, scale, shift = R.pool_inputs(11, N, hw[0], hw[1], C, "bf16", integer)
        dy = R.operand(13, (N, hw[0] // 2, hw[1] // 2, C), "bf16")
        y, code = R.bn_relu_maxpool(x, scale, shift)
        yt, ct, gt = torch_pool(x, scale, shift, dy)
        assert relmax(y, yt) < 1e-12 and np.array_equal(code, ct)
        assert relmax(R.maxpool_bwd(dy, code, x, scale, shift), gt) < 1e-12
        assert code.max() <= 8
        if integer:   # the integer levels do make positive ties common: windows in which more than one tap attains a positive maximum
            ties = ((R._pool_taps(R.bn_apply(x, scale, shift, None, True), -np.inf) == y).sum(0) > 1) & (y > 0)
            assert ties.mean() > 0.05, ties.mean()
        # fp32 evaluation inside half the bound; same tap codes
        z32 = F.relu(torch.from_numpy(x.astype(np.float32)) * torch.from_numpy(scale) + torch.from_numpy(shift))
        y32 = F.max_pool2d(z32.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
        assert half_bound_ratio(y32, y, R.bn_relu_maxpool_mag(x, scale, shift), R.K_POOL) <= 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_seeded_pool_and_mask_inputs_leave_nothing_out(kind):
    """the GPU cases' seeded inputs: no ReLU sign within fp32 rounding of 0, no window whose two best DISTINCT candidates are within rounding"""
    for (H, W) in R.POOL_HW:
        for N in (1, 3):
            for C in R.POOL_C:
                for integer in (False, True):
                    x, scale, shift = R.pool_inputs(1000 + H * 37 + W, N, H, W, C, kind, integer)
                    assert not R.affine_sign_margin(x, scale, shift).any(), (H, W, N, C, integer)
                    gap, mag = R.pool_top2_gap(x, scale, shift)
                    assert not ((gap > 0) & (gap <= 2.0 ** -22 * mag)).any(), (H, W, N, C, integer)
    for C in R.BN_C:
        for npix in R.bn_npix(C, kind):
            x = R.operand(2000 + npix, (npix, C), kind, 2.0, 0.5)
            scale, shift = R.channel_consts(2001 + npix, C)
            assert not R.affine_sign_margin(x, scale, shift).any(), (C, npix)


# ---------------------------------------------------------------------------------------------- bilinear
HW16 = R.UP_HW + [(2, 3), (4, 4), (5, 2), (9, 9), (12, 7), (31, 32), (128, 4), (4, 128)]


@pytest.mark.parametrize("hw", HW16)
def test_bilinear_pair_equals_autograd_is_adjoint_and_fp32_sits_inside_half_the_bound(hw):
    H, W = hw
    N, C = 2, 8
    x = R.operand(21, (N, H, W, C), "bf16")
    dy = R.operand(22, (N, 2 * H, 2 * W, C), "bf16")
    xt = nchw(x).requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    yt.backward(nchw(dy))
    y, dx = R.upsample2x(x), R.upsample2x_adjoint(dy)
    assert relmax(y, nhwc(yt)) < 1e-12 and relmax(dx, nhwc(xt.grad)) < 1e-12
    assert abs((y * dy).sum() - (x * dx).sum()) <= 1e-12 * np.abs(y * dy).sum()
    assert np.allclose(R.up_matrix(H).sum(1), 1.0, atol=1e-15) and R.up_matrix(H)[0, 0] == 1.0 and R.up_matrix(H)[-1, -1] == 1.0
    x32 = torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2).requires_grad_(True)
    y32 = F.interpolate(x32, scale_factor=2, mode="bilinear", align_corners=True)
    y32.backward(torch.from_numpy(dy.astype(np.float32)).permute(0, 3, 1, 2))
    k = R.k_bilinear(H, W)
    rf = half_bound_ratio(nhwc(y32), y, np.broadcast_to(R.upsample_mag(x), y.shape), k)
    rb = half_bound_ratio(nhwc(x32.grad), dx, np.broadcast_to(R.upsample_mag(dy, 4.0), dx.shape), k)
    print(f"bilinear {hw}: torch fp32 at {rf:.3f} (forward) / {rb:.3f} (backward) of half the bound")
    assert rf <= 1.0 and rb <= 1.0


# ---------------------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("case", [(128, 32, 49), (64, 1, 36), (64, 2, 49), (128, 2, 36), (256, 1, 49), (512, 4, 36)])
def test_groupnorm_reference_equals_autograd_and_fp32_sits_inside_half_the_bound(case):
    C, G, HW = case
    N, eps = 3, float(np.float32(1e-5))
    x = R.operand(31, (N, HW, C), "bf16", 1.5, 0.3)
    dy = R.operand(32, (N, HW, C), "bf16")
    gam = (np.float32(0.5) + np.random.default_rng(33).random(C).astype(np.float32))
    bet = (np.random.default_rng(34).random(C).astype(np.float32) - np.float32(0.5))
    xt = t64(x).permute(0, 2, 1).contiguous().requires_grad_(True)    # [N, C, HW]
    gt, bt = t64(gam).requires_grad_(True), t64(bet).requires_grad_(True)
    yt = F.relu(F.group_norm(xt, G, gt, bt, eps))
    yt.backward(t64(dy).permute(0, 2, 1))
    y, mean, rstd = R.gn_relu_fwd(x, gam, bet, G, eps)
    assert relmax(y, yt.detach().permute(0, 2, 1).numpy()) < 1e-12
    dx, dgamma, dbeta = R.gn_relu_bwd(dy, y, x, gam, mean, rstd, G)
    assert relmax(dx, xt.grad.permute(0, 2, 1).numpy()) < 1e-12
    assert relmax(dgamma, gt.grad.numpy()) < 1e-12 and relmax(dbeta, bt.grad.numpy()) < 1e-12
    x32 = torch.from_numpy(x.astype(np.float32)).permute(0, 2, 1).contiguous()
    y32 = F.relu(F.group_norm(x32, G, torch.from_numpy(gam), torch.from_numpy(bet), eps)).permute(0, 2, 1).numpy()
    # (torch's fp32 statistics carry their own error: allowed for as the 1 ulp of mean / rstd the GPU test grants the kernel, inside K_GN_FWD)
    assert half_bound_ratio(y32, y, R.gn_relu_fwd_mag(x, gam, bet, mean, rstd, G), R.K_GN_FWD) <= 1.0


# ---------------------------------------------------------------------------------------------- element-wise, sums
def test_elementwise_references_and_fp32_inside_half_the_bound():
    n = 4099
    y = R.operand(41, (n,), "bf16")
    y[:4] = [0.0, -0.0, 2.0 ** -133, -(2.0 ** -133)]
    dy = R.operand(42, (n,), "bf16")
    yt = t64(y)
    assert relmax(R.leaky_bwd(dy, y), (t64(dy) * torch.where(yt > 0, 1.0, R.SLOPE)).numpy()) < 1e-15
    d32 = (torch.from_numpy(dy.astype(np.float32)) * torch.where(torch.from_numpy(y.astype(np.float32)) > 0, 1.0, 0.1)).numpy()
    assert half_bound_ratio(d32, R.leaky_bwd(dy, y), R.SLOPE * np.abs(dy) * (y <= 0), R.K_LEAKY) <= 1.0
    a = R.operand(43, (333, 128), "bf16")
    assert relmax(R.col_sums(a, 69), t64(a)[:, :69].sum(0).numpy()) < 1e-12
    # BN apply / backward apply in fp32 (x * scale rounded, then + shift, then + res: one rounding more than the kernel's fma)
    C, npix = 64, 433
    x, res, g = R.operand(44, (npix, C), "fp32", 2.0, 0.5), R.operand(45, (npix, C), "fp32"), R.operand(46, (npix, C), "fp32")
    scale, shift = R.channel_consts(47, C)
    f32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32))
    y32 = torch.addcmul(f32(shift), f32(x), f32(scale)) + f32(res)
    assert half_bound_ratio(y32.numpy(), R.bn_apply(x, scale, shift, res), R.bn_apply_mag(x, scale, shift, res), R.K_BN_APPLY) <= 1.0
    a_, b_, c_ = (np.random.default_rng(48 + i).standard_normal(C).astype(np.float32) for i in range(3))
    d32 = torch.addcmul(torch.addcmul(f32(c_), f32(b_), f32(x)), f32(a_), f32(g))
    assert half_bound_ratio(d32.numpy(), R.bn_bwd_apply(g, x, a_, b_, c_), R.bn_bwd_apply_mag(g, x, a_, b_, c_), R.K_BN_BWD_APPLY) <= 1.0
    # sums: a sequential fp32 walk of n terms, held to k_sum(n)
    mean, invstd = (np.random.default_rng(50).random(C).astype(np.float32) - np.float32(0.5)), (np.float32(0.5) + np.random.default_rng(51).random(C).astype(np.float32))
    s1, s2 = R.bn_bwd_sums(g, x, mean, invstd)
    m1, m2 = R.bn_bwd_sums_mag(g, x, mean, invstd)
    t1 = f32(g).sum(0).numpy()
    t2 = (f32(g) * (f32(x) - f32(mean)) * f32(invstd)).sum(0).numpy()
    assert half_bound_ratio(t1, s1, m1, R.k_sum(npix)) <= 1.0 and half_bound_ratio(t2, s2, m2, R.k_sum(npix)) <= 1.0


# ---------------------------------------------------------------------------------------------- the remaining derived k, each against plain fp32
def f32(v):
    return np.asarray(v, dtype=np.float32)


def fp32_grid_walk(terms, rpp, rpb):
    """column sums of fp32 terms [rows, C] the way the row-walking kernels form them, every addition in fp32 and sequential: a workgroup takes rpb
    rows, row lane l adds rows l, l + rpp, ... in order, the lanes are added in order, the workgroups are added in order"""
    terms = f32(terms)
    total = np.zeros(terms.shape[1], dtype=np.float32)
    for r0 in range(0, terms.shape[0], rpb):
        blk = terms[r0:r0 + rpb]
        acc = np.zeros_like(total)
        for lane in range(min(rpp, blk.shape[0])):
            s = np.zeros_like(total)
            for row in blk[lane::rpp]:
                s = s + row
            acc = acc + s
        total = total + acc
    return total


def ratio(err, bnd):
    """max |err| / (half of bnd); a zero bound demands an exact result"""
    err, bnd = np.abs(R.f64(err)), 0.5 * R.f64(bnd)
    assert np.all(err[bnd == 0] == 0)
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if np.any(bnd > 0) else 0.0


@pytest.mark.parametrize("hw", [(6, 10), (24, 24)])
def test_pool_backward_fp32_sits_inside_half_the_bound(hw):
    N, C = 3, 64
    x, scale, shift = R.pool_inputs(61, N, hw[0], hw[1], C, "fp32", False)
    dy = R.operand(62, (N, hw[0] // 2, hw[1] // 2, C), "fp32")
    _, code = R.bn_relu_maxpool(x, scale, shift)
    z = (torch.from_numpy(f32(x)).permute(0, 3, 1, 2) * torch.from_numpy(scale).view(1, -1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1)).requires_grad_(True)
    F.max_pool2d(F.relu(z), 3, 2, 1).backward(torch.from_numpy(f32(dy)).permute(0, 3, 1, 2))
    gref = R.maxpool_bwd(dy, code, x, scale, shift)
    assert half_bound_ratio(nhwc(z.grad), gref, R.maxpool_bwd(dy, code, x, scale, shift, mag=True), R.K_POOL_BWD) <= 1.0


@pytest.mark.parametrize("C", [8, 512])
def test_bn_coef_and_finalize_fp32_sit_inside_half_the_bound(C):
    rg = np.random.default_rng(63)
    s1, s2 = rg.standard_normal(C) * 40.0, rg.standard_normal(C) * 40.0     # fp64 totals, as the kernels have them
    gamma, mean, invstd = f32(0.5 + rg.random(C)), f32(rg.random(C) - 0.5), f32(0.5 + rg.random(C))
    gamma[1::4] *= -1
    npix = 1283
    inv_n = np.float32(1.0 / npix)
    m1, m2 = f32(s1) * inv_n, f32(s2) * inv_n
    a = gamma * invstd
    b = -a * invstd * m2
    c = -a * m1 - b * mean
    ra, rb, rc, _, _ = R.bn_bwd_coef(s1, s2, npix, gamma, mean, invstd)
    ma, mb, mc = R.bn_bwd_coef_mag(s1, s2, npix, gamma, mean, invstd)
    for got, ref, mag in ((a, ra, ma), (b, rb, mb), (c, rc, mc)):
        assert got.dtype == np.float32 and half_bound_ratio(got, ref, mag, R.K_COEF) <= 1.0
    # finalize: fp64 up to mean / invstd, fp32 from there
    xs = rg.standard_normal((64, C)) * 1.5 + 0.3
    beta, rm0, rv0 = f32(rg.random(C) - 0.5), f32(rg.random(C) - 0.5), f32(0.5 + rg.random(C))
    fin = R.bn_finalize(xs.sum(0), (xs * xs).sum(0), 64, gamma, beta, 1e-5, rm0, rv0, 0.1)
    m, istd, mom = f32(fin["mean"]), f32(fin["invstd"]), np.float32(0.1)
    scale = gamma * istd
    shift = beta - m * scale
    rmean = (np.float32(1) - mom) * rm0 + mom * m
    rvar = (np.float32(1) - mom) * rv0 + mom * f32(fin["var"] * 64 / 63)
    assert half_bound_ratio(scale, fin["scale"], np.abs(fin["scale"]), R.K_FINALIZE) <= 1.0
    assert half_bound_ratio(shift, fin["shift"], fin["shift_mag"], R.K_FINALIZE) <= 1.0
    assert half_bound_ratio(rmean, fin["running_mean"], fin["running_mean_mag"], R.K_FINALIZE) <= 1.0
    assert half_bound_ratio(rvar, fin["running_var"], fin["running_var_mag"], R.K_FINALIZE) <= 1.0


def fp32_tree_walk(terms, rpp, walk):
    """one workgroup of bn_bwd_reduce_kernel in fp32: every row lane adds its `walk` rows in order, the rpp / 4 lanes of a wave meet in a
    pairwise (shuffle) tree, the four waves are added in order"""
    terms = f32(terms)
    lanes = []
    for lane in range(rpp):
        s = np.zeros(terms.shape[1], dtype=np.float32)
        for row in terms[lane::rpp][:walk]:
            s = s + row
        lanes.append(s)
    waves = []
    for w in range(4):
        part = lanes[w * (rpp // 4):(w + 1) * (rpp // 4)]
        while len(part) > 1:
            part = [part[i] + part[i + len(part) // 2] for i in range(len(part) // 2)]
        waves.append(part[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


@pytest.mark.parametrize("rpp", [4, 32, 256])
def test_fp32_sums_in_the_kernels_order_sit_inside_half_of_k_sum(rpp):
    """bn_bwd_reduce's sums in fp32 in the kernel's order (a sequential walk of 4 and of 23 rows per thread, shuffle tree, wave adds) against
    k_sum(walk); gdrn_bias_grad's walk (rows, then the lanes and workgroups one after the other) against k_bias"""
    C = 16
    mean, invstd = f32(np.random.default_rng(66).random(C) - 0.5), f32(0.5 + np.random.default_rng(67).random(C))
    for walk in (4, 23):
        npix = walk * rpp
        g, x = R.operand(64 + walk, (npix, C), "fp32"), R.operand(65 + walk, (npix, C), "fp32", 2.0, 0.5)
        s1, s2 = R.bn_bwd_sums(g, x, mean, invstd)
        m1, m2 = R.bn_bwd_sums_mag(g, x, mean, invstd)
        t1 = fp32_tree_walk(g, rpp, walk)
        t2 = fp32_tree_walk(f32(g) * (f32(x) - mean) * invstd, rpp, walk)
        k = R.k_sum(walk)
        assert ratio(t1 - s1, k * R.EPS32 * m1) <= 1.0 and ratio(t2 - s2, k * R.EPS32 * m2) <= 1.0
    if rpp <= 32:
        for rows in (37, 16 * rpp * 2 + 5):
            d = R.operand(68, (rows, C), "fp32")
            tb = fp32_grid_walk(d, rpp, 16 * rpp)
            assert ratio(tb - R.col_sums(d), R.k_bias(rows, rpp) * R.EPS32 * np.abs(d).sum(0)) <= 1.0


@pytest.mark.parametrize("case", [(128, 32, 49), (64, 1, 36), (128, 2, 100), (256, 1, 49), (512, 4, 36)])
def test_groupnorm_backward_fp32_sits_inside_half_of_each_derived_bound(case):
    """dx, dgamma, dbeta evaluated in fp32 with the kernel's order of additions (row lanes, then lanes, then the group's channels, then samples)
    against K_GN_BWD_EW / k_gn_A / k_gn_B / k_gn_dgamma / k_gn_dbeta"""
    C, G, HW = case
    N, cpg = 3, C // G
    rpp = 256 // (R.gn_slab(C, G, 4) // 4)
    x, dy = R.operand(71, (N, HW, C), "fp32", 1.5, 0.3), R.operand(72, (N, HW, C), "fp32")
    gam, bet = f32(0.5 + np.random.default_rng(73).random(C)), f32(np.random.default_rng(74).random(C) - 0.5)
    gam[1::4] *= -1
    y, mean, rstd = R.gn_relu_fwd(x, gam, bet, G, 1e-5)
    mean, rstd = f32(mean), f32(rstd)                      # the fp32 statistics the backward is given
    dref, dgam, dbet = R.gn_relu_bwd(dy, y, x, gam, mean, rstd, G)
    dmag, gmag, bmag = R.gn_relu_bwd(dy, y, x, gam, mean, rstd, G, mag=True)
    shA, shB = R.gn_relu_bwd_shares(dy, y, x, gam, mean, rstd, G)
    dg, db = np.zeros(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
    dx = np.empty((N, HW, C), dtype=np.float32)
    inv_m = np.float32(1.0) / np.float32(HW * cpg)
    for n in range(N):
        mu, rs = np.repeat(mean[n], cpg), np.repeat(rstd[n], cpg)
        g = np.where(y[n] > 0, f32(dy[n]), np.float32(0))
        xh = (f32(x[n]) - mu) * rs
        sb, sg_ = fp32_grid_walk(g, rpp, HW), fp32_grid_walk(g * xh, rpp, HW)
        dg, db = dg + sg_, db + sb
        A, B = np.zeros(G, dtype=np.float32), np.zeros(G, dtype=np.float32)
        for k in range(cpg):
            A = A + sb[k::cpg] * gam[k::cpg]
            B = B + sg_[k::cpg] * gam[k::cpg]
        A, B = np.repeat(A * inv_m, cpg), np.repeat(B * inv_m, cpg)
        dx[n] = rs * (g * gam - A - xh * B)
        assert dx[n].dtype == np.float32
    u = R.U["fp32"]
    assert ratio(dx - dref, R.gn_dx_bound(dref, dmag, shA, shB, HW, rpp, cpg, u)) <= 1.0
    assert ratio(dg - dgam, R.k_gn_dgamma(HW, rpp, N) * R.EPS32 * gmag) <= 1.0
    assert ratio(db - dbet, R.k_gn_dbeta(HW, rpp, N) * R.EPS32 * bmag) <= 1.0
