"""Pins tests/head_host.py -- the fp64 yardstick of the head-tail, map-loss and fused head-conv kernel tests -- without a GPU: its tail, losses and
backward replay equal fp64 autograd of oracle.gdrn_oracle.gdrn_loss plus the tail glue, an independent fp32 evaluation (torch on the CPU) sits
inside HALF of every bound, and every bound has teeth: a reference perturbed in one place fails hiputil.assert_within at exactly that index."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_host as R
import hiputil as H
import norm_host as NH
from oracle import gdrn_oracle as O

CASES = [(N, HW, nreg) for (N, HW) in R.SMALL for nreg in (R.GENERIC_NREG + [64]) if (N, HW) != (3, 1023) or nreg in (17, 64)]
T = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def autograd(a, dt=torch.float64, with_dpnp=True):
    """the repository's oracle on the case's arrays: (pnp [M][C], losses [5], d_head [M][C]) by torch.autograd in dtype dt"""
    N, HW, nreg, M = a["N"], a["HW"], a["nreg"], a["M"]
    C = nreg + 5
    head = T(a["head"][:, :C], dt).requires_grad_(True)
    h4 = head.view(N, HW, C).permute(0, 2, 1)[..., None]                    # [N][C][HW][1]
    mask, cx, cy, cz, region = h4[:, :1], h4[:, 1:2], h4[:, 2:3], h4[:, 3:4], h4[:, 4:]
    ext = T(a["extents"], dt)
    batch = dict(roi_mask_visib=T(a["mvis"], dt).view(N, HW, 1), roi_xyz=T(a["gt_xyz"], dt)[..., None], roi_mask_trunc=T(a["mtr"], dt).view(N, HW, 1),
                 roi_region=torch.from_numpy(a["gt_region"]).view(N, HW, 1), ego_rot=torch.eye(3, dtype=dt).expand(N, 3, 3),
                 roi_points=torch.zeros(N, 1, 3, dtype=dt), roi_extent=ext, roi_trans_ratio=torch.zeros(N, 3, dtype=dt))
    L = O.gdrn_loss(mask, cx, cy, cz, region, batch["ego_rot"], torch.zeros(N, 3, dtype=dt), batch)
    xyz = (torch.cat([cx, cy, cz], 1) - 0.5) * ext.view(N, 3, 1, 1)
    pnp = torch.cat([xyz, T(a["coord2d"], dt)[..., None], F.softmax(region[:, 1:], dim=1)], 1)
    ls = torch.stack([L[k] for k in ("loss_coor_x", "loss_coor_y", "loss_coor_z", "loss_mask", "loss_region")])
    tot = (T(a["gw"], dt) * ls).sum()
    if with_dpnp:
        tot = tot + (pnp * T(a["d_pnp"], dt).view(N, HW, C).permute(0, 2, 1)[..., None]).sum()
    tot.backward()
    flat = lambda t: t.detach()[..., 0].permute(0, 2, 1).reshape(M, C).numpy()
    return flat(pnp), ls.detach().numpy(), head.grad.numpy()


def half(ref, b32, kind):
    """half of the bound's arithmetic part (the fp32 bound); a 16-bit store's own rounding u_T |ref| comes on top in full: it alone can use all of it"""
    if kind == "fp32":
        return 0.5 * b32
    u = NH.U[kind]
    return np.maximum(u * np.abs(ref), NH.TINY[u]) + 0.5 * b32


def offenders(got, ref, bnd):
    """the indices hiputil.assert_within objects to (it must object exactly when there are any)"""
    bad = np.argwhere(~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= np.broadcast_to(bnd, np.shape(ref))))
    try:
        H.assert_within(got, ref, bnd, "perturbed")
        raised = False
    except AssertionError:
        raised = True
    assert raised == (len(bad) > 0)
    return [tuple(int(v) for v in i) for i in bad]


@pytest.mark.parametrize("N,HW,nreg,masked", [c + (False,) for c in CASES] + [c + (True,) for c in CASES if c[:2] == (1, 16)])
def test_references_equal_fp64_autograd_of_the_oracle(N, HW, nreg, masked):
    c = R.case(N, HW, nreg, "fp32", masked)
    pnp, ls, dh = autograd(c.a)
    np.testing.assert_allclose(c.p64, pnp, rtol=0, atol=1e-12)
    np.testing.assert_allclose(c.losses, ls, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(c.bwd(c.p64, True)["d"], dh, rtol=0, atol=1e-12 * max(1.0, float(np.abs(dh).max())))
    np.testing.assert_allclose(c.bwd(None, False)["d"], autograd(c.a, with_dpnp=False)[2], rtol=0, atol=1e-12)
    if masked:
        assert c.den == 1.0 and abs(c.tot[4] - 16 * np.log(nreg + 1.0)) < 1e-12 and not c.tot[:3].any()


def test_the_seeded_rows_hold_every_edge():
    for (N, HW) in R.SMALL + R.FAST_SHAPES[2:3]:
        a = R.case(N, HW, 64).a
        z = a["head"][:, 4:69].astype(np.float64)
        spread = z.max(1) - z.min(1)
        vis = a["mvis"] > 0
        assert (spread > 55).any() and (spread == 0).any() and (z.min(1) > 70).any() and ((z == -80).any(1) & (z.max(1) > -10)).any()
        assert {0, 1, 63, 64} <= set(a["gt_region"][vis].tolist()) and (~vis).any()
        assert (a["head"][:, 0] == a["mtr"]).any()
        g = a["gt_xyz"].transpose(0, 2, 1).reshape(-1, 3)
        assert all((a["head"][vis, 1 + c_] == g[vis, c_]).any() for c_ in range(3))
        # without the max subtraction expf overflows on the offset rows: the edge is real
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(a["head"][:, 4:69].astype(np.float32) * 1.2)).any()


@pytest.mark.parametrize("N,HW,nreg", CASES)
@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_an_independent_fp32_evaluation_sits_inside_half_of_every_bound(N, HW, nreg, kind):
    c = R.case(N, HW, nreg, kind)
    a = c.a
    pnp, ls, dh = autograd(a, torch.float32)
    st = lambda v: NH.store(v, kind)
    b, _ = R.tail_bound(c.p64, c.p32, c.mag_xyz, kind)
    hb = half(c.p64, R.tail_bound(c.p64, c.p32, c.mag_xyz, "fp32")[0], kind)
    cols = [0, 1, 2] + list(range(5, nreg + 5))
    assert (hb[:, cols] <= b[:, cols]).all()
    H.assert_within(st(pnp)[:, cols], c.p64[:, cols], hb[:, cols], "tail")
    H.assert_same(st(pnp)[:, 3:5], st(c.p64[:, 3:5]), "coord2d copies")
    # the totals, a lane's carry replayed as sequential fp32 adds over pixel pairs (carry = 2)
    t32 = torch.from_numpy(np.ascontiguousarray(c.t32))
    pairs = F.pad(t32, (0, 0, 0, c.M % 2)).view(-1, 2, 6)
    tot32 = (pairs[:, 0] + pairs[:, 1]).double().sum(0).numpy()
    tb, _ = R.totals_bound(c.t64, c.t32, c.a_ce, 2)
    H.assert_within(tot32, c.tot, 0.5 * tb, "totals", exact=np.arange(6) == 5)
    H.assert_within(ls, c.losses, 0.5 * R.losses_bound(tb, c.tot, c.M), "losses")
    # the backward pass from the stored fp64 tail
    pst = st(c.p64)
    r64, r32 = c.bwd(pst, True), c.bwd(pst, True, np.float32)
    bb, _ = R.tail_bwd_bound(r64, r32, kind, True)
    hbb = half(r64["d"], R.tail_bwd_bound(r64, r32, "fp32", True)[0], kind)
    assert (hbb[:, 4:] <= bb[:, 4:]).all()
    # torch in fp32: the losses' gradient by autograd, the attention chain from the STORED tail (what the kernel reads; autograd would
    # differentiate its own fp32 softmax instead) with torch's fp32 operations
    g32 = torch.from_numpy(autograd(a, torch.float32, False)[2].copy())
    s32, d32 = T(pst, torch.float32), T(a["d_pnp"], torch.float32)
    g32[:, 5:] += s32[:, 5:] * (d32[:, 5:] - (s32[:, 5:] * d32[:, 5:]).sum(1, keepdim=True))
    g32[:, 1:4] += d32[:, :3] * T(a["extents"], torch.float32)[torch.arange(c.M) // HW]
    for name, g in (("numpy replay", st(r32["d"])), ("torch", st(g32.numpy()))):
        H.assert_within(g[:, 1:], r64["d"][:, 1:], hbb[:, 1:], f"d_head {name}")
    ex = R.tail_bwd_exact(a["head"], a["gt_xyz"], a["mvis"], a["mtr"], a["gw"], c.den, HW, kind)
    # (a replay of the kernels' own operations -- gmask * (float)(1 / M), not torch's gmask / M: held to the fp64 value, its sign pattern exactly)
    H.assert_same(np.sign(ex), np.sign(c.bwd(None, False)["d"][:, :4]), "sign pattern")
    r0 = c.bwd(None, False)
    H.assert_within(ex, r0["d"][:, :4], np.maximum(NH.U[kind] * np.abs(r0["d"][:, :4]), 1e-30) + 3 * R.EPS32 * np.abs(r0["d"][:, :4]), "sign constants")


def test_each_bound_has_teeth():
    N, HW, nreg, kind = 3, 80, 64, "fp32"
    c = R.case(N, HW, nreg, kind)
    a = c.a
    b, _ = R.tail_bound(c.p64, c.p32, c.mag_xyz, kind)
    # one class of one pixel off by 4 bounds
    got = c.p64.copy()
    got[HW - 1, 5 + 17] += 4 * b[HW - 1, 5 + 17]
    assert offenders(got, c.p64, b) == [(HW - 1, 22)]
    # extents of the neighbouring RoI for the first pixel of a RoI
    wrong = c.p64.copy()
    wrong[HW, :3] = (R.f64(a["head"])[HW, 1:4] - 0.5) * R.f64(a["extents"])[0]
    assert offenders(wrong, c.p64, b) == [(HW, 0), (HW, 1), (HW, 2)]
    # class 0 included in the attention softmax
    sm0 = c.p64.copy()
    sm0[:, 5:] = R.softmax(a["head"][:, 4:69], np.float64)[:, 1:]
    bad = offenders(sm0, c.p64, b)
    assert bad and all(k >= 5 for _, k in bad) and len({m for m, _ in bad}) > c.M // 2
    pst = c.p64
    r64, r32 = c.bwd(pst, True), c.bwd(pst, True, np.float32)
    bb, _ = R.tail_bwd_bound(r64, r32, kind, True)
    att0 = R.tail_bwd(a["head"], pst, a["d_pnp"], a["extents"], a["gt_xyz"], a["mvis"], a["mtr"], a["gt_region"], a["gw"], c.den, nreg, HW, att0=True)
    bad = offenders(att0["d"], r64["d"], bb)
    assert bad and all(k >= 4 for _, k in bad)
    # the target class of one visible pixel off by one
    m = int(np.nonzero(a["mvis"] > 0)[0][7])
    t0 = int(a["gt_region"][m])
    greg = a["gt_region"].copy()
    greg[m] = (t0 + 1) % 65
    off = R.tail_bwd(a["head"], pst, a["d_pnp"], a["extents"], a["gt_xyz"], a["mvis"], a["mtr"], greg, a["gw"], c.den, nreg, HW)
    assert offenders(off["d"], r64["d"], bb) == sorted([(m, 4 + t0), (m, 4 + (t0 + 1) % 65)])
    tb, _ = R.totals_bound(c.t64, c.t32, c.a_ce, 1)
    tot_off = R.map_sums(a["head"], a["gt_xyz"], a["mvis"], a["mtr"], greg, nreg)[0]
    assert offenders(tot_off, c.tot, tb) == [(4,)]
    # one element of d_head off by 4 bounds
    g2 = r64["d"].copy()
    g2[m, 4 + 64] -= 4 * bb[m, 68]
    assert offenders(g2, r64["d"], bb) == [(m, 68)]
    # den without the clamp: the all-masked batch
    cm = R.case(1, 16, 64, kind, True)
    tbm, _ = R.totals_bound(cm.t64, cm.t32, cm.a_ce, 1)
    assert offenders(R.losses(cm.tot, cm.M, clamp=False), cm.losses, R.losses_bound(tbm, cm.tot, cm.M)) == [(0,), (1,), (2,), (4,)]
    noclamp = R.tail_bwd(cm.a["head"], None, None, cm.a["extents"], cm.a["gt_xyz"], cm.a["mvis"], cm.a["mtr"], cm.a["gt_region"], cm.a["gw"], 0.0, 64, 16)
    rm, rm32 = cm.bwd(None, False), cm.bwd(None, False, np.float32)
    bad = offenders(noclamp["d"], rm["d"], R.tail_bwd_bound(rm, rm32, kind, False)[0])
    assert len(bad) == 16 * 68 and all(k >= 1 for _, k in bad)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_fused_references_and_their_inputs(kind):
    M = 96
    x, w, bias = R.conv_inputs(11, M, kind, 264, 128)
    y, mag, yb = R.conv_logits(x, w, bias)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v[:, :256])).float()
    y32 = (t(x) @ t(w[:69]).t() + torch.from_numpy(bias)).numpy()
    H.assert_within(y32, y, 0.5 * yb, "logits in fp32")
    assert np.isfinite(y).all() and (np.abs(x[:, 256:]) > 5e4).all() and (np.abs(w[69:]) > 5e4).all()
    yo = y.copy()
    yo[5, 68] += 4 * yb[5, 68]
    assert offenders(yo, y, yb) == [(5, 68)]
    # the data gradient: fp32 torch inside half the bound, the marginal share of the fp64 reference under 1e-3 at every shape of the GPU module
    for (N, HW) in R.DGRAD_SHAPES[:3]:
        M = N * HW
        d = R.dgrad_inputs(R.seed_of(N, HW, 64), M, kind, 96, 128, 264)
        r = R.out_dgrad(d["dy"], d["wd"], d["raw"], d["mean"], d["invstd"], d["scale"], d["shift"], terms=2)
        assert r["marginal"].mean() <= 1e-3 and 0.3 < r["keep"].mean() < 0.7
        g32 = torch.from_numpy(d["dy"][:, :96]).float() @ torch.from_numpy(d["wd"][:, :96]).float().t()
        raw32 = torch.from_numpy(d["raw"][:, :256]).float()
        keep32 = raw32 * torch.from_numpy(d["scale"]) + torch.from_numpy(d["shift"]) > 0
        gm32 = torch.where(keep32, g32, torch.zeros(()))
        ok = ~r["marginal"]
        H.assert_within(np.where(ok, NH.store(gm32.numpy(), kind), r["g"]), r["g"], half(r["g"], r["gbound"], kind), "dx in fp32", exact=~r["keep"] & ok)
        # a lane's sums: pixel pairs sequentially in fp32, then fp64
        pad = (0, 0, 0, M % 2)
        s1 = F.pad(gm32, pad).view(-1, 2, 256)
        t2 = F.pad(gm32 * (raw32 - torch.from_numpy(d["mean"])) * torch.from_numpy(d["invstd"]), pad).view(-1, 2, 256)
        H.assert_within((s1[:, 0] + s1[:, 1]).double().sum(0).numpy(), r["s1"], 0.5 * r["b1"], "sum 1")
        H.assert_within((t2[:, 0] + t2[:, 1]).double().sum(0).numpy(), r["s2"], 0.5 * r["b2"], "sum 2")
        bad1 = r["s1"].copy()
        bad1[200] += 4 * r["b1"][200]
        assert offenders(bad1, r["s1"], r["b1"]) == [(200,)]
    for (N, HW) in R.DGRAD_SHAPES[3:]:
        d = R.dgrad_inputs(R.seed_of(N, HW, 64), N * HW, kind)
        arg = R.f64(d["scale"])[None] * d["raw"][:, :256] + R.f64(d["shift"])[None]
        assert (np.abs(arg) <= 4 * R.EPS32 * (np.abs(R.f64(d["scale"])[None] * d["raw"][:, :256]) + np.abs(R.f64(d["shift"])[None]))).mean() <= 1e-3
