"""Pins tests/conv_host.py -- the yardstick of tests/test_conv3x3_edges_gpu.py -- without a GPU: its convolution equals F.conv2d and autograd in
fp64; an independent fp32 evaluation (torch on the CPU) sits inside HALF of every bound on every case the GPU module runs (and inside the bound
after its store to the 16-bit format, whose rounding alone may take all of the u |y| term); every mutated
reference leaves its bound, inside the region its defect can reach and nowhere else; the cases have the properties they are listed for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_host as CH

T = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
NCHW = lambda a, dt=torch.float64: T(a, dt).permute(0, 3, 1, 2).contiguous()
OIHW = lambda w, dt=torch.float64: T(w, dt).reshape(w.shape[0], 3, 3, w.shape[2]).permute(0, 3, 1, 2).contiguous()
NHWC = lambda t: t.permute(0, 2, 3, 1).contiguous().double().numpy()


def test_reference_equals_conv2d_and_autograd_in_fp64():
    r = np.random.default_rng(1)
    for B, H, W, Cin, Cout in [(2, 8, 24, 64, 40), (1, 5, 3, 8, 16), (3, 16, 8, 32, 8)]:
        x, w = r.standard_normal((B, H, W, Cin)), r.standard_normal((Cout + 8, 9, Cin))
        bias, add = r.standard_normal(Cout), r.standard_normal((B, H, W, Cout + 4))
        xt = NCHW(x).requires_grad_(True)
        ref = F.conv2d(xt, OIHW(w[:Cout]), None, 1, 1)
        for act, fn in ((0, lambda t: t), (1, F.relu), (2, lambda t: F.leaky_relu(t, CH.SLOPE))):
            y, A, _ = CH.conv(x, w, Cout, bias, add, act)
            want = NHWC(fn(ref.detach() + T(bias).view(1, -1, 1, 1) + NCHW(add[..., :Cout])))
            assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
            assert (A >= np.abs(y) * (1 - 1e-12)).all()
        dy = r.standard_normal((B, H, W, Cout))
        ref.backward(NCHW(dy))
        dx, _, _ = CH.dgrad(dy, w[:Cout])
        assert np.abs(dx - NHWC(xt.grad)).max() <= 1e-12 * np.abs(NHWC(xt.grad)).max()


def _conv32(x, w, Cout):
    return NHWC(F.conv2d(NCHW(x, torch.float32), OIHW(w[:Cout], torch.float32), None, 1, 1))


def _epi32(v, f):
    v = torch.from_numpy(v.astype(np.float32))
    if f.bias is not None:
        v = v + torch.from_numpy(f.bias)
    if f.addend is not None:
        v = v + T(f.addend[..., :v.shape[-1]], torch.float32)
    if f.act == 1:
        v = F.relu(v)
    elif f.act == 2:
        v = torch.where(v > 0, v, np.float32(0.1) * v)
    return v.numpy()


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_fp32_torch_sits_inside_half_of_every_bound(half):
    """the forward, second-generation, probe and statistics cases of the GPU module: output elements and statistics rows"""
    worst = 0.0
    for c in CH.ALL_CASES:
        if half == "fp16" and c["kern"] == "f32":
            continue
        f = CH.fwd(c, half)
        v32 = _conv32(f.x[..., :c["Cin"]], f.w, c["Cout"])
        y32 = _epi32(v32, f)
        ratio = np.abs(y32 - f.y) / f.bound                  # the fp32 value: half the bound; after its store (at most u |y| more): the bound
        assert ratio.max() <= 0.5, (c["id"], ratio.max())
        ratio = np.abs(CH.store(y32, f.out_kind) - f.y) / f.bound
        assert ratio.max() <= 1.0, (c["id"], ratio.max())
        worst = max(worst, ratio.max())
        if f.want_stats:
            mt, nt = CH.tile_of(c["B"], c["H"], c["W"], c["th"], c["tw"]), CH.n_tiles(c["B"], c["H"], c["W"], c["th"], c["tw"])
            rows = np.zeros((nt, 2, c["Cout"]), dtype=np.float32)
            v32f = v32.astype(np.float32).reshape(-1, c["Cout"])
            np.add.at(rows[:, 0], mt.reshape(-1), v32f)                 # a sequential fp32 walk: more adds per term than any kernel's tree
            np.add.at(rows[:, 1], mt.reshape(-1), v32f * v32f)
            assert (np.abs(rows - f.rows_ref) <= 0.5 * f.rows_bound).all(), c["id"]
        if c["nonneg"]:
            assert np.abs(f.A - np.abs(f.y)).max() <= 1e-12 * f.A.max()      # no cancellation: the bound has no slack to hide a defect in
    assert worst > 0.05    # (and the bounds are not vacuous: the store rounding alone reaches a fair share of them)


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_fp32_torch_inside_the_other_bounds(half):
    """data gradients, the fused BatchNorm-backward epilogue, the transforms (unfused fp32: one rounding more than the fma counted in K_XF, so
    held to the whole bound) and block64"""
    for cs in CH.DGRAD_CASES:
        if half == "fp16" and cs[0] == "f32":
            continue
        d = CH.dgrad_case(*cs, half=half)
        wt = OIHW(d["wf"], torch.float32)
        got = NHWC(F.conv_transpose2d(NCHW(d["dy"], torch.float32), wt, None, 1, 1))
        assert (np.abs(got - d["dx"]) <= 0.5 * d["bound"]).all() and (np.abs(CH.store(got, d["kind"]) - d["dx"]) <= d["bound"]).all(), cs
    for cs in CH.BNB_CASES:
        d = CH.bnb_case(*cs, half=half)
        ref, Cout = d["ref"], cs[6]
        assert not ref["marginal"].any()
        g = _conv32(d["x"][..., :cs[5]], d["w"], Cout).astype(np.float32)
        if d["addend"] is not None:
            g = g + d["addend"][..., :Cout].astype(np.float32)
        g = np.where(ref["keep"], g, np.float32(0))
        assert (np.abs(g - ref["g"]) <= 0.5 * ref["gbound"]).all() and (np.abs(CH.store(g, half) - ref["g"]) <= ref["gbound"]).all(), cs
        bx = d["bx"][..., :Cout].astype(np.float32)
        t2 = (g * (bx - d["mean"]) * d["invstd"]).astype(np.float32)
        mt = CH.tile_of(cs[2], cs[3], cs[4], d["th"], d["tw"]).reshape(-1)
        rows = np.zeros(ref["rows"].shape, dtype=np.float32)
        np.add.at(rows[:, 0], mt, g.reshape(-1, Cout))
        np.add.at(rows[:, 1], mt, t2.reshape(-1, Cout))
        assert (np.abs(rows - ref["rows"]) <= 0.5 * ref["rbound"]).all(), cs
    for cs in CH.XF_CASES:
        d = CH.xf_case(*cs, half=half)
        Cin, mode, relu = cs[5], cs[7], cs[8]
        f = lambda a, dflt: np.full(Cin, dflt, dtype=np.float32) if a is None else a
        x = d["x"][..., :Cin].astype(np.float32)
        a, c = f(d["a"], 1.0), d["c"]
        if mode == 1:
            v = x * a + c
        else:
            x2, b = d["x2"][..., :Cin].astype(np.float32), f(d["b"], 1.0)
            if mode == 2:
                v = (x * a + c) + CH.store(x2 * b + f(d["c2"], 0.0), half).astype(np.float32)
            else:
                if mode == 4:
                    x = np.where(x2 * d["msc"] + d["msh"] > 0, x, np.float32(0))
                v = a * x + (b * x2 + c)
        v = np.maximum(v, 0) if relu else v
        assert v.dtype == np.float32
        # (mode 2: the unfused second branch may round to the other 16-bit neighbour: one spacing of q, the only place a double rounding enters)
        slack = 2 * CH.U_STORE[half] * np.abs(d["Av"]) if mode == 2 else 0.0
        assert (np.abs(CH.store(v, half) - d["v"]) <= d["vbound"] + slack).all(), cs
    for cs in CH.BLOCK_CASES:
        d = CH.block_case(*cs, half=half)
        a1 = CH.store(np.maximum(_conv32(d["x"], d["w1"], 64) + d["b1"], 0), half)
        y = np.maximum(_conv32(a1, d["w2"], 64) + d["b2"] + d["x"].astype(np.float32), 0)
        assert (np.abs(y - d["y"]) <= 0.5 * d["bound"]).all() and (np.abs(CH.store(y, half) - d["y"]) <= d["bound"]).all(), cs


# ---------------------------------------------------------------------------------------------- the mutations
# name: (case, output format of the comparison, smallest share of its region a defect must move out of the bound,
#        does the old test -- one Frobenius ratio under conv_host.OLD_TOL -- pass it)
_GEN = CH._case("halo", 8, 3, 16, 24, 192, 128, "all_relu", pads=(0, 8, 16))          # non-square, three chunks, the 128-channel tile, B = 3
_NN = CH._case("halo", 8, 3, 16, 24, 192, 128, "f32probe", nonneg=True)
_ST = CH._case("halo", 0, 3, 16, 24, 64, 64, "stats", nonneg=True)
_STG = CH._case("halo", 0, 3, 16, 24, 64, 64, "stats")
MUT = {
    "corner_tap": (_GEN, 0.3, True),
    "edge_tap": (_GEN, 0.3, False),
    "left_halo_wraps": (_GEN, 0.3, False),
    "bottom_halo_next_image": (_GEN, 0.3, False),
    "hw_swapped": (_GEN, 0.3, False),
    "taps_not_flipped": (_GEN, 0.3, False),
    "last_kstep_dropped": (_GEN, 0.3, False),
    "chunk_read_twice": (_GEN, 0.3, False),
    "interleave_undone": (_GEN, 0.3, False),
    "dead_element": (_GEN, 1.0, True),
    "partials_16bit": (_NN, 0.9, True),
    "stats_from_rounded": (_ST, 0.3, True),
    "stats_row_neighbour": (_STG, 0.9, True),
    "addend_stride": (_GEN, 0.3, False),
}


def test_every_mutation_is_listed():
    assert set(MUT) == set(CH.MUTATIONS)


@pytest.mark.parametrize("name", CH.MUTATIONS)
def test_mutation_leaves_its_bound_at_its_indices(name):
    c, share, old_passes = MUT[name]
    f = CH.fwd(c)
    m = f.mutation_input()
    if name == "taps_not_flipped":      # the case's weights are the data gradient's operand of these forward weights
        m["wf"] = np.ascontiguousarray(f.w[:c["Cout"], ::-1].transpose(2, 1, 0))
        assert np.array_equal(CH.dgrad_operand(m["wf"]), f.w[:c["Cout"]])
    what, arr, region = CH.mutate(name, m)
    if what == "y":
        ref, bnd, got = f.y, f.bound, CH.store(arr, f.out_kind)
        honest = CH.store(f.y, f.out_kind)
    else:
        ref, bnd, got, honest = f.rows_ref, f.rows_bound, CH.store(arr, "fp32"), CH.store(f.rows_ref, "fp32")
    assert (np.abs(honest - ref) <= bnd).all()
    bad = ~(np.abs(got - ref) <= bnd)
    assert region.any() and not (bad & ~region).any(), "moved an element outside its region"
    assert bad[region].mean() >= share, (name, bad[region].mean())
    assert np.array_equal(got[~region], honest[~region])
    # what the old assertion made of it: one ratio over the whole tensor (for the rows: over their sum over the tiles, at 1e-3)
    if what == "y":
        passed = CH.frobenius(got, ref) < CH.OLD_TOL[f.kind]
    else:
        passed = all(CH.frobenius(got.sum(0)[i], ref.sum(0)[i]) < 1e-3 for i in (0, 1))
    assert passed == old_passes, (name, passed)


# ---------------------------------------------------------------------------------------------- the cases' properties
@pytest.mark.parametrize("prop", sorted(CH.CLAIMS))
def test_cases_have_the_properties_they_are_listed_for(prop):
    ids = CH.CLAIMS[prop]
    assert len(ids) >= 3
    for i in ids:
        assert prop in CH.case_props(CH.BY_ID[i]), (prop, i)


def test_every_tile_meets_every_edge():
    """each tile of the first kernel has a case with an XCD-remap remainder, a grid below 8, an odd chunk count, a partial channel tile, a
    non-square map and an interior tile; every input channel count and both B of the issue occur"""
    for tw in (8, 16):
        for bn in (64, 128):
            fam = [c for c in CH.FWD_CASES if c["kern"] == "halo" and (c["tw"], c["bn"]) == (tw, bn)]
            props = set().union(*(CH.case_props(c) for c in fam))
            assert props >= {"xcd_remainder", "grid_below_8", "odd_chunks", "partial_tile", "non_square", "interior_tile"}, (tw, bn, props)
            assert {c["Cin"] for c in fam} == {64, 128, 192, 512} and {c["B"] for c in fam} == {1, 3}
            assert {c["epi"] for c in fam} >= set(CH.LONG_EPI)
            if bn == 128:
                assert {c["waves"] for c in fam} >= {4, 8}
    assert len({c["id"] for c in CH.ALL_CASES}) == len(CH.ALL_CASES)
