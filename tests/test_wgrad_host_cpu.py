"""Pins tests/wgrad_host.py -- the yardstick of tests/test_wgrad_edges_gpu.py -- without a GPU: its gradient equals fp64 autograd of F.conv2d /
F.conv_transpose2d on every geometry the GPU module uses; the slab order equals the index expressions of the kernel's store and of the
reduction's reader; torch's own fp32 autograd sits inside HALF of every bound on every GPU case; every random case keeps the detectability
condition (max bound <= half a median term); every mutated reference leaves its bound inside the region it touches and nowhere else; the
case tables have the properties they are listed for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_host as WH

ALL_HALO = list(WH.HALO_BY_ID.values())


def _nchw(a, C_):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a[..., :C_], (0, 3, 1, 2))))


def _autograd(x, dy, c, KH, KW, dtype=torch.float64):
    """dw[co][tap][ci] by autograd of F.conv2d on the operands' first Cin / Cout channels"""
    xt, dyt = _nchw(x, c["Cin"]).to(dtype), _nchw(dy, c["Cout"]).to(dtype)
    w = torch.zeros(c["Cout"], c["Cin"], KH, KW, dtype=dtype, requires_grad=True)
    y = F.conv2d(xt, w, None, c["stride"], c["pad"] if "pad" in c else 1)
    assert y.shape[2] >= dyt.shape[2] and y.shape[3] >= dyt.shape[3]
    g = torch.zeros_like(y)
    g[:, :, :dyt.shape[2], :dyt.shape[3]] = dyt          # (the window cases use the first Wo columns of the map only)
    y.backward(g)
    return w.grad.permute(0, 2, 3, 1).reshape(c["Cout"], KH * KW, c["Cin"]).double().numpy()


def _expanded(x, Cin):
    """window form -> the explicit [B][Hi][Wi][Cin] operand (windows that leave the buffer are cut: no case reads them)"""
    flat = np.concatenate([x.reshape(-1), np.zeros(Cin)])
    idx = np.arange(x.size // x.shape[-1])[:, None] * x.shape[-1] + np.arange(Cin)[None]
    return flat[idx].reshape(x.shape[:3] + (Cin,))


# ---------------------------------------------------------------------------------------------- the gradient itself
@pytest.mark.parametrize("cid", [c["id"] for c in ALL_HALO])
def test_halo_geometries_match_fp64_autograd(cid):
    c = WH.HALO_BY_ID[cid]
    h = WH.halo(c)
    ref = _autograd(h.x, h.dy, c, 3, 3)
    assert np.abs(h.dw - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(WH.wgrad(h.x, h.dy, c["Cin"], c["Cout"], 3, 3, c["stride"], 1)[0] - h.dw).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert (h.A >= np.abs(h.dw) - 1e-9).all()
    if c["exact"]:
        assert np.array_equal(h.dw, np.round(h.dw)) and np.abs(h.dw0 + h.dw).max() < 2 ** 24 and h.PA.sum(0).max() < 2 ** 24


@pytest.mark.parametrize("cid", [c["id"] for c in WH.GEN_CASES + WH.GEN_EXACT])
def test_generic_geometries_match_fp64_autograd(cid):
    c = WH.GEN_BY_ID[cid]
    g = WH.gen(c)
    x = _expanded(g.x, c["Cin"]) if c["x_cs"] < c["Cin"] else g.x
    ref = _autograd(x, g.dy, c, c["KH"], c["KW"])
    assert np.abs(g.dw - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    if c["exact"]:
        assert np.array_equal(g.dw, np.round(g.dw)) and (g.A + np.abs(g.dw0)).max() < 2 ** 24
        assert WH.gen_splits(c)[0] > 8


def test_conv_transpose_with_the_roles_swapped():
    """ConvTranspose2d(3, 2, 1, 1): its weight gradient [in][out][3][3] is the stride-2 gradient with x = the gradient of its OUTPUT and
    dy = its INPUT (plan.py), tap for tap"""
    r = np.random.default_rng(5)
    B, Hh, Ww, Ci, Co = 2, 4, 8, 64, 128
    inp = torch.from_numpy(r.standard_normal((B, Ci, Hh, Ww)))
    w = torch.from_numpy(r.standard_normal((Ci, Co, 3, 3))).requires_grad_(True)
    out = F.conv_transpose2d(inp, w, None, 2, 1, 1)
    dout = torch.from_numpy(r.standard_normal(tuple(out.shape)))
    out.backward(dout)
    dw, _ = WH.wgrad(dout.permute(0, 2, 3, 1).numpy(), inp.permute(0, 2, 3, 1).numpy(), Co, Ci, 3, 3, 2, 1)
    ref = w.grad.permute(0, 2, 3, 1).reshape(Ci, 9, Co).numpy()
    assert np.abs(dw - ref).max() <= 1e-12 * np.abs(ref).max()
    # ... and the reduction's scatter with the parameter's strides puts it where .grad has it
    dst, written = WH.reduce_ref(dw[None], 0, Co * 9, 9, 1, Ci * Co * 9)
    assert written.all() and np.abs(dst - w.grad.numpy().reshape(-1)).max() <= 1e-12 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("Cout,Cin", [(64, 64), (192, 128)])
def test_slab_order_is_the_kernels_store_and_the_reductions_read(Cout, Cin):
    ncot = Cout // 64
    dw = np.arange(Cout * 9 * Cin, dtype=np.float64).reshape(Cout, 9, Cin)
    slab = WH.to_slab(dw)
    assert np.array_equal(WH.from_slab(slab, Cout, Cin), dw)
    # the store of wgrad_tile: wave, a (fragment), lane = g 16 + q, j; tile = cit ncot + cot
    cit, cot, t, a, wave, lane, j = np.meshgrid(np.arange(Cin // 64), np.arange(ncot), np.arange(9), np.arange(4), np.arange(4), np.arange(64),
                                                np.arange(4), indexing="ij")
    g, q = lane >> 4, lane & 15
    off = (cit * ncot + cot) * 36864 + ((t * 2 + (a & 1)) * 2 + (wave & 1)) * 1024 + (((a & 3) >> 1) * 2 + (wave >> 1)) * 256 + lane * 4 + j
    assert np.array_equal(slab[off], dw[cot * 64 + a * 16 + g * 4 + j, t, cit * 64 + wave * 16 + q])
    assert len(np.unique(off)) == slab.size
    # the read of wgrad_reduce_multi_kernel: unit = (tile, wv, a, b), column (t, ln), element j
    tile, wv, a, b, t, ln, j = np.meshgrid(np.arange(ncot * (Cin // 64)), np.arange(4), np.arange(2), np.arange(2), np.arange(9), np.arange(64),
                                           np.arange(4), indexing="ij")
    g, q = ln >> 4, ln & 15
    off = tile * 36864 + ((a * 2 + b) * 4 + wv) * 256 + t * 4096 + ln * 4 + j
    co = (tile % ncot) * 64 + (wv >> 1) * 32 + a * 16 + g * 4 + j
    ci = (tile // ncot) * 64 + (wv & 1) * 32 + b * 16 + q
    assert np.array_equal(slab[off], dw[co, t, ci])


def test_reduce_scatter_and_cin_valid():
    dw = np.arange(2 * 64 * 9 * 128, dtype=np.float64).reshape(2, 64, 9, 128)
    dst, written = WH.reduce_ref(dw, 69, 69 * 9, 9, 1, 64 * 69 * 9)
    assert written.all() and np.array_equal(dst.reshape(64, 69, 9), dw.sum(0)[:, :, :69].transpose(0, 2, 1))
    dst, written = WH.reduce_ref(dw, 69, 128 * 9, 9, 1, 64 * 128 * 9)
    assert np.array_equal(written.reshape(64, 128, 9), np.broadcast_to((np.arange(128) < 69)[None, :, None], (64, 128, 9)))


def test_split_ranges_and_patches():
    for c in ALL_HALO:
        pid = WH.patch_of(c["B"], c["Ho"], c["Wo"], c["stride"])
        assert pid.max() + 1 == c["npatch"] and (np.bincount(pid.reshape(-1)) == 8 * WH.patch_rows(c["stride"])).all()
        assert (np.diff(pid[:, 0, 0]) > 0).all()                      # image first
        for req in WH.split_requests(c["npatch"]):
            for ws in (True, False):
                ns = WH.n_splits(c["npatch"], c["tiles"], req, ws)
                rng = WH.split_ranges(c["npatch"], ns)
                assert rng[0][0] == 0 and rng[-1][1] == c["npatch"] and all(a < b for a, b in rng)
                assert all(rng[i][1] == rng[i + 1][0] for i in range(ns - 1))
    # the grid: 1, 2, 3 and many patches per split, a short last split, a boundary inside a tile row and one across an image boundary
    per = set()
    short = inside_row = across_image = False
    for c in WH.HALO_CASES:
        tx, ty = c["Wo"] // 8, c["Ho"] // WH.patch_rows(c["stride"])
        for req in WH.split_requests(c["npatch"]):
            rng = WH.split_ranges(c["npatch"], WH.n_splits(c["npatch"], c["tiles"], req, True))
            per.add(rng[0][1] - rng[0][0])
            short |= (rng[-1][1] - rng[-1][0]) < (rng[0][1] - rng[0][0])
            inside_row |= any(a % tx for a, _ in rng)
            across_image |= any(a // (tx * ty) != (b - 1) // (tx * ty) and a % (tx * ty) for a, b in rng)
    assert {1, 2, 3} <= per and max(per) >= 9 and short and inside_row and across_image


def test_case_tables_have_the_properties_they_are_listed_for():
    assert {c["Ho"] != c["Wo"] for c in WH.HALO_CASES} == {True, False}
    assert {(c["Cin"], c["Cout"]) for c in WH.HALO_CASES} == set(WH.HALO_CH)
    assert {(c["stride"], c["B"], c["Ho"], c["Wo"]) for c in WH.HALO_CASES} == (
        {(1, b, h, w) for b in (1, 3) for h, w in WH.S1_MAPS} | {(2, b, h, w) for b in (1, 3) for h, w in WH.S2_MAPS})
    assert max(c["M"] for c in WH.HALO_CASES + WH.GEN_CASES) <= 1152
    rem = set()
    for name, table in WH.GROUPED.items():
        ns, starts = WH.grouped_blocks(table)
        rem.add(starts[-1] % 8)
        assert len(table) == {"one": 1, "two": 2, "five": 5}[name]
    assert rem == {0, 1, 7}
    assert any(WH.n_splits(c["npatch"], c["tiles"], r, True) != r for t in WH.GROUPED.values() for c, r in t)       # a normalised request
    assert {c["stride"] for c, _ in WH.GROUPED["five"]} == {1, 2}
    for c in WH.HALO_EXACT:
        assert WH.n_splits(c["npatch"], c["tiles"], 0, True) > 8 and (c["tiles"] * WH.n_splits(c["npatch"], c["tiles"], 0, True)) % 8
    assert {WH.gen_tile(c) for c in WH.GEN_CASES if not c["fp32"]} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {WH.gen_tile(c) for c in WH.GEN_CASES if c["fp32"]} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {4, 37, 64, 65, 81, 256} <= {c["M"] for c in WH.GEN_CASES}
    assert {(c["Cout"], c["dy_cs"]) for c in WH.GEN_CASES} >= {(9, 64), (69, 128), (130, 256)}
    assert any(WH.gen_splits(c)[0] > WH.gen_splits(c)[1] for c in WH.GEN_CASES)                                       # more splits than stages
    pow2 = {(c["Wo"] & (c["Wo"] - 1)) == 0 and ((c["Ho"] * c["Wo"]) & (c["Ho"] * c["Wo"] - 1)) == 0 for c in WH.GEN_CASES}
    assert pow2 == {True, False}


# ---------------------------------------------------------------------------------------------- an independent fp32 evaluation; detectability
@pytest.mark.parametrize("cid", [c["id"] for c in ALL_HALO])
def test_halo_torch_fp32_inside_half_the_bound_and_a_term_outside_it(cid):
    c = WH.HALO_BY_ID[cid]
    for kind in ("bf16", "fp16"):
        h = WH.halo(c, kind)
        got = _autograd(h.x, h.dy, c, 3, 3, torch.float32)
        assert (np.abs(got - h.dw) <= 0.5 * h.bound(1)).all(), kind                    # (the smallest k any test uses for the whole gradient)
        if not c["exact"]:
            worst, half_term = WH.detectable(h.bound(c["npatch"] + 5, True), h.x[..., :c["Cin"]], h.dy[..., :c["Cout"]])
            assert worst <= half_term, (kind, worst, half_term)


@pytest.mark.parametrize("cid", [c["id"] for c in WH.GEN_CASES])
def test_generic_torch_fp32_inside_half_the_bound_and_a_term_outside_it(cid):
    c = WH.GEN_BY_ID[cid]
    for kind in ("bf16", "fp16"):
        g = WH.gen(c, kind)
        x = _expanded(g.x, c["Cin"]) if c["x_cs"] < c["Cin"] else g.x
        got = _autograd(x, g.dy, c, c["KH"], c["KW"], torch.float32)
        assert (np.abs(got - g.dw) <= 0.5 * WH.bound(g.A, WH.k_wgrad(c["M"], 1, c["fp32"]))).all(), kind
        worst, half_term = WH.detectable(g.bound, g.x[..., :min(c["Cin"], c["x_cs"])], g.dy[..., :c["Cout"]])
        assert worst <= half_term, (kind, worst, half_term)


# ---------------------------------------------------------------------------------------------- the mutations
_S1 = WH._halo(1, 3, 8, 24, 64, 64)          # M = 576, nine patches, non-square, B = 3
_S1L = WH._halo(1, 3, 16, 24, 64, 64)        # M = 1152: the largest random case
_S1C = WH._halo(1, 3, 8, 24, 128, 128)       # ... with a 2 x 2 grid of 64 x 64 tiles and 128 operand channels (69 of them valid)
_S2 = WH._halo(2, 3, 4, 24, 64, 64)
_P3 = WH._halo(1, 1, 8, 24, 64, 64)          # three patches
# name: (case, splits, smallest share of its region the defect must move out of the bound, does `rel < 1e-2` on the same operands pass it)
MUT = {
    "corner_term": (_S1L, 1, 0.60, False),     # (rel 1.4e-2 at M = 1152; it falls like 1 / sqrt(M): under 1e-2 from M ~ 2200 on)
    "top_halo_previous_image": (_S1, 1, 0.95, False),
    "right_halo_wraps": (_S1, 1, 0.95, False),
    "hw_swapped": (_S1, 1, 0.60, False),
    "taps_transposed": (_S1, 1, 0.95, False),
    "taps_flipped": (_S1, 1, 0.95, False),
    "stride2_unshifted": (_S2, 1, 0.95, False),
    "last_patch_dropped": (_S1, 3, 0.95, False),
    "first_patch_twice": (_S1, 3, 0.95, False),
    "fifth_slab_dropped": (_S1, 5, 0.95, False),
    "partials_16bit": (_P3, 3, 0.50, True),
    "blocks_exchanged": (_S1C, 1, 0.95, False),
    "cin_valid_ignored": (_S1C, 2, 1.00, None),
    "strides_exchanged": (_S1C, 2, 0.95, None),
    "atomics_overwrite": (_S1, 2, 0.95, False),
}


def test_every_mutation_is_listed():
    assert set(MUT) == set(WH.MUTATIONS)


@pytest.mark.parametrize("name", WH.MUTATIONS)
def test_mutation_leaves_its_bound_inside_its_region_and_nowhere_else(name):
    c, nsplit, share, old_passes = MUT[name]
    h = WH.halo(c)
    got, ref, bnd, region = WH.mutate(name, h, nsplit)
    assert not WH.offenders(ref, ref, bnd).any()
    bad = WH.offenders(got, ref, bnd)
    assert region.any() and not (bad & ~region).any(), "moved an element outside its region"
    frac = bad[region].mean()
    print(f"{name}: {frac:.3f} of its region outside the bound", end="")
    assert frac >= share, (name, frac)
    same = ~region
    assert np.array_equal(got[same], ref[same], equal_nan=True)
    if old_passes is not None:          # what the old assertion makes of it: one ratio over the whole tensor
        rel = WH.frobenius(got, ref)
        print(f", rel {rel:.2e}")
        assert (rel < WH.OLD_TOL) == old_passes, (name, rel)
