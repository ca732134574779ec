"""The stride-1 3x3 halo conv kernels per element at their tile and image edges (-m gpu): conv3x3_halo.hip (tiles 8x8 / 8x16 x 64 / 128
channels, four- and eight-wave form, operand transforms, the fused BatchNorm-backward epilogue, the fp32 instantiation), conv3x3_v3.hip
(16x16x256, 8x16x128) and block64.hip against the fp64 yardstick tests/conv_host.py: EVERY assertion on a value is per element against a bound
derived there (tests/test_conv_host_cpu.py shows what those bounds reject).  Outputs, statistics rows and xf_out live in fenced buffers
(hiputil.Fenced): guard rows in front and behind and the pad columns (y_cs > Cout) must come back bit for bit; operand pad channels
(x_cs > Cin, add_cs > Cout, bnb_cs > Cout) hold 1e30.  The library's own answers (gdrn_conv3x3_tile, gdrn_conv3x3_halo_waves,
gdrn_conv3x3_stats_rows) must name the instantiation a case is listed for.

This module tests libgdrn_hip.so (bf16 and the fp32 instantiation); tests/test_conv3x3_edges_fp16_gpu.py executes the same source with `BF16`
bound to the fp16 code and libgdrn_hip_f16.so.  Every case prints `RATIO <family> <worst error / bound>` before it asserts."""
import numpy as np
import pytest
import torch

import conv_host as CH
from gdrnet_amd import cabi
from gdrnet_amd.cabi import F32, check, ptr

pytestmark = pytest.mark.gpu

BF16 = globals().get("__HALF__", cabi.BF16)       # the 16-bit dtype code under test
IS_F16 = BF16 == cabi.F16
HALF = "fp16" if IS_F16 else "bf16"
HT = torch.float16 if IS_F16 else torch.bfloat16
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hiputil

    cabi.load(BF16)
    return hiputil


def _ids(cases):
    return [c["id"] for c in cases if not (IS_F16 and c["kern"] == "f32")]     # (the fp32 instantiation: in the bf16 module only)


def _dt(kern):
    return F32 if kern == "f32" else BF16


def _v3(kern, waves):
    return True if kern.startswith("v3") else (waves or False)


def _waves_expected(kern, waves, bn, grid):
    if kern.startswith("v3"):
        return 0
    return 8 if (kern == "halo" and bn == 128 and (waves == 8 or (waves == 0 and grid <= 256))) else 4


def within(H, got, ref, bnd, what, family):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / bnd
    print(f"RATIO {HALF} {family} {np.nanmax(np.where(bnd > 0, r, 0.0)):.4f}  ({what})")
    H.assert_within(got, ref, bnd, what)


def _confirm(info, kern, waves, B, Hh, Ww, Cout, th, tw, bn):
    assert info["tile"] == (th, tw, bn), (info, (th, tw, bn))
    assert info["halo_waves"] == _waves_expected(kern, waves, bn, CH.grid_size(B, Hh, Ww, Cout, th, tw, bn)), info
    assert info["stats_rows"] == CH.n_tiles(B, Hh, Ww, th, tw), info


def _family(c_kern, waves, th, tw, bn, out_kind):
    form = {"halo": "halo", "f32": "fp32", "v3_256": "v3", "v3_128": "v3"}[c_kern]
    return f"{form}-{th}x{tw}x{bn}" + ("-8w" if waves == 8 else "") + f"-out-{out_kind}"


# ---------------------------------------------------------------------------------------------- forward: every tile, every epilogue
@pytest.mark.parametrize("cid", _ids(CH.ALL_CASES))
def test_forward_per_element_with_fences(H, cid):
    c = CH.BY_ID[cid]
    f = CH.fwd(c, HALF)
    dt, B, Hh, Ww, Cin, Cout = _dt(c["kern"]), c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    M, th, tw, bn = B * Hh * Ww, c["th"], c["tw"], c["bn"]
    y = H.Fenced(M, f.y_cs, Cout, TD[f.out_kind])
    st = H.Fenced(2 * CH.n_tiles(B, Hh, Ww, th, tw), Cout, Cout, torch.float32) if f.want_stats else None
    info = {}
    H.conv_gemm(H.to_dev(f.x, dt), H.to_dev(f.w, dt), B, Hh, Ww, Cin, f.x_cs, Hh, Ww, Cout, 3, 3, 1, 1, dt,
                bias=None if f.bias is None else H.f32_dev(f.bias), addend=None if f.addend is None else H.to_dev(f.addend, dt),
                act=f.act, out_f32=f.out_f32, y_cs=f.y_cs, want_stats=bool(f.want_stats), halo=True, v3=_v3(c["kern"], c["waves"]),
                y_buf=y.t, stats_buf=None if st is None else st.t, info=info)
    _confirm(info, c["kern"], c["waves"], B, Hh, Ww, Cout, th, tw, bn)
    fam = _family(c["kern"], info["halo_waves"], th, tw, bn, f.out_kind) + ("-nonneg" if c["nonneg"] else "")
    within(H, y.host(cid).reshape(B, Hh, Ww, Cout), f.y, f.bound, cid, fam)
    if st is not None:
        within(H, st.host(cid + " statistics").reshape(-1, 2, Cout), f.rows_ref, f.rows_bound, cid + " statistics rows",
               "statistics" + ("-nonneg" if c["nonneg"] else ""))


# ---------------------------------------------------------------------------------------------- data gradient, Cin != Cout
@pytest.mark.parametrize("case", [c for c in CH.DGRAD_CASES if not (IS_F16 and c[0] == "f32")], ids=lambda c: "-".join(map(str, c)))
def test_data_gradient_per_element(H, case):
    """the operand is the library's own (gdrn_pack4 with flipped taps, transposed) of the forward weights: unflipped taps or a swapped
    transpose leave the bound everywhere (mutation taps_not_flipped)"""
    kern, waves, B, Hh, Ww, Cf_in, Cf_out = case
    dt = _dt(kern)
    d = CH.dgrad_case(*case, half=HALF)
    th, tw, bn = CH.expected_tile(kern, Ww, Cf_in)
    w_oihw = torch.from_numpy(d["wf"].reshape(Cf_out, 3, 3, Cf_in).transpose(0, 3, 1, 2).copy()).float()
    wd = H.pack_dgrad(w_oihw, dt, flip=1)
    assert tuple(wd.shape) == (CH.rows_of(Cf_in, bn), 9, Cf_out)
    y = H.Fenced(B * Hh * Ww, Cf_in + 8, Cf_in, TD[d["kind"]])
    info = {}
    H.conv_gemm(H.to_dev(d["dy"], dt), wd, B, Hh, Ww, Cf_out, Cf_out, Hh, Ww, Cf_in, 3, 3, 1, 1, dt, y_cs=Cf_in + 8, halo=True,
                v3=_v3(kern, waves), y_buf=y.t, info=info)
    _confirm(info, kern, waves, B, Hh, Ww, Cf_in, th, tw, bn)
    within(H, y.host().reshape(B, Hh, Ww, Cf_in), d["dx"], d["bound"], str(case), "dgrad-" + _family(kern, info["halo_waves"], th, tw, bn, d["kind"]))


# ---------------------------------------------------------------------------------------------- fused BatchNorm-backward epilogue
@pytest.mark.parametrize("case", CH.BNB_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fused_bn_backward_epilogue_per_element_and_row_by_row(H, case):
    kern, waves, B, Hh, Ww, Cin, Cout, mask_kind, with_add = case
    dt = BF16
    d = CH.bnb_case(*case, half=HALF)
    ref, th, tw, bn, cs = d["ref"], d["th"], d["tw"], d["bn"], d["cs"]
    assert not ref["marginal"].any()
    bnb = dict(x=H.to_dev(d["bx"], dt), mean=H.f32_dev(d["mean"]), invstd=H.f32_dev(d["invstd"]))
    if mask_kind == "stored":
        bnb["mask"] = H.to_dev(d["mask"], dt)
    elif mask_kind == "affine":
        bnb["scale"], bnb["shift"] = H.f32_dev(d["scale"]), H.f32_dev(d["shift"])
    y = H.Fenced(B * Hh * Ww, cs, Cout, HT)
    rows = H.Fenced(2 * CH.n_tiles(B, Hh, Ww, th, tw), Cout, Cout, torch.float32)
    info = {}
    H.conv_gemm(H.to_dev(d["x"], dt), H.to_dev(d["w"], dt), B, Hh, Ww, Cin, Cin, Hh, Ww, Cout, 3, 3, 1, 1, dt,
                addend=None if d["addend"] is None else H.to_dev(d["addend"], dt), y_cs=cs, halo=True, bnb=bnb, v3=_v3(kern, waves),
                y_buf=y.t, rows_buf=rows.t, info=info)
    _confirm(info, kern, waves, B, Hh, Ww, Cout, th, tw, bn)
    fam = _family(kern, info["halo_waves"], th, tw, bn, HALF)
    within(H, y.host().reshape(B, Hh, Ww, Cout), ref["g"], ref["gbound"], f"{case} masked gradient", "bnb-output-" + fam)
    got = y.host().reshape(B, Hh, Ww, Cout)
    assert (got[~ref["keep"]] == 0.0).all(), "a masked element is not exactly 0"
    within(H, rows.host("rows").reshape(-1, 2, Cout), ref["rows"], ref["rbound"], f"{case} sums, row by row", "bnb-sums")


# ---------------------------------------------------------------------------------------------- operand transforms
@pytest.mark.parametrize("case", CH.XF_CASES, ids=lambda c: "-".join(map(str, c)))
def test_operand_transform_and_the_conv_of_its_own_output(H, case):
    """xf_out against the transform's bound; the conv's output against the conv of the DEVICE's xf_out, zero-padded: a halo whose out-of-image
    pixels were transformed (v(0) = c != 0) instead of zeroed leaves the bound along every image edge"""
    kern, waves, B, Hh, Ww, Cin, Cout, mode, relu, given, xpad = case
    dt = BF16
    d = CH.xf_case(*case, half=HALF)
    th, tw, bn, x_cs, M = d["th"], d["tw"], d["bn"], Cin + xpad, B * Hh * Ww
    out = H.Fenced(M, x_cs, Cin, HT)
    y = H.Fenced(M, Cout + 8, Cout, HT)
    dev = lambda a: None if a is None else H.f32_dev(a)
    xf = dict(mode=mode, relu=relu, x2=None if d["x2"] is None else H.to_dev(d["x2"], dt), a=dev(d["a"]), b=dev(d["b"]), c=dev(d["c"]),
              c2=dev(d["c2"]), msc=dev(d["msc"]), msh=dev(d["msh"]), out=out.t)
    info = {}
    H.conv_gemm(H.to_dev(d["x"], dt), H.to_dev(d["w"], dt), B, Hh, Ww, Cin, x_cs, Hh, Ww, Cout, 3, 3, 1, 1, dt, y_cs=Cout + 8, halo=True, xf=xf,
                v3=_v3(kern, waves), y_buf=y.t, info=info)
    _confirm(info, kern, waves, B, Hh, Ww, Cout, th, tw, bn)
    v_dev = out.host("xf_out").reshape(B, Hh, Ww, Cin)
    within(H, v_dev, d["v"], d["vbound"], f"{case} xf_out", f"xf_out-mode{mode}")
    yr, A, bnd = CH.conv(v_dev, d["w"], Cout, kind=HALF)
    within(H, y.host().reshape(B, Hh, Ww, Cout), yr, bnd, f"{case} conv of xf_out", "xf-conv-" + _family(kern, info["halo_waves"], th, tw, bn, HALF))


# ---------------------------------------------------------------------------------------------- block64
@pytest.mark.parametrize("case", CH.BLOCK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_block64_per_element(H, case):
    """against the two-conv fp64 reference with the intermediate rounded to the storage format (conv_host.block64: an intermediate within
    its accumulation bound of a rounding tie may sit on either neighbour -- that, and nothing else, widens conv2's bound)"""
    B, Hh, Ww = case
    lib, dt = cabi.load(BF16), BF16
    d = CH.block_case(*case, half=HALF)
    wf = []
    for w in (d["w1"], d["w2"]):
        src = H.to_dev(w, dt)
        dst = torch.empty_like(src)
        check(lib.gdrn_pack_wfrag(ptr(src), ptr(dst), 64, 64, dt, H.stream()), "pack_wfrag")
        wf.append(dst)
    xd, b1, b2 = H.to_dev(d["x"], dt), H.f32_dev(d["b1"]), H.f32_dev(d["b2"])
    y = H.Fenced(B * Hh * Ww, 64, 64, HT)
    assert lib.gdrn_block64_eval_ok(B, Hh, Ww, dt) == 1
    check(lib.gdrn_block64_eval(ptr(xd), ptr(wf[0]), ptr(b1), ptr(wf[1]), ptr(b2), ptr(y.t), B, Hh, Ww, dt, H.stream()), "block64_eval")
    within(H, y.host().reshape(B, Hh, Ww, 64), d["y"], d["bound"], str(case), "block64")


# ---------------------------------------------------------------------------------------------- refusals: return code only, outputs untouched
def _refuse(H, dt, B, Hh, Ww, Cin, Cout, x_cs=None, y_cs=None, v3=False, big_x=False, **kw):
    """(status, output untouched).  Every buffer has the size the shape asks for, so that a launch that should have been refused stays
    inside its buffers (big_x: uninitialised, never read)."""
    tdt = H.tdt(dt)
    x_cs, y_cs = x_cs or Cin, y_cs or Cout
    M = B * Hh * Ww
    x = torch.empty((M, x_cs), dtype=tdt, device=H.DEV) if big_x else torch.zeros((M, x_cs), dtype=tdt, device=H.DEV)
    w = torch.zeros((max(kw.get("w_rows") or 0, CH.rows_of(Cout, 128)), 9, Cin), dtype=tdt, device=H.DEV)
    y = H.Fenced(M, y_cs, min(Cout, y_cs), tdt)
    st = H.conv_gemm(x, w, B, Hh, Ww, Cin, x_cs, Hh, Ww, Cout, 3, 3, 1, 1, dt, y_cs=y_cs, halo=True, v3=v3, y_buf=y.t, prepacked=True, rc=True, **kw)
    return st, y.untouched()


def test_refusals_by_return_code_with_the_output_untouched(H):
    dt = BF16
    SHAPE, ARG = -2, -1
    assert _refuse(H, dt, 1, 12, 8, 64, 64) == (SHAPE, True)                       # H not a multiple of 8
    assert _refuse(H, dt, 1, 8, 12, 64, 64) == (SHAPE, True)                       # W not a multiple of 8
    assert _refuse(H, dt, 1, 8, 8, 96, 64) == (SHAPE, True)                        # Cin bytes not a multiple of 128
    assert _refuse(H, dt, 1, 8, 8, 64, 64, y_cs=66) == (SHAPE, True)               # y_cs & 3
    assert _refuse(H, dt, 1, 8, 8, 64, 128, y_cs=132) == (SHAPE, True)             # the 128 tile: y_cs & 7
    assert _refuse(H, dt, 1, 8, 8, 64, 128, w_rows=64) == (SHAPE, True)            # w_rows short of the channel tiles
    assert _refuse(H, dt, 1, 8, 8, 64, 72, w_rows=72) == (SHAPE, True)             # ... of a partial last tile
    assert _refuse(H, dt, 1, 8, 8, 64, 128, halo_waves=3) == (ARG, True)
    assert _refuse(H, dt, 1, 8, 16, 64, 72, y_cs=72, v3=True) == (SHAPE, True)     # the second-generation kernel takes no partial channel tile
    assert _refuse(H, dt, 1, 8, 16, 64, 192, v3=True) == (SHAPE, True)
    if not IS_F16:
        c = H.f32_dev(np.ones(64))
        assert _refuse(H, F32, 1, 8, 8, 64, 64, xf=dict(mode=1, c=c)) == (ARG, True)   # fp32 with a transform
        assert _refuse(H, F32, 1, 8, 16, 64, 128, v3=True) == (SHAPE, True)            # fp32 on a second-generation operand


@pytest.mark.parametrize("dt_name", ["half"] + ([] if IS_F16 else ["fp32"]))
def test_patch_offsets_past_32_bits_are_refused(H, dt_name):
    """M * x_cs * sizeof(T) = 2^32 with M * max(y_cs, add_cs) * 4 = 2^28: the kernel's 32-bit patch offsets would wrap.  Refused by return
    code, output untouched (both buffers are allocated in full: nothing here could run out of bounds)."""
    dt = F32 if dt_name == "fp32" else BF16
    x_cs = 1024 if dt == F32 else 2048
    assert _refuse(H, dt, 16, 256, 256, 64, 64, x_cs=x_cs, big_x=True) == (-2, True)
    assert _refuse(H, dt, 1, 8, 8, 64, 64, x_cs=x_cs) == (0, False)                # the same strides on a small map run
