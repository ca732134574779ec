"""The weight-gradient kernels per element at their split and image edges (-m gpu): conv3x3_wgrad.hip (the halo kernel on its own, the grouped
launch, the workspace reduction) and conv_wgrad.hip (the generic kernel, its four tile shapes, 16-bit and fp32) against the fp64 yardstick
tests/wgrad_host.py: EVERY assertion on a value is per element against a bound derived there, or bit for bit where the operands are exact
(tests/test_wgrad_host_cpu.py shows what those bounds reject).  dw, the workspace and the reduction's destination live in fenced buffers
(hiputil.Fenced): guard rows in front and behind must come back bit for bit, every slab the split query announces must be fully written;
operand pad channels hold 1e30 (6e4 in fp16).

This module tests libgdrn_hip.so (bf16 and the generic kernel's fp32 instantiation); tests/test_wgrad_edges_fp16_gpu.py executes the same
source with `BF16` bound to the fp16 code and libgdrn_hip_f16.so.  Every comparison prints `RATIO <family> <worst error / bound>` first."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_host as WH
from gdrnet_amd import cabi
from gdrnet_amd.cabi import F32, ptr, to_device_table

pytestmark = pytest.mark.gpu

BF16 = globals().get("__HALF__", cabi.BF16)       # the 16-bit dtype code under test
IS_F16 = BF16 == cabi.F16
HALF = "fp16" if IS_F16 else "bf16"
HT = torch.float16 if IS_F16 else torch.bfloat16
OK, ARG, SHAPE = 0, -1, -2


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hiputil

    cabi.load(BF16)
    return hiputil


def _lib():
    return cabi.load(BF16)


def within(H, got, ref, bnd, what, family):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / bnd
    print(f"RATIO {HALF} {family} {np.nanmax(np.where(bnd > 0, r, 0.0)):.4f}  ({what})")
    H.assert_within(got, ref, bnd, what)


def _params(H, h, x, dy, dw=None, ws=None, splits=0):
    c = h.c
    return H.wgrad_params(x, dy, dw, ws, c["Hi"], c["Wi"], c["Cin"], h.x_cs, c["Ho"], c["Wo"], c["Cout"], h.dy_cs, 3, 3, c["stride"], 1, c["M"], BF16, splits)


def _slabs(ws, ns, Cout, Cin, what):
    flat = ws.host(what).reshape(ns, -1)           # (host(): fences intact; a slot never written is NaN and fails the comparison)
    return np.stack([WH.from_slab(flat[s], Cout, Cin) for s in range(ns)])


def _halo_ws(H, h, x, dy, req):
    """the workspace path of one request: (splits, fenced workspace, fenced OIHW gradient), both launched twice and bit-identical"""
    lib, c = _lib(), h.c
    Cin, Cout = c["Cin"], c["Cout"]
    ns = lib.gdrn_conv3x3_wgrad_splits(C.byref(_params(H, h, x, dy, ws=x, splits=req)))
    assert ns == WH.n_splits(c["npatch"], c["tiles"], req, True), (req, ns)
    runs = []
    for _ in range(2):
        ws = H.fenced_flat(ns * Cout * Cin * 9)
        assert lib.gdrn_conv3x3_wgrad(C.byref(_params(H, h, x, dy, ws=ws.t, splits=req)), H.stream()) == OK
        dst = H.Fenced(Cout, Cin * 9, Cin * 9, torch.float32)
        assert H.wgrad_reduce(lib, [dict(ws=ws.t, dst=dst.t, nsplit=ns, Cout=Cout, Cin=Cin, cin_valid=0, s_co=Cin * 9, s_ci=9, s_t=1)]) == OK
        runs.append((ws, dst))
    assert H.same_bits(runs[0][0].t, runs[1][0].t), "two runs of the workspace path differ"
    assert H.same_bits(runs[0][1].t, runs[1][1].t), "two runs of the reduction differ"
    return ns, runs[0][0], runs[0][1]


# ---------------------------------------------------------------------------------------------- the halo kernel, single launch
@pytest.mark.parametrize("cid", [c["id"] for c in WH.HALO_CASES])
def test_halo_every_split_request_slab_by_slab_reduced_and_with_atomics(H, cid):
    c = WH.HALO_BY_ID[cid]
    h = WH.halo(c, HALF)
    lib, Cin, Cout, fam = _lib(), c["Cin"], c["Cout"], f"halo-s{c['stride']}"
    x, dy = H.to_dev(h.x, BF16), H.to_dev(h.dy, BF16)
    assert lib.gdrn_conv3x3_wgrad_ok(C.byref(_params(H, h, x, dy, ws=x))) == 1
    for req in WH.split_requests(c["npatch"]):
        what = f"{cid} splits={req}"
        ns, ws, dst = _halo_ws(H, h, x, dy, req)
        ref, refA, pix = h.slabs(ns)
        bnd = np.stack([WH.bound(refA[s], pix[s]) for s in range(ns)])
        within(H, _slabs(ws, ns, Cout, Cin, what), ref, bnd, what + " raw slabs", fam + "-slabs")
        within(H, dst.host(what).reshape(Cout, Cin, 9).transpose(0, 2, 1), h.dw, h.bound(ns), what + " reduced", fam + "-reduced")
        # atomics onto a dw that already holds values
        na = lib.gdrn_conv3x3_wgrad_splits(C.byref(_params(H, h, x, dy, dw=x, splits=req)))
        assert na == WH.n_splits(c["npatch"], c["tiles"], req, False), (req, na)
        dw = H.Fenced(Cout, 9 * Cin, 9 * Cin, torch.float32)
        dw.t.copy_(H.f32_dev(h.dw0.reshape(Cout, -1)))
        assert lib.gdrn_conv3x3_wgrad(C.byref(_params(H, h, x, dy, dw=dw.t, splits=req)), H.stream()) == OK
        within(H, dw.host(what).reshape(Cout, 9, Cin), h.dw0 + h.dw, h.bound(na, True), what + " atomics", fam + "-atomics")


@pytest.mark.parametrize("cid", [c["id"] for c in WH.HALO_EXACT])
def test_halo_exact_operands_bit_for_bit_past_eight_splits(H, cid):
    c = WH.HALO_BY_ID[cid]
    h = WH.halo(c, HALF)
    lib, Cin, Cout = _lib(), c["Cin"], c["Cout"]
    x, dy = H.to_dev(h.x, BF16), H.to_dev(h.dy, BF16)
    ns, ws, dst = _halo_ws(H, h, x, dy, 0)
    assert ns > 8 and (ns * c["tiles"]) % 8
    H.assert_same(_slabs(ws, ns, Cout, Cin, cid), h.slabs(ns)[0], cid + " raw slabs")
    H.assert_same(dst.host(cid).reshape(Cout, Cin, 9).transpose(0, 2, 1), h.dw, cid + " reduced")
    dw = H.Fenced(Cout, 9 * Cin, 9 * Cin, torch.float32)
    dw.t.copy_(H.f32_dev(h.dw0.reshape(Cout, -1)))
    assert lib.gdrn_conv3x3_wgrad(C.byref(_params(H, h, x, dy, dw=dw.t)), H.stream()) == OK
    H.assert_same(dw.host(cid).reshape(Cout, 9, Cin), h.dw0 + h.dw, cid + " atomics")


# ---------------------------------------------------------------------------------------------- the reduction on its own
# (nsplit, Cout, Cin, cin_valid, layout): "oihw" = the parameter's own [Cout][cin_valid or Cin][3][3] (also ConvTranspose's [in][out][3][3] with the
# roles swapped), "pitch" = OIHW rows of all Cin channels (the skipped slots lie inside the buffer and must stay NaN), "packed" = [co][tap][ci]
REDUCE_TABLES = {
    "one": [(1, 64, 64, 0, "oihw")],
    "two": [(2, 64, 128, 69, "oihw"), (3, 64, 64, 3, "pitch")],
    "five": [(4, 128, 64, 0, "oihw"), (5, 64, 64, 3, "oihw"), (7, 64, 128, 69, "pitch"), (8, 192, 64, 0, "packed"), (9, 64, 64, 0, "pitch")],
}


@pytest.mark.parametrize("name", list(REDUCE_TABLES))
def test_reduce_hand_filled_slabs_exactly_with_skipped_slots_fenced(H, name):
    tasks, want = [], []
    for ti, (ns, Cout, Cin, civ, layout) in enumerate(REDUCE_TABLES[name]):
        n = Cout * 9 * Cin
        g = (np.arange(ns)[:, None] * 8192 + (np.arange(n)[None] * 7 + ti) % 8191).astype(np.float64).reshape(ns, Cout, 9, Cin)   # distinct per (split, element), sums exact
        ws = H.f32_dev(np.stack([WH.to_slab(g[s]) for s in range(ns)]))
        cv = civ or Cin
        s_co, s_ci, s_t = {"oihw": (cv * 9, 9, 1), "pitch": (Cin * 9, 9, 1), "packed": (9 * Cin, 1, Cin)}[layout]
        dst = H.Fenced(Cout, s_co, s_co, torch.float32, guard=2 + 4096 // s_co)
        tasks.append(dict(ws=ws, dst=dst.t, nsplit=ns, Cout=Cout, Cin=Cin, cin_valid=civ, s_co=s_co, s_ci=s_ci, s_t=s_t))
        want.append((dst, WH.reduce_ref(g, civ, s_co, s_ci, s_t, Cout * s_co)))
    assert H.wgrad_reduce(_lib(), tasks) == OK
    for ti, (dst, (ref, written)) in enumerate(want):
        got = dst.host(f"{name}[{ti}]").reshape(-1)
        assert np.array_equal(np.isnan(got), ~written), f"{name}[{ti}]: the set of written slots differs ({int(np.isnan(got).sum())} unwritten, {int((~written).sum())} expected)"
        H.assert_same(got[written], ref[written], f"{name}[{ti}]")


# ---------------------------------------------------------------------------------------------- the grouped launch
@pytest.mark.parametrize("lds", [0, 84 * 1024])
@pytest.mark.parametrize("name", list(WH.GROUPED))
def test_grouped_launch_per_element_and_bit_for_bit_with_the_single_launch(H, name, lds):
    lib, table = _lib(), WH.GROUPED[name]
    nsl, starts = WH.grouped_blocks(table)
    keep, wps, outs = [], [], []
    for (c, req), ns in zip(table, nsl):
        h = WH.halo(c, HALF)
        x, dy = H.to_dev(h.x, BF16), H.to_dev(h.dy, BF16)
        assert lib.gdrn_conv3x3_wgrad_splits(C.byref(_params(H, h, x, dy, ws=x, splits=req))) == ns
        ws = H.fenced_flat(ns * c["Cout"] * c["Cin"] * 9)
        single = H.fenced_flat(ns * c["Cout"] * c["Cin"] * 9)
        assert lib.gdrn_conv3x3_wgrad(C.byref(_params(H, h, x, dy, ws=single.t, splits=ns)), H.stream()) == OK
        wps.append(_params(H, h, x, dy, ws=ws.t, splits=ns))
        keep.append((x, dy))
        outs.append((h, ns, ws, single))
    tab = to_device_table(wps, H.DEV)
    stt = torch.tensor(starts, dtype=torch.int32, device=H.DEV)
    assert lib.gdrn_conv3x3_wgrad_multi_lds(ptr(tab), ptr(stt), len(table), starts[-1], 161 * 1024, H.stream()) == ARG
    assert all(ws.untouched() for _, _, ws, _ in outs), "a refused grouped launch wrote to a workspace"
    if lds:
        assert lib.gdrn_conv3x3_wgrad_multi_lds(ptr(tab), ptr(stt), len(table), starts[-1], lds, H.stream()) == OK
    else:
        assert lib.gdrn_conv3x3_wgrad_multi(ptr(tab), ptr(stt), len(table), starts[-1], H.stream()) == OK
    torch.cuda.synchronize()
    for ti, (h, ns, ws, single) in enumerate(outs):
        what = f"{name}[{ti}] {h.c['id']} lds={lds}"
        ref, refA, pix = h.slabs(ns)
        bnd = np.stack([WH.bound(refA[s], pix[s]) for s in range(ns)])
        within(H, _slabs(ws, ns, h.c["Cout"], h.c["Cin"], what), ref, bnd, what, "grouped")
        single.check(what)
        assert H.same_bits(ws.t, single.t), what + ": differs from the single launch of the same params"


# ---------------------------------------------------------------------------------------------- the generic kernel
def _gen_ids(cases):
    return [c["id"] for c in cases if not (IS_F16 and c["fp32"])]       # (the fp32 instantiation: in the bf16 module only)


def _gen_launch(H, g, dw_buf, **over):
    c = dict(g.c, **over)
    dt = F32 if c["fp32"] else BF16
    x, dy = H.to_dev(g.x, dt), H.to_dev(g.dy, dt)
    wp = H.wgrad_params(x, dy, dw_buf, None, c["Hi"], c["Wi"], c["Cin"], c["x_cs"], c["Ho"], c["Wo"], c["Cout"], c["dy_cs"], c["KH"], c["KW"],
                        c["stride"], c["pad"], c["M"], dt, c["splits"])
    rc = _lib().gdrn_conv_wgrad(C.byref(wp), H.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("cid", _gen_ids(WH.GEN_CASES))
def test_generic_kernel_per_element_onto_a_filled_gradient(H, cid):
    c = WH.GEN_BY_ID[cid]
    g = WH.gen(c, HALF)
    KK = c["KH"] * c["KW"]
    dw = H.Fenced(c["Cout"], KK * c["Cin"], KK * c["Cin"], torch.float32)           # (rows co >= Cout of a partial tile: the fence behind)
    dw.t.copy_(H.f32_dev(g.dw0.reshape(c["Cout"], -1)))
    assert _gen_launch(H, g, dw.t) == OK
    bco, bci = WH.gen_tile(c)
    within(H, dw.host(cid).reshape(c["Cout"], KK, c["Cin"]), g.ref, g.bound, cid, f"generic-{'fp32' if c['fp32'] else '16bit'}-{bco}x{bci}")


@pytest.mark.parametrize("cid", [c["id"] for c in WH.GEN_EXACT])
def test_generic_kernel_exact_operands_bit_for_bit_past_eight_splits(H, cid):
    c = WH.GEN_BY_ID[cid]
    g = WH.gen(c, HALF)
    assert WH.gen_splits(c)[0] > 8
    dw = H.Fenced(c["Cout"], 9 * c["Cin"], 9 * c["Cin"], torch.float32)
    dw.t.copy_(H.f32_dev(g.dw0.reshape(c["Cout"], -1)))
    assert _gen_launch(H, g, dw.t) == OK
    H.assert_same(dw.host(cid).reshape(c["Cout"], 9, c["Cin"]), g.ref, cid)


# ---------------------------------------------------------------------------------------------- refusals: return code only, outputs untouched
def test_halo_refusals_by_return_code_with_every_output_untouched(H):
    lib = _lib()
    # buffers large enough for any of the shapes below, had it been launched: 3 x 32 x 32 pixels of 256 channels, 256 x 256 gradients, 8 slabs
    x = torch.zeros(3 * 32 * 32 * 256, dtype=HT, device=H.DEV)
    dy = torch.zeros_like(x)
    dw = H.fill(H.Fenced(256, 9 * 256, 9 * 256, torch.float32))     # (finite: an atomic add onto NaN would not show)
    ws = H.fenced_flat(8 * 256 * 256 * 9)
    base = dict(Hi=16, Wi=16, Cin=64, x_cs=64, Ho=16, Wo=16, Cout=64, dy_cs=64, KH=3, KW=3, stride=1, pad=1, M=2 * 256, dt=BF16, splits=0, variant=0)

    def rc(xb=x, dyb=dy, dwb=dw.t, wsb=None, **over):
        p = dict(base, **over)
        wp = H.wgrad_params(xb, dyb, dwb, wsb, p["Hi"], p["Wi"], p["Cin"], p["x_cs"], p["Ho"], p["Wo"], p["Cout"], p["dy_cs"], p["KH"], p["KW"],
                            p["stride"], p["pad"], p["M"], p["dt"], p["splits"], p["variant"])
        ok, ns = lib.gdrn_conv3x3_wgrad_ok(C.byref(wp)), lib.gdrn_conv3x3_wgrad_splits(C.byref(wp))
        st = lib.gdrn_conv3x3_wgrad(C.byref(wp), H.stream())
        return st, ok, ns > 0, H.holds(dw) and ws.untouched()

    refused = (SHAPE, 0, False, True)
    # every condition of gdrn_conv3x3_wgrad_ok, one at a time
    for over in (dict(dt=F32), dict(KH=1), dict(KW=1), dict(KH=5, KW=5, pad=2), dict(pad=0), dict(Cin=96, x_cs=96), dict(Cout=96, dy_cs=96),
                 dict(x_cs=68), dict(dy_cs=68), dict(Wo=12, Wi=12, M=2 * 16 * 12), dict(variant=1), dict(Hi=18), dict(Wi=24),
                 dict(Ho=12, Hi=12, M=2 * 12 * 16), dict(stride=2), dict(stride=2, Hi=28, Wi=32, Ho=14, Wo=16, M=2 * 14 * 16),
                 dict(stride=2, Hi=12, Wi=32, Ho=6, Wo=16, M=2 * 6 * 16), dict(stride=3), dict(stride=0),
                 dict(Cin=0, x_cs=64), dict(Cout=0), dict(Cin=-64), dict(Ho=0, Hi=0, M=0), dict(Wo=0, Wi=0, M=0),
                 dict(Cin=128, x_cs=64), dict(Cout=128, dy_cs=64)):
        for path in (dict(), dict(dwb=None, wsb=ws.t)):
            assert rc(**path, **over) == refused, (over, list(path))
    # covered shapes the launcher still turns down
    for over in (dict(M=2 * 256 + 8), dict(M=0), dict(M=-256)):
        st, ok, ns, clean = rc(**over)
        assert (st, ok, ns, clean) == (SHAPE, 1, False, True), over
    assert rc(dwb=None, wsb=None)[0::3] == (ARG, True)
    assert rc(xb=None)[0::3] == (ARG, True)
    assert rc(dyb=None)[0::3] == (ARG, True)
    assert rc(dwb=None, wsb=ws.t, stride=2, Hi=32, Wi=32) == (OK, 1, True, False)      # the stride-2 form of the base shape runs (and writes its slabs)


def test_generic_refusals_by_return_code_with_the_gradient_untouched(H):
    c = WH.GEN_BY_ID["3x3-7x7-M147-128x128"]          # Cin 128, Cout 69 in dy_cs 128
    g = WH.gen(c, HALF)
    dw = H.fill(H.Fenced(128, 9 * 128, 9 * 128, torch.float32))
    for over, want in ((dict(Cin=96), SHAPE), (dict(Cin=0), SHAPE), (dict(Cout=0), SHAPE), (dict(M=0), SHAPE), (dict(M=146), SHAPE),
                       (dict(dy_cs=64), SHAPE),                   # below the 128-column slab of Cout = 69
                       (dict(dy_cs=132), SHAPE),                  # rows of 264 bytes: no multiple of 16
                       (dict(x_cs=131), SHAPE), (dict(x_cs=0), SHAPE), (dict(stride=0), SHAPE), (dict(stride=-1), SHAPE), (dict(KH=0), SHAPE),
                       (dict(KW=0), SHAPE), (dict(pad=-1), SHAPE), (dict(Ho=0), SHAPE), (dict(Wo=0), SHAPE), (dict(Hi=0), SHAPE), (dict(Wi=0), SHAPE)):
        assert (_gen_launch(H, g, dw.t, **over), H.holds(dw)) == (want, True), over
    dt = BF16
    x, dy = H.to_dev(g.x, dt), H.to_dev(g.dy, dt)
    mk = lambda xb, dyb, dwb, dtype: H.wgrad_params(xb, dyb, dwb, None, 7, 7, 128, 128, 7, 7, 69, 128, 3, 3, 1, 1, 147, dtype)
    for wp in (mk(x, dy, dw.t, 7), mk(None, dy, dw.t, dt), mk(x, None, dw.t, dt), mk(x, dy, None, dt)):
        assert (_lib().gdrn_conv_wgrad(C.byref(wp), H.stream()), H.holds(dw)) == (ARG, True)
    assert _lib().gdrn_conv_wgrad(None, H.stream()) == ARG


@pytest.mark.parametrize("which", ["dy", "x"])
def test_halo_offsets_past_32_bits_are_refused(H, which):
    """M * dy_cs * 2 = 2^32 (or images * Hi * Wi * x_cs * 2 = 2^32): wgrad_tile's 32-bit byte offsets would wrap.  Refused by return code on both
    paths, outputs untouched; both operands are allocated in full, so nothing here could run out of bounds.  The same strides on a small map run."""
    lib = _lib()
    B, S = 16, 256
    M = B * S * S
    x_cs, dy_cs = (64, 2048) if which == "dy" else (2048, 64)
    x = torch.empty((M, x_cs), dtype=HT, device=H.DEV)
    dy = torch.empty((M, dy_cs), dtype=HT, device=H.DEV)
    dw = H.fill(H.Fenced(64, 9 * 64, 9 * 64, torch.float32))
    ws = H.fenced_flat(64 * 64 * 9)
    mk = lambda dwb, wsb, b, s: H.wgrad_params(x, dy, dwb, wsb, s, s, 64, x_cs, s, s, 64, dy_cs, 3, 3, 1, 1, b * s * s, BF16, 1)
    for wp in (mk(dw.t, None, B, S), mk(None, ws.t, B, S)):
        assert lib.gdrn_conv3x3_wgrad_ok(C.byref(wp)) == 0 and lib.gdrn_conv3x3_wgrad_splits(C.byref(wp)) == 0
        assert lib.gdrn_conv3x3_wgrad(C.byref(wp), H.stream()) == SHAPE
        assert H.holds(dw) and ws.untouched()
    half = mk(dw.t, None, B // 2, S)                                           # 2^31 bytes: covered (asked, not launched)
    assert lib.gdrn_conv3x3_wgrad_ok(C.byref(half)) == 1
    x[:64].zero_()
    dy[:64].zero_()
    small = mk(None, ws.t, 1, 8)
    assert lib.gdrn_conv3x3_wgrad_ok(C.byref(small)) == 1
    assert lib.gdrn_conv3x3_wgrad(C.byref(small), H.stream()) == OK
    assert np.array_equal(ws.host(), np.zeros((36, 1024)))
