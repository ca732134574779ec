"""Thin test-side wrappers that call the C-ABI entry points of libgdrn_hip.so on torch tensors."""
import ctypes as C

import numpy as np
import torch

from gdrnet_amd import cabi
from gdrnet_amd.cabi import BF16, F16, F32, ConvParams, WgradParams, check, ptr

DEV = "cuda:0"


def tdt(dt):
    return {BF16: torch.bfloat16, F16: torch.float16}.get(dt, torch.float32)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ru(a, b):
    return (a + b - 1) // b * b


def rel(a, b):
    a = a.detach().double().cpu().flatten()
    b = b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(b.norm().item(), 1e-30))


def nhwc(x, dt, cpad=None):
    """NCHW fp32 cpu -> NHWC device tensor of dtype dt, channels zero-padded to cpad."""
    x = x.permute(0, 2, 3, 1).contiguous()
    if cpad is not None and cpad > x.shape[-1]:
        x = torch.nn.functional.pad(x, (0, cpad - x.shape[-1]))
    return x.to(DEV).to(tdt(dt)).contiguous()


def nchw(y, C_=None):
    y = y.float().cpu()
    if C_ is not None:
        y = y[..., :C_]
    return y.permute(0, 3, 1, 2).contiguous()


def rounded(x, dt):
    """value a tensor has after storage in dt (for building references of bf16 runs)."""
    return x.to(tdt(dt)).float()


def pack(w_src, A1, A2, T, B, A1v, A2v, Bv, s1, s2, st, sb, flip, dt):
    lib = cabi.load(dt)
    dst = torch.zeros(A1, A2, T, B, dtype=tdt(dt), device=DEV)
    w = w_src.to(DEV).float().contiguous()
    check(lib.gdrn_pack4(ptr(w), ptr(dst), A1, A2, T, B, A1v, A2v, Bv, s1, s2, st, sb, flip, dt, stream()), "pack4")
    return dst


def bn_rows(c):
    return 64 if c <= 64 else ru(c, 128)


def pack_fwd(w, dt, cin_p=None):
    """OIHW -> [rows][KK][cin_p]"""
    O, I, KH, KW = w.shape
    KK = KH * KW
    cin_p = cin_p or ru(I, 64)
    return pack(w, bn_rows(O), 1, KK, cin_p, O, 1, I, I * KK, 0, 1, KK, 0, dt).view(bn_rows(O), KK, cin_p)


def pack_dgrad(w, dt, flip, rows_valid_pad=None, cout_p=None):
    """OIHW -> [rows = in channels][KK][cout_p] (optionally tap-flipped)"""
    O, I, KH, KW = w.shape
    KK = KH * KW
    cout_p = cout_p or ru(O, 64)
    rows = bn_rows(rows_valid_pad or ru(I, 64))
    return pack(w, rows, 1, KK, cout_p, I, 1, O, KK, 0, 1, I * KK, flip, dt).view(rows, KK, cout_p)


def conv_gemm(x, w, B, Hi, Wi, Cin, x_cs, Ho, Wo, Cout, KH, KW, stride, pad, dt, mode=0, bias=None, addend=None, act=0,
              out_f32=0, y_cs=None, want_stats=False, halo=False, bnb=None, xf=None, v3=False, reps=0,
              y_buf=None, stats_buf=None, rows_buf=None, w_rows=None, halo_waves=None, prepacked=False, rc=False, info=None):
    """bnb (halo and generic kernel, bf16): dict(x, mask|None, mean, invstd, scale|None, shift|None) -> fused BatchNorm-backward statistics;
    the second return value is then the [tiles][2][Cout] rows buffer.
    xf (halo only): dict(mode, relu, x2, a, b, c, c2, msc, msh, out) device tensors -> operand transform while staging.
    v3 (with halo): True = the second-generation kernel (operand of gdrn_pack_wfrag32, w_frag = 2); 4 / 8 = the first kernel with
    gdrn_conv_params.halo_waves forced (the default, 0, lets the library pick by grid size: the small test grids get the eight-wave form).
    reps > 0: also time `reps` back-to-back launches with HIP events; the average (ms) is returned as a third value.
    Optional, for tests/test_conv3x3_edges_gpu.py (the defaults are what every other caller gets): y_buf / stats_buf / rows_buf = the caller's
    own (fenced) output, statistics and BatchNorm-backward rows tensors instead of fresh ones; w_rows / halo_waves = the values to put into
    gdrn_conv_params whatever w and v3 say; prepacked = w is passed as it is; rc = return the entry point's status instead of raising on
    it; info = a dict that receives the library's own answers for the launch (tile, halo_waves, stats_rows)."""
    lib = cabi.load(dt)
    waves = v3 if (v3 is not True and v3 in (4, 8)) else 0   # v3 = 4 / 8: first halo kernel, forced four- / eight-wave form (halo_waves)
    v3 = v3 is True
    if halo and not prepacked:  # the halo kernels take a fragment-major permutation of the same operand
        wf = torch.empty_like(w)
        check((lib.gdrn_pack_wfrag32 if v3 else lib.gdrn_pack_wfrag)(ptr(w), ptr(wf), w.shape[0], Cin, dt, stream()), "pack_wfrag")
        w = wf
    y_cs = y_cs or ru(Cout, 4)
    ydt = torch.float32 if (out_f32 or dt == F32) else tdt(dt)
    y = y_buf if y_buf is not None else torch.full((B, Ho, Wo, y_cs), float("nan"), dtype=ydt, device=DEV)
    cp = ConvParams()
    cp.x, cp.w, cp.y = ptr(x), ptr(w), ptr(y)
    cp.bias, cp.addend = ptr(bias), ptr(addend)
    cp.Hi, cp.Wi, cp.Cin, cp.x_cs = Hi, Wi, Cin, x_cs
    cp.Ho, cp.Wo, cp.Cout, cp.y_cs = Ho, Wo, Cout, y_cs
    cp.add_cs = addend.shape[-1] if addend is not None else 0
    cp.KH, cp.KW, cp.stride, cp.pad = KH, KW, stride, pad
    cp.mode, cp.act, cp.out_f32 = mode, act, out_f32
    cp.M = B * (Ho // 2) * (Wo // 2) if mode == 1 else B * Ho * Wo
    cp.w_rows, cp.dtype = (w.shape[0] if w_rows is None else w_rows), dt
    cp.w_frag = 2 if (halo and v3) else 0
    cp.halo_waves = (waves if halo else 0) if halo_waves is None else halo_waves
    cp.v3_min_wg = 1   # the 256-channel tile of the second-generation kernel also on the small grids of these tests
    # (every operand goes in before the tile / statistics-row queries: the second-generation kernel's tile depends on them)
    if bnb is not None:
        cp.bnb_mask = ptr(bnb.get("mask"))
    if xf is not None:
        cp.xf_mode, cp.xf_relu = xf["mode"], 1 if xf.get("relu") else 0
        cp.xf_x2, cp.xf_a, cp.xf_b, cp.xf_c, cp.xf_c2 = ptr(xf.get("x2")), ptr(xf.get("a")), ptr(xf.get("b")), ptr(xf.get("c")), ptr(xf.get("c2"))
        cp.xf_msc, cp.xf_msh, cp.xf_out = ptr(xf.get("msc")), ptr(xf.get("msh")), ptr(xf.get("out"))
    stats = None
    if want_stats:
        rows = (lib.gdrn_conv3x3_stats_rows if halo else lib.gdrn_conv_stats_rows)(C.byref(cp))
        stats = stats_buf if stats_buf is not None else torch.zeros(rows, 2, Cout, dtype=torch.float32, device=DEV)
        cp.stats = ptr(stats)
    if bnb is not None:
        nrows = (lib.gdrn_conv3x3_stats_rows if halo else lib.gdrn_conv_stats_rows)(C.byref(cp))
        rows_t = rows_buf if rows_buf is not None else torch.full((nrows, 2, Cout), float("nan"), dtype=torch.float32, device=DEV)
        cp.bnb_x, cp.bnb_mask, cp.bnb_cs = ptr(bnb["x"]), ptr(bnb.get("mask")), bnb["x"].shape[-1]
        cp.bnb_mean, cp.bnb_invstd, cp.bnb_scale, cp.bnb_shift = ptr(bnb["mean"]), ptr(bnb["invstd"]), ptr(bnb.get("scale")), ptr(bnb.get("shift"))
        cp.bnb_rows = ptr(rows_t)
        stats = rows_t  # per-tile rows [nrows][2][Cout]: callers sum over dim 0
    fn = lib.gdrn_conv3x3_halo if halo else lib.gdrn_conv_gemm
    if info is not None and halo:
        th, tw, bn = C.c_int(0), C.c_int(0), C.c_int(0)
        lib.gdrn_conv3x3_tile(C.byref(cp), C.byref(th), C.byref(tw), C.byref(bn))
        info.update(tile=(th.value, tw.value, bn.value), halo_waves=lib.gdrn_conv3x3_halo_waves(C.byref(cp)),
                    stats_rows=lib.gdrn_conv3x3_stats_rows(C.byref(cp)))
    if rc:
        status = fn(C.byref(cp), stream())
        torch.cuda.synchronize()
        return status
    check(fn(C.byref(cp), stream()), "conv")
    torch.cuda.synchronize()
    if reps > 0:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(C.byref(cp), stream())
        e1.record()
        torch.cuda.synchronize()
        return y, stats, e0.elapsed_time(e1) / reps
    return y, stats


def conv_wgrad(x, dy, B, Hi, Wi, Cin, x_cs, Ho, Wo, Cout, dy_cs, KH, KW, stride, pad, dt, variant=0, splits=0, halo=False, ws=False):
    """ws: halo kernel with workspace partials + gdrn_wgrad_reduce_multi; returns the OIHW gradient in that case."""
    lib = cabi.load(dt)
    dw = torch.zeros(Cout, KH * KW, Cin, dtype=torch.float32, device=DEV)
    wp = WgradParams()
    wp.x, wp.dy, wp.dw = ptr(x), ptr(dy), ptr(dw)
    wp.Hi, wp.Wi, wp.Cin, wp.x_cs = Hi, Wi, Cin, x_cs
    wp.Ho, wp.Wo, wp.Cout, wp.dy_cs = Ho, Wo, Cout, dy_cs
    wp.KH, wp.KW, wp.stride, wp.pad = KH, KW, stride, pad
    wp.M, wp.dtype, wp.splits, wp.variant = B * Ho * Wo, dt, splits, variant
    if halo:
        assert lib.gdrn_conv3x3_wgrad_ok(C.byref(wp)) == 1
    if ws:
        from gdrnet_amd.cabi import WreduceTask, to_device_table

        wp.ws = ptr(dw)  # non-null: query the split count of the workspace mode
        ns = lib.gdrn_conv3x3_wgrad_splits(C.byref(wp))
        assert ns >= 1
        wsb = torch.full((ns * Cout * Cin * 9,), float("nan"), dtype=torch.float32, device=DEV)  # every slab must be written
        wp.ws, wp.dw = ptr(wsb), None
        check(lib.gdrn_conv3x3_wgrad(C.byref(wp), stream()), "conv3x3_wgrad(ws)")
        grad = torch.full((Cout, Cin, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
        tab = to_device_table([WreduceTask(ws=ptr(wsb), dst=ptr(grad), nsplit=ns, Cout=Cout, Cin=Cin, cin_valid=0, s_co=Cin * 9, s_ci=9, s_t=1)], DEV)
        stt = torch.tensor([0, Cout * Cin // 256], dtype=torch.int32, device=DEV)
        check(lib.gdrn_wgrad_reduce_multi(ptr(tab), ptr(stt), 1, Cout * Cin // 256, stream()), "wgrad_reduce_multi")
        torch.cuda.synchronize()
        return grad
    check((lib.gdrn_conv3x3_wgrad if halo else lib.gdrn_conv_wgrad)(C.byref(wp), stream()), "conv_wgrad")
    torch.cuda.synchronize()
    return dw


def randn(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


# ---------------------------------------------------------------------------------------------- helpers of tests/test_norm_edges_gpu.py
KIND = {F32: "fp32", BF16: "bf16", F16: "fp16"}   # the storage-type names of tests/norm_host.py


def to_dev(a, dt):
    """numpy array of values that are exact in storage type dt -> device tensor of that type"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(tdt(dt)).to(DEV).contiguous()   # (converted on the host)


def f32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def nans(shape, dtype=torch.float32):
    """an output buffer no element of which may survive (uint8: 0xff, not a tap code)"""
    if dtype == torch.uint8:
        return torch.full(tuple(shape), 255, dtype=dtype, device=DEV)
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=DEV)


def to_host(t):
    return t.detach().cpu().to(torch.float64).numpy()


def rows_buf(nrows, C_):
    """partial-row buffer sized by the library's own *_rows query plus ONE guard row of NaN that must stay NaN"""
    return nans((nrows + 1, 2, C_))


def rows_total(buf, nrows):
    """fp64 sum of the partial rows; every row written (no NaN left), the guard row untouched"""
    torch.cuda.synchronize()
    h = to_host(buf)
    assert not np.isnan(h[:nrows]).any(), "a partial row was not written"
    assert np.isnan(h[nrows]).all(), "the guard row behind the partial rows was written"
    return h[:nrows].sum(0)


def assert_within(got, ref, bnd, what, exact=None):
    """per element |got - ref| <= bnd (no NaN); where `exact` is set got == ref bit for bit.  Reports the first few offenders with their index."""
    got, ref, bnd = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.broadcast_to(np.asarray(bnd, dtype=np.float64), np.shape(ref))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= bnd)     # (NaN compares false: an unwritten element is an offender)
    if exact is not None:
        bad |= np.broadcast_to(exact, ref.shape) & (got != ref)
    if bad.any():
        idx = np.argwhere(bad)
        lines = [f"  {tuple(int(v) for v in i)}: got {got[tuple(i)]!r} want {ref[tuple(i)]!r} bound {bnd[tuple(i)]:.3e}" for i in idx[:6]]
        raise AssertionError(f"{what}: {len(idx)} of {bad.size} elements outside their bound, first at\n" + "\n".join(lines))


def assert_same(got, want, what):
    """exact comparison of discrete outputs (tap codes, masks, bit patterns) with an index report"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        idx = np.argwhere(bad)
        lines = [f"  {tuple(int(v) for v in i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}" for i in idx[:6]]
        raise AssertionError(f"{what}: {len(idx)} of {bad.size} elements differ, first at\n" + "\n".join(lines))


class Guarded:
    """an output tensor of `shape` pre-filled with NaN (uint8: 0xff) inside a buffer with one more innermost row behind it that must stay as it is"""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.buf = nans((self.n + int(shape[-1]),), dtype)
        self.t = self.buf[:self.n].view(tuple(shape))

    def host(self, what="output"):
        torch.cuda.synchronize()
        tail = self.buf[self.n:]
        assert bool((tail == 255).all() if tail.dtype == torch.uint8 else torch.isnan(tail).all()), f"{what}: written past its end"
        return self.t.cpu().numpy() if self.t.dtype == torch.uint8 else to_host(self.t)


# ---------------------------------------------------------------------------------------------- helpers of tests/test_conv3x3_edges_gpu.py
FENCE = {torch.int16: 0x7FB5, torch.int32: 0x7FB5A5A5}   # a NaN with a payload in bf16, fp16 and fp32: a guard must come back bit for bit


class Fenced:
    """a [rows][cs] tensor of `dtype` with `guard` rows in front of it and behind it; the guard rows and the pad columns >= C hold FENCE, the
    interior NaN.  check(): every fence element is still the same bits; host(): the interior [rows][C] in fp64 (after check())."""

    def __init__(self, rows, cs, C_, dtype, guard=2):
        it = torch.int32 if dtype == torch.float32 else torch.int16
        self.rows, self.cs, self.C, self.guard, self.pat = rows, cs, C_, guard, FENCE[it]
        self.raw = torch.full(((rows + 2 * guard), cs), self.pat, dtype=it, device=DEV)
        self.all = self.raw.view(dtype)
        self.t = self.all[guard:guard + rows]
        self.t[:, :C_] = float("nan")

    def check(self, what="output"):
        torch.cuda.synchronize()
        g = self.guard
        r = self.raw.cpu().numpy()
        assert (r[:g] == self.pat).all(), f"{what}: written in front of its first row"
        assert (r[g + self.rows:] == self.pat).all(), f"{what}: written behind its last row"
        assert (r[g:g + self.rows, self.C:] == self.pat).all(), f"{what}: pad columns written"

    def host(self, what="output"):
        self.check(what)
        return to_host(self.t[:, :self.C])

    def untouched(self):
        torch.cuda.synchronize()
        g = self.guard   # (on the device: the refusal tests hold buffers of 256 MB)
        fence = (self.raw[:g] == self.pat).all() & (self.raw[g + self.rows:] == self.pat).all() & (self.raw[:, self.C:] == self.pat).all()
        return bool(fence) and bool(torch.isnan(self.t[:, :self.C]).all())


# ---------------------------------------------------------------------------------------------- helpers of tests/test_wgrad_edges_gpu.py
def wgrad_params(x, dy, dw, ws, Hi, Wi, Cin, x_cs, Ho, Wo, Cout, dy_cs, KH, KW, stride, pad, M, dt, splits=0, variant=0):
    """gdrn_wgrad_params of tensors (or None) -- nothing is checked here: the refusal tests pass shapes the library must turn down"""
    wp = WgradParams()
    wp.x, wp.dy, wp.dw, wp.ws = ptr(x), ptr(dy), ptr(dw), ptr(ws)
    wp.Hi, wp.Wi, wp.Cin, wp.x_cs = Hi, Wi, Cin, x_cs
    wp.Ho, wp.Wo, wp.Cout, wp.dy_cs = Ho, Wo, Cout, dy_cs
    wp.KH, wp.KW, wp.stride, wp.pad = KH, KW, stride, pad
    wp.M, wp.dtype, wp.splits, wp.variant = M, dt, splits, variant
    return wp


def fenced_flat(n, row=1024):
    """n fp32 elements (a multiple of `row`) as a Fenced buffer of rows of `row`: workspace slabs and flat gradients"""
    assert n % row == 0
    return Fenced(n // row, row, row, torch.float32)


def same_bits(a, b):
    """two fp32 device tensors hold the same bit patterns (NaN payloads included)"""
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def wgrad_reduce(lib, tasks):
    """gdrn_wgrad_reduce_multi on a table of dict(ws, dst, nsplit, Cout, Cin, cin_valid, s_co, s_ci, s_t) (ws, dst: tensors); the status"""
    from gdrnet_amd.cabi import WreduceTask, to_device_table

    tab = to_device_table([WreduceTask(ws=ptr(t["ws"]), dst=ptr(t["dst"]), nsplit=t["nsplit"], Cout=t["Cout"], Cin=t["Cin"], cin_valid=t["cin_valid"],
                                       s_co=t["s_co"], s_ci=t["s_ci"], s_t=t["s_t"]) for t in tasks], DEV)
    starts = [0]
    for t in tasks:
        starts.append(starts[-1] + t["Cout"] * t["Cin"] // 256)
    stt = torch.tensor(starts, dtype=torch.int32, device=DEV)
    rc = lib.gdrn_wgrad_reduce_multi(ptr(tab), ptr(stt), len(tasks), starts[-1], stream())
    torch.cuda.synchronize()
    return rc


def fill(f, value=1.0):
    """give the interior of a Fenced buffer a finite value: an atomic add onto NaN leaves NaN, so `untouched()` cannot see it"""
    f.t[:, :f.C] = value
    return f


def holds(f, value=1.0):
    """the fences of a Fenced buffer are intact and its interior still holds `value` everywhere"""
    torch.cuda.synchronize()
    g = f.guard
    fence = (f.raw[:g] == f.pat).all() & (f.raw[g + f.rows:] == f.pat).all() & (f.raw[:, f.C:] == f.pat).all()
    return bool(fence) and bool((f.t[:, :f.C] == value).all())
