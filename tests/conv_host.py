"""Independent yardstick of the stride-1 3x3 halo conv kernels (csrc/conv3x3_halo.hip, conv3x3_v3.hip, block64.hip): plain numpy restatements in
fp64 of the convolution, its epilogues, the per-tile statistics rows, the fused BatchNorm-backward epilogue and the operand transforms of
halo_xf.h, on NHWC arrays, no device code and nothing from the library.  Operands enter as the values they have after storage (16-bit rounded
x, w, addend; fp32 bias and per-channel vectors).  tests/test_conv_host_cpu.py pins this module against F.conv2d in fp64 and shows that each
mutated reference of mutate() leaves its bound; tests/test_conv3x3_edges_gpu.py holds the kernels to it.

Layout: x [B][H][W][Cin]; w [rows >= Cout][9][Cin], tap t = 3 ky + kx, the row-major operand gdrn_pack_wfrag permutes; y [B][H][W][Cout];
statistics rows [tiles][2][Cout], tile mt = (n * (H / th) + ty) * (W / tw) + tx (the kernels' `mt`).

The bound of an output element (bound()):

    |got - ref| <= (1 + u) * k * 2^-23 * A + max(u * |ref|, tiny)

A = sum |x w| + |bias| + |addend| (the reference's expression on absolute values), u the unit roundoff of the OUTPUT format (2^-8 bf16, 2^-11
fp16, 0 for fp32 output), tiny half the spacing of the format's subnormals (2^-25 for fp16: an activation of 2e-5 sits on a grid of 2^-24).
k counts the fp32 operations on the kernel's path (k_conv()); its unit is a WHOLE ulp, 2^-23, not the half ulp of round-to-nearest, so the
bound holds however the matrix unit rounds its internal adds (truncation included) and covers the second-order terms of the chain.  No
constant here comes from a device result."""
import numpy as np

import norm_host as NH

ULP32 = 2.0 ** -23
U_STORE = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}
TINY = {"bf16": 2.0 ** -134, "fp16": 2.0 ** -25, "fp32": 2.0 ** -150}   # half the subnormal spacing of the format (norm_host.TINY)
SLOPE = NH.SLOPE                                                       # act 2: the kernel's constant 0.1f
POISON = {"fp32": 1e30, "bf16": 1e30, "fp16": 6e4}                     # operand pad channels no kernel may read (finite: a NaN hides in fmaxf)
OLD_TOL = {"bf16": 6e-3, "fp16": 8e-4, "fp32": 2e-5}                   # the Frobenius tolerances of tests/test_kernels_gpu.py

f64 = NH.f64
store = NH.store


# ------------------------------------------------------------------------------------------------ the operation counts
def k_conv(Cin, act=0, fp32=False):
    """fp32 operations between the exact products and the stored value, per output element.
    16-bit operands: a product of two 8- or 11-bit significands is exact in fp32, so the 9 Cin products cost nothing and the 9 Cin
    accumulations one rounding each (the first add to the zeroed accumulator is exact; it pays for the matrix unit's own order inside a
    k-step).  Epilogue: + 1 the meeting of the two partial accumulators of the eight-wave / K-split forms, + 1 bias, + 1 addend (counted
    whether present or not: the bound is one formula for every form), -> 9 Cin + 3.  act 2 multiplies by 0.1f: + 1.
    fp32 instantiation: operands are fp32, every product rounds (+ 9 Cin; v_mfma_f32_16x16x4_f32 may fuse them, the count does not rely on
    it), and every 32-channel tap stage accumulates in a fresh tile that is then added to the running sum: + 9 Cin / 32 partial adds."""
    k = 9 * Cin + 3 + (1 if act == 2 else 0)
    if fp32:
        k += 9 * Cin + 9 * Cin // 32
    return k


# operand transforms (halo_xf.h), fp32 roundings before the one rounding to the 16-bit format:
#   mode 1: fma(x, a, c) -> 1.   mode 2: fma(x, a, c) [1] + q [1], q = the second branch fma(x2, b, c2) rounded to 16 bits ON ITS OWN (part of
#   the operation's definition: xf_ref() restates it, see there) -> 2.   modes 3, 4: fma(a, x, fma(b, x2, c)) -> 2 (the mask of mode 4 selects).
K_XF = {1: 1, 2: 2, 3: 2, 4: 2}


def bound(ref, A, k, kind):
    u = U_STORE[kind]
    return (1.0 + u) * k * ULP32 * f64(A) + np.maximum(u * np.abs(f64(ref)), TINY[kind])


# ------------------------------------------------------------------------------------------------ the convolution
def _pad1(x):
    return np.pad(f64(x), ((0, 0), (1, 1), (1, 1), (0, 0)))


def _tap(xp, w, t, H, W, ch=slice(None)):
    """contribution of tap t (channels ch) to every output pixel: [B][H][W][rows]"""
    ky, kx = divmod(t, 3)
    v = np.ascontiguousarray(xp[:, ky:ky + H, kx:kx + W, ch])
    return (v.reshape(-1, v.shape[-1]) @ w[:, t, ch].T).reshape(v.shape[:3] + (w.shape[0],))


def acc(x, w, Cout=None):
    """the accumulators: (sum over taps and channels of x w, the same sum on absolute values), [B][H][W][Cout] in fp64"""
    x, w = f64(x), f64(w)[:Cout]
    B, H, W, Cin = x.shape
    w = w[:, :, :Cin]
    xp, xa, wa = _pad1(x), _pad1(np.abs(x)), np.abs(w)
    v, A = 0.0, 0.0
    for t in range(9):
        v = v + _tap(xp, w, t, H, W)
        A = A + _tap(xa, wa, t, H, W)
    return v, A


def epilogue(v, A, bias=None, addend=None, act=0):
    """(y, A) after bias [Cout], addend [B][H][W][Cout] and the activation (0 none, 1 ReLU, 2 leaky 0.1f)"""
    Cout = v.shape[-1]
    if bias is not None:
        v, A = v + f64(bias)[:Cout], A + np.abs(f64(bias)[:Cout])
    if addend is not None:
        v, A = v + f64(addend)[..., :Cout], A + np.abs(f64(addend)[..., :Cout])
    if act == 1:
        v = np.maximum(v, 0.0)
    elif act == 2:
        v = np.where(v > 0.0, v, SLOPE * v)
    return v, A


def conv(x, w, Cout=None, bias=None, addend=None, act=0, kind="bf16", fp32=False):
    """(y, A, bound) of the forward conv; kind = the OUTPUT format, fp32 = the fp32 instantiation"""
    v, A = acc(x, w, Cout)
    y, A = epilogue(v, A, bias, addend, act)
    return y, A, bound(y, A, k_conv(np.shape(x)[-1], act, fp32), kind)


def dgrad_operand(w):
    """forward weights [Cout][9][Cin] -> the data gradient's operand [Cin][9 taps, flipped][Cout]: dx = conv(dy, dgrad_operand(w))"""
    return np.ascontiguousarray(f64(w)[:, ::-1, :].transpose(2, 1, 0))


def dgrad(dy, w, **kw):
    """(dx, A, bound): dx[b][h][w][ci] = sum dy[b][h - ky + 1][w - kx + 1][co] w[co][ky][kx][ci]"""
    return conv(dy, dgrad_operand(w), **kw)


# ------------------------------------------------------------------------------------------------ tiles and statistics rows
def tile_of(B, H, W, th, tw):
    """the statistics row (the kernels' mt) of every pixel: [B][H][W]"""
    n, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    return (n * (H // th) + y // th) * (W // tw) + x // tw


def n_tiles(B, H, W, th, tw):
    return B * (H // th) * (W // tw)


def grid_size(B, H, W, Cout, th, tw, bn):
    return n_tiles(B, H, W, th, tw) * (-(-Cout // bn))


def _tile_sum(a, mt, nt):
    out = np.zeros((nt, a.shape[-1]))
    np.add.at(out, mt.reshape(-1), a.reshape(-1, a.shape[-1]))
    return out


def stats_rows(v, A, k, th, tw):
    """rows [tiles][2][Cout] of (sum v, sum v^2) over each tile's pixels -- v the fp32 ACCUMULATORS (no bias, no addend, not the rounded
    output) -- and their bounds.  An accumulator carries b = k 2^-23 A.  Row 0: sum b, plus n_pix adds (in-lane walk, lane reduction, wave
    partials: fewer than the th tw pixels of a tile) each relative to a partial sum <= sum |v|.  Row 1: a square carries 2 |v| b + b^2 and its
    own rounding 2^-23 v^2; the adds as above relative to sum v^2."""
    B, H, W, _ = v.shape
    mt, nt, npix = tile_of(B, H, W, th, tw), n_tiles(B, H, W, th, tw), th * tw
    b = k * ULP32 * A
    rows = np.stack([_tile_sum(v, mt, nt), _tile_sum(v * v, mt, nt)], 1)
    bnd = np.stack([_tile_sum(b, mt, nt) + npix * ULP32 * _tile_sum(np.abs(v), mt, nt),
                    _tile_sum(2 * np.abs(v) * b + b * b, mt, nt) + (npix + 1) * ULP32 * _tile_sum(v * v, mt, nt)], 1)
    return rows, bnd


# ------------------------------------------------------------------------------------------------ the fused BatchNorm-backward epilogue
def bnb(v, A, k, th, tw, kind, addend, bx, mean, invstd, mask=None, scale=None, shift=None):
    """data gradient feeding a BatchNorm(+ReLU) backward: g = (v + addend) where kept, else exactly 0; kept = (mask > 0) [stored],
    (bx scale + shift > 0) [affine] or everywhere [none]; rows [tiles][2][Cout] of (sum g, sum g (bx - mean) invstd) taken from the fp32 g
    BEFORE its store.  Returns dict(g, gbound, keep, marginal, rows, rbound).  `marginal`: affine arguments within 4 * 2^-24 (|bx scale| +
    |shift|) of zero, whose sign fp32 does not determine (the cases use power-of-two scales and quarter-integer shifts: the argument is
    exact and none is marginal -- the CPU module checks that).
    Bounds: g carries bg = k 2^-23 A (the addend's add is in k, its magnitude in A); row 0 as stats_rows; a term of row 1 is g (bx - mean) invstd: 3 roundings relative to |g| (|bx| + |mean|) |invstd| = |g| xh, plus bg xh."""
    Cout = v.shape[-1]
    g, Ag = epilogue(v, A, None, addend, 0)
    bx, mean, invstd = f64(bx)[..., :Cout], f64(mean)[:Cout], f64(invstd)[:Cout]
    keep = np.ones(g.shape, dtype=bool)
    marginal = np.zeros(g.shape, dtype=bool)
    if mask is not None:
        keep = f64(mask)[..., :Cout] > 0.0
    elif scale is not None:
        arg = bx * f64(scale)[:Cout] + f64(shift)[:Cout]
        keep = arg > 0.0
        marginal = (arg != 0.0) & (np.abs(arg) <= 4 * NH.EPS32 * (np.abs(bx * f64(scale)[:Cout]) + np.abs(f64(shift)[:Cout])))
    g = np.where(keep, g, 0.0)
    bg = np.where(keep, k * ULP32 * Ag, 0.0)
    B, H, W, _ = g.shape
    mt, nt, npix = tile_of(B, H, W, th, tw), n_tiles(B, H, W, th, tw), th * tw
    xh = (np.abs(bx) + np.abs(mean)) * np.abs(invstd)
    t2 = g * (bx - mean) * invstd
    rows = np.stack([_tile_sum(g, mt, nt), _tile_sum(t2, mt, nt)], 1)
    rb = np.stack([_tile_sum(bg, mt, nt) + npix * ULP32 * _tile_sum(np.abs(g), mt, nt),
                   _tile_sum(bg * xh + 3 * ULP32 * np.abs(g) * xh, mt, nt) + npix * ULP32 * _tile_sum(np.abs(g) * xh, mt, nt)], 1)
    u = U_STORE[kind]
    return dict(g=g, gbound=(1.0 + u) * bg + np.where(keep, np.maximum(u * np.abs(g), TINY[kind]), 0.0), keep=keep, marginal=marginal,
                rows=rows, rbound=rb)


# ------------------------------------------------------------------------------------------------ operand transforms (halo_xf.h)
def _fma32(a, b, c):
    """fmaf on fp32-representable inputs: the product of a 16-bit value and an fp32 value has <= 35 significant bits and is exact in fp64, the
    sum rounds to fp64 and then to fp32 (a double rounding differs from fmaf only where the fp64 sum lands within 2^-53 relative of an fp32
    tie: not with these operands' magnitudes more often than once in 2^29 elements)"""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32).astype(np.float64)


def xf_ref(mode, relu, x, x2=None, a=None, b=None, c=None, c2=None, msc=None, msh=None, kind="bf16"):
    """the conv's input v(x, x2) per element in fp64, its magnitude A_v and its bound (K_XF roundings, one store to `kind`).  NULL a / b are 1,
    NULL c2 is 0 (gdrn_hip.h).  Mode 2's second branch q is DEFINED as a value rounded to the 16-bit format (the separate pass that produced
    it stored it): it is restated operation by operation (fp32 fma, one rounding) so that the reference holds the same q; mode 4's mask is the
    sign of fmaf(x2, msc, msh), restated the same way."""
    x = f64(x)
    one = np.ones(x.shape[-1])
    a = one if a is None else f64(a)
    c = f64(c)
    if mode == 1:
        v, A = x * a + c, np.abs(x) * np.abs(a) + np.abs(c)
    else:
        x2 = f64(x2)
        b = one if b is None else f64(b)
        if mode == 2:
            q = store(_fma32(x2, b, np.zeros_like(one) if c2 is None else c2), kind)
            v, A = (x * a + c) + q, np.abs(x) * np.abs(a) + np.abs(c) + np.abs(q)
        else:
            if mode == 4:
                x = np.where(_fma32(x2, msc, msh) > 0.0, x, 0.0)
            v, A = a * x + (b * x2 + c), np.abs(a) * np.abs(x) + np.abs(b) * np.abs(x2) + np.abs(c)
    if relu:
        v = np.maximum(v, 0.0)
    return v, A, bound(v, A, K_XF[mode], kind)


# ------------------------------------------------------------------------------------------------ block64: two convs, the intermediate in the storage format
def _spacing(a, kind):
    """spacing of the 16-bit format's grid at |a| (the binade's, at least the subnormal spacing)"""
    bits, emin = (8, -126) if kind == "bf16" else (11, -14)
    e = np.frexp(np.abs(a))[1] - 1                       # |a| in [2^e, 2^(e+1))
    return np.ldexp(1.0, np.maximum(e, emin) - (bits - 1))


def block64(x, w1, b1, w2, b2, kind):
    """y = relu(conv2(a1) + b2 + x), a1 = the storage format's rounding of relu(conv1(x) + b1): (y, A, bound, a1, share of flippable
    intermediates).  The device's fp32 accumulator of conv1 sits within e1 = k 2^-23 A1 of the fp64 value; where that value lies within e1
    of a rounding tie of the 16-bit grid the device may legitimately store the OTHER neighbour, one grid spacing away (`flip`).  conv2's
    bound is its own plus sum |w2| flip over its taps: rigorous, and zero for the majority of intermediates that sit clear of every tie."""
    v1, A1 = acc(x, w1, 64)
    t1, A1 = epilogue(v1, A1, b1, None, 1)
    a1 = store(t1, kind)
    e1 = k_conv(64) * ULP32 * A1
    sp = _spacing(np.where(a1 != 0, a1, t1), kind)
    flip = np.where((t1 > 0) & (0.5 * sp - np.abs(t1 - a1) <= e1), sp, 0.0)
    flip = flip + np.where(np.abs(t1) <= e1, np.abs(a1) + e1, 0.0)      # within e1 of the ReLU's kink: the device may hold 0 or a value <= 2 e1
    v2, A2 = acc(a1, w2, 64)
    extra, _ = acc(flip, np.abs(f64(w2)), 64)
    y, A = epilogue(v2, A2, b2, f64(x)[..., :64], 1)
    return y, A, bound(y, A, k_conv(64), kind) + extra, a1, float((flip > 0).mean())


# ------------------------------------------------------------------------------------------------ mutated references
MUTATIONS = ("corner_tap", "edge_tap", "left_halo_wraps", "bottom_halo_next_image", "hw_swapped", "taps_not_flipped", "last_kstep_dropped",
             "chunk_read_twice", "interleave_undone", "dead_element", "partials_16bit", "stats_from_rounded", "stats_row_neighbour",
             "addend_stride")


def interleaved_channel(cb, rr, bn):
    """output channel of fragment row rr of 16-row block cb in gdrn_pack_wfrag's order (the 128-channel tile interleaves the two blocks of a
    32-channel group in units of 4 rows; the 64-channel tile keeps the natural order)"""
    F = 1 if bn <= 64 else 2
    return (cb // F) * 16 * F + (rr >> 2) * (4 * F) + (cb % F) * 4 + (rr & 3)


def mutate(name, c):
    """the result a kernel with defect `name` would store: (what, array, region).  `what` is "y" (output [B][H][W][Cout] BEFORE the store
    rounding unless the defect is the rounding) or "rows" (statistics rows); `region` marks the elements the defect may move -- every other
    element equals the reference.  c: dict(x, w, Cout, bias, addend (a [M][add_cs] buffer), add_cs, y_cs, act, kind, th, tw, bn) and, for
    taps_not_flipped, wf (the forward weights of a data gradient whose operand c["w"] is)."""
    x, w, Cout = f64(c["x"]), f64(c["w"])[:c["Cout"]], c["Cout"]
    B, H, W, Cin = x.shape
    kind, th, tw = c["kind"], c["th"], c["tw"]
    add = None if c.get("addend") is None else f64(c["addend"]).reshape(B, H, W, -1)[..., :Cout]
    ep = lambda v: epilogue(v, np.zeros_like(v), c.get("bias"), add, c.get("act", 0))[0]
    v, A = acc(x, w)
    xp = _pad1(x)
    region = np.zeros(v.shape, dtype=bool)
    mt = tile_of(B, H, W, th, tw)
    if name == "corner_tap":                       # the centre tap dropped at the last pixel of the last image
        d = _tap(xp, w, 4, H, W)
        region[B - 1, H - 1, W - 1] = True
        return "y", ep(v - np.where(region, d, 0.0)), region
    if name == "edge_tap":                         # the tap above (ky = 0, kx = 1) dropped along the bottom edge
        d = _tap(xp, w, 1, H, W)
        region[:, H - 1] = True
        return "y", ep(v - np.where(region, d, 0.0)), region
    if name == "left_halo_wraps":                  # x = -1 read as the flat pixel in front: the previous row's last pixel (image 0, row 0: zero)
        flat = np.concatenate([np.zeros((1, Cin)), x.reshape(-1, Cin)])[:-1].reshape(B, H, W, Cin)   # flat[p] = x[p - 1]
        m = v.copy()
        for ky in range(3):                         # tap (ky, kx = 0) of output pixel (h, 0) reads flat pixel (h + ky - 1, 0) - 1
            for h in range(H):
                r = h + ky - 1
                if 0 <= r < H:
                    m[:, h, 0] += flat[:, r, 0] @ w[:, 3 * ky].T
        region[:, :, 0] = True
        return "y", ep(m), region
    if name == "bottom_halo_next_image":           # y = H read as the next image's first row (last image: zero)
        nxt = np.concatenate([x[1:, 0], np.zeros((1, W, Cin))])               # [B][W][Cin]
        np_ = np.pad(nxt, ((0, 0), (1, 1), (0, 0)))
        m = v.copy()
        for kx in range(3):
            m[:, H - 1] += (np_[:, kx:kx + W].reshape(-1, Cin) @ w[:, 6 + kx].T).reshape(B, W, Cout)
        region[:B - 1, H - 1] = True
        return "y", ep(m), region
    if name == "hw_swapped":                       # the map walked as [W][H]
        m, _ = acc(x.reshape(B, W, H, Cin), w)
        region[:] = True
        return "y", ep(m.reshape(B, H, W, Cout)), region
    if name == "taps_not_flipped":
        m, _ = acc(x, np.ascontiguousarray(f64(c["wf"]).transpose(2, 1, 0)))
        region[:] = True
        return "y", ep(m), region
    if name == "last_kstep_dropped":               # tap 8, the last 32 channels, in the last tile
        region[mt == mt.max()] = True
        d = _tap(xp, w, 8, H, W, slice(Cin - 32, Cin))
        return "y", ep(v - np.where(region, d, 0.0)), region
    if name == "chunk_read_twice":                 # the third 64-channel chunk of the patch is the second one again (the double buffer's parity)
        x2 = x.copy()
        x2[..., 128:192] = x[..., 64:128]
        region[:] = True
        return "y", ep(acc(x2, w)[0]), region
    if name == "interleave_undone":                # block cb = 1 computes rows 16 .. 31 in natural order but stores at the interleaved channels
        y = ep(v)
        m = y.copy()
        for rr in range(16):
            co = interleaved_channel(1, rr, c["bn"])
            m[..., co] = y[..., 16 + rr]
            region[..., co] = co != 16 + rr
        return "y", m, region
    if name == "dead_element":                     # the median-magnitude element of the last tile is never written (reads back 0)
        y = ep(v)
        sel = np.argwhere(mt == mt.max())
        cand = [(abs(y[tuple(p)][ch]), tuple(p) + (ch,)) for p in sel for ch in range(Cout)]
        cand.sort()
        idx = cand[len(cand) // 2][1]
        m = y.copy()
        m[idx] = 0.0
        region[idx] = True
        return "y", m, region
    if name == "partials_16bit":                   # the running sum rounded to the 16-bit format after every 64-channel chunk
        s = np.zeros_like(v)
        for kc in range(Cin // 64):
            for t in range(9):
                s = s + _tap(xp, w, t, H, W, slice(64 * kc, 64 * kc + 64))
            s = store(s, kind if kind != "fp32" else "bf16")
        region[:] = True
        return "y", ep(s), region
    k = k_conv(Cin)
    rows, _ = stats_rows(v, A, k, th, tw)
    rreg = np.zeros(rows.shape, dtype=bool)
    if name == "stats_from_rounded":
        rreg[:] = True
        return "rows", stats_rows(store(v, kind), A, k, th, tw)[0], rreg
    if name == "stats_row_neighbour":              # the last two tiles write each other's slot (their sum over the tiles is unchanged)
        m = rows.copy()
        m[-2], m[-1] = rows[-1], rows[-2]
        rreg[-2:] = True
        return "rows", m, rreg
    if name == "addend_stride":                    # addend[m][c] read at m * y_cs + c
        flat = f64(c["addend"]).reshape(-1)
        M = B * H * W
        idx = (np.arange(M)[:, None] * c["y_cs"] + np.arange(Cout)[None]) % flat.size
        region[1:] = True
        region[0, 0, 1:] = True
        region[0, 1:] = True
        return "y", epilogue(v, A, c.get("bias"), flat[idx].reshape(B, H, W, Cout), c.get("act", 0))[0], region
    raise KeyError(name)


def frobenius(a, b):
    return float(np.linalg.norm(f64(a) - f64(b)) / max(np.linalg.norm(f64(b)), 1e-30))


# ------------------------------------------------------------------------------------------------ seeded operands
def operands(seed, B, H, W, Cin, rows, kind, nonneg=False, x_cs=None):
    """x [B][H][W][x_cs] (pad channels poisoned) at scale 1, w [rows][9][Cin] at 1 / sqrt(9 Cin) -- every row random, the rows behind Cout
    too: a partial channel tile multiplies them and must not store them --, both as stored in `kind`; nonneg: |.| of both (no cancellation:
    A == |y|)"""
    r = np.random.default_rng(seed)
    x_cs = x_cs or Cin
    xv, wv = r.standard_normal((B, H, W, Cin)), r.standard_normal((rows, 9, Cin)) / np.sqrt(9.0 * Cin)
    if nonneg:
        xv, wv = np.abs(xv), np.abs(wv)
    x = np.full((B, H, W, x_cs), POISON[kind])
    x[..., :Cin] = xv
    return store(x, kind), store(wv, kind)


def padded(seed, B, H, W, C, cs, kind, std=1.0, nonneg=False):
    """an addend-like tensor [B][H][W][cs] as stored in `kind`, channels >= C poisoned"""
    v = np.random.default_rng(seed).standard_normal((B, H, W, C)) * std
    a = np.full((B, H, W, cs), POISON[kind])
    a[..., :C] = np.abs(v) if nonneg else v
    return store(a, kind)


def bias_of(seed, C, nonneg=False):
    v = np.random.default_rng(seed).standard_normal(C).astype(np.float32)
    return np.abs(v) if nonneg else v


def pow2_vectors(seed, C):
    """fp32 per-channel vectors whose products with 16-bit values and sums stay exact in fp32: scale in {+-0.5, +-1, +-2}, shift a multiple of
    1/4 in [-1, 1] -> the sign of x scale + shift is decided exactly (no marginal element in the mask)"""
    r = np.random.default_rng(seed)
    pw = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], dtype=np.float32)
    return pw[r.integers(0, 6, C)], (r.integers(-4, 5, C) / 4.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the case tables (shared by the CPU and the GPU module)
def rows_of(Cout, bn):
    return -(-Cout // bn) * bn


def expected_tile(kern, W, Cout):
    """(th, tw, bn) the library must report for a case (the GPU module asserts gdrn_conv3x3_tile / gdrn_v3_tile agree)"""
    if kern == "v3_256":
        return 16, 16, 256
    if kern == "v3_128":
        return 8, 16, 128
    if kern == "f32":
        return 8, 8, 64
    return 8, (16 if W % 16 == 0 else 8), (64 if Cout <= 64 else 128)


EPI = {  # name: (bias, addend, act, out_f32, stats)
    "none": (0, 0, 0, 0, 0), "bias": (1, 0, 0, 0, 0), "addend": (0, 1, 0, 0, 0), "all_relu": (1, 1, 1, 0, 0), "stats": (0, 0, 0, 0, 1),
    "leaky": (1, 1, 2, 0, 0), "f32out": (1, 0, 0, 1, 1), "f32probe": (0, 0, 0, 1, 0),
}
FAST_EPI = ("none", "bias", "addend", "all_relu", "stats")
LONG_EPI = FAST_EPI + ("leaky", "f32out")


def _case(kern, waves, B, H, W, Cin, Cout, epi, pads=(0, 0, 0), nonneg=False, props=()):
    th, tw, bn = expected_tile(kern, W, Cout)
    return dict(kern=kern, waves=waves, B=B, H=H, W=W, Cin=Cin, Cout=Cout, epi=epi, pads=pads, nonneg=nonneg, props=frozenset(props),
                th=th, tw=tw, bn=bn, id=f"{kern}{waves or ''}-{B}x{H}x{W}-{Cin}to{Cout}-{epi}" + ("-pad" if any(pads) else "") + ("-nn" if nonneg else ""))


def case_props(c):
    """the properties a case really has (the CPU module checks the claimed ones against these)"""
    grid = grid_size(c["B"], c["H"], c["W"], c["Cout"], c["th"], c["tw"], c["bn"])
    esz = 4 if c["kern"] == "f32" else 2
    p = set()
    if grid % 8:
        p.add("xcd_remainder")
    if grid < 8:
        p.add("grid_below_8")
    if (c["Cin"] * esz // 128) % 2:
        p.add("odd_chunks")
    if c["Cout"] % c["bn"]:
        p.add("partial_tile")
    if c["H"] != c["W"]:
        p.add("non_square")
    if c["H"] // c["th"] >= 3 and c["W"] // c["tw"] >= 3:
        p.add("interior_tile")
    return p


MAPS8 = [(1, 8, 8), (3, 8, 24), (1, 24, 8), (3, 16, 24), (1, 24, 24)]      # 8-wide tiles (W % 16 != 0); 24 x 24: an interior tile
MAPS16 = [(1, 8, 16), (3, 8, 32), (1, 24, 48), (3, 8, 16), (3, 24, 48)]    # 16-wide tiles
CINS = [64, 128, 192, 512]


def _family(kern, waves, tw, bn):
    """the cases of one tile: the straight-line epilogue (full channel tiles) with its five forms, the long epilogue (a partial channel tile,
    act 2 or fp32 output) with its seven, over the maps, the input channel counts and the output channel counts of the tile"""
    maps = MAPS8 if tw == 8 else MAPS16
    full, part = ([64], [40, 24]) if bn == 64 else ([128, 256], [72, 192])
    out = []
    fast = () if kern == "f32" else FAST_EPI     # (the fp32 instantiation has the long epilogue only)
    for i, e in enumerate(fast):
        B, H, W = maps[i % len(maps)]
        out.append(_case(kern, waves, B, H, W, CINS[i % 4], full[i % len(full)], e, pads=(64, 8, 16) if i % 2 else (0, 0, 0)))
    for i, e in enumerate(LONG_EPI):
        B, H, W = maps[(i + 2) % len(maps)]
        Cout = full[i % len(full)] if e in ("leaky", "f32out") and i % 2 else part[i % len(part)]
        Cin = CINS[(i + 1) % 4] if B * H * W <= 1200 else CINS[(i + 1) % 2]
        out.append(_case(kern, waves, B, H, W, Cin, Cout, e, pads=(0, 0, 0) if i % 2 else (64, 8, 16)))
    return out


FWD_CASES = (_family("halo", 0, 8, 64) + _family("halo", 0, 16, 64) + _family("halo", 4, 8, 128) + _family("halo", 8, 8, 128)
             + _family("halo", 4, 16, 128) + _family("halo", 8, 16, 128) + _family("f32", 0, 8, 64))
# the library's own pick on these small grids is the eight-wave form (<= 256 workgroups)
FWD_CASES.append(_case("halo", 0, 3, 8, 24, 128, 128, "all_relu"))
# the second-generation kernel: 16x16x256 (no addend: its lean epilogue) on 16 x 16 and 32 x 16 maps, 8x16x128 on the 16-wide maps
V3_CASES = [_case("v3_256", 0, 1, 16, 16, 64, 256, "none"), _case("v3_256", 0, 3, 32, 16, 128, 256, "bias", pads=(64, 8, 0)),
            _case("v3_256", 0, 3, 16, 16, 192, 256, "stats"), _case("v3_256", 0, 1, 32, 16, 512, 256, "stats", pads=(64, 8, 0)),
            _case("v3_128", 0, 1, 8, 16, 64, 128, "none"), _case("v3_128", 0, 3, 8, 32, 128, 128, "bias", pads=(64, 8, 16)),
            _case("v3_128", 0, 1, 24, 48, 192, 128, "addend", pads=(64, 8, 16)), _case("v3_128", 0, 3, 24, 48, 128, 256, "all_relu"),
            _case("v3_128", 0, 3, 8, 16, 512, 128, "stats")]
# the precision probe: fp32 output of non-negative operands (A == |y|, no store term: nothing hides a lossy meeting of partial sums) on the
# four-wave form, the eight-wave form and the fp32 instantiation
PROBE_CASES = [_case("halo", 4, 3, 8, 24, 512, 128, "f32probe", nonneg=True), _case("halo", 8, 3, 8, 24, 512, 128, "f32probe", nonneg=True),
               _case("halo", 8, 1, 8, 16, 192, 128, "f32probe", nonneg=True), _case("halo", 0, 1, 24, 24, 192, 64, "f32probe", nonneg=True),
               _case("f32", 0, 3, 8, 24, 96, 64, "f32probe", nonneg=True), _case("f32", 0, 1, 16, 24, 512, 40, "f32probe", nonneg=True)]
ALL_CASES = FWD_CASES + V3_CASES + PROBE_CASES

# properties the GPU module relies on: (property, ids of cases that claim it) -- filled from the tables, checked by the CPU module
CLAIMS = {
    "xcd_remainder": [c["id"] for c in ALL_CASES if (c["B"], c["H"], c["W"]) in ((3, 8, 24), (1, 24, 8), (1, 24, 24), (3, 8, 16)) and c["Cout"] <= c["bn"]],
    "grid_below_8": [c["id"] for c in ALL_CASES if c["B"] == 1 and c["H"] == 8 and c["Cout"] <= 2 * c["bn"]],
    "odd_chunks": [c["id"] for c in ALL_CASES if c["kern"] != "f32" and c["Cin"] in (64, 192)],
    "partial_tile": [c["id"] for c in ALL_CASES if c["Cout"] in (24, 40, 72, 192) and c["kern"] in ("halo", "f32")],
    "non_square": [c["id"] for c in ALL_CASES if c["H"] != c["W"]],
    "interior_tile": [c["id"] for c in ALL_CASES if (c["H"], c["W"]) in ((24, 24), (24, 48)) and c["kern"] != "v3_256"],
}
BY_ID = {c["id"]: c for c in ALL_CASES}


def seed_of(c):
    return 4000 + 7 * c["B"] + 11 * c["H"] + 13 * c["W"] + c["Cin"] + 3 * c["Cout"] + 17 * len(c["epi"]) + c["waves"]


def kind_of(c, half="bf16"):
    return "fp32" if c["kern"] == "f32" else half


class Fwd:
    """one forward case with its operands and fp64 reference, computed once per (case, 16-bit format)"""

    def __init__(self, c, half="bf16"):
        self.c, self.kind = c, kind_of(c, half)
        B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
        bias, addend, act, out_f32, stats = EPI[c["epi"]]
        xp, yp, ap = c["pads"]
        self.x_cs, self.y_cs, self.add_cs = Cin + xp, -(-Cout // 8) * 8 + yp, -(-Cout // 8) * 8 + ap
        self.rows = rows_of(Cout, c["bn"])
        sd = seed_of(c)
        self.x, self.w = operands(sd, B, H, W, Cin, self.rows, self.kind, c["nonneg"], self.x_cs)
        self.bias = bias_of(sd + 1, Cout, c["nonneg"]) if bias else None
        self.addend = padded(sd + 2, B, H, W, Cout, self.add_cs, self.kind, nonneg=c["nonneg"]) if addend else None
        self.act, self.out_f32, self.want_stats = act, out_f32, stats
        self.out_kind = "fp32" if (out_f32 or self.kind == "fp32") else self.kind
        self.fp32 = self.kind == "fp32"
        self.v, self.Aacc = acc(self.x[..., :Cin], self.w, Cout)
        self.y, self.A = epilogue(self.v, self.Aacc, self.bias, self.addend, act)
        self.k = k_conv(Cin, act, self.fp32)
        self.bound = bound(self.y, self.A, self.k, self.out_kind)
        if stats:
            self.rows_ref, self.rows_bound = stats_rows(self.v, self.Aacc, self.k, c["th"], c["tw"])

    def mutation_input(self):
        c = self.c
        return dict(x=self.x[..., :c["Cin"]], w=self.w, Cout=c["Cout"], bias=self.bias, addend=self.addend, add_cs=self.add_cs, y_cs=self.y_cs,
                    act=self.act, kind=self.kind, th=c["th"], tw=c["tw"], bn=c["bn"])


_FWD = {}


def fwd(c, half="bf16"):
    key = (c["id"], half)
    if key not in _FWD:
        _FWD[key] = Fwd(c, half)
    return _FWD[key]


# statistics of non-negative operands at Cin = 64: the rows' bounds have no cancellation slack and the smallest k -- where rows taken from the
# ROUNDED outputs leave them (mutation stats_from_rounded)
STATS_PROBES = [_case("halo", 0, 1, 24, 24, 64, 64, "stats", nonneg=True), _case("halo", 8, 3, 8, 16, 64, 128, "stats", nonneg=True),
                _case("halo", 4, 3, 8, 24, 64, 128, "stats", nonneg=True), _case("v3_128", 0, 3, 8, 16, 64, 128, "stats", nonneg=True),
                _case("v3_256", 0, 1, 16, 16, 64, 256, "stats", nonneg=True)]
ALL_CASES = ALL_CASES + STATS_PROBES
BY_ID.update({c["id"]: c for c in STATS_PROBES})

# data gradients with Cin != Cout, both ways (forward channels Cf_in -> Cf_out; the launch reads Cf_out channels and writes Cf_in)
DGRAD_CASES = [("halo", 0, 3, 8, 24, 64, 128), ("halo", 0, 1, 24, 48, 64, 128), ("halo", 4, 3, 8, 24, 128, 64), ("halo", 8, 1, 8, 32, 128, 64),
               ("f32", 0, 1, 16, 24, 64, 128), ("v3_128", 0, 3, 8, 16, 128, 64)]


def dgrad_case(kern, waves, B, H, W, Cf_in, Cf_out, half="bf16"):
    """dict(dy [B][H][W][Cf_out], wf forward weights [Cf_out][9][Cf_in], dx, A, bound) -- all as stored in the case's format"""
    kind = "fp32" if kern == "f32" else half
    r = np.random.default_rng(5000 + Cf_in + 3 * Cf_out + W)
    dy = store(r.standard_normal((B, H, W, Cf_out)), kind)
    wf = store(r.standard_normal((Cf_out, 9, Cf_in)) / np.sqrt(9.0 * Cf_in), kind)
    dx, A, bnd = dgrad(dy, wf, kind=kind, fp32=kern == "f32")
    return dict(dy=dy, wf=wf, dx=dx, A=A, bound=bnd, kind=kind)


# the fused BatchNorm-backward epilogue: (kern, waves, B, H, W, Cin, Cout, mask kind, addend)
BNB_CASES = ([("halo", 0, 3, 8, 24, 128, 64, m, m != "none") for m in ("stored", "affine", "none")]
             + [("halo", 4, 1, 16, 24, 64, 128, m, m == "stored") for m in ("stored", "affine", "none")]
             + [("halo", 8, 3, 8, 16, 192, 128, m, m != "stored") for m in ("stored", "affine", "none")]
             + [("v3_128", 0, 1, 24, 48, 64, 128, m, True) for m in ("stored", "affine", "none")]
             + [("v3_256", 0, 3, 16, 16, 128, 256, m, False) for m in ("affine", "none")])


def bnb_case(kern, waves, B, H, W, Cin, Cout, mask_kind, with_add, half="bf16"):
    th, tw, bn = expected_tile(kern, W, Cout)
    sd = 6000 + Cin + 3 * Cout + W + len(mask_kind)
    r = np.random.default_rng(sd)
    x, w = operands(sd, B, H, W, Cin, rows_of(Cout, bn), half)
    cs = Cout + 8                                                         # bnb_cs = add_cs > Cout: pad channels poisoned
    bx = padded(sd + 1, B, H, W, Cout, cs, half, std=1.5)
    mask = padded(sd + 2, B, H, W, Cout, cs, half) if mask_kind == "stored" else None
    if mask is not None:
        mask[..., :Cout] = np.maximum(mask[..., :Cout], 0.0)              # a stored ReLU output: half of it exactly 0
    addend = padded(sd + 3, B, H, W, Cout, cs, half) if with_add else None
    mean, invstd = (0.2 * r.standard_normal(Cout)).astype(np.float32), (0.5 + r.random(Cout)).astype(np.float32)
    scale, shift = pow2_vectors(sd + 4, Cout) if mask_kind == "affine" else (None, None)
    v, A = acc(x, w, Cout)
    ref = bnb(v, A, k_conv(Cin), th, tw, half, addend, bx, mean, invstd, mask, scale, shift)
    return dict(x=x, w=w, bx=bx, mask=mask, addend=addend, mean=mean, invstd=invstd, scale=scale, shift=shift, cs=cs, th=th, tw=tw, bn=bn, ref=ref)


# operand transforms: (kern, waves, B, H, W, Cin, Cout, mode, relu, vectors given, x pad channels)
XF_CASES = []
for _mode in (1, 2, 3, 4):
    for _relu in (0, 1):
        for _cin in (64, 128):
            for _given in (0, 1):
                _i = len(XF_CASES) // 2
                XF_CASES.append(("halo", 4 if (_relu and _cin == 128) else 0, 3, 8, 24, _cin, 64 if _cin == 64 else 128, _mode, _relu, _given, 64 * (_i % 2)))
                XF_CASES.append(("v3_256", 0, (1, 3)[_i % 2], (16, 32)[_i % 2], 16, _cin, 256, _mode, _relu, _given, 64 * ((_i + 1) % 2)))


def xf_case(kern, waves, B, H, W, Cin, Cout, mode, relu, given, xpad, half="bf16"):
    """operands of one transform case; c != 0 everywhere (v(0) != 0: a transformed halo shows), mode 4's mask vectors exact (pow2_vectors)"""
    th, tw, bn = expected_tile(kern, W, Cout)
    sd = 7000 + 10 * mode + relu + Cin + W
    r = np.random.default_rng(sd)
    x, w = operands(sd, B, H, W, Cin, rows_of(Cout, bn), half, x_cs=Cin + xpad)
    x2 = padded(sd + 1, B, H, W, Cin, Cin + xpad, half)
    f = lambda a: np.asarray(a, dtype=np.float32)
    c = f(np.where(r.random(Cin) < 0.5, -1.0, 1.0) * (0.25 + 0.5 * r.random(Cin)))
    d = dict(x=x, x2=x2 if mode >= 2 else None, w=w, c=c, a=f(0.5 + r.random(Cin)) if given else None,
             b=f(0.7 * r.standard_normal(Cin)) if (given and mode >= 2) else None, c2=f(0.2 * r.standard_normal(Cin)) if (given and mode == 2) else None,
             msc=None, msh=None, th=th, tw=tw, bn=bn)
    if mode == 4:
        d["msc"], d["msh"] = pow2_vectors(sd + 2, Cin)
    d["v"], d["Av"], d["vbound"] = xf_ref(mode, relu, x[..., :Cin], None if d["x2"] is None else d["x2"][..., :Cin], d["a"], d["b"], c, d["c2"],
                                          d["msc"], d["msh"], half)
    return d


BLOCK_CASES = [(1, 8, 16), (3, 8, 16), (1, 24, 48), (3, 24, 48)]


def block_case(B, H, W, half="bf16"):
    r = np.random.default_rng(8000 + B + H + W)
    x = store(np.maximum(r.standard_normal((B, H, W, 64)), 0.0), half)                 # a post-ReLU activation
    w1, w2 = (store(r.standard_normal((64, 9, 64)) / 24.0, half) for _ in range(2))
    b1, b2 = (0.3 * r.standard_normal(64)).astype(np.float32), (0.3 * r.standard_normal(64)).astype(np.float32)
    y, A, bnd, a1, share = block64(x, w1, b1, w2, b2, half)
    return dict(x=x, w1=w1, w2=w2, b1=b1, b2=b2, y=y, A=A, bound=bnd, a1=a1, flippable=share)
