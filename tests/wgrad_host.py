"""Independent yardstick of the weight-gradient kernels (csrc/conv3x3_wgrad.hip: conv3x3_wgrad_kernel, conv3x3_wgrad_multi_kernel,
wgrad_reduce_multi_kernel; csrc/conv_wgrad.hip: the generic kernel): plain fp64 numpy on the NHWC operands as stored, no device code and
nothing from the library.  tests/test_wgrad_host_cpu.py pins this module against fp64 autograd and shows that every mutated reference of
mutate() leaves its bound; tests/test_wgrad_edges_gpu.py (and its fp16 twin) hold the kernels to it.

Operands: x [B][Hi][Wi][x_cs], dy [B][Ho][Wo][dy_cs].  Result: the packed gradient dw[co][tap][ci], tap = KW ky + kx,

    dw[co][tap][ci] = sum over output pixels (n, oy, ox) of dy[n][oy][ox][co] * x[n][oy stride - pad + ky][ox stride - pad + kx][ci]

(out-of-image terms are zero), and A[co][tap][ci], the same sum on absolute values.  x_cs < Cin is the WINDOW form the generic kernel is
given for the stem fallback (KH = 7, KW = 1, x_cs = 4, Cin = 64): "channel" c of pixel (iy, ix) is element c of the flat row that starts
at that pixel.

Layouts restated here: the workspace slab ws[split][ci tile][co tile][36][4][64][4] of the halo kernel (slab_order(): the comment above the
store in wgrad_tile, the reader in wgrad_reduce_multi_kernel), the pixel patches and their split ranges (patch_of(), split_ranges():
patch = 8 x 8 output pixels for stride 1, 4 x 8 for stride 2, ordered image, tile row, tile column; slab s = patches
[s per, min(npatch, (s + 1) per)), per = ceil(npatch / nsplit)), and the reduction's scatter dst[co s_co + ci s_ci + t s_t] with cin_valid
(reduce_ref()).

The bound of an element:   |got - ref| <= k 2^-23 A + 2^-149.
The unit is a WHOLE ulp of fp32 (round-to-nearest costs half of one), so the bound holds however the matrix unit orders and rounds its
internal adds.  k counts the fp32 roundings on the element's path, read off the kernels:
  * 16-bit operands: the product of two 8- or 11-bit significands is exact in fp32; every one of the M pixel terms is accumulated once
    (M roundings, wherever the split boundaries fall); the nsplit partial tiles meet in nsplit adds -- wgrad_reduce_multi_kernel's four
    running sums and their three-add meeting are a tree no deeper than that, the atomics path adds one partial per split --; one more for
    the value already in dw, whose magnitude joins A; one spare:  k = M + nsplit + 2.
  * the fp32 instantiation of the generic kernel multiplies fp32 operands: + M product roundings.
  * a raw workspace slab: k = the pixels of that split.
No constant here comes from a device result.

DETECTABILITY.  The bound grows like M^2 (k ~ M, A ~ M), a single term |x| |dy| does not: every random-operand case keeps
max bound <= 1/2 median|x| median|dy| (detectable(); M <= 1152), so that one dropped or doubled pixel term leaves the bound.  What needs more
pixels (more than 8 splits, the generic kernel's automatic split) uses EXACT operands: integers in {-2 .. 2}, every partial sum an integer
below 2^24, the result the same bits in any summation order, atomics included; those are compared bit for bit."""
import numpy as np

import norm_host as NH

ULP32 = 2.0 ** -23
TINY = 2.0 ** -149
POISON = {"fp32": 1e30, "bf16": 1e30, "fp16": 6e4}    # operand pad channels no kernel may read
OLD_TOL = 1e-2                                         # the Frobenius tolerance of the weight-gradient tests of tests/test_kernels_gpu.py

f64 = NH.f64
store = NH.store


def k_wgrad(M, nsplit, fp32=False):
    return M + nsplit + 2 + (M if fp32 else 0)


def bound(A, k):
    return k * ULP32 * f64(A) + TINY


def frobenius(a, b):
    return float(np.linalg.norm(f64(a) - f64(b)) / max(np.linalg.norm(f64(b)), 1e-30))


# ------------------------------------------------------------------------------------------------ the gradient
def out_size(Hi, K, stride, pad):
    return (Hi + 2 * pad - K) // stride + 1


def gather(x, Cin, Ho, Wo, KH, KW, stride, pad, tap):
    """the x operand of one tap: [B Ho Wo][Cin], zero where the tap leaves the image.  x [B][Hi][Wi][x_cs]; x_cs >= Cin: the first Cin
    channels of the pixel; x_cs < Cin: the window of Cin elements that starts at the pixel (inside the buffer, or this raises)"""
    x = f64(x)
    B, Hi, Wi, x_cs = x.shape
    ky, kx = divmod(tap, KW)
    n, oy, ox = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing="ij")
    iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
    ok = ((iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)).reshape(-1)
    base = (((n * Hi + iy) * Wi + ix) * x_cs).reshape(-1)
    idx = np.where(ok, base, 0)[:, None] + np.arange(Cin)[None]
    assert idx.max() < x.size, "a window leaves the buffer"
    return np.where(ok[:, None], x.reshape(-1)[idx], 0.0)


def gathered(x, Cin, Ho, Wo, KH, KW, stride, pad):
    return np.stack([gather(x, Cin, Ho, Wo, KH, KW, stride, pad, t) for t in range(KH * KW)])


def from_gathered(X, dyv, rows=slice(None)):
    """(dw, A) [Cout][taps][Cin] of the pixel rows `rows` from X [taps][M][Cin], dyv [M][Cout]"""
    d, Xr = dyv[rows], X[:, rows]
    dw = np.einsum("mo,tmi->oti", d, Xr, optimize=True)
    A = np.einsum("mo,tmi->oti", np.abs(d), np.abs(Xr), optimize=True)
    return dw, A


def wgrad(x, dy, Cin, Cout, KH, KW, stride, pad):
    """(dw, A) in fp64, [Cout][KH KW][Cin]"""
    dy = f64(dy)
    _, Ho, Wo, _ = dy.shape
    return from_gathered(gathered(x, Cin, Ho, Wo, KH, KW, stride, pad), dy[..., :Cout].reshape(-1, Cout))


# ------------------------------------------------------------------------------------------------ the halo kernel's patches, splits and slabs
def patch_rows(stride):
    return 4 if stride == 2 else 8


def n_patches(B, Ho, Wo, stride):
    return B * (Ho // patch_rows(stride)) * (Wo // 8)


def patch_of(B, Ho, Wo, stride):
    """the pixel patch of every output pixel, [B][Ho][Wo]: image, then tile row, then tile column"""
    th = patch_rows(stride)
    n, y, x = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing="ij")
    return (n * (Ho // th) + y // th) * (Wo // 8) + x // 8


def n_splits(npatch, tiles, request, ws):
    """gdrn_conv3x3_wgrad_splits: the automatic choice (request <= 0), the clamp to npatch and the normalisation that leaves no split empty"""
    s = request
    if s <= 0:
        s = max(1, min(max(npatch // 4, 1), -(-(512 if ws else 256) // tiles)))
    s = min(s, npatch)
    per = -(-npatch // s)
    return -(-npatch // per)


def split_ranges(npatch, nsplit):
    per = -(-npatch // nsplit)
    return [(s * per, min(npatch, (s + 1) * per)) for s in range(nsplit)]


def slab_order(Cout, Cin):
    """index arrays (co, t, ci), each [ci tiles][co tiles][36][4][64][4]: the element of dw[co][t][ci] a workspace slot holds.
    Slot (f, w, lane, j) of tile (cit, cot): f = (t * 2 + a') * 2 + b', w = wa' * 2 + wb', lane = g * 16 + q holds
    co = cot 64 + wa' 32 + a' 16 + g 4 + j and ci = cit 64 + wb' 32 + b' 16 + q (the 16 x 16 accumulator fragment D[g 4 + j][q])"""
    ncot, ncit = Cout // 64, Cin // 64
    cit, cot, f, w, lane, j = np.meshgrid(np.arange(ncit), np.arange(ncot), np.arange(36), np.arange(4), np.arange(64), np.arange(4), indexing="ij")
    t, a_, b_ = f >> 2, (f >> 1) & 1, f & 1
    wa_, wb_ = w >> 1, w & 1
    g, q = lane >> 4, lane & 15
    return cot * 64 + wa_ * 32 + a_ * 16 + g * 4 + j, t, cit * 64 + wb_ * 32 + b_ * 16 + q


def to_slab(dw):
    """dw [Cout][9][Cin] -> one workspace slab, flat [Cout Cin 9]"""
    co, t, ci = slab_order(dw.shape[0], dw.shape[2])
    return dw[co, t, ci].reshape(-1)


def from_slab(flat, Cout, Cin):
    co, t, ci = slab_order(Cout, Cin)
    dw = np.full((Cout, 9, Cin), np.nan)
    dw[co.reshape(-1), t.reshape(-1), ci.reshape(-1)] = np.asarray(flat, dtype=np.float64).reshape(-1)
    return dw


def reduce_ref(slabs, cin_valid, s_co, s_ci, s_t, size):
    """gdrn_wgrad_reduce_multi on one task: slabs [nsplit][Cout][9][Cin] (as gradients, not in slab order) ->
    (dst [size] with NaN where nothing is written, the written mask).  cin_valid = 0: every input channel has a slot"""
    s = f64(slabs).sum(0)
    Cout, _, Cin = s.shape
    civ = cin_valid if cin_valid > 0 else Cin
    co, t, ci = np.meshgrid(np.arange(Cout), np.arange(9), np.arange(Cin), indexing="ij")
    keep = ci < civ
    idx = (co * s_co + ci * s_ci + t * s_t)[keep]
    assert len(np.unique(idx)) == idx.size and idx.max() < size and idx.min() >= 0, "the scatter is no injection into dst"
    dst = np.full(size, np.nan)
    dst[idx] = s[keep]
    return dst, ~np.isnan(dst)


# ------------------------------------------------------------------------------------------------ seeded operands
def operands(seed, B, Hi, Wi, Ho, Wo, Cin, Cout, x_cs, dy_cs, kind, exact=False):
    """x [B][Hi][Wi][x_cs], dy [B][Ho][Wo][dy_cs] as stored in `kind`; N(0, 1), or (exact) integers in {-2 .. 2}.  Pad channels
    (x_cs > Cin, dy_cs > Cout) hold POISON; in the window form (x_cs < Cin) every element is an operand"""
    r = np.random.default_rng(seed)
    draw = (lambda shp: r.integers(-2, 3, shp).astype(np.float64)) if exact else r.standard_normal
    x = np.full((B, Hi, Wi, x_cs), POISON[kind])
    x[..., :min(Cin, x_cs)] = draw((B, Hi, Wi, min(Cin, x_cs)))
    dy = np.full((B, Ho, Wo, dy_cs), POISON[kind])
    dy[..., :Cout] = draw((B, Ho, Wo, Cout))
    return store(x, kind), store(dy, kind)


def prefill(seed, shape, exact=False):
    """the fp32 values already in dw when the atomics path adds to it"""
    r = np.random.default_rng(seed)
    v = r.integers(-64, 65, shape).astype(np.float64) if exact else 3.0 * r.standard_normal(shape)
    return store(v, "fp32")


def detectable(bnd, x, dy):
    """(max bound, half the median single term): the condition of the module docstring"""
    return float(np.max(bnd)), 0.5 * float(np.median(np.abs(x))) * float(np.median(np.abs(dy)))


# ------------------------------------------------------------------------------------------------ the halo cases
HALO_CH = [(64, 64), (128, 64), (64, 192), (192, 128)]                   # Cin x Cout
S1_MAPS = [(8, 8), (8, 24), (24, 8), (16, 24)]
S2_MAPS = [(4, 8), (4, 24), (12, 8), (8, 16)]                             # output maps; the inputs are twice that


def _halo(stride, B, Ho, Wo, Cin, Cout, pads=False, exact=False):
    return dict(stride=stride, B=B, Ho=Ho, Wo=Wo, Hi=stride * Ho, Wi=stride * Wo, Cin=Cin, Cout=Cout, pads=pads, exact=exact,
                npatch=n_patches(B, Ho, Wo, stride), tiles=(Cin // 64) * (Cout // 64), M=B * Ho * Wo,
                id=f"s{stride}-{B}x{Ho}x{Wo}-{Cin}to{Cout}" + ("-pad" if pads else "") + ("-exact" if exact else ""))


HALO_CASES = []
for _s, _maps in ((1, S1_MAPS), (2, S2_MAPS)):
    for _b in (1, 3):
        for _mi, (_h, _w) in enumerate(_maps):
            _i = len(HALO_CASES)
            _cin, _cout = HALO_CH[(_i + _i // 4) % 4]
            HALO_CASES.append(_halo(_s, _b, _h, _w, _cin, _cout, pads=bool(_i % 2)))
# 72 patches: the automatic choice is 18 splits (more than 8), the grid 18 workgroups (remainder 2 in the XCD remap)
HALO_EXACT = [_halo(1, 8, 24, 24, 64, 64, exact=True), _halo(2, 8, 12, 24, 128, 64, pads=True, exact=True)]
HALO_BY_ID = {c["id"]: c for c in HALO_CASES + HALO_EXACT}


def split_requests(npatch):
    out = []
    for s in (0, 1, 2, 3, npatch - 1, npatch, npatch + 5):
        if s >= 0 and s not in out:
            out.append(s)
    return out


class Halo:
    """operands and fp64 partial gradients per pixel patch of one halo case, computed once per (case, 16-bit format)"""

    def __init__(self, c, kind):
        self.c, self.kind = c, kind
        B, Ho, Wo, Hi, Wi, Cin, Cout, stride = (c[k] for k in ("B", "Ho", "Wo", "Hi", "Wi", "Cin", "Cout", "stride"))
        self.x_cs, self.dy_cs = Cin + (64 if c["pads"] else 0), Cout + (64 if c["pads"] else 0)
        sd = 9000 + 131 * stride + 17 * B + 3 * Ho + 5 * Wo + Cin + 7 * Cout
        self.x, self.dy = operands(sd, B, Hi, Wi, Ho, Wo, Cin, Cout, self.x_cs, self.dy_cs, kind, c["exact"])
        self.dw0 = prefill(sd + 1, (Cout, 9, Cin), c["exact"])
        X = gathered(self.x, Cin, Ho, Wo, 3, 3, stride, 1)
        dyv = self.dy[..., :Cout].reshape(-1, Cout)
        pid = patch_of(B, Ho, Wo, stride).reshape(-1)
        parts = [from_gathered(X, dyv, np.flatnonzero(pid == p)) for p in range(c["npatch"])]
        self.P, self.PA = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        self.dw, self.A = self.P.sum(0), self.PA.sum(0)

    def slabs(self, nsplit):
        """([nsplit][Cout][9][Cin] partial gradients, the same on absolute values, pixels per split)"""
        rng = split_ranges(self.c["npatch"], nsplit)
        ppx = 8 * patch_rows(self.c["stride"])
        return (np.stack([self.P[a:b].sum(0) for a, b in rng]), np.stack([self.PA[a:b].sum(0) for a, b in rng]), [(b - a) * ppx for a, b in rng])

    def bound(self, nsplit, with_dw0=False):
        return bound(self.A + (np.abs(self.dw0) if with_dw0 else 0.0), k_wgrad(self.c["M"], nsplit))


_HALO = {}


def halo(c, kind="bf16"):
    key = (c["id"], kind)
    if key not in _HALO:
        _HALO[key] = Halo(c, kind)
    return _HALO[key]


# ------------------------------------------------------------------------------------------------ grouped launches
# (case, requested splits): tables of 1, 2 and 5 tasks mixing strides, non-square maps, tile counts; the requests 7 and 4 are normalised
# (18 patches / 7 -> 6 splits, 9 / 4 -> 3); total workgroups 15, 9 and 56: remainders 7, 1 and 0 in the XCD remap
_TA, _TB, _TC = _halo(1, 1, 8, 24, 64, 64), _halo(2, 3, 4, 24, 128, 64, pads=True), _halo(1, 3, 16, 24, 64, 192)
_TD, _TE = _halo(2, 1, 12, 8, 192, 128), _halo(1, 1, 24, 8, 64, 64, pads=True)
GROUPED = {"one": [(_TC, 5)], "two": [(_TB, 4), (_TA, 3)], "five": [(_TC, 7), (_TD, 3), (_TB, 9), (_TA, 1), (_TE, 1)]}
HALO_BY_ID.update({c["id"]: c for c in (_TA, _TB, _TC, _TD, _TE)})


def grouped_blocks(table):
    """(splits per task, blk_start) as the header defines them"""
    ns = [n_splits(c["npatch"], c["tiles"], req, True) for c, req in table]
    starts = [0]
    for (c, _), n in zip(table, ns):
        starts.append(starts[-1] + c["tiles"] * n)
    return ns, starts


# ------------------------------------------------------------------------------------------------ the generic kernel's cases
def _gen(name, B, Hi, Wi, KH, KW, stride, pad, Cin, Cout, dy_cs, splits, x_cs=None, Ho=None, Wo=None, fp32=False, exact=False):
    Ho = out_size(Hi, KH, stride, pad) if Ho is None else Ho
    Wo = out_size(Wi, KW, stride, pad) if Wo is None else Wo
    return dict(id=name + ("-f32" if fp32 else ""), B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, KH=KH, KW=KW, stride=stride, pad=pad, Cin=Cin, Cout=Cout,
                x_cs=x_cs or Cin, dy_cs=dy_cs, splits=splits, fp32=fp32, exact=exact, M=B * Ho * Wo)


# tile = (64 if Cout <= 64 else 128) x (128 if Cin % 128 == 0 else 64); stage = 64 pixels (16-bit) or 32 (fp32)
_GEN16 = [
    _gen("1x1-M4-64x128", 4, 1, 1, 1, 1, 1, 0, 256, 9, 64, 0),                      # less than one stage; fc_rt's form
    _gen("1x1-M37-128x64", 37, 1, 1, 1, 1, 1, 0, 64, 69, 128, 1, x_cs=128),         # (64 poisoned pad channels behind x)
    _gen("1x1-M64-128x128", 1, 8, 8, 1, 1, 1, 0, 128, 130, 256, 3),                 # one stage, three splits: two of them empty
    _gen("1x1-M65-64x64", 65, 1, 1, 1, 1, 1, 0, 192, 64, 64, 0),                    # a ragged second stage of one pixel
    _gen("3x3-9x9-M81-64x64", 1, 9, 9, 3, 3, 1, 1, 64, 9, 64, 3),                   # no power of two: the division path; split 2 of 3 empty
    _gen("3x3-7x7-M147-128x128", 3, 7, 7, 3, 3, 1, 1, 128, 69, 128, 0),
    _gen("3x3s2-M256-128x64", 4, 16, 16, 3, 3, 2, 1, 64, 130, 256, 3),              # powers of two: the shift path
    _gen("1x1s2p0-M64-64x128", 4, 8, 8, 1, 1, 2, 0, 128, 64, 64, 1),
    _gen("8x8-Ho1-M37-128x128", 37, 8, 8, 8, 8, 1, 0, 128, 130, 256, 0),            # fc1's form: 64 taps, a 1 x 1 output map
    _gen("8x8-Ho1-M4-64x64", 4, 8, 8, 8, 8, 1, 0, 64, 9, 64, 5),                    # five splits of one stage
    _gen("7x1s2-window-M64-64x64", 4, 13, 24, 7, 1, 2, 0, 64, 64, 64, 0, x_cs=4, Wo=4),      # windows of 16 pixels: 2 * 3 + 16 <= 24
    _gen("7x1s2-window-M20-64x64", 1, 13, 26, 7, 1, 2, 0, 64, 9, 64, 2, x_cs=4, Wo=5),
]
_GEN32 = [dict(c, id=c["id"] + "-f32", fp32=True) for c in _GEN16 if c["id"] in (
    "1x1-M4-64x128", "1x1-M37-128x64", "1x1-M64-128x128", "1x1-M65-64x64", "3x3-9x9-M81-64x64", "3x3s2-M256-128x64", "7x1s2-window-M64-64x64")]
# 4608 pixels = 72 stages of 64, 9 tiles: the automatic split is min(72 / 8, ceil(2048 / 9)) = 9 (more than 8); exact operands
GEN_EXACT = [_gen("3x3-48x48-M4608-exact", 2, 48, 48, 3, 3, 1, 1, 64, 64, 64, 0, exact=True)]
GEN_CASES = _GEN16 + _GEN32
GEN_BY_ID = {c["id"]: c for c in GEN_CASES + GEN_EXACT}


def gen_tile(c):
    return (64 if c["Cout"] <= 64 else 128), (128 if c["Cin"] % 128 == 0 else 64)


def gen_splits(c):
    """(workgroup splits the launcher uses, splits that own at least one stage) -- conv_wgrad.hip's launch() and the kernel's split ranges"""
    bco, bci = gen_tile(c)
    nst = -(-c["M"] // (32 if c["fp32"] else 64))
    tiles = -(-c["Cout"] // bco) * (c["Cin"] // bci) * c["KH"] * c["KW"]
    s = c["splits"]
    if s <= 0:
        s = max(1, min(max(nst // 8, 1), -(-2048 // tiles)))
    per = -(-nst // s)
    return s, -(-nst // per)


class Gen:
    def __init__(self, c, half):
        self.c, self.kind = c, ("fp32" if c["fp32"] else half)
        sd = 9500 + 13 * c["M"] + c["Cin"] + 3 * c["Cout"] + 7 * c["KH"] + c["stride"]
        self.x, self.dy = operands(sd, c["B"], c["Hi"], c["Wi"], c["Ho"], c["Wo"], c["Cin"], c["Cout"], c["x_cs"], c["dy_cs"], self.kind, c["exact"])
        KK = c["KH"] * c["KW"]
        self.dw0 = prefill(sd + 1, (c["Cout"], KK, c["Cin"]), c["exact"])
        self.dw, self.A = wgrad(self.x, self.dy, c["Cin"], c["Cout"], c["KH"], c["KW"], c["stride"], c["pad"])
        self.nsplit = gen_splits(c)[1]
        self.ref = self.dw0 + self.dw
        self.bound = bound(self.A + np.abs(self.dw0), k_wgrad(c["M"], self.nsplit, c["fp32"]))


_GEN = {}


def gen(c, half="bf16"):
    key = (c["id"], half)
    if key not in _GEN:
        _GEN[key] = Gen(c, half)
    return _GEN[key]


# ------------------------------------------------------------------------------------------------ mutated references
MUTATIONS = ("corner_term", "top_halo_previous_image", "right_halo_wraps", "hw_swapped", "taps_transposed", "taps_flipped", "stride2_unshifted",
             "last_patch_dropped", "first_patch_twice", "fifth_slab_dropped", "partials_16bit", "blocks_exchanged", "cin_valid_ignored",
             "strides_exchanged", "atomics_overwrite")


def mutate(name, h, nsplit=1):
    """what a kernel with defect `name` would leave for halo case h (a Halo): (got, ref, bound, region), arrays [Cout][9][Cin] (or, for the
    two scatter defects, the flat OIHW destination with NaN = not written).  `region` marks what the defect may move."""
    c = h.c
    B, Ho, Wo, Hi, Wi, Cin, Cout, stride = (c[k] for k in ("B", "Ho", "Wo", "Hi", "Wi", "Cin", "Cout", "stride"))
    x, dy = f64(h.x)[..., :Cin], f64(h.dy)[..., :Cout]
    ref, bnd = h.dw, h.bound(nsplit)
    region = np.zeros(ref.shape, dtype=bool)
    taps = lambda sel: region.__setitem__((slice(None), sel), True)
    if name == "corner_term":                      # the last pixel of the last image misses from the centre tap
        m = ref.copy()
        m[:, 4] -= np.outer(dy[B - 1, Ho - 1, Wo - 1], x[B - 1, stride * (Ho - 1), stride * (Wo - 1)])
        taps(4)
        return m, ref, bnd, region
    if name == "top_halo_previous_image":          # input row -1 read as the previous image's last row (image 0: zero)
        m = ref.copy()
        for kx in range(3):
            for ox in range(Wo):
                ix = ox * stride - 1 + kx
                if 0 <= ix < Wi:
                    m[:, kx] += dy[1:, 0, ox].T @ x[:-1, Hi - 1, ix]
        taps([0, 1, 2])
        return m, ref, bnd, region
    if name == "right_halo_wraps":                 # input column Wi read as the flat pixel behind: the next row's first (the very last: zero)
        assert stride == 1
        flat = np.concatenate([x.reshape(-1, Cin), np.zeros((1, Cin))])
        m = ref.copy()
        for ky in range(3):
            for n in range(B):
                for oy in range(Ho):
                    iy = oy - 1 + ky
                    if 0 <= iy < Hi:
                        m[:, 3 * ky + 2] += np.outer(dy[n, oy, Wo - 1], flat[(n * Hi + iy) * Wi + Wi])
        taps([2, 5, 8])
        return m, ref, bnd, region
    if name == "hw_swapped":                       # the maps walked as [W][H]
        taps([0, 1, 2, 3, 5, 6, 7, 8])             # (the centre tap pairs pixel p with pixel p whatever the map's shape)
        return wgrad(x.reshape(B, Wi, Hi, Cin), dy.reshape(B, Wo, Ho, Cout), Cin, Cout, 3, 3, stride, 1)[0], ref, bnd, region
    if name == "taps_transposed":
        taps([1, 2, 3, 5, 6, 7])
        return ref.reshape(Cout, 3, 3, Cin).transpose(0, 2, 1, 3).reshape(Cout, 9, Cin).copy(), ref, bnd, region
    if name == "taps_flipped":
        taps([0, 1, 2, 3, 5, 6, 7, 8])
        return ref[:, ::-1].copy(), ref, bnd, region
    if name == "stride2_unshifted":                # sampled at 2 y + ky instead of 2 y + ky - 1
        assert stride == 2
        region[:] = True
        return wgrad(x, dy, Cin, Cout, 3, 3, 2, 0)[0], ref, bnd, region
    rng = split_ranges(c["npatch"], nsplit)
    if name == "last_patch_dropped":               # ... of the first split
        region[:] = True
        return ref - h.P[rng[0][1] - 1], ref, bnd, region
    if name == "first_patch_twice":                # the first patch of the second split also counted by the first
        region[:] = True
        return ref + h.P[rng[1][0]], ref, bnd, region
    if name == "fifth_slab_dropped":               # the remainder loop behind the four-way unrolled sum
        assert nsplit == 5
        region[:] = True
        return h.slabs(5)[0][:4].sum(0), ref, bnd, region
    if name == "partials_16bit":                   # every patch's partial sum rounded to the 16-bit format
        region[:] = True
        return store(h.P, h.kind).sum(0), ref, bnd, region
    if name == "blocks_exchanged":                 # 16 x 16 block (co16 = a, ci16 = wave) stored in the slot of (wave, a), in every 64 x 64 tile
        v = ref.reshape(Cout // 64, 4, 16, 9, Cin // 64, 4, 16)
        m = v.transpose(0, 5, 2, 3, 4, 1, 6).reshape(Cout, 9, Cin).copy()
        blk = np.arange(Cout)[:, None, None] // 16 % 4 != np.arange(Cin)[None, None, :] // 16 % 4
        region[:] = np.broadcast_to(blk, ref.shape)
        return m, ref, bnd, region
    slabs = h.slabs(nsplit)[0]
    size = Cout * 9 * Cin
    rdst, _ = reduce_ref(slabs, Cin - 59, Cin * 9, 9, 1, size)     # 59 operand channels have no slot in the parameter
    rb = reduce_ref(bnd[None], Cin - 59, Cin * 9, 9, 1, size)[0]
    if name == "cin_valid_ignored":
        m, _ = reduce_ref(slabs, 0, Cin * 9, 9, 1, size)
        return m, rdst, rb, np.isnan(rdst)
    if name == "strides_exchanged":                # s_ci and s_t exchanged, every channel valid (colliding writes: the last one stays)
        s = slabs.sum(0)
        co, t, ci = np.meshgrid(np.arange(Cout), np.arange(9), np.arange(Cin), indexing="ij")
        m = np.full(size, np.nan)
        m[(co * Cin * 9 + ci * 1 + t * 9).reshape(-1)] = s.reshape(-1)
        return m, reduce_ref(slabs, 0, Cin * 9, 9, 1, size)[0], reduce_ref(bnd[None], 0, Cin * 9, 9, 1, size)[0], np.ones(size, dtype=bool)
    if name == "atomics_overwrite":                # the first partial is stored over dw, not added to it
        region[:] = True
        return ref, h.dw0 + ref, h.bound(nsplit, True), region
    raise KeyError(name)


def offenders(got, ref, bnd):
    """elements outside their bound; NaN = not written: an offender exactly where only one side is written"""
    g, r = np.isnan(got), np.isnan(ref)
    with np.errstate(invalid="ignore"):
        return (g != r) | (~g & ~r & ~(np.abs(got - ref) <= np.where(np.isnan(bnd), 0.0, bnd)))
