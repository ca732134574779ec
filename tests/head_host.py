"""Independent yardstick of the head-tail, map-loss and fused head-conv kernels (csrc/head_tail.hip: head_tail_fwd*/bwd*, map_loss_fwd and the two
finalizers; csrc/head_conv.hip: head_conv_tail64, head_out_dgrad64): plain numpy restatements of each operation from its definition on [M][C] row-major
arrays, M = N * HW pixels, no device code.  Operands enter as the values they have after storage (logits, coordinates, extents, targets and
statistics fp32; pnp, d_pnp, x, w, dy, raw in the type under test).  Every function takes the dtype it computes in: np.float64 is the
reference, np.float32 the "reference at the kernel's precision" whose distance from the fp64 run (e32) sizes the bounds of everything that goes
through expf / logf -- the convention of tests/pose_host.py.  tests/test_head_host_cpu.py pins this module against fp64 autograd of
oracle.gdrn_oracle.gdrn_loss; tests/test_head_tail_edges_gpu.py holds the kernels to it.

Layout: head [M][>= nreg + 5] = (mask, x, y, z, region class 0 .. nreg); coord2d [N][2][HW]; extents [N][3]; gt_xyz [N][3][HW]; mvis, mtr [M]
(0 or 1: products with them are exact, which the counts below use); gt_region [M] int64; pnp / d_pnp / d_head [M][>= nreg + 5] =
(xyz * extent (3), coord2d (2), softmax over classes 1 .. nreg).

Bounds.  Where a result is a handful of fp32 operations the bound is norm_host.bound(ref, A, k, u): A the reference's expression on absolute
values, k = 2 r for r fp32 roundings on the kernel's path (counted next to each function, for the uncontracted form).  Where it goes through the
device's expf / logf (softmax, cross entropy) nobody has measured libm here, so no ulp figure is assumed: the kernel is held to
pose_host.decode_bound(e32) = 8 e32 + 16 * 2^-24 relative to the row's largest magnitude, plus u_T |ref| for a 16-bit store.  Signs, copies,
zeros and sentinels are exact.  No figure observed from a kernel enters anything here."""
import numpy as np

import norm_host as NH
from pose_host import decode_bound

EPS32 = NH.EPS32
# below the smallest normal fp32 number a softmax value is at the mercy of subnormal rounding (2^-149 absolute per operation) and of whether
# the device's expf flushes: everything derived from one gets this absolute floor (1.2e-38) on top of its relative bound
FLOOR = 2.0 ** -126
GW = np.array([1.0, 0.5, 2.0, 1.5, 0.7], dtype=np.float32)   # dL/d(loss_coor_x, _y, _z, loss_mask, loss_region) of every case


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _roi(M, HW):
    return np.arange(M) // HW


def _planes(a, dt):
    """[N][C][HW] -> [M][C]"""
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(0, 2, 1).reshape(-1, a.shape[1])).astype(dt)


def softmax(z, dt):
    z = np.asarray(z).astype(dt)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def rel_rows(a32, a64):
    """e32 of a [rows][C] quantity: largest |fp32 run - fp64 run| relative to the fp64 row's largest magnitude (rows of zeros count as 1)"""
    m = np.abs(f64(a64)).max(1, keepdims=True)
    m = np.where(m > 0, m, 1.0)
    return float((np.abs(f64(a32) - f64(a64)) / m).max()), m


# ------------------------------------------------------------------------------------------------ the tail
# channels 0..2: (h - 0.5f) [1] * extent [1]  ->  r = 2, k = 4, A = (|h| + 0.5) |extent|.  Channels 3, 4: copies of coord2d (exact; a 16-bit
# store rounds them: the tests compare with norm_host.store(coord2d)).  Channels 5..: exp(r - max) / sum, relative to the row's largest softmax
# value by decode_bound(e32).
K_XYZ = 4


def tail(head, coord2d, extents, nreg, dt=np.float64):
    N, _, HW = np.shape(coord2d)
    M = N * HW
    h = np.asarray(head)[:, :nreg + 5].astype(dt)
    out = np.empty((M, nreg + 5), dtype=dt)
    out[:, :3] = (h[:, 1:4] - dt(0.5)) * np.asarray(extents).astype(dt)[_roi(M, HW)]
    out[:, 3:5] = _planes(coord2d, dt)
    out[:, 5:] = softmax(h[:, 5:], dt)
    return out


def tail_mag(head, extents, HW):
    M = np.shape(head)[0]
    return (np.abs(f64(head)[:, 1:4]) + 0.5) * np.abs(f64(extents))[_roi(M, HW)]


def tail_bound(p64, p32, mag_xyz, kind):
    """(bound [M][nreg + 5], e32 of the softmax); channels 3, 4 get 0: they are copies"""
    u = NH.U[kind]
    e32, rowmax = rel_rows(p32[:, 5:], p64[:, 5:])
    b = np.zeros(p64.shape)
    b[:, :3] = NH.bound(p64[:, :3], mag_xyz, K_XYZ, u)
    b[:, 5:] = np.maximum(u * np.abs(p64[:, 5:]), NH.TINY[u]) + decode_bound(e32) * rowmax + FLOOR
    return b, e32


# ------------------------------------------------------------------------------------------------ the map losses
# per pixel: three terms |h_c mv - gt_c mv| and |h0 - mtr| (mv in {0, 1}: the products are exact, the subtraction rounds once relative to the
# term itself) and the cross entropy over the nreg + 1 classes of z = logits * mv with target gt_region * mv: (logf(sum exp(z - max)) + max) - z_t.
# Its magnitude A_ce = |max| + max(|log sum|, 1) + |z_t|: the sum lies in [1, nreg + 1] and carries roundings of 2^-24 of itself, which logf
# turns into 2^-24 ABSOLUTE however small log(sum) is -- hence the floor of 1.
def map_terms(head, gt_xyz, mvis, mtr, gt_region, nreg, dt=np.float64):
    """terms [M][6] (three masked L1 terms, mask L1, cross entropy, mv) and A_ce [M]"""
    M = np.shape(head)[0]
    h = np.asarray(head)[:, :nreg + 5].astype(dt)
    mv = np.asarray(mvis).astype(dt)
    t = np.empty((M, 6), dtype=dt)
    t[:, :3] = np.abs(h[:, 1:4] * mv[:, None] - _planes(gt_xyz, dt) * mv[:, None])
    t[:, 3] = np.abs(h[:, 0] - np.asarray(mtr).astype(dt))
    z = h[:, 4:] * mv[:, None]
    tgt = np.asarray(gt_region, dtype=np.int64) * np.asarray(mvis).astype(np.int64)
    mz = z.max(1)
    ls = np.log(np.exp(z - mz[:, None]).sum(1))
    zt = z[np.arange(M), tgt]
    t[:, 4] = (ls + mz) - zt
    t[:, 5] = mv
    return t, np.abs(f64(mz)) + np.maximum(np.abs(f64(ls)), 1.0) + np.abs(f64(zt))


def map_sums(head, gt_xyz, mvis, mtr, gt_region, nreg, dt=np.float64):
    """(totals [6] in fp64, terms [M][6], A_ce [M])"""
    t, a_ce = map_terms(head, gt_xyz, mvis, mtr, gt_region, nreg, dt)
    return f64(t).sum(0), t, a_ce


def losses(totals, M, clamp=True):
    """the five map losses of GDRN.gdrn_loss from the six totals; den = max(sum mv, 1) (clamp=False: the CPU module's perturbation)"""
    tot = f64(totals)
    den = max(tot[5], 1.0) if clamp else tot[5]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([tot[0] / den, tot[1] / den, tot[2] / den, tot[3] / float(M), tot[4] / den])


# Totals: lane 0 of a pixel's 16 lanes carries its pixels' terms in fp32 -- `carry` terms, the grid-stride iterations of the kernel (x 4 passes
# per group in the fused kernel) -- then everything is fp64 (16 lanes per workgroup, atomics or partial rows: 2^-53 per add, under the
# u |total| term).  A term meets its own rounding [1] and carry - 1 adds relative to a partial sum <= sum|terms|: r = carry, k = 2 carry.  The
# cross-entropy terms add their own decode_bound(e32) A_ce each.  sum mv is a count below 2^24: exact.
def totals_bound(t64, t32, a_ce, carry):
    """(bound [6], e32 of the cross-entropy term relative to A_ce)"""
    tot, A = f64(t64).sum(0), np.abs(f64(t64)).sum(0)
    e32 = float((np.abs(f64(t32[:, 4]) - f64(t64[:, 4])) / a_ce).max())
    b = NH.bound(tot, A, 2 * carry, EPS32)
    b[4] += decode_bound(e32) * a_ce.sum()
    b[5] = 0.0
    return b, e32


def losses_bound(tot_bound, totals, M):
    """the finalizers divide the fp64 totals in fp64 and round once to fp32"""
    ref = losses(totals, M)
    den = max(f64(totals)[5], 1.0)
    return np.array([tot_bound[0] / den, tot_bound[1] / den, tot_bound[2] / den, tot_bound[3] / M, tot_bound[4] / den]) + EPS32 * np.abs(ref)


# ------------------------------------------------------------------------------------------------ the tail's backward pass
# A replay from the stored pnp and d_pnp (what the kernel reads).  cs = gce * mv [1] * (float)(1 / den) [1 + 1] -> 3 roundings.
#   class k: cs * (p_k - [k = tgt]) + s_k * (d_k - sum s d) for k >= 1 (class 0: the first term only), p = softmax(z mv) over nreg + 1 classes.
#     first term: cs 3, the difference 1, the product 1 -> 5 of A_cs = |cs| (p_k + [k = tgt]); p itself by decode_bound(e32) of the row maximum.
#     second term: the dot product -- products [1], <= 4 adds in the lane, 4 DPP adds -> 9 of sum|s d|; d_k - dot [1], * s_k [1] -> 11 of
#     A_att = |s_k| (|d_k| + sum|s d|).  The sum of the two [1] relative to <= A_cs + A_att  ->  r = 6 resp. 12, k = 12 resp. 24.
#   channel 0: gmask * (float)(1 / M) * sign(h0 - mtr); channels 1..3: gx_c * mv * (float)(1 / den) * sign(h_c mv - gt_c mv): a sign times an
#     fp32 constant -- sign_consts() replays the constant operation by operation, the tests compare bit for bit.  With d_pnp: + d_c * extent_c
#     [1], the sum [1], on top of the constant's 3 -> r = 5, k = 10 of |const| + |d_c| |extent_c|.
K_CS, K_ATT, K_LIN = 12, 24, 10


def tail_bwd(head, pnp, d_pnp, extents, gt_xyz, mvis, mtr, gt_region, gw, den, nreg, HW, dt=np.float64, att0=False):
    """dict(d [M][nreg + 5], p [M][nreg + 1], cs [M], A_cs, A_att [M][nreg + 1], A_lin [M][3]); pnp = d_pnp = None: the losses' gradient alone.
    att0: the CPU module's perturbation "class 0 included in the attention softmax" (channel 4 read as a class)."""
    M = np.shape(head)[0]
    h = np.asarray(head)[:, :nreg + 5].astype(dt)
    mv = np.asarray(mvis).astype(dt)
    gw = np.asarray(gw).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_den = dt(1.0) / dt(den)
        cs = gw[4] * mv * inv_den
        cx = gw[:3][None] * mv[:, None] * inv_den
    p = softmax(h[:, 4:] * mv[:, None], dt)
    tgt = np.asarray(gt_region, dtype=np.int64) * np.asarray(mvis).astype(np.int64)
    hot = np.zeros((M, nreg + 1), dtype=dt)
    hot[np.arange(M), tgt] = 1
    d = np.zeros((M, nreg + 5), dtype=dt)
    d[:, 4:] = cs[:, None] * (p - hot)
    d[:, 0] = gw[3] / dt(M) * np.sign(h[:, 0] - np.asarray(mtr).astype(dt))
    d[:, 1:4] = cx * np.sign(h[:, 1:4] * mv[:, None] - _planes(gt_xyz, dt) * mv[:, None])
    A_att, A_lin = np.zeros((M, nreg + 1)), np.abs(f64(cx))
    if d_pnp is not None:
        lo = 4 if att0 else 5
        s, g = np.asarray(pnp)[:, lo:nreg + 5].astype(dt), np.asarray(d_pnp)[:, lo:nreg + 5].astype(dt)
        dot = (s * g).sum(1, keepdims=True)
        d[:, lo:] += s * (g - dot)
        A_att[:, lo - 4:] = np.abs(f64(s)) * (np.abs(f64(g)) + np.abs(f64(s) * f64(g)).sum(1, keepdims=True))
        ex = np.asarray(extents).astype(dt)[_roi(M, HW)]
        d[:, 1:4] += np.asarray(d_pnp)[:, :3].astype(dt) * ex
        A_lin = A_lin + np.abs(f64(d_pnp)[:, :3]) * np.abs(f64(ex))
    return dict(d=d, p=p, cs=cs, A_cs=np.abs(f64(cs))[:, None] * (f64(p) + f64(hot)), A_att=A_att, A_lin=A_lin)


def tail_bwd_bound(r64, r32, kind, with_dpnp):
    """(bound [M][nreg + 5], e32 of softmax(z mv)).  Channel 0 -- and channels 1..3 without d_pnp -- get 0: the tests compare them with the
    stored sign_consts() bit for bit."""
    u = NH.U[kind]
    e32, rowmax = rel_rows(r32["p"], r64["p"])
    d = f64(r64["d"])
    b = np.zeros(d.shape)
    b[:, 4:] = (np.maximum(u * np.abs(d[:, 4:]), NH.TINY[u]) + (1.0 + u) * EPS32 * (K_CS * r64["A_cs"] + K_ATT * r64["A_att"])
                + np.abs(f64(r64["cs"]))[:, None] * decode_bound(e32) * rowmax + FLOOR)
    if with_dpnp:
        b[:, 1:4] = NH.bound(d[:, 1:4], r64["A_lin"], K_LIN, u)
    return b, e32


def sign_consts(gw, M, den, kind):
    """the fp32 constants of d_head's channels 0 and 1..3 at mv = 1, one IEEE operation at a time as the kernels do it, after storage in `kind`"""
    gw = f32(gw)
    inv_np, inv_den = np.float32(1.0 / float(M)), np.float32(1.0 / float(den))
    c0 = np.float32(gw[3] * inv_np)
    cx = (gw[:3] * np.float32(1.0)).astype(np.float32) * inv_den
    return float(NH.store(c0, kind)), NH.store(cx.astype(np.float32), kind)


def tail_bwd_exact(head, gt_xyz, mvis, mtr, gw, den, HW, kind):
    """channels 0..3 of d_head without d_pnp, as stored: sign * constant"""
    M = np.shape(head)[0]
    h, mv = f64(head), f64(mvis)
    c0, cx = sign_consts(gw, M, den, kind)
    out = np.empty((M, 4))
    out[:, 0] = c0 * np.sign(h[:, 0] - f64(mtr))
    out[:, 1:] = cx[None] * mv[:, None] * np.sign(h[:, 1:4] * mv[:, None] - _planes(gt_xyz, np.float64) * mv[:, None])
    return out


# ------------------------------------------------------------------------------------------------ the fused kernels' GEMMs
# logits = bias + sum over 256 products of 16-bit operands (exact in fp32), accumulated in fp32 in the MFMA's order: the form of pose_host's
# fc_bound, (256 + 2) 2^-24 sum|w||x| + |bias| (255 adds, the bias, one for the accumulator's own order).
def conv_logits(x, w, bias):
    """x [M][256], w [69][256] (values of the 16-bit type), bias [69] fp32 -> (logits [M][69], magnitude, bound)"""
    x, w, b = f64(x)[:, :256], f64(w)[:69, :256], f64(bias)[:69]
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)[None]
    return x @ w.T + b[None], mag, (256 + 2) * EPS32 * mag


# data gradient: g[m][ci] = sum over the 69 logit gradients dy[m][k] wd[ci][k] (columns >= 69 of both are zero and add exact zeros): (69 + 2)
# 2^-24 sum|dy||wd| in fp32, kept where scale * raw + shift > 0 (two roundings, or one as an fma: elements with |scale raw + shift| <= 4 * 2^-24
# (|scale raw| + |shift|) are `marginal` -- their mask is not determined by the inputs), stored in 16 bits.  The two BatchNorm-backward sums
# take the fp32 g BEFORE that store: per channel a lane adds `terms` values in order, then 3 shuffle levels, 3 wave adds (norm_host.k_sum covers
# 6 + 3), the partial rows are added in fp64 by the test; a term of the second sum carries 3 more roundings (norm_host.bn_bwd_sums); on top
# every term carries its g's own GEMM bound, and a marginal element may enter or leave with its whole |term|.
def out_dgrad(dy, wd, raw, mean, invstd, scale, shift, terms):
    dy, wd, raw = f64(dy), f64(wd), f64(raw)[:, :256]
    K = min(dy.shape[1], wd.shape[1])
    g = dy[:, :K] @ wd[:256, :K].T
    gmag = np.abs(dy[:, :K]) @ np.abs(wd[:256, :K]).T
    sc, sh, mean, invstd = f64(scale)[None], f64(shift)[None], f64(mean), f64(invstd)
    arg = sc * raw + sh
    keep = arg > 0.0
    marginal = np.abs(arg) <= 4 * EPS32 * (np.abs(sc * raw) + np.abs(sh))
    gm = np.where(keep, g, 0.0)
    gb = np.where(keep, (69 + 2) * EPS32 * gmag, 0.0)
    s1, s2 = NH.bn_bwd_sums(gm, raw, mean, invstd)
    m1, m2 = NH.bn_bwd_sums_mag(gm, raw, mean, invstd)
    xh = (np.abs(raw) + np.abs(mean)[None]) * np.abs(invstd)[None]
    flip = np.where(marginal, np.abs(g), 0.0)
    b1 = NH.bound(s1, m1, NH.k_sum(terms), EPS32) + gb.sum(0) + flip.sum(0)
    b2 = NH.bound(s2, m2, NH.k_sum(terms) + 3, EPS32) + (gb * xh).sum(0) + (flip * xh).sum(0)
    return dict(g=gm, keep=keep, marginal=marginal, gmag=gmag, gbound=gb, s1=s1, s2=s2, b1=b1, b2=b2)


def dx_bound(r, kind):
    u = NH.U[kind]
    return np.maximum(u * np.abs(r["g"]), NH.TINY[u]) + (1.0 + u) * r["gbound"]


# ------------------------------------------------------------------------------------------------ seeded inputs (shared by the CPU and the GPU module)
ROW_KINDS = ("random", "one-hot", "equal", "offset", "minus80")


def make_inputs(seed, N, HW, nreg, kind="fp32", all_masked=False):
    """fp32 arrays of one case.  Logit rows (classes 0 .. nreg): random at scale 1.5; near-one-hot (one class 30, the others -30: a spread of
    60); all equal; a common offset of +80; rows with -80 entries.  Targets 0, 1, nreg - 1 and nreg sit on the first visible pixels, a quarter
    of the pixels is masked out (all_masked: every one), every fifth pixel has h0 == mtr and every seventh h_c == gt_c for one coordinate.
    d_pnp holds values of the storage type `kind`."""
    rg = np.random.default_rng(seed)
    M, C = N * HW, nreg + 5
    head = 1.5 * rg.standard_normal((M, C))
    rk = rg.integers(0, 8, M)
    rk[:min(M, 5)] = np.arange(min(M, 5))            # the first pixels take one row of each kind, the last ones too
    rk[max(M - 5, 0):] = np.arange(5)[:M - max(M - 5, 0)]
    hot = rg.integers(0, nreg + 1, M)
    r1 = rk == 1
    head[r1, 4:] = -30.0 + 0.5 * rg.standard_normal((int(r1.sum()), nreg + 1))
    head[np.nonzero(r1)[0], 4 + hot[r1]] += 60.0
    head[rk == 2, 4:] = (3.0 * rg.standard_normal(int((rk == 2).sum())))[:, None]
    head[rk == 3, 4:] += 80.0
    m80 = (rk == 4)[:, None] & (rg.random((M, nreg + 1)) < 0.5)
    head[:, 4:][m80] = -80.0
    head = f32(head)
    mvis = f32(rg.random(M) < 0.75)
    if M >= 8:
        mvis[:4] = 1.0
        mvis[M - 1] = 1.0
    if all_masked:
        mvis[:] = 0.0
    mtr = f32(rg.random(M) < 0.5)
    greg = rg.integers(0, nreg + 1, M).astype(np.int64)
    vis = np.nonzero(mvis > 0)[0]
    for i, t in zip(vis, (0, 1, nreg - 1, nreg)):
        greg[i] = t
    if len(vis):
        greg[vis[-1]] = nreg
    head[::5, 0] = mtr[::5]
    gxyz = f32(rg.random((N, 3, HW)))
    flat = gxyz.transpose(0, 2, 1).reshape(M, 3)
    for c in range(3):
        flat[c::7, c] = head[c::7, 1 + c]
    gxyz = f32(flat.reshape(N, HW, 3).transpose(0, 2, 1))
    return dict(head=head, coord2d=f32(rg.standard_normal((N, 2, HW))), extents=f32(0.05 + 0.25 * rg.random((N, 3))), gt_xyz=gxyz,
                mvis=mvis, mtr=mtr, gt_region=greg, d_pnp=f32(NH.store(0.01 * rg.standard_normal((M, C)), kind)), gw=GW.copy(),
                N=N, HW=HW, nreg=nreg, M=M)


def seed_of(N, HW, nreg):
    return 9000 + 131 * nreg + 7 * N + HW


class Case:
    """one seeded case with its fp64 and fp32 references, computed once (tail, losses, backward from the fp64 tail stored in `kind`)"""

    def __init__(self, N, HW, nreg, kind="fp32", all_masked=False):
        a = self.a = make_inputs(seed_of(N, HW, nreg), N, HW, nreg, kind, all_masked)
        self.kind, self.M, self.nreg, self.HW = kind, a["M"], nreg, HW
        self.p64, self.p32 = (tail(a["head"], a["coord2d"], a["extents"], nreg, dt) for dt in (np.float64, np.float32))
        self.mag_xyz = tail_mag(a["head"], a["extents"], HW)
        (self.tot, self.t64, self.a_ce), (_, self.t32, _) = (map_sums(a["head"], a["gt_xyz"], a["mvis"], a["mtr"], a["gt_region"], nreg, dt)
                                                            for dt in (np.float64, np.float32))
        self.den = max(self.tot[5], 1.0)
        self.losses = losses(self.tot, self.M)

    def bwd(self, pnp, with_dpnp, dt=np.float64):
        a = self.a
        return tail_bwd(a["head"], pnp if with_dpnp else None, a["d_pnp"] if with_dpnp else None, a["extents"], a["gt_xyz"], a["mvis"], a["mtr"],
                        a["gt_region"], a["gw"], self.den, self.nreg, self.HW, dt)


_CASES = {}


def case(N, HW, nreg, kind="fp32", all_masked=False):
    key = (N, HW, nreg, kind, all_masked)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


POISON = {"fp32": 1e30, "bf16": 1e30, "fp16": 6e4}   # columns a kernel must not read: large and finite in the type (NaN would hide in a max)


def conv_inputs(seed, M, kind, x_cs=256, w_rows=69):
    """16-bit operands of the fused forward: activations at scale 1 (post-ReLU-like: half of them zero), weights at 1/16, fp32 bias; the
    columns >= 256 of x and the rows >= 69 of w are poisoned: the kernel must not read them"""
    rg = np.random.default_rng(seed)
    x = np.full((M, x_cs), POISON[kind])
    x[:, :256] = np.maximum(rg.standard_normal((M, 256)), 0.0)
    w = np.full((w_rows, 256), POISON[kind])
    w[:69] = rg.standard_normal((69, 256)) / 16.0
    return NH.store(x, kind), NH.store(w, kind), f32(0.3 * rg.standard_normal(69))


def dgrad_inputs(seed, M, kind, dy_cs=128, wd_cs=128, raw_cs=256):
    """dy [M][dy_cs] and wd [256][wd_cs] with zero columns >= 69, raw [M][raw_cs] (columns >= 256 poisoned), fp32 statistics.  raw at scale 1.5
    around 0.3 against scale in [0.5, 1.5) and shift at 0.3: about half of the elements are kept and next to none is marginal"""
    rg = np.random.default_rng(seed)
    dy, wd = np.zeros((M, dy_cs)), np.zeros((256, wd_cs))
    dy[:, :69] = 0.02 * rg.standard_normal((M, 69))
    wd[:, :69] = rg.standard_normal((256, 69)) / 16.0
    raw = np.full((M, raw_cs), POISON[kind])
    raw[:, :256] = 1.5 * rg.standard_normal((M, 256)) + 0.3
    scale = f32(0.5 + rg.random(256))
    scale[1::4] *= -1.0
    return dict(dy=NH.store(dy, kind), wd=NH.store(wd, kind), raw=NH.store(raw, kind), mean=f32(0.2 * rg.standard_normal(256)),
                invstd=f32(0.5 + rg.random(256)), scale=scale, shift=f32(0.3 * rg.standard_normal(256)))


# the case tables
SMALL = [(1, 16), (1, 17), (3, 80), (3, 1023)]                     # the CPU module's shapes
FAST_SHAPES = [(1, 16), (1, 17), (3, 4095), (2, 4096), (3, 21861)]  # 64-region kernels: 4096 workgroups of 16 pixels -> M = 65583 leaves 47 for a second pass
GENERIC_SHAPES = [(1, 16), (3, 1023), (2, 16400)]                  # M = 32800 passes the 2048-workgroup cap of map_loss_fwd_kernel
GENERIC_NREG = [1, 5, 16, 17, 32, 63]
FUSED_SHAPES = [(1, 16), (1, 48), (3, 80), (2, 32784)]             # 4098 groups against 1024 workgroups x 4 waves
DGRAD_SHAPES = FUSED_SHAPES + [(1, 32800)]                         # 2050 groups against 512 x 4 waves
