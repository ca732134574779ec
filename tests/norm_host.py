"""Independent fp64 numpy yardstick of the normalisation / pooling / resampling tests (csrc/norm.hip): plain restatements of each operation from
its definition, NHWC like the kernels' tensors, no torch.  Per-channel constants (scale, shift, mean, invstd, gamma, ...) enter as the fp32
values the device is given, operands as the values they have after storage in the type under test; everything is promoted to fp64 here.

Next to every reference stands its MAGNITUDE (`*_mag`): the same expression evaluated on the absolute values of its terms, the `A` of the
per-element bound of the tests

    |got - ref| <= u_T * |ref| + (1 + u_T) * k * 2^-24 * A          (bound() below)

u_T the unit roundoff of the storage type (one final rounding of the result), k from the number r of fp32 roundings on the kernel's path (derived
in a comment next to each reference; first-order: every rounding perturbs by at most 2^-24 of an intermediate that is itself bounded by A, so
r * 2^-24 * A is the worst case of ANY fp32 evaluation with these roundings).  The element-wise kernels are held to k = 2 r (r counted for the
uncontracted form, hipcc being free to fuse or not): tests/test_norm_host_cpu.py demands that an independent fp32 evaluation (torch on the CPU)
sits inside HALF of every bound, which a worst-case count can only promise with that factor.  No device figure enters any k."""
import numpy as np

U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}
EPS32 = 2.0 ** -24
# the bilinear pair: the fp32 source coordinate sh * o carries an absolute error of up to 2^-23 * H
def k_bilinear(H, W):
    return 8 + 4 * max(H, W)


def k_sum(terms_per_thread):
    """per-thread sequential walk + up to six shuffle levels + three wave adds (A = sum of |terms|)"""
    return terms_per_thread + 9


def f64(a):
    return np.asarray(a, dtype=np.float64)


# half the spacing of the storage type's subnormals: what the final rounding can cost a result below the smallest normal number, where
# u_T |ref| no longer covers it (an fp16 activation of 2e-5 sits on a grid of 2^-24)
TINY = {2.0 ** -8: 2.0 ** -134, 2.0 ** -11: 2.0 ** -25, 2.0 ** -24: 2.0 ** -150}


def bound(ref, A, k, u):
    return np.maximum(u * np.abs(ref), TINY[u]) + (1.0 + u) * k * EPS32 * f64(A)


# ------------------------------------------------------------------------------------------------ BatchNorm
# bn_apply_kernel: t = x * scale [1] + shift [1] (one rounding as an fma); t += res [1]; max(t, 0) [exact]  ->  r = 3, k = 6
K_BN_APPLY = 6


def bn_apply(x, scale, shift, res=None, relu=False):
    t = f64(x) * f64(scale) + f64(shift)
    if res is not None:
        t = t + f64(res)
    return np.maximum(t, 0.0) if relu else t


def bn_apply_mag(x, scale, shift, res=None):
    t = np.abs(f64(x)) * np.abs(f64(scale)) + np.abs(f64(shift))
    return t if res is None else t + np.abs(f64(res))


def bn_mask(dy, ymask=None, x=None, msc=None, msh=None):
    """g = dy where (ymask > 0) and (x * msc + msh > 0), each mask optional; else exactly 0"""
    keep = np.ones(np.shape(dy), dtype=bool)
    if ymask is not None:
        keep &= f64(ymask) > 0.0
    if msc is not None:
        keep &= f64(x) * f64(msc) + f64(msh) > 0.0
    return np.where(keep, f64(dy), 0.0), keep


# bn_bwd_reduce_kernel, per channel: s1 = sum g (no term rounding), s2 = sum g * (x - mean) * invstd (3 roundings per term, each relative to a
# quantity <= the term's magnitude |g| (|x| + |mean|) |invstd|); accumulation: a term passes through at most (terms per thread - 1) sequential
# adds, log2(64 / tpr) <= 6 shuffle levels and 3 wave adds  ->  k <= terms per thread + 11 to first order; the tests hold the kernels to
# k_sum() = terms per thread + 9
def bn_bwd_sums(g, x, mean, invstd):
    C = g.shape[-1]
    g2, x2 = f64(g).reshape(-1, C), f64(x).reshape(-1, C)
    return g2.sum(0), (g2 * (x2 - f64(mean)) * f64(invstd)).sum(0)


def bn_bwd_sums_mag(g, x, mean, invstd):
    C = g.shape[-1]
    g2, x2 = np.abs(f64(g)).reshape(-1, C), np.abs(f64(x)).reshape(-1, C)
    return g2.sum(0), (g2 * (x2 + np.abs(f64(mean))) * np.abs(f64(invstd))).sum(0)


# bn_bwd_coef_kernel (from fp64 totals): m1 = (float)s1 [1] * inv_n [inv_n rounded: 1, product: 1] -> 3, likewise m2; a = gamma * invstd [1];
# b = -a * invstd * m2 [a 1, m2 3, two products 2 -> 6]; c = -a * m1 - b * mean [first term a 1 + m1 3 + product 1 = 5 of |a m1|, second term
# b 6 + product 1 = 7 of |b mean|, the difference 1 -> at most 8 of the magnitude]  ->  r = 8, k = 16
K_COEF = 16


def bn_bwd_coef(s1, s2, npix, gamma, mean, invstd):
    """(a, b, c, dgamma, dbeta) of dx = a*g + (b*x + c)"""
    s1, s2, gamma, mean, invstd = f64(s1), f64(s2), f64(gamma), f64(mean), f64(invstd)
    a = gamma * invstd
    b = -a * invstd * (s2 / npix)
    c = -a * (s1 / npix) - b * mean
    return a, b, c, s2, s1


def bn_bwd_coef_mag(s1, s2, npix, gamma, mean, invstd):
    s1, s2, gamma, mean, invstd = (np.abs(f64(v)) for v in (s1, s2, gamma, mean, invstd))
    a = gamma * invstd
    b = a * invstd * (s2 / npix)
    return a, b, a * (s1 / npix) + b * mean


# bn_bwd_apply_kernel: o = a * g + (b * x + c): two products, two sums (two roundings as the kernel's nested fma)  ->  r = 4, k = 8
K_BN_BWD_APPLY = 8


def bn_bwd_apply(g, x, a, b, c):
    return f64(a) * f64(g) + (f64(b) * f64(x) + f64(c))


def bn_bwd_apply_mag(g, x, a, b, c):
    return np.abs(f64(a)) * np.abs(f64(g)) + (np.abs(f64(b)) * np.abs(f64(x)) + np.abs(f64(c)))


# bn_finalize_rows_kernel: fp64 up to mean / invstd (each 1 rounding to fp32); scale = gamma * (float)is [2]; shift = beta - (float)m * scale
# [on top of scale: m 1, product 1, difference 1 -> 5]; running = (1 - mom) * r + mom * (float)v [(1 - mom): 1, products 2, sum 1, v: 1 -> 5]
# ->  r = 5, k = 10
K_FINALIZE = 10


def bn_finalize(s1, s2, count, gamma, beta, eps, running_mean=None, running_var=None, momentum=0.1):
    s1, s2 = f64(s1), f64(s2)
    m = s1 / count
    var = np.maximum(s2 / count - m * m, 0.0)
    istd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    scale = f64(gamma) * istd
    out = dict(mean=m, invstd=istd, scale=scale, shift=f64(beta) - m * scale, var=var)
    if running_mean is not None:
        mom = float(np.float32(momentum))
        unb = var * count / (count - 1.0) if count > 1 else var
        out["running_mean"] = (1.0 - mom) * f64(running_mean) + mom * m
        out["running_var"] = (1.0 - mom) * f64(running_var) + mom * unb
        out["running_mean_mag"] = (1.0 - mom) * np.abs(f64(running_mean)) + mom * np.abs(m)
        out["running_var_mag"] = (1.0 - mom) * np.abs(f64(running_var)) + mom * unb
    out["shift_mag"] = np.abs(f64(beta)) + np.abs(m) * np.abs(scale)
    return out


# ------------------------------------------------------------------------------------------------ stem pool
# bn_relu_maxpool_fwd_kernel: a = max(x * scale + shift, 0) [2 roundings, or 1 when contracted]; the maximum itself is exact  ->  r = 2, k = 4
K_POOL = 4


def _pool_taps(a, fill):
    """a [N,H,W,C] -> [9,N,H/2,W/2,C]: tap ky*3+kx of the 3x3 stride-2 pad-1 window of every output pixel, `fill` outside the map"""
    N, H, W, C = a.shape
    p = np.full((N, H + 2, W + 2, C), fill, dtype=a.dtype)
    p[:, 1:-1, 1:-1] = a
    return np.stack([p[:, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)])


def bn_relu_maxpool(x, scale, shift):
    """max over the window of relu(x*scale + shift) and the code ky*3 + kx of the FIRST tap in (ky, kx) scan order that attains it"""
    a = np.maximum(f64(x) * f64(scale) + f64(shift), 0.0)
    taps = _pool_taps(a, -np.inf)
    return taps.max(0), taps.argmax(0).astype(np.uint8)     # (argmax returns the first maximum)


def bn_relu_maxpool_mag(x, scale, shift):
    return _pool_taps(np.abs(f64(x)) * np.abs(f64(scale)) + np.abs(f64(shift)), 0.0).max(0)


def pool_top2_gap(x, scale, shift):
    """per window: (best - second best candidate, their magnitude) over DISTINCT values of relu(x*scale + shift) -- exact ties have a rule (first
    tap) and are compared; a window is ambiguous only when two different candidates sit within rounding of each other"""
    a = np.maximum(f64(x) * f64(scale) + f64(shift), 0.0)
    m = np.abs(f64(x) * f64(scale)) + np.abs(f64(shift))
    taps, mt = _pool_taps(a, -np.inf), _pool_taps(m, 0.0)
    best = taps.max(0)
    second = np.where(taps < best, taps, -np.inf).max(0)
    return best - second, mt.max(0)


# maxpool_bwd_kernel: at most four windows contain a pixel; acc += dy of those whose tap code points here [<= 3 roundings], masked by
# x*scale + shift > 0  ->  r = 3, k = 6 (A = sum of |dy| over the contributing windows)
K_POOL_BWD = 6


def maxpool_bwd(dy, idx, x, scale, shift, mag=False):
    N, H, W, C = x.shape
    d = np.abs(f64(dy)) if mag else f64(dy)
    g = np.zeros((N, H + 2, W + 2, C))
    for ky in range(3):
        for kx in range(3):
            g[:, ky:ky + H:2, kx:kx + W:2] += np.where(idx == ky * 3 + kx, d, 0.0)
    g = g[:, 1:-1, 1:-1]
    return np.where(f64(x) * f64(scale) + f64(shift) > 0.0, g, 0.0)


def affine_sign_margin(x, scale, shift):
    """elements whose sign of x*scale + shift an fp32 evaluation that may or may not contract the product could see differently:
    |x*scale + shift| <= 2^-22 (|x*scale| + |shift|), zero magnitude (an exact 0 in every evaluation) excepted"""
    p, s = f64(x) * f64(scale), f64(shift) + np.zeros(np.shape(x))
    mag = np.abs(p) + np.abs(s)
    return (np.abs(p + s) <= 2.0 ** -22 * mag) & (mag > 0.0) & (p + s != 0.0)


# ------------------------------------------------------------------------------------------------ 2x bilinear, align_corners=True
def up_matrix(n_in):
    """[2*n_in, n_in] interpolation matrix; source coordinate of output o is the exact rational o*(in-1)/(out-1)"""
    n_out = 2 * n_in
    U_ = np.zeros((n_out, n_in))
    for o in range(n_out):
        num = o * (n_in - 1)
        i0, rem = divmod(num, n_out - 1)
        l1 = rem / (n_out - 1)
        U_[o, i0] += 1.0 - l1
        U_[o, min(i0 + 1, n_in - 1)] += l1
    return U_


# forward (up_lerp): weights from f = sh * o in fp32 (sh rounded: 2^-24 relative, the product another 2^-24: |df| <= 2^-23 * H; ly1 = f - y0 exact,
# ly0 = 1 - ly1 [1]); a weight error dw moves the result by <= |dw| * 2 max|x| per axis -> 4 * max(H, W) * 2^-24 * max|x|, and where floor(f) lands
# one cell off at a grid point the two evaluations differ by the same |df| * |slope|; the combination itself: 2 products, 2 fma, 1 product,
# 1 fma = 6 roundings  ->  k = 6 + 4 max(H, W) <= k_bilinear.  backward: the same weights (up_weight), at most 16 products and adds of
# wy * wx * dy whose weights sum to <= 4 per input pixel: A = 4 max|dy|, the adds and products stay under 8 roundings of A.
def upsample2x(x):
    N, H, W, C = x.shape
    return np.einsum("oh,pw,nhwc->nopc", up_matrix(H), up_matrix(W), f64(x), optimize=True)


def upsample2x_adjoint(dy):
    N, Ho, Wo, C = dy.shape
    return np.einsum("oh,pw,nopc->nhwc", up_matrix(Ho // 2), up_matrix(Wo // 2), f64(dy), optimize=True)


def upsample_mag(x, factor=1.0):
    """per-(sample, channel) maximum of |x| (times 4 for the adjoint), broadcastable against [N, *, *, C]"""
    return factor * np.abs(f64(x)).max(axis=(1, 2), keepdims=True)


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU
# gn_relu_fwd_kernel: mean / rstd from fp64 sums, rounded to fp32 (the tests hold mean_rstd to 1 ulp); y = max((x - mu) * rs * gm + bt, 0): sub, 2 products, add [4] + mu, rs rounded [2] -> r = 6, k = 12
K_GN_FWD = 12


# gn_relu_bwd_kernel.  Its sums are walks without a shuffle tree: a thread adds its ceil(HW / rpp) rows sequentially, the rpp row lanes are
# added sequentially out of LDS (sc[]), and only then do the paths part:
#   dbeta  = sum g:                    no term rounding; walk + lanes + one atomic add per sample           -> ceil(HW/rpp) + rpp + N
#   dgamma = sum g * (x - mu) * rs:    3 roundings per term on top                                           -> ceil(HW/rpp) + rpp + N + 3
#   A = mean_group(g * gamma):         sc[] (walk + lanes) * gamma [1], the cpg channels of the group added sequentially [cpg], * inv_m [inv_m: 1,
#                                      product: 1]                                                           -> ceil(HW/rpp) + rpp + cpg + 3
#   B = mean_group(g * gamma * xhat):  the same on terms with 3 roundings                                    -> ceil(HW/rpp) + rpp + cpg + 6
# (A = the sum of the |terms| in each case).  dx = rs * ((g*gm - A) - xh*B) is element-wise around A and B: xh = (x - mu) * rs [2], xh * B [1],
# g*gm [1], two differences [2], the outer product [1]; the longest path of one term (xh * B) collects 5  ->  r = 5, k = 10 of the whole
# magnitude, and A, B bring their own sum-type k on their own share of it, rs * |A| and rs * |xh| * |B| (gn_relu_bwd_shares)
K_GN_BWD_EW = 10


def k_gn_dbeta(HW, rpp, N):
    return -(-HW // rpp) + rpp + N


def k_gn_dgamma(HW, rpp, N):
    return k_gn_dbeta(HW, rpp, N) + 3


def k_gn_A(HW, rpp, cpg):
    return -(-HW // rpp) + rpp + cpg + 3


def k_gn_B(HW, rpp, cpg):
    return k_gn_A(HW, rpp, cpg) + 3


def gn_slab(C, G, V):
    """channels per workgroup of the GroupNorm kernels: 32 when groups and 16-byte vectors tile it, else all of C (the rule of csrc/norm.hip's
    host wrapper, restated once here: it fixes the row-lane count the k above depend on)"""
    cpg = C // G
    return 32 if (C % 32 == 0 and 32 % cpg == 0 and 32 % V == 0) else C


def gn_relu_fwd(x, gamma, beta, G, eps):
    """x [N,HW,C] -> y, mean [N,G], rstd [N,G]"""
    N, HW, C = x.shape
    xg = f64(x).reshape(N, HW, G, C // G)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    xh = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(N, HW, C)
    return np.maximum(xh * f64(gamma) + f64(beta), 0.0), mean, rstd


def gn_relu_fwd_mag(x, gamma, beta, mean, rstd, G):
    N, HW, C = x.shape
    mu, rs = np.repeat(np.abs(f64(mean)), C // G, axis=1)[:, None, :], np.repeat(f64(rstd), C // G, axis=1)[:, None, :]
    return (np.abs(f64(x)) + mu) * rs * np.abs(f64(gamma)) + np.abs(f64(beta))


def gn_relu_bwd(dy, y, x, gamma, mean, rstd, G, mag=False):
    """g = dy where the stored y > 0; dgamma = sum g*xhat, dbeta = sum g (over samples and pixels);
    dx = rstd * (g*gamma - mean_group(g*gamma) - xhat * mean_group(g*gamma*xhat)).  mag: the same on absolute values"""
    N, HW, C = x.shape
    cpg = C // G
    ab = np.abs if mag else (lambda v: v)
    g = np.where(f64(y) > 0.0, ab(f64(dy)), 0.0)
    mu, rs = np.repeat(f64(mean), cpg, axis=1)[:, None, :], np.repeat(f64(rstd), cpg, axis=1)[:, None, :]
    xh = (np.abs(f64(x)) + np.abs(mu)) * rs if mag else (f64(x) - mu) * rs
    gg = g * ab(f64(gamma))
    A = gg.reshape(N, HW, G, cpg).mean(axis=(1, 3))
    B = (gg * xh).reshape(N, HW, G, cpg).mean(axis=(1, 3))
    A, B = np.repeat(A, cpg, axis=1)[:, None, :], np.repeat(B, cpg, axis=1)[:, None, :]
    dx = rs * (gg + A + xh * B) if mag else rs * (gg - A - xh * B)
    return dx, (g * xh).sum((0, 1)), g.sum((0, 1))


def gn_relu_bwd_shares(dy, y, x, gamma, mean, rstd, G):
    """(rs * |A|, rs * |xh| * |B|) on absolute values: the shares of dx's magnitude that carry the sum-type error of A and of B"""
    N, HW, C = x.shape
    cpg = C // G
    g = np.where(f64(y) > 0.0, np.abs(f64(dy)), 0.0)
    mu, rs = np.repeat(f64(mean), cpg, axis=1)[:, None, :], np.repeat(f64(rstd), cpg, axis=1)[:, None, :]
    xh = (np.abs(f64(x)) + np.abs(mu)) * rs
    gg = g * np.abs(f64(gamma))
    A = np.repeat(gg.reshape(N, HW, G, cpg).mean(axis=(1, 3)), cpg, axis=1)[:, None, :]
    B = np.repeat((gg * xh).reshape(N, HW, G, cpg).mean(axis=(1, 3)), cpg, axis=1)[:, None, :]
    return np.broadcast_to(rs * A, xh.shape), rs * xh * B


def gn_dx_bound(dref, dmag, shA, shB, HW, rpp, cpg, u):
    return bound(dref, K_GN_BWD_EW * dmag + k_gn_A(HW, rpp, cpg) * shA + k_gn_B(HW, rpp, cpg) * shB, 1, u)


# ------------------------------------------------------------------------------------------------ misc
SLOPE = float(np.float32(0.1))   # the kernel's constant 0.1f
K_LEAKY = 2


def leaky_bwd(dy, y):
    """dx = dy where y > 0 (exactly), else 0.1f * dy [r = 1 -> k = 2, A = 0.1 |dy| there and 0 where dx = dy]"""
    return np.where(f64(y) > 0.0, f64(dy), SLOPE * f64(dy))


def k_bias(rows, rpp):
    """bias_grad_kernel: a thread walks <= 16 rows, the rpp row lanes meet in one LDS word, the workgroups (16 * rpp rows each below the re-grid)
    in one global word -- within k_sum of the walk for the strides the tests use"""
    return min(16, -(-rows // rpp)) + rpp + -(-rows // (16 * rpp))


def col_sums(a, C=None):
    a = f64(a)
    return a.reshape(-1, a.shape[-1])[:, :C].sum(0)


# ------------------------------------------------------------------------------------------------ storage formats and the seeded inputs
def store(a, kind):
    """the value a (finite) number has after storage in `kind` ("fp32" | "bf16" | "fp16"), round-to-nearest-even, as fp64"""
    a32 = np.asarray(a, dtype=np.float32)
    if kind == "fp32":
        return a32.astype(np.float64)
    if kind == "fp16":
        return a32.astype(np.float16).astype(np.float64)
    b = a32.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def operand(seed, shape, kind, std=1.0, offset=0.0):
    return store(np.random.default_rng(seed).standard_normal(shape) * std + offset, kind)


def levels(seed, shape, lo=-3, hi=3):
    """small integers (seven levels by default): exact in every storage type, ties are common"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def channel_consts(seed, C):
    """fp32 (scale, shift) of the BN apply / pool / mask cases: a quarter of the channels has a negative scale, channels 2 and 5 have scale exactly 0
    (one with a positive shift: every tap ties; one with a negative shift: every value is 0), channel 3 has a shift that makes every value
    negative (an all-zero pool window)"""
    r = np.random.default_rng(seed)
    scale = (0.5 + r.random(C)).astype(np.float32)
    shift = (r.random(C) - 0.5).astype(np.float32)
    scale[1::4] *= -1.0
    scale[2], shift[2] = 0.0, 0.25
    scale[5], shift[5] = 0.0, -0.25
    shift[3] = -64.0
    return scale, shift


def pow2_consts(seed, C):
    """regime (b): mean in {-1, 0, 1}, invstd and scale in {+-0.5, +-1, +-2}, shift in {-1, 0, 1} (fp32)"""
    r = np.random.default_rng(seed)
    pw = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], dtype=np.float32)
    return dict(mean=r.integers(-1, 2, C).astype(np.float32), invstd=pw[r.integers(0, 6, C)], scale=pw[r.integers(0, 6, C)],
                shift=r.integers(-1, 2, C).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the case tables (shared by the CPU and GPU files)
UP_HW = [(2, 2), (2, 9), (3, 5), (7, 8), (16, 16), (17, 31), (33, 15), (64, 65)]
UP_C = [8, 24, 256]                    # row kernel at its smallest channel-vector count, the generic kernel (3 or 6 vectors), row kernel
UP_LDS_SWITCH = {"bf16": [(4, 64), (4, 65)], "fp16": [(4, 64), (4, 65)], "fp32": [(4, 32), (4, 33)]}   # C = 256: 2*W*C*sizeof(T) = / > 64 KiB
POOL_HW = [(2, 2), (2, 6), (6, 10), (24, 24), (14, 30)]
POOL_C = [8, 64, 256, 512]               # (fp32: the row totals up to C = 256, 64 channel vectors; C = 512 is refused with rows)
BN_C = [8, 64, 256, 512]
GN_SLAB32 = [(128, 32, hw) for hw in (49, 511, 512, 513, 1023, 1024, 1025, 1600)]
GN_WHOLE = [(c, g, hw) for (c, g) in ((64, 1), (64, 2), (128, 2), (256, 1), (512, 4)) for hw in (36, 49, 100)]


def vec(kind):
    return 4 if kind == "fp32" else 8


def bn_npix(C, kind):
    """1, one short of a full pass of the workgroup's row lanes, and two odd sizes with a partial last workgroup"""
    rpp = 256 // (C // vec(kind))
    return sorted({1, max(1, rpp - 1), 433, 1283})


def pool_inputs(seed, N, H, W, C, kind, integer):
    """x of a pool case: real-valued, or seven integer levels (positive ties are common); (scale, shift) of channel_consts"""
    x = levels(seed, (N, H, W, C)) if integer else operand(seed, (N, H, W, C), kind, 1.5)
    return (x,) + channel_consts(seed + 1, C)
