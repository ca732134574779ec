"""fp64 yardstick of pose_loss_kernel (csrc/pose_loss.hip, entry point gdrn_pose_loss): the functions of oracle/gdrn_oracle.py
(ortho6d_to_mat_batch, pose_decode_train, pose_decode_test, get_closest_rot_batch and the loss_PM_R / loss_centroid / loss_z lines of
gdrn_loss) run in torch.float64 on the CPU on exactly the arrays gdrn_pose_params takes, their unit gradients by torch.autograd, and the
same oracle once more in torch.float32: the "reference at the kernel's precision" whose distance from the fp64 run (e32) sizes the
bounds of the decode-dependent outputs.  No device figure enters anything here; tests/test_pose_host_cpu.py pins this module on the CPU,
tests/test_pose_loss_gpu.py holds the kernel to it.

Inputs are a dict `a` of fp32 numpy arrays keyed like the struct: fc [N,fs], cams [N,3,3], centers [N,2], whs [N,2], ratios [N], extents [N,3],
gt_rot [N,3,3], gt_trans [N,3], gt_trans_ratio [N,3], points [N,npts,3], and optionally sym [N,Kmax,3,3] + sym_count [N] (int32; slots
behind a RoI's count are never read and hold NaN).

Bounds (derivations next to the functions):
  decode-dependent outputs (rot, trans, dfc[0])  err / rowmax <= 8 e32 + 16 * 2^-24         decode_bound(), check_decode()
  loss rows                                       fp32 summation of 3 npts terms + e32(R) w sum|p|   rows_bound()
  fc tail                                         f2_out bit-exact; fc_w <= (256 + 2) 2^-24 sum|a w|   fc_tail()
  signs, zeros, sentinels                         exact
"""
import math

import numpy as np
import torch

from oracle import bf16_emulation as E16
from oracle import gdrn_oracle as O

EPS32 = 2.0 ** -24
LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)   # LineMOD intrinsics (dataset constant)
ORIGIN_K = np.array([[572.4114, 0.0, 0.0], [0.0, 573.57043, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)           # principal point (0, 0): sub-ulp-of-325 offsets stay representable


def f64(x):
    return np.asarray(x, dtype=np.float64)


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ the reference
def _tensors(a, dtype):
    N = a["fc"].shape[0]
    T = lambda k: torch.from_numpy(np.ascontiguousarray(a[k])).to(dtype)   # (an fp64 array passes unrounded: the CPU module's central differences)
    return N, T, T("cams").view(N, 3, 3), T("centers"), T("whs"), T("ratios")


def _sym_list(a, N):
    if a.get("sym") is None or a.get("sym_count") is None:
        return [None] * N
    return [None if int(a["sym_count"][n]) == 0 else f64(a["sym"][n, :int(a["sym_count"][n])]) for n in range(N)]


def decode_test(a, dtype=torch.float64):
    """test mode (no eps, `if angle > 0`): rot [N,3,3], trans [N,3]"""
    N, T, cams, ctr, wh, rat = _tensors(a, dtype)
    fc9 = T("fc")[:, :9]
    R_allo = O.ortho6d_to_mat_batch(fc9[:, :6])
    rot, trans = O.pose_decode_test(R_allo, fc9[:, 6:9], cams, ctr, rat, wh)
    return dict(rot=f64(rot.numpy()), trans=f64(trans.numpy()), rot_allo=f64(R_allo.numpy()))


def reference(a, dtype=torch.float64):
    """train mode.  Returns fp64 numpy arrays:
    rot [N,3,3], trans [N,3], rot_allo; chosen [N,3,3] (the closest symmetric ground truth, as the fp32 value it is stored as), chosen_idx [N]
    (-1: the plain gt) and margin_deg [N] (runner-up minus best; inf without candidates); vis [N,2]; rows [N,3] (per RoI, already divided by
    N npts, 2 N, N) and losses [3] (the oracle's three lines); dfc [3,N,fs]; d [N,npts,3] = w (R p - G p); S [N,3,3] = d loss_PM_R / d rot,
    S_wave [4,N,3,3] (its split over the kernel's four waves: point i belongs to wave (i % 256) // 64) and J [N,9,9] = d rot_ab / d fc_k, so
    that dfc[0][n][k] = sum_ab S[n][ab] J[n][ab][k]."""
    N, T, cams, ctr, wh, rat = _tensors(a, dtype)
    fs = a["fc"].shape[1]
    fc9 = T("fc")[:, :9].clone().requires_grad_(True)
    R_allo = O.ortho6d_to_mat_batch(fc9[:, :6])
    rot, trans = O.pose_decode_train(R_allo, fc9[:, 6:9], cams, ctr, rat, wh)
    gt = T("gt_rot").view(N, 3, 3)
    syms = _sym_list(a, N)
    # the target is stored in fp32 by the reference (`.to(gt_rots.dtype)`) and by the kernel (sG): a value, not an error
    chosen = O.get_closest_rot_batch(rot, gt, syms).float().to(dtype)
    P, G = f64(rot.detach().numpy()), f64(gt.numpy())
    idx, margin = np.full(N, -1), np.full(N, np.inf)
    for n in range(N):
        if syms[n] is not None:
            errs = [O.re_deg(P[n], G[n])] + [O.re_deg(P[n], G[n].dot(S_)) for S_ in syms[n]]
            order = np.argsort(errs, kind="stable")
            idx[n], margin[n] = order[0] - 1, errs[order[1]] - errs[order[0]]
    pts = T("points")
    npts = pts.shape[1]
    w = (1.0 / T("extents").max(1, keepdim=True)[0]).view(-1, 1, 1)
    est = torch.matmul(rot[:, None], pts[..., None]).squeeze(-1)
    tgt = torch.matmul(chosen[:, None], pts[..., None]).squeeze(-1)
    d = w * est - w * tgt
    gtr = T("gt_trans_ratio")
    L = [3 * d.abs().mean(), (fc9[:, 6:8] - gtr[:, :2]).abs().mean(), (fc9[:, 8] - gtr[:, 2]).abs().mean()]   # gdrn_loss: loss_PM_R, loss_centroid, loss_z
    rows = torch.stack([d.abs().sum((1, 2)) / (N * npts), (fc9[:, 6:8] - gtr[:, :2]).abs().sum(1) / (2 * N), (fc9[:, 8] - gtr[:, 2]).abs() / N], 1)
    dfc = np.zeros((3, N, fs))
    for k in range(3):
        dfc[k, :, :9] = f64(torch.autograd.grad(L[k], fc9, retain_graph=True)[0].numpy())
    S = torch.autograd.grad(L[0], rot, retain_graph=True)[0]
    J = np.stack([f64(torch.autograd.grad(rot.reshape(N, 9)[:, ab].sum(), fc9, retain_graph=True)[0].numpy()) for ab in range(9)], 1)
    sg = torch.sign(d.detach()) * w / (N * npts)
    wave = (torch.arange(npts) % 256) // 64
    S_wave = np.stack([f64(torch.einsum("nia,nib->nab", sg[:, wave == v], pts[:, wave == v]).numpy()) for v in range(4)])
    te = (T("gt_trans") - trans).norm(dim=1)
    vis = np.stack([[O.re_deg(P[n], G[n]) for n in range(N)], f64(te.detach().numpy())], 1)
    out = dict(rot=rot, trans=trans, rot_allo=R_allo, chosen=chosen, rows=rows, losses=torch.stack(L), d=d, S=S)
    out = {k: f64(v.detach().numpy()) for k, v in out.items()}
    out.update(chosen_idx=idx, margin_deg=margin, vis=vis, dfc=dfc, J=J, S_wave=S_wave)
    return out


def both(a):
    """(fp64 reference, the same oracle in fp32)"""
    return reference(a, torch.float64), reference(a, torch.float32)


# ------------------------------------------------------------------------------------------------ decode-dependent outputs
# rot, trans and dfc[0] are conditioned by the decode (the `+ eps` norms of allo_to_ego close to the optical axis amplify an input rounding of
# 2^-24 by up to ~1e2): e32 = max over the case's RoIs and elements of |oracle_fp32 - oracle_fp64| / (the RoI row's largest fp64 magnitude) is one
# SAMPLE of that conditioning under fp32 rounding.  The kernel runs the same formulas in forward mode with the device's acosf / sinf / cosf:
# other roundings of the same conditioning, so it is held to 8 e32 plus 16 roundings of 2^-24 (a floor for cases where the fp32 oracle happens
# to land on the fp64 value).  Row = one RoI's 9 rotation entries / 3 translation entries / 9 gradient entries.
_ROWS = {"rot": lambda r: r["rot"].reshape(len(r["rot"]), 9), "trans": lambda r: r["trans"], "dfc0": lambda r: r["dfc"][0][:, :9]}


def rowmax(r64, key):
    m = np.abs(_ROWS[key](r64)).max(1, keepdims=True)
    return np.where(m > 0, m, 1.0)


def e32_of(r64, r32, key):
    return float((np.abs(_ROWS[key](r32) - _ROWS[key](r64)) / rowmax(r64, key)).max())


def decode_bound(e32):
    return 8.0 * e32 + 16.0 * EPS32


def check_decode(got, r64, r32, key):
    """got: [N, 9 or 3] (the kernel's rows, or a perturbed reference's).  Returns (ok, e32, worst normalised error); NaN is never ok."""
    e32 = e32_of(r64, r32, key)
    err = np.abs(f64(got).reshape(_ROWS[key](r64).shape) - _ROWS[key](r64)) / rowmax(r64, key)
    worst = float(np.nanmax(err)) if not np.isnan(err).all() else float("nan")
    return bool((err <= decode_bound(e32)).all()), e32, worst


# vis[:, 0] = acos(c) in degrees, c = (tr(P G^T) - 1) / 2 evaluated in fp64 from the kernel's fp32 rot P: |dc| <= 0.5 dR sum|G| for entries of
# P within dR of the reference's; |acos'| = 1 / sqrt(1 - c^2) is increasing in |c|, so over [c - dc, c + dc] it is at most its value at
# |c| + dc (mean value theorem); plus the final fp32 rounding.  vis[:, 1] = ||gt_trans - t||: three differences (one rounding each, of
# magnitude <= |gt| + |t|), squares, two adds, a square root (<= 5 roundings relative to the result) and the translation's own deviation dt.
def vis_bound(a, r64, dR, dt):
    G = f64(a["gt_rot"]).reshape(-1, 3, 3)
    c = np.clip(0.5 * (np.einsum("nij,nij->n", r64["rot"], G) - 1.0), -1.0, 1.0)
    dc = 0.5 * dR * np.abs(G).sum((1, 2))
    cm = np.minimum(np.abs(c) + dc, 1.0)
    with np.errstate(divide="ignore"):
        b0 = np.degrees(dc / np.sqrt(1.0 - cm * cm)) + EPS32 * r64["vis"][:, 0]
    mag = np.abs(f64(a["gt_trans"])) + np.abs(r64["trans"])
    b1 = math.sqrt(3.0) * (dt + EPS32 * mag.max(1)) + 5 * EPS32 * r64["vis"][:, 1]
    return np.stack([b0, b1], 1)


# ------------------------------------------------------------------------------------------------ the point loop: d = w e - w g
# e = R p and g = G p are three products and two adds each, every intermediate at most M_e = sum_b |R_ab| |p_b| (M_g likewise) in magnitude:
# <= 5 roundings of 2^-24 M (3 when the compiler fuses), the products w e and w g one more each: |fl(d) - d| <= 6 * 2^-24 * w (M_e + M_g) (the
# final subtraction rounds relative to d itself and cannot change its sign).  On top the kernel's R is its own fp32 decode: entries within dR of
# the reference's move d by at most w dR sum_b |p_b|.
def d_rounding(a, r64):
    p = np.abs(f64(a["points"]))
    w = (1.0 / f64(a["extents"]).max(1))[:, None, None]
    M = np.einsum("nab,nib->nia", np.abs(r64["rot"]), p) + np.einsum("nab,nib->nia", np.abs(r64["chosen"]), p)
    return 6 * EPS32 * w * M, w * p.sum(2, keepdims=True)


def sign_uncertain(a, r64, r32):
    """(RoI, point, axis) of the elements whose fp64 d is smaller in magnitude than what fp32 evaluation from a rot inside its own bound can
    move it by: their sign -- hence the sign sums and dfc[0] -- is not determined by the inputs"""
    rnd, wp = d_rounding(a, r64)
    dR = decode_bound(e32_of(r64, r32, "rot")) * rowmax(r64, "rot")[:, :, None]
    return np.argwhere(np.abs(r64["d"]) < rnd + dR * wp)


# loss row 0 of RoI n = inv * sum over the 3 npts terms |d|, inv = 1 / (N npts).  The kernel: a thread adds its ceil(npts / 256) * 3 terms in
# order, six shuffle levels, three wave adds, then the product with inv (itself two conversions and a division): a term passes through at most
# t = 3 ceil(npts / 256) + 6 + 3 + 3 roundings relative to a partial sum <= sum|d|, and carries its own evaluation error (d_rounding, plus one
# rounding of d itself); the propagated decode term is e32 of R (absolute) times w sum_b|p_b| per term.  Rows 1 and 2 are |x - g| (+ |y - h|) / (2 N)
# resp. / N from fp32 inputs: 5 resp. 3 roundings relative to the row.  A total over the N rows adds N - 1 fp32 atomic adds.
def rows_bound(a, r64, r32):
    N, npts = a["points"].shape[:2]
    rnd, wp = d_rounding(a, r64)
    absd = np.abs(r64["d"])
    t = 3 * (-(-npts // 256)) + 12
    eR = e32_of(r64, r32, "rot") * rowmax(r64, "rot")[:, :, None]
    b0 = (t * EPS32 * absd.sum((1, 2)) + (rnd + EPS32 * absd).sum((1, 2)) + (eR * wp * np.ones((1, 1, 3))).sum((1, 2))) / (N * npts)
    return np.stack([b0, 5 * EPS32 * r64["rows"][:, 1], 3 * EPS32 * r64["rows"][:, 2]], 1)


def totals_bound(a, r64, r32):
    N = a["points"].shape[0]
    return rows_bound(a, r64, r32).sum(0) + (N - 1) * EPS32 * np.abs(r64["rows"]).sum(0)


# ------------------------------------------------------------------------------------------------ the fc tail
def round16(x, kind):
    """fp32 -> the build's 16-bit storage format -> fp32 (round to nearest even)"""
    t = torch.from_numpy(f32(x))
    return (t.to(torch.float16).float() if kind == "fp16" else E16.r(t)).numpy()


def fc_tail(ws, bias, w_rt, b_rt, kind):
    """ws [splits,N,256] fp32, bias [256], w_rt [9,256] (values exact in the 16-bit format), b_rt [9].  Every step of the finish pass is a single
    IEEE fp32 operation in a stated order (the slabs in order onto 0, + bias, the LeakyReLU product with 0.1f), so numpy's float32 replays it bit
    for bit: f2_out [N,256] as stored.  fc_w = 256 products of the stored activation with w_rt added up in fp32 in some order, + b_rt: the fp64
    value and the bound (256 + 2) 2^-24 sum|a w| (255 adds, the product, the bias add)."""
    ws, bias = f32(ws), f32(bias)
    v = np.zeros(ws.shape[1:], dtype=np.float32)
    for sp in range(ws.shape[0]):
        v = (v + ws[sp]).astype(np.float32)
    v = (v + bias[None]).astype(np.float32)
    pre = v
    v = np.where(v > 0, v, (np.float32(0.1) * v).astype(np.float32)).astype(np.float32)
    f2 = round16(v, kind)
    prod = f64(f2)[:, None, :] * f64(w_rt)[None]
    return dict(pre=pre, f2=f2, fc=prod.sum(2) + f64(b_rt)[None], fc_bound=(256 + 2) * EPS32 * np.abs(prod).sum(2))


# ------------------------------------------------------------------------------------------------ seeded inputs (shared by the CPU and the GPU module)
def rotations(rg, n):
    q, r = np.linalg.qr(rg.standard_normal((n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    return q * np.linalg.det(q)[:, None, None]


def rot_axis(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def make_inputs(seed, N, fs, npts, K=LM_K):
    """a generic batch: RoIs of 60..180 px around the image centre, objects of 5..30 cm, points inside the extents, z_rel around 1"""
    rg = np.random.default_rng(seed)
    a = {}
    fc = np.zeros((N, fs))
    fc[:, :6] = rg.standard_normal((N, 6))
    fc[:, 6:8] = 0.3 * rg.standard_normal((N, 2))
    fc[:, 8] = 1.0 + 0.25 * (2 * rg.random(N) - 1)
    fc[:, 9:] = rg.standard_normal((N, fs - 9))          # (entries the kernel must not read)
    scale = 60.0 + 120.0 * rg.random(N)
    a["fc"], a["cams"] = f32(fc), f32(np.repeat(K[None], N, 0))
    a["centers"] = f32(K[:2, 2][None] + 120.0 * (rg.random((N, 2)) - 0.5))
    a["whs"] = f32(scale[:, None] * (0.7 + 0.3 * rg.random((N, 2))))
    a["ratios"] = f32(64.0 / scale)
    a["extents"] = f32(0.05 + 0.25 * rg.random((N, 3)))
    a["gt_rot"] = f32(rotations(rg, N))
    a["gt_trans"] = f32(np.concatenate([0.2 * (rg.random((N, 2)) - 0.5), 0.4 + rg.random((N, 1))], 1))
    a["gt_trans_ratio"] = f32(fc[:, 6:9] + 0.2 * rg.standard_normal((N, 3)))
    a["points"] = f32((rg.random((N, npts, 3)) - 0.5) * a["extents"][:, None, :])
    return a


GENERIC_FS = (9, 12, 64, 256)
GENERIC_NPTS = (1, 63, 65, 256, 257, 700)
AXIS_OFFSETS = (0.0, 1e-5, 1e-3, 0.1, 1.0, 30.0)
AXIS_Z = (0.3, 1.5)


RESEED = {(9, 700): 1, (256, 700): 1}    # cases whose first seed drew an element within rounding of d = 0 (tests/test_pose_host_cpu.py asserts none is left)


def generic(fs, npts, N=5):
    return make_inputs(1000 + 7 * fs + npts + 100000 * N + 1000000 * RESEED.get((fs, npts), 0), N, fs, npts)


def optical_axis(z, K=LM_K):
    """one RoI per offset: t_(cx, cy) = 0 and center = (px, py) + offset, so the object sits `offset` pixels off the optical axis (both
    coordinates).  With the LineMOD principal point (325.26, 242.05) the fp32 `center` cannot hold 1e-5 px (its ulp there is 3e-5): that RoI
    coincides with offset 0; ORIGIN_K (principal point 0) keeps every offset."""
    offs = AXIS_OFFSETS + (0.0,)
    a = make_inputs(2000 + int(10 * z) + (0 if K is LM_K else 1), len(offs), 64, 65, K)
    a["fc"][:, 6:8] = 0.0
    a["fc"][:, 8] = z
    a["fc"][AXIS_EXACT_ROI, :6] = [0.0, 2.0, 0.0, 0.0, 0.0, -3.0]
    a["ratios"][:] = 1.0
    a["centers"] = f32(f64(K[:2, 2])[None] + f64(offs)[:, None])
    return a


# the last RoI of optical_axis(): on the axis with a1 = (0, 2, 0), a2 = (0, 0, -3): x = (0, 1, 0), x x a2 = (-3, 0, 0), z = (-1, 0, 0), y = z x x =
# (0, 0, -1) without a rounding; columns (x, y, z)
AXIS_EXACT_ROI = len(AXIS_OFFSETS)
AXIS_EXACT_ALLO = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def degenerate_rot6d():
    """RoI 0: a1 = 0 (x = 0 / eps, the cross products vanish).  RoI 1, 2: a2 parallel / antiparallel to an axis-aligned a1: both crosses are
    exactly zero in fp32 and fp64.  RoI 3: generic, next to them in one batch."""
    a = make_inputs(3000, 4, 64, 65)
    a["fc"][0, :3] = 0.0
    a["fc"][1, :6] = [2.0, 0.0, 0.0, 3.0, 0.0, 0.0]
    a["fc"][2, :6] = [0.0, -1.5, 0.0, 0.0, 0.5, 0.0]
    return a


def sign_edges(k):
    """fc[k] bit-equal to its regression target for every RoI (k in 6, 7, 8)"""
    a = make_inputs(4000 + k, 3, 64, 65)
    a["gt_trans_ratio"][:, k - 6] = a["fc"][:, k]
    return a


def exact_match_first():
    """the first launch of the exact-match case; the second feeds the returned rot back as gt_rot"""
    return make_inputs(5000, 3, 64, 700)


SYM_COUNT = (0, 1, 3, 2)
SYM_CHOICE = (-1, 0, 1, -1)    # index of the closest candidate per RoI (-1: the plain gt)


def symmetry():
    """sym_count = {0, 1, Kmax = 3, 2}: RoI 1 and 2 are closest to a non-identity symmetry (gt = pred * D * S^-1 with D a 10 degree turn), RoI 3
    has two symmetries and is closest to its plain gt; unused slots hold NaN"""
    a = make_inputs(6000, 4, 64, 257)
    P = reference(a)["rot"]
    D = rot_axis(0, 10.0)
    sets = [[], [rot_axis(2, 180)], [rot_axis(2, 90), rot_axis(2, 180), rot_axis(2, 270)], [rot_axis(2, 180), rot_axis(0, 180)]]
    sym = np.full((4, 3, 3, 3), np.nan)
    gt = f64(a["gt_rot"]).copy()
    for n, (ss, ch) in enumerate(zip(sets, SYM_CHOICE)):
        for k, S_ in enumerate(ss):
            sym[n, k] = S_
        if ss:
            gt[n] = P[n].dot(D) if ch < 0 else P[n].dot(D).dot(ss[ch].T)
    a["gt_rot"], a["sym"], a["sym_count"] = f32(gt), f32(sym), np.array(SYM_COUNT, dtype=np.int32)
    return a


def fc_tail_inputs(splits, N=3, fs=64, kind="bf16"):
    """slabs whose sum + bias is negative, exactly zero (channels 0..15) and positive; w_rt exact in the 16-bit format; the nine outputs are a
    usable pose input (z_rel around 1 through b_rt)"""
    rg = np.random.default_rng(7000 + splits)
    ws = (rg.integers(-64, 65, (splits, N, 256)) / 64.0).astype(np.float32) + f32(0.01 * rg.standard_normal((splits, N, 256)))
    bias = f32(0.1 * rg.standard_normal(256))
    ws[:, :, :16] = (rg.integers(-64, 65, (splits, N, 16)) / 64.0).astype(np.float32)    # dyadic: every partial sum of these channels is exact
    part = np.zeros((N, 256), dtype=np.float32)
    for sp in range(splits - 1):
        part = (part + ws[sp]).astype(np.float32)
    bias[:16] = (rg.integers(-8, 9, 16) / 16.0).astype(np.float32)
    ws[splits - 1, :, :16] = (-(part[:, :16] + bias[None, :16])).astype(np.float32) if splits > 1 else -bias[None, :16]
    w_rt = round16(0.02 * rg.standard_normal((9, 256)), kind)
    b_rt = f32([0.3, -0.2, 0.5, 0.1, 0.6, -0.4, 0.05, -0.03, 1.1])
    return dict(ws=ws, bias=bias, w_rt=w_rt, b_rt=b_rt)


def seeded_cases():
    """name -> inputs of every train-mode launch of the GPU module on seeded data (the second exact-match launch takes a device output and is
    sign-uncertain on purpose)"""
    c = {}
    for fs in GENERIC_FS:
        for npts in GENERIC_NPTS:
            c[f"generic fs{fs} npts{npts}"] = generic(fs, npts)
    c["generic N1"], c["generic N8"] = generic(64, 257, 1), generic(64, 257, 8)
    for z in AXIS_Z:
        c[f"axis z{z} lm"], c[f"axis z{z} origin"] = optical_axis(z, LM_K), optical_axis(z, ORIGIN_K)
    c["degenerate"] = degenerate_rot6d()
    for k in (6, 7, 8):
        c[f"sign fc{k}"] = sign_edges(k)
    c["exact first"], c["symmetry"] = exact_match_first(), symmetry()
    return c
