"""GPU tests of the hypothesis verification (csrc/verify.hip through gdrnet_amd.verify) against the host restatement tests/verify_host.py.

The counts are integers and the score is one fixed fp64 operation sequence, so every comparison with the restatement is bitwise (float bits
through an int64 view, so that -inf and signed zeros count): on hand-made maps that put the class boundaries, the unusable observations, the
coverage threshold and the empty union where the pass can go wrong, at the edges of the launch shape, inside guard bands, and on the device's
own renders."""
import numpy as np
import pytest
import torch

import verify_host as VH
from gdrnet_amd import cabi, devargs, render, synth, verify

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = np.float32(0.1)
TAU = float(np.float32(0.2))           # == 2 C exactly: a difference can EQUAL tau
MIN_COVERED = 64
KEYS = VH.KEYS
MASK_MM = 1.5


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    """an integer view that compares NaNs, infinities and signed zeros bit by bit"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _tbits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _host_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _assert_equal(got, ref, what, keys=KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and np.array_equal(_bits(got[k]), _bits(ref[k])), (what, k, got[k], ref[k])


def _make_maps():
    """N = 9 candidates in F = 2 frames of 37 x 53 (1961 pixels: no multiple of 64 or 256, W no multiple of 4) with M = 6 masks:
    dict(ren, frames, frame, masks, mask_index)"""
    N, F, M, H, W = 9, 2, 6, 37, 53
    u = lambda tag, *s: synth.hash_uniform(411, tag, s)  # noqa: E731
    mult = lambda k: (np.asarray(k, dtype=np.float32) * C).astype(np.float32)  # noqa: E731   fp32 multiples of C
    idx = np.arange(H * W).reshape(H, W)
    frames = np.zeros((F, H, W), dtype=np.float32)
    frames[0] = mult(4 + np.floor(8 * u("f0", H, W)))                     # 4 C .. 11 C
    bad = u("bad0", H, W)
    frames[0][bad < 0.03] = 0.0
    frames[0][(bad >= 0.03) & (bad < 0.06)] = np.nan
    frames[0][(bad >= 0.06) & (bad < 0.09)] = np.inf
    frames[0][(bad >= 0.09) & (bad < 0.12)] = -C
    frames[1] = np.choose(idx % 4, [2 * C, C, 4 * C, 2 * C])
    usable0 = np.isfinite(frames[0]) & (frames[0] > 0)
    ren = np.zeros((N, H, W), dtype=np.float32)
    masks = np.zeros((M, H, W), dtype=np.uint8)
    frame = np.array([0, 1, 0, 0, 1, 1, 0, 1, 1])
    mask_index = np.array([0, 1, 2, 3, 4, 1, 5, 5, 4])                    # rows 1 and 5, 6 and 7, 4 and 8 share a mask; mask 4 is empty
    # row 0: hashed renders 3 C .. 12 C over hashed observations: every class, holes, NaN renders, the last row and column covered
    ren[0] = mult(3 + np.floor(10 * u("r0", H, W)))
    hole = u("hole0", H, W)
    ren[0][hole < 0.2] = 0.0
    ren[0][(hole >= 0.2) & (hole < 0.23)] = np.nan
    ren[0][-1, -1], ren[0][-1, 0], ren[0][0, -1] = frames[1][-1, -1], C, C
    masks[0] = 255 * (u("m0", H, W) < 0.5)
    masks[0][-1, -1] = 1
    # row 1: the boundaries.  Under 4 C: 2 C (e = -tau, an inlier) and the float below 2 C (violated); under 2 C: 4 C (e = +tau, an inlier) and
    # the float above 4 C (occluded); 100 more inliers of e = -C, 30 of e = +C
    two_c, four_c = np.float32(2 * C), np.float32(4 * C)
    flat = ren[1].reshape(-1)
    flat[2], flat[6] = two_c, np.nextafter(two_c, np.float32(0))
    flat[4], flat[8] = four_c, np.nextafter(four_c, np.float32(1))
    flat[np.arange(102, 502, 4)] = np.float32(3 * C)                       # under 4 C: e = 3 C - 4 C
    flat[np.arange(1001, 1121, 4)] = two_c                                 # under C: e = +C
    masks[1] = 3 * (u("m1", H, W) < 0.3)
    # rows 2 and 3: exactly MIN_COVERED and MIN_COVERED - 1 covered pixels, inliers of hashed residuals, in the mask and out of it
    for row, count in ((2, MIN_COVERED), (3, MIN_COVERED - 1)):
        ys, xs = np.nonzero(usable0)
        pick = np.argsort(u(f"pick{row}", len(ys)))[:count]
        d = 0.3 * (u(f"d{row}", count) - 0.5)
        ren[row, ys[pick], xs[pick]] = (frames[0, ys[pick], xs[pick]].astype(np.float64) + d).astype(np.float32)
        masks[row] = ren[row] > 0
        masks[row][u(f"m{row}", H, W) < 0.1] ^= 1
    # row 4: an empty render under the empty mask: the union is 0
    # row 5: every inlier at |e| == tau: 4 C over 2 C and 2 C under 4 C; the fit is what floor leaves of it
    flat = ren[5].reshape(-1)
    flat[np.arange(0, 800, 4)] = four_c
    flat[np.arange(2, 802, 4)] = two_c
    # rows 6 and 7: hashed renders in either frame under one mask
    ren[6] = mult(3 + np.floor(10 * u("r6", H, W)))
    ren[6][u("hole6", H, W) < 0.6] = 0.0
    ren[7] = mult(1 + np.floor(5 * u("r7", H, W)))
    ren[7][u("hole7", H, W) < 0.4] = 0.0
    masks[5] = u("m5", H, W) < 0.4
    # row 8: covered and occluded everywhere under the empty mask: ok, and the union is 0
    ren[8][5:20, 7:40] = np.float32(8 * C)
    return dict(ren=ren, frames=frames, frame=frame, masks=masks, mask_index=mask_index, N=N, F=F, M=M, H=H, W=W)


@pytest.fixture(scope="module")
def maps():
    return _make_maps()


@pytest.fixture(scope="module")
def restated(maps):
    """the restatement of the hand-made maps with and without the masks, computed once"""
    return {True: VH.verify(maps["ren"], maps["frames"], maps["frame"], maps["masks"], maps["mask_index"], TAU, 1.0, MIN_COVERED),
            False: VH.verify(maps["ren"], maps["frames"], maps["frame"], None, None, TAU, 1.0, MIN_COVERED)}


def _device_maps(maps, with_mask, rows=None, **kw):
    r = np.arange(maps["N"]) if rows is None else np.asarray(rows)
    m = (_dev(maps["masks"]), maps["mask_index"][r]) if with_mask else (None, None)
    kw = dict(dict(tau=TAU, penalty=1.0, min_covered=MIN_COVERED), **kw)
    return _host_np(verify.verify_maps(_dev(maps["ren"][r]), _dev(maps["frames"]), maps["frame"][r], *m, **kw))


def test_the_maps_are_what_they_are_meant_to_be(maps, restated):
    ren, frames, masks, ref = maps["ren"], maps["frames"], maps["masks"], restated[True]
    cls = [VH.classify(ren[i], frames[maps["frame"][i]], TAU) for i in range(maps["N"])]
    for k in ("inlier", "occluded", "violated", "unknown", "mask_px", "inter"):
        assert ref[k][0] > 20, k
    f0, c0 = frames[0], cls[0]
    for unusable in (f0 == 0, np.isnan(f0), np.isinf(f0), f0 < 0):
        assert (unusable & c0["covered"]).any() and not (unusable & (c0["inlier"] | c0["occluded"] | c0["violated"])).any()
    assert np.isnan(ren[0]).any() and not c0["covered"][np.isnan(ren[0]) | (ren[0] == 0)].any()
    assert c0["covered"][-1].any() and c0["covered"][:, -1].any() and c0["covered"][-1, -1] and masks[0][-1, -1]
    assert ((masks[0] != 0) & c0["covered"]).any() and ((masks[0] != 0) & ~c0["covered"]).any() and ((masks[0] == 0) & c0["covered"]).any()
    e1 = cls[1]["e"].reshape(-1)
    inl, occ, vio = (cls[1][k].reshape(-1) for k in ("inlier", "occluded", "violated"))
    assert e1[2] == -TAU and inl[2] and e1[4] == TAU and inl[4] and e1[6] < -TAU and vio[6] and e1[8] > TAU and occ[8]
    assert list(ref[k][1] for k in ("covered", "inlier", "occluded", "violated", "unknown")) == [134, 132, 1, 1, 0]
    assert ref["covered"][2] == MIN_COVERED and ref["ok"][2] == 1 and ref["covered"][3] == MIN_COVERED - 1 and ref["ok"][3] == 0
    assert ref["score"][3] == -np.inf and ref["inlier"][2] == MIN_COVERED and 0 < ref["inter"][2] < ref["mask_px"][2]
    assert ref["covered"][4] == 0 and ref["mask_px"][4] == 0 and ref["ok"][4] == 0 and ref["score"][4] == -np.inf
    n5 = ref["inlier"][5]
    assert n5 == 400 == ref["covered"][5] and ref["sum_q"][5] == n5 * int(np.floor(TAU * 2.0 ** 20)) and 0.0 < ref["score"][5] < 1e-5
    assert np.all(np.abs(cls[5]["e"][cls[5]["inlier"]]) == TAU)
    assert ref["covered"][8] == ref["occluded"][8] > MIN_COVERED and ref["visible"][8] == 0 and ref["mask_px"][8] == 0 and ref["ok"][8] == 1
    assert _bits(ref["score"][8:9])[0] == 0                                # +0.0: an empty union and no evidence
    assert np.array_equal(ref["mask_px"][[1, 6, 4]], ref["mask_px"][[5, 7, 8]]) and ref["mask_px"][6] > 500
    assert list(ref["ok"]) == [1, 1, 1, 0, 0, 1, 1, 1, 1]
    assert not restated[False]["mask_px"].any() and not restated[False]["inter"].any()


@pytest.mark.parametrize("with_mask", (True, False))
def test_counts_and_scores_on_hand_made_maps_equal_the_restatement_bitwise(maps, restated, with_mask):
    got = _device_maps(maps, with_mask)
    ref = restated[with_mask]
    for i in range(maps["N"]):
        print(f"row {i}: " + ", ".join(f"{k} {got[k][i]}" for k in KEYS) + f" (host score {ref['score'][i]!r})")
    _assert_equal(got, ref, f"maps, mask {with_mask}")
    # other scalars move the decisions
    kw = dict(tau=0.05, penalty=0.25, min_covered=135)
    got = _device_maps(maps, with_mask, **kw)
    m = (maps["masks"], maps["mask_index"]) if with_mask else (None, None)
    _assert_equal(got, VH.verify(maps["ren"], maps["frames"], maps["frame"], *m, **kw), f"maps, mask {with_mask}, other scalars")
    assert got["ok"][1] == 0 and got["ok"][0] == 1 and got["inlier"][5] == 0


def _hashed_case(N, H, W):
    u = lambda tag, *s: synth.hash_uniform(412, f"{tag}/{N}x{H}x{W}", s)  # noqa: E731
    frames = ((4 + np.floor(8 * u("f", 2, H, W))).astype(np.float32) * C).astype(np.float32)
    frames[u("fbad", 2, H, W) < 0.1] = 0.0
    ren = ((3 + np.floor(10 * u("r", N, H, W))).astype(np.float32) * C).astype(np.float32)
    ren[u("hole", N, H, W) < 0.3] = 0.0
    ren[:, -1, -1] = frames[0, -1, -1] if frames[0, -1, -1] > 0 else C     # the last pixel is covered
    masks = (u("m", N, H, W) < 0.5).astype(np.uint8)
    return ren, frames, np.arange(N) % 2, masks


@pytest.mark.parametrize("shape", ((2, 16, 3), (2, 3, 3), (2, 2, 9), (1, 1, 1), (3, 35, 64), (2, 61, 71)))
def test_launch_edges(shape):
    """one pixel, fewer pixels than a wave, than a workgroup's chunk (2048), just more than one chunk (35 x 64 = 2240) and three chunks"""
    ren, frames, frame, masks = _hashed_case(*shape)
    for with_mask in (True, False):
        m = masks if with_mask else None
        got = _host_np(verify.verify_maps(_dev(ren), _dev(frames), frame, None if m is None else _dev(m), tau=TAU, min_covered=1))
        ref = VH.verify(ren, frames, frame, m, None, TAU, 1.0, 1)
        _assert_equal(got, ref, (shape, with_mask))
        assert ref["covered"].min() >= 1 and (shape[1] * shape[2] < 10 or ref["inlier"].sum() > 0)


def test_calls_are_deterministic_and_rows_independent(maps, restated):
    a = _device_maps(maps, True)
    b = _device_maps(maps, True)
    _assert_equal(a, b, "twice")
    perm = np.array([3, 6, 0, 8, 5, 1, 4, 7, 2])
    _assert_equal(_device_maps(maps, True, perm), {k: a[k][perm] for k in KEYS}, "permuted")
    sub = np.array([7, 1, 5])
    _assert_equal(_device_maps(maps, True, sub), {k: a[k][sub] for k in KEYS}, "a subset")
    _assert_equal(_device_maps(maps, False, sub), {k: restated[False][k][sub] for k in KEYS}, "a subset without masks")
    for i in (0, 4):
        _assert_equal(_device_maps(maps, True, [i]), {k: a[k][i : i + 1] for k in KEYS}, f"row {i} alone")


def _selection_case():
    n = 700
    u = lambda tag: synth.hash_uniform(413, tag, (n,))  # noqa: E731
    group = np.array([0] * 300 + [1] + [2] * 50 + [3] * 249 + [4] * 100)[np.argsort(u("perm"))]
    for row in (17, 400):                                                   # both in group 3: swap with a row that is
        if group[row] != 3:
            other = [k for k in np.nonzero(group == 3)[0] if k not in (17, 400)][0]
            group[other], group[row] = group[row], 3
    score = 0.9 * u("score")
    ok = np.ones(n, dtype=np.int32)
    score[[17, 400]] = 0.95                                                 # the tie at the top of group 3
    score[group == 4] = -0.1 - u("neg")[group == 4]
    ok[group == 2] = 0
    g0 = np.nonzero(group == 0)[0]
    score[g0[5]], ok[g0[5]] = 2.0, 0                                        # the highest score of group 0 is not ok
    score[g0[-3]] = np.nan                                                  # a NaN is never picked
    return score, ok, group.astype(np.int64)


def test_selection_equals_the_restatement_and_breaks_ties_to_the_lowest_row():
    score, ok, group = _selection_case()
    assert np.any(np.diff(group) < 0) and (group == 0).sum() == 300 and (group == 1).sum() == 1 and group[17] == group[400] == 3
    g0 = np.nonzero(group == 0)[0]
    assert g0.max() - g0.min() > 256                                        # the group crosses a workgroup of 256 rows
    got = _host_np(verify.select_best(_dev(score), _dev(ok), group, 5))
    best, best_score = VH.select(score, ok, group, 5)
    assert got["best"].dtype == np.int32 and got["best_score"].dtype == np.float64
    assert np.array_equal(got["best"], best) and np.array_equal(_bits(got["best_score"]), _bits(best_score))
    assert best[1] == np.nonzero(group == 1)[0][0] and best[2] == -1 and best_score[2] == -np.inf and best[3] == 17 and best_score[3] == 0.95
    assert best_score[4] < 0 and group[best[4]] == 4 and ok[best[0]] == 1 and best_score[0] < 0.9
    again = _host_np(verify.select_best(_dev(score), _dev(ok), _dev(group), 5))   # the groups from the device
    assert np.array_equal(again["best"], best) and np.array_equal(_bits(again["best_score"]), _bits(best_score))
    none = _host_np(verify.select_best(_dev(score[:0]), _dev(ok[:0]), [], 3))
    assert list(none["best"]) == [-1] * 3 and np.all(none["best_score"] == -np.inf)


def test_nothing_is_written_outside_the_outputs(maps):
    """the three entry points on buffers with a guard band on both sides, filled with a sentinel: the bands are unchanged, the payload is the
    wrapper's, and what the workspace held before the call does not matter"""
    lib, G = cabi.load(), 64
    stream = devargs.stream(torch.device(DEV))

    def banded(n, dtype, fill):
        return torch.full((G + n + G,), fill, dtype=dtype, device=DEV)

    def intact(bufs, fills, what):
        torch.cuda.synchronize()
        for k, b in bufs.items():
            f = torch.full((G,), fills[k], dtype=b.dtype, device=DEV)
            assert torch.equal(_tbits(b[:G]), _tbits(f)) and torch.equal(_tbits(b[-G:]), _tbits(f)), (what, k)

    N, F, M, H, W = (maps[k] for k in ("N", "F", "M", "H", "W"))
    ren, frames, masks = _dev(maps["ren"]), _dev(maps["frames"]), _dev(maps["masks"])
    fr_host, mi_host = maps["frame"].astype(np.int32), maps["mask_index"].astype(np.int32)
    fr, mi = _dev(fr_host), _dev(mi_host)
    want = _host_np(verify.verify_maps(ren, frames, fr_host, masks, mi_host, tau=TAU, penalty=1.0, min_covered=MIN_COVERED))
    ws_bytes = int(lib.gdrn_verify_workspace_bytes(N, H, W))
    assert ws_bytes == N * 32
    for ws_fill in (float("nan"), -7.25, 0.0):
        fills = dict(counts=-77, sum_q=-77, score=-7.25, ok=-77, ws=ws_fill)
        bufs = dict(counts=banded(N * 8, torch.int32, -77), sum_q=banded(N, torch.int64, -77), score=banded(N, torch.float64, -7.25),
                    ok=banded(N, torch.int32, -77), ws=banded(ws_bytes // 8, torch.float64, ws_fill))
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        cabi.check(lib.gdrn_verify_maps(ren.data_ptr(), frames.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, masks.data_ptr(), mi.data_ptr(),
                                        mi_host.ctypes.data, M, N, H, W, TAU, ptr["counts"], ptr["sum_q"], ptr["ws"], stream), "verify_maps")
        cabi.check(lib.gdrn_verify_score(ptr["counts"], ptr["sum_q"], N, 1, TAU, 1.0, MIN_COVERED, ptr["score"], ptr["ok"], stream), "verify_score")
        intact(bufs, fills, "maps and score")
        counts = bufs["counts"][G:-G].view(N, 8).cpu().numpy()
        got = {k: np.ascontiguousarray(counts[:, j]) for j, k in enumerate(VH.COUNTS)}
        got.update({k: bufs[k][G:-G].cpu().numpy() for k in ("sum_q", "score", "ok")})
        _assert_equal(got, want, f"workspace of {ws_fill}")
    score, ok, group = _selection_case()
    want = _host_np(verify.select_best(_dev(score), _dev(ok), group, 5))
    gr_host = group.astype(np.int32)
    s_dev, ok_dev, gr = _dev(score), _dev(ok), _dev(gr_host)
    for fill in (-7.25, float("nan")):
        fills = dict(best=-77, best_score=fill)
        bufs = dict(best=banded(5, torch.int32, -77), best_score=banded(5, torch.float64, fill))
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        cabi.check(lib.gdrn_verify_select(s_dev.data_ptr(), ok_dev.data_ptr(), gr.data_ptr(), gr_host.ctypes.data, len(score), 5, ptr["best"],
                                          ptr["best_score"], stream), "verify_select")
        intact(bufs, fills, "select")
        assert np.array_equal(bufs["best"][G:-G].cpu().numpy(), want["best"])
        assert np.array_equal(_bits(bufs["best_score"][G:-G].cpu().numpy()), _bits(want["best_score"]))


def _along(t, mm):
    """the translation moved so that its depth grows by ``mm`` millimetres and the model origin keeps its image"""
    return t * (1.0 + 1e-3 * mm / t[2])


class Scene:
    """a synth.make_refine_inputs scene on the device: the mesh table, the frames composed from the device's own renders of the ground truth,
    the mask of every ground truth (its render within MASK_MM of the frame) and, per ground truth as a detection, seven candidates: one of the
    fixture's starts, the ground truth 8 mm nearer, the ground truth itself, then +8, -30, +30 mm along its ray and 10 mm along camera x"""

    GT = 2   # the ground truth's place among the candidates

    def __init__(self, inp):
        self.inp, self.H, self.W = inp, inp["H"], inp["W"]
        self.meshes = render.MeshTable(inp["vertices"], inp["faces"])
        G = self.M = len(inp["gt_labels"])
        K_of = {int(g): inp["K"][i] for i, g in enumerate(inp["target"])}
        self.K = np.stack([K_of.get(g, inp["K"][0]) for g in range(G)])
        self.labels, self.frame = inp["gt_labels"], inp["gt_frame"]
        gt = self.render(inp["R_gt"], inp["t_gt"]).cpu().numpy()
        self.frames = synth.refine_scene(inp, gt)
        self.frames_dev = _dev(self.frames)
        obs = self.frames[self.frame].astype(np.float64)
        self.masks = ((gt > 0) & (np.abs(gt.astype(np.float64) - obs) <= 1e-3 * MASK_MM)).astype(np.uint8)
        start = [int(np.nonzero(inp["target"] == g)[0][0]) for g in range(G)]
        R_gt, t_gt = inp["R_gt"], inp["t_gt"]
        moved = lambda mm: np.stack([_along(t, mm) for t in t_gt])  # noqa: E731
        self.candidates = [(inp["R0"][start], inp["t0"][start]), (R_gt, moved(-8.0)), (R_gt, t_gt), (R_gt, moved(8.0)), (R_gt, moved(-30.0)),
                           (R_gt, moved(30.0)), (R_gt, t_gt + np.array([0.010, 0.0, 0.0]))]

    def render(self, R, t, rows=None):
        r = np.arange(self.M) if rows is None else rows
        return render.render_depth(self.meshes, self.labels[r], _dev(R), _dev(t), _dev(self.K[r]), self.H, self.W, self.inp["near"], self.inp["far"])

    def kw(self):
        return dict(near=self.inp["near"], far=self.inp["far"])


@pytest.fixture(scope="module")
def scenes():
    out = {"mixed": Scene(synth.make_refine_inputs("mixed"))}
    for inp in synth.make_refine_inputs("noisy"):
        out[inp["case"]] = Scene(inp)
    return out


def test_verify_poses_is_render_depth_then_verify_maps_bit_for_bit(scenes):
    for name, sc in scenes.items():
        Cn, M = len(sc.candidates), sc.M
        R = np.concatenate([c[0] for c in sc.candidates])
        t = np.concatenate([c[1] for c in sc.candidates])
        det = np.tile(np.arange(M), Cn)
        R_dev, t_dev = _dev(R), _dev(t)
        for with_mask in (True, False):
            m = (_dev(sc.masks), det) if with_mask else (None, None)
            got = _host_np(verify.verify_poses(sc.meshes, sc.labels[det], R_dev, t_dev, _dev(sc.K[det]), sc.frames_dev, sc.frame[det], *m, **sc.kw()))
            ren = sc.render(R, t, det)
            two = _host_np(verify.verify_maps(ren, sc.frames_dev, sc.frame[det], *m))
            _assert_equal(got, two, f"{name}, mask {with_mask}: the loop against the two calls")
            mh = (sc.masks, det) if with_mask else (None, None)
            _assert_equal(got, VH.verify(ren.cpu().numpy(), sc.frames, sc.frame[det], *mh), f"{name}, mask {with_mask}: the restatement")
            s = got["score"].reshape(Cn, M)
            print(f"{name}, mask {with_mask}: scores per candidate\n{np.round(s, 3)}")
            assert got["ok"].all() and np.all(s.argmax(axis=0) == Scene.GT)
        assert torch.equal(R_dev, _dev(R)) and torch.equal(t_dev, _dev(t))  # the caller's tensors stay


def test_best_of_returns_the_ground_truth_and_keeps_candidate_0_without_a_winner(scenes):
    for name, sc in scenes.items():
        # one more detection, a copy of detection 0 all of whose candidates lie outside the frame
        ext = lambda a: np.concatenate([a, a[:1]])  # noqa: E731
        away = np.array([50.0, 0.0, 0.0])
        cands = [(ext(R), np.concatenate([t, t[:1] + away])) for R, t in sc.candidates]
        M = sc.M + 1
        for mask in (_dev(ext(sc.masks)), None):
            out = verify.best_of(sc.meshes, ext(sc.labels), [(_dev(R), _dev(t)) for R, t in cands], _dev(ext(sc.K)), sc.frames_dev, ext(sc.frame),
                                 mask, **sc.kw())
            got = _host_np(out)
            assert got["which"].dtype == np.int32 and got["score"].dtype == np.float64 and got["R"].shape == (M, 3, 3) and got["t"].shape == (M, 3)
            assert list(got["which"]) == [Scene.GT] * sc.M + [-1], (name, got["which"])
            assert np.array_equal(_bits(got["R"][:-1]), _bits(cands[Scene.GT][0][:-1])) and np.array_equal(_bits(got["t"][:-1]), _bits(cands[Scene.GT][1][:-1]))
            assert np.array_equal(_bits(got["R"][-1]), _bits(cands[0][0][-1])) and np.array_equal(_bits(got["t"][-1]), _bits(cands[0][1][-1]))
            assert got["score"][-1] == -np.inf and np.all(got["score"][:-1] > 0)
            every = _host_np(out["all"])
            assert all(every[k].shape == (len(cands), M) for k in KEYS) and not every["covered"][:, -1].any() and not every["ok"][:, -1].any()
            assert np.array_equal(_bits(got["score"][:-1]), _bits(every["score"][Scene.GT, :-1]))


def test_no_rows_give_empty_tensors_and_arguments_are_checked(maps, scenes):
    sc = scenes["mixed"]
    dtypes = dict({k: torch.int32 for k in KEYS}, sum_q=torch.int64, score=torch.float64)
    off = verify.verify_maps(torch.zeros(0, sc.H, sc.W, device=DEV), sc.frames_dev, [])
    assert set(off) == set(KEYS) and all(off[k].shape == (0,) and off[k].dtype == dtypes[k] for k in KEYS)
    R, t = _dev(sc.candidates[0][0]), _dev(sc.candidates[0][1])
    out = verify.verify_poses(sc.meshes, [], R[:0], t[:0], _dev(sc.K[:0]), sc.frames_dev, [], _dev(sc.masks), [])
    assert all(out[k].shape == (0,) and out[k].dtype == dtypes[k] for k in KEYS)
    sel = verify.select_best(torch.zeros(0, dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), [], 0)
    assert sel["best"].shape == (0,) and sel["best"].dtype == torch.int32 and sel["best_score"].dtype == torch.float64
    none = verify.best_of(sc.meshes, [], [(R[:0], t[:0])] * 3, _dev(sc.K[:0]), sc.frames_dev, [])       # M == 0
    assert none["R"].shape == (0, 3, 3) and none["t"].shape == (0, 3) and none["which"].shape == (0,) and none["all"]["score"].shape == (3, 0)
    none = verify.best_of(sc.meshes, sc.labels, [], _dev(sc.K), sc.frames_dev, sc.frame)                 # C == 0
    assert none["R"].shape == (sc.M, 3, 3) and list(none["which"].cpu().numpy()) == [-1] * sc.M and none["all"]["ok"].shape == (0, sc.M)
    assert none["which"].dtype == torch.int32 and bool(torch.isinf(none["score"]).all())
    ren, frames = _dev(maps["ren"]), _dev(maps["frames"])
    with pytest.raises(ValueError, match="frame"):
        verify.verify_maps(ren, frames, [0, 1, 2, 0, 0, 0, 1, 1, 1])
    with pytest.raises(ValueError, match="mask_index"):
        verify.verify_maps(ren, frames, maps["frame"], _dev(maps["masks"]), [0, 1, 2, 3, 4, 5, 6, 0, 0])
    with pytest.raises(ValueError, match="mask_index"):
        verify.verify_maps(ren, frames, maps["frame"], _dev(maps["masks"]))                               # 6 masks for 9 rows, no index
    with pytest.raises(ValueError, match="group"):
        verify.select_best(torch.zeros(2, dtype=torch.float64, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV), [0, 2], 2)
    with pytest.raises(ValueError, match="differ in H, W"):
        verify.verify_maps(ren, frames, maps["frame"], torch.zeros(9, 37, 54, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="differ in H, W"):
        verify.verify_maps(torch.zeros(2, 37, 54, device=DEV), frames, [0, 0])
    torch.cuda.synchronize()
