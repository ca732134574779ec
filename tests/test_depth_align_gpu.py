"""GPU tests of the coarse depth alignment (csrc/depth_align.hip through gdrnet_amd.refine) against the host restatement tests/align_host.py.

The median is an exact order statistic and the shift one fixed fp64 operation sequence, so every comparison with the restatement is bitwise:
on hand-made maps that put the two ranks, the ties, the gate and the pair threshold where the selection can go wrong, and on the device's own
renders, round by round.  The geometric bounds are those of tests/test_refine_gpu.py for the same fixtures."""
import numpy as np
import pytest
import torch

import align_host as AH
import icp_host as IH
from gdrnet_amd import cabi, devargs, refine, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLEAN_BOUND, NOISY_BOUND = 1e-3, 0.1   # degrees and millimetres (tests/test_refine_gpu.py)
EXTRA_MM = (30.0, -40.0, 60.0)         # along the ground truth's ray, on top of the fixture's own start
C = np.float32(0.1)
GATE = float(np.float32(0.2))          # == 2 C exactly: a difference can EQUAL the gate
MIN_PAIRS = 64
KEYS = ("offset", "pairs", "covered", "ok")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    """an integer view that compares NaNs and signed zeros bit by bit"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _tbits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _host_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _restated(ren, frames, frame, gate=GATE, min_pairs=MIN_PAIRS):
    rows = [AH.offset(ren[i], frames[frame[i]], gate, min_pairs) for i in range(len(ren))]
    return dict(offset=np.array([r["offset"] for r in rows], dtype=np.float64), pairs=np.array([r["pairs"] for r in rows], dtype=np.int32),
                covered=np.array([r["covered"] for r in rows], dtype=np.int32), ok=np.array([r["ok"] for r in rows], dtype=np.int32))


def _assert_equal(got, ref, what, keys=KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and np.array_equal(_bits(got[k]), _bits(ref[k])), (what, k, got[k], ref[k])


def _make_maps():
    """N = 7 estimates in F = 2 frames of 37 x 53 (three bands of 16, 16 and 5 rows; 1961 pixels, no multiple of 256): dict(ren, frames, frame)"""
    N, F, H, W = 7, 2, 37, 53
    u = lambda tag, *s: synth.hash_uniform(311, tag, s)  # noqa: E731
    idx = np.arange(H * W).reshape(H, W)
    frames = np.zeros((F, H, W), dtype=np.float32)
    frames[0] = (512 + np.floor(512 * u("f0", H, W))) / 1024.0          # multiples of 1 / 1024 in [0.5, 1)
    frames[1] = np.choose(idx % 4, [2 * C, C, 4 * C, 2 * C])             # exact multiples of C
    ren = np.zeros((N, H, W), dtype=np.float32)
    frame = np.array([0, 1, 1, 0, 0, 0, 1])
    # row 0: hashed differences on both sides of the gate in all three bands, uncovered pixels, and pixels without a usable observation
    ren[0] = (frames[0].astype(np.float64) - 0.5 * (u("d0", H, W) - 0.5)).astype(np.float32)
    ren[0][u("hole0", H, W) < 0.2] = 0.0
    bad = u("bad0", H, W)
    frames[0][bad < 0.03] = 0.0
    frames[0][(bad >= 0.03) & (bad < 0.06)] = np.nan
    frames[0][(bad >= 0.06) & (bad < 0.09)] = np.inf
    if AH.offset(ren[0], frames[0], GATE, MIN_PAIRS)["pairs"] % 2 == 0:   # an odd count: drop one pair
        ys, xs = np.nonzero(AH.pair_differences(ren[0], frames[0], GATE)[1])
        ren[0, ys[0], xs[0]] = 0.0
    # row 1: half the differences -C, half +C (pixels 4 k and 4 k + 1 of the first 1000)
    ren[1][(idx % 4 == 0) & (idx < 1000)] = C
    ren[1][(idx % 4 == 1) & (idx < 1000)] = 2 * C
    # row 2: all differences equal
    ren[2][idx % 4 == 0] = C
    # row 3: differences that are multiples of 1 / 1024 of both signs, exact zeros among them
    k3 = np.floor(41 * u("k3", H, W)) - 20
    ren[3] = (frames[0].astype(np.float64) - k3 / 1024.0).astype(np.float32)
    ren[3][u("hole3", H, W) < 0.5] = 0.0
    # rows 4 and 5: exactly MIN_PAIRS and MIN_PAIRS - 1 pairs, all of them in the second band (rows 16 .. 31)
    usable = np.isfinite(frames[0]) & (frames[0] > 0)
    for row, count in ((4, MIN_PAIRS), (5, MIN_PAIRS - 1)):
        ys, xs = np.nonzero(usable[16:32])
        pick = np.argsort(u(f"pick{row}", len(ys)))[:count]
        d = 0.1 * (u(f"d{row}", count) - 0.5)
        ren[row, ys[pick] + 16, xs[pick]] = (frames[0, ys[pick] + 16, xs[pick]].astype(np.float64) - d).astype(np.float32)
    # row 6: |d| == the gate is a pair, the next float above it is not; -gate is one too; 130 pairs of -C and +C around them
    two_c, four_c = np.float32(2 * C), np.float32(4 * C)
    flat = ren[6].reshape(-1)
    flat[2], flat[6] = two_c, np.nextafter(two_c, np.float32(0))          # under 4 C: d = 2 C | d = the float after 2 C
    flat[4], flat[8] = four_c, np.nextafter(four_c, np.float32(1))        # under 2 C: d = -2 C | d below -2 C
    flat[np.arange(101, 501, 4)] = two_c                                   # under C: d = -C, 100 of them
    flat[np.arange(1000, 1120, 4)] = C                                     # under 2 C: d = +C, 30 of them
    return dict(ren=ren, frames=frames, frame=frame, N=N, F=F, H=H, W=W)


@pytest.fixture(scope="module")
def maps():
    return _make_maps()


def _maps_are_what_they_are_meant_to_be(maps, ref):
    ren, frames, frame = maps["ren"], maps["frames"], maps["frame"]
    d = [AH.pair_differences(ren[i], frames[frame[i]], GATE) for i in range(maps["N"])]
    bands = lambda m: [bool(m[0:16].any()), bool(m[16:32].any()), bool(m[32:].any())]  # noqa: E731
    assert ref["pairs"][0] % 2 == 1 and ref["pairs"][0] > 300 and bands(d[0][1]) == [True] * 3 and ref["covered"][0] > ref["pairs"][0] + 300
    f0, m0 = frames[0], d[0][1]
    assert ((f0 == 0) & (ren[0] > 0)).any() and (np.isnan(f0) & (ren[0] > 0)).any() and (np.isinf(f0) & (ren[0] > 0)).any()
    assert not m0[(f0 == 0) | ~np.isfinite(f0) | (ren[0] == 0)].any()
    assert ref["pairs"][1] == 500 and (d[1][0] == -C).sum() == 250 and (d[1][0] == C).sum() == 250 and _bits(ref["offset"][1:2])[0] == 0   # +0.0
    assert AH.key(-C) >> 21 != AH.key(C) >> 21                             # lo and hi part at the first level
    assert ref["pairs"][2] > 400 and np.all(d[2][0] == C) and ref["offset"][2] == np.float64(C)
    q = d[3][0].astype(np.float64) * 1024.0
    assert np.all(q == np.round(q)) and (q == 0).sum() > 5 and (q < 0).any() and (q > 0).any() and len(np.unique(q)) < 50 < ref["pairs"][3]
    assert ref["pairs"][4] == MIN_PAIRS and ref["ok"][4] == 1 and bands(d[4][1]) == [False, True, False]
    assert ref["pairs"][5] == MIN_PAIRS - 1 and ref["ok"][5] == 0 and np.isnan(ref["offset"][5]) and ref["covered"][5] == MIN_PAIRS - 1
    m6 = d[6][1].reshape(-1)
    e6 = (frames[1] - ren[6]).reshape(-1)
    assert m6[2] and e6[2] == np.float32(GATE) and not m6[6] and e6[6] == np.nextafter(np.float32(GATE), np.float32(1))
    assert m6[4] and e6[4] == -np.float32(GATE) and not m6[8] and e6[8] < -np.float32(GATE) and ref["pairs"][6] == 132 and ref["covered"][6] == 134


def test_offsets_on_hand_made_maps_equal_the_restatement_bitwise(maps):
    ren, frames, frame = maps["ren"], maps["frames"], maps["frame"]
    ref = _restated(ren, frames, frame)
    _maps_are_what_they_are_meant_to_be(maps, ref)
    got = _host_np(refine.depth_offset(_dev(ren), _dev(frames), frame, gate=GATE, min_pairs=MIN_PAIRS))
    for i in range(maps["N"]):
        print(f"row {i}: pairs {got['pairs'][i]} of {got['covered'][i]} covered, ok {got['ok'][i]}, offset {got['offset'][i]!r} (host {ref['offset'][i]!r})")
    _assert_equal(got, ref, "maps")
    assert list(got["ok"]) == [1, 1, 1, 1, 1, 0, 1]
    # a smaller gate and a larger threshold move both decisions
    got = _host_np(refine.depth_offset(_dev(ren), _dev(frames), frame, gate=0.05, min_pairs=150))
    _assert_equal(got, _restated(ren, frames, frame, 0.05, 150), "maps, gate 0.05")
    assert got["ok"][1] == 0 and got["pairs"][1] == 0 and got["ok"][0] == 1


def test_a_frame_of_pairs_distinct_and_all_equal():
    H, W = 120, 160
    n = H * W
    order = np.argsort(synth.hash_uniform(312, "perm", (n,)))
    ren = np.zeros((2, n), dtype=np.float32)
    ren[0] = np.float32(0.9) + order.astype(np.float32) * np.float32(2.0 ** -18)   # exact: below 1, multiples of 2^-18 above fp32(0.9)
    ren[1] = 0.875
    ren = ren.reshape(2, H, W)
    frames = np.ones((1, H, W), dtype=np.float32)
    ref = _restated(ren, frames, [0, 0])
    assert list(ref["pairs"]) == [n, n] and len(np.unique(frames[0] - ren[0])) == n and ref["offset"][1] == 0.125
    got = _host_np(refine.depth_offset(_dev(ren), _dev(frames), [0, 0], gate=GATE))
    _assert_equal(got, ref, "full frames")
    assert list(got["covered"]) == [n, n]


def test_calls_are_deterministic_and_rows_independent(maps):
    ren, frames, frame = _dev(maps["ren"]), _dev(maps["frames"]), maps["frame"]
    a = _host_np(refine.depth_offset(ren, frames, frame, gate=GATE))
    b = _host_np(refine.depth_offset(ren, frames, frame, gate=GATE))
    _assert_equal(a, b, "twice")
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    p = _host_np(refine.depth_offset(ren[_dev(perm)], frames, _dev(frame[perm]), gate=GATE))   # frames from the device
    _assert_equal(p, {k: a[k][perm] for k in KEYS}, "permuted")
    for i in range(maps["N"]):
        one = _host_np(refine.depth_offset(ren[i : i + 1], frames, frame[i : i + 1], gate=GATE))
        _assert_equal(one, {k: a[k][i : i + 1] for k in KEYS}, f"row {i} alone")


class Scene:
    """a synth.make_refine_inputs scene on the device: the mesh table, the frames composed from the device's own renders of the ground truth,
    and per row of the fixture three starts: its own, moved by EXTRA_MM along the ground truth's ray"""

    def __init__(self, inp, extras=EXTRA_MM):
        self.inp, self.H, self.W = inp, inp["H"], inp["W"]
        self.meshes = render.MeshTable(inp["vertices"], inp["faces"])
        G = len(inp["gt_labels"])
        gt = render.render_depth(self.meshes, inp["gt_labels"], _dev(inp["R_gt"]), _dev(inp["t_gt"]), _dev(inp["K"][:1].repeat(G, axis=0)), self.H, self.W,
                                 inp["near"], inp["far"])
        self.frames = synth.refine_scene(inp, gt.cpu().numpy())
        self.frames_dev = _dev(self.frames)
        self.rows = np.repeat(np.arange(len(inp["labels"])), len(extras))
        t_gt = inp["t_gt"][inp["target"][self.rows]]
        self.R0 = inp["R0"][self.rows]
        self.t0 = inp["t0"][self.rows] + 1e-3 * np.tile(extras, len(inp["labels"]))[:, None] * t_gt / t_gt[:, 2:3]

    def args(self, t, rows=None):
        inp, r = self.inp, self.rows if rows is None else rows
        R = self.R0 if rows is None else inp["R0"][rows]
        return (self.meshes, inp["labels"][r], _dev(R), _dev(np.asarray(t)), _dev(inp["K"][r]), self.frames_dev, inp["frame"][r])

    def kw(self):
        return dict(near=self.inp["near"], far=self.inp["far"])

    def render(self, t):
        inp = self.inp
        d = render.render_depth(self.meshes, inp["labels"][self.rows], _dev(self.R0), _dev(np.asarray(t)), _dev(inp["K"][self.rows]), self.H, self.W,
                                inp["near"], inp["far"])
        return d.cpu().numpy()


@pytest.fixture(scope="module")
def scenes():
    out = {"sphere": Scene(synth.make_refine_inputs("sphere"))}
    for inp in synth.make_refine_inputs("noisy"):
        out[inp["case"]] = Scene(inp)
    return out


def test_every_round_on_the_devices_renders_equals_the_restatement_bitwise(scenes):
    for name, sc in scenes.items():
        inp = sc.inp
        fr = inp["frame"][sc.rows]
        t = sc.t0
        two = _host_np(refine.depth_align(*sc.args(sc.t0), rounds=2, **sc.kw()))
        for rnd in (1, 2):
            got = _host_np(refine.depth_align(*sc.args(t), rounds=1, **sc.kw()))
            ren = sc.render(t)
            ref = _restated(ren, sc.frames, fr, 0.2, 64)
            _assert_equal(got, ref, f"{name} round {rnd}")
            assert ref["ok"].all() and ref["pairs"].min() >= 400
            want = np.stack([AH.shift(t[k], ref["offset"][k]) for k in range(len(t))])
            assert np.array_equal(_bits(got["t"]), _bits(want)), (name, rnd)
            g = inp["t_gt"][inp["target"][sc.rows]]
            along = 1e3 * np.abs(np.sum((want - g) * g / np.linalg.norm(g, axis=1, keepdims=True), axis=1))
            print(f"{name} round {rnd}: pairs {list(ref['pairs'])}, offsets (mm) {[round(1e3 * o, 3) for o in ref['offset']]}, along-ray error after (mm) "
                  f"{[round(a, 3) for a in along]}")
            t = want
        _assert_equal(two, got, f"{name}: two rounds in one call")          # the second round's outputs
        assert np.array_equal(_bits(two["t"]), _bits(t)), name
        assert along.max() < 10.0                                            # half of the ICP's dist_gate
        zero = _host_np(refine.depth_align(*sc.args(sc.t0), rounds=0, **sc.kw()))
        n = len(sc.rows)
        assert np.array_equal(_bits(zero["t"]), _bits(sc.t0)) and list(zero["ok"]) == [1] * n and not zero["pairs"].any() and not zero["covered"].any()
        assert np.isnan(zero["offset"]).all()


def test_refine_rgbd_refines_the_starts_the_icp_alone_returns_unchanged(scenes):
    for name, sc in scenes.items():
        inp = sc.inp
        bound = CLEAN_BOUND if name == "sphere" else NOISY_BOUND
        start_t = _dev(sc.t0)
        alone = _host_np(refine.icp_refine(*sc.args(sc.t0), **sc.kw()))
        assert not alone["ok"].any() and not alone["iters_done"].any() and alone["pairs"].max() < 64
        assert np.array_equal(_bits(alone["R"]), _bits(sc.R0)) and np.array_equal(_bits(alone["t"]), _bits(sc.t0))
        args = sc.args(sc.t0)
        res = refine.refine_rgbd(args[0], args[1], args[2], start_t, *args[4:], **sc.kw())
        align = _host_np(res["align"])
        out = _host_np(res)
        assert torch.equal(start_t, _dev(sc.t0))                             # the caller's tensors stay
        assert align["ok"].all() and out["ok"].all() and set(res) == {"R", "t", "ok", "iters_done", "pairs", "rms", "align"}
        for k, row in enumerate(sc.rows):
            g = int(inp["target"][row])
            re, te = IH.pose_errors(out["R"][k], out["t"][k], inp["R_gt"][g], inp["t_gt"][g])
            print(f"{name} row {row} {EXTRA_MM[k % 3]:+g} mm: offset {1e3 * align['offset'][k]:.3f} mm in the last round, then {re:.2e} deg, {te:.2e} mm after "
                  f"{out['iters_done'][k]} steps, pairs {out['pairs'][k]}")
            assert re < bound and te < bound, (name, row, re, te)
            assert 1 <= out["iters_done"][k] <= 10 and out["pairs"][k] >= 400


def test_rows_without_an_overlap_keep_their_translation():
    inp = synth.make_refine_inputs("degenerate")
    sc = Scene(inp, extras=(0.0,))
    rows = np.array([1, 2, 0])   # out of the frame | behind the camera | the rectangle, which overlaps
    out = _host_np(refine.depth_align(*sc.args(inp["t0"][rows], rows), **sc.kw()))
    assert list(out["ok"]) == [0, 0, 1] and list(out["pairs"][:2]) == [0, 0] and list(out["covered"][:2]) == [0, 0] and np.isnan(out["offset"][:2]).all()
    assert np.array_equal(_bits(out["t"][:2]), _bits(inp["t0"][rows[:2]])) and out["pairs"][2] > 3000
    res = refine.refine_rgbd(*sc.args(inp["t0"][rows], rows), **sc.kw())       # a row that could not be moved goes on with the pose it had
    torch.cuda.synchronize()
    assert np.array_equal(_bits(res["t"][:2].cpu().numpy()), _bits(inp["t0"][rows[:2]])) and list(res["ok"][:2].cpu().numpy()) == [0, 0]


def test_nothing_is_written_outside_the_outputs_and_the_workspace(maps, scenes):
    """both entry points on buffers with a guard band on both sides, filled with a sentinel: the bands are unchanged, the payload is the
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

    N, F, H, W = maps["N"], maps["F"], maps["H"], maps["W"]
    ren, frames = _dev(maps["ren"]), _dev(maps["frames"])
    fr_host = maps["frame"].astype(np.int32)
    fr = _dev(fr_host)
    want = _host_np(refine.depth_offset(ren, frames, fr_host, gate=GATE))
    ws_bytes = int(lib.gdrn_depth_align_workspace_bytes(N, H, W))
    assert ws_bytes == N * 8 + (3 * N + 1) * 4 + N * H * W * 4
    ws_doubles = (ws_bytes + 7) // 8
    for ws_fill in (float("nan"), -7.25, 0.0):
        fills = dict(offset=-7.25, pairs=-77, covered=-77, ok=-77, ws=ws_fill)
        bufs = dict(offset=banded(N, torch.float64, -7.25), pairs=banded(N, torch.int32, -77), covered=banded(N, torch.int32, -77),
                    ok=banded(N, torch.int32, -77), ws=banded(ws_doubles, torch.float64, ws_fill))
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        cabi.check(lib.gdrn_depth_offset(ren.data_ptr(), frames.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, N, H, W, GATE, MIN_PAIRS, ptr["offset"],
                                         ptr["pairs"], ptr["covered"], ptr["ok"], ptr["ws"], stream), "depth_offset")
        intact(bufs, fills, "offset")
        _assert_equal({k: bufs[k][G:-G].cpu().numpy() for k in KEYS}, want, f"offset, workspace of {ws_fill}")
    # the whole loop
    sc = scenes["noisy/mixed"]
    inp = sc.inp
    N, H, W, F = len(sc.rows), sc.H, sc.W, inp["num_frames"]
    want = _host_np(refine.depth_align(*sc.args(sc.t0), **sc.kw()))
    tb = sc.meshes.on(torch.device(DEV))
    lab_host, fr_host = inp["labels"][sc.rows].astype(np.int32), inp["frame"][sc.rows].astype(np.int32)
    lab, fr, K, R = _dev(lab_host), _dev(fr_host), _dev(inp["K"][sc.rows]), _dev(sc.R0)
    ws_doubles = (int(lib.gdrn_depth_align_workspace_bytes(N, H, W)) + 7) // 8
    scratches = []
    for ws_fill in (float("nan"), 3.0e300):
        fills = dict(t=-7.25, scratch=-7.25, ok=-77, pairs=-77, covered=-77, offset=-7.25, ws=ws_fill)
        bufs = dict(t=banded(N * 3, torch.float64, -7.25), scratch=banded(N * H * W, torch.float32, -7.25), ok=banded(N, torch.int32, -77),
                    pairs=banded(N, torch.int32, -77), covered=banded(N, torch.int32, -77), offset=banded(N, torch.float64, -7.25),
                    ws=banded(ws_doubles, torch.float64, ws_fill))
        bufs["t"][G:-G] = _dev(sc.t0).reshape(-1)
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        p = cabi.ptr
        cabi.check(lib.gdrn_depth_align(p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]),
                                        sc.meshes.num_classes, sc.meshes.f_max, lab.data_ptr(), lab_host.ctypes.data, R.data_ptr(), ptr["t"], K.data_ptr(), N,
                                        sc.frames_dev.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, H, W, inp["near"], inp["far"], 2, 0.2, 64,
                                        ptr["scratch"], ptr["ok"], ptr["pairs"], ptr["covered"], ptr["offset"], ptr["ws"], stream), "depth_align")
        intact(bufs, fills, "align")
        got = {k: bufs[k][G:-G].cpu().numpy() for k in KEYS}
        got["t"] = bufs["t"][G:-G].view(N, 3).cpu().numpy()
        _assert_equal(got, want, f"align, workspace of {ws_fill}", keys=KEYS + ("t",))
        scratches.append(bufs["scratch"][G:-G].clone())
    assert torch.equal(scratches[0], scratches[1]) and not bool((scratches[0] == -7.25).any())
    assert torch.equal(R, _dev(sc.R0))


def test_no_rows_give_empty_tensors_and_arguments_are_checked(maps, scenes):
    sc = scenes["sphere"]
    inp = sc.inp
    a = sc.args(sc.t0)
    out = refine.depth_align(a[0], [], a[2][:0], a[3][:0], a[4][:0], a[5], [])
    assert out["t"].shape == (0, 3) and out["t"].dtype == torch.float64 and all(out[k].shape == (0,) for k in KEYS)
    off = refine.depth_offset(torch.zeros(0, sc.H, sc.W, device=DEV), sc.frames_dev, [])
    assert all(off[k].shape == (0,) for k in KEYS) and off["offset"].dtype == torch.float64 and off["ok"].dtype == torch.int32
    both = refine.refine_rgbd(a[0], [], a[2][:0], a[3][:0], a[4][:0], a[5], [])
    assert both["R"].shape == (0, 3, 3) and both["align"]["t"].shape == (0, 3)
    with pytest.raises(ValueError, match="labels"):
        refine.depth_align(a[0], [0, 1], *a[2:])
    with pytest.raises(ValueError, match="frame"):
        refine.depth_align(*a[:6], [0])
    with pytest.raises(ValueError, match="frame"):
        refine.depth_offset(_dev(maps["ren"]), _dev(maps["frames"]), [0, 1, 2, 0, 0, 0, 1])
    with pytest.raises(ValueError, match="differ in H, W"):
        refine.depth_offset(torch.zeros(2, sc.H, sc.W + 1, device=DEV), sc.frames_dev, [0, 0])
    with pytest.raises(ValueError, match="float32"):
        refine.depth_align(*a[:5], sc.frames_dev.double(), a[6])
    torch.cuda.synchronize()
