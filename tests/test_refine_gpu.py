"""GPU tests of the depth refinement (csrc/icp.hip through gdrnet_amd.refine) against the host restatement tests/icp_host.py fed the device's own
renders, and against geometry.

Bounds.  A sum of n fp64 terms differs between two orders by at most about n 2^-53 sum|terms|; the device and the host evaluate each term with
the same operation sequence, so 4 pairs 2^-53 sum|terms| leaves headroom for the products.  The solve amplifies a relative perturbation of the
system by cond_2(S A S): a step is held to pairs 2^-50 cond_2 |xi|.  The geometric bounds are those the host restatement meets on the host
rasterizer's renders in tests/test_refine_cpu.py (a thousandth of a degree and of a millimetre clean, a tenth on millimetre-rounded frames)."""
import numpy as np
import pytest
import torch

import icp_host as IH
from gdrnet_amd import cabi, devargs, refine, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLEAN_BOUND, NOISY_BOUND = 1e-3, 0.1   # degrees and millimetres (tests/test_refine_cpu.py)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    """an integer view that compares NaNs and signed zeros bit by bit"""
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b, keys=("R", "t", "ok", "iters_done", "pairs", "rms"), rows=None):
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        if not torch.equal(_bits(x), _bits(y)):
            return k
    return None


class Scene:
    """a synth.make_refine_inputs scene on the device: the mesh table, the frames composed from the device's own renders of the ground truth"""

    def __init__(self, inp):
        self.inp, self.H, self.W = inp, inp["H"], inp["W"]
        self.meshes = render.MeshTable(inp["vertices"], inp["faces"])
        G = len(inp["gt_labels"])
        gt = render.render_depth(self.meshes, inp["gt_labels"], _dev(inp["R_gt"]), _dev(inp["t_gt"]), _dev(inp["K"][:1].repeat(G, axis=0)), self.H, self.W,
                                 inp["near"], inp["far"])
        self.frames = synth.refine_scene(inp, gt.cpu().numpy())
        self.frames_dev = _dev(self.frames)

    def render(self, rows, R, t):
        """the device's renders [len(rows),H,W] (host copy) of the rows' meshes under the poses R, t"""
        inp = self.inp
        d = render.render_depth(self.meshes, inp["labels"][rows], _dev(np.asarray(R)), _dev(np.asarray(t)), _dev(inp["K"][rows]), self.H, self.W,
                                inp["near"], inp["far"])
        return d.cpu().numpy()

    def refine(self, rows, R, t, **kw):
        inp = self.inp
        return refine.icp_refine(self.meshes, inp["labels"][rows], _dev(np.asarray(R)), _dev(np.asarray(t)), _dev(inp["K"][rows]), self.frames_dev,
                                 inp["frame"][rows], near=inp["near"], far=inp["far"], **kw)

    def start(self, **kw):
        rows = np.arange(len(self.inp["labels"]))
        return self.refine(rows, self.inp["R0"], self.inp["t0"], **kw)


@pytest.fixture(scope="module")
def scenes():
    out = {c: Scene(synth.make_refine_inputs(c)) for c in ("sphere", "mixed", "degenerate")}
    for inp in synth.make_refine_inputs("noisy"):
        out[inp["case"]] = Scene(inp)
    return out


def _host_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_system(got, ren, frames, frame, K, what, gates=(0.02, 0.01)):
    """device sums of one call against the restatement fed the same arrays, row by row; returns the pair counts"""
    counts = []
    for i in range(len(ren)):
        ref = IH.accumulate(ren[i], frames[frame[i]], K[i], *gates)
        n = ref["pairs"]
        assert int(got["pairs"][i]) == n, (what, i, int(got["pairs"][i]), n)
        A, b, sq = got["A"][i], got["b"][i], float(got["sq"][i])
        assert np.array_equal(A, A.T), (what, i)
        u = 4.0 * n * 2.0 ** -53
        eA, eb, es = np.abs(A - ref["A"]), np.abs(b - ref["b"]), abs(sq - ref["sq"])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(float(np.nanmax(eA / (u * ref["A_abs"]))) if n else 0.0, float(np.nanmax(eb / (u * ref["b_abs"]))) if n else 0.0,
                        es / (u * ref["sq"]) if ref["sq"] > 0 else 0.0)
        print(f"{what}[{i}]: pairs {n}, worst |device - host| = {worst:.3f} of 4 pairs 2^-53 sum|terms|")
        assert np.all(eA <= u * ref["A_abs"]) and np.all(eb <= u * ref["b_abs"]) and es <= u * ref["sq"], (what, i, worst)
        counts.append(n)
    return counts


def test_normal_equations_on_the_devices_renders_equal_the_restatement(scenes):
    for name in ("sphere", "mixed", "degenerate"):   # 96 rows = 6 bands | 120 rows = 7 bands and a half | a frame covered up to its last row and column
        sc = scenes[name]
        inp = sc.inp
        rows = np.arange(len(inp["labels"]))
        ren = render.render_depth(sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]), _dev(inp["K"]), sc.H, sc.W, inp["near"], inp["far"])
        got = _host_np(refine.normal_equations(ren, sc.frames_dev, inp["frame"], _dev(inp["K"])))
        assert got["A"].shape == (len(rows), 6, 6) and got["b"].shape == (len(rows), 6) and got["sq"].shape == got["pairs"].shape == (len(rows),)
        counts = _check_system(got, ren.cpu().numpy(), sc.frames, inp["frame"], inp["K"], name)
        for r in inp["convergent"]:
            assert counts[r] >= 400
        if name == "degenerate":
            assert (sc.frames > 0).all() and counts[0] > 3000 and counts[1] == counts[2] == 0
            ref = IH.accumulate(ren[0].cpu().numpy(), sc.frames[0], inp["K"][0])
            assert ref["mask"][62, 1:63].all() and ref["mask"][1:63, 62].all() and not ref["mask"][63].any() and not ref["mask"][:, 63].any()
            assert not ref["mask"][0].any() and not ref["mask"][:, 0].any() and ref["mask"][15:17, 1:63].all()   # across the first band's edge


@pytest.mark.parametrize("shape", ((3, 37, 53), (2, 16, 3), (2, 3, 3), (2, 2, 9), (1, 1, 1), (3, 35, 64)), ids=lambda s: "x".join(str(v) for v in s))
def test_normal_equations_on_hand_made_maps_at_the_launch_edges(shape):
    """full frames of a smooth surface with holes, renders a few millimetres off with holes of their own: pairs on every interior row and column,
    bands that do not divide H, frames narrower than the stencil, a K with a skew term"""
    N, H, W = shape
    F = 2
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u = lambda tag, *s: synth.hash_uniform(251, f"{tag}/{N}x{H}x{W}", s)  # noqa: E731
    frames = np.stack([0.5 + 0.1 * f + 0.02 * np.sin(x / 5.0 + f) * np.cos(y / 7.0) + 2e-4 * u(f"s{f}", H, W) for f in range(F)])
    frames[u("holes_s", F, H, W) < 0.03] = 0.0
    frame = np.arange(N) % F
    ren = frames[frame] + 0.05 * (u("off", N, H, W) - 0.5)    # up to 25 mm off: both sides of the 20 mm gate
    ren[u("holes_r", N, H, W) < 0.1] = 0.0
    frames, ren = frames.astype(np.float32), ren.astype(np.float32)
    K = np.array([[143.1, 0.4, 0.5 * W], [0.0, 141.7, 0.5 * H], [0.0, 0.0, 1.0]])[None].repeat(N, axis=0)
    K[:, 0, 2] += np.arange(N)
    got = _host_np(refine.normal_equations(_dev(ren), _dev(frames), frame, _dev(K)))
    counts = _check_system(got, ren, frames, frame, K, f"maps {shape}")
    if H < 3 or W < 3:
        assert max(counts) == 0 and not got["A"].any() and not got["b"].any() and not got["sq"].any()
    if H >= 35:   # pairs on both sides of every band edge and in the last interior row and column; none on the border
        assert min(counts) > 100
        m = IH.accumulate(ren[0], frames[0], K[0])["mask"]
        assert m[15].any() and m[16].any() and m[31].any() and m[32].any() and m[H - 2].any() and m[:, W - 2].any() and m[:, 1].any()
        assert not m[H - 1].any() and not m[0].any() and not m[:, 0].any() and not m[:, W - 1].any()
    one = _host_np(refine.normal_equations(_dev(ren), _dev(frames), frame, _dev(K[0] * 1.0)))   # a single K: instance 0 sees its own
    assert np.array_equal(one["A"][0], got["A"][0]) and np.array_equal(one["pairs"][:1], got["pairs"][:1])


def _check_steps(sc, rows, R, t, what):
    """icp_refine(iters=1) from the poses (R, t) of `rows` against the restatement's step on the device's renders of those poses"""
    ren = sc.render(rows, R, t)
    got = _host_np(sc.refine(rows, R, t, iters=1))
    inp = sc.inp
    for k, row in enumerate(rows):
        acc = IH.accumulate(ren[k], sc.frames[inp["frame"][row]], inp["K"][row])
        sol = IH.solve(acc["A"], acc["b"], acc["pairs"])
        assert int(got["ok"][k]) == int(sol["ok"]) and int(got["pairs"][k]) == acc["pairs"], (what, row, got["ok"][k], sol)
        if not sol["ok"]:
            assert int(got["iters_done"][k]) == 0 and np.array_equal(got["R"][k], R[k]) and np.array_equal(got["t"][k], t[k]), (what, row)
            continue
        assert int(got["iters_done"][k]) == 1
        w = IH.log_so3(got["R"][k] @ np.asarray(R[k]).T)
        v = got["t"][k] - IH.exp_so3(w) @ np.asarray(t[k])
        xi = sol["xi"]
        bound = acc["pairs"] * 2.0 ** -50 * sol["cond"] * np.linalg.norm(xi)
        ew, ev = np.linalg.norm(w - xi[:3]), np.linalg.norm(v - xi[3:])
        print(f"{what} row {row}: |xi| {np.linalg.norm(xi):.2e}, cond {sol['cond']:.1e}, pairs {acc['pairs']}, |dw| {ew:.2e} |dv| {ev:.2e}, bound {bound:.2e}")
        assert ew <= bound and ev <= bound, (what, row, ew, ev, bound)
        rms = np.sqrt(acc["sq"] / acc["pairs"])
        assert abs(float(got["rms"][k]) - rms) <= 1e-12 * rms


def test_one_step_equals_the_restatements_step(scenes):
    for name in ("sphere", "mixed"):   # the four icosphere starts, and the cubes and rectangles beside them
        sc = scenes[name]
        rows = np.arange(len(sc.inp["labels"]))
        _check_steps(sc, rows, sc.inp["R0"], sc.inp["t0"], name)
    # from the restatement's own poses after its iterations 1 .. 3 on the device's renders: small residuals without comparing trajectories
    sc = scenes["sphere"]
    rows, Rs, ts = [], [], []
    for row in (0, 1):
        res = IH.refine(lambda R, t: sc.render(np.array([row]), R[None], t[None])[0], sc.inp["R0"][row], sc.inp["t0"][row], sc.inp["K"][row],
                        sc.frames[0], iters=3)
        assert res["ok"] == 1 and res["iters_done"] == 3
        for tr in res["trace"][1:] + [dict(R=res["R"], t=res["t"])]:
            rows.append(row)
            Rs.append(tr["R"])
            ts.append(tr["t"])
    _check_steps(sc, np.array(rows), np.stack(Rs), np.stack(ts), "sphere after iterations 1-3")


def test_ten_iterations_meet_the_geometric_bounds_of_the_host(scenes):
    for name, bound in (("sphere", CLEAN_BOUND), ("mixed", CLEAN_BOUND), ("noisy/sphere", NOISY_BOUND), ("noisy/mixed", NOISY_BOUND)):
        sc = scenes[name]
        inp = sc.inp
        first, out = _host_np(sc.start(iters=1)), _host_np(sc.start())   # iters = 10 is the default
        for row in inp["convergent"]:
            g = int(inp["target"][row])
            re, te = IH.pose_errors(out["R"][row], out["t"][row], inp["R_gt"][g], inp["t_gt"][g])
            print(f"{name} row {row} from {inp['start_deg'][row]:g} deg / {inp['start_mm'][row]:g} mm: {re:.2e} deg, {te:.2e} mm after {out['iters_done'][row]} "
                  f"steps, pairs {out['pairs'][row]}, rms {first['rms'][row]:.2e} -> {out['rms'][row]:.2e} m")
            assert re < bound and te < bound, (name, row, re, te)
            assert out["ok"][row] == 1 and 1 <= out["iters_done"][row] <= 10 and out["pairs"][row] >= 400
            if bound == CLEAN_BOUND:
                assert out["rms"][row] <= first["rms"][row]
        assert np.all(out["iters_done"] <= 10) and np.all((out["ok"] == 0) | (out["ok"] == 1))
        assert out["R"].dtype == out["t"].dtype == out["rms"].dtype == np.float64 and out["ok"].dtype == out["iters_done"].dtype == out["pairs"].dtype == np.int32


def test_degenerate_instances_keep_their_pose_and_leave_the_others_alone(scenes):
    sc = scenes["degenerate"]
    inp = sc.inp
    out = _host_np(sc.start())
    assert list(out["ok"]) == [0, 0, 0] and list(out["iters_done"]) == [0, 0, 0]
    assert np.array_equal(out["R"], inp["R0"]) and np.array_equal(out["t"], inp["t0"])          # bit for bit
    assert out["pairs"][0] > 3000 and out["rms"][0] > 1e-4                                       # enough pairs: the matrix is what fails
    assert list(out["pairs"][1:]) == [0, 0] and np.isnan(out["rms"][1:]).all()                   # out of the frame | behind the camera
    # the same two beside the estimates of "mixed": its rows get the bits they get without them
    sc = scenes["mixed"]
    inp = sc.inp
    n = len(inp["labels"])
    rows = np.concatenate([[0], np.arange(n), [0]])
    R, t = inp["R0"][rows].copy(), inp["t0"][rows].copy()
    t[0] += np.array([50.0, 0.0, 0.0])
    t[-1] *= np.array([1.0, 1.0, -1.0])
    both, alone = sc.refine(rows, R, t), sc.start()
    assert _same(both, alone, rows=(slice(1, n + 1), slice(0, n))) is None
    both = _host_np(both)
    assert both["ok"][0] == both["ok"][-1] == 0 and both["pairs"][0] == both["pairs"][-1] == 0 and np.isnan(both["rms"][[0, -1]]).all()
    assert np.array_equal(both["R"][[0, -1]], R[[0, -1]]) and np.array_equal(both["t"][[0, -1]], t[[0, -1]])
    assert both["ok"][1] == 1 and both["ok"][n] == 1


def test_calls_are_deterministic_and_instances_independent(scenes):
    sc = scenes["mixed"]
    inp = sc.inp
    n = len(inp["labels"])
    a, b = sc.start(iters=4), sc.start(iters=4)
    assert _same(a, b) is None
    for row in range(n):
        one = sc.refine(np.array([row]), inp["R0"][[row]], inp["t0"][[row]], iters=4)
        assert _same(one, a, rows=(slice(0, 1), slice(row, row + 1))) is None, row
    args = (sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]))
    kw = dict(iters=4, near=inp["near"], far=inp["far"])
    shared = refine.icp_refine(*args, _dev(inp["K"][0]), sc.frames_dev, _dev(inp["frame"]), **kw)   # one K for all; frames from the device
    assert _same(shared, a) is None
    R32, t32 = _dev(inp["R0"], torch.float32), _dev(inp["t0"], torch.float32)
    lo = refine.icp_refine(sc.meshes, inp["labels"], R32, t32, _dev(inp["K"], torch.float32), sc.frames_dev, inp["frame"], **kw)
    hi = refine.icp_refine(sc.meshes, inp["labels"], R32.double(), t32.double(), _dev(inp["K"], torch.float32).double(), sc.frames_dev, inp["frame"], **kw)
    assert _same(lo, hi) is None and lo["R"].dtype == torch.float64
    start = _dev(inp["R0"])
    again = refine.icp_refine(sc.meshes, inp["labels"], start, _dev(inp["t0"]), _dev(inp["K"]), sc.frames_dev, inp["frame"], **kw)
    assert torch.equal(start, _dev(inp["R0"])) and _same(again, a) is None                       # the caller's tensors stay
    zero = sc.start(iters=0)
    z = _host_np(zero)
    assert np.array_equal(z["R"], inp["R0"]) and list(z["ok"]) == [1] * n and not z["iters_done"].any() and not z["pairs"].any() and np.isnan(z["rms"]).all()


def test_arguments_are_checked_before_any_launch_and_no_rows_gives_empty_tensors(scenes):
    sc = scenes["sphere"]
    inp = sc.inp
    R0, t0, K = _dev(inp["R0"]), _dev(inp["t0"]), _dev(inp["K"])
    with pytest.raises(ValueError, match="labels"):
        refine.icp_refine(sc.meshes, [0, 1], R0, t0, K, sc.frames_dev, inp["frame"])
    with pytest.raises(ValueError, match="frame"):
        refine.icp_refine(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev, [0, 1])
    with pytest.raises(ValueError, match="frame"):
        refine.icp_refine(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev, [0])
    with pytest.raises(ValueError, match="frame"):
        refine.normal_equations(torch.zeros(2, sc.H, sc.W, device=DEV), sc.frames_dev, [0, -1], K)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.icp_refine(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev.cpu(), inp["frame"])
    with pytest.raises(ValueError, match="float32"):
        refine.icp_refine(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev.double(), inp["frame"])
    with pytest.raises(ValueError, match="differ in H, W"):
        refine.normal_equations(torch.zeros(2, sc.H, sc.W + 1, device=DEV), sc.frames_dev, [0, 0], K)
    out = refine.icp_refine(sc.meshes, [], R0[:0], t0[:0], K[:0], sc.frames_dev, [])
    assert out["R"].shape == (0, 3, 3) and out["t"].shape == (0, 3) and all(out[k].shape == (0,) for k in ("ok", "iters_done", "pairs", "rms"))
    ne = refine.normal_equations(torch.zeros(0, sc.H, sc.W, device=DEV), sc.frames_dev, [], K[:0])
    assert ne["A"].shape == (0, 6, 6) and ne["b"].shape == (0, 6) and ne["sq"].shape == (0,) and ne["pairs"].shape == (0,)
    torch.cuda.synchronize()


def test_nothing_is_written_outside_the_outputs_and_the_workspace(scenes):
    """the entry points on buffers with a guard band on both sides, filled with a sentinel: the bands are unchanged, the payload is the wrapper's,
    and what the workspace held before the call does not matter"""
    lib, G = cabi.load(), 64
    sc = scenes["mixed"]
    inp = sc.inp
    N, H, W, F = len(inp["labels"]), sc.H, sc.W, inp["num_frames"]
    stream = devargs.stream(torch.device(DEV))
    K, lab, fr = _dev(inp["K"]), _dev(inp["labels"], torch.int32), _dev(inp["frame"], torch.int32)
    lab_host, fr_host = inp["labels"].astype(np.int32), inp["frame"].astype(np.int32)
    ren = render.render_depth(sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]), K, H, W, inp["near"], inp["far"])
    ws_doubles = int(lib.gdrn_icp_workspace_bytes(N, H, W) + 7) // 8
    assert ws_doubles * 8 >= N * 8 * 28 * 8 + N * 10 * 4

    def banded(n, dtype, fill):
        return torch.full((G + n + G,), fill, dtype=dtype, device=DEV)

    def intact(bufs, fills, what):
        torch.cuda.synchronize()
        for k, b in bufs.items():
            f = torch.full((G,), fills[k], dtype=b.dtype, device=DEV)
            assert torch.equal(_bits(b[:G]), _bits(f)) and torch.equal(_bits(b[-G:]), _bits(f)), (what, k)

    ref = refine.normal_equations(ren, sc.frames_dev, inp["frame"], K)
    iu = torch.triu_indices(6, 6, device=DEV)
    results = []
    for ws_fill in (float("nan"), -7.25):
        fills = dict(sys=-7.25, pairs=-77, ws=ws_fill)
        bufs = dict(sys=banded(N * 28, torch.float64, -7.25), pairs=banded(N, torch.int32, -77), ws=banded(ws_doubles, torch.float64, ws_fill))
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        cabi.check(lib.gdrn_icp_accumulate(ren.data_ptr(), sc.frames_dev.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, K.data_ptr(), N, H, W, 0.02, 0.01,
                                           ptr["sys"], ptr["pairs"], ptr["ws"], stream), "icp_accumulate")
        intact(bufs, fills, "accumulate")
        sys = bufs["sys"][G:-G].view(N, 28)
        assert torch.equal(_bits(sys[:, :21]), _bits(ref["A"][:, iu[0], iu[1]])) and torch.equal(_bits(sys[:, 21:27]), _bits(ref["b"]))
        assert torch.equal(_bits(sys[:, 27]), _bits(ref["sq"])) and torch.equal(bufs["pairs"][G:-G], ref["pairs"])
        results.append(sys.clone())
    assert torch.equal(_bits(results[0]), _bits(results[1]))
    # one step from the combined systems: the pose of icp_refine(iters=1)
    want = sc.start(iters=1)
    fills = dict(R=-7.25, t=-7.25, state=-77)
    bufs = dict(R=banded(N * 9, torch.float64, -7.25), t=banded(N * 3, torch.float64, -7.25), state=banded(N * 2, torch.int32, -77))
    bufs["R"][G:-G] = _dev(inp["R0"]).reshape(-1)
    bufs["t"][G:-G] = _dev(inp["t0"]).reshape(-1)
    bufs["state"][G:-G] = 0
    ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
    cabi.check(lib.gdrn_icp_step(results[0].data_ptr(), ref["pairs"].data_ptr(), N, 64, ptr["R"], ptr["t"], ptr["state"], stream), "icp_step")
    intact(bufs, fills, "step")
    assert torch.equal(_bits(bufs["R"][G:-G].view(N, 3, 3)), _bits(want["R"])) and torch.equal(_bits(bufs["t"][G:-G].view(N, 3)), _bits(want["t"]))
    state = bufs["state"][G:-G].view(N, 2)
    assert torch.equal(state[:, 1], want["iters_done"]) and torch.equal((state[:, 0] != refine.DEGENERATE).to(torch.int32), want["ok"])
    frozen = bufs["R"].clone()
    cabi.check(lib.gdrn_icp_step(results[0].data_ptr(), ref["pairs"].data_ptr(), N, 64, ptr["R"], ptr["t"], ptr["state"], stream), "icp_step")
    torch.cuda.synchronize()
    deg = state[:, 0] == refine.DEGENERATE
    assert bool(deg.any()) and torch.equal(_bits(frozen[G:-G].view(N, 9)[deg]), _bits(bufs["R"][G:-G].view(N, 9)[deg]))   # a frozen instance is left alone
    # the whole loop
    want = sc.start(iters=3)
    tb = sc.meshes.on(torch.device(DEV))
    outs = []
    for ws_fill in (float("nan"), 3.0e300):
        fills = dict(R=-7.25, t=-7.25, scratch=-7.25, ok=-77, iters_done=-77, pairs=-77, rms=-7.25, ws=ws_fill)
        bufs = dict(R=banded(N * 9, torch.float64, -7.25), t=banded(N * 3, torch.float64, -7.25), scratch=banded(N * H * W, torch.float32, -7.25),
                    ok=banded(N, torch.int32, -77), iters_done=banded(N, torch.int32, -77), pairs=banded(N, torch.int32, -77),
                    rms=banded(N, torch.float64, -7.25), ws=banded(ws_doubles, torch.float64, ws_fill))
        bufs["R"][G:-G] = _dev(inp["R0"]).reshape(-1)
        bufs["t"][G:-G] = _dev(inp["t0"]).reshape(-1)
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        p = cabi.ptr
        cabi.check(lib.gdrn_icp_refine(p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]),
                                       sc.meshes.num_classes, sc.meshes.f_max, lab.data_ptr(), lab_host.ctypes.data, ptr["R"], ptr["t"], K.data_ptr(), N,
                                       sc.frames_dev.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, H, W, inp["near"], inp["far"], 3, 0.02, 0.01, 64,
                                       ptr["scratch"], ptr["ok"], ptr["iters_done"], ptr["pairs"], ptr["rms"], ptr["ws"], stream), "icp_refine")
        intact(bufs, fills, "refine")
        got = dict(R=bufs["R"][G:-G].view(N, 3, 3), t=bufs["t"][G:-G].view(N, 3), ok=bufs["ok"][G:-G], iters_done=bufs["iters_done"][G:-G],
                   pairs=bufs["pairs"][G:-G], rms=bufs["rms"][G:-G])
        assert _same(got, want) is None, _same(got, want)
        outs.append(bufs["scratch"][G:-G].clone())
    assert torch.equal(outs[0], outs[1]) and not bool((outs[0] == -7.25).any())
