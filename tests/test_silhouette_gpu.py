"""GPU tests of the silhouette term of the depth refinement (csrc/silhouette.hip through gdrnet_amd.refine) against the host restatement
tests/sil_host.py fed the device's own renders, and against geometry.

Bounds.  The transform is integer arithmetic: bit for bit.  A sum of n fp64 terms differs between two orders by at most about n 2^-53
sum|terms|; a pair pixel gives two terms to every sum and the device and the host evaluate each term with the same operation sequence, so
4 (2 pairs) 2^-53 sum|terms| leaves the headroom tests/test_refine_gpu.py leaves.  The solve amplifies a relative perturbation of the system by
cond_2(S A S): a step is held to terms 2^-50 cond_2 |xi|, terms = depth pairs + 2 silhouette pairs (test_refine_gpu.py's bound with the
number of terms of the combined sums).  The geometric bounds are those of tests/test_silhouette_cpu.py: one pixel's footprint, 1.0 mm, and one
pixel at the half-length of the plate's long side, 1.43 degrees."""
import numpy as np
import pytest
import torch

import contour_masks
import icp_host as IH
import sil_host as SH
from gdrnet_amd import cabi, devargs, refine, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATERAL_MM = 1e3 * 0.6 / 600.0
ROTATION_DEG = float(np.degrees(np.arctan(1.0 / 40.0)))
CLEAN_BOUND = 1e-3
SHAPES = ((1, 1, 1), (2, 3, 3), (2, 16, 3), (2, 17, 5), (3, 37, 53), (3, 35, 64), (2, 20, 130))
KEYS = ("R", "t", "ok", "iters_done", "pairs", "rms", "sil_pairs", "sil_rms")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    """an integer view that compares NaNs and signed zeros bit by bit"""
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b, keys=KEYS, rows=None):
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        if not torch.equal(_bits(x), _bits(y)):
            return k
    return None


def _host_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


class Scene:
    """a synth.make_silhouette_inputs scene on the device: the mesh table, frames and masks composed from the device's own renders of the ground truth"""

    def __init__(self, inp):
        self.inp, self.H, self.W = inp, inp["H"], inp["W"]
        self.meshes = render.MeshTable(inp["vertices"], inp["faces"])
        G = len(inp["gt_labels"])
        gt = render.render_depth(self.meshes, inp["gt_labels"], _dev(inp["R_gt"]), _dev(inp["t_gt"]), _dev(inp["K"][:1].repeat(G, axis=0)), self.H, self.W,
                                 inp["near"], inp["far"])
        self.frames, gt_masks = synth.silhouette_scene(inp, gt.cpu().numpy())
        self.masks = gt_masks[inp["target"]]                    # one mask per estimate
        self.frames_dev, self.masks_dev = _dev(self.frames), _dev(self.masks)
        self.rows = np.arange(len(inp["labels"]))

    def render(self, rows, R, t):
        inp = self.inp
        d = render.render_depth(self.meshes, inp["labels"][rows], _dev(np.asarray(R)), _dev(np.asarray(t)), _dev(inp["K"][rows]), self.H, self.W,
                                inp["near"], inp["far"])
        return d.cpu().numpy()

    def refine(self, rows, R, t, **kw):
        inp = self.inp
        return refine.icp_refine_sil(self.meshes, inp["labels"][rows], _dev(np.asarray(R)), _dev(np.asarray(t)), _dev(inp["K"][rows]), self.frames_dev,
                                     inp["frame"][rows], self.masks_dev[torch.as_tensor(rows, device=DEV)], near=inp["near"], far=inp["far"], **kw)

    def start(self, **kw):
        return self.refine(self.rows, self.inp["R0"], self.inp["t0"], **kw)

    def depth_only(self, **kw):
        inp = self.inp
        return refine.icp_refine(self.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]), _dev(inp["K"]), self.frames_dev, inp["frame"],
                                 near=inp["near"], far=inp["far"], **kw)


@pytest.fixture(scope="module")
def scenes():
    return {c: Scene(synth.make_silhouette_inputs(c)) for c in synth.SILHOUETTE_CASES}


def _hand_made(shape):
    """masks [N,H,W] uint8 (blob, noise, empty, full, single pixel and a second blob, N at a time), two depth frames of 10 cm steps hashed per
    pixel with holes (a neighbour is nearer, farther or missing on either side of every contour) and the frame of each instance"""
    N, H, W = shape
    kinds = [("blob", ""), ("noise", ""), ("empty", ""), ("full", ""), ("pixel", ""), ("blob", "/b")]
    masks = np.stack([contour_masks.random_mask(k, (H, W), tag) for k, tag in kinds])
    u = lambda tag, *s: synth.hash_uniform(257, f"{tag}/{H}x{W}", s)  # noqa: E731
    frames = 0.5 + 0.1 * np.floor(3.0 * u("steps", 2, H, W))
    frames[u("holes", 2, H, W) < 0.15] = 0.0
    return masks, frames.astype(np.float32), kinds


def _batches(n_masks, N):
    """index batches of N covering range(n_masks), the last one wrapped round"""
    return [np.arange(s, s + N) % n_masks for s in range(0, n_masks, N)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_transform_equals_the_restatement_bit_for_bit(shape):
    N, H, W = shape
    masks, frames, kinds = _hand_made(shape)
    seen = 0
    for as_bool in (False, True):
        for b in _batches(len(masks), N):
            frame = (b + int(as_bool)) % 2
            m = _dev(masks[b])
            got = _host_np(refine.contour_transform(m.bool() if as_bool else m * 255, _dev(frames), frame))
            assert got["d2"].dtype == got["nearest"].dtype == got["contour"].dtype == np.int32 and got["d2"].shape == (N, H, W)
            for k, i in enumerate(b):
                ref = SH.contour_transform(masks[i], frames[frame[k]])
                assert int(got["contour"][k]) == ref["contour"], (kinds[i], got["contour"][k], ref["contour"])
                assert np.array_equal(got["d2"][k], ref["d2"]), kinds[i]
                assert np.array_equal(got["nearest"][k], ref["nearest"]), kinds[i]
                if ref["contour"] == 0:
                    assert (got["d2"][k] == 2 ** 31 - 1).all() and (got["nearest"][k] == -1).all()
                seen += ref["contour"]
                plain = SH.observed_contour(masks[i])
                if kinds[i][0] in ("blob", "noise") and H * W >= 48:
                    assert 0 < ref["contour"] < plain.sum(), kinds[i]          # the depth rule took some of the contour away and left some
    assert seen > 0 or H * W == 1


def test_the_transform_on_the_fixtures_and_a_row_wider_than_a_tile(scenes):
    for name, sc in scenes.items():
        got = _host_np(refine.contour_transform(sc.masks_dev, sc.frames_dev, sc.inp["frame"]))
        for i in sc.rows:
            ref = SH.contour_transform(sc.masks[i], sc.frames[sc.inp["frame"][i]])
            assert int(got["contour"][i]) == ref["contour"] > 100 and np.array_equal(got["d2"][i], ref["d2"]) and np.array_equal(got["nearest"][i], ref["nearest"])
    # 2 x 2100: more columns than the row pass holds in LDS at a time (2048), contour pixels in the first and in the second tile
    m = np.zeros((1, 2, 2100), np.uint8)
    m[0, 0, [5, 6, 1000, 2047, 2048, 2099]] = 1
    m[0, 1, 2060:2070] = 1
    z = np.zeros((1, 2, 2100), np.float32)
    got = _host_np(refine.contour_transform(_dev(m), _dev(z), [0]))
    ref = SH.contour_transform(m[0], z[0])
    assert int(got["contour"][0]) == ref["contour"] == 16 and np.array_equal(got["d2"][0], ref["d2"]) and np.array_equal(got["nearest"][0], ref["nearest"])


def _check_system(got, ren, frames, frame, K, masks, what, sil_gate=8.0, dist_gate=0.02):
    counts = []
    for i in range(len(ren)):
        tr = SH.contour_transform(masks[i], frames[frame[i]])
        ref = SH.accumulate(ren[i], frames[frame[i]], K[i], tr["d2"], tr["nearest"], sil_gate, dist_gate)
        n = ref["pairs"]
        assert int(got["pairs"][i]) == n, (what, i, int(got["pairs"][i]), n)
        A, b, sq = got["A"][i], got["b"][i], float(got["sq"][i])
        assert np.array_equal(A, A.T), (what, i)
        u = 4.0 * (2 * n) * 2.0 ** -53
        eA, eb, es = np.abs(A - ref["A"]), np.abs(b - ref["b"]), abs(sq - ref["sq"])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(float(np.nanmax(eA / (u * ref["A_abs"]))) if n else 0.0, float(np.nanmax(eb / (u * ref["b_abs"]))) if n else 0.0,
                        es / (u * ref["sq"]) if ref["sq"] > 0 else 0.0)
        print(f"{what}[{i}]: pairs {n}, worst |device - host| = {worst:.3f} of 4 (2 pairs) 2^-53 sum|terms|")
        assert np.all(eA <= u * ref["A_abs"]) and np.all(eb <= u * ref["b_abs"]) and es <= u * ref["sq"], (what, i, worst)
        counts.append(n)
    return counts


def test_systems_on_the_devices_renders_equal_the_restatement(scenes):
    for name, sc in scenes.items():
        inp = sc.inp
        ren = render.render_depth(sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]), _dev(inp["K"]), sc.H, sc.W, inp["near"], inp["far"])
        got = _host_np(refine.silhouette_equations(ren, sc.masks_dev, sc.frames_dev, inp["frame"], _dev(inp["K"])))
        n = len(sc.rows)
        assert got["A"].shape == (n, 6, 6) and got["b"].shape == (n, 6) and got["sq"].shape == got["pairs"].shape == (n,)
        counts = _check_system(got, ren.cpu().numpy(), sc.frames, inp["frame"], inp["K"], sc.masks, name)
        assert min(counts) > 100
        tight = _host_np(refine.silhouette_equations(ren, sc.masks_dev, sc.frames_dev, inp["frame"], _dev(inp["K"][0]), sil_gate=2.0, dist_gate=0.01))
        fewer = _check_system(tight, ren.cpu().numpy(), sc.frames, inp["frame"], inp["K"], sc.masks, name + " gate 2", sil_gate=2.0, dist_gate=0.01)
        assert sum(fewer) < sum(counts)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_systems_on_hand_made_maps_at_the_launch_edges(shape):
    """renders that are blobs of their own a few centimetres round the frames' depths (in front of, within and behind the hidden rule's gate),
    every mask kind, a K with a skew term, a gate of 3 pixels with rendered contour on both sides of it"""
    N, H, W = shape
    masks, frames, kinds = _hand_made(shape)
    u = lambda tag, *s: synth.hash_uniform(263, f"{tag}/{N}x{H}x{W}", s)  # noqa: E731
    K = np.array([[143.1, 0.4, 0.5 * W], [0.0, 141.7, 0.5 * H], [0.0, 0.0, 1.0]])[None].repeat(N, axis=0)
    K[:, 0, 2] += np.arange(N)
    total = 0
    for b in _batches(len(masks), N):
        frame = b % 2
        cover = np.stack([contour_masks.random_mask("blob", (H, W), f"/ren{i}") for i in b]) != 0
        ren = np.where(cover, 0.6 + 0.1 * (u("z", len(masks), H, W)[b] - 0.5), 0.0).astype(np.float32)
        got = _host_np(refine.silhouette_equations(_dev(ren), _dev(masks[b]), _dev(frames), frame, _dev(K), sil_gate=3.0))
        counts = _check_system(got, ren, frames, frame, K, masks[b], f"maps {shape} {[kinds[i][0] for i in b]}", sil_gate=3.0)
        for k, i in enumerate(b):
            if kinds[i][0] in ("empty", "full"):
                assert counts[k] == 0 and not got["A"][k].any() and not got["b"][k].any() and got["sq"][k] == 0.0
        total += sum(counts)
        if H >= 35:   # pairs in the first and the last band, in the first and the last row and column
            tr = [SH.contour_transform(masks[i], frames[frame[k]]) for k, i in enumerate(b)]
            m = np.any([SH.accumulate(ren[k], frames[frame[k]], K[k], tr[k]["d2"], tr[k]["nearest"], 3.0)["mask"] for k in range(N)], axis=0)
            assert m[:16].any() and m[32:].any() and m[15:17].any()
    if H >= 35:
        assert total > 100
    if H * W == 1:
        assert total == 0


def _check_steps(sc, rows, R, t, what, **kw):
    """icp_refine_sil(iters=1) from the poses (R, t) of `rows` against the restatement's combined step on the device's renders of those poses"""
    ren = sc.render(rows, R, t)
    got = _host_np(sc.refine(rows, R, t, iters=1, **kw))
    inp = sc.inp
    weight = kw.get("sil_weight", 1.0)
    for k, row in enumerate(rows):
        frame = sc.frames[inp["frame"][row]]
        tr = SH.contour_transform(sc.masks[row], frame)
        dep = IH.accumulate(ren[k], frame, inp["K"][row])
        sil = SH.accumulate(ren[k], frame, inp["K"][row], tr["d2"], tr["nearest"])
        A, b, n = SH.combine(dep, sil, weight)
        sol = IH.solve(A, b, n)
        assert int(got["ok"][k]) == int(sol["ok"]) == 1 and int(got["iters_done"][k]) == 1, (what, row)
        assert int(got["pairs"][k]) == dep["pairs"] and int(got["sil_pairs"][k]) == sil["pairs"] > 100, (what, row)
        w = IH.log_so3(got["R"][k] @ np.asarray(R[k]).T)
        v = got["t"][k] - IH.exp_so3(w) @ np.asarray(t[k])
        xi = sol["xi"]
        terms = dep["pairs"] + 2 * sil["pairs"]
        bound = terms * 2.0 ** -50 * sol["cond"] * np.linalg.norm(xi)
        ew, ev = np.linalg.norm(w - xi[:3]), np.linalg.norm(v - xi[3:])
        print(f"{what} row {row}: |xi| {np.linalg.norm(xi):.2e}, cond {sol['cond']:.1e}, terms {terms}, |dw| {ew:.2e} |dv| {ev:.2e}, bound {bound:.2e}")
        assert ew <= bound and ev <= bound, (what, row, ew, ev, bound)
        rms, sil_rms = np.sqrt(dep["sq"] / dep["pairs"]), np.sqrt(sil["sq"] / sil["pairs"])
        assert abs(float(got["rms"][k]) - rms) <= 1e-12 * rms and abs(float(got["sil_rms"][k]) - sil_rms) <= 1e-12 * sil_rms


def test_one_step_equals_the_restatements_combined_step(scenes):
    for name, sc in scenes.items():
        _check_steps(sc, sc.rows, sc.inp["R0"], sc.inp["t0"], name)
    sc = scenes["isolated"]
    _check_steps(sc, sc.rows[:8], sc.inp["R0"][:8], sc.inp["t0"][:8], "isolated weight 0.25", sil_weight=0.25)
    # from the restatement's own poses after its iterations 1 .. 3 on the device's renders: small residuals without comparing trajectories
    rows, Rs, ts = [], [], []
    for row in (1, 7, 9):   # a start of the fronto-parallel plate, of the tilted plate and of the two-face cube
        g = int(sc.inp["target"][row])
        res = SH.refine(lambda R, t: sc.render(np.array([row]), R[None], t[None])[0], sc.inp["R0"][row], sc.inp["t0"][row], sc.inp["K"][row],
                        sc.frames[g], sc.masks[row], iters=3)
        assert res["ok"] == 1 and res["iters_done"] == 3
        for tr in res["trace"][1:] + [dict(R=res["R"], t=res["t"])]:
            rows.append(row)
            Rs.append(tr["R"])
            ts.append(tr["t"])
    _check_steps(sc, np.array(rows), np.stack(Rs), np.stack(ts), "isolated after iterations 1-3")


def test_flat_faced_objects_come_back_inside_the_bounds_that_depth_alone_leaves_untouched(scenes):
    for name, sc in scenes.items():
        inp = sc.inp
        dep, out = _host_np(sc.depth_only()), _host_np(sc.start())   # icp_refine's 10 iterations | icp_refine_sil's 20
        worst = [0.0, 0.0]
        assert len(inp["flat"]) >= 10
        for row in inp["flat"]:
            g = int(inp["target"][row])
            assert dep["ok"][row] == 0 and dep["iters_done"][row] == 0 and dep["pairs"][row] > 2000, (name, row)        # enough pairs: the matrix fails
            assert np.array_equal(dep["R"][row], inp["R0"][row]) and np.array_equal(dep["t"][row], inp["t0"][row])       # bit for bit
            re, lat = SH.lateral_errors(out["R"][row], out["t"][row], inp["R_gt"][g], inp["t_gt"][g])
            _, te = IH.pose_errors(out["R"][row], out["t"][row], inp["R_gt"][g], inp["t_gt"][g])
            print(f"{name} row {row} (gt {g}) from {inp['start_deg'][row]:g} deg / {inp['start_mm'][row]:.2f} mm: {re:.4f} deg, lateral {lat:.4f} mm (|dt| {te:.4f} mm) "
                  f"after {out['iters_done'][row]} steps, pairs {out['pairs'][row]} + {out['sil_pairs'][row]}, sil_rms {out['sil_rms'][row]:.2e} m")
            worst = [max(worst[0], lat), max(worst[1], re)]
            assert out["ok"][row] == 1 and 1 <= out["iters_done"][row] <= 20 and out["sil_pairs"][row] > 100
            assert lat <= LATERAL_MM and re <= ROTATION_DEG, (name, row, lat, re)
        print(f"{name}: worst lateral {worst[0]:.3f} mm (bound {LATERAL_MM:.2f}), worst rotation {worst[1]:.3f} deg (bound {ROTATION_DEG:.2f})")
        for row in sorted(set(sc.rows) - set(inp["flat"])):   # the cube seen on three faces: unchanged within the clean bound
            assert dep["ok"][row] == 1 and out["ok"][row] == 1
            re, te = IH.pose_errors(out["R"][row], out["t"][row], dep["R"][row], dep["t"][row])
            print(f"{name} row {row}: {re:.2e} deg, {te:.2e} mm from the depth-only result")
            assert re < CLEAN_BOUND and te < CLEAN_BOUND, (name, row, re, te)
        assert out["R"].dtype == out["t"].dtype == out["rms"].dtype == out["sil_rms"].dtype == np.float64
        assert out["ok"].dtype == out["iters_done"].dtype == out["pairs"].dtype == out["sil_pairs"].dtype == np.int32


def test_calls_are_deterministic_and_instances_independent(scenes):
    sc = scenes["occluded"]
    inp = sc.inp
    n = len(sc.rows)
    a, b = sc.start(iters=4), sc.start(iters=4)
    assert _same(a, b) is None
    for row in (0, 4, 5, 9):
        one = sc.refine(np.array([row]), inp["R0"][[row]], inp["t0"][[row]], iters=4)
        assert _same(one, a, rows=(slice(0, 1), slice(row, row + 1))) is None, row
    # a row out of the frame and a row behind the camera beside them: the others get the bits they get without them, these two keep their pose
    rows = np.concatenate([[0], sc.rows, [0]])
    R, t = inp["R0"][rows].copy(), inp["t0"][rows].copy()
    t[0] += np.array([50.0, 0.0, 0.0])
    t[-1] *= np.array([1.0, 1.0, -1.0])
    both = sc.refine(rows, R, t, iters=4)
    assert _same(both, a, rows=(slice(1, n + 1), slice(0, n))) is None
    both = _host_np(both)
    assert both["ok"][0] == both["ok"][-1] == 0 and both["pairs"][0] == both["sil_pairs"][0] == both["sil_pairs"][-1] == 0
    assert np.isnan(both["rms"][[0, -1]]).all() and np.isnan(both["sil_rms"][[0, -1]]).all()
    assert np.array_equal(both["R"][[0, -1]], R[[0, -1]]) and np.array_equal(both["t"][[0, -1]], t[[0, -1]])
    args = (sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]))
    kw = dict(iters=4, near=inp["near"], far=inp["far"])
    shared = refine.icp_refine_sil(*args, _dev(inp["K"][0]), sc.frames_dev, _dev(inp["frame"]), sc.masks_dev.bool(), **kw)   # one K; a bool mask
    assert _same(shared, a) is None
    start = _dev(inp["R0"])
    again = refine.icp_refine_sil(sc.meshes, inp["labels"], start, _dev(inp["t0"]), _dev(inp["K"]), sc.frames_dev, inp["frame"], sc.masks_dev * 7, **kw)
    assert torch.equal(start, _dev(inp["R0"])) and _same(again, a) is None                       # the caller's tensors stay; nonzero = object
    z = _host_np(sc.start(iters=0))
    assert np.array_equal(z["R"], inp["R0"]) and np.array_equal(z["t"], inp["t0"]) and list(z["ok"]) == [1] * n and not z["iters_done"].any()
    assert not z["pairs"].any() and not z["sil_pairs"].any() and np.isnan(z["rms"]).all() and np.isnan(z["sil_rms"]).all()


def test_no_rows_give_empty_tensors_and_arguments_are_checked_before_any_launch(scenes):
    sc = scenes["isolated"]
    inp = sc.inp
    R0, t0, K = _dev(inp["R0"]), _dev(inp["t0"]), _dev(inp["K"])
    out = refine.icp_refine_sil(sc.meshes, [], R0[:0], t0[:0], K[:0], sc.frames_dev, [], sc.masks_dev[:0])
    assert out["R"].shape == (0, 3, 3) and out["t"].shape == (0, 3) and all(out[k].shape == (0,) for k in KEYS[2:])
    tr = refine.contour_transform(sc.masks_dev[:0], sc.frames_dev, [])
    assert tr["d2"].shape == tr["nearest"].shape == (0, sc.H, sc.W) and tr["contour"].shape == (0,)
    ne = refine.silhouette_equations(torch.zeros(0, sc.H, sc.W, device=DEV), sc.masks_dev[:0], sc.frames_dev, [], K[:0])
    assert ne["A"].shape == (0, 6, 6) and ne["b"].shape == (0, 6) and ne["sq"].shape == (0,) and ne["pairs"].shape == (0,)
    with pytest.raises(ValueError, match="mask_obs"):
        refine.icp_refine_sil(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev, inp["frame"], sc.masks_dev[:3])
    with pytest.raises(ValueError, match="mask_obs"):
        refine.icp_refine_sil(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev, inp["frame"], sc.masks_dev.float())
    with pytest.raises(ValueError, match="differ in H, W"):
        refine.icp_refine_sil(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev, inp["frame"], sc.masks_dev[:, :, :-1])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        refine.icp_refine_sil(sc.meshes, inp["labels"], R0, t0, K, sc.frames_dev, inp["frame"], sc.masks_dev.cpu())
    with pytest.raises(ValueError, match="frame"):
        refine.contour_transform(sc.masks_dev, sc.frames_dev, [0] * 15 + [4])
    with pytest.raises(ValueError, match="mask_obs"):
        refine.silhouette_equations(torch.zeros(2, sc.H, sc.W, device=DEV), sc.masks_dev[:3], sc.frames_dev, [0, 0], K[:2])
    torch.cuda.synchronize()


def test_refine_rgbd_without_a_mask_is_todays_call_and_with_one_runs_the_term(scenes):
    sc = scenes["isolated"]
    inp = sc.inp
    args = (sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]), _dev(inp["K"]), sc.frames_dev, inp["frame"])
    kw = dict(near=inp["near"], far=inp["far"])
    align = refine.depth_align(*args, **kw)
    today = refine.icp_refine(sc.meshes, inp["labels"], args[2], align["t"], args[4], sc.frames_dev, inp["frame"], **kw)
    got = refine.refine_rgbd(*args, **kw)
    assert _same(got, today, keys=KEYS[:6]) is None and "sil_pairs" not in got and torch.equal(_bits(got["align"]["t"]), _bits(align["t"]))
    assert not bool(got["ok"][:12].any()) and bool(got["ok"][12:].all())
    want = refine.icp_refine_sil(sc.meshes, inp["labels"], args[2], align["t"], args[4], sc.frames_dev, inp["frame"], sc.masks_dev, iters=10, **kw)
    with_mask = refine.refine_rgbd(*args, mask_obs=sc.masks_dev, **kw)
    assert _same(with_mask, want) is None and bool(with_mask["ok"].all()) and torch.equal(_bits(with_mask["align"]["t"]), _bits(align["t"]))
    gated = refine.refine_rgbd(*args, mask_obs=sc.masks_dev, sil_gate=2.0, sil_weight=0.5, **kw)
    want = refine.icp_refine_sil(sc.meshes, inp["labels"], args[2], align["t"], args[4], sc.frames_dev, inp["frame"], sc.masks_dev, iters=10, sil_gate=2.0,
                                 sil_weight=0.5, **kw)
    assert _same(gated, want) is None and _same(gated, with_mask) is not None


def test_nothing_is_written_outside_the_outputs_and_the_workspace(scenes):
    """the entry points on buffers with a guard band on both sides, filled with a sentinel: the bands are unchanged, the payload is the wrapper's,
    and what the workspace held before the call does not matter"""
    lib, G = cabi.load(), 64
    sc = scenes["occluded"]
    inp = sc.inp
    N, H, W, F = len(sc.rows), sc.H, sc.W, inp["num_frames"]
    stream = devargs.stream(torch.device(DEV))
    K, lab, fr = _dev(inp["K"]), _dev(inp["labels"], torch.int32), _dev(inp["frame"], torch.int32)
    lab_host, fr_host = inp["labels"].astype(np.int32), inp["frame"].astype(np.int32)
    ren = render.render_depth(sc.meshes, inp["labels"], _dev(inp["R0"]), _dev(inp["t0"]), K, H, W, inp["near"], inp["far"])
    ws_doubles = int(lib.gdrn_sil_workspace_bytes(N, H, W) + 7) // 8
    assert ws_doubles * 8 >= 3 * N * H * W * 4 + N * H * W

    def banded(n, dtype, fill):
        return torch.full((G + n + G,), fill, dtype=dtype, device=DEV)

    def intact(bufs, fills, what):
        torch.cuda.synchronize()
        for k, b in bufs.items():
            f = torch.full((G,), fills[k], dtype=b.dtype, device=DEV)
            assert torch.equal(_bits(b[:G]), _bits(f)) and torch.equal(_bits(b[-G:]), _bits(f)), (what, k)

    def pointers(bufs):
        return {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}

    tr_ref = refine.contour_transform(sc.masks_dev, sc.frames_dev, inp["frame"])
    ne_ref = refine.silhouette_equations(ren, sc.masks_dev, sc.frames_dev, inp["frame"], K)
    dep_ref = refine.normal_equations(ren, sc.frames_dev, inp["frame"], K)
    iu = torch.triu_indices(6, 6, device=DEV)
    pack = lambda ne: torch.cat([ne["A"][:, iu[0], iu[1]], ne["b"], ne["sq"][:, None]], dim=1).contiguous()  # noqa: E731
    for ws_fill in (float("nan"), -7.25):
        fills = dict(d2=-77, nearest=-77, contour=-77, ws=ws_fill)
        bufs = dict(d2=banded(N * H * W, torch.int32, -77), nearest=banded(N * H * W, torch.int32, -77), contour=banded(N, torch.int32, -77),
                    ws=banded(ws_doubles, torch.float64, ws_fill))
        ptr = pointers(bufs)
        cabi.check(lib.gdrn_sil_contour_transform(sc.masks_dev.data_ptr(), sc.frames_dev.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, N, H, W, ptr["d2"],
                                                  ptr["nearest"], ptr["contour"], ptr["ws"], stream), "sil_contour_transform")
        intact(bufs, fills, "transform")
        assert torch.equal(bufs["d2"][G:-G].view(N, H, W), tr_ref["d2"]) and torch.equal(bufs["nearest"][G:-G].view(N, H, W), tr_ref["nearest"])
        assert torch.equal(bufs["contour"][G:-G], tr_ref["contour"])
        fills = dict(sys=-7.25, pairs=-77, ws=ws_fill)
        bufs = dict(sys=banded(N * 28, torch.float64, -7.25), pairs=banded(N, torch.int32, -77), ws=banded(ws_doubles, torch.float64, ws_fill))
        ptr = pointers(bufs)
        cabi.check(lib.gdrn_sil_accumulate(ren.data_ptr(), sc.frames_dev.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, K.data_ptr(), tr_ref["d2"].data_ptr(),
                                           tr_ref["nearest"].data_ptr(), N, H, W, 8.0, 0.02, ptr["sys"], ptr["pairs"], ptr["ws"], stream), "sil_accumulate")
        intact(bufs, fills, "accumulate")
        assert torch.equal(_bits(bufs["sys"][G:-G].view(N, 28)), _bits(pack(ne_ref))) and torch.equal(bufs["pairs"][G:-G], ne_ref["pairs"])
    # one combined step from the combined systems: the pose of icp_refine_sil(iters=1)
    want = sc.start(iters=1, sil_weight=0.5)
    fills = dict(R=-7.25, t=-7.25, state=-77)
    bufs = dict(R=banded(N * 9, torch.float64, -7.25), t=banded(N * 3, torch.float64, -7.25), state=banded(N * 2, torch.int32, -77))
    bufs["R"][G:-G] = _dev(inp["R0"]).reshape(-1)
    bufs["t"][G:-G] = _dev(inp["t0"]).reshape(-1)
    bufs["state"][G:-G] = 0
    ptr = pointers(bufs)
    sys_d, sys_s = pack(dep_ref), pack(ne_ref)
    cabi.check(lib.gdrn_icp_step_sil(sys_d.data_ptr(), dep_ref["pairs"].data_ptr(), sys_s.data_ptr(), ne_ref["pairs"].data_ptr(), 0.5, N, 64, ptr["R"], ptr["t"],
                                     ptr["state"], stream), "icp_step_sil")
    intact(bufs, fills, "step")
    assert torch.equal(_bits(bufs["R"][G:-G].view(N, 3, 3)), _bits(want["R"])) and torch.equal(_bits(bufs["t"][G:-G].view(N, 3)), _bits(want["t"]))
    state = bufs["state"][G:-G].view(N, 2)
    assert torch.equal(state[:, 1], want["iters_done"]) and bool((state[:, 1] == 1).all())
    # the whole loop
    want = sc.start(iters=3)
    tb = sc.meshes.on(torch.device(DEV))
    outs = []
    for ws_fill in (float("nan"), 3.0e300):
        fills = dict(R=-7.25, t=-7.25, scratch=-7.25, ok=-77, iters_done=-77, pairs=-77, rms=-7.25, sil_pairs=-77, sil_rms=-7.25, ws=ws_fill)
        bufs = dict(R=banded(N * 9, torch.float64, -7.25), t=banded(N * 3, torch.float64, -7.25), scratch=banded(N * H * W, torch.float32, -7.25),
                    ok=banded(N, torch.int32, -77), iters_done=banded(N, torch.int32, -77), pairs=banded(N, torch.int32, -77),
                    rms=banded(N, torch.float64, -7.25), sil_pairs=banded(N, torch.int32, -77), sil_rms=banded(N, torch.float64, -7.25),
                    ws=banded(ws_doubles, torch.float64, ws_fill))
        bufs["R"][G:-G] = _dev(inp["R0"]).reshape(-1)
        bufs["t"][G:-G] = _dev(inp["t0"]).reshape(-1)
        ptr = pointers(bufs)
        p = cabi.ptr
        cabi.check(lib.gdrn_icp_refine_sil(p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]),
                                           sc.meshes.num_classes, sc.meshes.f_max, lab.data_ptr(), lab_host.ctypes.data, ptr["R"], ptr["t"], K.data_ptr(), N,
                                           sc.frames_dev.data_ptr(), fr.data_ptr(), fr_host.ctypes.data, F, sc.masks_dev.data_ptr(), H, W, inp["near"],
                                           inp["far"], 3, 0.02, 0.01, 64, 1.0, 8.0, ptr["scratch"], ptr["ok"], ptr["iters_done"], ptr["pairs"], ptr["rms"],
                                           ptr["sil_pairs"], ptr["sil_rms"], ptr["ws"], stream), "icp_refine_sil")
        intact(bufs, fills, "refine")
        got = dict(R=bufs["R"][G:-G].view(N, 3, 3), t=bufs["t"][G:-G].view(N, 3), ok=bufs["ok"][G:-G], iters_done=bufs["iters_done"][G:-G],
                   pairs=bufs["pairs"][G:-G], rms=bufs["rms"][G:-G], sil_pairs=bufs["sil_pairs"][G:-G], sil_rms=bufs["sil_rms"][G:-G])
        assert _same(got, want) is None, _same(got, want)
        outs.append(bufs["scratch"][G:-G].clone())
    assert torch.equal(outs[0], outs[1]) and not bool((outs[0] == -7.25).any())
