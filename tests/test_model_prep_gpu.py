"""GPU tests of the model preparation (csrc/model_prep.hip through gdrnet_amd.model_prep) against the naive host restatement
(tests/model_prep_host.py) and golden G16 (the reference's own outputs).  The comparison is EXACT equality for the farthest-point-sampling (FPS)
indices and points, the largest squared distance, the diameter, minimum, maximum, extents and box corners; the mean is held to
n 2^-52 max|x| of the math.fsum mean, the bound of a sum in any order."""
import math
import os

import numpy as np
import pytest
import torch

import model_prep_host as MH
from gdrnet_amd import cabi, model_prep as MP, pose_metrics, roi_data, synth
from gdrnet_amd.cfg import lm13_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG_MAX = 16384   # FPS_REG_MAX of csrc/model_prep.hip: up to here an object's points and running minima stay in registers, beyond in the workspace
TILE = 512        # DM_TILE: the tile side of the diameter kernel
PAD = 1.0e6       # fills the packed rows beyond an object's own points: far outside every cloud, so a padding row that entered would win
_cache = {}


def g16():
    if "g16" not in _cache:
        _cache["g16"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "g16_model_prep.npz")))
    return _cache["g16"]


def cloud(n, tag="c"):
    """n points uniform in the 0.12 x 0.08 x 0.2 m box, fp64; computed once"""
    key = ("cloud", n, tag)
    if key not in _cache:
        _cache[key] = (synth.hash_uniform(synth.MODEL_PREP_SEED, f"gpu/{tag}/{n}", (n, 3)) - 0.5) * synth.MODEL_PREP_BOX
    return _cache[key]


def host_fps(pts, K, key):
    """the restatement's indices at K, computed once per cloud at the largest K asked for so far (a prefix serves the smaller ones)"""
    have = _cache.get(("fps", key))
    if have is None or len(have) < K:
        have = _cache[("fps", key)] = MH.fps_indices(pts, K)
    return have[:K]


def check(prep, clouds, keys, K, diameter=True):
    assert prep.fps_indices.shape == (len(clouds), K) and prep.fps_indices.dtype == np.int32
    for c, (p, key) in enumerate(zip(clouds, keys)):
        idx = host_fps(p, K, key)
        assert np.array_equal(prep.fps_indices[c], idx), (key, K, int(np.argmax(prep.fps_indices[c] != idx)))
        assert np.array_equal(prep.fps_points(K)[c], p.astype(np.float32)[idx].astype(np.float64)), key
        lo, hi, mean = MH.bounds(p)
        assert np.array_equal(prep.bounds_min[c], lo) and np.array_equal(prep.bounds_max[c], hi), key
        assert np.array_equal(prep.extents[c], MH.extents(p)) and np.array_equal(prep.bbox3d_and_center[c][:8], MH.bbox3d_and_center(p)[:8]), key
        err, bound = np.abs(prep.centers[c] - MH.fsum_mean(p)), MH.mean_bound(p)
        assert np.all(err <= bound), (key, err, bound)
        if diameter:
            want = MH.max_sq_dist(p)
            assert prep.max_sq_dist[c] == want and prep.diameters[c] == math.sqrt(want), (key, prep.max_sq_dist[c], want)


# ---- FPS -----------------------------------------------------------------------------------------------------------------
FPS_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 1029)   # a wave +- 1, the workgroup's 1024 threads +- 1, and a ragged second register row


@pytest.mark.parametrize("K", [1, 8, 64, 256])
def test_fps_point_and_iteration_counts(K):
    """one batch of all the counts (so every object but the largest has padding behind it); K = 64 and 256 exceed the smaller objects' counts"""
    clouds = [cloud(n) for n in FPS_COUNTS]
    prep = MP.prepare_models(clouds, num_fps=K, device=DEV, pad_value=PAD)
    check(prep, clouds, FPS_COUNTS, K)
    if K > 1:
        assert not prep.fps_indices[0].any() and not prep.fps_indices[1, 63:].any()   # beyond the object's points: index 0


def test_reference_cases_ties_and_degenerate_clouds():
    g = g16()
    cases = [c for c in synth.MODEL_PREP_CASES if c != "rand70000"]
    clouds = [synth.make_model_prep_inputs(c) for c in cases]
    prep = MP.prepare_models(clouds, device=DEV, pad_value=PAD)
    assert prep.num_fps == MP.NUM_FPS
    for c, case in enumerate(cases):
        assert np.array_equal(prep.fps_indices[c], g[f"{case}/fps"]), case
        assert prep.diameters[c] == float(g[f"{case}/diameter"]), case
        assert np.array_equal(prep.extents[c], g[f"{case}/extents"]) and np.array_equal(prep.bbox3d_and_center[c][:8], g[f"{case}/bbox"][:8]), case
        assert np.all(np.abs(prep.centers[c] - g[f"{case}/mean"]) <= MH.mean_bound(clouds[c])), case
    grid = prep.fps_indices[cases.index("grid125")]
    assert grid[:8].tolist() == [0, 4, 20, 24, 100, 104, 120, 124]        # eight corners at one distance: the lowest index first
    assert 62 not in grid.tolist() and len(set(grid[:124].tolist())) == 124 and not grid[124:].any()   # the point on the box centre is never chosen
    rep = prep.fps_indices[cases.index("repeat20")]
    assert sorted(rep[:5].tolist()) == [0, 1, 2, 3, 4] and not rep[5:].any()                            # K beyond the distinct points: index 0
    check(prep, clouds, cases, 256)


def test_fps_mixed_batch_and_winner_placement():
    """an object of 1 point beside one of 5000; an object whose outlier is its LAST valid point (padding right behind it) and one whose outlier
    is point 0: box centre + outlier put that point among the first two picks"""
    last, first = cloud(1500, "last").copy(), cloud(1029, "first").copy()
    last[-1] = (1.0, 0.3, -0.2)
    first[0] = (-0.7, 1.0, 0.4)
    clouds, keys = [cloud(1, "one"), cloud(5000), last, first], ("one", 5000, "last", "first")
    prep = MP.prepare_models(clouds, num_fps=(8, 64), device=DEV, pad_value=PAD)
    check(prep, clouds, keys, 64)
    assert not prep.fps_indices[0].any()
    assert 1499 in prep.fps_indices[2, :2].tolist() and 0 in prep.fps_indices[3, :2].tolist()
    assert prep.fps_indices.max() < 5000 and all(prep.fps_indices[c].max() < len(p) for c, p in enumerate(clouds))
    again = MP.prepare_models(clouds, num_fps=(8, 64), device=DEV, pad_value=-PAD)   # a second call: identical, whatever the padding holds
    assert np.array_equal(again.fps_indices, prep.fps_indices) and np.array_equal(again.fps_xyz, prep.fps_xyz)
    assert np.array_equal(again.max_sq_dist, prep.max_sq_dist)


def test_fps_on_each_side_of_the_register_limit():
    clouds = [cloud(REG_MAX), cloud(REG_MAX + 1), cloud(REG_MAX - 1023)]   # the last register row full | one point in the workspace path | ragged
    prep = MP.prepare_models(clouds, num_fps=64, diameter=False, device=DEV, pad_value=PAD)
    check(prep, clouds, (REG_MAX, REG_MAX + 1, REG_MAX - 1023), 64, diameter=False)
    assert prep.max_sq_dist is None


def test_large_cloud_matches_the_reference():
    """70 000 points, K = 256, the workspace path: the reference's own indices and diameter (golden G16)"""
    g, pts = g16(), synth.make_model_prep_inputs("rand70000")
    prep = MP.prepare_models([pts, cloud(65)], device=DEV, pad_value=PAD)
    assert np.array_equal(prep.fps_indices[0], g["rand70000/fps"])
    assert prep.diameters[0] == float(g["rand70000/diameter"])
    assert np.array_equal(prep.extents[0], g["rand70000/extents"]) and np.array_equal(prep.bbox3d_and_center[0][:8], g["rand70000/bbox"][:8])
    assert np.all(np.abs(prep.centers[0] - g["rand70000/mean"]) <= MH.mean_bound(pts))
    check(prep, [pts, cloud(65)], ("rand70000", 65), 256, diameter=False)
    assert prep.max_sq_dist[1] == MH.max_sq_dist(cloud(65))


# ---- diameter ------------------------------------------------------------------------------------------------------------
def test_diameter_point_counts():
    """1 (0.0), 2, one tile, one tile + 1 (two tiles: an even count), 1029 (three), 2000 (four), 8209 (seventeen) in one batch"""
    counts = (1, 2, TILE, TILE + 1, 1029, 2000)
    clouds = [cloud(n) for n in counts] + [synth.make_model_prep_inputs("rand8209")]
    prep = MP.prepare_models(clouds, num_fps=1, device=DEV, pad_value=PAD)
    check(prep, clouds, counts + ("rand8209",), 1)
    assert prep.diameters[0] == 0.0 and prep.diameters[6] == float(g16()["rand8209/diameter"])
    d = clouds[1][0] - clouds[1][1]
    assert prep.max_sq_dist[1] == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


@pytest.mark.parametrize("i, j", [(10, 20), (3, 1597), (0, 1599), (600, 1100)])
def test_diameter_placement_of_the_farthest_pair(i, j):
    """1600 points = four tiles (the even count, where opposite tiles meet once): both ends in one tile | in the first and the last tile |
    at (0, n - 1) | in the two middle tiles.  A shorter object beside it, padded with a value far outside."""
    pts = cloud(1600, "pair").copy()
    pts[i], pts[j] = (1.0, 1.0, 1.0), (-1.0, -1.0, -1.0)
    prep = MP.prepare_models([cloud(700, "short"), pts], num_fps=1, device=DEV, pad_value=PAD)
    assert prep.max_sq_dist[1] == 12.0 and prep.diameters[1] == math.sqrt(12.0)
    assert prep.max_sq_dist[0] == MH.max_sq_dist(cloud(700, "short")) < 0.1


# ---- downstream and the C ABI ----------------------------------------------------------------------------------------------
def test_tables_feed_the_cropper_and_the_metrics():
    """extents and fps_points(64) into RoiCropper, diameters into ModelTable: the same targets and recall table as with the restatement's values"""
    d = synth.make_roi_frames(6)
    ncls = len(d["extents"])
    clouds = [cloud(300 + 37 * c, "roi") * (d["extents"][c].astype(np.float64) / synth.MODEL_PREP_BOX) for c in range(ncls)]
    prep = MP.prepare_models(clouds, num_fps=(64,), device=DEV)
    host_ext = np.stack([MH.extents(p) for p in clouds])
    host_fps_pts = np.stack([MH.fps_points(p, 64) for p in clouds])
    frames = [torch.from_numpy(f).to(DEV) for f in d["frames"]]
    rois = []
    for r in d["rois"]:
        q = dict(r, image=frames[r["frame"]], xyz_crop=torch.from_numpy(r["xyz_crop"]).to(DEV), segmentation=torch.from_numpy(r["segmentation"]).to(DEV),
                 mask_trunc=None if r["mask_trunc"] is None else torch.from_numpy(r["mask_trunc"]).to(DEV))
        rois.append(q)
    cfg = lm13_cfg(device=DEV)
    a = roi_data.RoiCropper(cfg, extents=prep.extents, fps_points=prep.fps_points(64), device=DEV)(rois, train=True)
    b = roi_data.RoiCropper(cfg, extents=host_ext, fps_points=host_fps_pts, device=DEV)(rois, train=True)
    torch.cuda.synchronize()
    for k in ("roi_region", "roi_xyz", "roi_mask_obj"):
        assert torch.equal(a[k], b[k]), k
    assert int((a["roi_region"] > 0).sum()) > 1000
    inp = synth.make_pose_metric_inputs("A")
    pp = MP.prepare_models(inp["points"], num_fps=1, device=DEV)
    host_diam = np.array([MH.diameter(p) for p in inp["points"]])
    assert np.array_equal(pp.diameters, host_diam)
    poses = [torch.from_numpy(inp[k]).to(DEV) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    errs = [pose_metrics.pose_errors(pose_metrics.ModelTable(inp["points"], dm, inp["sym_infos"], inp["sym_classes"]), *poses, inp["labels"])["err"]
            for dm in (pp.diameters, host_diam)]
    assert torch.equal(errs[0], errs[1])


def test_c_abi_argument_errors_return_before_any_launch():
    lib, p = cabi.load(), cabi.ptr
    host = np.array([40, 7], dtype=np.int32)
    pts = torch.zeros(2, 40, 3, dtype=torch.float64, device=DEV)
    npts = torch.from_numpy(host).to(DEV)
    bounds = torch.full((2, 9), 7.0, dtype=torch.float64, device=DEV)
    max_sq = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((2, 8), 7, dtype=torch.int32, device=DEV)
    xyz = torch.full((2, 8, 3), 7.0, dtype=torch.float64, device=DEV)

    def calls(P=p(pts), N=p(npts), H=host.ctypes.data, C=2, n_max=40, K=8, fps_only=False):
        fps = lib.gdrn_model_fps(P, N, H, C, n_max, K, p(idx), p(xyz), None, None)
        return (fps,) if fps_only else (lib.gdrn_model_bounds(P, N, H, C, n_max, p(bounds), None), lib.gdrn_model_diameter(P, N, H, C, n_max, p(max_sq), None), fps)

    bad = np.array([40, 0], dtype=np.int32)
    for kw in (dict(P=None), dict(N=None), dict(H=None), dict(C=0), dict(n_max=0), dict(n_max=39), dict(H=bad.ctypes.data), dict(K=0, fps_only=True),
               dict(K=-3, fps_only=True)):
        assert set(calls(**kw)) == {-1}, kw
    assert set(calls(n_max=715827883)) == {-2}
    assert lib.gdrn_model_bounds(p(pts), p(npts), host.ctypes.data, 2, 40, None, None) == -1
    assert lib.gdrn_model_diameter(p(pts), p(npts), host.ctypes.data, 2, 40, None, None) == -1
    assert lib.gdrn_model_fps(p(pts), p(npts), host.ctypes.data, 2, 40, 8, None, p(xyz), None, None) == -1
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((bounds == 7.0).all()) and bool((max_sq == 7.0).all()) and bool((idx == 7).all()) and bool((xyz == 7.0).all())
    with pytest.raises(cabi.GdrnHipError):
        MP.prepare_models([np.zeros((4, 3))], device="cpu")
    assert calls() == (0, 0, 0)
    torch.cuda.synchronize()
    assert bool((idx == 0).all()) and bool((max_sq == 0.0).all()) and bool((bounds == 0.0).all())   # all-zero clouds
