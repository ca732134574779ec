"""CPU tests (-m "not gpu") of gdrnet_amd.model_prep: the host restatement (tests/model_prep_host.py) against golden G16 -- the reference's own
farthest-point-sampling (FPS) indices, diameters and boxes on the clouds of synth.make_model_prep_inputs -- exactly; ModelPrep's host-side views;
the argument errors; the C-ABI symbols and their host-only checks."""
import math
import os

import numpy as np
import pytest
import torch

import model_prep_host as MH
from gdrnet_amd import cabi, model_prep as MP, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdrn_model_prep_workspace_bytes", "gdrn_model_bounds", "gdrn_model_fps", "gdrn_model_diameter")
PAIRWISE_MAX = 8209   # the restatement's O(n^2) diameter stays quick up to here; the 70 000-point cloud's is compared on the device
_g16 = {}


def g16():
    if not _g16:
        _g16.update(np.load(os.path.join(ROOT, "tests", "golden", "g16_model_prep.npz")))
    return _g16


def host_prep(clouds, num_fps=MP.NUM_FPS, diameter=True):
    """a ModelPrep from the host restatement's values: what prepare_models returns, without a device"""
    clouds, num_fps = MP.check_models(clouds, num_fps)
    K = num_fps[-1]
    b = [MH.bounds(p) for p in clouds]
    return MP.ModelPrep([x[0] for x in b], [x[1] for x in b], [x[2] for x in b], [MH.fps_indices(p, K) for p in clouds],
                        [MH.fps_points(p, K) for p in clouds], num_fps, [MH.max_sq_dist(p) for p in clouds] if diameter else None)


# ---- the restatement against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", synth.MODEL_PREP_CASES)
def test_restatement_equals_the_reference(case):
    g, pts = g16(), synth.make_model_prep_inputs(case)
    assert int(g["K"]) == 256 and int(g["seed"]) == synth.MODEL_PREP_SEED
    idx = MH.fps_indices(pts, 256)
    assert idx.dtype == np.int32 and np.array_equal(idx, g[f"{case}/fps"])
    for k in (1, 8, 64):
        assert np.array_equal(MH.fps_indices(pts, k), idx[:k])
    if len(pts) <= PAIRWISE_MAX:
        assert MH.diameter(pts) == float(g[f"{case}/diameter"])
    assert np.array_equal(MH.extents(pts), g[f"{case}/extents"]) and g[f"{case}/extents"].dtype == np.float32
    box = MH.bbox3d_and_center(pts)
    assert box.dtype == np.float32 and np.array_equal(box[:8], g[f"{case}/bbox"][:8])
    assert np.array_equal(MH.bounds(pts)[2], g[f"{case}/mean"]) and np.array_equal(box[8], g[f"{case}/bbox"][8])
    assert np.all(np.abs(g[f"{case}/mean"] - MH.fsum_mean(pts)) <= MH.mean_bound(pts))


def test_the_cases_hold_what_they_are_for():
    g = g16()
    grid = synth.make_model_prep_inputs("grid125")
    centre = int(np.nonzero((grid == 0).all(axis=1))[0][0])
    assert centre == 62 and centre not in g["grid125/fps"][:124].tolist()      # the point on the box centre has distance 0 from the start
    assert sorted(g["grid125/fps"][:8].tolist()) == [0, 4, 20, 24, 100, 104, 120, 124] and g["grid125/fps"][:8].tolist() == sorted(g["grid125/fps"][:8])
    assert len(set(g["repeat20/fps"][:5].tolist())) == 5 and max(g["repeat20/fps"][:5]) < 5 and not g["repeat20/fps"][5:].any()
    assert not g["single/fps"].any() and float(g["single/diameter"]) == 0.0
    assert float(g["grid125/diameter"]) == math.sqrt(3.0)
    p = synth.make_model_prep_inputs("rand1000")
    assert not np.array_equal(p, p.astype(np.float32).astype(np.float64))       # fp64 values: the fp32 rounding is part of the case
    w = synth.make_model_prep_workload()
    assert [len(x) for x in w] == [16008] * 21 + [259854]


# ---- ModelPrep -----------------------------------------------------------------------------------------------------------
def test_views_follow_the_reference_layouts():
    g = g16()
    cases = ("rand1000", "grid125", "repeat20", "single")
    clouds = [synth.make_model_prep_inputs(c) for c in cases]
    prep = host_prep(clouds)
    assert prep.num_classes == 4 and prep.num_fps == MP.NUM_FPS
    assert prep.extents.dtype == np.float32 and prep.extents.shape == (4, 3)
    assert prep.bbox3d_and_center.dtype == np.float32 and prep.bbox3d_and_center.shape == (4, 9, 3)
    assert prep.diameters.dtype == np.float64 and prep.fps_indices.dtype == np.int32 and prep.fps_indices.shape == (4, 256)
    for c, case in enumerate(cases):
        assert np.array_equal(prep.extents[c], g[f"{case}/extents"]) and np.array_equal(prep.bbox3d_and_center[c], g[f"{case}/bbox"])
        assert prep.diameters[c] == float(g[f"{case}/diameter"]) and np.array_equal(prep.fps_indices[c], g[f"{case}/fps"])
    full = prep.fps_points(256)
    assert full.shape == (4, 256, 3) and full.dtype == np.float64
    for k in MP.NUM_FPS:   # the prefix property
        assert np.array_equal(prep.fps_points(k), full[:, :k])
        wc = prep.fps_points(k, with_center=True)
        assert wc.shape == (4, k + 1, 3) and np.array_equal(wc[:, :k], full[:, :k]) and np.array_equal(wc[:, k], prep.centers)
    # the values are the fp32-rounded vertices, held in float64: get_fps_and_center's np.concatenate of the fp32 points with the fp64 mean
    assert np.array_equal(full[0], clouds[0].astype(np.float32)[g["rand1000/fps"]].astype(np.float64))
    d = prep.fps_dict([1, 5, 6, 15])
    assert list(d) == ["1", "5", "6", "15"]
    for c, o in enumerate(d):
        assert list(d[o]) == [f"fps{k}_and_center" for k in (4, 8, 12, 16, 20, 32, 64, 128, 256)]
        for k in MP.NUM_FPS:
            e = d[o][f"fps{k}_and_center"]
            assert e.shape == (k + 1, 3) and e.dtype == np.float64 and np.array_equal(e[:k], full[c, :k]) and np.array_equal(e[k], prep.centers[c])
    with pytest.raises(ValueError):
        prep.fps_dict([1, 2, 3])
    for k in (0, 257):
        with pytest.raises(ValueError):
            prep.fps_points(k)
    few = host_prep(clouds[:1], num_fps=(8, 4, 8), diameter=False)
    assert few.num_fps == (4, 8) and few.fps_indices.shape == (1, 8) and list(few.fps_dict(["7"])["7"]) == ["fps4_and_center", "fps8_and_center"]
    with pytest.raises(ValueError):
        few.diameters


def test_argument_errors():
    ok = synth.make_model_prep_inputs("repeat20")
    for bad in ([ok, np.zeros((0, 3))], [np.zeros((4, 2))], [np.zeros(3)], [np.zeros((2, 3, 1))], [], [np.array([[0.0, np.nan, 0.0]])],
                [np.array([[0.0, 1e39, 0.0]])]):
        with pytest.raises(ValueError):
            MP.prepare_models(bad)
    for num in ((4, 0), (), 0, (-1,)):
        with pytest.raises(ValueError):
            MP.prepare_models([ok], num_fps=num)
    with pytest.raises(NotImplementedError, match="init_center"):
        MP.prepare_models([ok], init_center=False)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        MP.prepare_models([ok], device="cpu")
    with pytest.raises(cabi.GdrnHipError):
        MP.prepare_models([torch.from_numpy(ok)], device=torch.device("cpu"))
    src = open(MP.__file__).read()
    assert "model_prep_host" not in src


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_by_both_builds():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NAMES:
            assert name in cabi.EXPORTS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "#define GDRN_ABI_VERSION 5" in header
    from gdrnet_amd import build

    assert "model_prep.hip" in build.SOURCES


def test_workspace_query():
    lib = cabi.load()
    q = lib.gdrn_model_prep_workspace_bytes
    assert q(22, 16384, 256) == 0                        # the register path needs none
    assert q(22, 16385, 256) == 22 * 16385 * 16          # x, y, z, running minimum per point
    assert q(1, 1, 1) == 0
    for bad in ((0, 100, 8), (-1, 100, 8), (1, 0, 8), (1, 100, 0), (1, -5, 8), (1, 715827883, 8), (70000, 100, 8)):
        assert q(*bad) == -1, bad
    assert q(1, 715827882, 8) == 715827882 * 16          # n_max * 3 = 2^31 - 2


def test_entry_points_check_arguments_before_touching_a_device():
    """every call below returns from the host-side checks: nothing is launched (there is no device where this runs)"""
    lib = cabi.load()
    PTS, NP, OUT, XYZ, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (pointers are only compared with NULL here)
    host = np.array([100, 7], dtype=np.int32)
    H = host.ctypes.data

    def calls(pts=PTS, npts=NP, npts_host=H, C=2, n_max=100, K=8, out=OUT, ws=WS):
        return (lib.gdrn_model_bounds(pts, npts, npts_host, C, n_max, out, None), lib.gdrn_model_diameter(pts, npts, npts_host, C, n_max, out, None),
                lib.gdrn_model_fps(pts, npts, npts_host, C, n_max, K, out, XYZ, ws, None))

    for kw in (dict(pts=None), dict(npts=None), dict(npts_host=None), dict(out=None), dict(C=0), dict(C=-2), dict(n_max=0), dict(n_max=99),
               dict(npts_host=np.array([100, 0], dtype=np.int32).ctypes.data), dict(npts_host=np.array([-1, 7], dtype=np.int32).ctypes.data)):
        assert calls(**kw) == (-1, -1, -1), kw
    for K in (0, -1):
        assert lib.gdrn_model_fps(PTS, NP, H, 2, 100, K, OUT, XYZ, WS, None) == -1
    big = np.array([100, 7], dtype=np.int32)
    assert calls(npts_host=big.ctypes.data, n_max=715827883) == (-2, -2, -2)          # n_max * 3 >= 2^31
    many = np.ones(70000, dtype=np.int32)
    assert calls(npts_host=many.ctypes.data, C=70000) == (-2, -2, -2)
    large = np.array([16385, 7], dtype=np.int32)                                      # beyond the register path: the workspace is needed
    assert lib.gdrn_model_fps(PTS, NP, large.ctypes.data, 2, 20000, 8, OUT, XYZ, None, None) == -1
    assert lib.gdrn_model_fps(PTS, NP, large.ctypes.data, 2, 20000, 8, OUT, XYZ, WS + 8, None) == -1
    huge = np.array([3000000], dtype=np.int32)                                        # 5860 tiles a side: 2^32 threads and more
    assert lib.gdrn_model_diameter(PTS, NP, huge.ctypes.data, 1, 3000000, OUT, None) == -2
