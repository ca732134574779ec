"""CPU tests (-m "not gpu") of gdrnet_amd.scene_gt: the host restatement (tests/scene_gt_host.py) against golden G17 -- the reference's own
estimate_visib_mask_gt, depth_im_to_dist_im_fast and calc_2d_bbox_xywh on the fixture's maps -- bit for bit; the fixture's margins and kinds;
SceneGt's host-side views; the argument errors; the C-ABI symbols and their host-only checks."""
import os

import numpy as np
import pytest
import torch

import scene_gt_host as SH
from gdrnet_amd import cabi, render, scene_gt as SG, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdrn_scene_gt_canvas", "gdrn_scene_gt_compose", "gdrn_scene_gt_visibility")
MODES = ("bop19", "bop18")
_g17 = {}


def g17():
    if not _g17:
        _g17.update(np.load(os.path.join(ROOT, "tests", "golden", "g17_scene_gt.npz")))
    return _g17


def unpacked(bits, shape):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape)


# ---- the restatement against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", synth.SCENE_GT_CASES)
def test_restatement_equals_the_reference(case, mode):
    g = g17()
    assert int(g["seed"]) == synth.SCENE_GT_SEED
    r = SH.result(case, mode, False)[0]
    assert np.array_equal(r["mask"], unpacked(g[f"{case}/mask"], r["mask"].shape))
    assert np.array_equal(r["mask_visib"], unpacked(g[f"{case}/{mode}/mask_visib"], r["mask"].shape))
    assert np.array_equal(r["px_count_all"], g[f"{case}/px_count_all"]) and np.array_equal(r["px_count_valid"], g[f"{case}/px_count_valid"])
    assert np.array_equal(r["px_count_visib"], g[f"{case}/{mode}/px_count_visib"])
    assert np.array_equal([SH.xywh(b) for b in r["bbox_obj"]], g[f"{case}/bbox_obj"])
    assert np.array_equal([SH.xywh(b) for b in r["bbox_visib"]], g[f"{case}/{mode}/bbox_visib"])
    assert np.array_equal([SG.xywh(b) for b in r["bbox_visib"]], g[f"{case}/{mode}/bbox_visib"])   # the module's own writer


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_the_seed_keeps_geometry_in_charge_of_every_bit():
    for case in synth.SCENE_GT_CASES:
        assert SH.scene(case)[3] >= 1e-6, case                    # every pixel centre of every canvas: off every edge (tests/test_render_cpu.py)
        for composed in (False, True):
            for mode in MODES:
                assert SH.result(case, mode, composed)[1] > 1e-5, (case, composed)   # | f32(dist_gt) - f32(dist_scene) - delta | of every covered pixel


def test_the_scene_holds_every_kind_of_instance():
    inp, canv, scene_d, _ = SH.scene("mixed")
    assert (inp["H"], inp["W"], tuple(inp["pad"]), canv.shape) == (47, 61, (61, 47), (12, 141, 183)) and inp["num_frames"] == 3
    assert sorted(set(inp["labels"].tolist())) == [0, 1, 2] and not np.array_equal(inp["K"][11], inp["K"][0])
    k = synth.SCENE_GT_KINDS
    for mode in MODES:
        r, c = SH.result("mixed", mode, False)[0], SH.result("mixed", mode, True)[0]
        win = r["mask"].reshape(12, -1).sum(1)
        i = k["inside"]
        assert r["px_count_all"][i] == win[i] == r["px_count_visib"][i] == r["px_count_valid"][i] > 100 and r["visib_fract"][i] == 1.0
        x1, y1, x2, y2 = r["bbox_obj"][i]
        assert 0 < x1 and 0 < y1 and x2 < 60 and y2 < 46 and np.array_equal(r["bbox_obj"][i], r["bbox_visib"][i])
        i = k["truncated"]
        assert r["px_count_all"][i] > win[i] > 100 and r["bbox_obj"][i][2] > 60 and r["bbox_obj"][i][3] > 46 and r["bbox_visib"][i][2] == 60
        assert 0.0 < r["visib_fract"][i] < 1.0
        i = k["outside_image"]
        assert win[i] == 0 and r["px_count_all"][i] > 100 and r["bbox_obj"][i][2] < 0 and tuple(r["bbox_visib"][i]) == SH.EMPTY
        assert r["visib_fract"][i] == 0.0
        i = k["outside_canvas"]
        assert not canv[i].any() and tuple(r["bbox_obj"][i]) == SH.EMPTY and tuple(r["bbox_visib"][i]) == SH.EMPTY and r["visib_fract"][i] == 0.0
        for res in (r, c):   # mutual occlusion: the same with the depth images and composed
            i, j = k["partly_hidden"], k["hider"]
            assert 0 < res["px_count_visib"][i] < win[i] and res["px_count_visib"][j] == win[j]
            both = (res["mask"][i] == 1) & (res["mask"][j] == 1)
            assert both.sum() > 50 and np.all(res["depth"][i][both] - res["depth"][j][both] > inp["delta"]) and not res["mask_visib"][i][both].any()
            i, j = k["fully_hidden"], k["cover"]
            assert win[i] > 50 and res["px_count_visib"][i] == 0 and tuple(res["bbox_visib"][i]) == SH.EMPTY and res["px_count_visib"][j] == win[j]
        i, j = k["pair"]
        both = (c["mask"][i] == 1) & (c["mask"][j] == 1)
        gap = np.abs(c["depth"][i][both] - c["depth"][j][both])
        assert both.sum() > 100 and 0 < gap.min() and gap.max() < inp["delta"]
        assert c["px_count_visib"][i] == win[i] and c["px_count_visib"][j] == win[j]      # closer than delta along the ray: both visible
        assert np.array_equal(c["px_count_valid"], win)                                   # composed: every mask pixel has a scene depth
        holes = (r["mask"][i] == 1) & (scene_d[1] == 0)
        assert holes.sum() == 20 and r["px_count_valid"][i] == win[i] - 20
        assert bool(r["mask_visib"][i][holes].all()) == (mode == "bop19") and bool(r["mask_visib"][i][holes].any()) == (mode == "bop19")
        i = k["occluded_left"]
        assert 0 < r["px_count_visib"][i] < win[i] and c["px_count_visib"][i] == win[i] and r["bbox_visib"][i][0] > r["bbox_obj"][i][0]
        assert list(inp["frame"]).count(2) == 1 and inp["frame"][k["single"]] == 2 and c["px_count_visib"][k["single"]] == win[k["single"]] > 100
    p0 = SH.result("pad0", "bop19", False)[0]
    full = SH.result("mixed", "bop19", False)[0]
    assert tuple(synth.make_scene_gt_inputs("pad0")["pad"]) == (0, 0)
    assert np.array_equal(p0["px_count_all"], p0["mask"].reshape(12, -1).sum(1)) and np.array_equal(p0["mask_visib"], full["mask_visib"])
    assert tuple(p0["bbox_obj"][k["outside_image"]]) == SH.EMPTY and p0["bbox_obj"][k["truncated"]][2] == 60


def test_composed_mode_does_not_depend_on_instance_order():
    inp, canv, _, _ = SH.scene("mixed")
    perm = np.array([5, 4, 3, 2, 1, 0, 10, 8, 6, 9, 7, 11])   # within each frame
    assert np.array_equal(inp["frame"][perm], inp["frame"])
    for mode in MODES:
        a = SH.result("mixed", mode, True)[0]
        b = SH.scene_gt(canv[perm], inp["K"][perm], inp["frame"][perm], 3, None, inp["delta"], mode, inp["pad"])
        assert np.array_equal(a["depth_scene"].view(np.uint32), b["depth_scene"].view(np.uint32))
        for key in ("mask", "mask_visib", "px_count_all", "px_count_valid", "px_count_visib", "bbox_obj", "bbox_visib"):
            assert np.array_equal(a[key][perm], b[key]), key
        assert np.array_equal(a["visib_fract"][perm].view(np.uint64), b["visib_fract"].view(np.uint64))


# ---- SceneGt -------------------------------------------------------------------------------------------------------------
def test_to_scene_gt_info_layout_and_box_convention():
    r = SH.result("mixed", "bop19", False)[0]
    frame = synth.make_scene_gt_inputs("mixed")["frame"]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items()}
    gt = SG.SceneGt(t["mask"], t["mask_visib"], t["px_count_all"], t["px_count_valid"], t["px_count_visib"], t["bbox_obj"], t["bbox_visib"],
                    t["visib_fract"], t["depth"], t["depth_scene"], frame, 4)   # (a fourth frame without instances)
    info = gt.to_scene_gt_info()
    assert list(info) == [0, 1, 2, 3] and [len(info[f]) for f in info] == [6, 5, 1, 0] and len(gt) == 12
    flat = info[0] + info[1] + info[2]
    g = g17()
    for i, d in enumerate(flat):
        assert tuple(d) == SG.INFO_KEYS
        assert d["bbox_obj"] == g["mixed/bbox_obj"][i].tolist() and d["bbox_visib"] == g["mixed/bop19/bbox_visib"][i].tolist()
        assert all(type(v) is int for v in d["bbox_obj"] + d["bbox_visib"] + [d["px_count_all"], d["px_count_valid"], d["px_count_visib"]])
        assert (d["px_count_all"], d["px_count_valid"], d["px_count_visib"]) == (r["px_count_all"][i], r["px_count_valid"][i], r["px_count_visib"][i])
        assert type(d["visib_fract"]) is float and d["visib_fract"] == r["visib_fract"][i]
    assert flat[3]["bbox_obj"] == [-1, -1, -1, -1] and flat[2]["bbox_visib"] == [-1, -1, -1, -1] and flat[2]["bbox_obj"][0] < 0
    x, y, w, h = flat[0]["bbox_obj"]
    assert [x, y, x + w - 1, y + h - 1] == r["bbox_obj"][0].tolist()               # calc_2d_bbox_xywh: width = x2 - x1 + 1
    named = gt.to_scene_gt_info(frame_ids=["a", "b", "c", "d"])
    assert list(named) == ["a", "b", "c", "d"] and named["c"] == info[2]
    import json

    json.dumps(info)   # plain Python numbers throughout
    for bad in (["a", "b"], ["a", "a", "b", "c"]):
        with pytest.raises(ValueError):
            gt.to_scene_gt_info(frame_ids=bad)
    assert SG.xywh((3, 4, 3, 4)) == [3, 4, 1, 1] and SG.xywh((0, 0, -1, -1)) == [-1, -1, -1, -1]
    off, inst = SG.csr_of_frames([2, 0, 2, 0, 0], 4)
    assert off.tolist() == [0, 3, 3, 5, 5] and inst.tolist() == [1, 3, 4, 0, 2] and off.dtype == inst.dtype == np.int32


def test_argument_errors():
    inp = synth.make_scene_gt_inputs("mixed")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    R, t, K = (torch.from_numpy(inp[k]) for k in ("R", "t", "K"))
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        SG.scene_gt(meshes, inp["labels"], R, t, K, 47, 61, inp["frame"])
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        SG.scene_gt_from_depth(torch.zeros(12, 141, 183), K, inp["frame"])
    # everything below is refused before a tensor is looked at
    for kw in (dict(visib_mode="bop20"), dict(delta=-0.1), dict(delta=float("nan")), dict(pad=(-1, 0)), dict(pad=(0, -3)), dict(pad=5), dict(chunk=0),
               dict(chunk=-2)):
        with pytest.raises(ValueError):
            SG.scene_gt(meshes, inp["labels"], R, t, K, 47, 61, inp["frame"], **kw)
    for hw in ((0, 61), (47, -1)):
        with pytest.raises(ValueError):
            SG.scene_gt(meshes, inp["labels"], R, t, K, *hw, inp["frame"])
    for kw in (dict(visib_mode="x"), dict(delta=-1.0), dict(pad=(-1, -1))):
        with pytest.raises(ValueError):
            SG.scene_gt_from_depth(torch.zeros(12, 141, 183), K, inp["frame"], **kw)
    src = open(SG.__file__).read()
    assert "scene_gt_host" not in src and "render_host" not in src and "bop_host" not in src


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_by_both_builds():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NAMES:
            assert name in cabi.EXPORTS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "#define GDRN_ABI_VERSION 5" in header and "GDRN_VISIB_BOP19 = 0, GDRN_VISIB_BOP18 = 1" in header
    assert SG.VISIB_MODES == {"bop19": 0, "bop18": 1}
    from gdrnet_amd import build

    assert "scene_gt.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "gdr-net_amd", "csrc", "dist64.h"))
    bop = open(os.path.join(ROOT, "gdr-net_amd", "csrc", "bop_metrics.hip")).read()
    assert '#include "dist64.h"' in bop and "double dist_of(" not in bop      # one definition of the distance, shared


def test_entry_points_check_arguments_before_touching_a_device():
    """every call below returns from the host-side checks: nothing is launched (there is no device where this runs)"""
    lib = cabi.load()
    A, B, C_, D, E, F_, G, H_, I_, J = (0x1000 * k for k in range(1, 11))   # (pointers are only compared with NULL here)

    def canvas(c=A, N=3, H=47, W=61, px=61, py=47, depth=B, cnt=C_, box=D):
        return lib.gdrn_scene_gt_canvas(c, N, H, W, px, py, depth, cnt, box, None)

    for kw in (dict(c=None), dict(depth=None), dict(cnt=None), dict(box=None), dict(N=0), dict(N=-1), dict(H=0), dict(W=-5), dict(px=-1), dict(py=-1),
               dict(H=(1 << 20) + 1), dict(px=(1 << 20) + 1)):
        assert canvas(**kw) == -1, kw
    assert canvas(N=65536) == -2 and canvas(H=40000, W=40000, px=10000, py=0) == -2

    off = np.array([0, 2, 2, 3], dtype=np.int32)
    inst = np.array([0, 2, 1], dtype=np.int32)

    def compose(depth=A, o=B, oh=off.ctypes.data, i=C_, ih=inst.ctypes.data, F=3, N=3, H=47, W=61, out=D):
        return lib.gdrn_scene_gt_compose(depth, o, oh, i, ih, F, N, H, W, out, None)

    bad_off = [np.array(v, dtype=np.int32) for v in ([1, 2, 2, 3], [0, 2, 1, 3], [0, 2, 2, 2], [0, 2, 2, 4])]
    bad_inst = [np.array(v, dtype=np.int32) for v in ([0, 3, 1], [0, -1, 1])]
    for kw in [dict(depth=None), dict(o=None), dict(oh=None), dict(i=None), dict(ih=None), dict(out=None), dict(F=0), dict(N=0), dict(H=0), dict(W=0)] + \
              [dict(oh=b.ctypes.data) for b in bad_off] + [dict(ih=b.ctypes.data) for b in bad_inst]:
        assert compose(**kw) == -1, kw

    frame = np.array([0, 2, 1], dtype=np.int32)

    def visib(depth=A, scene=B, fr=C_, fh=frame.ctypes.data, F=3, K=D, N=3, H=47, W=61, delta=0.015, mode=0, m=E, mv=F_, ca=G, cv=H_, cs=I_, bo=J,
              bv=J + 64, vf=J + 128):
        return lib.gdrn_scene_gt_visibility(depth, scene, fr, fh, F, K, N, H, W, delta, mode, m, mv, ca, cv, cs, bo, bv, vf, None)

    bad_frame = [np.array(v, dtype=np.int32) for v in ([0, 3, 1], [-1, 0, 0])]
    for kw in [dict(depth=None), dict(scene=None), dict(fr=None), dict(fh=None), dict(K=None), dict(m=None), dict(mv=None), dict(ca=None), dict(cv=None),
               dict(cs=None), dict(bo=None), dict(bv=None), dict(vf=None), dict(F=0), dict(N=0), dict(H=0), dict(W=-1), dict(delta=-1e-9),
               dict(delta=float("nan")), dict(mode=2), dict(mode=-1), dict(F=2)] + [dict(fh=b.ctypes.data) for b in bad_frame]:
        assert visib(**kw) == -1, kw
    many = np.zeros(65536, dtype=np.int32)
    assert visib(N=65536, fh=many.ctypes.data) == -2
