"""GPU tests of the scene ground truth (csrc/scene_gt.hip through gdrnet_amd.scene_gt) against the numpy restatement (tests/scene_gt_host.py) and
golden G17 (the reference's estimate_visib_mask_gt / depth_im_to_dist_im_fast / calc_2d_bbox_xywh on the fixture's maps).

Every comparison is exact.  On the host rasterizer's canvases (scene_gt_from_depth) the device reads the same bits as the restatement, evaluates
the same fp64 operation sequence without contraction and so gives the same bytes, counts, boxes and visib_fract bits.  End to end (scene_gt) the
device's own renders agree with the host's to one fp32 ulp; the fixture's seed keeps every pixel centre 1e-6 px off every edge and every
visibility difference 1e-5 m (about 80 ulps at 1 m) off delta -- tests/test_scene_gt_cpu.py asserts both -- so geometry decides every bit."""
import os

import numpy as np
import pytest
import torch

import scene_gt_host as SH
from gdrnet_amd import cabi, masks, render, scene_gt as SG, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("bop19", "bop18")
DISCRETE = ("mask", "mask_visib", "px_count_all", "px_count_valid", "px_count_visib", "bbox_obj", "bbox_visib")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(gt):
    torch.cuda.synchronize()
    assert gt.mask.dtype == gt.mask_visib.dtype == torch.uint8 and gt.depth.dtype == gt.depth_scene.dtype == torch.float32
    assert gt.px_count_all.dtype == gt.px_count_valid.dtype == gt.px_count_visib.dtype == gt.bbox_obj.dtype == gt.bbox_visib.dtype == torch.int32
    assert gt.visib_fract.dtype == torch.float64
    return {k: getattr(gt, k).cpu().numpy() for k in DISCRETE + ("visib_fract", "depth", "depth_scene")}


def same(got, want, what, keys=DISCRETE + ("visib_fract",), rows=None):
    for k in keys:
        a, b = got[k], want[k] if rows is None else want[k][rows]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if k == "visib_fract":
            a, b = a.view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} places, first at {bad[0].tolist()}: got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def poses(inp, rows=slice(None)):
    return [dev(inp[k][rows]) for k in ("R", "t", "K")]


def end_to_end(inp, composed=False, mode="bop19", rows=slice(None), chunk=64, scene=None):
    table = render.MeshTable(inp["vertices"], inp["faces"], device=DEV)
    return SG.scene_gt(table, inp["labels"][rows], *poses(inp, rows), inp["H"], inp["W"], inp["frame"][rows], None if composed else dev(scene),
                       inp["delta"], mode, inp["pad"], inp["near"], inp["far"], chunk)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", synth.SCENE_GT_CASES)
def test_from_depth_equals_the_restatement_and_the_reference(case, mode, golden_dir):
    inp, canv, scene, _ = SH.scene(case)
    want = SH.result(case, mode, False)[0]
    got = host(SG.scene_gt_from_depth(dev(canv), dev(inp["K"]), inp["frame"], dev(scene), inp["delta"], mode, inp["pad"]))
    same(got, want, f"{case}/{mode}")
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    g = np.load(os.path.join(golden_dir, "g17_scene_gt.npz"))
    N, H, W = got["mask"].shape
    unpack = lambda b: np.unpackbits(b)[: N * H * W].reshape(N, H, W)  # noqa: E731
    assert np.array_equal(got["mask"], unpack(g[f"{case}/mask"])) and np.array_equal(got["mask_visib"], unpack(g[f"{case}/{mode}/mask_visib"]))
    for k in ("px_count_all", "px_count_valid"):
        assert np.array_equal(got[k], g[f"{case}/{k}"]), k
    assert np.array_equal(got["px_count_visib"], g[f"{case}/{mode}/px_count_visib"])
    assert np.array_equal([SG.xywh(b) for b in got["bbox_obj"]], g[f"{case}/bbox_obj"])
    assert np.array_equal([SG.xywh(b) for b in got["bbox_visib"]], g[f"{case}/{mode}/bbox_visib"])


def test_default_margin_is_the_canvas_of_three_times_the_image():
    inp, canv, scene, _ = SH.scene("mixed")
    got = host(SG.scene_gt_from_depth(dev(canv), dev(inp["K"]), dev(inp["frame"]), dev(scene)))   # pad, delta, mode: the defaults; frame from the device
    same(got, SH.result("mixed", "bop19", False)[0], "defaults")
    with pytest.raises(ValueError):
        SG.scene_gt_from_depth(dev(canv[:, :140]), dev(inp["K"]), inp["frame"])


@pytest.mark.parametrize("case", synth.SCENE_GT_CASES)
def test_end_to_end_with_depth_images(case):
    inp, canv, scene, _ = SH.scene(case)
    px, py = inp["pad"]
    H, W = inp["H"], inp["W"]
    for mode in MODES:
        got = host(end_to_end(inp, mode=mode, scene=scene))
        same(got, SH.result(case, mode, False)[0], f"{case}/{mode}")
    table = render.MeshTable(inp["vertices"], inp["faces"], device=DEV)
    R, t, K = poses(inp)
    big = render.render_depth(table, inp["labels"], R, t, dev(SH.canvas_K(inp["K"], px, py)), H + 2 * py, W + 2 * px, inp["near"], inp["far"])
    assert np.array_equal(got["depth"].view(np.uint32), big[:, py : py + H, px : px + W].cpu().numpy().view(np.uint32))
    assert np.all(np.abs(got["depth"].astype(np.float64) - SH.window(canv, H, W, px, py)) <= 2.0 ** -23 * got["depth"])   # one ulp off the host's


def test_composed_mode_permutation_and_repeat():
    inp, _, _, _ = SH.scene("mixed")
    for mode in MODES:
        want = SH.result("mixed", mode, True)[0]
        first = host(end_to_end(inp, composed=True, mode=mode))
        same(first, want, f"composed/{mode}")
        assert np.array_equal(first["px_count_valid"], first["mask"].reshape(12, -1).sum(1))
    perm = np.array([5, 4, 3, 2, 1, 0, 10, 8, 6, 9, 7, 11])   # within each frame
    again, moved = host(end_to_end(inp, composed=True, mode="bop18")), host(end_to_end(inp, composed=True, mode="bop18", rows=perm))
    for k in DISCRETE + ("visib_fract", "depth"):
        assert np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)), k             # a repeated call: the same bits
        assert np.array_equal(np.ascontiguousarray(first[k][perm]).view(np.uint8), moved[k].view(np.uint8)), k   # permuted rows, no bit changed
    assert np.array_equal(first["depth_scene"].view(np.uint32), moved["depth_scene"].view(np.uint32))
    # the composed scene on the host rasterizer's canvases: the restatement's bits
    _, canv, _, _ = SH.scene("mixed")
    got = host(SG.scene_gt_from_depth(dev(canv), dev(inp["K"]), inp["frame"], None, inp["delta"], "bop19", inp["pad"]))
    want = SH.result("mixed", "bop19", True)[0]
    same(got, want, "composed from host canvases")
    assert np.array_equal(got["depth_scene"].view(np.uint32), want["depth_scene"].view(np.uint32))


def test_results_do_not_depend_on_chunk():
    inp, _, scene, _ = SH.scene("mixed")
    ref = host(end_to_end(inp, scene=scene, chunk=12))
    for chunk in (1, 5):
        got = host(end_to_end(inp, scene=scene, chunk=chunk))
        for k in DISCRETE + ("visib_fract", "depth"):
            assert np.array_equal(ref[k].view(np.uint8), got[k].view(np.uint8)), (chunk, k)


def test_cross_checks_with_masks_and_render():
    inp, _, scene, _ = SH.scene("mixed")
    gt = end_to_end(inp, scene=scene)
    h = host(gt)
    area, box = masks.stats(gt.mask_visib)
    area, box = area.cpu().numpy(), box.cpu().numpy()
    assert np.array_equal(area, h["px_count_visib"])
    some = h["px_count_visib"] > 0
    assert 0 < some.sum() < 12 and np.array_equal(box[some], h["bbox_visib"][some])
    enc = masks.encode(gt.mask_visib)
    back = masks.decode(enc)
    torch.cuda.synchronize()
    assert all(np.array_equal(back[i].cpu().numpy(), h["mask_visib"][i]) for i in range(12))
    segs = gt.segmentations()
    assert len(segs) == 12 and segs == enc.to_coco() and segs[0]["size"] == [47, 61] and isinstance(segs[0]["counts"], str)
    xyz = render.xyz_from_depth(gt.depth, *poses(inp))
    assert torch.equal(xyz["mask"], gt.mask)
    info = gt.to_scene_gt_info(frame_ids=[7, 8, 9])
    assert [len(info[k]) for k in (7, 8, 9)] == [6, 5, 1] and info[9][0]["px_count_visib"] == int(h["px_count_visib"][11])
    assert info[7][1]["bbox_obj"] == SH.xywh(h["bbox_obj"][1]) and info[7][0]["visib_fract"] == 1.0


def test_no_instances_and_a_frame_without_instances():
    inp, canv, scene, _ = SH.scene("mixed")
    table = render.MeshTable(inp["vertices"], inp["faces"], device=DEV)
    e3, e33 = torch.zeros(0, 3, dtype=torch.float64, device=DEV), torch.zeros(0, 3, 3, dtype=torch.float64, device=DEV)
    for gt in (SG.scene_gt(table, [], e33, e3, e33, 47, 61, [], dev(scene)), SG.scene_gt(table, [], e33, e3, e33, 47, 61, []),
               SG.scene_gt_from_depth(dev(canv[:0]), dev(inp["K"][0]), [], None, pad=(61, 47))):
        assert len(gt) == 0 and gt.mask.shape == (0, 47, 61) and gt.bbox_visib.shape == (0, 4) and gt.visib_fract.shape == (0,)
        assert gt.to_scene_gt_info() == {f: [] for f in range(gt.num_frames)}
    # frame 1 of 3 has no instance: rows 0-5 (frame 0) and 11 (frame 2)
    rows = np.array([0, 1, 2, 3, 4, 5, 11])
    want = SH.result("mixed", "bop19", True)[0]
    gt = end_to_end(inp, composed=True, rows=rows)
    got = host(gt)
    same(got, want, "empty middle frame", rows=rows)
    assert gt.num_frames == 3 and not got["depth_scene"][1].any() and got["depth_scene"][0].any() and gt.to_scene_gt_info()[1] == []
    # a depth image that is all holes: bop19 sees everything, bop18 nothing
    for mode, seen in (("bop19", True), ("bop18", False)):
        got = host(SG.scene_gt_from_depth(dev(canv), dev(inp["K"]), inp["frame"], torch.zeros(3, 47, 61, device=DEV), inp["delta"], mode, inp["pad"]))
        assert np.array_equal(got["mask_visib"], got["mask"] if seen else np.zeros_like(got["mask"])) and not got["px_count_valid"].any()
        assert np.array_equal(got["bbox_visib"][0], got["bbox_obj"][0] if seen else SH.EMPTY)


def test_c_abi_argument_errors_return_before_any_launch():
    inp, canv, scene, _ = SH.scene("mixed")
    N, H, W, (px, py) = 12, 47, 61, inp["pad"]
    lib, p = cabi.load(), cabi.ptr
    fill = lambda *shape, dtype=torch.int32: torch.full(shape, 7, dtype=dtype, device=DEV)  # noqa: E731
    c, K, sc = dev(canv), dev(inp["K"]), dev(scene)
    depth, cnt_all, box_obj = fill(N, H, W, dtype=torch.float32), fill(N), fill(N, 4)
    scene_out = fill(3, H, W, dtype=torch.float32)
    mask, mask_v = fill(N, H, W, dtype=torch.uint8), fill(N, H, W, dtype=torch.uint8)
    cnt_valid, cnt_vis, box_vis, fract = fill(N), fill(N), fill(N, 4), fill(N, dtype=torch.float64)
    fr_host = inp["frame"].astype(np.int32)
    fr = dev(fr_host)
    off_host, inst_host = SG.csr_of_frames(fr_host, 3)
    off, inst = dev(off_host), dev(inst_host)

    def canvas(cv=p(c), n=N, h=H, w=W, mx=px, my=py, d=p(depth), ca=p(cnt_all), bo=p(box_obj)):
        return lib.gdrn_scene_gt_canvas(cv, n, h, w, mx, my, d, ca, bo, None)

    for kw in (dict(cv=None), dict(d=None), dict(ca=None), dict(bo=None), dict(n=0), dict(h=0), dict(w=-1), dict(mx=-1), dict(my=-2)):
        assert canvas(**kw) == -1, kw

    def compose(d=p(c), o=p(off), oh=off_host.ctypes.data, i=p(inst), ih=inst_host.ctypes.data, F=3, n=N, h=H, w=W, out=p(scene_out)):
        return lib.gdrn_scene_gt_compose(d, o, oh, i, ih, F, n, h, w, out, None)

    bad_off, bad_inst = off_host.copy(), inst_host.copy()
    bad_off[1], bad_inst[3] = 13, 12
    for kw in (dict(d=None), dict(o=None), dict(oh=None), dict(i=None), dict(ih=None), dict(out=None), dict(F=0), dict(n=0), dict(h=0), dict(F=2),
               dict(oh=bad_off.ctypes.data), dict(ih=bad_inst.ctypes.data)):
        assert compose(**kw) == -1, kw

    def visib(d=p(c), s=p(sc), f=p(fr), fh=fr_host.ctypes.data, F=3, k=p(K), n=N, h=H, w=W, delta=0.015, mode=0, m=p(mask), mv=p(mask_v),
              ca=p(cnt_all), cv=p(cnt_valid), cs=p(cnt_vis), bo=p(box_obj), bv=p(box_vis), vf=p(fract)):
        return lib.gdrn_scene_gt_visibility(d, s, f, fh, F, k, n, h, w, delta, mode, m, mv, ca, cv, cs, bo, bv, vf, None)

    bad_fr = fr_host.copy()
    bad_fr[4] = 3
    for kw in (dict(d=None), dict(s=None), dict(f=None), dict(fh=None), dict(k=None), dict(m=None), dict(mv=None), dict(ca=None), dict(cv=None),
               dict(cs=None), dict(bo=None), dict(bv=None), dict(vf=None), dict(F=0), dict(F=2), dict(n=0), dict(h=0), dict(w=0), dict(delta=-1.0),
               dict(delta=float("nan")), dict(mode=2), dict(fh=bad_fr.ctypes.data)):
        assert visib(**kw) == -1, kw
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    for t in (depth, cnt_all, box_obj, scene_out, mask, mask_v, cnt_valid, cnt_vis, box_vis, fract):
        assert bool((t == 7).all())
    for kw in (dict(frame=bad_fr), dict(frame=fr_host[:5]), dict(frame=-fr_host - 1)):
        with pytest.raises(ValueError):
            SG.scene_gt_from_depth(c, K, kw["frame"], sc, pad=(px, py))
    with pytest.raises(ValueError):
        SG.scene_gt_from_depth(c, K, fr_host, sc[:, :40], pad=(px, py))
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        SG.scene_gt_from_depth(c, K, fr_host, torch.from_numpy(scene), pad=(px, py))
