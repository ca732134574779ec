"""GPU tests of the predicted frame masks (csrc/roi_paste.hip through gdrnet_amd.frame_masks) against the host restatement
tests/paste_host.py.  The sampled value is one fixed fp64 operation sequence and everything else is integers, so every comparison with the
restatement is bitwise: on the seven geometries of the CPU tests in one launch, on maps whose components are known by construction, on frames
shared by several RoIs, on a frame size whose masks start at odd addresses, inside guard bands, and through the chain from the network's mask
output to the steps that take an observed mask."""
import numpy as np
import pytest
import torch

import paste_host as PH
from gdrnet_amd import cabi, devargs, frame_masks, masks, postproc, refine, render, roi_data, synth, verify
from gdrnet_amd.cfg import lm13_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = PH.FRAME_H, PH.FRAME_W
THR = 0.5
GEOM = np.array(PH.GEOMS, dtype=np.float64)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _host_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _assert_equal(got, ref, what, keys=("mask", "area", "bbox")):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))


def _paste(maps, geom, h, w, **kw):
    return _host_np(frame_masks.paste_masks(_dev(maps), geom[:, :2], geom[:, 2], h, w, **kw))


@pytest.fixture(scope="module")
def seven():
    """the seven geometries: dict(maps, ref = the restatement, got = one launch of B = 7)"""
    maps = PH.geometry_maps()
    return dict(maps=maps, ref=PH.paste(maps, GEOM, H, W, THR), got=_paste(maps, GEOM, H, W, thr=THR))


def test_paste_equals_the_restatement_bit_for_bit(seven):
    _assert_equal(seven["got"], seven["ref"], "seven geometries")
    got = seven["got"]
    assert set(np.unique(got["mask"])) <= {0, 1} and got["area"][5] == 0 and list(got["bbox"][5]) == [0, 0, W - 1, H - 1]
    assert all(got["area"][n] > 0 for n in (0, 1, 2, 3, 4, 6))
    sub = [4, 0, 6]                                      # other rows, another order, host geometry as tensors of either kind
    out = _host_np(frame_masks.paste_masks(_dev(seven["maps"][sub])[:, None], torch.from_numpy(GEOM[sub, :2]), _dev(GEOM[sub, 2]), H, W))
    _assert_equal(out, {k: v[sub] for k, v in seven["ref"].items()}, "rows 4, 0, 6")
    for thr in (0.0, 0.93):                              # thr == 0 sets what is touched at all; a high one leaves rows empty
        _assert_equal(_paste(seven["maps"], GEOM, H, W, thr=thr), PH.paste(seven["maps"], GEOM, H, W, thr), f"thr {thr}")


def test_area_and_bbox_are_masks_stats(seven):
    area, bbox = masks.stats(_dev(seven["got"]["mask"]))
    torch.cuda.synchronize()
    assert np.array_equal(area.cpu().numpy(), seven["got"]["area"]) and np.array_equal(bbox.cpu().numpy(), seven["got"]["bbox"])


def test_a_large_frame_and_masks_at_odd_addresses():
    maps = PH.geometry_maps()[:3]
    big = np.array([(600.5, 440.25, 150.0), (100.0, 200.0, 333.3)])       # 2 x 307 200 pixels: indices beyond 16 bits, row 1 behind row 0
    _assert_equal(_paste(maps[:2], big, 480, 640, thr=THR), PH.paste(maps[:2], big, 480, 640, THR), "480 x 640")
    odd = np.array([(6.0, 5.5, 11.0), (15.2, 8.0, 17.0), (10.0, 6.0, 40.0)])  # 13 x 21 = 273 bytes a mask: rows 1 and 2 start unaligned, W < 32
    _assert_equal(_paste(maps, odd, 13, 21, thr=THR), PH.paste(maps, odd, 13, 21, THR), "13 x 21")
    got = _host_np(frame_masks.paste_masks(_dev(maps), odd[:, :2], odd[:, 2], 13, 21, THR, frame=[0, 0, 0], exclusive=True))
    _assert_equal(got, PH.paste_exclusive(maps, odd, [0, 0, 0], 1, 13, 21, THR), "13 x 21 exclusive", ("mask", "area", "bbox", "index"))
    thin = np.array([(2.0, 30.0, 64.0), (3.0, 10.0, 20.0), (0.0, 0.0, 9.0)])  # W = 5: every vector runs over row ends
    _assert_equal(_paste(maps, thin, 50, 5, thr=THR), PH.paste(maps, thin, 50, 5, THR), "50 x 5")


def test_identity_scale_copies_the_map_into_place():
    m = (synth.hash_uniform(43, "bin", (2, 64, 64)) < 0.4).astype(np.float32)
    geom = np.array([(28.0, 20.0, 64.0), (40.0, 30.0, 64.0)])
    got = _paste(m, geom, H, W, thr=THR)
    assert np.array_equal(got["mask"][0], m[0][12:12 + H, 4:4 + W].astype(np.uint8))
    want = np.zeros((H, W), dtype=np.uint8)
    want[:, 8:] = m[1][2:2 + H, :W - 8]
    assert np.array_equal(got["mask"][1], want)


def test_a_mask_cropped_by_the_roi_cropper_and_pasted_back_is_itself():
    fh, fw = 96, 80
    frame_mask = (PH.smooth_map(47, "frame", 96)[:, :fw] > 0.5).astype(np.uint8)
    image = _dev(np.repeat(frame_mask[:, :, None] * np.uint8(255), 3, axis=2))
    crop = roi_data.RoiCropper(lm13_cfg(device=DEV), device=DEV)
    crop.input_res = crop.out_res = 64
    rois = [dict(image=image, bbox_center=(40.0, 50.0), scale=64.0, bbox=(8, 18, 72, 82)),       # the window inside the frame
            dict(image=image, bbox_center=(70.0, 10.0), scale=64.0, bbox=(38, 0, 80, 42))]       # ... over its top-right corner
    batch = crop(rois)
    out = _host_np(frame_masks.paste_masks(batch["roi_img"][:, 0], batch["bbox_center"], batch["scale"], fh, fw, THR))   # the cropper's fp32 device tensors
    for n, (cx, cy) in enumerate(((40, 50), (70, 10))):
        window = np.zeros((fh, fw), dtype=bool)
        window[max(cy - 32, 0):cy + 32, max(cx - 32, 0):cx + 32] = True
        assert np.array_equal(out["mask"][n][window], frame_mask[window]) and not out["mask"][n][~window].any(), n
        assert out["area"][n] == int(frame_mask[window].sum()) > 0


def _component_maps():
    """8 maps of 64 x 64, each different: two blobs | an exact tie | blobs touching at a corner | a checkerboard | a one-pixel serpentine over
    the whole map | empty | full | hashed"""
    m = np.zeros((8, 64, 64), dtype=np.float32)
    m[0, 5:15, 5:15], m[0, 30:50, 20:45] = 0.9, 0.6
    m[1, 20:23, 40:44], m[1, 19, 5], m[1, 20:29, 5], m[1, 28, 6:8], m[1, 50, 50] = 0.9, 0.8, 0.8, 0.8, 0.7
    m[2, 10:14, 10:14], m[2, 14:20, 14:20], m[2, 40:45, 40:44] = 1.0, 0.75, 0.9
    m[3] = (np.indices((64, 64)).sum(axis=0) % 2) * (0.6 + 0.3 * synth.hash_uniform(53, "board", (64, 64)))
    m[4, 0::2, :] = 0.7
    m[4, 1::4, 63], m[4, 3::4, 0] = 0.8, 0.8
    m[4, 63, :] = 0.0                                                      # (row 62 is the serpentine's last; 63 stays empty)
    m[4, 63, 10] = 0.9                                                     # ... but for one pixel that touches it
    m[6] = 0.51 + 0.4 * synth.hash_uniform(53, "full", (64, 64))
    m[7] = synth.hash_uniform(53, "hashed", (64, 64))
    m[7, 3, 3], m[7, 40, 41] = np.nan, np.inf
    return m


def test_components_equal_the_restatement_bit_for_bit():
    maps = _component_maps()
    ref = PH.components(maps, 0.5)
    assert list(ref["num_comp"][:7]) == [2, 3, 2, 1, 1, 0, 1] and ref["num_comp"][7] > 20
    assert list(ref["kept_px"][:7]) == [500, 12, 52, 2048, 32 * 64 + 31 + 1, 0, 4096]
    assert ref["filtered"][1][19, 5] == np.float32(0.8) and not ref["filtered"][1][20:23, 40:44].any()        # the tie: the lower first pixel
    got = _host_np(frame_masks.largest_component(_dev(maps), 0.5))
    for k in ("num_comp", "kept_px"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert got["filtered"].dtype == np.float32 and np.array_equal(got["filtered"].view(np.int32), ref["filtered"].view(np.int32))
    small = synth.hash_uniform(53, "small", (3, 5, 5)).astype(np.float32)                                      # res = 5, [B, 1, res, res] in and out
    small[1] = 0.0
    got = _host_np(frame_masks.largest_component(_dev(small)[:, None], 0.45))
    ref = PH.components(small, 0.45)
    assert got["filtered"].shape == (3, 1, 5, 5) and np.array_equal(got["filtered"][:, 0].view(np.int32), ref["filtered"].view(np.int32))
    assert np.array_equal(got["num_comp"], ref["num_comp"]) and np.array_equal(got["kept_px"], ref["kept_px"]) and ref["kept_px"][1] == 0
    two = _host_np(frame_masks.largest_component(_dev(maps[[7, 4]]), 0.5))                                     # other rows: nothing carried over
    assert np.array_equal(two["filtered"].view(np.int32), PH.components(maps[[7, 4]], 0.5)["filtered"].view(np.int32))


EXCL_FRAME = np.array([0, 1, 0, 0, 1])
# rows 0 and 2 overlap in frame 0, row 3 lies apart from both; row 1 repeats row 0 (map and geometry) in frame 1, where row 4 overlaps it
EXCL_GEOM = np.array([(20.3, 17.9, 37.7), (20.3, 17.9, 37.7), (30.0, 22.0, 30.0), (50.0, 6.0, 10.0), (12.0, 25.0, 28.0)])


@pytest.mark.parametrize("identical", (False, True))
def test_exclusive_paste_equals_the_restatement_and_shares_no_pixel(identical):
    maps = PH.geometry_maps()[[0, 0, 1, 2, 3]]
    geom = EXCL_GEOM.copy()
    if identical:                                        # frame 0's overlapping pair replaced by identical rows
        maps[2], geom[2] = maps[0], geom[0]
    ref = PH.paste_exclusive(maps, geom, EXCL_FRAME, 2, H, W, THR)
    got = _host_np(frame_masks.paste_masks(_dev(maps), geom[:, :2], geom[:, 2], H, W, THR, frame=EXCL_FRAME, num_frames=2, exclusive=True))
    _assert_equal(got, ref, "exclusive", ("mask", "area", "bbox", "index"))
    plain = _paste(maps, geom, H, W, thr=THR)["mask"].astype(bool)
    mask = got["mask"].astype(bool)
    for f in range(2):
        rows = np.flatnonzero(EXCL_FRAME == f)
        assert mask[rows].sum(axis=0).max() <= 1                                              # disjoint
        assert np.array_equal(mask[rows].any(axis=0), plain[rows].any(axis=0))               # and nothing lost
        assert np.array_equal(got["index"][f] >= 0, mask[rows].any(axis=0))
        for n in rows:
            assert np.array_equal(got["index"][f] == n, mask[n])
    assert (plain[0] & plain[2]).any() and (plain[1] & plain[4]).any() and not (plain[3] & (plain[0] | plain[2])).any()
    assert np.array_equal(mask[3], plain[3])                                                  # the row that lies apart keeps everything
    assert np.array_equal(mask[1] | mask[4], plain[0] | plain[4])                             # frame 1 has not seen frame 0's rows
    if identical:
        assert np.array_equal(mask[0], plain[0]) and not mask[2].any() and got["area"][2] == 0 and list(got["bbox"][2]) == [0, 0, W - 1, H - 1]
    else:
        assert mask[0].any() and mask[2].any() and not np.array_equal(mask[0], plain[0])
    with_default = _host_np(frame_masks.paste_masks(_dev(maps), _dev(geom[:, :2], torch.float32), _dev(geom[:, 2], torch.float32), H, W, THR,
                                                    frame=_dev(EXCL_FRAME), exclusive=True))   # num_frames from the frames; fp32 device geometry
    geom32 = geom.astype(np.float32).astype(np.float64)
    _assert_equal(with_default, PH.paste_exclusive(maps, geom32, EXCL_FRAME, 2, H, W, THR), "fp32 geometry", ("mask", "area", "bbox", "index"))


def test_nothing_is_written_outside_the_outputs(seven):
    """the three entry points on buffers with a guard band on both sides, filled with a sentinel: the bands are unchanged, the payload is the
    wrapper's, a second call gives the same bits, and B == 0 writes nothing at all"""
    lib, G = cabi.load(), 64
    stream = devargs.stream(torch.device(DEV))

    def banded(n, dtype, fill):
        return torch.full((G + n + G,), fill, dtype=dtype, device=DEV)

    def payload(bufs):
        torch.cuda.synchronize()
        return {k: b[G:-G].cpu().numpy().copy() for k, b in bufs.items()}

    def intact(bufs, fills, what):
        torch.cuda.synchronize()
        for k, b in bufs.items():
            edge = torch.cat([b[:G], b[-G:]]).cpu().numpy()
            assert (edge == np.asarray(fills[k]).astype(edge.dtype)).all(), (what, k)

    def ptrs(bufs):
        return {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}

    maps, B = _dev(seven["maps"]), len(GEOM)
    geom = _dev(GEOM)
    fills = dict(mask=0xA5, area=-77, bbox=-77, index=-77, filtered=-7.25, num_comp=-77, kept_px=-77)

    def fresh(keys, sizes):
        dt = dict(mask=torch.uint8, filtered=torch.float32)
        return {k: banded(n, dt.get(k, torch.int32), fills[k]) for k, n in zip(keys, sizes)}

    # the plain paste
    runs = []
    for _ in range(2):
        bufs = fresh(("mask", "area", "bbox"), (B * H * W, B, B * 4))
        p = ptrs(bufs)
        cabi.check(lib.gdrn_roi_paste_masks(maps.data_ptr(), geom.data_ptr(), GEOM.ctypes.data, B, 64, H, W, THR, p["mask"], p["area"], p["bbox"], stream),
                   "roi_paste_masks")
        intact(bufs, fills, "paste")
        runs.append(payload(bufs))
    for k, shape in (("mask", (B, H, W)), ("area", (B,)), ("bbox", (B, 4))):
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k].reshape(shape), seven["ref"][k]), k
    # the exclusive paste
    fr = np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.int32)
    csr_host = frame_masks._csr(fr, 2)
    csr = _dev(csr_host)
    ref = PH.paste_exclusive(seven["maps"], GEOM, fr, 2, H, W, THR)
    runs = []
    for _ in range(2):
        bufs = fresh(("index", "mask", "area", "bbox"), (2 * H * W, B * H * W, B, B * 4))
        p = ptrs(bufs)
        cabi.check(lib.gdrn_roi_paste_exclusive(maps.data_ptr(), geom.data_ptr(), GEOM.ctypes.data, fr.ctypes.data, csr.data_ptr(), csr_host.ctypes.data,
                                                B, 2, 64, H, W, THR, p["index"], p["mask"], p["area"], p["bbox"], stream), "roi_paste_exclusive")
        intact(bufs, fills, "exclusive")
        runs.append(payload(bufs))
    for k, shape in (("index", (2, H, W)), ("mask", (B, H, W)), ("area", (B,)), ("bbox", (B, 4))):
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k].reshape(shape), ref[k]), k
    # the components
    prob = _component_maps()
    ref = PH.components(prob, 0.5)
    prob_dev, n = _dev(prob), len(prob)
    runs = []
    for _ in range(2):
        bufs = fresh(("filtered", "num_comp", "kept_px"), (n * 4096, n, n))
        p = ptrs(bufs)
        cabi.check(lib.gdrn_roi_components(prob_dev.data_ptr(), n, 64, 0.5, p["filtered"], p["num_comp"], p["kept_px"], stream), "roi_components")
        intact(bufs, fills, "components")
        runs.append(payload(bufs))
    assert np.array_equal(runs[0]["filtered"].view(np.int32), runs[1]["filtered"].view(np.int32))
    assert np.array_equal(runs[0]["filtered"].reshape(n, 64, 64).view(np.int32), ref["filtered"].view(np.int32))
    assert np.array_equal(runs[0]["num_comp"], ref["num_comp"]) and np.array_equal(runs[1]["kept_px"], ref["kept_px"])
    # B == 0: success, and not a byte changes
    bufs = fresh(("index", "mask", "area", "bbox", "filtered", "num_comp", "kept_px"), (64,) * 7)
    p = ptrs(bufs)
    assert lib.gdrn_roi_paste_masks(maps.data_ptr(), geom.data_ptr(), GEOM.ctypes.data, 0, 64, H, W, THR, p["mask"], p["area"], p["bbox"], stream) == 0
    assert lib.gdrn_roi_paste_exclusive(maps.data_ptr(), geom.data_ptr(), GEOM.ctypes.data, fr.ctypes.data, csr.data_ptr(), csr_host.ctypes.data, 0, 2, 64,
                                        H, W, THR, p["index"], p["mask"], p["area"], p["bbox"], stream) == 0
    assert lib.gdrn_roi_components(prob_dev.data_ptr(), 0, 64, 0.5, p["filtered"], p["num_comp"], p["kept_px"], stream) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert (b.cpu().numpy() == np.asarray(fills[k]).astype(b.cpu().numpy().dtype)).all(), k
    empty = frame_masks.paste_masks(maps[:0], np.zeros((0, 2)), np.zeros(0), H, W, frame=[], num_frames=2, exclusive=True)
    assert empty["mask"].shape == (0, H, W) and empty["index"].shape == (2, H, W) and bool((empty["index"] == -1).all())
    assert frame_masks.largest_component(maps[:0])["filtered"].shape == (0, 64, 64)


def test_the_chain_from_the_networks_output_to_the_steps_that_take_a_mask():
    cfg = lm13_cfg(device=DEV)
    inp = synth.make_refine_inputs("sphere")                       # a 96 x 128 frame with two estimates of one pose
    fh, fw = inp["H"], inp["W"]
    pred = synth.make_postproc_inputs(4)["mask"]                    # [4, 1, 64, 64] as the network emits it; row 2 is flat
    pred[1, 0] = 1.4 * PH.smooth_map(59, "chain1") - 0.2
    pred[3, 0] = 1.4 * PH.smooth_map(59, "chain3") - 0.2
    centre = np.array([(64.0, 48.0), (60.5, 40.25), (30.0, 30.0), (100.0, 70.0)])
    scale = np.array([80.0, 70.0, 50.0, 90.0])
    out_dict = dict(mask=_dev(pred))
    out = frame_masks.masks_from_maps(cfg, out_dict, centre, scale, fh, fw)
    got = _host_np(out)
    prob = postproc.get_out_mask(cfg, out_dict["mask"])
    torch.cuda.synchronize()
    prob = prob.cpu().numpy()[:, 0]
    thr = cfg.MODEL.CDPN.ROT_HEAD.MASK_THR_TEST
    cc = PH.components(prob, thr)
    geom = np.concatenate([centre, scale[:, None]], axis=1)
    ref = PH.paste(cc["filtered"], geom, fh, fw, thr)
    _assert_equal(got, ref, "chain")
    assert np.array_equal(got["num_comp"], cc["num_comp"]) and np.array_equal(got["kept_px"], cc["kept_px"])
    assert got["num_comp"][0] > 20 and got["area"][2] == 0 and all(got["area"][n] > 0 for n in (0, 1, 3))   # hashed | flat: NaN after min-max | blobs
    whole = _host_np(frame_masks.masks_from_maps(cfg, out_dict, centre, scale, fh, fw, keep_largest=False, mask_thr=0.25))
    _assert_equal(whole, PH.paste(prob, geom, fh, fw, 0.25), "chain without the component step")
    assert "num_comp" not in whole and whole["area"][0] > got["area"][0]
    # masks.encode takes it: the strings decode on the host codec to the same pixels
    enc = masks.encode(out["mask"])
    for n, seg in enumerate(enc.to_coco()):
        runs = masks.rle_from_string(seg["counts"]).astype(np.int64)
        flat = np.repeat(np.arange(len(runs)) % 2, runs).astype(np.uint8)
        assert seg["size"] == [fh, fw] and np.array_equal(flat.reshape(fw, fh).T, got["mask"][n]), n
    assert np.array_equal(enc.area.cpu().numpy(), got["area"])
    # verify and the silhouette ICP take it (the contract only: no score is judged)
    rows = np.array([0, 1, 0, 1])
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    R0, t0, K = _dev(inp["R0"][rows]), _dev(inp["t0"][rows]), _dev(inp["K"][rows])
    ren = render.render_depth(meshes, inp["labels"][rows], R0, t0, K, fh, fw, inp["near"], inp["far"])
    gt = render.render_depth(meshes, inp["gt_labels"], _dev(inp["R_gt"]), _dev(inp["t_gt"]), _dev(inp["K"][:1]), fh, fw, inp["near"], inp["far"])
    scene = _dev(synth.refine_scene(inp, gt.cpu().numpy()))
    ver = _host_np(verify.verify_maps(ren, scene, inp["frame"][rows], mask_obs=out["mask"], mask_index=np.arange(4)))
    assert np.array_equal(ver["mask_px"], got["area"]) and ver["score"].shape == (4,)
    sil = _host_np(refine.icp_refine_sil(meshes, inp["labels"][rows], R0, t0, K, scene, inp["frame"][rows], mask_obs=out["mask"], iters=2,
                                         near=inp["near"], far=inp["far"]))
    assert sil["R"].shape == (4, 3, 3) and sil["t"].shape == (4, 3)
