"""GPU tests of the depth rasterizer and the xyz-target generation (csrc/render.hip through gdrnet_amd.render) against the brute-force host
rasterizer (tests/render_host.py) and golden G13 (the reference's calc_xyz_bp_fast / mask2bbox_xyxy on the fixture depths).

Bounds.  Coverage: identical on every pixel -- the fixtures' seeds keep every pixel centre at least 1e-6 px off every edge (or exactly on it),
so geometry decides it, not rounding (tests/test_render_cpu.py asserts that).  Depth: |d - d_ref| <= 2^-23 d_ref, one fp32 ulp -- both sides are
fp64 before the one rounding and fp64's conditioning error is orders of magnitude below an fp32 ulp.  xyz against G13: 2^-23 |ref| + 1e-12 -- one
fp32 rounding of an fp64 value whose own error is ~1e-16."""
import os

import numpy as np
import pytest
import torch

import render_host as RH
from gdrnet_amd import cabi, render, roi_data, synth
from gdrnet_amd.cfg import lm13_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -23
_host = {}


def _scene(case):
    """(inputs, host depth) of a scene, computed once per session"""
    if case not in _host:
        inp = synth.make_render_inputs(case)
        _host[case] = (inp, RH.render_depth(inp))
    return _host[case]


def _poses(inp):
    return [torch.from_numpy(inp[k]).to(DEV) for k in ("R", "t", "K")]


def _render(inp, faces=None):
    table = render.MeshTable(inp["vertices"], inp["faces"] if faces is None else faces)
    d = render.render_depth(table, inp["labels"], *_poses(inp), inp["H"], inp["W"], inp["near"], inp["far"])
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and d.shape == (len(inp["labels"]), inp["H"], inp["W"])
    return d.cpu().numpy()


def _check_against_host(got, ref, what):
    assert np.array_equal(got != 0, ref != 0), (what, int(((got != 0) != (ref != 0)).sum()))   # coverage: every pixel
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    worst = float(np.max(err / np.maximum(ref.astype(np.float64), 1e-30) * (ref != 0)))
    print(f"{what}: {int((ref != 0).sum())} covered pixels, worst depth error {worst / ULP:.3f} ulp, {int((got != ref).sum())} pixels differ")
    assert np.all(err <= ULP * ref.astype(np.float64)), (what, worst)


def test_cube_matches_the_host_oracle():
    inp, ref = _scene("cube")
    got = _render(inp)
    _check_against_host(got, ref, "cube")
    for i in range(4):   # and the analytic ray-box depth behind the oracle
        ana, _ = RH.cube_depth_analytic(0.1, inp["R"][i], inp["t"][i], inp["K"][i], inp["H"], inp["W"])
        assert np.array_equal(ana != 0, got[i] != 0) and np.all(np.abs(got[i] - ana) <= ULP * ana)


def test_shared_edges_are_watertight():
    inp, ref = _scene("watertight")
    got = _render(inp)[0]
    assert np.all(got[1:-1, 1:-1] == np.float32(2.0))   # every pixel centre strictly inside the outline lies on an edge or a vertex: no holes
    assert np.array_equal(got, ref[0])                  # (the outline itself: edges are inclusive)


def test_result_does_not_depend_on_face_order_winding_or_the_run():
    inp, ref = _scene("sphere")
    first = _render(inp)
    _check_against_host(first, ref, "sphere")
    assert np.array_equal(first.view(np.uint32), _render(inp).view(np.uint32))   # repeated call: the same bits
    f = inp["faces"][0]
    perm = np.argsort(synth.hash_uniform(11, "perm", (len(f),)))
    flip = synth.hash_uniform(11, "flip", (len(f),)) < 0.5
    g = f[perm].copy()
    g[flip[perm]] = g[flip[perm]][:, ::-1]
    assert len(f) == 1280 and 400 < flip.sum() < 900 and not np.array_equal(g, f)
    assert np.array_equal(first.view(np.uint32), _render(inp, [g]).view(np.uint32))


def test_mixed_batch_of_three_classes_in_one_launch():
    inp, ref = _scene("mixed")
    assert [len(f) for f in inp["faces"]] == [12, 2048, 1280] and list(inp["labels"]) == [2, 0, 1, 1, 0]
    got = _render(inp)
    _check_against_host(got, ref, "mixed")
    # a class with fewer faces than the launch is sized for draws nothing beyond its own: each slice equals the class rendered alone
    for i in (1, 2):
        c = inp["labels"][i]
        one = dict(inp, vertices=[inp["vertices"][c]], faces=[inp["faces"][c]], labels=np.zeros(1, dtype=np.int64), R=inp["R"][i : i + 1],
                   t=inp["t"][i : i + 1], K=inp["K"][i : i + 1])
        assert np.array_equal(_render(one)[0].view(np.uint32), got[i].view(np.uint32))
    # self-occlusion: the perturbed sphere is a closed, non-convex surface -- every covered pixel has a front and a back layer at least, and the
    # comparison above holds each to the nearest one (the host keeps the minimum over all covering triangles)
    assert (ref[0] != 0).sum() > 500


def test_clipping_and_dropped_geometry():
    inp, ref = _scene("clip")
    got = _render(inp)
    _check_against_host(got, ref, "clip")
    assert (got[0] != 0)[:, -1].any()                                        # half outside the frame: drawn up to the last column
    assert not got[1].any() and not got[2].any() and not got[4].any()        # outside the frame | behind the camera | beyond far
    assert (got[3] != 0).sum() > 100                                         # a triangle crossing near is dropped, the rest is drawn
    out = render.xyz_from_depth(torch.from_numpy(got).to(DEV), *_poses(inp))
    H, W = inp["H"], inp["W"]
    assert out["visible"].tolist() == [1, 0, 0, 1, 0]
    for i in (1, 2, 4):
        assert out["xyxy"][i].tolist() == [0, 0, W - 1, H - 1] and not out["xyz"][i].any() and not out["mask"][i].any()


@pytest.mark.parametrize("case", ["cube", "watertight", "sphere", "mixed", "clip"])
def test_xyz_from_depth_matches_golden_g13(case, golden_dir):
    g = np.load(os.path.join(golden_dir, "g13_xyz_targets.npz"))
    inp = synth.make_render_inputs(case)
    assert int(g[f"{case}/seed"]) == inp["seed"]
    depth, ref = g[f"{case}/depth"], g[f"{case}/xyz"]
    out = render.xyz_from_depth(torch.from_numpy(depth).to(DEV), *_poses(inp))   # the golden's depth: independent of the rasterizer
    torch.cuda.synchronize()
    xyz, mask = out["xyz"].cpu().numpy(), out["mask"].cpu().numpy()
    assert xyz.dtype == np.float32 and xyz.shape == ref.shape and mask.dtype == np.uint8
    assert np.array_equal(mask, (depth != 0).astype(np.uint8))
    assert np.array_equal(out["xyxy"].cpu().numpy(), g[f"{case}/xyxy"]) and out["xyxy"].dtype == torch.int32
    assert np.array_equal(out["visible"].cpu().numpy(), (depth != 0).any(axis=(1, 2)).astype(np.int32))
    err = np.abs(xyz.astype(np.float64) - ref)
    print(f"{case}: worst xyz error {float(np.max(err / (ULP * np.abs(ref) + 1e-12))):.3f} of the bound")
    assert np.all(err <= ULP * np.abs(ref) + 1e-12)
    assert not xyz[mask == 0].any()   # exactly 0 outside the mask


def test_xyz_targets_feed_the_roi_cropper():
    inp, ref = _scene("mixed")
    N, H, W = ref.shape
    table = render.MeshTable(inp["vertices"], inp["faces"], device=DEV)
    tg = render.xyz_targets(table, inp["labels"], *_poses(inp), H, W)
    # the cropper's own tables: extents of at least 0.05 m per axis (the flat rectangle has none along z), hashed fps points inside them
    ext = np.stack([np.maximum(np.ptp(v, axis=0), 0.05) for v in inp["vertices"]]).astype(np.float32)
    fps = (synth.hash_uniform(21, "fps", (3, 64, 3)) - 0.5) * ext[:, None, :].astype(np.float64)
    crop = roi_data.RoiCropper(lm13_cfg(device=DEV), extents=ext, fps_points=fps, device=DEV)
    frame = torch.from_numpy(np.floor(synth.hash_uniform(21, "frame", (H, W, 3)) * 256).astype(np.uint8)).to(DEV)
    rois_dev, rois_host = [], []
    for i in range(N):
        xyz, mask, xyxy, vis = RH.xyz_from_depth(ref[i], inp["R"][i], inp["t"][i], inp["K"][i])
        assert vis == 1 and tg[i]["visible"] and tuple(tg[i]["xyxy"]) == tuple(xyxy)
        assert np.array_equal(tg[i]["mask_obj"].cpu().numpy(), mask.astype(np.uint8))
        x1, y1, x2, y2 = xyxy
        uv = inp["K"][i] @ inp["t"][i]
        common = dict(image=frame, bbox=np.array(xyxy, np.float64), bbox_center=np.array([0.5 * (x1 + x2), 0.5 * (y1 + y2)]),
                      scale=float(min(1.5 * max(x2 - x1, y2 - y1, 1), max(H, W))), segmentation=torch.from_numpy(mask.astype(np.uint8)).to(DEV),
                      roi_cls=int(inp["labels"][i]), trans=inp["t"][i].astype(np.float32), centroid_2d=uv[:2] / uv[2])
        rois_dev.append(dict(common, xyz_crop=tg[i]["xyz_crop"], xyxy=tg[i]["xyxy"]))
        rois_host.append(dict(common, xyz_crop=torch.from_numpy(xyz[y1 : y2 + 1, x1 : x2 + 1].astype(np.float32)).to(DEV), xyxy=xyxy))
    a, b = crop(rois_dev, train=True), crop(rois_host, train=True)
    torch.cuda.synchronize()
    for k in ("roi_mask_trunc", "roi_mask_visib", "roi_mask_obj", "roi_region"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["roi_mask_obj"].sum()) > 1000
    worst = float((a["roi_xyz"] - b["roi_xyz"]).abs().max())
    print(f"roi_xyz: worst difference {worst:.3e}")
    # one ulp of a ~1 m depth is 1.2e-7 m; over the smallest extent, 0.05 m, 2.4e-6; 1e-5 leaves a factor 4
    assert worst <= 1e-5


def test_c_abi_argument_errors_return_before_any_launch():
    inp = synth.make_render_inputs("cube")
    tb = render.MeshTable(inp["vertices"], inp["faces"]).on(DEV)
    R, t, K = _poses(inp)
    lab_host = np.zeros(4, dtype=np.int32)
    lab = torch.from_numpy(lab_host).to(DEV)
    depth = torch.full((4, 48, 64), 7.0, dtype=torch.float32, device=DEV)
    lib, p = cabi.load(), cabi.ptr

    def call(N=4, H=48, W=64, near=0.01, far=6.5, verts=p(tb["verts"]), out=p(depth), labels_host=lab_host.ctypes.data, Rp=p(R)):
        return lib.gdrn_render_depth(verts, p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]), 1, 12, p(lab),
                                     labels_host, Rp, p(t), p(K), N, H, W, near, far, out, None)

    bad_lab = np.array([0, 0, 1, 0], dtype=np.int32)
    for kw in (dict(N=0), dict(H=0), dict(W=-3), dict(near=6.5), dict(near=7.0, far=6.5), dict(near=0.0), dict(verts=None), dict(out=None),
               dict(labels_host=None), dict(Rp=None), dict(labels_host=bad_lab.ctypes.data)):
        assert call(**kw) == -1, kw
    xyz, mask = torch.full((4, 48, 64, 3), 7.0, device=DEV), torch.full((4, 48, 64), 7, dtype=torch.uint8, device=DEV)
    xyxy, vis = torch.full((4, 4), 7, dtype=torch.int32, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV)

    def call2(N=4, H=48, W=64, d=p(depth), o=p(xyz), m=p(mask), b=p(xyxy), v=p(vis)):
        return lib.gdrn_xyz_from_depth(d, p(R), p(t), p(K), N, H, W, o, m, b, v, None)

    for kw in (dict(N=0), dict(H=-1), dict(W=0), dict(d=None), dict(o=None), dict(m=None), dict(b=None), dict(v=None)):
        assert call2(**kw) == -1, kw
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((depth == 7.0).all()) and bool((xyz == 7.0).all()) and bool((mask == 7).all()) and bool((xyxy == 7).all()) and bool((vis == 7).all())
    with pytest.raises(ValueError):
        render.render_depth(render.MeshTable(inp["vertices"], inp["faces"]), [0, 0, 1, 0], R, t, K, 48, 64)
    assert call() == 0
