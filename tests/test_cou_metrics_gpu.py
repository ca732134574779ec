"""GPU tests of the complement-over-union errors (csrc/cou_metrics.hip through gdrnet_amd.cou_metrics) against golden G19 -- the reference's own
pose_error.cus / cou_mask / cou_bb on the fixture of synth.make_cou_inputs (tests/golden/make_golden_g19.py) -- and against the host restatement
tests/cou_host.py at the launch edges.

Every comparison is exact equality.  Counts and boxes are integers; each error is one correctly rounded fp64 division and one subtraction of those
integers, the box IoU the same fp64 operation sequence with contraction off: there is nothing to tolerate."""
import os

import numpy as np
import pytest
import torch

import cou_host as CH
from gdrnet_amd import cabi, cou_metrics as CM, devargs, render, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 1, 1), (1, 1, 67), (3, 3, 5), (5, 47, 61), (2, 64, 64), (3, 17, 256))
# ^ one pixel | one ragged wave | a batch smaller than a wave, rows at odd offsets | the fixture's odd H * W, two workgroups per row | exactly two
#   full workgroups per row | a workgroup's threads spread over several image rows, three workgroups per row, the last one ragged


@pytest.fixture(scope="module")
def g19(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g19_cou_metrics.npz")))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _host(parts):
    torch.cuda.synchronize()
    err, counts, boxes = parts
    assert err.dtype == torch.float64 and counts.dtype == torch.int32 and boxes.dtype == torch.int32
    return err.cpu().numpy(), counts.cpu().numpy(), boxes.cpu().numpy()


def _check_golden(parts, g19, what):
    err, counts, boxes = parts
    rows = g19["cus/bb_rows"]
    others = np.setdiff1d(np.arange(14), rows)
    print(f"{what}: counts differ in {int((counts != g19['cus/counts']).sum())} cells, boxes in {int((boxes != g19['cus/boxes']).sum())}, cus in "
          f"{int((_bits(err[:, 0]) != _bits(g19['cus/cus'])).sum())} rows, cou_bb_proj in {int((_bits(err[rows, 1]) != _bits(g19['cus/cou_bb_proj'][rows])).sum())}")
    assert err.shape == (14, 2) and counts.shape == (14, 2) and boxes.shape == (14, 2, 4), what
    assert np.array_equal(counts, g19["cus/counts"]) and np.array_equal(boxes, g19["cus/boxes"]), what
    assert np.array_equal(_bits(err[:, 0]), _bits(g19["cus/cus"])), what
    assert np.array_equal(_bits(err[rows, 1]), _bits(g19["cus/cou_bb_proj"][rows])) and np.all(err[others, 1] == 1.0), what


def test_cus_from_poses_equals_the_reference(g19):
    inp, est, gt = CH.cus_scene()
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    for host, R, t in ((est, "R_est", "t_est"), (gt, "R_gt", "t_gt")):   # the device depth is the host rasterizer's, bit for bit, on this seed
        d = render.render_depth(meshes, inp["labels"], _dev(inp[R]), _dev(inp[t]), _dev(inp["K"]), inp["H"], inp["W"], inp["near"], inp["far"])
        assert np.array_equal(d.cpu().numpy().view(np.uint32), host.view(np.uint32)), R
    poses = [_dev(inp[k]) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    parts = _host(CM.cus(meshes, inp["labels"], *poses, inp["H"], inp["W"], inp["near"], inp["far"], return_parts=True))
    _check_golden(parts, g19, "cus")
    err = CM.cus(meshes, _dev(inp["labels"]), *poses, inp["H"], inp["W"])   # the default planes are the fixture's; labels from the device
    assert err.shape == (14, 2) and np.array_equal(_bits(err.cpu().numpy()), _bits(parts[0]))


def test_cou_from_depth_and_cou_mask_equal_the_reference(g19):
    _, est, gt = CH.cus_scene()
    _check_golden(_host(CM.cou_from_depth(_dev(est), _dev(gt), return_parts=True)), g19, "cou_from_depth")
    assert np.array_equal(_bits(g19["cus/cou_mask_u8"]), _bits(g19["cus/cus"])) and np.array_equal(_bits(g19["cus/cou_mask_bool"]), _bits(g19["cus/cus"]))
    u8 = lambda d: (d > 0).astype(np.uint8) * 255  # noqa: E731
    _check_golden(_host(CM.cou_mask(_dev(u8(est)), _dev(u8(gt)), return_parts=True)), g19, "cou_mask uint8 {0, 255}")
    _check_golden(_host(CM.cou_mask(_dev(est > 0), _dev(gt > 0), return_parts=True)), g19, "cou_mask bool")
    _check_golden(_host(CM.cou_mask(_dev(est > 0), _dev(u8(gt)), return_parts=True)), g19, "cou_mask bool / uint8")
    a, b = CM.cou_from_depth(_dev(est), _dev(gt)), CM.cou_from_depth(_dev(est), _dev(gt))   # repeated calls: the same bits
    assert a.shape == (14, 2) and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_cou_bb_equals_the_reference(g19):
    pairs = g19["bb/pairs"]
    got = CM.cou_bb(_dev(pairs[:, 0]), _dev(pairs[:, 1]))
    assert got.dtype == torch.float64 and got.shape == (16,) and np.array_equal(_bits(got.cpu().numpy()), _bits(g19["bb/cou_bb"]))
    rows = g19["cus/bb_rows"]
    b = g19["cus/boxes"][rows].astype(np.int64)
    xywh = np.stack([b[..., 0], b[..., 1], b[..., 2] - b[..., 0] + 1, b[..., 3] - b[..., 1] + 1], axis=-1)   # [rows, 2, 4]
    for dtype in (torch.int32, torch.int64, torch.float32, torch.float64):
        got = CM.cou_bb(_dev(xywh[:, 0], dtype), _dev(xywh[:, 1], dtype)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(g19["cus/cou_bb_proj"][rows])), dtype
    nan = np.array([[np.nan, 0, 2, 2], [0, 0, 2, 2], [0, 0, np.nan, 2], [0, 0, 2, 2]]), np.array([[0, 0, 2, 2], [0, np.nan, 2, 2], [0, 0, 2, 2], [0, 0, 2, 2]])
    assert CM.cou_bb(_dev(nan[0]), _dev(nan[1])).cpu().tolist() == [1.0, 1.0, 1.0, 0.0] and list(CH.cou_bb(*nan)) == [1.0, 1.0, 1.0, 0.0]


def _contents(N, H, W, kind):
    """(name, est, gt) hand-made map pairs [N,H,W] of the element kind; `on` are two covered values, 0 is not covered in either kind"""
    dtype, on = (np.float32, (0.7, 3.0e38)) if kind == "depth" else (np.uint8, (1, 255))
    z = lambda: np.zeros((N, H, W), dtype)  # noqa: E731
    full = lambda k: np.full((N, H, W), on[k], dtype)  # noqa: E731
    out = [("all empty", z(), z()), ("all covered", full(0), full(1)), ("est covered, gt empty", full(1), z())]
    corners = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))
    for k, (y, x) in enumerate(corners):
        e, g = z(), z()
        e[:, y, x] = on[0]
        g[:, corners[(k + 1) % 4][0], corners[(k + 1) % 4][1]] = on[1]
        out.append((f"corner {k}", e, g))
    e = z()
    e[N - 1, H - 1, W - 1] = on[0]
    out.append(("the last pixel of the batch", e, z()))
    e, g = z(), z()
    for i in range(N):   # nothing may leak across rows: row i must see one est pixel, row i + 1 one gt pixel, and no intersection
        if i % 2 == 0:
            e[i, H - 1, W - 1] = on[1]
        elif i > 0:
            g[i, 0, 0] = on[0]
    out.append(("last pixel of row i, first pixel of row i + 1", e, g))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    chk = ((yy + xx) % 2 == 0)
    out.append(("checkerboard against its complement", np.where(chk, on[0], 0).astype(dtype)[None].repeat(N, 0),
                np.where(~chk, on[1], 0).astype(dtype)[None].repeat(N, 0)))
    out.append(("checkerboard against all", np.where(chk, on[0], 0).astype(dtype)[None].repeat(N, 0), full(0)))
    r = CH.hash_maps(23, f"a{N}x{H}x{W}", (N, H, W), kind)
    out.append(("est = gt", r, r.copy()))
    out.append(("hash maps, 30 % covered", r, CH.hash_maps(23, f"b{N}x{H}x{W}", (N, H, W), kind)))
    if kind == "depth":   # NaN (both signs), -0.0, 0.0, negatives, -inf: not covered; +inf, the smallest subnormal, FLT_MIN: covered
        vals = np.array([0x7FC00000, 0x80000000, 0xBF800000, 0x7F800000, 0x00000001, 0x00800000, 0x00000000, 0xFFC00000, 0xFF800000, 0x7F800001,
                         0x3F800000, 0x80000001, 0x007FFFFF], dtype=np.uint32).view(np.float32)
    else:
        vals = np.array([0, 1, 2, 128, 255, 0, 0, 64, 0, 254], dtype=np.uint8)
    idx = np.arange(N * H * W)
    out.append(("value rules", vals[idx % len(vals)].reshape(N, H, W), vals[(idx // 3) % len(vals)].reshape(N, H, W)))
    return out


@pytest.mark.parametrize("kind", ("depth", "mask"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_launch_edges_against_the_host_restatement(shape, kind):
    fn = CM.cou_from_depth if kind == "depth" else CM.cou_mask
    for name, est, gt in _contents(*shape, kind):
        err, counts, boxes = _host(fn(_dev(est), _dev(gt), return_parts=True))
        ref_err, ref_counts, ref_boxes = CH.cou_maps(est, gt, kind)
        what = f"{name} {shape} {kind}"
        assert np.array_equal(counts, ref_counts), (what, counts.tolist(), ref_counts.tolist())
        assert np.array_equal(boxes, ref_boxes), (what, boxes.tolist(), ref_boxes.tolist())
        assert np.array_equal(_bits(err), _bits(ref_err)), what
    if kind == "depth" and shape == (3, 3, 5):   # what the value rules are meant to show did happen
        _, est, gt = _contents(*shape, kind)[-1]
        with np.errstate(invalid="ignore"):
            assert np.array_equal(CH.covered(est, kind), est > 0) and np.isnan(est).any() and np.isinf(est).any() and (est > 0).sum() == 18


def test_views_and_unaligned_bases_give_the_result_of_their_copy():
    N, H, W = 3, 9, 13
    for kind, fn in (("depth", CM.cou_from_depth), ("mask", CM.cou_mask)):
        big_e, big_g = (_dev(CH.hash_maps(29, f"v{k}", (N, 2 * H, W + 3), kind)) for k in "eg")
        ve, vg = big_e[:, ::2, 2:-1], big_g[:, 1::2, 1:-2]
        assert not ve.is_contiguous() and ve.shape == (N, H, W)
        ref = CH.cou_maps(ve.cpu().numpy(), vg.cpu().numpy(), kind)
        for parts in (fn(ve, vg, return_parts=True), fn(ve.contiguous(), vg.contiguous(), return_parts=True)):
            got = _host(parts)
            assert all(np.array_equal(a, b) for a, b in zip(got[1:], ref[1:])) and np.array_equal(_bits(got[0]), _bits(ref[0]))
        # a contiguous map whose base sits one element into an allocation: 1 byte off (masks), 4 bytes off 16 (depth)
        flat_e, flat_g = big_e.reshape(-1), big_g.reshape(-1)
        oe, og = flat_e[1 : 1 + N * H * W].view(N, H, W), flat_g[3 : 3 + N * H * W].view(N, H, W)
        assert oe.is_contiguous() and oe.data_ptr() % 16 != 0 and og.data_ptr() % 16 != 0
        got, ref = _host(fn(oe, og, return_parts=True)), CH.cou_maps(oe.cpu().numpy(), og.cpu().numpy(), kind)
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], ref[1:])) and np.array_equal(_bits(got[0]), _bits(ref[0]))


def test_no_rows_gives_empty_tensors():
    d = torch.zeros(0, 5, 7, device=DEV)
    for parts in (CM.cou_from_depth(d, d, return_parts=True), CM.cou_mask(d.to(torch.uint8), d.to(torch.bool), return_parts=True)):
        err, counts, boxes = _host(parts)
        assert err.shape == (0, 2) and counts.shape == (0, 2) and boxes.shape == (0, 2, 4)
    assert CM.cou_from_depth(d, d).shape == (0, 2)
    bb = torch.zeros(0, 4, device=DEV)
    got = CM.cou_bb(bb, bb)
    assert got.shape == (0,) and got.dtype == torch.float64
    inp = synth.make_cou_inputs("cus")
    meshes = render.MeshTable(inp["vertices"], inp["faces"])
    none = [_dev(inp[k][:0]) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    assert CM.cus(meshes, [], *none, 5, 7).shape == (0, 2)
    torch.cuda.synchronize()


def test_nothing_is_written_outside_the_outputs_and_the_workspace():
    """the entry points on buffers with a guard band on both sides, filled with a sentinel: the band is unchanged, the payload is the wrapper's"""
    lib, G = cabi.load(), 64
    for kind, shape in (("depth", (5, 47, 61)), ("mask", (3, 17, 256)), ("depth", (1, 1, 1))):
        N = shape[0]
        est, gt = _dev(CH.hash_maps(31, "ge", shape, kind)), _dev(CH.hash_maps(31, "gg", shape, kind))
        ws_ints = int(lib.gdrn_cou_maps_workspace_bytes(N)) // 4
        assert ws_ints == 10 * N
        bufs = dict(err=torch.full((G + 2 * N + G,), -7.25, dtype=torch.float64, device=DEV),
                    counts=torch.full((G + 2 * N + G,), -77, dtype=torch.int32, device=DEV),
                    boxes=torch.full((G + 8 * N + G,), -77, dtype=torch.int32, device=DEV),
                    ws=torch.full((G + ws_ints + G,), -77, dtype=torch.int32, device=DEV))
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        cabi.check(lib.gdrn_cou_maps(est.data_ptr(), gt.data_ptr(), CM.KINDS[kind], *shape, ptr["err"], ptr["counts"], ptr["boxes"], ptr["ws"],
                                     devargs.stream(torch.device(DEV))), "cou_maps")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            sentinel = -7.25 if k == "err" else -77
            assert bool((b[:G] == sentinel).all()) and bool((b[-G:] == sentinel).all()), (k, kind, shape)
            assert k == "ws" or bool((b[G:-G] != sentinel).all()), (k, kind, shape)
        ref = _host((CM.cou_from_depth if kind == "depth" else CM.cou_mask)(est, gt, return_parts=True))
        assert np.array_equal(_bits(bufs["err"][G:-G].cpu().numpy().reshape(N, 2)), _bits(ref[0]))
        assert np.array_equal(bufs["counts"][G:-G].cpu().numpy().reshape(N, 2), ref[1])
        assert np.array_equal(bufs["boxes"][G:-G].cpu().numpy().reshape(N, 2, 4), ref[2])
    pairs = np.array(synth.COU_BB_PAIRS, dtype=np.float64)
    a, b = _dev(pairs[:, 0]), _dev(pairs[:, 1])
    out = torch.full((G + 16 + G,), -7.25, dtype=torch.float64, device=DEV)
    cabi.check(lib.gdrn_cou_bb(a.data_ptr(), b.data_ptr(), 16, out.data_ptr() + G * 8, devargs.stream(torch.device(DEV))), "cou_bb")
    torch.cuda.synchronize()
    assert bool((out[:G] == -7.25).all()) and bool((out[-G:] == -7.25).all())
    assert np.array_equal(_bits(out[G:-G].cpu().numpy()), _bits(CH.cou_bb(pairs[:, 0], pairs[:, 1])))


def test_cou_recall_counts_the_golden_errors(g19):
    inp = synth.make_cou_inputs("cus")
    err, labels, missing = g19["cus/cus"], inp["labels"], {1: 2, 2: 1}
    rec = CM.CouRecall(inp["obj_names"])
    rec.update(_dev(err[:9]), labels[:9])
    rec.update(_dev(err)[9:], _dev(labels[9:]))   # labels from the device as well
    for c, n in missing.items():
        rec.add_missing(c, n)
    got, ref = rec.counters(), CH.recall_counts(err, labels, 3, CM.CUS_TH, missing)
    for k in ("correct", "seen"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), k
    assert list(got["seen"]) == [5, 7, 5] and 0 < got["correct"].sum() < 14
    out = rec.summarize()
    assert out["targets"] == 17 and out["all"] == float(ref["correct"].sum()) / 17.0 and len(out["rows"]) == 5
    for c, name in enumerate(inp["obj_names"]):
        assert out["objects"][name] == float(ref["correct"][c]) / float(ref["seen"][c])
    at = CM.CouRecall(["x"], th=0.25)   # an error equal to the threshold is not correct
    at.update(_dev(np.array([0.25, np.nextafter(0.25, 0.0), np.nan, 0.0])), [0, 0, 0, 0])
    assert list(at.counters()["correct"]) == [2] and list(at.counters()["seen"]) == [4]
    rec.reset()
    assert not rec.counters()["seen"].any()
