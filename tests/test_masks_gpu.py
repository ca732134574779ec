"""GPU parity of gdrnet_amd.masks (COCO run-length strings <-> device masks) through the C ABI.  Every comparison is exact equality -- bytes of masks,
characters of strings, integers of counts / area / bbox -- with the naive restatement of maskApi in tests/rle_host.py (the format is pinned to
that restatement, not to pycocotools, which is not installed where this is built)."""
import numpy as np
import pytest
import torch

import rle_host as RH
from gdrnet_amd import augment as A, cabi, masks as M, synth
from gdrnet_amd.cfg import lmo_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the smallest shapes at which the 64 x 64 tiling, the 16-byte store edges, the 16-row segments and the 1024-character chunks can go wrong
SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 129), (130, 200), (480, 640)]


@pytest.fixture(scope="module")
def cases():
    """{(h, w): [(name, mask, string), ...]} from the restatement, computed once; 480 x 640 carries the all-zero mask (its single count 307 200 is
    a four-character token) and the ellipses only"""
    out = {}
    for h, w in SHAPES:
        cs = RH.contents(h, w)
        if (h, w) == (480, 640):
            cs = [c for c in cs if c[0] in ("zeros", "ellipses")]
        out[(h, w)] = [(name, m, RH.mask_to_string(m)) for name, m in cs]
    # the checkerboard: a leading 0, a run per pixel except that the 199 column seams join two pixels (h is even) -- 25 802 one-character
    # tokens, 26 chunks of the parser
    assert out[(480, 640)][0][2] == "PP\\9" and len(out[(130, 200)][8][2]) == 130 * 200 - 199 + 1
    return out


def _segms(items):
    return [dict(size=list(m.shape), counts=s) for _, m, s in items]


def _np(t):
    return t.cpu().numpy()


def _check_decoded(got, items):
    assert len(got) == len(items)
    for g, (name, m, _) in zip(got, items):
        assert g.dtype == torch.uint8 and tuple(g.shape) == m.shape and g.is_contiguous() and g.data_ptr() % 16 == 0, name
        assert np.array_equal(_np(g), m), (name, m.shape, int((_np(g) != m).sum()))


# ---- decode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_equals_the_restatement(cases, shape):
    items = cases[shape]
    got = M.decode(M.RleBatch.from_coco(_segms(items)), device=DEV, check=True)
    _check_decoded(got, items)


def _mixed(cases):
    return [cases[(37, 53)][11], cases[(1, 70)][8], cases[(130, 200)][9], cases[(70, 1)][6], cases[(65, 129)][11]]


def test_decode_mixed_sizes_one_mask_and_seventy(cases):
    items = _mixed(cases)
    _check_decoded(M.decode(M.RleBatch.from_coco(_segms(items)), device=DEV), items)
    _check_decoded(M.decode(M.RleBatch.from_coco(_segms(items[:1])), device=DEV), items[:1])
    pool = cases[(37, 53)] + cases[(65, 129)] + cases[(1, 70)] + cases[(64, 64)]
    many = [pool[(7 * i) % len(pool)] for i in range(70)]
    _check_decoded(M.decode(M.RleBatch.from_coco(_segms(many)), device=DEV, check=True), many)
    assert M.decode(M.RleBatch.from_coco([]), device=DEV) == []


def test_decode_accepts_interior_zero_runs():
    """legal non-canonical input, as pycocotools' merge produces it"""
    segs, want = [], []
    for h, w in ((37, 53), (65, 129), (2, 3)):
        for counts in ([3, 0, 2, 0, 0, h * w - 5], [0, 0, 0, 4, 0, 1, h * w - 5], [0, 2, 0, 0, 1, 0, 1, h * w - 4, 0, 0]):
            segs.append(dict(size=[h, w], counts=counts))
            want.append(RH.mask_of_counts(counts, h, w))
            assert RH.counts_of_string(M.rle_to_string(counts)) == counts
    batch = M.RleBatch.from_coco(segs)
    got = M.decode(batch, device=DEV, check=True)
    for g, m in zip(got, want):
        assert np.array_equal(_np(g), m)
    canon = M.encode(got).to_coco()
    assert [c["counts"] for c in canon] == [RH.canonical(s["counts"], *s["size"]) for s in batch.to_coco()]


def test_decode_never_writes_outside_a_mask():
    """strings whose totals are short and long of h w: the remainder is 0, the excess is dropped, and no byte outside a mask's extent changes (a
    bounds property read from the outputs: the batch sits in a poisoned allocation)"""
    segs = []
    for h, w in ((37, 53), (64, 64), (1, 70), (65, 129)):
        hw = h * w
        segs += [dict(size=[h, w], counts=[5, 7]), dict(size=[h, w], counts=[hw - 3, 1]), dict(size=[h, w], counts=[2, hw + 500]),
                 dict(size=[h, w], counts=[1, 2, 3, 2 ** 32 - 1, 9, 9]), dict(size=[h, w], counts=[0, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 5]),
                 dict(size=[h, w], counts=[hw, 4, 4]), dict(size=[h, w], counts="")]
    batch = M.RleBatch.from_coco(segs)
    need, guard = M.decode_bytes(batch), 4096
    buf = torch.full((need + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    got = M.decode(batch, out=buf[guard:guard + need])
    torch.cuda.synchronize()
    host = _np(buf)
    expect = np.full_like(host, 0xAB)
    pos = guard
    for g, s in zip(got, segs):
        h, w = s["size"]
        assert g.data_ptr() == buf.data_ptr() + pos
        counts = RH.counts_of_string(M.rle_to_string(s["counts"])) if s["counts"] != "" else []
        expect[pos:pos + h * w] = RH.mask_of_counts(counts, h, w).reshape(-1)
        pos += (h * w + 15) // 16 * 16
    assert pos == guard + need
    assert np.array_equal(host, expect), np.nonzero(host != expect)[0][:8]   # masks, the padding between them and both guard bands
    with pytest.raises(ValueError):
        M.decode(batch, device=DEV, check=True)
    for s in (segs[0], segs[2]):   # one short, one long
        with pytest.raises(ValueError):
            M.decode(M.RleBatch.from_coco([s]), device=DEV, check=True)


# ---- encode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_equals_the_restatement(cases, shape):
    items = cases[shape]
    dev = [torch.from_numpy(m).to(DEV) for _, m, _ in items]
    enc = M.encode(dev)
    assert enc.on_device and enc.data.dtype == torch.uint8 and int(enc.offsets[-1]) == enc.data.numel() == sum(len(s) for _, _, s in items)
    coco = enc.to_coco()
    for c, (name, m, s) in zip(coco, items):
        assert c["size"] == list(m.shape) and c["counts"] == s, (name, c["counts"][:40], s[:40])
    _check_decoded(M.decode(enc), items)                                     # decode(encode(m)) == m, the strings never leaving the device
    assert M.encode(M.decode(M.RleBatch.from_coco(_segms(items)), device=DEV)).to_coco() == coco
    for a, b, (name, m, _) in zip(_np(enc.area), _np(enc.bbox), items):
        assert int(a) == int(m.sum()), name


def test_encode_input_forms(cases):
    items = _mixed(cases)
    want = [s for _, _, s in items]
    masks = [torch.from_numpy(m).to(DEV) for _, m, _ in items]
    assert [c["counts"] for c in M.encode([m.bool() for m in masks]).to_coco()] == want
    assert [c["counts"] for c in M.encode([m * 255 for m in masks]).to_coco()] == want
    assert [c["counts"] for c in M.encode([m * 7 + (m * 64) for m in masks]).to_coco()] == want
    wide = []
    for m in masks:   # every mask a strided, offset slice of a larger tensor filled with ones
        h, w = m.shape
        big = torch.ones(2 * h + 3, 3 * w + 5, dtype=torch.uint8, device=DEV)
        big[1:1 + 2 * h:2, 2:2 + 3 * w:3] = m
        wide.append(big[1:1 + 2 * h:2, 2:2 + 3 * w:3])
        assert not wide[-1].is_contiguous()
    assert [c["counts"] for c in M.encode(wide).to_coco()] == want
    assert [c["counts"] for c in M.encode([m.t().contiguous().t() for m in masks]).to_coco()] == want     # column-major storage
    stack = torch.stack([torch.from_numpy(m).to(DEV) for _, m, _ in cases[(37, 53)]])                   # one [N, H, W] tensor
    assert [c["counts"] for c in M.encode(stack).to_coco()] == [s for _, _, s in cases[(37, 53)]]
    assert [c["counts"] for c in M.encode(stack.bool()[:, ::1, :]).to_coco()] == [s for _, _, s in cases[(37, 53)]]


def test_stats(cases):
    items = cases[(37, 53)] + cases[(65, 129)] + cases[(1, 70)] + cases[(70, 1)] + cases[(1, 1)] + cases[(130, 200)][9:]
    masks = [torch.from_numpy(m * 3).to(DEV) for _, m, _ in items]
    area, bbox = M.stats(masks)
    assert area.dtype == torch.int32 and bbox.dtype == torch.int32 and tuple(bbox.shape) == (len(items), 4) and area.device.type == "cuda"
    enc = M.encode(masks)
    assert torch.equal(enc.area, area) and torch.equal(enc.bbox, bbox)       # the shared pass
    empty = 0
    for a, b, (name, m, _) in zip(_np(area), _np(bbox), items):
        ys, xs = np.nonzero(m)
        assert int(a) == int(m.sum()), name
        if len(ys) == 0:
            empty += 1
            assert b.tolist() == [0, 0, m.shape[1] - 1, m.shape[0] - 1], name     # the bounds render.xyz_from_depth gives an empty mask
        else:
            assert b.tolist() == [xs.min(), ys.min(), xs.max(), ys.max()], name   # mask2bbox_xyxy, bottom-right inclusive
    assert empty >= 4


# ---- with its consumers ------------------------------------------------------------------------------------------------
def test_decoded_masks_feed_the_frame_augmenter():
    inputs = synth.make_augment_inputs()
    aug = A.FrameAugmenter(lmo_cfg(device=DEV), A.BackgroundBank(inputs["bank"], device=DEV), rng=np.random.default_rng(0))
    frames = [torch.from_numpy(f).to(DEV) for f in inputs["frames"][:3]]
    host_masks = [(np.asarray(m) != 0).astype(np.uint8) for m in inputs["masks"][:3]]
    segs = [dict(size=list(m.shape), counts=RH.mask_to_string(m)) for m in host_masks]
    plan = A.AugPlan([f.shape[:2] for f in frames])
    for i in range(3):
        plan.replace_bg[i], plan.bg_index[i], plan.trunc_mode[i], plan.trunc_u[i] = True, i, i, 0.6
    ours = aug.apply(frames, M.decode(M.RleBatch.from_coco(segs), device=DEV), plan)
    theirs = aug.apply(frames, [torch.from_numpy(RH.string_to_mask(s["counts"], *s["size"])).to(DEV) for s in segs], plan)
    for a, b, m in zip(ours, theirs, host_masks):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask_trunc"], b["mask_trunc"])
        assert 0 < int(a["mask_trunc"].sum()) <= int(m.sum())


def test_both_library_builds_agree(cases):
    """no 16-bit arithmetic in these kernels: libgdrn_hip.so and libgdrn_hip_f16.so give identical outputs"""
    items = _mixed(cases)
    batch = M.RleBatch.from_coco(_segms(items))
    outs = []
    for kind in (cabi.BF16, cabi.F16):
        lib = cabi.load(kind)
        dec = M.decode(batch, device=DEV, check=True, lib=lib)
        _check_decoded(dec, items)
        enc = M.encode(dec, lib=lib)
        area, bbox = M.stats(dec, lib=lib)
        outs.append((enc.to_coco(), _np(area).tolist(), _np(bbox).tolist()))
    assert outs[0] == outs[1] and [c["counts"] for c in outs[0][0]] == [s for _, _, s in items]
