"""GPU parity of the frame augmenter (gdrnet_amd.augment) through the C ABI: every comparison is exact equality with the host restatement
(tests/aug_host.py) -- all stages are integer or strictly ordered fp32 -- and with golden G15 (the reference's own replace_bg) where it applies."""
import os

import numpy as np
import pytest
import torch

import aug_host as AH
from gdrnet_amd import augment as A, cabi, roi_data, synth
from gdrnet_amd.cfg import lm13_cfg, lmo_cfg
from oracle import roi_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G15_BG = 4   # index of the ready-made 47 x 61 background in the test bank (behind the four fixture images)


@pytest.fixture(scope="module")
def inputs():
    d = synth.make_augment_inputs()
    d["bank_all"] = d["bank"] + [d["g15_bg"]]
    return d


@pytest.fixture(scope="module")
def aug(inputs):
    return A.FrameAugmenter(lmo_cfg(device=DEV), A.BackgroundBank(inputs["bank_all"], device=DEV), rng=np.random.default_rng(0))


def _keep(tag, gh, gw, p=0.3):
    k = synth.hash_uniform(15, tag, (gh, gw)) >= p
    k.flat[0], k.flat[-1] = False, True   # both kinds of cell in every grid
    return k


def _check(aug, bank, frames, masks, plan):
    """apply on the device, compare every frame with the host restatement; returns the outputs"""
    tf = [torch.from_numpy(f).to(DEV) for f in frames]
    tm = [None if m is None else torch.from_numpy(m).to(DEV) for m in masks]
    out = aug.apply(tf, tm, plan)
    torch.cuda.synchronize()
    assert len(out) == len(frames)
    for i, o in enumerate(out):
        img, trunc = AH.augment_frame(frames[i], masks[i], bank, plan, i)
        got = o["image"].cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == frames[i].shape
        assert np.array_equal(got, img), (i, plan.hw[i], int((got != img).sum()), int(np.abs(got.astype(int) - img).max()))
        if trunc is None:
            assert o["mask_trunc"] is None, i
        else:
            mt = o["mask_trunc"].cpu().numpy()
            assert mt.dtype == np.uint8 and np.array_equal(mt, trunc), i
        assert np.array_equal(tf[i].cpu().numpy(), frames[i])            # the inputs are not modified
        assert masks[i] is None or np.array_equal(tm[i].cpu().numpy(), masks[i])
    return out


def test_background_replacement_on_every_pair_and_cut_mode(aug, inputs):
    frames, masks, idx = [], [], []
    for fi in range(3):
        for bi in range(4):
            for mode in range(5):
                frames.append(inputs["frames"][fi])
                masks.append(inputs["masks"][fi])
                idx.append((bi, mode))
    plan = A.AugPlan([f.shape[:2] for f in frames])
    us = 0.2 + 0.75 * synth.hash_uniform(15, "trunc_u", (len(frames),))   # (far enough in that every cut removes at least a row / column)
    for i, (bi, mode) in enumerate(idx):
        plan.replace_bg[i], plan.bg_index[i], plan.trunc_mode[i], plan.trunc_u[i] = True, bi, mode, float(us[i]) if mode < 4 else 0.0
    out = _check(aug, inputs["bank_all"], frames, masks, plan)
    kept = [int(o["mask_trunc"].sum()) for o in out[:5]]
    assert all(k < kept[4] for k in kept[:4]) and kept[4] == int((inputs["masks"][0] != 0).sum())   # every cut removed something


def test_g15_composites_of_the_reference(aug, inputs, golden_dir):
    g = np.load(os.path.join(golden_dir, "g15_augment.npz"))
    n = len(g["seeds"])
    frames, masks = [inputs["frames"][0]] * n, [inputs["masks"][0]] * n
    plan = A.AugPlan([(47, 61)] * n)
    for i, k in enumerate(g["seeds"]):
        plan.replace_bg[i], plan.bg_index[i] = True, G15_BG
        plan.trunc_mode[i], plan.trunc_u[i] = int(g[f"case{k}/mode"]), float(g[f"case{k}/u"])
    out = _check(aug, inputs["bank_all"], frames, masks, plan)
    for i, k in enumerate(g["seeds"]):
        assert np.array_equal(out[i]["image"].cpu().numpy(), g[f"case{k}/image"]), k
        assert np.array_equal(out[i]["mask_trunc"].cpu().numpy().astype(bool), g[f"case{k}/mask"]), k


def test_empty_mask_gives_an_all_background_frame(aug, inputs):
    frames = [inputs["frames"][0], inputs["frames"][2]]
    masks = [np.zeros(f.shape[:2], np.uint8) for f in frames]
    plan = A.AugPlan([f.shape[:2] for f in frames])
    for i in range(2):
        plan.replace_bg[i], plan.bg_index[i], plan.trunc_mode[i], plan.trunc_u[i] = True, 2 + i, i, 0.5
    out = _check(aug, inputs["bank_all"], frames, masks, plan)
    for i, o in enumerate(out):
        assert not o["mask_trunc"].any()
        assert np.array_equal(o["image"].cpu().numpy(), AH.background(inputs["bank_all"][2 + i], *frames[i].shape[:2]))


def _colour_plans(hw):
    """(name, setter) of the single-stage plans and the full chain for a frame of size hw"""
    H, W = hw
    small, large = A.dropout_grid(H, W, 0.05), A.dropout_grid(H, W, 0.2)
    points = [("Add", (-40, 7, 90)), ("Invert", (1, 0, 1)), ("Multiply", (0.61, 1.0, 1.39)), ("Multiply", (1.2, 1.2, 1.2)), ("LinearContrast", (0.5, 2.2, 1.3))]
    cases = [("dropout_min", dict(dropout=_keep("k_small", *small))), ("dropout", dict(dropout=_keep("k_large", *large))),
             ("blur_r2", dict(blur_sigma=1.1)), ("blur_r3", dict(blur_sigma=1.9)), ("blur_r4", dict(blur_sigma=2.9)), ("blur_skipped", dict(blur_sigma=5e-4))]
    cases += [(p[0].lower(), dict(point_ops=[p])) for p in points]
    cases.append(("chain", dict(dropout=_keep("k_chain", *large), blur_sigma=0.8, point_ops=points)))
    cases.append(("chain_r4", dict(dropout=_keep("k_chain4", *small), blur_sigma=2.5, point_ops=points[::-1])))
    return small, cases


@pytest.mark.parametrize("fi", [0, 1, 2])
def test_each_colour_op_alone_and_the_full_chain(aug, inputs, fi):
    frame, mask = inputs["frames"][fi], inputs["masks"][fi]
    small, cases = _colour_plans(frame.shape[:2])
    assert small[0] == 3 and small[1] in (3, 4)   # the 3-cell minimum
    n = len(cases) + 2
    plan = A.AugPlan([frame.shape[:2]] * n)
    for i, (_, fields) in enumerate(cases):
        plan.color[i] = True
        for k, v in fields.items():
            getattr(plan, k)[i] = v
    for j, i in enumerate((n - 2, n - 1)):   # the chain behind a replaced background, up- and down-scaled
        plan.replace_bg[i], plan.bg_index[i], plan.trunc_mode[i], plan.trunc_u[i], plan.color[i] = True, (0, 3)[j], 1 + j, 0.4, True
        for k, v in cases[-2 + j][1].items():
            getattr(plan, k)[i] = v
    out = _check(aug, inputs["bank_all"], [frame] * n, [None] * (n - 2) + [mask, mask], plan)
    skipped = [c[0] for c in cases].index("blur_skipped")
    changed = [not np.array_equal(o["image"].cpu().numpy(), frame) for o in out]
    assert all(c for i, c in enumerate(changed) if i != skipped), changed


def test_mixed_batch_with_idle_and_colour_only_frames(aug, inputs):
    frames = [inputs["frames"][i % 3] for i in range(7)]
    masks = [inputs["masks"][i % 3] for i in range(7)]
    plan = A.AugPlan([f.shape[:2] for f in frames])
    plan.replace_bg[0], plan.bg_index[0], plan.trunc_mode[0], plan.trunc_u[0] = True, 1, 3, 0.25
    plan.color[1], plan.point_ops[1] = True, [("Add", (9, 9, 9))]                                 # colour only
    plan.color[3] = True                                                                           # colour drawn, no op fired: idle
    plan.color[4], plan.blur_sigma[4] = True, 1e-4                                                 # a blur below the threshold: idle
    plan.replace_bg[5], plan.bg_index[5], plan.color[5], plan.blur_sigma[5] = True, 2, True, 1.4
    plan.color[6], plan.dropout[6] = True, _keep("k_mixed", 3, 5)
    tf = [torch.from_numpy(f).to(DEV) for f in frames]
    tm = [torch.from_numpy(m).to(DEV).bool() if i == 5 else torch.from_numpy(m).to(DEV) for i, m in enumerate(masks)]   # a bool mask too
    out = aug.apply(tf, tm, plan)
    again = aug.apply(tf, [tm[0], None, None, None, None, tm[5], None], plan)
    torch.cuda.synchronize()
    for i in (2, 3, 4):
        assert out[i]["image"] is tf[i] and out[i]["mask_trunc"] is None
    for i in (1, 6):
        assert out[i]["mask_trunc"] is None and out[i]["image"] is not tf[i]
    for i in range(7):
        img, trunc = AH.augment_frame(frames[i], masks[i], inputs["bank_all"], plan, i)
        assert np.array_equal(out[i]["image"].cpu().numpy(), img), i
        assert (trunc is None and out[i]["mask_trunc"] is None) or np.array_equal(out[i]["mask_trunc"].cpu().numpy(), trunc), i
        # a second apply of the same plan: identical bytes
        assert torch.equal(out[i]["image"], again[i]["image"])
        assert (out[i]["mask_trunc"] is None and again[i]["mask_trunc"] is None) or torch.equal(out[i]["mask_trunc"], again[i]["mask_trunc"])
        assert np.array_equal(tf[i].cpu().numpy(), frames[i])


def test_sampled_plans_through_call(inputs):
    """aug(frames, masks, img_types) = apply(sample): the shipped chain on a batch of mixed sizes, equal to the host on the plan it drew"""
    bank = A.BackgroundBank(inputs["bank_all"], device=DEV)
    a = A.FrameAugmenter(lmo_cfg(device=DEV), bank, rng=np.random.default_rng(77))
    b = A.FrameAugmenter(lmo_cfg(device=DEV), bank, rng=np.random.default_rng(77))
    frames = [inputs["frames"][i % 3] for i in range(24)]
    masks = [inputs["masks"][i % 3] for i in range(24)]
    types = ["syn" if i % 4 == 0 else "real" for i in range(24)]
    plan = b.sample([(f.shape[0], f.shape[1], t) for f, t in zip(frames, types)])
    assert sum(plan.color) > 10 and sum(plan.replace_bg) > 8 and any(s is not None for s in plan.blur_sigma)
    out = a([torch.from_numpy(f).to(DEV) for f in frames], [torch.from_numpy(m).to(DEV) for m in masks], types)
    torch.cuda.synchronize()
    for i in range(24):
        img, trunc = AH.augment_frame(frames[i], masks[i], inputs["bank_all"], plan, i)
        assert np.array_equal(out[i]["image"].cpu().numpy(), img), i
        assert (trunc is None) == (out[i]["mask_trunc"] is None)


def test_argument_errors(aug, inputs):
    f, m = torch.from_numpy(inputs["frames"][0]).to(DEV), torch.from_numpy(inputs["masks"][0]).to(DEV)
    plan = A.AugPlan([(47, 61)])
    plan.replace_bg[0] = True
    with pytest.raises(ValueError):
        aug.apply([f], [None], plan)                       # the plan replaces the background: a mask is needed
    with pytest.raises(ValueError):
        aug.apply([f], [m[:, :60]], plan)
    with pytest.raises(cabi.GdrnHipError):
        aug.apply([f.cpu()], [m], plan)
    with pytest.raises(cabi.GdrnHipError):
        aug.apply([f], [m.cpu()], plan)
    plan.bg_index[0] = 5
    with pytest.raises(ValueError):
        aug.apply([f], [m], plan)
    thin = A.AugPlan([(4, 40)])
    thin.color[0], thin.blur_sigma[0] = True, 2.9          # radius 4 on a 4-row frame
    with pytest.raises(ValueError):
        aug.apply([torch.zeros(4, 40, 3, dtype=torch.uint8, device=DEV)], None, thin)
    with pytest.raises(ValueError):
        aug.apply([f], None, A.AugPlan([(47, 60)]))


def test_augmented_frames_feed_the_roi_cropper():
    """decoded frame -> augmenter -> RoiCropper(train=True): the cropper takes the outputs as they are, and roi_mask_trunc is the crop of the cut
    mask -- zero wherever the cut removed it"""
    d = synth.make_roi_frames(6)
    bank_np = [np.floor(synth.hash_uniform(15, "roi_bank", (375, 500, 3)) * 256).astype(np.uint8)]
    aug = A.FrameAugmenter(lmo_cfg(device=DEV), A.BackgroundBank(bank_np, device=DEV), rng=np.random.default_rng(4))
    frames = [d["frames"][r["frame"]] for r in d["rois"]]
    masks = [r["segmentation"] for r in d["rois"]]
    plan = A.AugPlan([f.shape[:2] for f in frames])
    for i in range(6):
        plan.replace_bg[i], plan.trunc_mode[i], plan.trunc_u[i] = True, i % 5, 0.5
        plan.color[i], plan.blur_sigma[i], plan.point_ops[i] = i % 2 == 0, 1.0, [("Multiply", (0.8, 1.1, 1.3))]
    out = _check(aug, bank_np, frames, masks, plan)
    rois = []
    for r, o in zip(d["rois"], out):
        q = dict(r)
        q.update(image=o["image"], mask_trunc=o["mask_trunc"], xyz_crop=torch.from_numpy(r["xyz_crop"]).to(DEV),
                 segmentation=torch.from_numpy(r["segmentation"]).to(DEV))
        rois.append(q)
    crop = roi_data.RoiCropper(lm13_cfg(device=DEV), extents=d["extents"], fps_points=d["fps_points"], device=DEV)(rois, train=True)
    torch.cuda.synchronize()
    cut_something = 0
    for n, r in enumerate(d["rois"]):
        H, W = frames[n].shape[:2]
        trunc = AH.truncate_mask(r["segmentation"] != 0, plan.trunc_mode[n], plan.trunc_u[n]).astype(np.uint8)
        ref = R.roi_targets(r["xyz_crop"], r["xyxy"], r["segmentation"], trunc, (H, W), r["bbox_center"], r["scale"], r["bbox"],
                            d["extents"][r["roi_cls"]], d["fps_points"][r["roi_cls"]], r["trans"], r["centroid_2d"])
        got, visib = crop["roi_mask_trunc"][n].cpu().numpy(), crop["roi_mask_visib"][n].cpu().numpy()
        assert np.array_equal(got, ref["roi_mask_trunc"]), n
        removed = R.roi_targets(r["xyz_crop"], r["xyxy"], r["segmentation"], 1 - trunc, (H, W), r["bbox_center"], r["scale"], r["bbox"],
                                d["extents"][r["roi_cls"]], d["fps_points"][r["roi_cls"]], r["trans"], r["centroid_2d"])["roi_mask_trunc"]
        assert not got[removed > 0].any(), n               # zero wherever the cut removed the mask
        cut_something += int((removed > 0).any())
        assert (got <= visib).all()
    assert cut_something >= 3
    assert bool(torch.isfinite(crop["roi_img"]).all())
