#!/usr/bin/env python3
"""Generate golden G15 (``g15_augment.npz``) by running the REFERENCE's background replacement on the augmenter fixtures.

Runs only where the reference checkout is present (see make_golden.py); only its outputs are stored.

* ``replace_bg`` (core/base_data_loader.py:320-364) runs unbound on a stand-in object -- ``cfg`` with ``TRUNCATE_FG=True``, four background paths
  and a ``get_bg_image`` that returns ``synth.make_augment_inputs()["g15_bg"]`` -- on the 47 x 61 fixture frame and mask, under
  ``random.seed(k)`` for k = 0..11.  Replaying ``random.randint`` / ``random.random`` / ``random.uniform``'s draw with the same seed gives the
  background index, the cut mode and ``u``.  Stored per seed: index, mode, u, the composited image and the returned mask.
* ``get_bg_image`` (:366-403) runs with ``utils.read_image`` and ``cv2.resize`` replaced by recorders (OpenCV is not in the image), which yields the
  crop size, the scale and -- through cv2's documented ``dsize = round(fx * w), round(fy * h)`` -- the output size for every (bank size, frame
  size) pair of ``GEOM_BANKS`` x ``GEOM_FRAMES``.  Stored: one row (bh, bw, H, W, ch, cw, oh, ow) per pair and the scales.

Usage:  python tests/golden/make_golden_g15.py
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims  # noqa: E402

SEEDS = tuple(range(12))
NUM_BG = 4
GEOM_FRAMES = ((47, 61), (33, 9), (64, 96), (480, 640), (640, 480), (540, 720))


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def main():
    install_shims()
    import core.base_data_loader as bdl
    import core.utils.data_utils as du

    from gdrnet_amd import synth

    inp = synth.make_augment_inputs()
    frame, mask, bg = inp["frames"][0], inp["masks"][0], inp["g15_bg"]
    g = {"seeds": np.array(SEEDS), "num_bg": np.array(NUM_BG), "fixture_seed": np.array(inp["seed"])}

    class Stand:
        cfg = _Cfg(INPUT=_Cfg(TRUNCATE_FG=True, BG_KEEP_ASPECT_RATIO=True))
        _bg_img_paths = [f"bg{i}" for i in range(NUM_BG)]

        def get_bg_image(self, filename, H, W):
            return bg.copy()

    modes = []
    for k in SEEDS:
        random.seed(k)
        im, m = bdl.Base_DatasetFromList.replace_bg(Stand(), frame.copy(), mask.copy(), return_mask=True)
        random.seed(k)
        ind, rnd = random.randint(0, NUM_BG - 1), random.random()
        mode = 0 if rnd < 0.2 else 1 if rnd < 0.4 else 2 if rnd < 0.6 else 3 if rnd < 0.8 else 4
        u = random.random() if mode < 4 else 0.0   # random.uniform(a, b) = a + (b - a) * random()
        assert im.dtype == np.uint8 and m.dtype == bool and m.shape == mask.shape
        g[f"case{k}/index"], g[f"case{k}/mode"], g[f"case{k}/u"] = np.array(ind), np.array(mode), np.array(u, dtype=np.float64)
        g[f"case{k}/image"], g[f"case{k}/mask"] = im, m
        modes.append(mode)
        print(f"seed {k}: bg {ind}, mode {mode}, u {u:.6f}, kept {int(m.sum())} of {int((mask != 0).sum())} mask pixels")
    assert set(modes) == {0, 1, 2, 3, 4}, modes

    rec = {}

    def fake_resize(im, dsize, dst=None, fx=0, fy=0, interpolation=None):
        assert dsize is None and fx == fy
        oh, ow = int(np.rint(fy * im.shape[0])), int(np.rint(fx * im.shape[1]))   # cv2.resize: dsize = Size(round(fx * cols), round(fy * rows))
        rec.update(crop=im.shape[:2], scale=float(fx), out=(oh, ow))
        return np.zeros((oh, ow, 3), np.uint8)

    du.cv2.resize = fake_resize
    rows, scales = [], []
    for bh, bw in synth.AUG_BANK_SIZES:
        bdl.utils.read_image = lambda filename, format=None, _s=(bh, bw): np.zeros(_s + (3,), np.uint8)
        stand = Stand()
        stand.img_format = "BGR"
        for H, W in GEOM_FRAMES:
            out = bdl.Base_DatasetFromList.get_bg_image(stand, "bg0", H, W)
            assert out.shape == (H, W, 3)
            rows.append([bh, bw, H, W, rec["crop"][0], rec["crop"][1], rec["out"][0], rec["out"][1]])
            scales.append(rec["scale"])
    g["geometry"], g["geometry_scale"] = np.array(rows, dtype=np.int64), np.array(scales, dtype=np.float64)
    print(f"{len(rows)} (bank, frame) pairs ran without raising")
    out = os.path.join(HERE, "g15_augment.npz")
    np.savez_compressed(out, **g)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
