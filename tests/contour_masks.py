"""The masks of golden G20 (tests/golden/g20_contours.npz), by name: the observed masks of synth.make_silhouette_inputs from the host
rasterizer's renders, and hashed random masks -- blobs, noise, empty, full, a single pixel, masks touching every border.  Values are 0 / 1 uint8
(the reference's get_edge compares with 1)."""
import numpy as np

import sil_host as SH
from gdrnet_amd import synth

SEED = 2011
RANDOM_SHAPES = ((1, 1), (3, 3), (16, 3), (17, 5), (37, 53), (35, 64), (20, 130))


def random_mask(kind, shape, tag=""):
    """one hashed mask [H,W] uint8: "noise" (half the pixels), "blob" (a smoothed field above its median: a few regions that touch the borders),
    "empty", "full", "pixel" (one pixel set)"""
    H, W = shape
    name = f"{kind}/{H}x{W}{tag}"
    if kind == "empty":
        return np.zeros(shape, np.uint8)
    if kind == "full":
        return np.ones(shape, np.uint8)
    if kind == "pixel":
        m = np.zeros(shape, np.uint8)
        m[int(synth.hash_randint(SEED, name + "/y", (1,), 0, H)[0]), int(synth.hash_randint(SEED, name + "/x", (1,), 0, W)[0])] = 1
        return m
    u = synth.hash_uniform(SEED, name, shape)
    if kind == "noise":
        return (u < 0.5).astype(np.uint8)
    assert kind == "blob"
    p = np.pad(u, 2, mode="edge")
    s = sum(p[dy : dy + H, dx : dx + W] for dy in range(5) for dx in range(5))
    return (s > np.median(s)).astype(np.uint8)


def masks():
    out = {}
    for case in synth.SILHOUETTE_CASES:
        inp = synth.make_silhouette_inputs(case)
        _, m = synth.silhouette_scene(inp, SH.host_gt_depth(inp))
        for g in range(len(m)):
            out[f"{case}/{g}"] = m[g]
    for shape in RANDOM_SHAPES:
        for kind in ("noise", "blob", "empty", "full", "pixel"):
            out[f"{kind}/{shape[0]}x{shape[1]}"] = random_mask(kind, shape)
    return out
