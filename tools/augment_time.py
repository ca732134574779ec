#!/usr/bin/env python3
"""Time gdrnet_amd.augment with HIP events: median of 20 calls after 5 warm-ups, 64 frames of 480 x 640 with masks, a bank of 375 x 500 images,
for three kinds of plan:
  full chain        every frame replaces its background (cut modes cycling) and runs every stage of the shipped chain (dropout, blur, 5 point ops),
  background only   replacement and cut, no colour stage,
  colour only       the colour stages on the frame as it is (no mask, no mask_trunc).
Reported per kind, for ``apply`` (host preparation -- table composition, output allocation, the upload -- and both launches, as the events see
them) and for ``launch`` alone on a prepared batch (the kernels): ms per batch, frames/s and GB/s over the bytes the kernels must move -- frame +
output, and mask + mask_trunc where the background is replaced (the bank reads come on top).  Reported, not gated: there is no earlier device
path to compare with.  Usage:  timeout 300 python tools/augment_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import augment as A, synth  # noqa: E402
from gdrnet_amd.cfg import lmo_cfg  # noqa: E402

B, H, W, BANK, SEED = 64, 480, 640, 8, 17


def plans(aug):
    full, bg, colour = A.AugPlan([(H, W)] * B), A.AugPlan([(H, W)] * B), A.AugPlan([(H, W)] * B)
    rng = np.random.default_rng(SEED)
    ops = {o["op"]: o for o in aug.ops}
    for i in range(B):
        for p in (full, bg):
            p.replace_bg[i], p.bg_index[i], p.trunc_mode[i], p.trunc_u[i] = True, i % BANK, i % 5, 0.5
        for p in (full, colour):
            p.color[i] = True
            p.dropout[i] = rng.random(A.dropout_grid(H, W, ops["CoarseDropout"]["size_percent"])) >= ops["CoarseDropout"]["p"]
            p.blur_sigma[i] = 1.0
            p.point_ops[i] = [("Add", (-20, 5, 20)), ("Invert", (0, 1, 0)), ("Multiply", (0.8, 1.0, 1.3)), ("Multiply", (1.1,) * 3), ("LinearContrast", (1.4,) * 3)]
    return (("full chain", full, True), ("background only", bg, True), ("colour only", colour, False))


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    u8 = lambda tag, *shape: torch.from_numpy(np.floor(synth.hash_uniform(SEED, tag, shape) * 256).astype(np.uint8)).to(dev)  # noqa: E731
    bank = A.BackgroundBank([u8(f"bank{i}", 375, 500, 3) for i in range(BANK)], device=dev)
    aug = A.FrameAugmenter(lmo_cfg(device=dev), bank, rng=np.random.default_rng(SEED))
    frames = [u8(f"frame{i}", H, W, 3) for i in range(B)]
    masks = []
    for i in range(B):
        m = torch.zeros(H, W, dtype=torch.uint8, device=dev)
        m[100 + i : 300 + i, 150 + 2 * i : 420 + 2 * i] = 1
        masks.append(m)
    res = []
    for name, plan, with_mask in plans(aug):
        prep = aug.prepare(frames, masks if with_mask else None, plan)
        nbytes = B * H * W * (3 + 3 + (2 if with_mask else 0))
        for call, fn in (("apply", lambda: aug.apply(frames, masks if with_mask else None, plan)), ("launch", lambda: aug.launch(prep))):
            times = timed(fn)[1]
            ms = statistics.median(times)
            row = dict(call=f"{call}, {name}", frames=B, H=H, W=W, gpu_ms_median=ms, gpu_ms_min=min(times), gpu_ms_max=max(times),
                       frames_per_s=B / ms * 1e3, gb_per_s=nbytes / ms / 1e6)
            res.append(row)
            print(json.dumps(row), flush=True)
    write_json(res)


if __name__ == "__main__":
    main()
