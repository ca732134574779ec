#!/usr/bin/env python3
"""Generate golden G13 (``g13_xyz_targets.npz``) by running the REFERENCE's back-projection on the rasterizer fixtures.

Runs only where the reference checkout is present (see make_golden.py); only its outputs are stored.  Per scene of
``synth.make_render_inputs`` the fixture depth is the host rasterizer's output (tests/render_host.py, rounded to fp32 as the device writes it);
the reference's own ``misc.calc_xyz_bp_fast`` (lib/pysixd/misc.py:288-316) and ``mask2bbox_xyxy`` (lib/utils/mask_utils.py:39-44) run on it exactly
as ``tools/lm/lm_pbr_1_gen_xyz_crop.py:140-190`` chains them, the tool's whole-frame box standing in for an instance that is not visible.  Stored per
scene: the seed, the depth, the reference's xyz (fp64) and xyxy.  A seed is accepted only if no pixel centre lies within 1e-6 px of a triangle edge
(the "watertight" scene: unless it lies exactly on it, which is its purpose) and no depth within 1e-9 (relative) of near or far; otherwise the next
seed is taken and must be recorded in ``synth.RENDER_SEEDS``.

Usage:  python tests/golden/make_golden_g13.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_shims  # noqa: E402

CASES = ("cube", "watertight", "sphere", "mixed", "clip")
EDGE_BAND, NEAR_FAR_BAND = 1e-6, 1e-9


def seed_ok(case, stats):
    edge = stats["edge_band_off"] if case == "watertight" else stats["edge_band"]
    return edge > EDGE_BAND and stats["near_far_band"] > NEAR_FAR_BAND


def main():
    install_shims()
    from lib.pysixd import misc
    from lib.utils.mask_utils import mask2bbox_xyxy

    import render_host as RH
    from gdrnet_amd import synth

    g = {}
    for case in CASES:
        seed = synth.RENDER_SEEDS[case]
        while True:
            inp = synth.make_render_inputs(case, seed=seed)
            stats = {}
            depth = RH.render_depth(inp, stats)
            if seed_ok(case, stats):
                break
            print(f"case {case}: seed {seed} puts a pixel centre on an edge or a depth on near / far, trying the next one")
            seed += 1
        assert seed == synth.RENDER_SEEDS[case], f"record seed {seed} for case {case} in synth.RENDER_SEEDS"
        N, H, W = depth.shape
        xyz, xyxy = np.zeros((N, H, W, 3)), np.zeros((N, 4), dtype=np.int64)
        for i in range(N):
            mask = (depth[i] > 0).astype("uint8")
            if mask.sum() == 0:
                xyxy[i] = [0, 0, W - 1, H - 1]   # the tool's record, with an all-zero xyz (:147-150)
                continue
            xyxy[i] = mask2bbox_xyxy(mask)
            xyz[i] = misc.calc_xyz_bp_fast(depth[i], inp["R"][i], inp["t"][i], inp["K"][i])
        g[f"{case}/seed"], g[f"{case}/depth"], g[f"{case}/xyz"], g[f"{case}/xyxy"] = np.array(seed), depth, xyz, xyxy
        print(f"case {case}: seed {seed}, {N} x {H} x {W}, covered {[int((d != 0).sum()) for d in depth]}, edge band {stats['edge_band']:.3g} px "
              f"(off-edge {stats['edge_band_off']:.3g}), near / far band {stats['near_far_band']:.3g}")
    out = os.path.join(HERE, "g13_xyz_targets.npz")
    np.savez_compressed(out, **g)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
