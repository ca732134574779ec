#!/usr/bin/env python3
"""Time gdrnet_amd.frame_masks with HIP events.  The workload: 64 RoIs, eight to a frame, in 8 frames of 480 x 640; predicted-like maps of
64 x 64 (hashed noise under box filters, stretched to [0, 1], no files); crop squares of 64 to 128 pixels with hashed centres inside the frame.
Six calls, timed INTERLEAVED (one of each per round, 5 untimed rounds, then the median and range of 20), each behind an untimed 512 MB fill, so
that it writes to HBM and not into what the call before it left in the last-level cache:
  gdrn_roi_paste_masks alone   the plain paste on buffers allocated once (needed bytes: B H W written, the maps read)
  gdrn_roi_paste_exclusive     the same rows, every frame pixel to at most one of its frame's eight (B H W + 4 F H W written)
  gdrn_roi_components alone    the largest blob of the 64 maps
  masks_from_maps              get_out_mask, largest_component, paste_masks through the module: allocations and the geometry upload included
  fill                         tensor.zero_() of the same B H W bytes: the floor of a pass that must write every byte
  plain torch                  the same masks by F.grid_sample of all RoIs into frame-size maps (fp32), a threshold, masks.stats
Per call: ms; for the paste and the fill the written bytes per second.  Then paste / fill and plain torch / paste, round by round.  Nothing is
gated: the figures go into README.md.
Usage:  timeout 600 python tools/paste_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import write_json  # noqa: E402
from gdrnet_amd import cabi, devargs, frame_masks, masks, synth  # noqa: E402
from gdrnet_amd.cfg import lm13_cfg  # noqa: E402

WARMUP, ROUNDS = 5, 20


def smooth_maps(B, res, seed, passes=3):
    """[B, res, res] fp32 in [0, 1]: hashed noise under ``passes`` 5 x 5 box filters"""
    m = synth.hash_uniform(seed, "maps", (B, res, res))
    for _ in range(passes):
        p = np.pad(m, ((0, 0), (2, 2), (2, 2)), mode="edge")
        m = sum(p[:, dy:dy + res, dx:dx + res] for dy in range(5) for dx in range(5)) / 25.0
    lo, hi = m.min(axis=(1, 2), keepdims=True), m.max(axis=(1, 2), keepdims=True)
    return ((m - lo) / (hi - lo)).astype(np.float32)


def torch_paste(maps, cx, cy, scale, H, W, thr):
    """the plain-torch composition: (mask [B, H, W] uint8, area, bbox); maps [B, 1, res, res] fp32, cx / cy / scale [B] fp32 on the device"""
    res = maps.shape[-1]
    k = (res / scale)[:, None]
    u = (torch.arange(W, device=maps.device, dtype=torch.float32)[None, :] - cx[:, None]) * k + 0.5 * res
    v = (torch.arange(H, device=maps.device, dtype=torch.float32)[None, :] - cy[:, None]) * k + 0.5 * res
    gx, gy = 2.0 * (u + 0.5) / res - 1.0, 2.0 * (v + 0.5) / res - 1.0
    grid = torch.stack([gx[:, None, :].expand(-1, H, W), gy[:, :, None].expand(-1, H, W)], dim=-1)
    p = torch.nn.functional.grid_sample(maps, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    mask = (p > thr).to(torch.uint8)
    area, bbox = masks.stats(mask)
    return mask, area, bbox


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, B, H, W, F, res, seed, thr = "cuda:0", 64, 480, 640, 8, 64, 11, 0.5
    maps_host = smooth_maps(B, res, seed)
    u = synth.hash_uniform(seed, "geom", (B, 3))
    geom_host = np.ascontiguousarray(np.stack([40.0 + 560.0 * u[:, 0], 40.0 + 400.0 * u[:, 1], 64.0 + 64.0 * u[:, 2]], axis=1))
    frame_host = (np.arange(B, dtype=np.int32) % F).astype(np.int32)
    csr_host = frame_masks._csr(frame_host, F)
    maps, geom, csr = torch.from_numpy(maps_host).to(dev), torch.from_numpy(geom_host).to(dev), torch.from_numpy(csr_host).to(dev)
    pred = (1.4 * maps - 0.2)[:, None].contiguous()               # as the network emits it: get_out_mask stretches it back
    cfg = lm13_cfg(device=dev)
    cx32, cy32, s32 = (geom[:, j].float().contiguous() for j in range(3))

    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(torch.device(dev))
    i32 = dict(dtype=torch.int32, device=dev)
    o_mask, o_area, o_bbox = torch.empty(B, H, W, dtype=torch.uint8, device=dev), torch.empty(B, **i32), torch.empty(B, 4, **i32)
    x_mask, x_area, x_bbox, x_index = torch.empty_like(o_mask), torch.empty(B, **i32), torch.empty(B, 4, **i32), torch.empty(F, H, W, **i32)
    c_filtered, c_num, c_kept = torch.empty_like(maps), torch.empty(B, **i32), torch.empty(B, **i32)
    fill_buf = torch.empty(B, H, W, dtype=torch.uint8, device=dev)

    def paste():
        cabi.check(lib.gdrn_roi_paste_masks(p(maps), p(geom), geom_host.ctypes.data, B, res, H, W, thr, p(o_mask), p(o_area), p(o_bbox), st),
                   "roi_paste_masks")

    def exclusive():
        cabi.check(lib.gdrn_roi_paste_exclusive(p(maps), p(geom), geom_host.ctypes.data, frame_host.ctypes.data, p(csr), csr_host.ctypes.data, B, F, res,
                                                H, W, thr, p(x_index), p(x_mask), p(x_area), p(x_bbox), st), "roi_paste_exclusive")

    def components():
        cabi.check(lib.gdrn_roi_components(p(maps), B, res, thr, p(c_filtered), p(c_num), p(c_kept), st), "roi_components")

    n_px = B * H * W
    calls = [("gdrn_roi_paste_masks alone", paste, n_px),
             ("gdrn_roi_paste_exclusive", exclusive, n_px + 4 * F * H * W),
             ("gdrn_roi_components alone", components, None),
             ("masks_from_maps", lambda: frame_masks.masks_from_maps(cfg, dict(mask=pred), geom_host[:, :2], geom_host[:, 2], H, W), None),
             ("fill of B H W bytes", lambda: fill_buf.zero_(), n_px),
             ("plain torch: grid_sample, threshold, masks.stats", lambda: torch_paste(maps[:, None], cx32, cy32, s32, H, W, thr), None)]
    times, last = [[] for _ in calls], [None] * len(calls)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for it in range(WARMUP + ROUNDS):
        for k, (_, fn, _) in enumerate(calls):
            flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = fn()
            e1.record()
            e1.synchronize()
            if it >= WARMUP:
                times[k].append(e0.elapsed_time(e1))
    ref = frame_masks.paste_masks(maps, geom_host[:, :2], geom_host[:, 2], H, W, thr)
    assert torch.equal(ref["mask"], o_mask) and torch.equal(ref["area"], o_area) and torch.equal(ref["bbox"], o_bbox)
    area, bbox = masks.stats(x_mask)
    assert torch.equal(area, x_area) and torch.equal(bbox, x_bbox) and int(x_mask.view(B // F, F, H, W).sum(dim=0).max()) <= 1
    t_mask = last[5][0]
    shape = dict(B=B, F=F, H=H, W=W, res=res, rounds=ROUNDS, set_fraction=float(o_mask.float().mean()),
                 pixels_inside_a_square=float(((geom_host[:, 2] + 1.0) ** 2).sum() / n_px),
                 exclusive_pixels_lost=int(o_area.sum() - x_area.sum()), components_median=float(c_num.float().median()),
                 torch_fp32_pixels_that_differ=int((t_mask != o_mask).sum()))
    res_rows = []
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        if nbytes is not None:
            row.update(written_mbytes=nbytes / 1e6, gb_per_s=nbytes / (ms * 1e-3) / 1e9)
        res_rows.append(row)
        print(json.dumps(row), flush=True)
    med = [statistics.median(ts) for ts in times]
    r_fill = [a / b for a, b in zip(times[0], times[4])]   # round by round
    r_torch = [a / b for a, b in zip(times[5], times[0])]
    verdict = dict(paste_over_fill=med[0] / med[4], paste_over_fill_min=min(r_fill), paste_over_fill_max=max(r_fill),
                   torch_over_paste=med[5] / med[0], torch_over_paste_min=min(r_torch), torch_over_paste_max=max(r_torch),
                   exclusive_over_paste=med[1] / med[0], chain_over_its_kernels=med[3] / (med[0] + med[2]))
    print(json.dumps(verdict), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res_rows, **shape, **verdict)


if __name__ == "__main__":
    main()
