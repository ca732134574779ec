#!/usr/bin/env python3
"""Time gdrnet_amd.masks with HIP events: median of 20 calls after 5 warm-ups, 64 masks of 480 x 640, each an object silhouette (a filled ellipse
with axes of 60-200 px, the size of an LM / YCB-V instance; strings of about 0.5 KB).  Reported:
  decode    the two launches (parse, fill) of a prepared batch;  ``decode`` of a host batch with its one upload (strings + task table);  and, beside
            them, what decode replaces on the device side: the pinned host-to-device copy of the 64 decoded masks (19.7 MB)
  encode    every entry point alone on prepared buffers (count with area / bbox; scan + emit; string lengths; string write), the four in a row,
            ``encode`` with its one read of the 64 string lengths, and ``encode`` + ``to_coco()`` with the read of the strings
  GB/s      over the mask bytes the kernels must move once: written by fill (its figure includes the parse launch), read by count
Reported, not gated: there is no earlier device path to compare with, and the host decoder the reference uses (pycocotools) is not part of this
project.  Usage:  timeout 300 python tools/rle_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timed, write_json  # noqa: E402
from gdrnet_amd import cabi, masks as M  # noqa: E402

B, H, W, SEED = 64, 480, 640, 23


def silhouettes():
    rng = np.random.default_rng(SEED)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), np.uint8)
    for i in range(B):
        ay, ax = rng.uniform(30, 100, 2)   # half axes: 60-200 px across
        cy, cx = rng.uniform(ay, H - ay), rng.uniform(ax, W - ax)
        out[i] = ((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1.0
    return out


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    lib = cabi.load()
    host_masks = silhouettes()
    pinned = torch.from_numpy(host_masks).pin_memory()
    dev_masks = pinned.to(dev)
    batch = M.RleBatch.from_coco(M.encode(dev_masks).to_coco())   # the host batch a dataset would hold
    got = torch.stack(M.decode(batch, device=dev, check=True))
    assert torch.equal(got, dev_masks), "decode(encode(m)) != m"
    nbytes = B * H * W
    res = []

    def report(call, fn, gb=None):
        times = timed(fn)[1]
        ms = statistics.median(times)
        row = dict(call=call, masks=B, H=H, W=W, gpu_ms_median=ms, gpu_ms_min=min(times), gpu_ms_max=max(times), masks_per_s=B / ms * 1e3)
        if gb:
            row["gb_per_s"] = gb / ms / 1e6
        res.append(row)
        print(json.dumps(row), flush=True)

    prep = M.decode_prepare(batch, device=dev)
    report("decode, launches (parse + fill)", lambda: M.decode_launch(prep), nbytes)
    report("decode, with the upload of the strings", lambda: M.decode(batch, device=dev))
    dst = torch.empty_like(dev_masks)
    report("pinned host-to-device copy of the decoded masks", lambda: dst.copy_(pinned, non_blocking=True), nbytes)

    masks = list(dev_masks.unbind(0))
    th, table, nseg, npos = M._encode_table(masks, dev)
    tab, st = table.data_ptr(), torch.cuda.current_stream(dev).cuda_stream
    i32 = dict(dtype=torch.int32, device=dev)
    seg, positions, ntrans = torch.empty(nseg, **i32), torch.empty(npos, **i32), torch.empty(B, **i32)
    area, bbox, lengths = torch.empty(B, **i32), torch.empty(B, 4, **i32), torch.empty(B, dtype=torch.int64, device=dev)
    P = cabi.ptr

    def count():
        cabi.check(lib.gdrn_rle_count(tab, th, B, P(seg), nseg, P(area), P(bbox), st), "rle_count")

    def positions_():
        cabi.check(lib.gdrn_rle_positions(tab, th, B, P(seg), nseg, P(ntrans), P(positions), npos, st), "rle_positions")

    def string_lengths():
        cabi.check(lib.gdrn_rle_string(tab, th, B, P(ntrans), P(positions), npos, None, None, 0, P(lengths), st), "rle_string")

    count(), positions_(), string_lengths()
    offsets = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lengths.cpu().numpy(), out=offsets[1:])
    offs, strings = torch.from_numpy(offsets).to(dev), torch.empty(int(offsets[-1]), dtype=torch.uint8, device=dev)

    def string_write():
        cabi.check(lib.gdrn_rle_string(tab, th, B, P(ntrans), P(positions), npos, P(offs), P(strings), strings.numel(), None, st), "rle_string")

    def positions_after_count():   # (the scan is in place: it needs fresh counts every time)
        count()
        positions_()

    report("encode, count + area / bbox", count, nbytes)
    report("encode, count + scan + emit", positions_after_count)
    report("encode, string lengths", string_lengths)
    report("encode, string write", string_write)
    report("encode, the four entry points in a row", lambda: (count(), positions_(), string_lengths(), string_write()))
    report("encode, with its read of the lengths", lambda: M.encode(masks))
    report("encode + to_coco, both reads", lambda: M.encode(masks).to_coco())
    report("stats (area, bbox) alone", lambda: M.stats(masks), nbytes)
    print(json.dumps(dict(string_bytes=int(batch.offsets[-1]), mask_bytes=nbytes)), flush=True)
    write_json(res, string_bytes=int(batch.offsets[-1]))


if __name__ == "__main__":
    main()
