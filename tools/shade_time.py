#!/usr/bin/env python3
"""Time gdrnet_amd.shade with HIP events.  The workload is 64 instances of the 20 480-face perturbed icosphere in 8 frames of 480 x 640, one call
with backgrounds.  Five calls on the same inputs, timed INTERLEAVED (one of each per round, 5 untimed rounds, then the median of 20):
  render_depth                 the depth rasterizer alone (clear, raster with 32-bit atomic min, resolve)
  render_visibility            the same walk with 64-bit keys (clear, raster with 64-bit atomic min; no resolve): twice the bytes per
                               fragment and per clear
  gdrn_shade_frames            the shade-and-compose pass alone on the keys, with backgrounds and every optional map off / on, with the bytes it
                               needs (N H W 8 read, F H W 11 written, + F H W 3 read for the backgrounds, + F H W 7 with face and normal maps)
                               over the time, and that rate's share of the HBM peak (8.0 TB/s specified, 6.3 TB/s a float4 copy reaches)
  gdrn_shade_frames, empty     the same call on keys that are all ~0 (no pixel covered: every frame is its background): the streaming part of
                               the pass alone, without the fp64 shading of the covered pixels and their gathers from the mesh table
  gdrn_scene_gt_compose        the pass of the same access pattern (every instance's map read once, one frame map written), measured in the
                               same rounds for comparison
then render_frames as a user calls it (visibility + shade + the two small uploads).  The calls that are rated in bytes per second run behind an
untimed 512 MB fill, so that each reads its inputs from HBM and not from what the call before it left in the 256 MB last-level cache.
Reported, not gated: there is no earlier device path.
Usage:  timeout 600 python tools/shade_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import write_json  # noqa: E402
from gdrnet_amd import cabi, devargs, render, scene_gt as SG, shade, synth  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12   # bytes / s
WARMUP, ROUNDS = 5, 20


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, F, seed = torch.device("cuda:0"), 64, 480, 640, 8, 7
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R = torch.from_numpy(synth._random_rotations(seed, "R", N)).to(dev)
    t = torch.from_numpy(np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)).to(dev)
    K = torch.from_numpy(np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)).to(dev)
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    table = shade.ShadedMeshTable([v], [f], [0.2 + 0.7 * u("col", len(v), 3)], device=dev)
    labels, frame = np.zeros(N, dtype=np.int64), np.arange(N) // (N // F)
    bg = torch.from_numpy(np.floor(256.0 * u("bg", F, H, W, 3)).astype(np.uint8)).to(dev)
    light, phong = shade.random_lights(F, np.random.default_rng(seed))

    full = shade.render_frames(table, labels, R, t, K, H, W, frame, F, light, phong, bg, want_face=True, want_normals=True)
    depth = render.render_depth(table, labels, R, t, K, H, W)
    assert torch.equal(shade.visibility_depth(full.vis).view(torch.int32), depth.view(torch.int32))
    lib, p, st, tb = cabi.load(), cabi.ptr, devargs.stream(dev), table.on(dev)
    lab_host = labels.astype(np.int32)
    lab = torch.from_numpy(lab_host).to(dev)
    off_host, inst_host = SG.csr_of_frames(frame, F)
    off, inst = torch.from_numpy(off_host).to(dev), torch.from_numpy(inst_host).to(dev)
    li, ph = torch.from_numpy(light).to(dev), torch.from_numpy(phong).to(dev)
    vis, composed = full.vis, torch.empty(F, H, W, dtype=torch.float32, device=dev)
    rgb, zmap, index = torch.empty_like(full.rgb), torch.empty_like(full.depth), torch.empty_like(full.index)
    face, nmap = torch.empty_like(full.face), torch.empty_like(full.normals)

    empty = torch.full_like(vis, -1)

    def shade_call(background, fc, nm, keys=vis):
        cabi.check(lib.gdrn_shade_frames(p(keys), p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]),
                                         p(tb["normals"]), p(tb["colors"]), 1, p(lab), lab_host.ctypes.data, p(R), p(t), p(K), p(off),
                                         off_host.ctypes.data, p(inst), inst_host.ctypes.data, F, N, H, W, p(li), p(ph), p(background), p(rgb), p(zmap),
                                         p(index), p(fc), p(nm), st), "shade_frames")

    b_keys, px = N * H * W * 8, F * H * W
    calls = [
        ("render_depth", lambda: render.render_depth(table, labels, R, t, K, H, W), None),
        ("render_visibility", lambda: shade.render_visibility(table, labels, R, t, K, H, W), None),
        ("gdrn_shade_frames, no background", lambda: shade_call(None, None, None), b_keys + px * 11),
        ("gdrn_shade_frames with backgrounds", lambda: shade_call(bg, None, None), b_keys + px * 14),
        ("gdrn_shade_frames with backgrounds, empty keys (streaming part alone)", lambda: shade_call(bg, None, None, empty), b_keys + px * 14),
        ("gdrn_shade_frames with backgrounds, face and normal maps", lambda: shade_call(bg, face, nmap), b_keys + px * 21),
        ("gdrn_scene_gt_compose", lambda: cabi.check(lib.gdrn_scene_gt_compose(p(depth), p(off), off_host.ctypes.data, p(inst), inst_host.ctypes.data, F, N,
                                                                               H, W, p(composed), st), "compose"), N * H * W * 4 + px * 4),
        ("render_frames (visibility + shade + uploads), backgrounds", lambda: shade.render_frames(table, labels, R, t, K, H, W, frame, F, light, phong, bg),
         None),
    ]
    times = [[] for _ in calls]
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for it in range(WARMUP + ROUNDS):
        for k, (_, fn, nbytes) in enumerate(calls):
            if nbytes is not None:
                flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= WARMUP:
                times[k].append(e0.elapsed_time(e1))
    assert torch.equal(rgb, full.rgb) and torch.equal(nmap, full.normals) and torch.equal(face, full.face) and torch.equal(composed, full.depth)
    res = []
    shape = dict(N=N, F=F, H=H, W=W, faces=int(len(f)), covered_fraction_of_frames=float((full.index >= 0).float().mean()))
    for (name, _, nbytes), ts in zip(calls, times):
        ms = statistics.median(ts)
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts))
        if nbytes is not None:
            rate = nbytes / (ms * 1e-3)
            row.update(needed_mbytes=nbytes / 1e6, gb_per_s=rate / 1e9, share_of_hbm_spec_peak=rate / HBM_SPEC, share_of_hbm_copy_rate=rate / HBM_COPY)
        res.append(row)
        print(json.dumps(row), flush=True)
    ratio = res[1]["gpu_ms_median"] / res[0]["gpu_ms_median"]
    print(json.dumps(dict(render_visibility_over_render_depth=ratio, **shape)), flush=True)
    write_json(res, render_visibility_over_render_depth=ratio, **shape)


if __name__ == "__main__":
    main()
