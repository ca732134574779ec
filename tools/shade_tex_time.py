#!/usr/bin/env python3
"""Time the textured shade pass (gdrn_shade_frames_tex) against the pass it was built from, with HIP events round the shade pass alone.  The workload
is that of tools/shade_time.py -- 64 instances of 20 480-face perturbed icospheres in 8 frames of 480 x 640, with backgrounds -- spread over 8
classes of the same geometry with one 1024 x 1024 texture each.  Four calls on the same keys, timed INTERLEAVED (one of each per round, 5 untimed
rounds, then the median and range of 20):
  gdrn_shade_frames                  the existing pass (vertex colours, Phong weights): the yardstick
  gdrn_shade_frames_tex, untextured  the new pass on a table without textures (vertex colours, the BOP light model)
  gdrn_shade_frames_tex, nearest     the 8 textures, one texel gathered per covered pixel
  gdrn_shade_frames_tex, bilinear    four texels per covered pixel
each behind an untimed 512 MB fill, so that it reads HBM and not what the call before it left in the 256 MB last-level cache.  Per call: the time,
its ratio to gdrn_shade_frames in the same run, the bytes it needs from the shapes (N H W 8 of keys read, F H W 14 of frames with backgrounds) and
-- for the textured calls -- the texel footprint actually touched: the distinct 4-byte texels and the distinct 128-byte lines the covered pixels
read, counted on the host from the result of a probe texture whose texels hold their own index.  Reported, not gated.
Usage:  timeout 600 python tools/shade_tex_time.py [--json FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import write_json  # noqa: E402
from gdrnet_amd import cabi, devargs, scene_gt as SG, shade, synth  # noqa: E402

WARMUP, ROUNDS = 5, 20
TEX = 1024


def sphere_uv(v):
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.stack([0.5 + np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi), 0.5 + np.arcsin(np.clip(d[:, 2], -1.0, 1.0)) / np.pi], axis=1)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, N, H, W, F, C, seed = torch.device("cuda:0"), 64, 480, 640, 8, 8, 7
    u = lambda tag, *shape: synth.hash_uniform(seed, tag, shape)  # noqa: E731
    R = torch.from_numpy(synth._random_rotations(seed, "R", N)).to(dev)
    t = torch.from_numpy(np.concatenate([0.3 * u("t_xy", N, 2) - 0.15, 0.6 + 0.8 * u("t_z", N, 1)], axis=1)).to(dev)
    K = torch.from_numpy(np.repeat(synth.LM_K.astype(np.float64)[None], N, axis=0)).to(dev)
    v, f = synth.mesh_icosphere(5, 0.1, 0.35, seed)
    col, uv = 0.2 + 0.7 * u("col", len(v), 3), sphere_uv(v)
    rng = np.random.default_rng(seed)
    textures = [rng.integers(0, 256, (TEX, TEX, 3), dtype=np.uint8) for _ in range(C)]
    table = shade.TexturedMeshTable([v] * C, [f] * C, [col] * C, None, [uv] * C, textures, device=dev)
    plain = shade.TexturedMeshTable([v] * C, [f] * C, [col] * C, device=dev)
    # a probe table of the same layout whose texel (row, column) of class c is its own index, 24 bits: which texels does a call touch?
    probe_img = np.arange(TEX * TEX, dtype=np.uint32).reshape(TEX, TEX)
    probe_img = np.stack([probe_img & 0xFF, (probe_img >> 8) & 0xFF, probe_img >> 16], axis=2).astype(np.uint8)
    probe = shade.TexturedMeshTable([v] * C, [f] * C, [col] * C, None, [uv] * C, [probe_img] * C, device=dev)
    labels, frame = np.arange(N) % C, np.arange(N) // (N // F)
    bg = torch.from_numpy(np.floor(256.0 * u("bg", F, H, W, 3)).astype(np.uint8)).to(dev)
    light, phong = shade.random_lights(F, np.random.default_rng(seed))
    ambient = np.full(F, 0.5)

    full = shade.render_frames_bop(table, labels, R, t, K, H, W, frame, F, light, ambient, "phong", "nearest", bg)
    lib, p, st = cabi.load(), cabi.ptr, devargs.stream(dev)
    lab_host = labels.astype(np.int32)
    lab = torch.from_numpy(lab_host).to(dev)
    off_host, inst_host = SG.csr_of_frames(frame, F)
    off, inst = torch.from_numpy(off_host).to(dev), torch.from_numpy(inst_host).to(dev)
    li, ph, am = torch.from_numpy(light).to(dev), torch.from_numpy(phong).to(dev), torch.from_numpy(ambient).to(dev)
    vis = full.vis
    rgb, zmap, index = torch.empty_like(full.rgb), torch.empty_like(full.depth), torch.empty_like(full.index)

    def mesh(tb):
        return [p(tb[k]) for k in ("verts", "faces", "vert_off", "nverts", "face_off", "nfaces", "normals", "colors")]

    def tail(weights):
        return (C, p(lab), lab_host.ctypes.data, p(R), p(t), p(K), p(off), off_host.ctypes.data, p(inst), inst_host.ctypes.data, F, N, H, W, p(li), weights)

    maps = (p(bg), p(rgb), p(zmap), p(index), None, None, st)

    def old_call():
        cabi.check(lib.gdrn_shade_frames(p(vis), *mesh(table.on(dev)), *tail(p(ph)), *maps), "shade_frames")

    def tex_call(tbl, filt):
        tb = tbl.on(dev)
        cabi.check(lib.gdrn_shade_frames_tex(p(vis), *mesh(tb), p(tb["uvs"]), p(tb["texels"]), p(tb["tex"]), tbl.tex.ctypes.data, int(tbl.texels.size),
                                             *tail(p(am)), 0, filt, *maps), "shade_frames_tex")

    # the texel footprint: ambient 1, nearest sampling of the probe table -> the pixel's bytes are the index of its texel within the class
    pr = shade.render_frames_bop(probe, labels, R, t, K, H, W, frame, F, light, 1.0, "phong", "nearest")
    covered = (pr.index >= 0)
    cls = torch.from_numpy(labels).to(dev)[pr.index[covered].long()]
    px = pr.rgb[covered].to(torch.int64)
    texel = cls * (TEX * TEX) + px[:, 0] + (px[:, 1] << 8) + (px[:, 2] << 16)
    n_cov = int(covered.sum())
    near_texels, near_lines = int(torch.unique(texel).numel()), int(torch.unique(texel // 32).numel())
    # bilinear: the 2 x 2 block round the sample; bounded here by the nearest texel and its three neighbours towards +x / +y
    quad = torch.cat([texel, texel + 1, texel + TEX, texel + TEX + 1]).clamp_(max=C * TEX * TEX - 1)
    bil_texels, bil_lines = int(torch.unique(quad).numel()), int(torch.unique(quad // 32).numel())

    b_keys, b_frames = N * H * W * 8, F * H * W * 14
    b_uv = 6 * 8   # six fp64 UV loads per covered pixel, from a table that stays in cache (20 480 faces: 164 KB of UVs per class)
    calls = [
        ("gdrn_shade_frames", old_call, dict()),
        ("gdrn_shade_frames_tex, untextured", lambda: tex_call(plain, 0), dict()),
        ("gdrn_shade_frames_tex, nearest", lambda: tex_call(table, 0), dict(texels_touched=near_texels, texel_lines_128B=near_lines,
                                                                            texel_mbytes_by_line=near_lines * 128 / 1e6)),
        ("gdrn_shade_frames_tex, bilinear", lambda: tex_call(table, 1), dict(texels_touched=bil_texels, texel_lines_128B=bil_lines,
                                                                             texel_mbytes_by_line=bil_lines * 128 / 1e6)),
    ]
    times = [[] for _ in calls]
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for it in range(WARMUP + ROUNDS):
        for k, (_, fn, _) in enumerate(calls):
            flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= WARMUP:
                times[k].append(e0.elapsed_time(e1))
    bil = shade.render_frames_bop(table, labels, R, t, K, H, W, frame, F, light, ambient, "phong", "bilinear", bg)
    assert torch.equal(rgb, bil.rgb) and torch.equal(index, full.index)   # (the last call of a round is the bilinear one)
    shape = dict(N=N, F=F, H=H, W=W, classes=C, faces=int(len(f)), texture=f"{TEX} x {TEX}", covered_pixels=n_cov,
                 covered_fraction_of_frames=n_cov / (F * H * W), uv_mbytes_requested=n_cov * b_uv / 1e6)
    base = statistics.median(times[0])
    res = []
    for (name, _, extra), ts in zip(calls, times):
        ms = statistics.median(ts)
        nbytes = b_keys + b_frames + int(extra.get("texel_lines_128B", 0)) * 128
        row = dict(call=name, gpu_ms_median=ms, gpu_ms_min=min(ts), gpu_ms_max=max(ts), ratio_to_gdrn_shade_frames=ms / base,
                   needed_mbytes=nbytes / 1e6, gb_per_s=nbytes / (ms * 1e-3) / 1e9, **extra)
        res.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(shape), flush=True)
    write_json(res, **shape)


if __name__ == "__main__":
    main()
