"""GPU tests of the textured / flat-shaded renderer (gdrn_shade_frames_tex in csrc/shade.hip, through gdrnet_amd.shade.render_frames_bop) against
the host oracle tests/tex_host.py on the scenes of synth.make_tex_inputs.

Bounds.  depth, index, face and the keys are those of render_frames, bit for bit (the same device functions).  Bytes: |q - 255 v| <= 0.5 + 1e-6
with v the oracle's fp64 value for the face the device reports -- the derived bound of tests/test_shade_gpu.py: about a hundred fp64 operations
on well-conditioned inputs keep the error below 1e-12, and both roundings (half up for the normal map, half to even for the colours) put the byte
within 0.5 of the value.  Nearest sampling is a step function of (u, v): the pixels whose u w or v h lies within 1e-9 of an integer in the oracle
may take the neighbouring texel and are left out; tests/test_shade_tex_cpu.py bounds their number (<= 1 %, none on "sphere" and "quad"), and the
size of the set is asserted here as well.  Bilinear sampling is continuous: nothing is left out."""
import itertools

import numpy as np
import pytest
import torch

import tex_host as TH
from gdrnet_amd import cabi, render, shade, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = synth.TEX_CASES
MODES = tuple(itertools.product(("phong", "flat"), ("nearest", "bilinear")))
_cache = {}


def _poses(inp, rows=slice(None)):
    return [torch.from_numpy(inp[k][rows]).to(DEV) for k in ("R", "t", "K")]


def _bop(inp, table, shading="phong", filt="nearest", background=True, rows=slice(None), frame=None, num_frames=None, **kw):
    bg = torch.from_numpy(inp["background"]).to(DEV) if background is True else background
    fr = inp["frame"][rows] if frame is None else frame
    F = inp["num_frames"] if num_frames is None else num_frames
    light, ambient = kw.pop("light", inp["light"]), kw.pop("ambient", inp["ambient"])
    out = shade.render_frames_bop(table, inp["labels"][rows], *_poses(inp, rows), inp["H"], inp["W"], fr, F, light, ambient, shading, filt, bg,
                                  near=inp["near"], far=inp["far"], **kw)
    torch.cuda.synchronize()
    return out


def _scene(case):
    """(inputs, oracle, table, {(shading, filter): the device result with every optional map and the background}), computed once per session and
    left unchanged"""
    if case not in _cache:
        inp = synth.make_tex_inputs(case)
        table = shade.TexturedMeshTable(inp["vertices"], inp["faces"], inp["colors"], None, inp["uvs"], inp["textures"], device=DEV)
        got = {m: _bop(inp, table, *m, want_face=True, want_normals=True) for m in MODES}
        _cache[case] = (inp, TH.TexScene(inp), table, got)
    return _cache[case]


@pytest.mark.parametrize("case", CASES)
def test_depth_index_face_and_keys_are_those_of_render_frames_bit_for_bit(case):
    inp, ora, table, got = _scene(case)
    ref = shade.render_frames(table, inp["labels"], *_poses(inp), inp["H"], inp["W"], inp["frame"], inp["num_frames"], want_face=True,
                              near=inp["near"], far=inp["far"])
    torch.cuda.synchronize()
    for m in MODES:
        g = got[m]
        assert g.depth.dtype == torch.float32 and g.index.dtype == torch.int32 and g.rgb.dtype == torch.uint8 and g.normals.dtype == torch.uint8
        assert torch.equal(g.depth.view(torch.int32), ref.depth.view(torch.int32)) and torch.equal(g.index, ref.index), (case, m)
        assert torch.equal(g.face, ref.face) and torch.equal(g.vis, ref.vis), (case, m)
    F, HW = inp["num_frames"], inp["H"] * inp["W"]
    assert np.array_equal(ref.index.cpu().numpy().reshape(F, HW), ora.index)     # and the oracle's owner on every pixel


@pytest.mark.parametrize("shading,filt", MODES)
@pytest.mark.parametrize("case", CASES)
def test_colours_and_normal_maps_on_every_covered_pixel(case, shading, filt):
    inp, ora, table, got = _scene(case)
    g = got[(shading, filt)]
    F, HW = inp["num_frames"], inp["H"] * inp["W"]
    index, face = (x.cpu().numpy().reshape(F, HW) for x in (g.index, g.face))
    rgb, nrm = (x.cpu().numpy().reshape(F, HW, 3).astype(np.float64) for x in (g.rgb, g.normals))
    worst, covered, left_out = 0.0, 0, 0
    for f in range(F):
        pixel = np.flatnonzero(index[f] >= 0)
        if len(pixel) == 0:
            continue
        v_rgb, v_nrm, dist = ora.values(f, pixel, index[f][pixel], face[f][pixel], shading, filt)
        keep = dist >= TH.NEAR_INT if filt == "nearest" else np.ones(len(pixel), dtype=bool)
        covered += len(pixel)
        left_out += int((~keep).sum())
        for q, v in ((rgb[f][pixel][keep], v_rgb[keep]), (nrm[f][pixel], v_nrm)):
            err = np.abs(q - 255.0 * v)
            worst = max(worst, float(err.max()))
            assert np.all(err <= 0.5 + 1e-6), (case, shading, filt, f, float(err.max()))
        assert not nrm[f][index[f] < 0].any()
    print(f"{case} {shading} {filt}: {covered} covered pixels, {left_out} left out, worst |q - 255 v| = {worst:.9f}")
    assert covered == int((ora.index >= 0).sum()) and left_out <= 0.01 * covered
    if case in ("sphere", "quad"):
        assert left_out == 0
    if case == "sphere":   # the three frames do what they are there for: a light behind the object leaves the ambient term, ambient 0.9 is brighter
        m = index[0] >= 0
        assert rgb[1][m].mean() < 0.8 * rgb[0][m].mean() and rgb[2][m].mean() > rgb[0][m].mean()


def test_quad_is_the_texture_byte_for_byte_in_both_filters():
    inp, _, _, got = _scene("quad")
    x0, y0 = synth.TEX_QUAD_ORIGIN
    tex = torch.from_numpy(inp["textures"][0]).to(DEV)
    bg = torch.from_numpy(inp["background"]).to(DEV)
    for m in MODES:
        rgb = got[m].rgb[0]
        assert torch.equal(rgb[y0 : y0 + 8, x0 : x0 + 8], tex), m
        want = bg[0].clone()
        want[y0 : y0 + 8, x0 : x0 + 8] = tex
        assert torch.equal(rgb, want), m
        assert int((got[m].index[0] >= 0).sum()) == 64


@pytest.mark.parametrize("case", ("scene", "sphere"))
def test_untextured_table_against_gdrn_shade_frames_with_phong_a_1_0(case):
    """a plain ShadedMeshTable through the new entry point: below the clip at 1 the light model is gdrn_shade_frames' with phong = (a, 1, 0)"""
    a = 0.1
    inp = synth.make_shade_inputs(case)
    table = shade.ShadedMeshTable(inp["vertices"], inp["faces"], inp["colors"], device=DEV)
    F, H, W = inp["num_frames"], inp["H"], inp["W"]
    bg = torch.from_numpy(inp["background"]).to(DEV)
    args = (table, inp["labels"], *_poses(inp), H, W, inp["frame"], F, inp["light"])
    old = shade.render_frames(*args, (a, 1.0, 0.0), bg, want_face=True, want_normals=True, near=inp["near"], far=inp["far"])
    new = shade.render_frames_bop(*args, a, "phong", "bilinear", bg, want_face=True, want_normals=True, near=inp["near"], far=inp["far"])
    torch.cuda.synchronize()
    assert torch.equal(new.normals, old.normals) and torch.equal(new.depth, old.depth) and torch.equal(new.index, old.index)
    assert torch.equal(new.face, old.face)
    ora = TH.TexScene(dict(inp, uvs=[None] * len(inp["vertices"]), textures=[None] * len(inp["vertices"]), ambient=np.full(F, a)))
    index, face = (x.cpu().numpy().reshape(F, H * W) for x in (new.index, new.face))
    q_new, q_old = (x.cpu().numpy().reshape(F, H * W, 3) for x in (new.rgb, old.rgb))
    compared = 0
    for f in range(F):
        pixel = np.flatnonzero(index[f] >= 0)
        if len(pixel) == 0:
            assert np.array_equal(q_new[f], q_old[f])
            continue
        v, _, _ = ora.values(f, pixel, index[f][pixel], face[f][pixel])
        lw = np.zeros(len(pixel))
        for i in np.unique(index[f][pixel]):
            m, c = index[f][pixel] == i, inp["labels"][i]
            lw[m] = TH.tex_values(inp["vertices"][c], inp["faces"][c], inp["colors"][c], ora.normals[c], None, None, inp["R"][i], inp["t"][i],
                                  inp["K"][i], H, W, inp["light"][f], a, pixel[m], face[f][pixel][m])["lw"]
        sel = (lw <= 1.0 - 1e-9)[:, None] & (np.abs((255.0 * v) % 1.0 - 0.5) > 1e-9)
        assert np.array_equal(q_new[f][pixel][sel], q_old[f][pixel][sel]), (case, f)
        assert np.array_equal(q_new[f][index[f] < 0], q_old[f][index[f] < 0])
        compared += int(sel.sum())
    print(f"{case}: {compared} bytes compared with gdrn_shade_frames")
    assert compared > 1000


def test_background_passes_through_and_the_empty_frame_is_its_background():
    for case in ("scene", "cube"):
        inp, _, table, got = _scene(case)
        g = got[("phong", "nearest")]
        bg = torch.from_numpy(inp["background"]).to(DEV)
        empty = g.index < 0
        assert torch.equal(g.rgb[empty], bg[empty])
        black = _bop(inp, table, background=None)
        assert not black.rgb[empty].any() and torch.equal(black.rgb[~empty], g.rgb[~empty])
        assert torch.equal(black.depth, g.depth) and torch.equal(black.index, g.index) and black.face is None and black.normals is None
    inp, _, table, got = _scene("scene")
    g = got[("flat", "bilinear")]
    assert not (inp["frame"] == 2).any() and torch.equal(g.rgb[2], torch.from_numpy(inp["background"][2]).to(DEV))
    assert not g.depth[2].any() and bool((g.index[2] == -1).all()) and bool((g.face[2] == -1).all()) and not g.normals[2].any()
    # a background view at an odd byte offset is taken as render_frames takes it
    flat = torch.zeros(inp["background"].size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(inp["background"]).to(DEV).reshape(-1)
    assert torch.equal(_bop(inp, table, "flat", "bilinear", background=flat[1:].view(inp["background"].shape)).rgb, g.rgb)
    # N == 0: every frame is its background; F == 0: empty maps
    F, H, W = inp["num_frames"], inp["H"], inp["W"]
    e = torch.zeros(0, dtype=torch.float64, device=DEV)
    bg = torch.from_numpy(inp["background"]).to(DEV)
    none = shade.render_frames_bop(table, [], e.reshape(0, 3, 3), e.reshape(0, 3), e.reshape(0, 3, 3), H, W, [], num_frames=F, background=bg,
                                   want_face=True)
    torch.cuda.synchronize()
    assert torch.equal(none.rgb, bg) and not none.depth.any() and bool((none.index == -1).all()) and bool((none.face == -1).all())
    assert none.vis.shape == (0, H, W)
    zero = shade.render_frames_bop(table, [], e.reshape(0, 3, 3), e.reshape(0, 3), e.reshape(0, 3, 3), H, W, [])
    assert zero.rgb.shape == (0, H, W, 3) and zero.depth.shape == (0, H, W) and zero.index.shape == (0, H, W)


def test_repeated_call_is_bit_identical_and_the_batch_equals_single_frames():
    for case, mode in (("scene", ("phong", "bilinear")), ("sphere", ("flat", "nearest"))):
        inp, _, table, got = _scene(case)
        g = got[mode]
        again = _bop(inp, table, *mode, want_face=True, want_normals=True)
        for k in ("rgb", "depth", "index", "face", "normals", "vis"):
            assert torch.equal(getattr(g, k), getattr(again, k)), (case, k)
        bg = torch.from_numpy(inp["background"]).to(DEV)
        for f in range(inp["num_frames"]):
            rows = np.flatnonzero(inp["frame"] == f)
            one = _bop(inp, table, *mode, background=bg[f : f + 1], rows=rows, frame=np.zeros(len(rows), np.int64), num_frames=1, light=inp["light"][f],
                       ambient=float(inp["ambient"][f]), want_face=True, want_normals=True)
            assert torch.equal(one.rgb[0], g.rgb[f]) and torch.equal(one.depth[0], g.depth[f]) and torch.equal(one.face[0], g.face[f])
            assert torch.equal(one.normals[0], g.normals[f])
            rows_dev = torch.from_numpy(np.append(rows, -1)).to(DEV).to(torch.int32)   # the batch row of a single-frame index, -1 kept
            assert torch.equal(rows_dev[one.index[0].long()], g.index[f])


def test_arguments():
    inp, _, table, got = _scene("cube")
    g = got[("phong", "nearest")]
    tb = table.on(DEV)
    R, t, K = _poses(inp)
    N, H, W, F = 4, 48, 64, 4
    lab_host = np.zeros(N, dtype=np.int32)
    lab = torch.from_numpy(lab_host).to(DEV)
    lib, p = cabi.load(), cabi.ptr
    off_host, inst_host = np.arange(F + 1, dtype=np.int32), np.arange(N, dtype=np.int32)
    off, inst = torch.from_numpy(off_host).to(DEV), torch.from_numpy(inst_host).to(DEV)
    light, ambient = torch.from_numpy(inp["light"]).to(DEV), torch.from_numpy(inp["ambient"]).to(DEV)
    rgb = torch.full((F, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    depth = torch.full((F, H, W), 7.0, dtype=torch.float32, device=DEV)
    index = torch.full((F, H, W), 7, dtype=torch.int32, device=DEV)
    tex_host = table.tex

    def call(F=F, N=N, H=H, W=W, v=p(g.vis), uvs=p(tb["uvs"]), texels=p(tb["texels"]), tex=p(tb["tex"]), tex_h=tex_host, n_texels=35,
             labels_host=lab_host.ctypes.data, off_h=off_host.ctypes.data, inst_h=inst_host.ctypes.data, li=p(light), am=p(ambient), shading=0, filt=0,
             o=p(rgb), d=p(depth), ix=p(index), bg=None):
        return lib.gdrn_shade_frames_tex(v, p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]),
                                         p(tb["normals"]), p(tb["colors"]), uvs, texels, tex, None if tex_h is None else tex_h.ctypes.data, n_texels, 1,
                                         p(lab), labels_host, p(R), p(t), p(K), p(off), off_h, p(inst), inst_h, F, N, H, W, li, am, shading, filt, bg, o,
                                         d, ix, None, None, None)

    assert tex_host.tolist() == [[0, 5, 7]]
    bad_lab, bad_off, bad_inst = np.array([0, 0, 1, 0], np.int32), np.array([0, 1, 2, 3, 3], np.int32), np.array([0, 1, 2, 4], np.int32)
    bad_tex = [np.array([r], np.int32) for r in ([-1, 5, 7], [1, 5, 7], [0, 0, 7], [0, 5, 0], [0, 16385, 1], [0, 6, 7], [0, -1, -1])]
    for kw in [dict(F=0), dict(N=-1), dict(H=0), dict(W=-1), dict(v=None), dict(uvs=None), dict(texels=None), dict(tex=None), dict(tex_h=None),
               dict(n_texels=-1), dict(n_texels=34), dict(labels_host=None), dict(labels_host=bad_lab.ctypes.data), dict(off_h=None),
               dict(off_h=bad_off.ctypes.data), dict(inst_h=None), dict(inst_h=bad_inst.ctypes.data), dict(li=None), dict(am=None), dict(shading=2),
               dict(shading=-1), dict(filt=2), dict(filt=-1), dict(o=None), dict(d=None), dict(ix=None), dict(o=p(rgb) + 1), dict(bg=p(rgb) + 2)] + \
              [dict(tex_h=b) for b in bad_tex]:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((rgb == 7).all()) and bool((depth == 7.0).all()) and bool((index == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    black = _bop(inp, table, background=None)
    assert torch.equal(index, g.index) and torch.equal(depth, g.depth) and torch.equal(rgb, black.rgb)

    # the Python layer
    args = (inp["labels"], R, t, K, H, W, inp["frame"])
    with pytest.raises(cabi.GdrnHipError):
        shade.render_frames_bop(table, inp["labels"], R.cpu(), t, K, H, W, inp["frame"])
    for bad in (dict(ambient=-0.1), dict(ambient=float("nan")), dict(ambient=np.ones(3)), dict(ambient=np.ones((F, 1))), dict(ambient="x"),
                dict(shading="gouraud"), dict(filter="trilinear"), dict(light=(0.0, float("inf"), 0.0)), dict(light=np.zeros((5, 3))),
                dict(num_frames=3), dict(background=torch.zeros(F, H, W, 4, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            shade.render_frames_bop(table, *args, **bad)
    with pytest.raises(ValueError):
        shade.render_frames_bop(render.MeshTable(inp["vertices"], inp["faces"]), *args)
    with pytest.raises(ValueError):
        shade.render_frames_bop(table, [0, 0, 1, 0], *args[1:])
    # ambient as a number, as [F] and as a tensor give the same frames
    one = shade.render_frames_bop(table, *args, ambient=0.5)
    two = shade.render_frames_bop(table, *args, ambient=torch.full((F,), 0.5, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(one.rgb, two.rgb) and torch.equal(one.rgb, black.rgb)
