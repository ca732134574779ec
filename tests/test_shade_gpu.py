"""GPU tests of the shaded renderer (gdrn_render_visibility in csrc/render.hip, csrc/shade.hip, through gdrnet_amd.shade) against the host oracle
tests/shade_host.py on the scenes of synth.make_shade_inputs.

Bounds.  Depth halves and the composition are exact (the same fragment arithmetic; a minimum and a first arg-min).  Face ids: the reported face
must cover the pixel in the oracle with an fp32 depth within one fp32 ulp of the device's (both sides fp64 before the one rounding), and equal
the oracle's wherever its two nearest fragments are more than 4 ulp apart; on "watertight", whose arithmetic is exact, everywhere.  Bytes:
|q - 255 v| <= 0.5 + 1e-6 with v the oracle's fp64 value for the face the device reports -- derived, not measured: about a hundred fp64 operations
on well-conditioned inputs keep the error below 1e-12, while an fp32 evaluation (~1.5e-5 * 255) does not fit."""
import numpy as np
import pytest
import torch

import shade_host as SH
from gdrnet_amd import cabi, render, shade, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -23
CASES = synth.SHADE_CASES
_cache = {}


def _scene(case):
    """(inputs, oracle, table, the device result with every optional map and the background), computed once per session and left unchanged"""
    if case not in _cache:
        inp = synth.make_shade_inputs(case)
        table = shade.ShadedMeshTable(inp["vertices"], inp["faces"], inp["colors"], device=DEV)
        _cache[case] = (inp, SH.Scene(inp), table, _frames(inp, table, want_face=True, want_normals=True))
    return _cache[case]


def _poses(inp, rows=slice(None)):
    return [torch.from_numpy(inp[k][rows]).to(DEV) for k in ("R", "t", "K")]


def _frames(inp, table, background=True, rows=slice(None), frame=None, num_frames=None, **kw):
    bg = torch.from_numpy(inp["background"]).to(DEV) if background is True else background
    fr = inp["frame"][rows] if frame is None else frame
    F = inp["num_frames"] if num_frames is None else num_frames
    light, phong = kw.pop("light", inp["light"]), kw.pop("phong", inp["phong"])
    out = shade.render_frames(table, inp["labels"][rows], *_poses(inp, rows), inp["H"], inp["W"], fr, F, light, phong, bg, near=inp["near"],
                              far=inp["far"], **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES)
def test_visibility_upper_halves_are_render_depth_bit_for_bit(case):
    inp, _, table, got = _scene(case)
    depth = render.render_depth(table, inp["labels"], *_poses(inp), inp["H"], inp["W"], inp["near"], inp["far"])
    vis = shade.render_visibility(table, inp["labels"], *_poses(inp), inp["H"], inp["W"], inp["near"], inp["far"])
    assert vis.dtype == torch.int64 and vis.shape == depth.shape and torch.equal(vis, got.vis)
    assert torch.equal(shade.visibility_depth(vis).view(torch.int32), depth.view(torch.int32))
    upper = (vis >> 32).to(torch.int32)
    assert torch.equal(upper == -1, depth == 0) and torch.equal((vis == -1), depth == 0)   # ~0 exactly where nothing is drawn
    face = shade.visibility_face(vis)
    nf = torch.from_numpy(table.nfaces[inp["labels"]]).to(DEV)[:, None, None]
    assert bool(((face >= 0) & (face < nf))[depth != 0].all()) and bool((face[depth == 0] == -1).all())


@pytest.mark.parametrize("case", CASES)
def test_depth_and_index_are_the_minimum_and_first_argmin_of_render_depth(case):
    inp, _, table, got = _scene(case)
    F, H, W = inp["num_frames"], inp["H"], inp["W"]
    depth = render.render_depth(table, inp["labels"], *_poses(inp), H, W, inp["near"], inp["far"])
    inf = torch.where(depth == 0, torch.full_like(depth, float("inf")), depth)
    for f in range(F):
        rows = np.flatnonzero(inp["frame"] == f)
        if len(rows) == 0:
            assert not got.depth[f].any() and bool((got.index[f] == -1).all()) and bool((got.face[f] == -1).all())
            continue
        sub = inf[torch.from_numpy(rows).to(DEV)]
        best = sub.min(dim=0).values
        first = (sub == best[None]).to(torch.int32).argmax(dim=0)   # the first row that reaches the minimum
        drawn = torch.isfinite(best)
        want_index = torch.where(drawn, torch.from_numpy(rows).to(DEV)[first].to(torch.int32), torch.full_like(first, -1, dtype=torch.int32))
        assert torch.equal(got.depth[f].view(torch.int32), torch.where(drawn, best, torch.zeros_like(best)).view(torch.int32))
        assert torch.equal(got.index[f], want_index)
    assert got.depth.dtype == torch.float32 and got.index.dtype == torch.int32 and got.depth.shape == (F, H, W)


@pytest.mark.parametrize("case", CASES)
def test_face_ids_against_the_oracle_on_every_covered_pixel(case):
    inp, ora, table, got = _scene(case)
    HW = inp["H"] * inp["W"]
    index, face, depth = (x.cpu().numpy().reshape(inp["num_frames"], HW) for x in (got.index, got.face, got.depth))
    assert np.array_equal(index, ora.index) and np.array_equal(depth != 0, ora.depth != 0)   # coverage and owner: every pixel
    checked = decided = 0
    for f in range(inp["num_frames"]):
        for i in np.unique(index[f][index[f] >= 0]):
            pixel = np.flatnonzero(index[f] == i)
            d_ora, f_ora, second, frags = ora.inst[i]
            zf = SH.fragment_depth(frags, len(inp["faces"][inp["labels"][i]]), pixel, face[f][pixel])
            assert not np.isnan(zf).any(), (case, f, i)                                                 # the reported face covers the pixel
            assert np.all(np.abs(zf.astype(np.float64) - depth[f][pixel]) <= ULP * depth[f][pixel])     # and lies at the device's depth
            if case == "watertight":
                clear = np.ones(len(pixel), dtype=bool)    # exact arithmetic: the lowest-index rule decides every tie
            else:
                clear = second[pixel].astype(np.float64) - d_ora[pixel] > 4 * ULP * d_ora[pixel]
            assert np.array_equal(face[f][pixel][clear], f_ora[pixel][clear]), (case, f, i)
            checked += len(pixel)
            decided += int(clear.sum())
    print(f"{case}: {checked} covered pixels, {decided} with a decided face")
    assert checked == int((ora.index >= 0).sum()) and decided > 0.9 * checked
    if case == "watertight":
        _, f_ora, second, _ = ora.inst[0]
        assert (second == ora.depth[0]).sum() > 3000   # the ties are there: most pixels lie on an edge shared by two faces at one depth


@pytest.mark.parametrize("case", CASES)
def test_colours_and_normal_maps_on_every_covered_pixel(case):
    inp, ora, table, got = _scene(case)
    F, HW = inp["num_frames"], inp["H"] * inp["W"]
    index, face = (x.cpu().numpy().reshape(F, HW) for x in (got.index, got.face))
    rgb, nrm = (x.cpu().numpy().reshape(F, HW, 3).astype(np.float64) for x in (got.rgb, got.normals))
    assert got.rgb.dtype == torch.uint8 and got.normals.dtype == torch.uint8
    worst = 0.0
    for f in range(F):
        pixel = np.flatnonzero(index[f] >= 0)
        if len(pixel) == 0:
            continue
        v_rgb, v_nrm = ora.values(f, pixel, index[f][pixel], face[f][pixel])
        for q, v in ((rgb[f][pixel], v_rgb), (nrm[f][pixel], v_nrm)):
            err = np.abs(q - 255.0 * v)
            worst = max(worst, float(err.max()))
            assert np.all(err <= 0.5 + 1e-6), (case, f, float(err.max()))
        assert not nrm[f][index[f] < 0].any()
    print(f"{case}: worst |q - 255 v| = {worst:.9f}")
    if case == "sphere":   # the three lightings do what they are there for
        m = index[0] >= 0
        assert rgb[1][m].mean() < 0.6 * rgb[0][m].mean() and (rgb[2][m] == 255).mean() > 0.5 and (rgb[0][m] == 255).mean() < 0.1


def test_ambient_only_of_a_uniform_u8_mesh_is_that_colour_exactly():
    inp = synth.make_shade_inputs("scene")
    colour = np.array([13, 200, 97], dtype=np.uint8)
    table = shade.ShadedMeshTable(inp["vertices"], inp["faces"], [np.tile(colour, (len(v), 1)) for v in inp["vertices"]], device=DEV)
    got = _frames(inp, table, background=None, phong=(1.0, 0.0, 0.0))
    drawn = got.index >= 0
    assert int(drawn.sum()) > 500
    assert bool((got.rgb[drawn] == torch.from_numpy(colour).to(DEV)).all()) and not got.rgb[~drawn].any()


def test_background_passes_through_and_the_empty_frame_is_its_background():
    for case in ("scene", "cube"):
        inp, _, table, got = _scene(case)
        bg = torch.from_numpy(inp["background"]).to(DEV)
        empty = got.index < 0
        assert torch.equal(got.rgb[empty], bg[empty])
        black = _frames(inp, table, background=None)
        assert not black.rgb[empty].any() and torch.equal(black.rgb[~empty], got.rgb[~empty])
        assert torch.equal(black.depth, got.depth) and torch.equal(black.index, got.index) and black.face is None and black.normals is None
    inp, _, table, got = _scene("scene")
    assert not (inp["frame"] == 2).any() and torch.equal(got.rgb[2], torch.from_numpy(inp["background"][2]).to(DEV))
    # a background view at an odd byte offset is taken as well
    flat = torch.zeros(inp["background"].size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(inp["background"]).to(DEV).reshape(-1)
    assert torch.equal(_frames(inp, table, background=flat[1:].view(inp["background"].shape)).rgb, got.rgb)


def test_repeated_call_is_bit_identical_and_the_batch_equals_single_frames():
    for case in ("scene", "sphere"):
        inp, _, table, got = _scene(case)
        again = _frames(inp, table, want_face=True, want_normals=True)
        for k in ("rgb", "depth", "index", "face", "normals", "vis"):
            assert torch.equal(getattr(got, k), getattr(again, k)), (case, k)
        bg = torch.from_numpy(inp["background"]).to(DEV)
        for f in range(inp["num_frames"]):
            rows = np.flatnonzero(inp["frame"] == f)
            one = _frames(inp, table, background=bg[f : f + 1], rows=rows, frame=np.zeros(len(rows), np.int64), num_frames=1, light=inp["light"][f],
                          phong=inp["phong"][f], want_face=True, want_normals=True)
            assert torch.equal(one.rgb[0], got.rgb[f]) and torch.equal(one.depth[0], got.depth[f]) and torch.equal(one.face[0], got.face[f])
            assert torch.equal(one.normals[0], got.normals[f])
            rows_dev = torch.from_numpy(np.append(rows, -1)).to(DEV).to(torch.int32)   # the batch row of a single-frame index, -1 kept
            assert torch.equal(rows_dev[one.index[0].long()], got.index[f])


def test_arguments():
    inp, _, table, got = _scene("cube")
    tb = table.on(DEV)
    R, t, K = _poses(inp)
    N, H, W, F = 4, 48, 64, 4
    lab_host = np.zeros(N, dtype=np.int32)
    lab = torch.from_numpy(lab_host).to(DEV)
    lib, p = cabi.load(), cabi.ptr
    vis = torch.full((N, H, W), 7, dtype=torch.int64, device=DEV)

    def call(N=N, H=H, W=W, near=0.01, far=6.5, verts=p(tb["verts"]), out=p(vis), labels_host=lab_host.ctypes.data, Rp=p(R)):
        return lib.gdrn_render_visibility(verts, p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]), 1, 12, p(lab),
                                          labels_host, Rp, p(t), p(K), N, H, W, near, far, out, None)

    bad_lab = np.array([0, 0, 1, 0], dtype=np.int32)
    for kw in (dict(N=0), dict(H=0), dict(W=-3), dict(near=6.5), dict(near=0.0), dict(verts=None), dict(out=None), dict(labels_host=None),
               dict(Rp=None), dict(labels_host=bad_lab.ctypes.data)):
        assert call(**kw) == -1, kw
    off_host, inst_host = np.arange(F + 1, dtype=np.int32), np.arange(N, dtype=np.int32)
    off, inst = torch.from_numpy(off_host).to(DEV), torch.from_numpy(inst_host).to(DEV)
    light, phong = torch.from_numpy(inp["light"]).to(DEV), torch.from_numpy(inp["phong"]).to(DEV)
    rgb = torch.full((F, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    depth = torch.full((F, H, W), 7.0, dtype=torch.float32, device=DEV)
    index = torch.full((F, H, W), 7, dtype=torch.int32, device=DEV)

    def call2(F=F, N=N, H=H, W=W, v=p(got.vis), normals=p(tb["normals"]), colors=p(tb["colors"]), labels_host=lab_host.ctypes.data,
              off_h=off_host.ctypes.data, inst_h=inst_host.ctypes.data, li=p(light), ph=p(phong), o=p(rgb), d=p(depth), ix=p(index), bg=None):
        return lib.gdrn_shade_frames(v, p(tb["verts"]), p(tb["faces"]), p(tb["vert_off"]), p(tb["nverts"]), p(tb["face_off"]), p(tb["nfaces"]), normals,
                                     colors, 1, p(lab), labels_host, p(R), p(t), p(K), p(off), off_h, p(inst), inst_h, F, N, H, W, li, ph, bg, o, d, ix,
                                     None, None, None)

    bad_off, bad_off2, bad_inst = np.array([0, 1, 2, 3, 3], np.int32), np.array([0, 2, 1, 3, 4], np.int32), np.array([0, 1, 2, 4], np.int32)
    for kw in (dict(F=0), dict(N=-1), dict(H=0), dict(W=-1), dict(v=None), dict(normals=None), dict(colors=None), dict(labels_host=None),
               dict(labels_host=bad_lab.ctypes.data), dict(off_h=None), dict(off_h=bad_off.ctypes.data), dict(off_h=bad_off2.ctypes.data),
               dict(inst_h=None), dict(inst_h=bad_inst.ctypes.data), dict(li=None), dict(ph=None), dict(o=None), dict(d=None), dict(ix=None),
               dict(o=p(rgb) + 1), dict(bg=p(rgb) + 2)):
        assert call2(**kw) == -1, kw
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((vis == 7).all()) and bool((rgb == 7).all()) and bool((depth == 7.0).all()) and bool((index == 7).all())
    assert call() == 0 and call2() == 0
    torch.cuda.synchronize()
    assert torch.equal(vis, got.vis) and torch.equal(index, got.index)

    # the Python layer: host tensors are refused, index vectors and tables are checked on the host
    args = (inp["labels"], R, t, K, H, W, inp["frame"])
    with pytest.raises(cabi.GdrnHipError):
        shade.render_frames(table, inp["labels"], R.cpu(), t, K, H, W, inp["frame"])
    with pytest.raises(cabi.GdrnHipError):
        shade.render_frames(table, inp["labels"], R, t, K.cpu(), H, W, inp["frame"])
    with pytest.raises(cabi.GdrnHipError):
        shade.render_frames(table, *args[:-1], inp["frame"], background=torch.zeros(F, H, W, 3, dtype=torch.uint8))
    with pytest.raises(cabi.GdrnHipError):
        shade.render_visibility(table, inp["labels"], R, t.cpu(), K, H, W)
    for bad in (dict(labels=[0, 0, 1, 0]), dict(frame=[0, 1, 2, -1]), dict(frame=[0, 1, 2]), dict(frame=[0, 1, 2, 4], num_frames=4),
                dict(phong=(0.4, -0.1, 0.3)), dict(phong=(0.4, float("nan"), 0.3)), dict(phong=np.ones((3, 3))), dict(light=(0.0, float("inf"), 0.0)),
                dict(light=np.zeros((5, 3))), dict(background=torch.zeros(F, H, W, 4, dtype=torch.uint8, device=DEV)),
                dict(background=torch.zeros(F, H, W, 3, dtype=torch.float32, device=DEV))):
        kw = dict(labels=inp["labels"], frame=inp["frame"])
        kw.update(bad)
        labels, frame = kw.pop("labels"), kw.pop("frame")
        with pytest.raises(ValueError):
            shade.render_frames(table, labels, R, t, K, H, W, frame, **kw)
    with pytest.raises(ValueError):
        shade.render_frames(render.MeshTable(inp["vertices"], inp["faces"]), *args)
    v, f = inp["vertices"][0], inp["faces"][0]
    for cols, nrms in ((np.full((8, 3), 1.5), None), (np.full((8, 3), np.nan), None), (np.zeros((7, 3)), None), (np.zeros((8, 3)), np.zeros((8, 3))),
                       (np.zeros((8, 3)), np.full((8, 3), np.inf))):
        with pytest.raises(ValueError):
            shade.ShadedMeshTable([v], [f], [cols], None if nrms is None else [nrms])

    # N == 0: every frame is its background; F == 0: empty maps
    e = torch.zeros(0, dtype=torch.float64, device=DEV)
    bg = torch.from_numpy(inp["background"]).to(DEV)
    none = shade.render_frames(table, [], e.reshape(0, 3, 3), e.reshape(0, 3), e.reshape(0, 3, 3), H, W, [], num_frames=F, background=bg, want_face=True)
    torch.cuda.synchronize()
    assert torch.equal(none.rgb, bg) and not none.depth.any() and bool((none.index == -1).all()) and bool((none.face == -1).all())
    assert none.vis.shape == (0, H, W)
    zero = shade.render_frames(table, [], e.reshape(0, 3, 3), e.reshape(0, 3), e.reshape(0, 3, 3), H, W, [])
    assert zero.rgb.shape == (0, H, W, 3) and zero.depth.shape == (0, H, W) and zero.index.shape == (0, H, W)
