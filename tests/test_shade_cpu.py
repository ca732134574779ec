"""CPU tests of the shaded renderer's host side: the oracle tests/shade_host.py against closed forms, the fixtures' acceptance conditions,
gdrnet_amd.shade's host functions (vertex_normals, ShadedMeshTable, random_lights) and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

import render_host as RH
import shade_host as SH
from gdrnet_amd import cabi, render, shade, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_scenes = {}


def _scene(case):
    if case not in _scenes:
        st = {}
        inp = synth.make_shade_inputs(case)
        _scenes[case] = (inp, SH.Scene(inp, st), st)
    return _scenes[case]


def test_oracle_on_a_fronto_parallel_plane_with_the_light_at_the_camera():
    """z = 1, normal towards the camera, light at the origin: L = V = N-ward ray, so N.L = cos(theta) = 1 / |d| and Rv.V = 2 cos^2 - 1 = cos(2 theta)"""
    H, W = 33, 41
    K = np.array([[30.0, 0.0, 20.0], [0.0, 30.0, 16.0], [0.0, 0.0, 1.0]])
    v, f = synth.mesh_rectangle(2, 2)
    v = v * np.array([4.0, 4.0, 1.0])
    col = np.tile([0.5, 0.25, 1.0], (len(v), 1))
    nrm = np.tile([0.0, 0.0, -1.0], (len(v), 1))
    R, t = np.eye(3), np.array([0.0, 0.0, 1.0])
    depth, face, _, _ = SH.visibility_one(v, f, R, t, K, H, W)
    assert (depth == 1.0).all()
    pixel = np.arange(H * W)
    amb, dif, spe = 0.1, 0.5, 0.6
    rgb, nmap = SH.shade_values(v, f, col, nrm, R, t, K, H, W, np.zeros(3), (amb, dif, spe), pixel, face)
    dx, dy = RH.pixel_rays(K, H, W)
    cos = 1.0 / np.sqrt(dx * dx + dy * dy + 1.0)
    want = (amb + dif * cos + spe * np.maximum(2.0 * cos * cos - 1.0, 0.0))[:, None] * col[0]
    assert np.abs(rgb - np.minimum(want, 1.0)).max() < 1e-14 and cos.min() < 0.8
    assert np.abs(nmap - np.array([0.5, 0.5, 0.0])).max() < 1e-15
    # the same plane seen from behind its normal: the diffuse clamp, and a specular term that is NOT gated on N.L > 0 but is zero here
    rgb2, _ = SH.shade_values(v, f, col, -nrm, R, t, K, H, W, np.zeros(3), (amb, dif, spe), pixel, face)
    assert np.abs(rgb2 - amb * col[0] - (spe * np.maximum(2.0 * cos * cos - 1.0, 0.0))[:, None] * col[0]).max() < 1e-14


def test_oracle_interpolation_is_affine_in_model_coordinates_on_a_slanted_rectangle():
    """colours affine in model coordinates, ambient only: the shaded colour at a pixel is that function of the model point the pixel shows,
    which render_host.xyz_from_depth gives from the depth alone -- perspective-correct interpolation, checked through another route"""
    H, W = 40, 56
    K = np.array([[60.0, 0.4, 27.3], [0.0, 61.0, 19.6], [0.0, 0.0, 1.0]])
    v, f = synth.mesh_rectangle(1, 1)
    v = v * np.array([0.5, 0.3, 1.0])
    A, b0 = np.array([[0.9, 0.1, 0.0], [-0.3, 1.1, 0.0], [0.5, -0.8, 0.0]]), np.array([0.5, 0.4, 0.5])
    col = v @ A.T + b0
    assert col.min() > 0 and col.max() < 1
    R = synth._axis_angle(np.array([[0.6, 0.8, 0.0]]), np.array([55.0]))[0]
    t = np.array([0.02, -0.01, 0.7])
    depth, face, _, _ = SH.visibility_one(v, f, R, t, K, H, W)
    pixel = np.flatnonzero(face >= 0)
    assert len(pixel) > 300 and depth[pixel].max() / depth[pixel].min() > 1.3   # slanted: a real perspective effect
    a, b, c, _ = SH._posed(v, f, R, t)
    n = np.cross(b - a, c - a)[face[pixel]]
    dx, dy = RH.pixel_rays(K, H, W)
    d = np.stack([dx[pixel], dy[pixel], np.ones(len(pixel))], axis=1)
    z64 = np.zeros(H * W)
    z64[pixel] = np.einsum("ij,ij->i", n, a[face[pixel]]) / np.einsum("ij,ij->i", n, d)
    # xyz_from_depth takes fp32 maps: feed it the fp64 depth in two fp32 halves (it is linear in the depth up to the translation)
    hi = z64.astype(np.float32)
    lo = (z64 - hi).astype(np.float32)
    xyz_hi = RH.xyz_from_depth(hi.reshape(H, W), R, t, K)[0].reshape(-1, 3)
    xyz_lo = RH.xyz_from_depth(lo.reshape(H, W), R, np.zeros(3), K)[0].reshape(-1, 3)
    xyz = (xyz_hi + xyz_lo)[pixel]
    assert np.abs(xyz[:, 2]).max() < 1e-12   # on the model plane
    rgb, _ = SH.shade_values(v, f, col, SH.vertex_normals(v, f), R, t, K, H, W, np.zeros(3), (1.0, 0.0, 0.0), pixel, face[pixel])
    assert np.abs(rgb - (xyz @ A.T + b0)).max() < 1e-12
    aff, _ = SH.shade_values(v, f, col, SH.vertex_normals(v, f), R, t, K, H, W, np.zeros(3), (1.0, 0.0, 0.0), pixel, face[pixel], affine=True)
    assert 255.0 * np.abs(aff - rgb).max() > 2.0


def test_vertex_normals_on_the_cube_and_the_sphere():
    v, f = synth.mesh_cube(0.1)
    n = shade.vertex_normals(v, f)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15 and np.abs(n - SH.vertex_normals(v, f)).max() < 1e-15
    out = shade.vertex_normals(v, f[:, ::-1])   # synth.mesh_cube winds its faces clockwise seen from outside: reversed, the normals point outward
    assert np.all(np.einsum("ij,ij->i", out, v) > 0) and np.array_equal(np.sign(out), np.sign(v))   # into the corner's octant
    assert np.abs(out + n).max() < 1e-15                                                         # the orientation follows the winding
    v, f = synth.mesh_icosphere(3, 0.06)
    n = shade.vertex_normals(v, f)
    cos = np.einsum("ij,ij->i", n, v / 0.06)
    assert cos.min() > 0.999 and np.abs(n - SH.vertex_normals(v, f)).max() < 1e-14               # radial on the unperturbed sphere
    with pytest.raises(ValueError):
        shade.vertex_normals(np.concatenate([v, [[0.0, 0.0, 0.0]]]), f)                          # a vertex without a face
    with pytest.raises(ValueError):
        shade.vertex_normals(np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0]]), [[0, 1, 2], [0, 2, 1]])   # the two sides cancel
    with pytest.raises(ValueError):
        shade.vertex_normals(v, f + 1)


def test_fixture_acceptance_conditions():
    for case in synth.SHADE_CASES:
        inp, ora, st = _scene(case)
        assert inp["seed"] == synth.SHADE_SEEDS[case]
        if case == "watertight":
            assert st["edge_band"] == 0.0 and st["edge_band_off"] > 1e-6
        else:
            assert st["edge_band"] > 1e-6, (case, st)
        assert st["near_far_band"] > 1e-9
        assert inp["background"].dtype == np.uint8 and inp["background"].shape == (inp["num_frames"], inp["H"], inp["W"], 3)
        for i in range(len(inp["labels"])):   # the oracle's depth is the depth oracle's
            c = inp["labels"][i]
            ref = RH.render_one(inp["vertices"][c], inp["faces"][c], inp["R"][i], inp["t"][i], inp["K"][i], inp["H"], inp["W"], inp["near"], inp["far"])
            assert np.array_equal(ora.inst[i][0].view(np.uint32), ref.ravel().view(np.uint32))
    # cube: 48 x 64, 4 poses in 4 frames, skewed K, distinct colours, and perspective-correct differs visibly from screen-space affine
    inp, ora, _ = _scene("cube")
    assert (inp["H"], inp["W"], inp["num_frames"]) == (48, 64, 4) and inp["K"][0, 0, 1] != 0 and list(inp["frame"]) == [0, 1, 2, 3]
    assert len(np.unique(np.round(inp["colors"][0], 6), axis=0)) == 8 and 0 <= inp["colors"][0].min() and inp["colors"][0].max() <= 1
    _, vals = ora.frames()
    _, aff = ora.frames(affine=True)
    assert 255.0 * np.nanmax(np.abs(vals - aff)) > 2.0
    # sphere: one pose, three lightings -- default | light behind (diffuse clamped: darker) | saturating weights (clamped at 1)
    inp, ora, _ = _scene("sphere")
    assert len(inp["faces"][0]) == 1280 and (inp["H"], inp["W"], inp["num_frames"]) == (96, 128, 3)
    assert np.array_equal(inp["R"][0], inp["R"][2]) and np.array_equal(ora.index[0] >= 0, ora.index[1] >= 0)
    _, vals = ora.frames()
    m = ora.index[0] >= 0
    assert inp["light"][1][2] > inp["t"][1][2] + 0.1 and vals[1][m].mean() < 0.6 * vals[0][m].mean()
    assert (vals[2][m] == 1.0).mean() > 0.5 and (vals[0][m] == 1.0).mean() < 0.1
    # watertight: exact ties between faces on most pixels
    inp, ora, _ = _scene("watertight")
    assert (ora.inst[0][2] == ora.inst[0][0]).sum() > 3000 and (ora.depth == 2.0).all() and inp["colors"][0].dtype == np.uint8
    # scene: 47 x 61, 3 frames, 7 instances, each there for its reason
    inp, ora, _ = _scene("scene")
    k = synth.SHADE_SCENE_KINDS
    assert (inp["H"], inp["W"], inp["num_frames"], len(inp["labels"])) == (47, 61, 3, 7) and (47 * 61) % 64 != 0
    own = [int((ora.index == i).sum()) for i in range(7)]
    drawn = [int((ora.inst[i][0] != 0).sum()) for i in range(7)]
    assert own[k["sphere_in_front"]] == drawn[k["sphere_in_front"]] > 100 and 30 < own[k["rectangle_behind"]] < drawn[k["rectangle_behind"]]
    a, b = ora.inst[k["tie_first"]], ora.inst[k["tie_second"]]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and own[k["tie_first"]] == drawn[k["tie_first"]] > 100 and own[k["tie_second"]] == 0
    assert not np.array_equal(SH.colors_f64(inp["colors"][1]), SH.colors_f64(inp["colors"][2]))
    tr = (ora.inst[k["truncated"]][0] != 0).reshape(47, 61)
    assert tr[:, -1].any() and tr[-1, :].any() and drawn[k["outside"]] == 0 and drawn[k["behind_camera"]] == 0
    assert not (inp["frame"] == 2).any() and (ora.index[2] == -1).all()
    rgb, _ = ora.frames()
    assert np.array_equal(rgb[2], inp["background"][2]) and not ora.frames(background=False)[0][2].any()


def test_shaded_mesh_table_validation():
    v, f = synth.mesh_cube(0.1)
    u8 = np.arange(24, dtype=np.uint8).reshape(8, 3) * 10
    tb = shade.ShadedMeshTable([v, v], [f, f], [u8, u8 / 255.0], [None, 3.0 * shade.vertex_normals(v, f)])
    assert isinstance(tb, render.MeshTable) and tb.TABLES[:6] == render.MeshTable.TABLES and tb.f_max == 12
    assert tb.colors.dtype == np.float64 and tb.colors.shape == (16, 3) and np.array_equal(tb.colors[:8], u8.astype(np.float64) / 255.0)
    assert np.array_equal(tb.colors[:8], tb.colors[8:]) and np.abs(tb.normals[:8] - tb.normals[8:]).max() < 1e-15
    assert np.abs(np.linalg.norm(tb.normals, axis=1) - 1.0).max() < 1e-15 and tb.normals.flags["C_CONTIGUOUS"]
    ok = np.full((8, 3), 0.5)
    for cols, nrms in ((np.full((8, 3), 1.0 + 1e-9), None), (np.full((8, 3), -1e-9), None), (np.full((8, 3), np.nan), None), (np.zeros((7, 3)), None),
                       (np.full((8, 3), 300, dtype=np.int64), None), (ok, np.zeros((8, 3))), (ok, np.full((8, 3), np.inf)), (ok, np.ones((7, 3))),
                       (ok, np.full((8, 3), np.nan))):
        with pytest.raises(ValueError):
            shade.ShadedMeshTable([v], [f], [cols], None if nrms is None else [nrms])
    with pytest.raises(ValueError):
        shade.ShadedMeshTable([v], [f], [ok, ok])
    with pytest.raises(ValueError):
        shade.ShadedMeshTable([np.concatenate([v, [[0.0, 0.0, 0.0]]])], [f], [np.full((9, 3), 0.5)])   # default normals: a vertex without a face


def test_random_lights_ranges_and_convention():
    assert shade.PHONG == synth.SHADE_PHONG == (0.4, 0.8, 0.3) and shade.LIGHT == synth.SHADE_LIGHT
    assert np.allclose(shade.from_gl_eye_mm([400.0, 400.0, 400.0]), shade.LIGHT, rtol=0, atol=1e-15)
    light, phong = shade.random_lights(4000, np.random.default_rng(5))
    assert light.shape == (4000, 3) and phong.shape == (4000, 3) and light.dtype == np.float64
    # GL eye (x, y, z) in [0, 1000) mm: right, UP, towards the viewer -> camera x in [0, 1), y in (-1, 0], z in (-1, 0] metres
    assert light[:, 0].min() >= 0 and light[:, 0].max() < 1 and light[:, 1].max() <= 0 and light[:, 1].min() > -1 and light[:, 2].max() <= 0
    assert light[:, 2].min() > -1 and np.abs(np.abs(light).mean(axis=0) - 0.5).max() < 0.03
    d = phong - np.array(shade.PHONG)
    assert np.abs(d).max() <= 0.1 and np.abs(d.mean(axis=0)).max() < 0.01 and d.min() < -0.09 and d.max() > 0.09
    a, b = shade.random_lights(3, np.random.default_rng(7)), shade.random_lights(3, np.random.default_rng(7))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert shade.random_lights(64, np.random.default_rng(1), phong=(0.05, 0.0, 1.0))[1].min() >= 0.0   # weights stay valid
    assert shade.random_lights(0, np.random.default_rng(1))[0].shape == (0, 3)


def test_header_section_and_export_list():
    txt = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    sec = txt[txt.index("Shaded colour frames of posed meshes"):]
    assert "added within ABI 5: new entry points, nothing changed" in sec[:200]
    for word in ("gdrn_render_visibility", "gdrn_shade_frames", "face index within the class", "first in input order", "NOT the fp32 depth",
                 "floor(255 rgb_k + 0.5)", "not gated on N.L > 0", "perspective-correct"):
        assert word in sec, word
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("gdrn_render_visibility", "gdrn_shade_frames"):
        assert name in cabi.EXPORTS
        proto = re.search(r"int %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(cabi._SIGS[name]), name
    assert "#define GDRN_ABI_VERSION 5" in txt
    from gdrnet_amd import build

    assert "shade.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "shade.hip"))
