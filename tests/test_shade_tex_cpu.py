"""CPU tests of the textured / flat-shaded renderer's host side (gdrnet_amd.shade.TexturedMeshTable, render_frames_bop, gdrn_shade_frames_tex):
the C-ABI declarations and the entry point's host checks, the table's packing, the oracle tests/tex_host.py against analysis (not against
itself), its tie to the pinned oracle tests/shade_host.py, and the size of the set of pixels the GPU test may leave out."""
import os
import re

import numpy as np
import pytest

import shade_host as SH
import tex_host as TH
from gdrnet_amd import cabi, render, shade, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gdrn_shade_frames_tex"
_scenes = {}


def _scene(case):
    if case not in _scenes:
        inp = synth.make_tex_inputs(case)
        _scenes[case] = (inp, TH.TexScene(inp))
    return _scenes[case]


# ---- the two that fail without the feature ---------------------------------------------------------------------------------
def test_header_section_and_export_list():
    txt = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    sec = txt[txt.index("Textured and flat-shaded frames with the BOP renderer's light model"):]
    assert "added within ABI 5: a new entry point, nothing changed" in sec[:200]
    for word in (NAME, "round-half-to-even", "v = 0 is the bottom row", "faces the camera", "clamp-to-edge", "rint(255 (lw c_k))", "No mipmaps",
                 "x first, then y", "min(1, ambient + diff)", "bit-identical", "GDRN_SHADING_PHONG = 0, GDRN_SHADING_FLAT = 1",
                 "GDRN_TEXFILTER_NEAREST = 0, GDRN_TEXFILTER_BILINEAR = 1", "GDRN_TEX_MAX_SIDE = 16384"):
        assert word in sec, word
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    proto = re.search(r"int %s\((.*?)\);" % NAME, code, flags=re.S).group(1)
    assert len(proto.split(",")) == len(cabi._SIGS[NAME]) == 39
    assert len(cabi._SIGS["gdrn_shade_frames"]) == 32                      # the existing entry point keeps its signature
    assert NAME in cabi.EXPORTS and "#define GDRN_ABI_VERSION 5" in txt
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        assert hasattr(lib, NAME) and hasattr(lib, "gdrn_shade_frames") and lib.gdrn_version() == 5
    assert shade.SHADINGS == {"phong": 0, "flat": 1} and shade.FILTERS == {"nearest": 0, "bilinear": 1} and shade.TEX_MAX_SIDE == 16384
    src = open(os.path.join(ROOT, "gdr-net_amd", "csrc", "shade.hip")).read()
    for fn in ("pick_winner(", "check_face(", "face_geometry("):             # one copy of the winner pick and the geometry, called by both kernels
        assert len(re.findall(r"__device__ __forceinline__ \w+ " + re.escape(fn), src)) == 1 and src.count(fn) == 3, fn


def test_textured_mesh_table_packing_and_validation():
    v, f = synth.mesh_cube(0.1)
    rv, rf = synth.mesh_rectangle(2, 1)
    rng = np.random.default_rng(3)
    t0, t2 = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.random((2, 3, 3))
    uv0, uv2 = rng.random((8, 2)) * 2 - 0.5, rng.random((6, 2))
    u8 = np.arange(24, dtype=np.uint8).reshape(8, 3) * 10
    tb = shade.TexturedMeshTable([v, v, rv], [f, f, rf], [u8, None, None], None, [uv0, None, uv2], [t0, None, t2])
    assert isinstance(tb, shade.ShadedMeshTable) and isinstance(tb, render.MeshTable)
    assert tb.TABLES == shade.ShadedMeshTable.TABLES + ("uvs", "texels", "tex")
    assert tb.tex.dtype == np.int32 and tb.tex.tolist() == [[0, 5, 7], [0, 0, 0], [35, 2, 3]]     # (offset, h, w); h = 0: no texture
    assert tb.texels.dtype == np.uint32 and tb.texels.shape == (41,) and tb.uvs.dtype == np.float64 and tb.uvs.shape == (22, 2)
    # one texel per dword, c0 in the low byte, rows in the order given (row 0 first: nothing is flipped)
    t0p = tb.texels[:35].reshape(5, 7)
    assert np.array_equal(t0p & 0xFF, t0[..., 0]) and np.array_equal((t0p >> 8) & 0xFF, t0[..., 1]) and np.array_equal(t0p >> 16, t0[..., 2])
    t2p = tb.texels[35:].reshape(2, 3)
    want = np.rint(255.0 * t2).astype(np.uint32)                            # floats are rounded with rint
    assert np.array_equal(np.stack([t2p & 0xFF, (t2p >> 8) & 0xFF, t2p >> 16], axis=2), want)
    assert np.array_equal(tb.uvs[:8], uv0) and not tb.uvs[8:16].any() and np.array_equal(tb.uvs[16:], uv2)
    assert np.array_equal(tb.colors[:8], u8 / 255.0) and (tb.colors[8:] == 0.5).all()          # a class without colours is gray
    assert np.abs(np.linalg.norm(tb.normals, axis=1) - 1.0).max() < 1e-15
    plain = shade.TexturedMeshTable([v], [f])                              # nothing but geometry: gray, no texture
    assert (plain.colors == 0.5).all() and plain.texels.shape == (0,) and not plain.tex.any() and not plain.uvs.any()

    def make(uv=uv0, tex=t0, cols=None):
        return shade.TexturedMeshTable([v], [f], None if cols is None else [cols], None, None if uv is None else [uv], [tex])

    make()
    for kw in (dict(uv=None), dict(uv=uv0[:7]), dict(uv=np.zeros((8, 3))), dict(uv=np.full((8, 2), np.nan)), dict(uv=np.full((8, 2), np.inf)),
               dict(tex=np.zeros((5, 7), np.uint8)), dict(tex=np.zeros((5, 7, 4), np.uint8)), dict(tex=np.zeros((0, 7, 3), np.uint8)),
               dict(tex=np.zeros((1, 16385, 3), np.uint8)), dict(tex=np.zeros((5, 7, 3), np.int32)), dict(tex=np.full((5, 7, 3), 1.5)),
               dict(tex=np.full((5, 7, 3), np.nan)), dict(cols=np.full((8, 3), 2.0))):
        with pytest.raises(ValueError):
            make(**kw)
    with pytest.raises(ValueError):
        shade.TexturedMeshTable([v], [f], None, None, [uv0, uv0], [t0])
    with pytest.raises(ValueError):
        shade.TexturedMeshTable([v], [f], None, None, [uv0], [t0, t0])
    big = np.broadcast_to(np.zeros((1, 1, 3), np.uint8), (16384, 16384, 3))   # 2^28 texels each, no memory behind them: the eighth reaches 2^31
    with pytest.raises(ValueError, match="int32"):
        shade.TexturedMeshTable([v] * 8, [f] * 8, None, None, [uv0] * 8, [big] * 8)


def test_entry_point_checks_arguments_before_touching_a_device():
    """every call below returns from the host-side checks: nothing is launched (there is no device where this runs)"""
    lib = cabi.load()
    A = [0x1000 * k for k in range(1, 30)]   # (pointers are only compared with NULL and checked for alignment here)
    F, N, C = 2, 3, 2
    lab, off, inst = np.array([0, 1, 1], np.int32), np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32)
    tex = np.array([[0, 5, 7], [35, 0, 0]], np.int32)

    def call(vis=A[0], uvs=A[9], texels=A[10], texd=A[11], tex_host=tex, n_texels=35, C=C, labels_host=lab, off_h=off, inst_h=inst, F=F, N=N, H=47, W=61,
             light=A[17], ambient=A[18], shading=0, filter=0, bg=None, rgb=A[20], depth=A[21], index=A[22], nmap=None, colors=A[8]):
        host = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return lib.gdrn_shade_frames_tex(vis, A[1], A[2], A[3], A[4], A[5], A[6], A[7], colors, uvs, texels, texd, host(tex_host), n_texels, C, A[12],
                                         host(labels_host), A[13], A[14], A[15], A[16], host(off_h), A[19], host(inst_h), F, N, H, W, light, ambient,
                                         shading, filter, bg, rgb, depth, index, None, nmap, None)

    rows = lambda *r: np.array(r, np.int32)  # noqa: E731
    bad_tex = [rows([-1, 5, 7], [0, 0, 0]), rows([0, 0, 7], [0, 0, 0]), rows([0, 5, 0], [0, 0, 0]), rows([0, -5, -7], [0, 0, 0]), rows([1, 5, 7], [0, 0, 0]),
               rows([0, 5, 7], [30, 2, 3]), rows([0, 16385, 1], [0, 0, 0]), rows([0, 1, 16385], [0, 0, 0]), rows([0, 5, 7], [36, 0, 0]),
               rows([0, 32768, 32768], [0, 0, 0]), rows([2 ** 31 - 1, 5, 7], [0, 0, 0])]
    for kw in [dict(uvs=None), dict(texd=None), dict(tex_host=None), dict(texels=None), dict(n_texels=-1), dict(ambient=None), dict(light=None),
               dict(colors=None), dict(vis=None), dict(shading=2), dict(shading=-1), dict(filter=2), dict(filter=-1), dict(F=0), dict(N=-1), dict(H=0),
               dict(W=-1), dict(C=0), dict(labels_host=None), dict(labels_host=np.array([0, 2, 1], np.int32)), dict(off_h=None),
               dict(off_h=np.array([0, 3, 2], np.int32)), dict(off_h=np.array([1, 2, 3], np.int32)), dict(inst_h=None),
               dict(inst_h=np.array([0, 3, 1], np.int32)), dict(rgb=None), dict(depth=None), dict(index=None), dict(rgb=A[20] + 1), dict(bg=A[23] + 2),
               dict(nmap=A[24] + 3)] + [dict(tex_host=b) for b in bad_tex]:
        assert call(**kw) == -1, kw
    assert call(H=1 << 16, W=1 << 16) == -2            # H * W beyond an int: refused before the launch as well
    assert call(tex_host=rows([0, 0, 0], [0, 0, 0]), n_texels=0, texels=None, H=1 << 16, W=1 << 16) == -2   # no texture at all is a valid table


# ---- the oracle against analysis ----------------------------------------------------------------------------------------------
def test_quad_reproduces_the_texture_row_for_row():
    inp, ora = _scene("quad")
    x0, y0 = synth.TEX_QUAD_ORIGIN
    assert inp["textures"][0].shape == (8, 8, 3) and (inp["H"], inp["W"]) == (32, 32) and inp["ambient"][0] == 1.0
    covered = (ora.index[0] >= 0).reshape(32, 32)
    want = np.zeros((32, 32), bool)
    want[y0 : y0 + 8, x0 : x0 + 8] = True
    assert np.array_equal(covered, want)
    for shading in ("phong", "flat"):
        for filt in ("nearest", "bilinear"):
            rgb, vals, dist = ora.frames(shading, filt)
            assert np.array_equal(rgb[0][y0 : y0 + 8, x0 : x0 + 8], inp["textures"][0]), (shading, filt)   # the flip and the orientation
            assert np.array_equal(rgb[0][~want], inp["background"][0][~want])
            assert (dist[0][want.ravel()] == 0.5).all()                                                    # texel centres, exactly
    # a vertically mirrored texture gives the mirrored image: the rows are not symmetric, so the test above can tell
    assert not np.array_equal(inp["textures"][0], inp["textures"][0][::-1])


def test_uv_on_a_slanted_plane_is_that_of_the_ray_plane_intersection():
    H, W = 40, 56
    K = np.array([[60.0, 0.4, 27.3], [0.0, 61.0, 19.6], [0.0, 0.0, 1.0]])
    v, f = synth.mesh_rectangle(1, 1)
    v = v * np.array([0.5, 0.3, 1.0])
    A, b0 = np.array([[1.7, 0.3], [-0.6, 2.1]]), np.array([0.45, 0.55])
    uv = v[:, :2] @ A.T + b0
    R = synth._axis_angle(np.array([[0.6, 0.8, 0.0]]), np.array([55.0]))[0]
    t = np.array([0.02, -0.01, 0.7])
    depth, face, _, _ = SH.visibility_one(v, f, R, t, K, H, W)
    pixel = np.flatnonzero(face >= 0)
    assert len(pixel) > 300 and depth[pixel].max() / depth[pixel].min() > 1.3   # slanted: a real perspective effect
    tex = np.zeros((4, 4, 3), np.uint8)
    r = TH.tex_values(v, f, None, SH.vertex_normals(v, f), uv, tex, R, t, K, H, W, np.zeros(3), 0.5, pixel, face[pixel])
    # analysis: the ray K^-1 [x, y, 1] meets the model plane z = 0 (normal R[:, 2] through t); the model point's xy gives uv
    y, x = np.divmod(pixel, W)
    d = np.linalg.solve(K, np.stack([x, y, np.ones(len(pixel))]).astype(np.float64)).T
    nrm = R[:, 2]
    P = d * ((nrm @ t) / (d @ nrm))[:, None]
    model = (P - t) @ R
    assert np.abs(model[:, 2]).max() < 1e-14
    assert np.abs(r["uv"] - (model[:, :2] @ A.T + b0)).max() < 1e-12
    assert np.ptp(r["uv"], axis=0).min() > 0.5   # (the coordinates vary over the plane: the check above is not one of a constant)


def test_samplers_at_centres_midpoints_and_outside():
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    h, w = 5, 7
    up = tex[::-1].astype(np.float64) / 255.0          # row j from the bottom
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    uc, vc = ((ii + 0.5) / w).ravel(), ((jj + 0.5) / h).ravel()
    # at a texel centre both filters return that texel; v = 0 is the bottom row
    assert np.array_equal(TH.sample_nearest(tex, uc, vc), up.reshape(-1, 3))
    assert np.abs(TH.sample_bilinear(tex, uc, vc) - up.reshape(-1, 3)).max() < 1e-15
    assert np.array_equal(TH.sample_nearest(tex, np.array([0.01]), np.array([0.01]))[0], tex[h - 1, 0] / 255.0)
    assert np.array_equal(TH.sample_nearest(tex, np.array([0.99]), np.array([0.99]))[0], tex[0, w - 1] / 255.0)
    # midway between two texels: their mean, along x and along y
    um, vm = ((ii[:, :-1] + 1.0) / w).ravel(), ((jj[:, :-1] + 0.5) / h).ravel()
    assert np.abs(TH.sample_bilinear(tex, um, vm) - (0.5 * (up[:, :-1] + up[:, 1:])).reshape(-1, 3)).max() < 1e-15
    um, vm = ((ii[:-1] + 0.5) / w).ravel(), ((jj[:-1] + 1.0) / h).ravel()
    assert np.abs(TH.sample_bilinear(tex, um, vm) - (0.5 * (up[:-1] + up[1:])).reshape(-1, 3)).max() < 1e-15
    # the centre of four texels: the mean of the four
    q = TH.sample_bilinear(tex, np.array([3.0 / w]), np.array([2.0 / h]))[0]
    assert np.abs(q - up[1:3, 2:4].reshape(4, 3).mean(axis=0)).max() < 1e-15
    # outside [0, 1]: the edge texels (clamp-to-edge), however far outside
    for sample in (TH.sample_nearest, TH.sample_bilinear):
        for u, v, want in ((-0.3, vc[0], up[0, 0]), (1.4, vc[0], up[0, w - 1]), (uc[2], -7.0, up[0, 2]), (uc[2], 1e300, up[h - 1, 2]),
                           (-1e300, 2.0, up[h - 1, 0]), (5.0, -5.0, up[0, w - 1])):
            assert np.abs(sample(tex, np.array([u]), np.array([v]))[0] - want).max() < 1e-15, (sample.__name__, u, v)
    one = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)   # a 1 x 1 texture is that colour everywhere
    for sample in (TH.sample_nearest, TH.sample_bilinear):
        assert np.array_equal(sample(one, np.array([0.2, -3.0, 0.5]), np.array([0.7, 9.0, 0.5])), np.tile(one[0, 0] / 255.0, (3, 1)))


def test_flat_normal_is_the_face_normal_turned_towards_the_camera():
    inp = synth.make_shade_inputs("cube")
    v, f0 = inp["vertices"][0], inp["faces"][0]
    H, W = inp["H"], inp["W"]
    for i in range(4):
        R, t, K = inp["R"][i], inp["t"][i], inp["K"][i]
        seen = []
        for f in (f0, f0[:, ::-1].copy()):                         # both windings
            _, face, _, _ = SH.visibility_one(v, f, R, t, K, H, W)
            pixel = np.flatnonzero(face >= 0)
            r = TH.tex_values(v, f, None, SH.vertex_normals(v, f), None, None, R, t, K, H, W, np.zeros(3), 0.5, pixel, face[pixel], "flat")
            vc = v @ R.T + t
            tri = vc[f[face[pixel]]]                                 # the face's vertices in FILE order, not sorted
            n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            par = np.abs(np.einsum("ij,ij->i", r["N"], n))
            assert np.abs(par - 1.0).max() < 1e-14                  # +- the face normal
            g = TH.pixel_geometry(v, f, R, t, K, H, W, pixel, face[pixel])
            assert (np.einsum("ij,ij->i", r["N"], g["P"]) < 0).all() and len(pixel) > 100    # N . P < 0: it faces the camera
            assert np.abs(np.linalg.norm(r["N"], axis=1) - 1.0).max() < 1e-15
            seen.append((pixel, r["N"], r["rgb"]))
        assert np.array_equal(seen[0][0], seen[1][0]) and np.abs(seen[0][1] - seen[1][1]).max() < 1e-15   # the winding does not matter
        assert np.abs(seen[0][2] - seen[1][2]).max() < 1e-15


def test_phong_with_constant_vertex_normals_is_flat_and_lw_never_exceeds_one():
    H, W = 40, 56
    K = np.array([[60.0, 0.4, 27.3], [0.0, 61.0, 19.6], [0.0, 0.0, 1.0]])
    v, f = synth.mesh_rectangle(3, 2)
    v = v * np.array([0.5, 0.3, 1.0])
    R = synth._axis_angle(np.array([[0.6, 0.8, 0.0]]), np.array([35.0]))[0] @ np.diag([1.0, -1.0, -1.0])   # the winding's +z turned to the camera
    t = np.array([0.02, -0.01, 0.7])
    _, face, _, _ = SH.visibility_one(v, f, R, t, K, H, W)
    pixel = np.flatnonzero(face >= 0)
    nrm = np.tile([0.0, 0.0, 1.0], (len(v), 1))
    col = 0.2 + 0.7 * np.random.default_rng(2).random((len(v), 3))
    light = np.array([0.3, -0.2, 0.1])
    out = {s: TH.tex_values(v, f, col, nrm, None, None, R, t, K, H, W, light, 0.25, pixel, face[pixel], s) for s in ("phong", "flat")}
    assert np.abs(out["phong"]["N"] - out["flat"]["N"]).max() < 1e-14 and np.abs(out["phong"]["rgb"] - out["flat"]["rgb"]).max() < 1e-14
    assert out["flat"]["lw"].min() > 0.3 and len(pixel) > 300                  # lit: the two agree on more than the ambient term
    for case in synth.TEX_CASES:
        inp, ora = _scene(case)
        for f_ in range(inp["num_frames"]):
            px = np.flatnonzero(ora.index[f_] >= 0)
            for i in np.unique(ora.index[f_][px]):
                m, c = ora.index[f_][px] == i, inp["labels"][i]
                r = TH.tex_values(inp["vertices"][c], inp["faces"][c], inp["colors"][c], ora.normals[c], inp["uvs"][c], inp["textures"][c], inp["R"][i],
                                  inp["t"][i], inp["K"][i], ora.H, ora.W, inp["light"][f_], inp["ambient"][f_], px[m], ora.face[f_][px][m])
                assert r["lw"].max() <= 1.0 and r["lw"].min() >= inp["ambient"][f_] - 1e-15 and r["rgb"].max() <= 1.0
                if case == "sphere" and f_ == 2:
                    assert (r["lw"] == 1.0).mean() > 0.3 and (r["lw"] < 1.0).any()       # ambient 0.9: the clip at 1 is reached
                if case == "sphere" and f_ == 1:
                    assert (r["lw"] == 0.5).mean() > 0.5                                   # a light behind the object: the diffuse term clamps at 0


# ---- the tie to the pinned oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("scene", "sphere"))
def test_untextured_oracle_equals_shade_host_with_phong_a_1_0(case):
    inp = synth.make_shade_inputs(case)
    ora = SH.Scene(inp)
    a, compared, clipped = 0.1, 0, 0
    for f in range(inp["num_frames"]):
        pixel = np.flatnonzero(ora.index[f] >= 0)
        for i in np.unique(ora.index[f][pixel]):
            m, c = ora.index[f][pixel] == i, inp["labels"][i]
            args = (inp["R"][i], inp["t"][i], inp["K"][i], ora.H, ora.W, inp["light"][f])
            px, fc = pixel[m], ora.face[f][pixel][m]
            old, old_n = SH.shade_values(inp["vertices"][c], inp["faces"][c], inp["colors"][c], ora.normals[c], *args, (a, 1.0, 0.0), px, fc)
            r = TH.tex_values(inp["vertices"][c], inp["faces"][c], inp["colors"][c], ora.normals[c], None, None, *args, a, px, fc)
            assert np.abs(r["nmap"] - old_n).max() < 1e-15
            ok = r["lw"] <= 1.0 - 1e-9       # below the clip the two light models are the same function
            assert np.abs(r["rgb"][ok] - old[ok]).max(initial=0.0) < 1e-14
            off_half = np.abs((255.0 * old) % 1.0 - 0.5) > 1e-9
            sel = ok[:, None] & off_half
            assert np.array_equal(TH.quantise(r["rgb"])[sel], SH.quantise(old)[sel])
            compared += int(sel.sum())
            clipped += int((~ok).sum())
    print(f"{case}: {compared} bytes compared, {clipped} pixels at the clip")
    assert compared > 1000 and clipped > 0   # (and the condition leaves pixels out: the clip at 1 is where the two models part)


# ---- the cap: how many pixels the GPU test may leave out in nearest mode ---------------------------------------------------------
@pytest.mark.parametrize("case", synth.TEX_CASES)
def test_few_covered_pixels_sit_on_a_texel_boundary(case):
    inp, ora = _scene(case)
    assert inp["seed"] == synth.TEX_SEEDS[case]
    _, _, dist = ora.frames()
    covered = ora.index >= 0
    near = int((dist[covered] < TH.NEAR_INT).sum())
    sampled = int(np.isfinite(dist[covered]).sum())
    print(f"{case}: {int(covered.sum())} covered pixels, {sampled} of them textured, {near} within {TH.NEAR_INT} of a texel boundary")
    assert sampled > 60 and near <= 0.01 * covered.sum()
    if case == "sphere":
        assert near == 0
    if case == "quad":
        assert (dist[covered] == 0.5).all()


def test_fixture_contents():
    inp, ora = _scene("cube")
    assert inp["textures"][0].shape == (5, 7, 3) and inp["uvs"][0].min() == -0.5 and inp["uvs"][0].max() == 1.5 and (inp["H"], inp["W"]) == (48, 64)
    r_uv = []
    for f in range(4):
        px = np.flatnonzero(ora.index[f] >= 0)
        r = TH.tex_values(inp["vertices"][0], inp["faces"][0], None, ora.normals[0], inp["uvs"][0], inp["textures"][0], inp["R"][f], inp["t"][f],
                          inp["K"][f], 48, 64, inp["light"][f], 0.5, px, ora.face[f][px])
        r_uv.append(r["uv"])
    r_uv = np.concatenate(r_uv)
    assert r_uv.min() < -0.1 and r_uv.max() > 1.1                       # clamp-to-edge is exercised on covered pixels
    inp, ora = _scene("sphere")
    assert len(inp["faces"][0]) == 1280 and inp["textures"][0].shape == (16, 16, 3) and (inp["H"], inp["W"], inp["num_frames"]) == (96, 128, 3)
    assert not inp["light"][0].any() and inp["light"][1][2] > inp["t"][1][2] + 0.1 and list(inp["ambient"]) == [0.5, 0.5, 0.9]
    inp, ora = _scene("scene")
    k = synth.SHADE_SCENE_KINDS
    assert (inp["H"], inp["W"], inp["num_frames"], len(inp["labels"])) == (47, 61, 3, 7) and (47 * 61) % 64 != 0 and (47 * 61 * 3) % 4 != 0
    own = [int((ora.index == i).sum()) for i in range(7)]
    drawn = [int((ora.inst[i][0] != 0).sum()) for i in range(7)]
    lab, tex = inp["labels"], inp["textures"]
    assert tex[lab[k["sphere_in_front"]]] is not None and tex[lab[k["rectangle_behind"]]] is None and inp["colors"][lab[k["rectangle_behind"]]] is not None
    assert own[k["sphere_in_front"]] == drawn[k["sphere_in_front"]] > 100 and 30 < own[k["rectangle_behind"]] < drawn[k["rectangle_behind"]]
    a, b = ora.inst[k["tie_first"]], ora.inst[k["tie_second"]]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and own[k["tie_first"]] == drawn[k["tie_first"]] > 100 and own[k["tie_second"]] == 0
    assert tex[lab[k["tie_first"]]].shape == (1, 1, 3) and tex[lab[k["tie_second"]]] is None
    c = lab[k["truncated"]]
    assert inp["colors"][c] is None and tex[c] is None
    tr = (ora.inst[k["truncated"]][0] != 0).reshape(47, 61)
    assert tr[:, -1].any() and tr[-1, :].any() and drawn[k["outside"]] == 0 and drawn[k["behind_camera"]] == 0
    assert not (inp["frame"] == 2).any() and (ora.index[2] == -1).all()
    rgb, _, _ = ora.frames()
    assert np.array_equal(rgb[2], inp["background"][2])
    gray = rgb[0].reshape(-1, 3)[ora.index[0] == k["truncated"]]
    assert (gray[:, 0] == gray[:, 1]).all() and (gray[:, 1] == gray[:, 2]).all()
