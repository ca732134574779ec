"""CPU tests (-m "not gpu") of gdrnet_amd.render and its oracle: the brute-force host rasterizer (tests/render_host.py) against an analytic
ray-box oracle, the acceptance condition of the fixtures' seeds (coverage is decided by geometry, never by rounding), its invariance to face
order and winding, golden G13 against synth, the packed mesh table, and the C-ABI symbols."""
import os

import numpy as np
import pytest
import torch

import render_host as RH
from gdrnet_amd import cabi, render, synth

CASES = ("cube", "watertight", "sphere", "mixed", "clip")


@pytest.fixture(scope="module")
def scenes():
    """every scene once: (inputs, host depth, band statistics)"""
    out = {}
    for case in CASES:
        inp, stats = synth.make_render_inputs(case), {}
        out[case] = (inp, RH.render_depth(inp, stats), stats)
    return out


def test_host_rasterizer_matches_the_analytic_cube(scenes):
    inp, depth, _ = scenes["cube"]
    for i in range(len(inp["labels"])):
        ref, thick = RH.cube_depth_analytic(0.1, inp["R"][i], inp["t"][i], inp["K"][i], inp["H"], inp["W"])
        assert np.array_equal(ref != 0, depth[i] != 0), i                     # coverage identical on every pixel
        hit = ref != 0
        assert hit.sum() > 300 and np.abs(thick[hit]).min() > 1e-9            # (no ray grazes an edge of the box: the slab test is decided too)
        # the host's fp64 depth before its rounding: re-evaluate without the cast
        d64 = _depth64(inp, i)
        assert np.max(np.abs(d64[hit] - ref[hit]) / ref[hit]) <= 1e-12
        assert np.array_equal(d64.astype(np.float32), depth[i])


def _depth64(inp, i):
    """the host rasterizer's depth of instance i before the rounding to fp32 (nearest over the covering triangles)"""
    c = inp["labels"][i]
    v = inp["vertices"][c] @ inp["R"][i].T + inp["t"][i]
    f = np.sort(inp["faces"][c], axis=1)
    dx, dy = RH.pixel_rays(inp["K"][i], inp["H"], inp["W"])
    best = np.full(dx.shape, np.inf)
    for ia, ib, ic in f:
        a, b, cc = v[ia], v[ib], v[ic]
        w = [dx * e[0] + (dy * e[1] + e[2]) for e in (np.cross(a, b), np.cross(b, cc), -np.cross(a, cc))]
        inside = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
        n = np.cross(b - a, cc - a)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = n.dot(a) / (dx * n[0] + (dy * n[1] + n[2]))
        best = np.where(inside & (z > 0) & (z < best), z, best)
    return np.where(np.isinf(best), 0.0, best).reshape(inp["H"], inp["W"])


def test_fixture_seeds_keep_pixel_centres_off_the_edges_and_depths_off_near_and_far(scenes):
    for case in CASES:
        inp, depth, st = scenes[case]
        assert inp["seed"] == synth.RENDER_SEEDS[case]
        if case == "watertight":   # on purpose: every pixel centre ON an edge or a vertex, exactly -- and nothing merely close to one
            assert st["edge_band"] == 0.0 and st["edge_band_off"] > 1e-6
        else:
            assert st["edge_band"] > 1e-6, (case, st)
        assert st["near_far_band"] > 1e-9, (case, st)
    # the watertight scene is exact: vertices on integer pixels, a covered frame at exactly 2.0
    inp, depth, _ = scenes["watertight"]
    v = inp["vertices"][0] + inp["t"][0]
    K = inp["K"][0]
    px, py = K[0, 0] * v[:, 0] / v[:, 2] + K[0, 2], K[1, 1] * v[:, 1] / v[:, 2] + K[1, 2]
    assert np.array_equal(px, np.round(px)) and np.array_equal(py, np.round(py)) and px.min() == 0 and px.max() == 63 and py.min() == 0 and py.max() == 63
    assert len(inp["faces"][0]) == 2048 and np.all(depth == np.float32(2.0))


def test_scenes_cover_what_they_are_meant_to(scenes):
    inp, depth, _ = scenes["mixed"]
    assert [len(f) for f in inp["faces"]] == [12, 2048, 1280] and list(inp["labels"]) == [2, 0, 1, 1, 0] and depth.shape == (5, 120, 160)
    assert all((d != 0).sum() > 50 for d in depth)
    inp, depth, _ = scenes["sphere"]
    assert len(inp["faces"][0]) == 1280 and len(inp["vertices"][0]) == 642
    r = np.linalg.norm(inp["vertices"][0], axis=1)
    assert r.max() / r.min() > 1.3   # perturbed: not convex
    inp, depth, _ = scenes["clip"]
    cov = [(d != 0) for d in depth]
    assert cov[0][:, -1].any() and not cov[0][:, :20].any()          # half outside: cut by the last column
    assert not cov[1].any() and not cov[2].any() and not cov[4].any()   # outside the frame | behind the camera | beyond far
    zc = (inp["vertices"][1] @ inp["R"][3].T + inp["t"][3])[:, 2]
    f = inp["faces"][1]
    dropped = (zc[f] < inp["near"]).any(axis=1)
    assert 0 < dropped.sum() < len(f) and (zc[f][dropped] >= inp["near"]).any()   # a triangle CROSSES near: it is dropped, the rest is drawn
    assert cov[3].sum() > 100
    full = RH.render_one(inp["vertices"][1], f[~dropped], inp["R"][3], inp["t"][3], inp["K"][3], inp["H"], inp["W"])
    assert np.array_equal(full, depth[3])


def test_host_rasterizer_is_invariant_to_face_order_and_winding(scenes):
    for case in ("sphere", "cube", "watertight"):
        inp, depth, _ = scenes[case]
        f = inp["faces"][0]
        perm = np.argsort(synth.hash_uniform(7, "perm", (len(f),)))
        flip = synth.hash_uniform(7, "flip", (len(f),)) < 0.5
        g = f[perm].copy()
        g[flip[perm]] = g[flip[perm]][:, ::-1]
        got = RH.render_one(inp["vertices"][0], g, inp["R"][0], inp["t"][0], inp["K"][0], inp["H"], inp["W"])
        assert np.array_equal(got, depth[0]), case


def test_golden_g13_was_drawn_from_these_fixtures(scenes, golden_dir):
    g = np.load(os.path.join(golden_dir, "g13_xyz_targets.npz"))
    for case in CASES:
        inp, depth, _ = scenes[case]
        assert int(g[f"{case}/seed"]) == synth.RENDER_SEEDS[case]
        assert g[f"{case}/depth"].dtype == np.float32 and np.array_equal(g[f"{case}/depth"], depth)
        assert g[f"{case}/xyz"].dtype == np.float64 and g[f"{case}/xyz"].shape == depth.shape + (3,)
        # the host form of the back-projection agrees with the reference's (fp64 against fp64, two ways of inverting K)
        for i in range(len(depth)):
            xyz, mask, xyxy, vis = RH.xyz_from_depth(depth[i], inp["R"][i], inp["t"][i], inp["K"][i])
            assert list(g[f"{case}/xyxy"][i]) == xyxy and vis == int(mask.any())
            assert np.max(np.abs(xyz - g[f"{case}/xyz"][i])) < 1e-13
            assert not g[f"{case}/xyz"][i][~mask].any()


def test_mesh_table_packs_without_padding_and_checks_ranges():
    inp = synth.make_render_inputs("mixed")
    t = render.MeshTable(inp["vertices"], inp["faces"])
    assert t.num_classes == 3 and list(t.nfaces) == [12, 2048, 1280] and list(t.nverts) == [8, 1089, 642] and t.f_max == 2048
    assert list(t.face_off) == [0, 12, 2060] and list(t.vert_off) == [0, 8, 1097]
    assert t.verts.shape == (8 + 1089 + 642, 3) and t.verts.dtype == np.float64 and t.faces.shape == (12 + 2048 + 1280, 3) and t.faces.dtype == np.int32
    for c in range(3):
        assert np.array_equal(t.verts[t.vert_off[c] : t.vert_off[c] + t.nverts[c]], inp["vertices"][c])
        assert np.array_equal(t.faces[t.face_off[c] : t.face_off[c] + t.nfaces[c]], inp["faces"][c])
    bad = inp["faces"][0].copy()
    bad[5, 1] = 8
    with pytest.raises(ValueError):
        render.MeshTable(inp["vertices"], [bad] + inp["faces"][1:])
    bad[5, 1] = -1
    with pytest.raises(ValueError):
        render.MeshTable(inp["vertices"], [bad] + inp["faces"][1:])
    with pytest.raises(ValueError):
        render.MeshTable(inp["vertices"], inp["faces"][:2])
    with pytest.raises(ValueError):
        render.MeshTable(inp["vertices"], [f.astype(np.float64) for f in inp["faces"]])
    assert list(t.check_labels([2, 0, 1])) == [2, 0, 1] and t.check_labels(torch.tensor([1, 1])).dtype == np.int32
    for labels in ([0, 3], [-1], torch.tensor([0, 1, 7])):
        with pytest.raises(ValueError):
            t.check_labels(labels)


def test_render_has_no_cpu_fallback():
    inp = synth.make_render_inputs("cube")
    t = render.MeshTable(inp["vertices"], inp["faces"])
    R, tt, K = (torch.from_numpy(inp[k]) for k in ("R", "t", "K"))
    with pytest.raises(cabi.GdrnHipError):
        render.render_depth(t, inp["labels"], R, tt, K, inp["H"], inp["W"])
    with pytest.raises(cabi.GdrnHipError):
        render.xyz_from_depth(torch.zeros(4, 48, 64), R, tt, K)
    with pytest.raises(cabi.GdrnHipError):
        render.xyz_targets(t, inp["labels"], R.numpy(), tt.numpy(), K.numpy(), inp["H"], inp["W"])


def test_render_symbols_are_declared_and_exported():
    lib = cabi.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gdrn_hip.h")).read()
    for name in ("gdrn_render_depth", "gdrn_xyz_from_depth"):
        assert name in cabi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
    assert lib.gdrn_version() == 5
    # the argument checks come before anything touches a device: a host-only call
    assert lib.gdrn_render_depth(None, None, None, None, None, None, 1, 1, None, None, None, None, None, 1, 8, 8, 0.01, 6.5, None, None) == -1
    assert lib.gdrn_xyz_from_depth(None, None, None, None, 1, 8, 8, None, None, None, None, None) == -1
