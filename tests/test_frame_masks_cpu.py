"""CPU tests (-m "not gpu") of the predicted frame masks (gdrnet_amd.frame_masks, csrc/roi_paste.hip): the exported symbols, the checks that
raise before any launch, and the host restatement tests/paste_host.py against implementations it shares nothing with --
torch.nn.functional.grid_sample on the CPU in fp64 for the sampled value p, scipy.ndimage.label for the components -- and against cases whose
answer is known in closed form.  The GPU tests hold the kernels to the restatement bit for bit; these hold the restatement to the world."""
import os

import numpy as np
import pytest
import torch

import paste_host as PH
from gdrnet_amd import cabi, frame_masks, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_roi_components", "gdrn_roi_paste_masks", "gdrn_roi_paste_exclusive")
H, W = PH.FRAME_H, PH.FRAME_W
THR = 0.5
BAND = 1e-9


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
        assert lib.gdrn_version() == 5
    assert "#define GDRN_ABI_VERSION 5" in header
    assert "Predicted instance masks in the frame (added within ABI 5: new entry points, nothing changed)" in header
    from gdrnet_amd import build

    assert "roi_paste.hip" in build.SOURCES
    assert all(callable(getattr(frame_masks, f)) for f in ("largest_component", "paste_masks", "masks_from_maps"))


def test_no_cpu_fallback_and_checks_before_any_launch():
    from gdrnet_amd.cfg import lm13_cfg

    maps = torch.zeros(2, 64, 64)
    centre, scale = [[10.0, 10.0], [20.0, 20.0]], [30.0, 40.0]
    for good in (maps, maps[:, None], np.zeros((2, 64, 64), np.float32)):
        with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
            frame_masks.largest_component(good)
        with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
            frame_masks.paste_masks(good, centre, scale, H, W)
        with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
            frame_masks.paste_masks(good, torch.tensor(centre), np.array(scale, np.float32), H, W, frame=[0, 1], exclusive=True)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):
        frame_masks.masks_from_maps(lm13_cfg(device="cpu"), dict(mask=maps[:, None]), centre, scale, H, W)
    with pytest.raises(cabi.GdrnHipError, match="no CPU fallback"):   # thr == 0, a 2 x 2 map and a 1 x 1 frame are allowed: the next check is the device's
        frame_masks.paste_masks(torch.zeros(1, 2, 2), [[0, 0]], [1e-3], 1, 1, thr=0.0)
    # the scalars, the shapes and the geometry are judged before the device is
    for thr in (-1e-9, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="thr"):
            frame_masks.largest_component(maps, thr)
        with pytest.raises(ValueError, match="thr"):
            frame_masks.paste_masks(maps, centre, scale, H, W, thr)
        with pytest.raises(ValueError, match="thr"):
            frame_masks.masks_from_maps(lm13_cfg(device="cpu"), dict(mask=maps[:, None]), centre, scale, H, W, mask_thr=thr)
    for bad in (torch.zeros(2, 1, 1), torch.zeros(2, 65, 65), torch.zeros(2, 64, 32), torch.zeros(2, 3, 64, 64), torch.zeros(64, 64), torch.zeros(2, 1, 1, 1)):
        with pytest.raises(ValueError):
            frame_masks.largest_component(bad)
        with pytest.raises(ValueError):
            frame_masks.paste_masks(bad, centre, scale, H, W)
    for hw in ((0, W), (H, 0), (-1, W), (32768, 32768), (65536, 16384)):   # 2 * H * W >= 2**31 for the last two
        with pytest.raises(ValueError):
            frame_masks.paste_masks(maps, centre, scale, *hw)
    for s in ([30.0, 0.0], [30.0, -1.0], [float("nan"), 40.0], [30.0, float("inf")], [30.0], [30.0, 40.0, 50.0]):
        with pytest.raises(ValueError, match="scale"):
            frame_masks.paste_masks(maps, centre, s, H, W)
    for c in ([[10.0, float("nan")], [20.0, 20.0]], [[10.0, 10.0], [float("inf"), 20.0]], [[10.0, 10.0]], [10.0, 10.0, 20.0]):
        with pytest.raises(ValueError, match="bbox_center"):
            frame_masks.paste_masks(maps, c, scale, H, W)
    with pytest.raises(ValueError, match="needs frame"):
        frame_masks.paste_masks(maps, centre, scale, H, W, exclusive=True)
    for frame, F in (([0, 2], 2), ([-1, 0], 2), ([0, 1], 1), ([0], 2), ([0, 1, 1], 2), ([0, 1], -1)):
        with pytest.raises(ValueError, match="frame"):
            frame_masks.paste_masks(maps, centre, scale, H, W, frame=frame, num_frames=F, exclusive=True)
    with pytest.raises(ValueError):   # two rows fit, 2**16 frames of 256 x 128 do not
        frame_masks.paste_masks(maps, centre, scale, 256, 128, frame=[0, 1], num_frames=65536, exclusive=True)


def test_entry_points_check_their_arguments_on_the_host():
    """nothing below touches a stream or a device pointer: the device pointers are absent or host memory, and every call is refused (or has
    nothing to do)"""
    lib = cabi.load()
    buf = np.ones(64, dtype=np.float64)
    p = buf.ctypes.data
    geom = np.array([[10.0, 10.0, 30.0], [20.0, 20.0, 40.0]])
    frame = np.array([0, 1], dtype=np.int32)
    csr = np.array([0, 1, 2, 0, 1], dtype=np.int32)
    g, fr, cs = geom.ctypes.data, frame.ctypes.data, csr.ctypes.data
    nan, inf = float("nan"), float("inf")

    comp = lib.gdrn_roi_components
    #       0  1  2   3    4  5  6
    good = [p, 2, 64, 0.5, p, p, p]
    for k, bad in ((1, -1), (2, 1), (2, 65), (2, 0), (3, -0.5), (3, nan), (3, inf), (0, None), (4, None), (5, None), (6, None), (1, 1 << 19)):
        args = list(good)
        args[k] = bad
        assert comp(*args, None) == -1, (k, bad)
    assert comp(None, 0, 64, 0.5, None, None, None, None) == 0       # B == 0
    assert comp(None, 0, 65, 0.5, None, None, None, None) == -1      # ... after the scalars

    paste = lib.gdrn_roi_paste_masks
    #       0  1  2  3  4   5   6   7    8  9  10
    good = [p, p, g, 2, 64, 40, 56, 0.5, p, p, p]
    for k, bad in ((3, -1), (4, 1), (4, 65), (5, 0), (6, 0), (5, -4), (7, -0.5), (7, nan), (7, inf), (0, None), (1, None), (2, None), (8, None),
                   (9, None), (10, None)):
        args = list(good)
        args[k] = bad
        assert paste(*args, None) == -1, (k, bad)
    assert paste(*(good[:5] + [32768, 32768] + good[7:]), None) == -1      # 2 * 2^30 pixels
    assert paste(*(good[:5] + [65536, 32768] + good[7:]), None) == -1      # H * W alone is 2^31
    for bad_geom in ([[10, 10, 0.0]] * 2, [[10, 10, -3.0]] * 2, [[10, 10, nan]] * 2, [[10, 10, inf]] * 2, [[nan, 10, 30]] * 2, [[10, -inf, 30]] * 2,
                     [[10, 10, 30], [10, 10, 0.0]]):
        bg = np.array(bad_geom, dtype=np.float64)
        assert paste(*(good[:2] + [bg.ctypes.data] + good[3:]), None) == -1, bad_geom
    assert paste(None, None, None, 0, 64, 40, 56, 0.5, None, None, None, None) == 0      # B == 0
    assert paste(None, None, None, 0, 64, 0, 56, 0.5, None, None, None, None) == -1      # ... after the scalars

    excl = lib.gdrn_roi_paste_exclusive
    #       0  1  2  3   4  5   6  7  8   9   10  11   12 13 14 15
    good = [p, p, g, fr, p, cs, 2, 2, 64, 40, 56, 0.5, p, p, p, p]
    for k, bad in ((6, -1), (7, -1), (7, 1), (7, 0), (8, 1), (8, 65), (9, 0), (10, 0), (11, -0.5), (11, nan), (11, inf), (0, None), (1, None), (2, None),
                   (3, None), (4, None), (5, None), (12, None), (13, None), (14, None), (15, None)):
        args = list(good)
        args[k] = bad
        assert excl(*args, None) == -1, (k, bad)
    assert excl(*(good[:7] + [1 << 20] + good[8:]), None) == -1            # F * H * W of 2^31 and more
    for bad_frame in ([0, 2], [-1, 0]):
        bf = np.array(bad_frame, dtype=np.int32)
        assert excl(*(good[:3] + [bf.ctypes.data] + good[4:]), None) == -1, bad_frame
    for bad_csr in ([0, 1, 2, 1, 0], [0, 2, 2, 0, 1], [0, 1, 2, 0, 0], [1, 1, 2, 0, 1], [0, 1, 1, 0, 1]):   # not the list of frame = [0, 1]
        bc = np.array(bad_csr, dtype=np.int32)
        assert excl(*(good[:5] + [bc.ctypes.data] + good[6:]), None) == -1, bad_csr
    same = np.array([1, 1], dtype=np.int32)
    for bad_csr in ([0, 0, 2, 1, 0], [0, 0, 2, 0, 0]):                                                      # frame = [1, 1]: rows descending, a row twice
        bc = np.array(bad_csr, dtype=np.int32)
        assert excl(*(good[:3] + [same.ctypes.data, p, bc.ctypes.data] + good[6:]), None) == -1, bad_csr
    bg = np.array([[10, 10, 30], [10, 10, 0.0]], dtype=np.float64)
    assert excl(*(good[:2] + [bg.ctypes.data] + good[3:]), None) == -1
    assert excl(None, None, None, None, None, None, 0, 2, 64, 40, 56, 0.5, None, None, None, None, None) == 0     # B == 0
    assert excl(None, None, None, None, None, None, 0, -1, 64, 40, 56, 0.5, None, None, None, None, None) == -1   # ... after the scalars
    # the module's own list is one the library accepts
    assert list(frame_masks._csr(np.array([1, 0, 1, 1, 0], dtype=np.int32), 3)) == [0, 2, 5, 5, 1, 4, 0, 2, 3]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against independent implementations
# ---------------------------------------------------------------------------------------------------------------------
def _grid_sample(map_, cx, cy, scale):
    """p of every frame pixel by torch's grid_sample on the CPU in fp64: bilinear, zero padding, align_corners=False, g = 2 (u + 0.5) / res - 1"""
    res = map_.shape[0]
    k = res / scale
    u = (torch.arange(W, dtype=torch.float64) - cx) * k + 0.5 * res
    v = (torch.arange(H, dtype=torch.float64) - cy) * k + 0.5 * res
    gx, gy = 2.0 * (u + 0.5) / res - 1.0, 2.0 * (v + 0.5) / res - 1.0
    grid = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W)], dim=-1)[None]
    inp = torch.from_numpy(np.asarray(map_, dtype=np.float64))[None, None]
    return torch.nn.functional.grid_sample(inp, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0].numpy()


def test_the_sampled_value_is_grid_samples():
    maps = PH.geometry_maps()
    ref = PH.paste(maps, PH.GEOMS, H, W, THR)
    worst = in_band = 0
    for n, (m, geo) in enumerate(zip(maps, PH.GEOMS)):
        p, inside = PH.sample(m, *geo, H, W)
        q = _grid_sample(m, *geo)
        d = float(np.abs(p - q).max())
        worst = max(worst, d)
        assert d <= 1e-12, (n, d)
        assert np.abs(q[~inside]).max(initial=0.0) <= 1e-12           # what the rule leaves unread is zero there too
        band = np.abs(q - THR) <= BAND
        in_band += int(band.sum())
        assert np.array_equal(ref["mask"][n][~band], (q > THR)[~band]), n
    print(f"max |p - grid_sample| {worst:.3g}, pixels within {BAND:g} of the threshold {in_band}")
    assert in_band == 0                                               # so no pixel was left out of the comparison
    assert ref["area"][5] == 0 and list(ref["bbox"][5]) == [0, 0, W - 1, H - 1] and not ref["mask"][5].any()   # wholly outside
    assert all(ref["area"][n] > 0 for n in (0, 1, 2, 3, 4, 6))       # every other geometry sets pixels


def _scipy_largest(fg):
    """(num_comp, kept_px, kept pixel set) with scipy.ndimage.label and np.bincount: the most pixels, then the lowest row-major pixel index"""
    from scipy import ndimage

    lab, n = ndimage.label(fg, structure=np.ones((3, 3)))
    if n == 0:
        return 0, 0, np.zeros_like(fg)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    flat = lab.ravel()
    first = np.array([np.flatnonzero(flat == c + 1)[0] for c in range(n)])
    cands = np.flatnonzero(sizes == sizes.max())
    keep = cands[np.argmin(first[cands])]
    return n, int(sizes[keep]), lab == keep + 1


def _tie_map(res=64):
    """two blobs of 12 pixels: the L-shaped one starts lower in the row-major order although most of it lies below the other"""
    m = np.zeros((res, res), dtype=np.float32)
    m[20:23, 40:44] = 0.9                      # a 3 x 4 block, first pixel (20, 40)
    m[19, 5] = 0.8                             # an L: one pixel in row 19, a column below it, a foot
    m[20:29, 5] = 0.8
    m[28, 6:8] = 0.8
    m[50, 50] = 0.7                            # and a third, smaller one
    return m


def test_the_component_rule_is_scipys_labels_and_bincount():
    probs = [synth.hash_uniform(29, f"cc{k}", (64, 64)).astype(np.float32) for k in range(4)]
    thrs = [0.7, 0.62, 0.55, 0.8]
    probs += [_tie_map(), PH.smooth_map(31, "blob"), synth.hash_uniform(29, "small", (5, 5)).astype(np.float32)]
    thrs += [0.5, 0.5, 0.5]
    for k, (m, thr) in enumerate(zip(probs, thrs)):
        got = PH.components(m[None], thr)
        n, px, kept = _scipy_largest(m > np.float32(thr))
        assert got["num_comp"][0] == n and got["kept_px"][0] == px, (k, got["num_comp"][0], n, got["kept_px"][0], px)
        assert np.array_equal(got["filtered"][0] != 0, kept) and np.array_equal(got["filtered"][0][kept], m[kept]), k
        if k < 4:
            assert n >= 20, (k, n)               # tens of components
    tie = PH.components(_tie_map()[None], 0.5)
    assert tie["num_comp"][0] == 3 and tie["kept_px"][0] == 12 and tie["filtered"][0][19, 5] == np.float32(0.8) and not tie["filtered"][0][20:23, 40:44].any()


# ---------------------------------------------------------------------------------------------------------------------
# cases with a known answer
# ---------------------------------------------------------------------------------------------------------------------
def test_identity_scale_copies_the_map():
    m = (0.25 + 0.5 * synth.hash_uniform(37, "id", (64, 64))).astype(np.float32)
    p, inside = PH.sample(m, 28.0, 20.0, 64.0, H, W)            # crop index 32 on (28, 20): map column x + 4, map row y + 12
    assert np.array_equal(p, m[12:12 + H, 4:4 + W].astype(np.float64)) and inside.all()
    out = PH.paste(m[None], [(28.0, 20.0, 64.0)], H, W, 0.125)  # below the map's minimum
    assert out["mask"].all() and out["area"][0] == H * W and list(out["bbox"][0]) == [0, 0, W - 1, H - 1]
    p, inside = PH.sample(m, 40.0, 30.0, 64.0, H, W)            # the window ends inside the frame: columns 8 .. 55 hold map columns 0 .. 47 ...
    assert np.array_equal(p[:, 8:], m[2:2 + H, :W - 8].astype(np.float64))
    assert not inside[:, :8].any() and not p[:, :8].any() and inside[:, 8:].all()   # ... and column 7 has u == -1 exactly: outside


def test_non_finite_taps_and_values_count_as_zero():
    m = PH.smooth_map(41, "nf")
    holes = m.copy()
    holes[10, 10], holes[30, 31], holes[63, 63] = np.nan, np.inf, -np.inf
    zeros = np.where(np.isfinite(holes), holes, np.float32(0))
    for geo in PH.GEOMS:
        a, b = PH.sample(holes, *geo, H, W), PH.sample(zeros, *geo, H, W)
        assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.isfinite(a[0]).all()
    got = PH.components(np.stack([holes, zeros]), 0.5)
    assert np.array_equal(got["filtered"][0], got["filtered"][1]) and got["kept_px"][0] == got["kept_px"][1] > 0


def test_connectivity_is_eight():
    board = (np.indices((64, 64)).sum(axis=0) % 2).astype(np.float32)
    got = PH.components(board[None], 0.5)
    assert got["num_comp"][0] == 1 and got["kept_px"][0] == 2048 and np.array_equal(got["filtered"][0], board)
    corner = np.zeros((64, 64), dtype=np.float32)
    corner[10:14, 10:14] = 1.0
    corner[14:20, 14:20] = 0.75                                 # touches the first blob at one corner only
    got = PH.components(corner[None], 0.5)
    assert got["num_comp"][0] == 1 and got["kept_px"][0] == 16 + 36 and np.array_equal(got["filtered"][0], corner)
    apart = corner.copy()
    apart[14, 14] = apart[14, 15] = apart[15, 14] = 0.0         # the corner pixel and its two neighbours gone: nothing of the second blob touches (13, 13)
    got = PH.components(apart[None], 0.5)
    assert got["num_comp"][0] == 2 and got["kept_px"][0] == 33 and not got["filtered"][0][10:14, 10:14].any()


def test_exclusive_rule_on_a_pair_written_out_by_hand():
    flat = np.full((2, 64, 64), 0.75, dtype=np.float32)
    flat[1] = 0.875
    geo = [(20.0, 20.0, 16.0), (28.0, 20.0, 16.0)]              # squares of 16 pixels, 8 apart in x
    out = PH.paste_exclusive(flat, geo, [0, 0], 1, H, W, THR)
    plain = PH.paste(flat, geo, H, W, THR)
    assert np.array_equal(out["mask"][0] | out["mask"][1], plain["mask"][0] | plain["mask"][1]) and not (out["mask"][0] & out["mask"][1]).any()
    both = (plain["mask"][0] & plain["mask"][1]).astype(bool)
    assert both.any() and (out["index"][0][both] == 1).all()    # the greater value wins the overlap
    same = PH.paste_exclusive(flat[[0, 0]], [geo[0], geo[0]], [0, 0], 1, H, W, THR)
    assert np.array_equal(same["mask"][0], plain["mask"][0]) and not same["mask"][1].any() and same["area"][1] == 0   # equal p: the lower row
    other = PH.paste_exclusive(flat, geo, [0, 1], 2, H, W, THR)  # in different frames nothing interacts
    assert np.array_equal(other["mask"], plain["mask"]) and np.array_equal(other["area"], plain["area"])
