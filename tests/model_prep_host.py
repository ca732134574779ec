"""A deliberately naive numpy restatement of the three reference functions behind gdrnet_amd.model_prep, for the tests: the farthest-point
sampling of core/csrc/fps/src/farthest_point_sampling.cpp:122-160 (``init_center=True``), ``misc.calc_pts_diameter`` (lib/pysixd/misc.py:952-966)
and the bounds of ``misc.get_bbox3d_and_center`` / data_loader.py:266-273.  Golden G16 holds the reference's own outputs; tests/test_model_prep_cpu.py
holds this file to them exactly."""
import math

import numpy as np

CORNERS = ((1, 1, 1), (0, 1, 1), (0, 0, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0), (1, 0, 0))   # max (1) or min (0) per axis, misc.py:1016-1027


def fps_indices(pts, K):
    """the reference's index vector [K] int32: fp32 points, start = farthest from the fp32 box centre, (d0 d0 + d1 d1) + d2 d2 in fp32, running
    minimum, arg-max with the lowest index among equal maxima, index 0 when no distance is above 0"""
    p = np.ascontiguousarray(pts, dtype=np.float32)
    q = (p.max(axis=0) + p.min(axis=0)) * np.float32(0.5)
    md = np.full(len(p), np.finfo(np.float32).max, dtype=np.float32)
    out = np.zeros(K, dtype=np.int32)
    for k in range(K):
        d = p - q
        d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d.dtype == np.float32
        md = np.minimum(md, d)
        out[k] = int(np.argmax(md)) if md.max() > 0 else 0   # (argmax: the first of equal maxima)
        q = p[out[k]]
    return out


def fps_points(pts, K):
    """[K,3] fp64: ``pts[idxs]`` of the fp32 array, as fps_utils.farthest_point_sampling returns it (widened by the concatenate behind it)"""
    return np.ascontiguousarray(pts, dtype=np.float32)[fps_indices(pts, K)].astype(np.float64)


def max_sq_dist(pts, chunk=256):
    """the largest (dx dx + dy dy) + dz dz over all pairs, fp64"""
    p = np.asarray(pts, dtype=np.float64)
    best = 0.0
    for i in range(0, len(p), chunk):
        d = p[i:i + chunk, None, :] - p[None, i:, :]
        best = max(best, float(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max()))
    return best


def diameter(pts):
    return math.sqrt(max_sq_dist(pts))


def bounds(pts):
    """(min [3], max [3], mean [3]) fp64"""
    p = np.asarray(pts, dtype=np.float64)
    return p.min(axis=0), p.max(axis=0), np.array([np.average(p[:, a]) for a in range(3)])


def extents(pts):
    lo, hi, _ = bounds(pts)
    return (hi - lo).astype(np.float32)


def bbox3d_and_center(pts):
    lo, hi, mean = bounds(pts)
    return np.array([[(hi if s else lo)[a] for a, s in enumerate(c)] for c in CORNERS] + [list(mean)], dtype=np.float32)


def mean_bound(pts):
    """n 2^-52 max|x| per axis: the error bound of a sum of n terms in ANY order (n - 1 additions, each within 2^-53 of a partial sum that
    max|x| n bounds) carried through the division by n, with a factor 2 to spare"""
    p = np.asarray(pts, dtype=np.float64)
    return len(p) * 2.0 ** -52 * np.abs(p).max(axis=0)


def fsum_mean(pts):
    p = np.asarray(pts, dtype=np.float64)
    return np.array([math.fsum(p[:, a]) / len(p) for a in range(3)])
