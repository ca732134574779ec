"""Plain numpy restatement of the coarse depth alignment (gdrnet_amd.refine.depth_offset / depth_align, include/gdrn_hip.h "Coarse depth
alignment"): the pair rule, the median by np.partition, the shift and the loop.  Written from the header's text, operation for operation; the
renders are an argument (a callable for the loop), so the same code serves the device's renders and the host rasterizer's.  ``key`` restates the
order-preserving integer map the device selects on."""
import numpy as np


def key(d):
    """fp32 -> uint32, order preserving: the sign bit of a non-negative flipped, all bits of a negative inverted"""
    b = np.asarray(d, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def pair_differences(depth_ren, depth_scene, gate):
    """(d [n] fp32 in pixel order, mask [H,W] of the pairs, covered) of one instance: ren, sc [H,W] fp32"""
    ren, sc = np.asarray(depth_ren), np.asarray(depth_scene)
    assert ren.dtype == np.float32 and sc.dtype == np.float32 and ren.shape == sc.shape
    with np.errstate(invalid="ignore"):
        both = (ren > 0) & (sc > 0)
        d = sc - ren                                               # one fp32 subtraction
        mask = both & (np.abs(d.astype(np.float64)) <= gate)
    return d[mask], mask, int((ren > 0).sum())


def median(d):
    """0.5 * (lo + hi) in fp64 of the fp32 values d, lo and hi the elements of ranks (n - 1) // 2 and n // 2"""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.size >= 1
    n = d.size
    part = np.partition(d, [(n - 1) // 2, n // 2])
    return 0.5 * (np.float64(part[(n - 1) // 2]) + np.float64(part[n // 2]))


def offset(depth_ren, depth_scene, gate=0.2, min_pairs=64):
    """dict(offset (NaN when ok is 0), pairs, covered, ok) of one instance"""
    d, _, covered = pair_differences(depth_ren, depth_scene, gate)
    if d.size < min_pairs:
        return dict(offset=np.float64(np.nan), pairs=int(d.size), covered=covered, ok=0)
    return dict(offset=median(d), pairs=int(d.size), covered=covered, ok=1)


def shift(t, off):
    """the translation moved along its viewing ray by `off` in depth"""
    t = np.array(t, dtype=np.float64)
    off = np.float64(off)
    s = off / t[2]
    return np.array([t[0] + s * t[0], t[1] + s * t[1], t[2] + off])


def align(render, R, t0, depth_scene, rounds=2, gate=0.2, min_pairs=64):
    """The loop for one instance: ``render(R, t)`` -> [H,W] fp32, depth_scene [H,W] its frame.  Returns dict(t, ok, pairs, covered, offset,
    trace): trace[k] = the translation round k was evaluated at and its result."""
    t = np.array(t0, dtype=np.float64)
    out = dict(ok=1, pairs=0, covered=0, offset=np.float64(np.nan), trace=[])
    for _ in range(rounds):
        res = offset(render(R, t), depth_scene, gate, min_pairs)
        out.update(res)
        out["trace"].append(dict(t=t.copy(), **res))
        if not res["ok"]:
            break
        t = shift(t, res["offset"])
    out["t"] = t
    return out
