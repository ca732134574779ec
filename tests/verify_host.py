"""Plain numpy integer / fp64 restatement of the hypothesis verification (gdrnet_amd.verify, include/gdrn_hip.h "Hypothesis verification"): the
classification of the pixels, the nine counts, the score in the header's operation order and the selection rule.  Written from the header's
text, per row; the renders are an argument, so the same code serves the device's renders and the host rasterizer's."""
import math

import numpy as np

import render_host as RH

COUNTS = ("covered", "inlier", "occluded", "violated", "unknown", "visible", "mask_px", "inter")
KEYS = COUNTS + ("sum_q", "score", "ok")
Q = 1048576.0


def classify(depth_ren, depth_scene, tau):
    """dict of [H,W] bool maps (covered, unknown, inlier, occluded, violated, visible) and e [H,W] fp64 of one row: ren, sc [H,W] fp32"""
    zr, zc = np.asarray(depth_ren), np.asarray(depth_scene)
    assert zr.dtype == np.float32 and zc.dtype == np.float32 and zr.shape == zc.shape
    with np.errstate(invalid="ignore"):
        covered = zr > 0                                           # a NaN is not, +inf is
        usable = np.isfinite(zc) & (zc > 0)
        e = zr.astype(np.float64) - zc.astype(np.float64)          # exact
        both = covered & usable
        inlier = both & (np.abs(e) <= tau)
        occluded = both & (e > tau)
        violated = both & (e < -tau)
    return dict(covered=covered, unknown=covered & ~usable, inlier=inlier, occluded=occluded, violated=violated, visible=covered & ~occluded, e=e)


def counts(depth_ren, depth_scene, tau, mask=None):
    """the nine integers of one row (python ints); mask [H,W] (nonzero = object) or None"""
    c = classify(depth_ren, depth_scene, tau)
    out = {k: int(c[k].sum()) for k in ("covered", "inlier", "occluded", "violated", "unknown", "visible")}
    m = np.zeros(c["covered"].shape, bool) if mask is None else np.asarray(mask) != 0
    out["mask_px"] = int(m.sum())
    out["inter"] = int((m & c["visible"]).sum())
    out["sum_q"] = int(np.floor(np.abs(c["e"][c["inlier"]]) * Q).astype(np.int64).sum())
    return out


def score(cnt, has_mask, tau=0.01, penalty=1.0, min_covered=64):
    """(score fp64, ok) from a row's counts, the header's operation sequence"""
    if cnt["covered"] < min_covered:
        return np.float64(-np.inf), 0
    tq = np.float64(tau) * np.float64(Q)
    fit = np.float64(cnt["inlier"]) - np.float64(cnt["sum_q"]) / tq
    iou = np.float64(1.0)
    if has_mask:
        uni = cnt["visible"] + cnt["mask_px"] - cnt["inter"]
        iou = np.float64(cnt["inter"]) / np.float64(uni) if uni > 0 else np.float64(0.0)
    return (iou * fit - np.float64(penalty) * np.float64(cnt["violated"])) / np.float64(cnt["covered"]), 1


def verify(depth_ren, depth_scene, frame, mask_obs=None, mask_index=None, tau=0.01, penalty=1.0, min_covered=64):
    """``gdrnet_amd.verify.verify_maps`` on host arrays: dict of [N] arrays (int32; sum_q int64; score fp64)"""
    N = len(depth_ren)
    rows = []
    for i in range(N):
        m = None if mask_obs is None else mask_obs[i if mask_index is None else int(mask_index[i])]
        c = counts(depth_ren[i], depth_scene[int(frame[i])], tau, m)
        c["score"], c["ok"] = score(c, mask_obs is not None, tau, penalty, min_covered)
        rows.append(c)
    out = {k: np.array([r[k] for r in rows], dtype=np.int32) for k in COUNTS + ("ok",)}
    out["sum_q"] = np.array([r["sum_q"] for r in rows], dtype=np.int64)
    out["score"] = np.array([r["score"] for r in rows], dtype=np.float64)
    return out


def key(v):
    """fp64 -> python int, order preserving (-0.0 below +0.0): the sign bit of a non-negative flipped, all bits of a negative inverted"""
    b = int(np.array(v, dtype=np.float64).view(np.uint64))
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def select(score_, ok, group, num_groups):
    """(best [G] int32, best_score [G] fp64): per group the eligible row (ok != 0, score not a NaN) with the highest score, the lowest row on a
    tie; -1 and -inf without one"""
    best = np.full(num_groups, -1, dtype=np.int32)
    best_score = np.full(num_groups, -np.inf, dtype=np.float64)
    for i in range(len(score_)):
        g = int(group[i])
        if ok[i] == 0 or math.isnan(score_[i]):
            continue
        if best[g] < 0 or key(score_[i]) > key(best_score[g]):
            best[g], best_score[g] = i, score_[i]
    return best, best_score


def host_renderer(inp, label, K):
    """render(R, t) -> [H,W] fp32 of class ``label`` of a synth.make_refine_inputs scene by the host rasterizer"""
    c = int(label)
    return lambda R, t: RH.render_one(inp["vertices"][c], inp["faces"][c], R, t, K, inp["H"], inp["W"], inp["near"], inp["far"])
