"""A deliberately naive restatement of COCO maskApi's run-length format (rleEncode, rleDecode, rleToString, rleFrString as published), in plain
Python loops over its rules; nothing is shared with gdrnet_amd.masks.  pycocotools is not installed where this project is built, so this file --
not pycocotools -- is what the tests pin the format to.

The rules: an h x w mask is scanned column-major (p = x * h + y); counts are the lengths of the alternating runs, the first a run of zeros (0 when
pixel (0, 0) is set).  The string holds counts[i] for i <= 2 and counts[i] - counts[i - 2] behind, each value least-significant first in 5-bit
groups as chr(48 + group); bit 0x20 = more groups follow; emission stops when the remaining value is 0 and bit 0x10 of the group is clear, or -1
and bit 0x10 set (arithmetic shifts); on reading, a final group with bit 0x10 set sign-extends the value."""
import numpy as np


def counts_of_mask(mask):
    """rleEncode: the run lengths of a 2-D mask (non-zero = foreground), column-major"""
    h, w = mask.shape
    flat = [1 if v else 0 for v in np.asarray(mask).T.reshape(-1).tolist()]   # column-major: x * h + y
    counts, prev, run = [], 0, 0
    for v in flat:
        if v != prev:
            counts.append(run)
            run, prev = 0, v
        run += 1
    counts.append(run)
    return counts


def string_of_counts(counts):
    """rleToString"""
    chars = []
    for i in range(len(counts)):
        x = int(counts[i])
        if i > 2:
            x -= int(counts[i - 2])
        while True:
            c = x & 0x1F
            x >>= 5
            if c & 0x10:
                more = x != -1
            else:
                more = x != 0
            if more:
                c |= 0x20
            chars.append(chr(c + 48))
            if not more:
                break
    return "".join(chars)


def counts_of_string(s):
    """rleFrString (counts are uint: sums wrap at 2^32)"""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = (c & 0x20) != 0
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[len(counts) - 2]
        counts.append(x % (1 << 32))
    return counts


def mask_of_counts(counts, h, w):
    """rleDecode with its bounds check: runs behind h * w are dropped, pixels behind the last run stay 0"""
    flat, v = [0] * (h * w), 0
    p = 0
    for c in counts:
        for _ in range(int(c)):
            if p >= h * w:
                break
            flat[p] = v
            p += 1
        v = 1 - v
        if p >= h * w:
            break
    return np.array(flat, dtype=np.uint8).reshape(w, h).T.copy()


def mask_to_string(mask):
    return string_of_counts(counts_of_mask(mask))


def string_to_mask(s, h, w):
    return mask_of_counts(counts_of_string(s), h, w)


def canonical(s, h, w):
    """the string rleEncode + rleToString give for the mask a (possibly non-canonical) string decodes to"""
    return mask_to_string(string_to_mask(s, h, w))


# ---- the mask contents the tests share ----------------------------------------------------------------------------------------------------------
def contents(h, w, seed=0):
    """[(name, u8 [h, w] 0 / 1 mask), ...]: all-zero, all-one, a pixel at each corner, single-pixel row and column stripes, a checkerboard,
    Bernoulli 0.5 and 0.02, two filled ellipses"""
    rng = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = [("zeros", np.zeros((h, w), np.uint8)), ("ones", np.ones((h, w), np.uint8))]
    for name, (y, x) in (("corner_tl", (0, 0)), ("corner_tr", (0, w - 1)), ("corner_bl", (h - 1, 0)), ("corner_br", (h - 1, w - 1))):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        out.append((name, m))
    out.append(("row_stripes", (yy % 2 == 0).astype(np.uint8)))
    out.append(("col_stripes", (xx % 2 == 1).astype(np.uint8)))
    out.append(("checker", ((yy + xx) % 2 == 0).astype(np.uint8)))
    out.append(("bernoulli_0.5", (rng.random((h, w)) < 0.5).astype(np.uint8)))
    out.append(("bernoulli_0.02", (rng.random((h, w)) < 0.02).astype(np.uint8)))
    e1 = ((yy - 0.40 * h) / (0.30 * h + 1)) ** 2 + ((xx - 0.35 * w) / (0.22 * w + 1)) ** 2 <= 1.0
    e2 = ((yy - 0.70 * h) / (0.18 * h + 1)) ** 2 + ((xx - 0.70 * w) / (0.27 * w + 1)) ** 2 <= 1.0
    out.append(("ellipses", (e1 | e2).astype(np.uint8)))
    return out
