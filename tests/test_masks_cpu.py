"""CPU tests (-m "not gpu") of gdrnet_amd.masks: the host codec against hand-checked vectors and against the naive restatement of maskApi
(tests/rle_host.py -- the format is pinned to that restatement, not to pycocotools, which is not installed where this is built), RleBatch.from_coco,
the refusal of host tensors and the C-ABI symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rle_host as RH
from gdrnet_amd import cabi, masks as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdrn_rle_decode", "gdrn_rle_count", "gdrn_rle_positions", "gdrn_rle_string")


# ---- the format ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts, string", [
    ([0, 4], "04"),                  # a 2 x 2 all-ones mask
    ([100], "T3"),                   # 100 = 4 + 32 * 3: group 4 with the continuation bit ('T'), then 3
    ([1], "1"),                      # a 1 x 1 zero mask
    ([5, 40, 3, 2], "5X13jN"),       # the fourth is stored as 2 - 40 = -38 = 26 - 64: 'j' = 48 + (26 | 32), then 30 = -2 & 31 with x = -1: 'N'
    ([1, 20, 1, 4], "1d01@"),        # a delta of exactly -16: one group, 16, x = -1 -> '@'
    ([1, 4, 1, 20], "141`0"),        # a delta of exactly 16: bit 0x10 is set and x = 0, so a second group 0 follows
    ([1, 20, 1, 3], "1d01_O"),       # -17: 15 with bit 0x10 clear and x = -1 -> continues; then 31
    ([1, 4, 1, 19], "141?"),         # 15: one group
])
def test_hand_vectors(counts, string):
    assert M.rle_to_string(counts) == string and RH.string_of_counts(counts) == string
    got = M.rle_from_string(string)
    assert got.dtype == np.uint32 and got.tolist() == counts and RH.counts_of_string(string) == counts
    assert M.rle_from_string(string.encode("ascii")).tolist() == counts


def test_hand_masks():
    assert RH.counts_of_mask(np.ones((2, 2), np.uint8)) == [0, 4] and RH.mask_to_string(np.ones((2, 2), np.uint8)) == "04"
    assert RH.counts_of_mask(np.zeros((1, 1), np.uint8)) == [1]
    m = np.array([[0, 1, 0], [1, 1, 0]], np.uint8)   # column-major: 0 1 | 1 1 | 0 0
    assert RH.counts_of_mask(m) == [1, 3, 2] and np.array_equal(RH.mask_of_counts([1, 3, 2], 2, 3), m)
    # zero-length runs: the value flips at every count -- 3 zeros, no ones, 2 zeros, no ones, no zeros, 1 one
    assert np.array_equal(RH.mask_of_counts([3, 0, 2, 0, 0, 1], 2, 3), np.array([[0, 0, 0], [0, 0, 1]], np.uint8))
    assert np.array_equal(RH.mask_of_counts([1, 2, 9], 2, 3), np.array([[0, 1, 0], [1, 0, 0]], np.uint8))    # long: the run is cut at h w
    assert np.array_equal(RH.mask_of_counts([1, 2], 2, 3), np.array([[0, 1, 0], [1, 0, 0]], np.uint8))       # short: the rest is 0


@pytest.mark.parametrize("h, w", [(1, 1), (1, 7), (7, 1), (5, 4), (37, 53)])
def test_round_trips_against_the_restatement(h, w):
    for name, m in RH.contents(h, w):
        counts = RH.counts_of_mask(m)
        s = RH.string_of_counts(counts)
        assert sum(counts) == h * w and (m[0, 0] == 0 or counts[0] == 0) and all(c > 0 for c in counts[1:]), name
        assert M.rle_to_string(counts) == s, name
        assert M.rle_from_string(s).tolist() == counts == RH.counts_of_string(s), name
        assert np.array_equal(RH.string_to_mask(s, h, w), m), name
        assert RH.canonical(s, h, w) == s, name


def test_large_counts_and_wrap():
    counts = [307200, 2 ** 31 - 1, 1, 7, 2 ** 31 - 1]   # four characters; the widest legal tokens; deltas of about -2^31 and +2^31
    s = RH.string_of_counts(counts)
    assert s.startswith("PP\\9") and len(RH.string_of_counts([307200])) == 4   # 307200 = 0 + 32 (0 + 32 (12 + 32 * 9)): 'P' 'P' '\\' '9'
    assert M.rle_to_string(counts) == s and M.rle_from_string(s).tolist() == counts == RH.counts_of_string(s)
    assert max(len(RH.string_of_counts([v])) for v in (2 ** 31 - 1, 2 ** 32 - 1)) == 7


# ---- RleBatch ----------------------------------------------------------------------------------------------------------
def test_from_coco():
    m = RH.contents(9, 11)[-1][1]
    counts = RH.counts_of_mask(m)
    s = RH.string_of_counts(counts)
    b = M.RleBatch.from_coco([dict(size=[9, 11], counts=counts), dict(size=[9, 11], counts=s), dict(size=(2, 2), counts=b"04")])
    assert len(b) == 3 and not b.on_device and b.sizes.tolist() == [[9, 11], [9, 11], [2, 2]]
    assert b.offsets.tolist() == [0, len(s), 2 * len(s), 2 * len(s) + 2] and b.data.dtype == np.uint8
    assert b.to_coco() == [dict(size=[9, 11], counts=s), dict(size=[9, 11], counts=s), dict(size=[2, 2], counts="04")]
    assert len(M.RleBatch.from_coco([])) == 0 and M.decode_bytes(b) == 2 * 112 + 16
    with pytest.raises(NotImplementedError):
        M.RleBatch.from_coco([[[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]])           # a polygon
    for bad in ("0/4", "04p", "04\x7f", "0é4"):
        with pytest.raises(ValueError):
            M.RleBatch.from_coco([dict(size=[2, 2], counts="04"), dict(size=[2, 2], counts=bad)])
    for size in ([0, 4], [4, -1], [65536, 32768], [2 ** 31, 1]):
        with pytest.raises(ValueError):
            M.RleBatch.from_coco([dict(size=size, counts="04")])
    M.RleBatch.from_coco([dict(size=[65536, 32767], counts="04")])          # h w = 2^31 - 65536 is allowed


def test_host_tensors_are_refused():
    b = M.RleBatch.from_coco([dict(size=[2, 2], counts="04")])
    with pytest.raises(cabi.GdrnHipError):
        M.decode(b, device="cpu")
    m = torch.ones(4, 5, dtype=torch.uint8)
    for arg in ([m], m[None], [m.numpy()], [m.bool()]):
        with pytest.raises(cabi.GdrnHipError):
            M.encode(arg)
        with pytest.raises(cabi.GdrnHipError):
            M.stats(arg)
    src = open(M.__file__).read()
    assert "rle_host" not in src and "pycocotools" not in src.replace("with pycocotools", "")


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_by_both_builds():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NAMES:
            assert name in cabi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
        assert lib.gdrn_version() == 5
    assert "#define GDRN_ABI_VERSION 5" in header


def test_ctypes_mirror_has_the_headers_field_order():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    body = re.search(r"typedef struct gdrn_rle_task \{(.*?)\} gdrn_rle_task;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", part).replace("*", " ").split()[-1] for part in decl.split(",")]
    assert fields == [f[0] for f in cabi.RleTask._fields_]
    assert C.sizeof(cabi.RleTask) == 8 + 5 * 8 + 4 * 4 and cabi.RleTask.str_len.offset == 48 and cabi.RleTask.h.offset == 52


def _task(**kw):
    base = dict(mask=0x1000, sy=50, sx=1, h=40, w=50, str_off=0, str_len=8, run_off=0, seg_off=0)   # (pointers are only compared with NULL here)
    base.update(kw)
    return (cabi.RleTask * 1)(cabi.RleTask(**base))


def test_entry_points_check_arguments_before_touching_a_device():
    """every call below returns from the host-side checks: nothing is launched (there is no device in this container)"""
    lib = cabi.load()
    ok = _task()
    D, S, R, NR, T = 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    assert lib.gdrn_rle_decode(None, ok, 1, S, 8, R, 8, NR, T, None) == -1
    assert lib.gdrn_rle_decode(D, None, 1, S, 8, R, 8, NR, T, None) == -1
    assert lib.gdrn_rle_decode(D, ok, 0, S, 8, R, 8, NR, T, None) == -1
    assert lib.gdrn_rle_decode(D, ok, 1, None, 8, R, 8, NR, T, None) == -1
    assert lib.gdrn_rle_decode(D, ok, 1, S, 8, None, 8, NR, T, None) == -1
    assert lib.gdrn_rle_decode(D, ok, 1, S, 8, R, 8, None, T, None) == -1
    assert lib.gdrn_rle_decode(D, ok, 1, S, 8, R, 8, NR, None, None) == -1
    assert lib.gdrn_rle_decode(D, ok, 70000, S, 8, R, 8, NR, T, None) == -2
    for bad in (dict(mask=None), dict(h=0), dict(w=-3), dict(sx=2), dict(sy=64), dict(str_len=-1), dict(str_off=-1), dict(str_off=1),
                dict(str_len=9), dict(run_off=1), dict(run_off=-1)):
        assert lib.gdrn_rle_decode(D, _task(**bad), 1, S, 8, R, 8, NR, T, None) == -1, bad
    assert lib.gdrn_rle_decode(D, _task(h=65536, w=32768, sy=32768), 1, S, 8, R, 8, NR, T, None) == -2
    SEGS, A, B, NTR, POS, LEN, OFF = 0x8000, 0x9000, 0xA000, 0xB000, 0xC000, 0xD000, 0xE000
    nseg, npos = 50 * 3, 40 * 50 + 1
    assert lib.gdrn_rle_count(None, ok, 1, SEGS, nseg, A, B, None) == -1
    assert lib.gdrn_rle_count(D, ok, 1, None, 0, None, None, None) == -1          # nothing wanted
    assert lib.gdrn_rle_count(D, ok, 1, SEGS, nseg, A, None, None) == -1          # area without bbox
    assert lib.gdrn_rle_count(D, ok, 1, SEGS, nseg - 1, A, B, None) == -1         # the segment counts do not fit
    assert lib.gdrn_rle_count(D, ok, 70000, SEGS, nseg, A, B, None) == -2
    assert lib.gdrn_rle_positions(D, ok, 1, SEGS, nseg, NTR, POS, npos - 1, None) == -1
    assert lib.gdrn_rle_positions(D, ok, 1, SEGS, nseg, None, POS, npos, None) == -1
    assert lib.gdrn_rle_positions(D, ok, 1, None, nseg, NTR, POS, npos, None) == -1
    assert lib.gdrn_rle_string(D, ok, 1, NTR, POS, npos, None, None, 0, None, None) == -1        # neither lengths nor strings
    assert lib.gdrn_rle_string(D, ok, 1, NTR, POS, npos, OFF, None, 0, None, None) == -1         # offsets without strings
    assert lib.gdrn_rle_string(D, ok, 1, NTR, POS, npos, OFF, S, 8, LEN, None) == -1             # both passes at once
    assert lib.gdrn_rle_string(D, ok, 1, NTR, POS, npos - 1, None, None, 0, LEN, None) == -1
    assert lib.gdrn_rle_string(D, ok, 1, None, POS, npos, None, None, 0, LEN, None) == -1
    for bad in (dict(mask=None), dict(h=0), dict(w=0), dict(seg_off=-1), dict(seg_off=1)):
        assert lib.gdrn_rle_count(D, _task(**bad), 1, SEGS, nseg, A, B, None) == -1, bad
        assert lib.gdrn_rle_positions(D, _task(**bad), 1, SEGS, nseg, NTR, POS, npos, None) == -1, bad
    for bad in (dict(mask=None), dict(h=-1), dict(run_off=-1), dict(run_off=1)):
        assert lib.gdrn_rle_string(D, _task(**bad), 1, NTR, POS, npos, None, None, 0, LEN, None) == -1, bad
