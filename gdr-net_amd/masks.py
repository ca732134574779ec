"""COCO run-length masks on the device: the link between the dataset dicts and ``FrameAugmenter`` / ``RoiCropper``, and back.

Device-side mirror of what the reference does per sample on the host with pycocotools: every dataset file under core/gdrn_modeling/datasets/ keeps
its instance masks as compressed RLE strings (``binary_mask_to_rle(mask, compressed=True)``, lib/utils/mask_utils.py:54-66), every sample decodes
one with ``cocosegm2mask`` (mask_utils.py:93-125; core/gdrn_modeling/data_loader.py:79,326,332), and the evaluator encodes the predicted full-frame
masks after copying them to the host (gdrn_evaluator.py:695-697, "time comsuming step").  Here a string of 1-2 KB goes up instead of a 307 KB
mask, and a string comes down: ``decode`` turns a batch of strings into device u8 [h, w] masks (``gdrn_rle_decode``), ``encode`` turns device masks
into canonical strings (``gdrn_rle_count`` / ``gdrn_rle_positions`` / ``gdrn_rle_string``), ``stats`` gives ``mask2bbox_xyxy`` (mask_utils.py:39-44)
and the pixel count.  The kernels are csrc/rle.hip; the format -- maskApi's, as published -- is specified in include/gdrn_hip.h.

``rle_to_string`` / ``rle_from_string`` are a plain host codec for single masks (tests, tools, a user without a GPU at hand); they are not on the
batch path.  Polygon segmentations (maskApi's ``frPoly``) are not handled: no shipped dataset file stores them.  There is no CPU fallback: host
tensors raise ``cabi.GdrnHipError``.
"""
import numpy as np
import torch

from . import cabi

SEG = 16   # rows of a (column, segment) of gdrn_rle_count


# ---------------------------------------------------------------------------------------------------------------------
# host codec for single masks
# ---------------------------------------------------------------------------------------------------------------------
def rle_to_string(counts):
    """maskApi's rleToString: counts (run lengths, the first a run of zeros) -> the compressed string"""
    c = [int(v) for v in counts]
    out = bytearray()
    for i, v in enumerate(c):
        x = v - c[i - 2] if i > 2 else v
        more = True
        while more:
            g = x & 0x1F
            x >>= 5   # arithmetic
            more = (x != -1) if g & 0x10 else (x != 0)
            out.append(48 + (g | 0x20 if more else g))
    return out.decode("ascii")


def rle_from_string(s):
    """maskApi's rleFrString: the compressed string (str or bytes) -> counts as uint32"""
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts, p = [], 0
    while p < len(b):
        x, k, more = 0, 0, True
        while more and p < len(b):
            c = b[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if more:
            break   # the string ends inside a token
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x & 0xFFFFFFFF)
    return np.array(counts, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
class RleBatch:
    """N masks as compressed strings: ``sizes`` [N, 2] int32 (h, w) and ``offsets`` [N + 1] int64 on the host, ``data`` the concatenated
    characters -- a numpy u8 array (a host batch) or a device u8 tensor (a device batch, what ``encode`` returns)."""

    def __init__(self, sizes, data, offsets):
        self.sizes = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.data = data
        if len(self.offsets) != len(self.sizes) + 1:
            raise ValueError("offsets must have N + 1 entries")

    def __len__(self):
        return len(self.sizes)

    @property
    def on_device(self):
        return isinstance(self.data, torch.Tensor) and self.data.device.type == "cuda"

    @classmethod
    def from_coco(cls, segms):
        """``[{"size": [h, w], "counts": str | bytes | list of ints}, ...]`` (what the dataset dicts hold) -> a host batch.  A list of counts
        is converted with ``rle_to_string``; a polygon raises ``NotImplementedError``; a non-positive size, ``h * w >= 2**31`` or a character
        outside [48, 111] raises ``ValueError``."""
        sizes, parts = [], []
        for s in segms:
            if not isinstance(s, dict) or "counts" not in s or "size" not in s:
                raise NotImplementedError("polygon segmentations (maskApi's frPoly) are not on the MI355X path: store the mask as RLE")
            h, w = (int(v) for v in s["size"])
            if h <= 0 or w <= 0 or h * w >= 2 ** 31:
                raise ValueError(f"mask size {h} x {w}: both sides positive and h * w < 2**31")
            c = s["counts"]
            if isinstance(c, str):
                try:
                    c = c.encode("ascii")
                except UnicodeEncodeError:
                    raise ValueError("RLE string with a character outside [48, 111]") from None
            elif isinstance(c, (bytes, bytearray, memoryview)):
                c = bytes(c)
            else:
                c = rle_to_string(c).encode("ascii")
            sizes.append((h, w))
            parts.append(c)
        data = np.frombuffer(b"".join(parts), dtype=np.uint8)
        if data.size and (int(data.min()) < 48 or int(data.max()) > 111):
            raise ValueError("RLE string with a character outside [48, 111]")
        offsets = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=offsets[1:])
        return cls(np.array(sizes, dtype=np.int32).reshape(-1, 2), data, offsets)

    def to_coco(self):
        """-> ``[{"size": [h, w], "counts": str}, ...]``.  For a device batch this is the one device-to-host copy of the strings."""
        raw = (self.data.cpu().numpy() if isinstance(self.data, torch.Tensor) else np.asarray(self.data)).tobytes()
        return [dict(size=[int(h), int(w)], counts=raw[int(a):int(b)].decode("ascii"))
                for (h, w), a, b in zip(self.sizes, self.offsets[:-1], self.offsets[1:])]


# ---------------------------------------------------------------------------------------------------------------------
def _cuda_device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise cabi.GdrnHipError("RLE masks are decoded and encoded on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _align16(n):
    return (int(n) + 15) & ~15


def decode_bytes(batch):
    """bytes of the one allocation ``decode`` places the masks of ``batch`` in (every mask starts 16-byte aligned)"""
    return int(sum(_align16(int(h) * int(w)) for h, w in batch.sizes))


def decode_prepare(batch, device=None, out=None):
    """Validate a batch, allocate the masks and the workspace and upload the task table with the strings (host work a loader thread can do ahead
    of time).  Arguments as for ``decode``."""
    if not isinstance(batch, RleBatch):
        raise TypeError("decode takes an RleBatch (RleBatch.from_coco)")
    device = batch.data.device if batch.on_device and device is None else _cuda_device(device)
    N = len(batch)
    if N == 0:
        return dict(masks=[], n=0)
    nbytes = decode_bytes(batch)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    elif (not isinstance(out, torch.Tensor) or out.device != device or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < nbytes or out.data_ptr() % 16):
        raise ValueError(f"out must be a contiguous, 16-byte aligned device u8 buffer of at least {nbytes} bytes")
    lens = np.diff(batch.offsets)
    if (lens < 0).any() or lens.max() >= 2 ** 31 or int(batch.offsets[-1]) > len(batch.data) or int(batch.offsets[0]) < 0:
        raise ValueError("offsets do not describe the string buffer")
    host = (cabi.RleTask * N)()
    masks, pos, run = [], 0, 0
    for i, (h, w) in enumerate(batch.sizes):
        h, w = int(h), int(w)
        t = host[i]
        t.mask, t.sy, t.sx, t.h, t.w = out.data_ptr() + pos, w, 1, h, w
        t.str_off, t.str_len, t.run_off = int(batch.offsets[i]), int(lens[i]), run
        masks.append(out[pos:pos + h * w].view(h, w))
        pos += _align16(h * w)
        run += int(lens[i])
    table = bytes(host)
    if batch.on_device:
        blob = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(device)
        strings, sbytes = batch.data.to(device).contiguous(), int(batch.data.numel())
        sptr = strings.data_ptr()
    else:
        data = np.ascontiguousarray(batch.data, dtype=np.uint8)
        blob = torch.frombuffer(bytearray(table) + bytearray(data.tobytes()) + bytearray(16), dtype=torch.uint8).to(device)   # one upload
        strings, sbytes, sptr = blob, int(data.size), blob.data_ptr() + len(table)
    run = max(run, 1)
    return dict(masks=masks, n=N, host=host, blob=blob, strings=strings, sptr=sptr, sbytes=sbytes, run_cap=run, device=device, out=out,
                ends=torch.empty(run, dtype=torch.int32, device=device), nruns=torch.empty(N, dtype=torch.int32, device=device),
                totals=torch.empty(N, dtype=torch.int64, device=device))


def decode_launch(prep, lib=None):
    """The two launches (parse, fill) of a prepared batch on the current stream; returns ``prep``'s list of masks."""
    if prep["n"] == 0:
        return prep["masks"]
    lib = lib or cabi.load()   # raises when libgdrn_hip.so is missing
    st = torch.cuda.current_stream(prep["device"]).cuda_stream
    cabi.check(lib.gdrn_rle_decode(prep["blob"].data_ptr(), prep["host"], prep["n"], prep["sptr"], prep["sbytes"], cabi.ptr(prep["ends"]),
                                   prep["run_cap"], cabi.ptr(prep["nruns"]), cabi.ptr(prep["totals"]), st), "rle_decode")
    return prep["masks"]


def decode(batch, device=None, check=False, out=None, lib=None):
    """``RleBatch`` -> N device u8 [h_i, w_i] tensors with values 0 / 1: views into one allocation (``out``, a 16-byte aligned device u8 buffer of
    ``decode_bytes(batch)`` bytes, when given), each starting 16-byte aligned; sizes may differ.  One upload -- the strings and the task table in
    one blob (a device batch uploads the table only) -- and two launches on the current stream; nothing is read back unless ``check`` is set: then
    the N run totals are read and a total that is not h * w raises ``ValueError``.  Whatever a string says, nothing outside a mask's h * w bytes
    is written: pixels behind the last run are 0, runs behind h * w are dropped.  The result goes straight into ``FrameAugmenter.apply(frames,
    masks, plan)`` and, as ``segmentation``, into ``RoiCropper``.  ``lib``: the library build to call (default ``cabi.load()``).
    ``decode_launch(decode_prepare(batch, device, out))`` is the same in two steps."""
    prep = decode_prepare(batch, device, out)
    masks = decode_launch(prep, lib)
    if check and prep["n"]:
        got = prep["totals"].cpu().numpy()
        want = batch.sizes[:, 0].astype(np.int64) * batch.sizes[:, 1].astype(np.int64)
        bad = np.nonzero(got != want)[0]
        if bad.size:
            raise ValueError(f"RLE string {int(bad[0])}: its runs add up to {int(got[bad[0]])}, the mask has {int(want[bad[0]])} pixels")
    return masks


def _mask_list(masks):
    if isinstance(masks, torch.Tensor):
        if masks.device.type != "cuda":
            masks = [masks]   # (refused below)
        elif masks.dim() != 3:
            raise ValueError("masks: a list of [H, W] tensors or one [N, H, W] tensor")
        else:
            masks = list(masks.unbind(0))
    out, device = [], None
    for m in masks:
        if not isinstance(m, torch.Tensor) or m.device.type != "cuda":
            raise cabi.GdrnHipError("mask must be a device tensor: RLE masks are encoded on the GPU (no CPU fallback)")
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)   # (same strides: no copy)
        if m.dtype != torch.uint8 or m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError("mask must be uint8 or bool [H, W]")
        if int(m.shape[0]) * int(m.shape[1]) >= 2 ** 31:
            raise ValueError("mask with h * w >= 2**31")
        device = m.device if device is None else device
        if m.device != device:
            raise ValueError("masks on different devices")
        out.append(m)
    return out, device


def _encode_table(masks, device):
    """the task table of a list of device masks (strides in bytes; non-contiguous masks are read where they are), on the host and uploaded"""
    N = len(masks)
    host = (cabi.RleTask * N)()
    seg = pos = 0
    for i, m in enumerate(masks):
        h, w = int(m.shape[0]), int(m.shape[1])
        t = host[i]
        t.mask, t.sy, t.sx, t.h, t.w, t.seg_off, t.run_off = m.data_ptr(), int(m.stride(0)), int(m.stride(1)), h, w, seg, pos
        seg += w * ((h + SEG - 1) // SEG)
        pos += h * w + 1
    return host, torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device), seg, pos


def stats(masks, lib=None):
    """``mask2bbox_xyxy`` and the pixel count of device masks (a list of u8 / bool [H, W] or one [N, H, W]; non-zero = foreground):
    ``(area [N] int32, bbox_xyxy [N, 4] int32)`` on the device, bottom-right inclusive; an empty mask gives area 0 and the box
    [0, 0, W - 1, H - 1], as ``render.xyz_from_depth`` does.  Nothing is read back."""
    masks, device = _mask_list(masks)
    N = len(masks)
    if N == 0:
        raise ValueError("no masks")
    lib = lib or cabi.load()
    host, table, _, _ = _encode_table(masks, device)
    area = torch.empty(N, dtype=torch.int32, device=device)
    bbox = torch.empty(N, 4, dtype=torch.int32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    cabi.check(lib.gdrn_rle_count(table.data_ptr(), host, N, None, 0, cabi.ptr(area), cabi.ptr(bbox), st), "rle_count")
    return area, bbox


def encode(masks, lib=None):
    """Device masks (a list of u8 / bool [H, W] tensors or one [N, H, W]; non-contiguous is fine; non-zero = foreground) -> a device ``RleBatch``
    of canonical strings: the counts are exactly ``rleEncode``'s (a leading 0 when pixel (0, 0) is set, no interior zero runs), the characters
    exactly ``rleToString``'s.  The string buffer is sized exactly, not by a cap: the host reads the N string lengths once and allocates.  That
    read and the one in ``to_coco()`` are the only two device-to-host copies.  The pass that counts the transitions also gives ``stats``: the
    result carries ``area`` [N] and ``bbox`` [N, 4] (device int32)."""
    masks, device = _mask_list(masks)
    N = len(masks)
    if N == 0:
        return RleBatch(np.zeros((0, 2), np.int32), np.zeros(0, np.uint8), np.zeros(1, np.int64))
    lib = lib or cabi.load()
    host, table, nseg, npos = _encode_table(masks, device)
    tab = table.data_ptr()
    i32 = dict(dtype=torch.int32, device=device)
    seg, positions, ntrans = torch.empty(nseg, **i32), torch.empty(npos, **i32), torch.empty(N, **i32)
    area, bbox = torch.empty(N, **i32), torch.empty(N, 4, **i32)
    lengths = torch.empty(N, dtype=torch.int64, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    cabi.check(lib.gdrn_rle_count(tab, host, N, cabi.ptr(seg), nseg, cabi.ptr(area), cabi.ptr(bbox), st), "rle_count")
    cabi.check(lib.gdrn_rle_positions(tab, host, N, cabi.ptr(seg), nseg, cabi.ptr(ntrans), cabi.ptr(positions), npos, st), "rle_positions")
    cabi.check(lib.gdrn_rle_string(tab, host, N, cabi.ptr(ntrans), cabi.ptr(positions), npos, None, None, 0, cabi.ptr(lengths), st), "rle_string")
    offsets = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lengths.cpu().numpy(), out=offsets[1:])   # the one read of encode
    total = int(offsets[-1])
    strings = torch.empty(total, dtype=torch.uint8, device=device)
    offs_dev = torch.from_numpy(offsets).to(device)
    cabi.check(lib.gdrn_rle_string(tab, host, N, cabi.ptr(ntrans), cabi.ptr(positions), npos, cabi.ptr(offs_dev), cabi.ptr(strings), total, None, st),
               "rle_string")
    res = RleBatch(np.array([(int(m.shape[0]), int(m.shape[1])) for m in masks], dtype=np.int32), strings, offsets)
    res.area, res.bbox = area, bbox
    return res
