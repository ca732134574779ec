"""Background replacement and colour augmentation of training frames on the device: the block between decoding and ``RoiCropper``.

Device-side mirror of what the reference's ``GDRN_DatasetFromList.read_data`` does per sample on the full frame with numpy, cv2 and imgaug
(core/gdrn_modeling/data_loader.py:319-343): ``replace_bg`` / ``get_bg_image`` with the ``TRUNCATE_FG`` cut (core/base_data_loader.py:320-403,
``resize_short_edge`` core/utils/data_utils.py:161-187) and the imgaug chain of ``INPUT.COLOR_AUG_CODE`` (``COLOR_AUG_TYPE="code"``,
base_data_loader.py:195-243).  Batched: the frames, masks and the background bank are device tensors, and ONE ``gdrn_aug_mask_cuts`` + ONE
``gdrn_aug_frames`` launch produce the whole batch (csrc/augment.hip; the arithmetic of every stage is specified in include/gdrn_hip.h).

``FrameAugmenter.sample`` makes every random decision of a batch on the host (no GPU needed) and returns an ``AugPlan``; ``apply`` contains no
randomness and no device-to-host copy.  The draws come from the ``numpy.random.Generator`` the augmenter was built with -- not from imgaug's or
``random``'s streams: a seeded run does not reproduce the reference's draws, only their distributions.  Order of the draws, per frame:

1. real frames (``img_type != "syn"``): ``random()`` < ``CHANGE_BG_PROB`` -> replace the background (synthetic frames always do, without a draw);
2. when replacing: ``integers(len(bank))`` -> ``bg_index``; with ``TRUNCATE_FG`` ``random()`` -> ``trunc_mode`` (< 0.2 upper, < 0.4 bottom, < 0.6 left,
   < 0.8 right, else none) and, unless none, ``random()`` -> ``trunc_u``;
3. with ``COLOR_AUG_PROB`` > 0 and a non-empty chain: ``random()`` < ``COLOR_AUG_PROB`` -> ``color``;
4. when ``color``: for every op of the chain in order ``random()`` < its ``Sometimes`` probability, and if it fires its own draws --
   ``CoarseDropout``: ``random((gh, gw))`` >= p -> keep grid;  ``GaussianBlur``: none (sigma is fixed per augmenter);  the point ops:
   ``random()`` < per_channel -> 3 values, else 1, then ``integers(a, b + 1, n)`` (``Add``), ``a + (b - a) random(n)`` (``Multiply``,
   ``LinearContrast``) or ``random(n)`` < p (``Invert``).

Differences from the reference, on purpose: an empty mask gives an all-zero ``mask_trunc`` and a frame that is all background (the reference raises
in ``np.min`` of an empty array); ``COLOR_AUG_SYN_ONLY`` has no effect there (both branches are the same line) and none here;
``BG_KEEP_ASPECT_RATIO=False``, other ``COLOR_AUG_TYPE`` values and imgaug ops outside the six below raise ``NotImplementedError``.
File decoding and the DZI jitter (``roi_data.aug_bbox``) stay on the host.  There is no CPU fallback: host tensors raise ``cabi.GdrnHipError``.
"""
import ast
import ctypes as C
import functools

import numpy as np
import torch

from . import cabi

MAX_CELLS = 4096   # GDRN_AUG_MAX_CELLS
MAX_RADIUS = 4     # GDRN_AUG_MAX_RADIUS
SPATIAL_OPS = ("CoarseDropout", "GaussianBlur")
POINT_OPS = ("Add", "Invert", "Multiply", "LinearContrast")


# ---------------------------------------------------------------------------------------------------------------------
# host geometry and tables
# ---------------------------------------------------------------------------------------------------------------------
def bg_geometry(bg_h, bg_w, H, W):
    """get_bg_image (base_data_loader.py:366-403) + resize_short_edge (data_utils.py:174-181) in integers: the top-left crop (ch, cw) of a
    bg_h x bg_w bank image, the resize scale s and the resized size (oh, ow) = cv2's rint(ch s), rint(cw s), clamped to the H x W frame."""
    bg_h, bg_w, H, W = int(bg_h), int(bg_w), int(H), int(W)
    real_hw_ratio = float(H) / float(W)
    if bg_h >= bg_w:   # both branches of :377-399 cut the same way: a slice past the end is the whole side
        ch, cw = min(int(np.ceil(bg_w * real_hw_ratio)), bg_h), bg_w
    else:
        ch, cw = bg_h, min(int(np.ceil(bg_h / real_hw_ratio)), bg_w)
    target_size, max_size = min(H, W), max(H, W)
    s = float(target_size) / float(min(ch, cw))
    if np.round(s * max(ch, cw)) > max_size:
        s = float(max_size) / float(max(ch, cw))
    oh, ow = int(np.rint(ch * s)), int(np.rint(cw * s))
    return ch, cw, s, min(oh, H), min(ow, W)


@functools.lru_cache(maxsize=64)
def blur_kernel(sigma):
    """(radius, fp32 weights) of imgaug's cv2 GaussianBlur: ksize = max(int(3.3 sigma), 5) made odd; exp(-d^2 / (2 sigma^2)) normalised in fp64."""
    sigma = float(sigma)
    ksize = max(int(3.3 * sigma), 5)
    ksize += 1 - ksize % 2
    r = ksize // 2
    if r > MAX_RADIUS:
        raise NotImplementedError(f"GaussianBlur sigma {sigma}: radius {r} > {MAX_RADIUS}")
    d = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return r, (w / w.sum()).astype(np.float32)


def dropout_grid(H, W, size_percent):
    gh, gw = max(int(H * size_percent), 3), max(int(W * size_percent), 3)
    if gh * gw > MAX_CELLS:
        raise ValueError(f"CoarseDropout grid {gh} x {gw} exceeds {MAX_CELLS} cells")
    return gh, gw


def point_table(point_ops):
    """the frame's point ops composed into one [3][256] u8 table (imgaug 0.4's u8 rules, include/gdrn_hip.h); all three channels at once"""
    tab = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    for name, vals in point_ops:
        if name == "Add":
            tab = np.clip(tab.astype(np.int32) + np.array([int(v) for v in vals], dtype=np.int32)[:, None], 0, 255).astype(np.uint8)
        elif name == "Multiply":
            tab = np.clip(tab.astype(np.float32) * np.array(vals, dtype=np.float32)[:, None], 0, 255).astype(np.uint8)
        elif name == "LinearContrast":
            tab = np.clip(np.float32(127) + np.array(vals, dtype=np.float32)[:, None] * (tab.astype(np.float32) - np.float32(127)), 0, 255).astype(np.uint8)
        elif name == "Invert":
            tab = np.where(np.array([bool(v) for v in vals])[:, None], 255 - tab, tab).astype(np.uint8)
        else:
            raise NotImplementedError(f"point op {name}")
    return tab


# ---------------------------------------------------------------------------------------------------------------------
# INPUT.COLOR_AUG_CODE -> structured op list
# ---------------------------------------------------------------------------------------------------------------------
def _name(node):
    if isinstance(node, ast.Name):
        return node.id
    if isinstance(node, ast.Attribute):   # iaa.Add
        return node.attr
    raise NotImplementedError(f"COLOR_AUG_CODE: {ast.dump(node)}")


def _is_rand_call(node):
    f = node.func
    return (isinstance(f, ast.Attribute) and f.attr == "rand" and isinstance(f.value, ast.Attribute) and f.value.attr == "random"
            and isinstance(f.value.value, ast.Name) and f.value.value.id in ("np", "numpy") and not node.args and not node.keywords)


def _number(node, rng):
    """a number or an arithmetic expression of numbers and np.random.rand(), the latter drawn from rng now"""
    if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)) and not isinstance(node.value, bool):
        return node.value
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
        v = _number(node.operand, rng)
        return -v if isinstance(node.op, ast.USub) else v
    if isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult, ast.Div)):
        a, b = _number(node.left, rng), _number(node.right, rng)
        return {ast.Add: a + b, ast.Sub: a - b, ast.Mult: a * b}[type(node.op)] if not isinstance(node.op, ast.Div) else a / b
    if isinstance(node, ast.Call) and _is_rand_call(node):
        return float(rng.random())
    raise NotImplementedError(f"COLOR_AUG_CODE: argument {ast.unparse(node)}")


def _scalar(node, rng, what):
    if isinstance(node, ast.Tuple):
        raise NotImplementedError(f"COLOR_AUG_CODE: a range for {what}")
    return float(_number(node, rng))


def _range(node, rng):
    if isinstance(node, ast.Tuple):
        if len(node.elts) != 2:
            raise NotImplementedError(f"COLOR_AUG_CODE: argument {ast.unparse(node)}")
        return _number(node.elts[0], rng), _number(node.elts[1], rng)
    v = _number(node, rng)
    return v, v


def _per_channel(node, rng):
    if node is None:
        return 0.0
    if isinstance(node, ast.Constant) and isinstance(node.value, bool):
        return 1.0 if node.value else 0.0
    return float(_number(node, rng))


def _args(call, names):
    """positional + keyword arguments of an op call as {name: node}; unknown or repeated names raise"""
    if len(call.args) > len(names):
        raise NotImplementedError(f"COLOR_AUG_CODE: {ast.unparse(call)}")
    got = dict(zip(names, call.args))
    for kw in call.keywords:
        if kw.arg not in names or kw.arg in got:
            raise NotImplementedError(f"COLOR_AUG_CODE: argument {kw.arg} of {ast.unparse(call)}")
        got[kw.arg] = kw.value
    return got


def _op(call, prob, rng):
    if not isinstance(call, ast.Call):
        raise NotImplementedError(f"COLOR_AUG_CODE: {ast.unparse(call)}")
    name = _name(call.func)
    if name == "CoarseDropout":
        a = _args(call, ("p", "size_percent"))
        if set(a) != {"p", "size_percent"}:
            raise NotImplementedError("COLOR_AUG_CODE: CoarseDropout needs p and size_percent")
        return dict(op=name, prob=prob, p=_scalar(a["p"], rng, "CoarseDropout p"), size_percent=_scalar(a["size_percent"], rng, "CoarseDropout size_percent"))
    if name == "GaussianBlur":
        a = _args(call, ("sigma",))
        if "sigma" not in a:
            raise NotImplementedError("COLOR_AUG_CODE: GaussianBlur needs sigma")
        sigma = _scalar(a["sigma"], rng, "GaussianBlur sigma")
        if not 0.0 <= sigma < 3.0:
            raise NotImplementedError(f"COLOR_AUG_CODE: GaussianBlur sigma {sigma} outside [0, 3.0)")
        return dict(op=name, prob=prob, sigma=sigma)
    if name in ("Add", "Multiply", "LinearContrast"):
        first = {"Add": "value", "Multiply": "mul", "LinearContrast": "alpha"}[name]
        a = _args(call, (first, "per_channel"))
        if first not in a:
            raise NotImplementedError(f"COLOR_AUG_CODE: {name} needs its range")
        lo, hi = _range(a[first], rng)
        if name == "Add" and (int(lo) != lo or int(hi) != hi):
            raise NotImplementedError("COLOR_AUG_CODE: Add with a non-integer range")
        if hi < lo:
            lo, hi = hi, lo
        return dict(op=name, prob=prob, value=(int(lo), int(hi)) if name == "Add" else (float(lo), float(hi)), per_channel=_per_channel(a.get("per_channel"), rng))
    if name == "Invert":
        a = _args(call, ("p", "per_channel"))
        if "p" not in a:
            raise NotImplementedError("COLOR_AUG_CODE: Invert needs p")
        return dict(op=name, prob=prob, p=_scalar(a["p"], rng, "Invert p"), per_channel=_per_channel(a.get("per_channel"), rng))
    raise NotImplementedError(f"COLOR_AUG_CODE: op {name}")


def check_op_order(ops):
    """CoarseDropout, then GaussianBlur (each at most once), before every point op: the order the fused kernel applies them in"""
    stage = 0
    for o in ops:
        name = o["op"]
        if name not in SPATIAL_OPS + POINT_OPS:
            raise NotImplementedError(f"colour augmentation op {name}")
        rank = SPATIAL_OPS.index(name) + 1 if name in SPATIAL_OPS else 3
        if rank < stage or (rank == stage and rank < 3):
            raise NotImplementedError(f"colour augmentation: {name} after {'a point op' if stage == 3 else 'GaussianBlur or a second time'}")
        stage = rank
    return ops


def parse_color_aug_code(code, rng):
    """``INPUT.COLOR_AUG_CODE`` -> ``[dict(op=..., prob=..., ...), ...]`` with ``ast`` (nothing is evaluated).  Grammar:
    ``Sequential([Sometimes(p, Op(...)), ...], random_order=False)``, a bare ``Op(...)`` standing for probability 1; ops ``CoarseDropout(p=,
    size_percent=)``, ``GaussianBlur(sigma)``, ``Add((a, b), per_channel=q)``, ``Invert(p, per_channel=True)``, ``Multiply((a, b), per_channel=q)``,
    ``LinearContrast((a, b), per_channel=q)``.  ``np.random.rand()`` inside an argument is drawn from ``rng`` here, once -- when the reference's
    ``eval`` draws it.  Anything else raises ``NotImplementedError`` naming the construct."""
    try:
        tree = ast.parse(code.strip(), mode="eval").body
    except SyntaxError as e:
        raise NotImplementedError(f"COLOR_AUG_CODE does not parse: {e}") from e
    if not isinstance(tree, ast.Call) or _name(tree.func) != "Sequential" or len(tree.args) != 1 or not isinstance(tree.args[0], ast.List):
        raise NotImplementedError("COLOR_AUG_CODE: expected Sequential([...])")
    for kw in tree.keywords:
        if kw.arg != "random_order" or not isinstance(kw.value, ast.Constant) or kw.value.value is not False:
            raise NotImplementedError(f"COLOR_AUG_CODE: Sequential({kw.arg}={ast.unparse(kw.value)})")
    ops = []
    for node in tree.args[0].elts:
        if isinstance(node, ast.Call) and _name(node.func) == "Sometimes":
            if len(node.args) != 2 or node.keywords:
                raise NotImplementedError(f"COLOR_AUG_CODE: {ast.unparse(node)}")
            ops.append(_op(node.args[1], float(_number(node.args[0], rng)), rng))
        else:
            ops.append(_op(node, 1.0, rng))
    return check_op_order(ops)


def resolve_ops(ops, rng):
    """``INPUT.COLOR_AUG_OPS`` (the structured notation of cfg.py) -> the same list with every ``("rand", k)`` value drawn as ``k * rng.random()``"""
    out = []
    for o in ops:
        o = dict(o)
        if o["op"] == "GaussianBlur" and isinstance(o["sigma"], (tuple, list)):
            kind, k = o["sigma"]
            if kind != "rand":
                raise NotImplementedError(f"GaussianBlur sigma {o['sigma']}")
            o["sigma"] = float(k) * float(rng.random())
        if o["op"] == "GaussianBlur" and not 0.0 <= o["sigma"] < 3.0:
            raise NotImplementedError(f"GaussianBlur sigma {o['sigma']} outside [0, 3.0)")
        out.append(o)
    return check_op_order(out)


# ---------------------------------------------------------------------------------------------------------------------
class AugPlan:
    """Every random decision of a batch, one list entry per frame (plain host data, all fields public): ``hw`` (H, W); ``replace_bg``;
    ``bg_index``; ``trunc_mode`` 0..4 and ``trunc_u``; ``color``; ``dropout`` None or a (gh, gw) boolean keep-grid; ``blur_sigma`` None or a
    float; ``point_ops`` ordered [(name, per-channel value triple)].  ``AugPlan(hws)`` is the plan that does nothing."""

    FIELDS = ("hw", "replace_bg", "bg_index", "trunc_mode", "trunc_u", "color", "dropout", "blur_sigma", "point_ops")

    def __init__(self, hws):
        n = len(hws)
        self.hw = [(int(h), int(w)) for h, w in hws]
        self.replace_bg, self.bg_index, self.trunc_mode, self.trunc_u = [False] * n, [0] * n, [4] * n, [0.0] * n
        self.color, self.dropout, self.blur_sigma, self.point_ops = [False] * n, [None] * n, [None] * n, [[] for _ in range(n)]

    def __len__(self):
        return len(self.hw)

    def __eq__(self, other):
        if not isinstance(other, AugPlan) or len(self) != len(other):
            return False
        for f in self.FIELDS:
            if f == "dropout":
                for a, b in zip(self.dropout, other.dropout):
                    if (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
                        return False
            elif getattr(self, f) != getattr(other, f):
                return False
        return True

    def active(self, i):
        """whether frame i needs a launch: its background is replaced, or a colour stage does something"""
        blur = self.blur_sigma[i] is not None and self.blur_sigma[i] >= 1e-3
        return bool(self.replace_bg[i] or (self.color[i] and (self.dropout[i] is not None or blur or len(self.point_ops[i]) > 0)))


class BackgroundBank:
    """The background images on the device, uploaded once: a list of u8 [h, w, 3] numpy arrays (decoding stays with the caller) or device tensors."""

    def __init__(self, images, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise cabi.GdrnHipError("the background bank lives on the GPU (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.images, self.shapes = [], []
        for im in images:
            t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError("bank images must be u8 [h, w, 3]")
            self.images.append(t.to(self.device).contiguous())
            self.shapes.append((int(t.shape[0]), int(t.shape[1])))
        if not self.images:
            raise ValueError("empty background bank")

    def __len__(self):
        return len(self.images)


def _dev(t, device, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise cabi.GdrnHipError(f"{what} must be a device tensor: the frame augmenter runs on the GPU (no CPU fallback)")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
    if t.dtype != torch.uint8:
        raise ValueError(f"{what} must be uint8" + (" or bool" if what == "mask" else ""))
    return t.to(device).contiguous()


class FrameAugmenter:
    """``cfg.INPUT``: ``CHANGE_BG_PROB``, ``TRUNCATE_FG``, ``BG_KEEP_ASPECT_RATIO``, ``COLOR_AUG_PROB``, ``COLOR_AUG_TYPE`` and the chain -- a
    non-empty ``COLOR_AUG_CODE`` string (parsed by ``parse_color_aug_code``) or else the structured ``COLOR_AUG_OPS``.  ``bank``: a
    ``BackgroundBank`` (``sample`` only needs its ``len``).  ``rng``: a ``numpy.random.Generator``; the chain's ``np.random.rand()`` / ``("rand", k)``
    values are drawn from it here, once."""

    def __init__(self, cfg, bank, rng=None):
        inp = cfg.INPUT
        self.rng = rng if rng is not None else np.random.default_rng()
        self.bank = bank
        self.change_bg_prob = float(inp.get("CHANGE_BG_PROB", 0.5))
        self.truncate_fg = bool(inp.get("TRUNCATE_FG", False))
        if not inp.get("BG_KEEP_ASPECT_RATIO", True):
            raise NotImplementedError("INPUT.BG_KEEP_ASPECT_RATIO=False (get_bg_image_v2) is not on the MI355X path")
        self.color_aug_prob = float(inp.get("COLOR_AUG_PROB", 0.0))
        self.ops = []
        if self.color_aug_prob > 0:
            if str(inp.get("COLOR_AUG_TYPE", "")).lower() != "code":
                raise NotImplementedError(f"INPUT.COLOR_AUG_TYPE={inp.get('COLOR_AUG_TYPE')!r}: only \"code\" is on the MI355X path")
            code = inp.get("COLOR_AUG_CODE", "")
            self.ops = parse_color_aug_code(code, self.rng) if code else resolve_ops(inp.get("COLOR_AUG_OPS", []), self.rng)

    # ------------------------------------------------------------------------------------------------------------
    def _values(self, o, draw):
        n = 3 if self.rng.random() < o["per_channel"] else 1
        v = draw(n)
        return tuple(v) if n == 3 else (v[0],) * 3

    def sample(self, frames):
        """``frames``: [(H, W, img_type), ...] -> ``AugPlan``.  Host only; the order of the draws is in the module docstring."""
        rng = self.rng
        plan = AugPlan([(h, w) for h, w, _ in frames])
        for i, (H, W, img_type) in enumerate(frames):
            replace = True if img_type == "syn" else bool(rng.random() < self.change_bg_prob)
            if replace:
                if len(self.bank) == 0:
                    raise ValueError("empty background bank")
                plan.replace_bg[i] = True
                plan.bg_index[i] = int(rng.integers(len(self.bank)))
                if self.truncate_fg:
                    r = rng.random()
                    mode = 0 if r < 0.2 else 1 if r < 0.4 else 2 if r < 0.6 else 3 if r < 0.8 else 4
                    plan.trunc_mode[i] = mode
                    plan.trunc_u[i] = float(rng.random()) if mode < 4 else 0.0
            if self.color_aug_prob > 0 and self.ops and rng.random() < self.color_aug_prob:
                plan.color[i] = True
                for o in self.ops:
                    if not rng.random() < o["prob"]:
                        continue
                    name = o["op"]
                    if name == "CoarseDropout":
                        plan.dropout[i] = rng.random(dropout_grid(H, W, o["size_percent"])) >= o["p"]
                    elif name == "GaussianBlur":
                        plan.blur_sigma[i] = float(o["sigma"])
                    elif name == "Add":
                        a, b = o["value"]
                        plan.point_ops[i].append((name, self._values(o, lambda n: [int(v) for v in rng.integers(a, b + 1, n)])))
                    elif name in ("Multiply", "LinearContrast"):
                        a, b = o["value"]
                        plan.point_ops[i].append((name, self._values(o, lambda n: [float(v) for v in a + (b - a) * rng.random(n)])))
                    else:   # Invert
                        p = o["p"]
                        plan.point_ops[i].append((name, self._values(o, lambda n: [int(v) for v in rng.random(n) < p])))
        return plan

    # ------------------------------------------------------------------------------------------------------------
    def prepare(self, frames, masks, plan):
        """Validate a batch against its plan, allocate the outputs and upload the task table with the keep grids and point-op tables (host
        work a loader thread can do ahead of time).  Arguments as for ``apply``."""
        B = len(plan)
        if len(frames) != B or (masks is not None and len(masks) != B):
            raise ValueError("frames / masks / plan differ in length")
        if B == 0:
            return dict(out=[], n=0)
        device = self.bank.device if isinstance(self.bank, BackgroundBank) else None
        out, tasks, keep, aux = [], [], [], bytearray()
        for i in range(B):
            img = _dev(frames[i], device, "frame")
            device = device or img.device
            H, W = plan.hw[i]
            if tuple(img.shape) != (H, W, 3):
                raise ValueError(f"frame {i} is {tuple(img.shape)}, the plan was drawn for {(H, W, 3)}")
            if not plan.active(i):
                out.append(dict(image=frames[i], mask_trunc=None))
                continue
            res = torch.empty_like(img)
            t = cabi.AugTask(frame=cabi.ptr(img), out=cabi.ptr(res), H=H, W=W, trunc_mode=4, keep_off=-1, lut_off=-1)
            keep += [img, res]
            trunc = None
            if plan.replace_bg[i]:
                if masks is None or masks[i] is None:
                    raise ValueError(f"frame {i}: the plan replaces the background, a mask is needed")
                m = _dev(masks[i], device, "mask")
                if tuple(m.shape) != (H, W):
                    raise ValueError("mask must be [H, W]")
                if not 0 <= plan.bg_index[i] < len(self.bank):
                    raise ValueError(f"bg_index {plan.bg_index[i]} outside the bank")
                if not 0 <= plan.trunc_mode[i] <= 4 or not 0.0 <= plan.trunc_u[i] <= 1.0:
                    raise ValueError("trunc_mode must be 0..4 and trunc_u in [0, 1]")
                bg = self.bank.images[plan.bg_index[i]]
                bh, bw = self.bank.shapes[plan.bg_index[i]]
                ch, cw, s, oh, ow = bg_geometry(bh, bw, H, W)
                trunc = torch.empty(H, W, dtype=torch.uint8, device=device)
                t.mask, t.bg, t.mask_trunc = cabi.ptr(m), cabi.ptr(bg), cabi.ptr(trunc)
                t.inv_scale, t.bg_h, t.bg_w, t.ch, t.cw, t.oh, t.ow = 1.0 / s, bh, bw, ch, cw, oh, ow
                t.trunc_mode, t.trunc_u = int(plan.trunc_mode[i]), float(plan.trunc_u[i])
                keep += [m, trunc]
            if plan.color[i]:
                if plan.dropout[i] is not None:
                    grid = np.ascontiguousarray(np.asarray(plan.dropout[i]) != 0, dtype=np.uint8)
                    if grid.ndim != 2 or grid.size > MAX_CELLS or grid.size == 0:
                        raise ValueError(f"dropout grid {grid.shape}: 2-D with at most {MAX_CELLS} cells")
                    t.gh, t.gw, t.keep_off = grid.shape[0], grid.shape[1], len(aux)
                    aux += grid.tobytes()
                if plan.blur_sigma[i] is not None and plan.blur_sigma[i] >= 1e-3:
                    r, w = blur_kernel(plan.blur_sigma[i])
                    if H <= r or W <= r:
                        raise ValueError(f"frame {i} ({H} x {W}) is not larger than the blur radius {r}")
                    t.blur_r = r
                    for k, v in enumerate(w):
                        t.blur_w[k] = float(v)
                if plan.point_ops[i]:
                    t.lut_off = len(aux)
                    aux += point_table(plan.point_ops[i]).tobytes()
            tasks.append(t)
            out.append(dict(image=res, mask_trunc=trunc))
        n = len(tasks)
        if n == 0:
            return dict(out=out, n=0)
        host = (cabi.AugTask * n)(*tasks)
        blob = torch.frombuffer(bytearray(bytes(host)) + aux + bytearray(16), dtype=torch.uint8).to(device)   # task table + aux, one upload
        cuts = torch.empty(n, 4, dtype=torch.int32, device=device) if any(t.mask for t in tasks) else None
        return dict(out=out, n=n, host=host, blob=blob, aux_bytes=len(aux), cuts=cuts, keep=keep, device=device)

    def launch(self, prep):
        """The two launches of a prepared batch on the current stream; returns ``prep``'s output list."""
        n = prep["n"]
        if n == 0:
            return prep["out"]
        lib = cabi.load()   # raises when libgdrn_hip.so is missing
        host, blob, cuts = prep["host"], prep["blob"], prep["cuts"]
        tab, auxp = blob.data_ptr(), blob.data_ptr() + C.sizeof(host)
        st = torch.cuda.current_stream(prep["device"]).cuda_stream
        if cuts is not None:
            cabi.check(lib.gdrn_aug_mask_cuts(tab, host, n, cabi.ptr(cuts), st), "aug_mask_cuts")
        cabi.check(lib.gdrn_aug_frames(tab, host, n, auxp, prep["aux_bytes"], cabi.ptr(cuts), st), "aug_frames")
        return prep["out"]

    def apply(self, frames, masks, plan):
        """``launch(prepare(frames, masks, plan))``.  ``frames``: device u8 [H, W, 3] each (sizes may differ); ``masks``: device u8 / bool
        [H, W], needed only where the plan replaces the background (``None`` elsewhere, or ``masks=None``).  Returns ``[dict(image=u8 [H, W, 3],
        mask_trunc=u8 [H, W] or None), ...]`` -- new tensors; a frame whose plan does nothing comes back as the input tensor.  No randomness,
        nothing is read back."""
        return self.launch(self.prepare(frames, masks, plan))


    def __call__(self, frames, masks, img_types):
        """``apply(frames, masks, sample(...))``.  The source tensors are only read by launches on the current stream, so dropping them
        afterwards is safe (stream-ordered reuse)."""
        return self.apply(frames, masks, self.sample([(int(f.shape[0]), int(f.shape[1]), ty) for f, ty in zip(frames, img_types)]))
