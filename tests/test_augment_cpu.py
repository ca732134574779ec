"""CPU tests (-m "not gpu") of gdrnet_amd.augment and its oracle: the host restatement (tests/aug_host.py) against golden G15 (the reference's own
replace_bg / get_bg_image), the product module's host geometry against the same tuples, the COLOR_AUG_CODE parser, the composed point-op table
against op-by-op application, the sampler's determinism and firing rates, the refusal of host tensors and the C-ABI symbols."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import aug_host as AH
from gdrnet_amd import augment as A, cabi, synth
from gdrnet_amd.cfg import lm13_cfg, lmo_cfg, ycbv_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the project's own chain (own numbers), every op once so that a plan shows which Sometimes fired
CODE = ("Sequential(["
        "Sometimes(0.4, CoarseDropout(p=0.1, size_percent=0.07)),"
        "Sometimes(0.6, GaussianBlur(0.2 + 0.9*np.random.rand())),"
        "Sometimes(0.55, Add((-17, 31), per_channel=0.25)),"
        "Sometimes(0.35, Invert(0.3, per_channel=True)),"
        "Sometimes(0.45, Multiply((0.7, 1.3), per_channel=0.6)),"
        "Sometimes(0.25, LinearContrast((0.6, 1.9), per_channel=0.4))"
        "], random_order=False)")


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_augment.npz"))


@pytest.fixture(scope="module")
def inputs():
    return synth.make_augment_inputs()


def _cfg(**over):
    cfg = lmo_cfg(device="cpu")
    cfg.INPUT.merge(dict(COLOR_AUG_CODE=CODE, CHANGE_BG_PROB=0.3, COLOR_AUG_PROB=0.7))
    cfg.INPUT.merge(over)
    return cfg


# ---- golden G15 ------------------------------------------------------------------------------------------------------
def test_host_restatement_reproduces_g15(g15, inputs):
    assert int(g15["fixture_seed"]) == inputs["seed"] and list(g15["seeds"]) == list(range(12))
    frame, mask, bg = inputs["frames"][0], inputs["masks"][0], inputs["g15_bg"]
    assert np.array_equal(AH.background(bg, *frame.shape[:2]), bg)   # a bank image of the frame's size is resized by exactly 1
    modes = set()
    for k in g15["seeds"]:
        mode, u = int(g15[f"case{k}/mode"]), float(g15[f"case{k}/u"])
        trunc = AH.truncate_mask(mask != 0, mode, u)
        assert trunc.dtype == np.bool_ and np.array_equal(trunc, g15[f"case{k}/mask"]), k
        assert np.array_equal(AH.composite(frame, trunc, bg), g15[f"case{k}/image"]), k
        modes.add(mode)
    assert modes == {0, 1, 2, 3, 4}


def test_host_geometry_equals_g15(g15):
    assert len(g15["geometry"]) == 24
    for row, s in zip(g15["geometry"], g15["geometry_scale"]):
        bh, bw, H, W, ch, cw, oh, ow = (int(v) for v in row)
        for fn in (A.bg_geometry, AH.bg_geometry):
            got = fn(bh, bw, H, W)
            assert got[:2] == (ch, cw) and got[2] == s and got[3:] == (min(oh, H), min(ow, W)), (fn.__module__, row, got)
    # the fixture pairs cover up- and down-scaling and a zero-padded remainder
    scales = [A.bg_geometry(bh, bw, H, W) for bh, bw in synth.AUG_BANK_SIZES for H, W in synth.AUG_FRAME_SIZES]
    assert any(g[2] > 1 for g in scales) and any(g[2] < 1 for g in scales)
    assert any(g[4] < W for g, (H, W) in zip(scales, list(synth.AUG_FRAME_SIZES) * 4))


def test_background_resize_properties(inputs):
    """the fixed-point bilinear rule: a constant image stays constant, and the result tracks exact bilinear sampling within the 11-bit weights"""
    const = np.full((40, 50, 3), 173, np.uint8)
    out = AH.background(const, 47, 61)
    ch, cw, s, oh, ow = AH.bg_geometry(40, 50, 47, 61)
    assert (out[:oh, :ow] == 173).all() and not out[oh:].any() and not out[:, ow:].any()
    img = inputs["bank"][2]
    H, W = 64, 96
    ch, cw, s, oh, ow = AH.bg_geometry(*img.shape[:2], H, W)
    got = AH.background(img, H, W)[:oh, :ow].astype(np.float64)
    y = np.clip((np.arange(oh) + 0.5) / s - 0.5, 0, ch - 1)
    x = np.clip((np.arange(ow) + 0.5) / s - 0.5, 0, cw - 1)
    y0, x0 = np.floor(y).astype(int), np.floor(x).astype(int)
    y1, x1 = np.minimum(y0 + 1, ch - 1), np.minimum(x0 + 1, cw - 1)
    fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
    c = img[:ch, :cw].astype(np.float64)
    ref = (c[y0][:, x0] * (1 - fx) + c[y0][:, x1] * fx) * (1 - fy) + (c[y1][:, x0] * (1 - fx) + c[y1][:, x1] * fx) * fy
    assert np.abs(got - ref).max() <= 0.5 + 255 * 3 / 2048 + 1e-3   # u8 rounding + three weight roundings of 2^-11 + the float32 position


# ---- parser ----------------------------------------------------------------------------------------------------------
def test_parser_yields_the_structure():
    ops = A.parse_color_aug_code(CODE, np.random.default_rng(3))
    sigma = 0.2 + 0.9 * np.random.default_rng(3).random()
    assert ops == [
        dict(op="CoarseDropout", prob=0.4, p=0.1, size_percent=0.07),
        dict(op="GaussianBlur", prob=0.6, sigma=sigma),
        dict(op="Add", prob=0.55, value=(-17, 31), per_channel=0.25),
        dict(op="Invert", prob=0.35, p=0.3, per_channel=1.0),
        dict(op="Multiply", prob=0.45, value=(0.7, 1.3), per_channel=0.6),
        dict(op="LinearContrast", prob=0.25, value=(0.6, 1.9), per_channel=0.4),
    ]
    assert isinstance(ops[2]["value"][0], int)


def test_parser_draws_an_arithmetic_sigma_once():
    rng = np.random.default_rng(5)
    ops = A.parse_color_aug_code("Sequential([Sometimes(0.5, GaussianBlur(1.1*np.random.rand())), Sometimes(0.5, Multiply((0.9, 1.1)))])", rng)
    ref = np.random.default_rng(5)
    assert ops[0]["sigma"] == 1.1 * ref.random() and ops[1] == dict(op="Multiply", prob=0.5, value=(0.9, 1.1), per_channel=0.0)
    assert rng.random() == ref.random()   # exactly one draw was taken
    # one number per augmenter, not per image: every blurred frame of every batch has it
    cfg = _cfg(COLOR_AUG_CODE="Sequential([GaussianBlur(2.5*np.random.rand())])", COLOR_AUG_PROB=1.0)
    aug = A.FrameAugmenter(cfg, [None], rng=np.random.default_rng(6))
    sig = {s for _ in range(3) for s in aug.sample([(40, 40, "real")] * 5).blur_sigma}
    assert sig == {2.5 * np.random.default_rng(6).random()}


@pytest.mark.parametrize("code", [
    "Sequential([Sometimes(0.5, Add((-5, 5)))], random_order=True)",                                   # random order
    "Sequential([Sometimes(0.5, Affine(scale=(1.0, 1.2)))])",                                          # another op
    "Sequential([Sometimes(0.5, Add((-5, 5))), Sometimes(0.5, GaussianBlur(0.5))])",                   # spatial after point
    "Sequential([Sometimes(0.5, GaussianBlur(0.5)), Sometimes(0.5, CoarseDropout(p=0.1, size_percent=0.1))])",   # dropout after blur
    "Sequential([GaussianBlur(0.5), GaussianBlur(0.7)])",                                              # twice
    "Sequential([Sometimes(0.5, GaussianBlur(3.0))])",                                                 # sigma >= 3.0
    "Sequential([Sometimes(0.5, GaussianBlur((0.1, 0.5)))])",                                          # a per-image sigma range
    "Sequential([Sometimes(0.5, Add((-5, 5), per_channel=0.5, name='x'))])",                           # unknown argument
    "Sequential([Sometimes(0.5, Add(__import__('os').getpid()))])",                                    # anything that would need eval
    "Sequential([Sometimes(0.5, Add(np.random.randint(5)))])",
    "SomeOf(2, [Add((-5, 5))])",
    "OneOf([Add((-5, 5))])",
    "Sequential([Sometimes(0.5, Add((-5, 5)), Add((1, 2)))])",                                         # Sometimes with an else branch
    "Sequential([Sometimes(0.5, Add((-5, 5))",                                                         # does not parse
])
def test_parser_rejects(code):
    with pytest.raises(NotImplementedError):
        A.parse_color_aug_code(code, np.random.default_rng(0))


def test_config_keys_and_rejected_configs():
    for cfg in (lmo_cfg(device="cpu"), ycbv_cfg(device="cpu")):
        inp = cfg.INPUT
        assert (inp.CHANGE_BG_PROB, inp.TRUNCATE_FG, inp.BG_KEEP_ASPECT_RATIO, inp.COLOR_AUG_PROB, inp.COLOR_AUG_TYPE) == (0.5, True, True, 0.8, "code")
        assert [o["op"] for o in inp.COLOR_AUG_OPS] == ["CoarseDropout", "GaussianBlur", "Add", "Invert", "Multiply", "Multiply", "LinearContrast"]
        assert inp.DZI_PAD_SCALE == 1.5   # (what was there stays)
        aug = A.FrameAugmenter(cfg, [None] * 3, rng=np.random.default_rng(2))
        assert aug.ops[1]["sigma"] == 1.2 * np.random.default_rng(2).random() and len(aug.ops) == 7
    assert "COLOR_AUG_PROB" not in lm13_cfg(device="cpu").INPUT
    assert A.FrameAugmenter(lm13_cfg(device="cpu"), [None]).ops == []
    with pytest.raises(NotImplementedError):
        A.FrameAugmenter(_cfg(BG_KEEP_ASPECT_RATIO=False), [None])
    for ty in ("ROI10D", "AAE", "code_albu"):
        with pytest.raises(NotImplementedError):
            A.FrameAugmenter(_cfg(COLOR_AUG_TYPE=ty), [None])


# ---- point-op table --------------------------------------------------------------------------------------------------
def _random_point_ops(rng):
    ops = []
    for _ in range(int(rng.integers(1, 6))):
        name = A.POINT_OPS[int(rng.integers(4))]
        if name == "Add":
            v = [int(x) for x in rng.integers(-60, 61, 3)]
        elif name == "Invert":
            v = [int(x) for x in rng.integers(0, 2, 3)]
        else:
            v = [float(x) for x in rng.uniform(0.3, 2.5, 3)]
        ops.append((name, tuple(v)))
    return ops


def test_composed_table_equals_op_by_op_application():
    rng = np.random.default_rng(11)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)   # a 1 x 256 image holding every value in every channel
    for _ in range(200):
        ops = _random_point_ops(rng)
        img = ramp
        for name, vals in ops:
            img = AH.point_op(img, name, vals)
        tab = A.point_table(ops)
        assert tab.dtype == np.uint8 and tab.shape == (3, 256)
        assert np.array_equal(tab, img[0].T), ops
    assert np.array_equal(A.point_table([]), np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    # the rules themselves, on known values
    assert A.point_table([("Add", (-10, 0, 300))])[:, 5].tolist() == [0, 5, 255]
    assert A.point_table([("Multiply", (1.5, 0.5, 1.0))])[:, 201].tolist() == [255, 100, 201]       # truncating
    assert A.point_table([("LinearContrast", (2.0, 0.5, 1.0))])[:, 100].tolist() == [73, 113, 100]  # 127 + a (i - 127), truncating
    assert A.point_table([("Invert", (1, 0, 1))])[:, 3].tolist() == [252, 3, 252]


# ---- sampler ---------------------------------------------------------------------------------------------------------
def test_sample_is_deterministic_for_equal_generators():
    frames = [(47, 61, "real"), (33, 9, "syn"), (64, 96, "real")] * 20
    a = A.FrameAugmenter(_cfg(), [None] * 4, rng=np.random.default_rng(21))
    b = A.FrameAugmenter(_cfg(), [None] * 4, rng=np.random.default_rng(21))
    pa, pb = a.sample(frames), b.sample(frames)
    assert pa == pb and a.ops == b.ops and len(pa) == 60
    assert a.sample(frames) == b.sample(frames) and not pa == a.sample(frames)
    assert all(pa.replace_bg[i] for i in range(1, 60, 3))        # synthetic frames always replace
    assert pa.hw[:3] == [(47, 61), (33, 9), (64, 96)]
    d = next(x for x in pa.dropout if x is not None)
    assert d.dtype == np.bool_
    assert A.AugPlan([(4, 5)]) == A.AugPlan([(4, 5)]) and not A.AugPlan([(4, 5)]).active(0)


def _within(k, n, p):
    return abs(k - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


def test_sample_fires_at_the_configured_rates():
    """4 000 real frames under a fixed seed: every decision's count lies within 5 binomial standard deviations (deterministic: cannot flake)"""
    N = 4000
    aug = A.FrameAugmenter(_cfg(), [None] * 4, rng=np.random.default_rng(31))
    plan = aug.sample([(40, 60, "real")] * N)
    nbg = sum(plan.replace_bg)
    assert _within(nbg, N, 0.3)
    for m in range(5):
        assert _within(sum(1 for i in range(N) if plan.replace_bg[i] and plan.trunc_mode[i] == m), nbg, 0.2), m
    for j in range(4):
        assert _within(sum(1 for i in range(N) if plan.replace_bg[i] and plan.bg_index[i] == j), nbg, 0.25), j
    assert all(plan.trunc_mode[i] == 4 and plan.trunc_u[i] == 0.0 for i in range(N) if not plan.replace_bg[i])
    us = np.array([plan.trunc_u[i] for i in range(N) if plan.replace_bg[i] and plan.trunc_mode[i] < 4])
    assert us.min() >= 0 and us.max() < 1 and abs(us.mean() - 0.5) <= 5 * math.sqrt(1 / 12 / len(us))
    ncol = sum(plan.color)
    assert _within(ncol, N, 0.7)
    col = [i for i in range(N) if plan.color[i]]
    assert all(plan.dropout[i] is None and plan.blur_sigma[i] is None and not plan.point_ops[i] for i in range(N) if not plan.color[i])
    assert _within(sum(plan.dropout[i] is not None for i in col), ncol, 0.4)
    assert _within(sum(plan.blur_sigma[i] is not None for i in col), ncol, 0.6)
    for name, p, pc in (("Add", 0.55, 0.25), ("Invert", 0.35, 1.0), ("Multiply", 0.45, 0.6), ("LinearContrast", 0.25, 0.4)):
        hits = [v for i in col for n, v in plan.point_ops[i] if n == name]
        assert _within(len(hits), ncol, p), name
        if name != "Invert":
            assert _within(sum(len(set(v)) > 1 for v in hits), len(hits), pc * (1 - (1 / 49 ** 2 if name == "Add" else 0))), name
    cells = np.concatenate([plan.dropout[i].ravel() for i in col if plan.dropout[i] is not None])
    assert plan.dropout[next(i for i in col if plan.dropout[i] is not None)].shape == (3, 4)   # max(int(40 * 0.07), 3), int(60 * 0.07)
    assert _within(int((~cells).sum()), len(cells), 0.1)
    adds = np.array([v for i in col for n, v in plan.point_ops[i] if n == "Add"])
    assert adds.min() == -17 and adds.max() == 31
    inv = np.array([v for i in col for n, v in plan.point_ops[i] if n == "Invert"])
    assert _within(int(inv.sum()), inv.size, 0.3)
    order = [n for n, _ in next(plan.point_ops[i] for i in col if len(plan.point_ops[i]) == 4)]
    assert order == ["Add", "Invert", "Multiply", "LinearContrast"]


# ---- product module, host side ---------------------------------------------------------------------------------------
def test_host_tensors_are_refused(inputs):
    aug = A.FrameAugmenter(_cfg(), [None] * 4, rng=np.random.default_rng(1))
    frame = torch.from_numpy(inputs["frames"][0])
    plan = A.AugPlan([(47, 61)])
    plan.color[0], plan.point_ops[0] = True, [("Add", (3, 3, 3))]
    with pytest.raises(cabi.GdrnHipError):
        aug.apply([frame], None, plan)
    with pytest.raises(cabi.GdrnHipError):
        aug.apply([inputs["frames"][0]], None, plan)          # numpy is not a device tensor either
    with pytest.raises(cabi.GdrnHipError):
        aug([frame], [None], ["real"])
    with pytest.raises(cabi.GdrnHipError):
        A.BackgroundBank(inputs["bank"], device="cpu")
    src = open(A.__file__).read()
    assert "aug_host" not in src and "eval(" not in src.replace("``eval``", "")


def test_blur_kernel_and_dropout_grid():
    r, w = A.blur_kernel(0.7)
    r2, w2 = AH.gaussian_weights(0.7)
    assert r == r2 == 2 and w.dtype == np.float32 and np.array_equal(w, w2) and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6
    assert A.blur_kernel(2.99)[0] == 4 and A.blur_kernel(1.9)[0] == 3 and A.blur_kernel(1.81)[0] == 2
    with pytest.raises(NotImplementedError):
        A.blur_kernel(3.1)
    assert A.dropout_grid(47, 61, 0.05) == (3, 3) and A.dropout_grid(480, 640, 0.05) == (24, 32)
    with pytest.raises(ValueError):
        A.dropout_grid(480, 640, 0.2)   # 96 x 128 cells


# ---- C ABI -----------------------------------------------------------------------------------------------------------
NAMES = ("gdrn_aug_mask_cuts", "gdrn_aug_frames")


def test_symbols_are_declared_and_exported_by_both_builds():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NAMES:
            assert name in cabi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
        assert lib.gdrn_version() == 5
    assert "#define GDRN_AUG_MAX_CELLS 4096" in header and "#define GDRN_AUG_MAX_RADIUS 4" in header
    assert (A.MAX_CELLS, A.MAX_RADIUS) == (4096, 4)


def test_ctypes_mirror_has_the_headers_field_order():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    body = re.search(r"typedef struct gdrn_aug_task \{(.*?)\} gdrn_aug_task;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", part).replace("*", " ").split()[-1] for part in decl.split(",")]
    assert fields == [f[0] for f in cabi.AugTask._fields_]
    assert C.sizeof(cabi.AugTask) == 5 * 8 + 2 * 8 + 14 * 4 + 9 * 4 + 4   # five pointers, two doubles, 14 ints, 9 floats, tail padding
    assert cabi.AugTask.blur_w.offset == 112 and cabi.AugTask.inv_scale.offset == 40 and cabi.AugTask.H.offset == 56


def _task(**kw):
    base = dict(frame=0x1000, out=0x2000, H=40, W=50, trunc_mode=4, keep_off=-1, lut_off=-1)   # (pointers are only compared with NULL here)
    base.update(kw)
    return cabi.AugTask(**base)


def _frames_status(lib, task, aux_bytes=4096, cuts=0x4000, B=1, dev=0x3000):
    host = (cabi.AugTask * 1)(task)
    return lib.gdrn_aug_frames(dev, host, B, 0x5000, aux_bytes, cuts, None)


def test_entry_points_check_arguments_before_touching_a_device():
    """every call below returns from the host-side checks: nothing is launched (there is no device in this container)"""
    lib = cabi.load()
    host = (cabi.AugTask * 1)(_task())
    assert lib.gdrn_aug_frames(None, host, 1, None, 0, None, None) == -1
    assert lib.gdrn_aug_frames(0x3000, None, 1, None, 0, None, None) == -1
    assert lib.gdrn_aug_frames(0x3000, host, 0, None, 0, None, None) == -1
    assert lib.gdrn_aug_frames(0x3000, host, 1, None, 16, None, None) == -1          # aux bytes without aux
    assert lib.gdrn_aug_frames(0x3000, host, 70000, None, 0, None, None) == -2
    assert lib.gdrn_aug_mask_cuts(None, host, 1, 0x4000, None) == -1
    assert lib.gdrn_aug_mask_cuts(0x3000, host, 1, None, None) == -1
    assert lib.gdrn_aug_mask_cuts(0x3000, host, 70000, 0x4000, None) == -2
    assert lib.gdrn_aug_mask_cuts(0x3000, (cabi.AugTask * 1)(_task(mask=0x6000, trunc_mode=5)), 1, 0x4000, None) == -1
    assert lib.gdrn_aug_mask_cuts(0x3000, (cabi.AugTask * 1)(_task(mask=0x6000, trunc_mode=1, trunc_u=1.5)), 1, 0x4000, None) == -1
    assert lib.gdrn_aug_mask_cuts(0x3000, host, 1, 0x4000, None) == 0                # no frame has a mask: nothing to launch
    bg = dict(mask=0x6000, bg=0x7000, mask_trunc=0x8000, inv_scale=1.0, bg_h=40, bg_w=50, ch=40, cw=50, oh=40, ow=50)
    for bad in (dict(frame=None), dict(out=None), dict(out=0x1000), dict(H=0), dict(W=-3), dict(blur_r=-1), dict(blur_r=4, H=4), dict(blur_r=2, W=2),
                dict(lut_off=-2), dict(lut_off=4096 - 767), dict(gh=3, gw=3), dict(gh=3, gw=0, keep_off=0), dict(gh=3, gw=3, keep_off=4096 - 8),
                dict(mask_trunc=0x8000), dict(bg, bg=None), dict(bg, ch=41), dict(bg, cw=0), dict(bg, oh=41), dict(bg, ow=-1), dict(bg, inv_scale=0.0),
                dict(bg, inv_scale=float("nan")), dict(bg, trunc_mode=-1)):
        assert _frames_status(lib, _task(**bad)) == -1, bad
    assert _frames_status(lib, _task(**bg), cuts=None) == -1                         # a mask needs the cuts
    for big in (dict(blur_r=5), dict(gh=64, gw=65, keep_off=0), dict(gh=4097, gw=1, keep_off=0)):
        assert _frames_status(lib, _task(**big), aux_bytes=8192) == -2, big
