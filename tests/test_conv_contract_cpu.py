"""Host contract of the stride-1 3x3 halo convs (csrc/conv3x3_halo.hip, csrc/conv3x3_v3.hip), without a device: the four layout / tile queries
on every stride-1 3x3 layer shape of the network and on the edge shapes, and the status with which the launch entry point gdrn_conv3x3_halo
refuses a bad gdrn_conv_params -- one row per `return GDRN_ERR_*` of gdrn_conv3x3_halo and of gdrn_v3_launch (reached through w_frag = 2),
plus rows that break two rules at once, where the order of the checks decides between GDRN_ERR_ARG and GDRN_ERR_SHAPE.  Every expected
value is a literal.  Both library builds (bf16 and IEEE half) are checked: their host code is the same source."""
import ctypes as C

import pytest
import torch

from gdrnet_amd import cabi

ARG, SHAPE = -1, -2
FAKE = 16   # a refused call returns before any HIP call: the pointers are never dereferenced
PTRS = ("x", "w", "y", "bias", "addend", "stats", "bnb_x", "bnb_mask", "bnb_mean", "bnb_invstd", "bnb_scale", "bnb_shift", "bnb_rows",
        "xf_x2", "xf_a", "xf_b", "xf_c", "xf_c2", "xf_msc", "xf_msh", "xf_out")


def cp(dt, H, W, Cin, Cout, B, /, **kw):
    """stride-1 pad-1 3x3 conv of B images of H x W, dense channel strides, in the library's 16-bit type (dtype="f32": fp32); kw overrides any
    field afterwards; a pointer field given as True becomes a non-null fake pointer"""
    p = cabi.ConvParams()
    p.Hi, p.Wi, p.Ho, p.Wo = H, W, H, W
    p.Cin = p.x_cs = Cin
    p.Cout = p.y_cs = p.w_rows = Cout
    p.KH = p.KW = 3
    p.stride, p.pad = 1, 1
    p.M, p.dtype = B * H * W, dt
    for k, v in kw.items():
        if k in PTRS:
            v = FAKE if v else None
        elif k == "dtype":
            v = {"f32": cabi.F32, "other": cabi.F16 if dt == cabi.BF16 else cabi.BF16}.get(v, v)
        setattr(p, k, v)
    return p


def query(lib, p):
    """(wfrag under policy 0, 1, 2 | halo tile | v3 tile | halo waves | stats rows of the halo kernel, of the v3 kernel)"""
    out = []
    for pol in (0, 1, 2):
        p.w_frag = pol
        out.append(lib.gdrn_conv3x3_wfrag(C.byref(p)))
    for wf in (1, 2):
        p.w_frag = wf
        th, tw, bn = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        assert lib.gdrn_conv3x3_tile(C.byref(p), C.byref(th), C.byref(tw), C.byref(bn)) == 0
        out.append((th.value, tw.value, bn.value))
    p.w_frag = 1
    out.append(lib.gdrn_conv3x3_halo_waves(C.byref(p)))
    out.append(lib.gdrn_conv3x3_stats_rows(C.byref(p)))
    p.w_frag = 2
    assert lib.gdrn_conv3x3_halo_waves(C.byref(p)) == 0
    out.append(lib.gdrn_conv3x3_stats_rows(C.byref(p)))
    return tuple(out)


NO = (0, 0, 0)
# (H, W, Cin, Cout, B, overrides) -> query(): the stride-1 3x3 layers of the network (ResNet-34 layer1..4: 64 ch at 64 x 64 ... 512 ch at 8 x 8;
# head: 256 ch at 32 x 32 and 64 x 64; tools/plan_trace.py) at batch 4 and 64, plain (xf_mode 0) and with an operand transform (xf_mode 1)
QUERY_ROWS = [
    (64, 64, 64, 64, 4, {}, (1, 1, 1, (8, 16, 64), NO, 4, 128, -2)),
    (64, 64, 64, 64, 4, dict(xf_mode=1), (1, 1, 1, (8, 16, 64), NO, 4, 128, -2)),
    (32, 32, 128, 128, 4, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 32, 32)),
    (32, 32, 128, 128, 4, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 32, 32)),
    (16, 16, 256, 256, 4, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 8, 8)),
    (16, 16, 256, 256, 4, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 8, 8)),
    (8, 8, 512, 512, 4, {}, (1, 1, 1, (8, 8, 128), NO, 8, 4, -2)),
    (8, 8, 512, 512, 4, dict(xf_mode=1), (1, 1, 1, (8, 8, 128), NO, 8, 4, -2)),
    (32, 32, 256, 256, 4, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 32, 32)),
    (32, 32, 256, 256, 4, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 32, 32)),
    (64, 64, 256, 256, 4, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 128, 128)),
    (64, 64, 256, 256, 4, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 128, 128)),
    (64, 64, 64, 64, 64, {}, (1, 1, 1, (8, 16, 64), NO, 4, 2048, -2)),
    (64, 64, 64, 64, 64, dict(xf_mode=1), (1, 1, 1, (8, 16, 64), NO, 4, 2048, -2)),
    (32, 32, 128, 128, 64, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 128, 128, 64, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (16, 16, 256, 256, 64, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 128, 128)),
    (16, 16, 256, 256, 64, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 128, 128)),
    (8, 8, 512, 512, 64, {}, (1, 1, 1, (8, 8, 128), NO, 8, 64, -2)),
    (8, 8, 512, 512, 64, dict(xf_mode=1), (1, 1, 1, (8, 8, 128), NO, 8, 64, -2)),
    (32, 32, 256, 256, 64, {}, (1, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    (32, 32, 256, 256, 64, dict(xf_mode=1), (2, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    (64, 64, 256, 256, 64, {}, (1, 1, 2, (8, 16, 128), (16, 16, 256), 4, 2048, 1024)),
    (64, 64, 256, 256, 64, dict(xf_mode=1), (2, 1, 2, (8, 16, 128), (16, 16, 256), 4, 2048, 1024)),
    # H or W no multiple of 8
    (12, 16, 128, 128, 4, {}, (0, 0, 0, NO, NO, 0, -2, -2)),
    (16, 12, 128, 128, 4, {}, (0, 0, 0, NO, NO, 0, -2, -2)),
    (20, 20, 256, 256, 64, dict(xf_mode=1), (0, 0, 0, NO, NO, 0, -2, -2)),
    # W = 8 against W = 16 (pixel tile 8 x 8 / 8 x 16; the v3 kernel needs 16)
    (16, 8, 128, 128, 4, {}, (1, 1, 1, (8, 8, 128), NO, 8, 8, -2)),
    (16, 16, 128, 128, 4, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 8, 8)),
    (24, 16, 256, 256, 64, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 192, 192)),
    (8, 16, 256, 256, 64, dict(xf_mode=1, v3_min_wg=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 64, 64)),
    # Cout 64, 72, 128, 192, 256 (channel tile 64 up to 64 channels, 128 beyond; the v3 kernel: whole 128-channel tiles)
    (16, 16, 64, 64, 4, dict(xf_mode=1, v3_min_wg=1), (1, 1, 1, (8, 16, 64), NO, 4, 8, -2)),
    (16, 16, 64, 72, 4, dict(xf_mode=1, v3_min_wg=1), (1, 1, 1, (8, 16, 128), NO, 8, 8, -2)),
    (16, 16, 64, 128, 4, dict(xf_mode=1, v3_min_wg=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 8, 8)),
    (16, 16, 64, 192, 4, dict(xf_mode=1, v3_min_wg=1), (1, 1, 1, (8, 16, 128), NO, 8, 8, -2)),
    (16, 16, 64, 256, 4, dict(xf_mode=1, v3_min_wg=1), (2, 1, 2, (8, 16, 128), (16, 16, 256), 8, 8, 4)),
    # fp32: always 8 x 8 x 64, never the v3 kernel, never eight waves
    (16, 16, 64, 64, 4, dict(dtype='f32'), (1, 1, 1, (8, 8, 64), NO, 4, 16, -2)),
    (32, 32, 128, 128, 4, dict(dtype='f32'), (1, 1, 1, (8, 8, 64), NO, 4, 64, -2)),
    (16, 16, 256, 256, 64, dict(dtype='f32'), (1, 1, 1, (8, 8, 64), NO, 4, 256, -2)),
    # v3_min_wg 0 against 1: the 256-channel tile on a grid of 8 workgroups
    (16, 16, 256, 256, 4, dict(xf_mode=1), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 8, 8)),
    (16, 16, 256, 256, 4, dict(xf_mode=1, v3_min_wg=1), (2, 1, 2, (8, 16, 128), (16, 16, 256), 8, 8, 4)),
    (32, 32, 256, 256, 64, dict(xf_mode=1, v3_min_wg=2048), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 256, 256, 64, dict(xf_mode=1, v3_min_wg=128), (2, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    # an addend or a stored ReLU mask blocks the 256-channel tile
    (32, 32, 256, 256, 64, dict(xf_mode=1, addend=True, add_cs=256), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 256, 256, 64, dict(xf_mode=1, bnb_mask=True), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 256, 256, 64, dict(xf_mode=3, bnb_x=True), (2, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    # LDS limit: two inputs (xf_mode >= 2) of 512 channels do not fit the 256-channel tile
    (32, 32, 512, 512, 64, dict(xf_mode=0), (1, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    (32, 32, 512, 512, 64, dict(xf_mode=1), (2, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    (32, 32, 512, 512, 64, dict(xf_mode=2), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 512, 512, 64, dict(xf_mode=3), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 512, 512, 64, dict(xf_mode=4), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 512, 512)),
    (32, 32, 256, 512, 64, dict(xf_mode=2), (2, 1, 2, (8, 16, 128), (16, 16, 256), 4, 512, 256)),
    # the halo kernel's eight-wave form: 16-bit, 128-channel tile, grids of <= 256 workgroups unless halo_waves says 4 or 8
    (16, 16, 256, 256, 64, dict(halo_waves=4), (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 128, 128)),
    (32, 32, 128, 128, 64, dict(halo_waves=8), (1, 1, 2, (8, 16, 128), (8, 16, 128), 8, 512, 512)),
    (16, 16, 256, 256, 65, {}, (1, 1, 2, (8, 16, 128), (8, 16, 128), 4, 130, 130)),
    (16, 16, 64, 64, 4, dict(halo_waves=8), (1, 1, 1, (8, 16, 64), NO, 4, 8, -2)),
    # not a stride-1 pad-1 3x3 conv
    (16, 16, 256, 256, 4, dict(stride=2), (0, 0, 0, NO, NO, 0, -2, -2)),
    (16, 16, 256, 256, 4, dict(KW=1), (0, 0, 0, NO, NO, 0, -2, -2)),
    (16, 16, 256, 256, 4, dict(pad=0), (0, 0, 0, NO, NO, 0, -2, -2)),
    (16, 16, 256, 256, 4, dict(mode=1), (0, 0, 0, NO, NO, 0, -2, -2)),
    (16, 16, 256, 256, 4, dict(Wi=18), (0, 0, 0, NO, NO, 0, -2, -2)),
    (16, 16, 256, 256, 4, dict(dtype=7), (0, 0, 0, NO, NO, 0, -2, -2)),
    # what the v3 kernel refuses and the halo kernel takes
    (16, 16, 256, 256, 4, dict(act=2), (1, 1, 1, (8, 16, 128), NO, 8, 8, -2)),
    (16, 16, 256, 256, 4, dict(out_f32=1), (1, 1, 1, (8, 16, 128), NO, 8, 8, -2)),
    (16, 16, 96, 256, 4, dict(x_cs=128), (1, 1, 1, (8, 16, 128), NO, 8, 8, -2)),
]


@pytest.mark.parametrize("dt", [cabi.BF16, cabi.F16])
def test_queries_on_the_network_shapes_and_the_edge_shapes(dt):
    lib = cabi.load(dt)
    for H, W, Cin, Cout, B, kw, want in QUERY_ROWS:
        assert query(lib, cp(dt, H, W, Cin, Cout, B, **kw)) == want, (H, W, Cin, Cout, B, kw)
    p = cp(dt, 16, 16, 256, 256, 4)
    assert lib.gdrn_conv3x3_wfrag(None) == ARG and lib.gdrn_conv3x3_halo_waves(None) == 0
    assert lib.gdrn_conv3x3_tile(C.byref(p), None, None, None) == ARG
    for bad in (-1, 3):
        p.w_frag = bad
        assert lib.gdrn_conv3x3_wfrag(C.byref(p)) == ARG


IO = dict(x=True, w=True, y=True)
BNB = dict(bnb_x=True, bnb_mean=True, bnb_invstd=True, bnb_rows=True, bnb_cs=256)
BIG = 4096   # images of 16 x 16: M = 2^20 pixels, a channel stride of 1024 (2048) elements x 4 (2) bytes reaches 2^32
# base launch: 4 images of 16 x 16 x 256 -> 256 channels; halo kernel (w_frag 1): tile 8 x 16 x 128; v3 (w_frag 2): tile 8 x 16 x 128 (cfg 2)
HALO_REFUSALS = [
    # --- gdrn_conv3x3_halo
    (dict(w_frag=1, w=True, y=True), ARG),                                  # !pp->x
    (dict(w_frag=1, x=True, y=True), ARG),                                  # !pp->w
    (dict(w_frag=1, x=True, w=True), ARG),                                  # !pp->y
    (dict(w_frag=1, **IO, dtype="other"), ARG),                             # dtype: the other build's 16-bit code
    (dict(w_frag=1, **IO, dtype=7), ARG),                                   # dtype: no code at all
    (dict(w_frag=1, **IO, Ho=12, Hi=12), SHAPE),                            # th == 0: Ho % 8
    (dict(w_frag=1, **IO, stride=2), SHAPE),                                # th == 0: stride
    (dict(w_frag=1, **IO, KH=1), SHAPE),                                    # th == 0: KH
    (dict(w_frag=1, **IO, mode=1), SHAPE),                                  # th == 0: mode
    (dict(w_frag=1, **IO, Hi=18), SHAPE),                                   # th == 0: Hi != Ho
    (dict(w_frag=1, **IO, Cin=0), SHAPE),                                   # Cin <= 0
    (dict(w_frag=1, **IO, Cin=32), SHAPE),                                  # Cin * esz % 128
    (dict(w_frag=1, **IO, x_cs=260), SHAPE),                                # x_cs * esz % 16
    (dict(w_frag=1, **IO, Cout=0), SHAPE),                                  # Cout <= 0
    (dict(w_frag=1, **IO, y_cs=258), SHAPE),                                # y_cs & 3
    (dict(w_frag=1, **IO, y_cs=260), SHAPE),                                # 128-channel tile: y_cs & 7
    (dict(w_frag=1, **IO, addend=True, add_cs=260), SHAPE),                 # 128-channel tile: add_cs & 7
    (dict(w_frag=1, **IO, **{**BNB, "bnb_cs": 260}), SHAPE),                # 128-channel tile: bnb_cs & 7
    (dict(w_frag=1, **IO, M=0), SHAPE),                                     # M <= 0
    (dict(w_frag=1, **IO, M=4 * 256 + 1), SHAPE),                           # M % (Ho * Wo)
    (dict(w_frag=1, **IO, w_rows=128), SHAPE),                              # w_rows < whole channel tiles
    (dict(w_frag=1, **IO, Cout=192, w_rows=192), SHAPE),                    # w_rows < whole channel tiles (192 -> 256 rows)
    (dict(w_frag=1, **IO, Cout=64, addend=True, add_cs=66), SHAPE),         # 64-channel tile: add_cs & 3
    (dict(w_frag=3, **IO), ARG),                                            # w_frag > 2
    (dict(w_frag=-1, **IO), ARG),                                           # w_frag < 0
    (dict(w_frag=1, **IO, halo_waves=5), ARG),                              # halo_waves not 0 / 4 / 8
    (dict(w_frag=1, **IO, **{**BNB, "bnb_mean": False}), ARG),              # bnb: no mean
    (dict(w_frag=1, **IO, **{**BNB, "bnb_invstd": False}), ARG),            # bnb: no invstd
    (dict(w_frag=1, **IO, **{**BNB, "bnb_rows": False}), ARG),              # bnb: no rows
    (dict(w_frag=1, **IO, **BNB, bnb_scale=True), ARG),                     # bnb: scale without shift
    (dict(w_frag=1, **IO, **BNB, bnb_shift=True), ARG),                     # bnb: shift without scale
    (dict(w_frag=1, **IO, **BNB, bias=True), SHAPE),                        # bnb: bias
    (dict(w_frag=1, **IO, **BNB, act=1), SHAPE),                            # bnb: act
    (dict(w_frag=1, **IO, **BNB, out_f32=1), SHAPE),                        # bnb: out_f32
    (dict(w_frag=1, **IO, **BNB, Cout=192, w_rows=256), SHAPE),             # bnb: Cout % bn
    (dict(w_frag=1, **IO, **{**BNB, "bnb_cs": 66}, Cout=64), SHAPE),        # bnb: bnb_cs & 3 (64-channel tile)
    (dict(w_frag=1, **IO, **{**BNB, "bnb_cs": 128}), SHAPE),                # bnb: bnb_cs < Cout
    (dict(w_frag=1, **IO, **{**BNB, "bnb_cs": 1024}, M=BIG * 256), SHAPE),  # bnb: M * bnb_cs * 4 >= 2^32
    (dict(w_frag=1, **IO, y_cs=1024, M=BIG * 256), SHAPE),                  # M * y_cs * 4 >= 2^32
    (dict(w_frag=1, **IO, addend=True, add_cs=1024, M=BIG * 256), SHAPE),   # M * add_cs * 4 >= 2^32
    (dict(w_frag=1, **IO, x_cs=2048, M=BIG * 256), SHAPE),                  # M * x_cs * esz >= 2^32
    (dict(w_frag=1, **IO, dtype="f32", xf_mode=1, xf_c=True), ARG),         # fp32 with an operand transform
    (dict(w_frag=1, **IO, dtype="f32", **BNB), ARG),                        # fp32 with the BatchNorm-backward epilogue
    (dict(w_frag=1, **IO, xf_mode=5, xf_c=True), ARG),                      # xf_mode > 4
    (dict(w_frag=1, **IO, xf_mode=-1, xf_c=True), ARG),                     # xf_mode < 0
    (dict(w_frag=1, **IO, xf_mode=1), ARG),                                 # xf: no xf_c
    (dict(w_frag=1, **IO, xf_mode=1, xf_c=True, Cin=576, x_cs=576), ARG),   # xf: Cin > 512
    (dict(w_frag=1, **IO, xf_mode=2, xf_c=True), ARG),                      # xf mode 2: no xf_x2
    (dict(w_frag=1, **IO, xf_mode=3, xf_c=True), ARG),                      # xf mode 3: no xf_x2
    (dict(w_frag=1, **IO, xf_mode=4, xf_c=True, xf_x2=True, xf_msh=True), ARG),   # xf mode 4: no xf_msc
    (dict(w_frag=1, **IO, xf_mode=4, xf_c=True, xf_x2=True, xf_msc=True), ARG),   # xf mode 4: no xf_msh
    (dict(w_frag=1, **IO, xf_mode=1, xf_c=True, xf_c2=True), ARG),          # xf_c2 outside mode 2
    (dict(w_frag=1, **IO, xf_mode=3, xf_c=True, xf_x2=True, xf_c2=True), ARG),    # xf_c2 outside mode 2
    # --- gdrn_v3_launch (w_frag = 2)
    (dict(w_frag=2, **IO, dtype="f32"), SHAPE),                             # cfg == 0: fp32
    (dict(w_frag=2, **IO, Cin=32, x_cs=32), SHAPE),                         # cfg == 0: Cin % 64
    (dict(w_frag=2, **IO, Cout=64, w_rows=64), SHAPE),                      # cfg == 0: Cout % 128
    (dict(w_frag=2, **IO, Wo=8, Wi=8, M=4 * 128), SHAPE),                   # cfg == 0: Wo % 16
    (dict(w_frag=2, **IO, Ho=12, Hi=12, M=4 * 192), SHAPE),                 # cfg == 0: Ho % 8
    (dict(w_frag=2, **IO, act=2), SHAPE),                                   # cfg == 0: act > 1
    (dict(w_frag=2, **IO, out_f32=1), SHAPE),                               # cfg == 0: out_f32
    (dict(w_frag=2, **IO, stride=2), SHAPE),                                # cfg == 0: stride
    (dict(w_frag=2, **IO, x_cs=260), SHAPE),                                # x_cs & 7
    (dict(w_frag=2, **IO, y_cs=260), SHAPE),                                # y_cs & 7
    (dict(w_frag=2, **IO, addend=True, add_cs=260), SHAPE),                 # add_cs & 7
    (dict(w_frag=2, **IO, **{**BNB, "bnb_cs": 260}), SHAPE),                # bnb_cs & 7
    (dict(w_frag=2, **IO, w_rows=192), SHAPE),                              # w_rows < Cout
    (dict(w_frag=2, **IO, w_rows=288), SHAPE),                              # w_rows & 63
    (dict(w_frag=2, **IO, M=0), SHAPE),                                     # M <= 0
    (dict(w_frag=2, **IO, M=4 * 256 + 16), SHAPE),                          # M % (Ho * Wo)
    (dict(w_frag=2, **IO, **{**BNB, "bnb_mean": False}), ARG),              # bnb: no mean
    (dict(w_frag=2, **IO, **{**BNB, "bnb_invstd": False}), ARG),            # bnb: no invstd
    (dict(w_frag=2, **IO, **{**BNB, "bnb_rows": False}), ARG),              # bnb: no rows
    (dict(w_frag=2, **IO, **BNB, bnb_scale=True), ARG),                     # bnb: scale without shift
    (dict(w_frag=2, **IO, **BNB, bias=True), SHAPE),                        # bnb: bias
    (dict(w_frag=2, **IO, **BNB, act=1), SHAPE),                            # bnb: act
    (dict(w_frag=2, **IO, **{**BNB, "bnb_cs": 128}), SHAPE),                # bnb: bnb_cs < Cout
    (dict(w_frag=2, **IO, **{**BNB, "bnb_cs": 2048}, M=BIG * 256), SHAPE),  # bnb: M * bnb_cs * 2 >= 2^32
    (dict(w_frag=2, **IO, y_cs=2048, M=BIG * 256), SHAPE),                  # M * y_cs * 2 >= 2^32
    (dict(w_frag=2, **IO, addend=True, add_cs=2048, M=BIG * 256), SHAPE),   # M * add_cs * 2 >= 2^32
    (dict(w_frag=2, **IO, x_cs=2048, M=BIG * 256), SHAPE),                  # M * x_cs * 2 >= 2^32
    (dict(w_frag=2, **IO, xf_mode=5, xf_c=True), ARG),                      # xf_mode > 4
    (dict(w_frag=2, **IO, xf_mode=1), ARG),                                 # xf: no xf_c
    (dict(w_frag=2, **IO, xf_mode=1, xf_c=True, Cin=576, x_cs=576), ARG),   # xf: Cin > 512
    (dict(w_frag=2, **IO, xf_mode=2, xf_c=True), ARG),                      # xf mode 2: no xf_x2
    (dict(w_frag=2, **IO, xf_mode=4, xf_c=True, xf_x2=True, xf_msh=True), ARG),   # xf mode 4: no xf_msc
    (dict(w_frag=2, **IO, xf_mode=4, xf_c=True, xf_x2=True, xf_msc=True), ARG),   # xf mode 4: no xf_msh
    (dict(w_frag=2, **IO, xf_mode=3, xf_c=True, xf_x2=True, xf_c2=True), ARG),    # xf_c2 outside mode 2
    # --- two rules broken at once: the order of the checks decides the code
    (dict(w_frag=1, **IO, halo_waves=5, M=4 * 256 + 1), SHAPE),             # halo: M % hw (SHAPE) stands before halo_waves (ARG)
    (dict(w_frag=3, **IO, w_rows=128), SHAPE),                              # halo: w_rows (SHAPE) before the w_frag range (ARG)
    (dict(w_frag=1, **IO, halo_waves=5, **BNB, bias=True), ARG),            # halo: halo_waves (ARG) before the bnb shape rules (SHAPE)
    (dict(w_frag=1, **IO, **{**BNB, "bnb_mean": False}, y_cs=1024, M=BIG * 256), ARG),   # halo: bnb pointers (ARG) before the y offsets (SHAPE)
    (dict(w_frag=1, **IO, **{**BNB, "bnb_rows": False}, bias=True), ARG),   # halo: bnb pointers (ARG) before the bnb shape rules (SHAPE)
    (dict(w_frag=1, **IO, dtype="f32", xf_mode=1, xf_c=True, x_cs=1024, M=BIG * 256), SHAPE),   # halo: x offsets (SHAPE) before fp32 + xf (ARG)
    (dict(w_frag=1, **IO, xf_mode=1, x_cs=2048, M=BIG * 256), SHAPE),       # halo: x offsets (SHAPE) before the xf pointers (ARG)
    (dict(w_frag=1, **IO, dtype="other", Ho=12, Hi=12), ARG),               # halo: dtype (ARG) before the tile (SHAPE)
    (dict(w_frag=1, w=True, y=True, stride=2), ARG),                        # halo: null x (ARG) before the tile (SHAPE)
    (dict(w_frag=2, **IO, dtype="other"), ARG),                             # dtype (ARG) in the entry point, before v3's config (SHAPE)
    (dict(w_frag=2, **IO, **{**BNB, "bnb_rows": False}, M=4 * 256 + 16), SHAPE),   # v3: M % hw (SHAPE) before the bnb pointers (ARG)
    (dict(w_frag=2, **IO, **{**BNB, "bnb_rows": False}, bias=True), ARG),   # v3: bnb pointers (ARG) before the bnb shape rules (SHAPE)
    (dict(w_frag=2, **IO, xf_mode=1, x_cs=2048, M=BIG * 256), SHAPE),       # v3: x offsets (SHAPE) before the xf pointers (ARG)
    (dict(w_frag=2, **IO, xf_mode=7, w_rows=192), SHAPE),                   # v3: w_rows (SHAPE) before the xf mode (ARG)
]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a refusal that a change broke would launch on fake pointers: run without a device only")
@pytest.mark.parametrize("dt", [cabi.BF16, cabi.F16])
def test_launch_entry_point_refusals(dt):
    lib = cabi.load(dt)
    assert lib.gdrn_conv3x3_halo(None, None) == ARG                         # !pp
    for kw, want in HALO_REFUSALS:
        assert want in (ARG, SHAPE)
        assert lib.gdrn_conv3x3_halo(C.byref(cp(dt, 16, 16, 256, 256, 4, **kw)), None) == want, kw
