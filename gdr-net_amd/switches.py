"""The environment switches of the package: one table (the rows of INTEGRATION.md section 3), one reader."""
# read(name) looks the variable up in os.environ when it is called, so every switch keeps the moment at which it takes effect: library load
# (import of cabi), model construction (GDRN.__init__), engine construction (Engine.__init__), every train step (GDRN.train_step), or bench.py's
# own command line.  A value outside the documented set raises ValueError naming the variable.  What each switch was measured against is in
# DESIGN.md section 4.  This module imports nothing from the package.
import os
from collections import namedtuple

LOAD, MODEL, ENGINE, STEP, BENCH = "library load", "model construction", "engine construction", "every train step", "bench.py"
# accepts: dict documented string -> value that read() returns, or a parser of the string that raises ValueError (the effect names the form)
Switch = namedtuple("Switch", "name default accepts read_at effect")
ON_OFF = {"0": False, "1": True}


def _same(*values):
    return {v: v for v in values}


def _int(v, lo):
    if not v.isdigit() or int(v) < lo:
        raise ValueError(v)
    return int(v)


def _loss_scale(v):
    spec = (v + ":2000").split(":")
    static = spec[1] == "static"
    return float(spec[0]), not static, 0 if static else int(spec[1])   # (scale, dynamic, growth interval)


TABLE = {s.name: s for s in (
    Switch("GDRN_HIP_LIB", None, str, LOAD, "an alternative libgdrn_hip.so (same-box A/B of two builds)"),
    Switch("GDRN_HIP_LIB_F16", None, str, LOAD, "an alternative libgdrn_hip_f16.so"),
    Switch("GDRN_HIP_DTYPE", None, _same("bf16", "fp16", "fp32"), MODEL, "arithmetic when cfg.MODEL.CDPN.HIP_DTYPE is unset (unset: bf16, fp16 under the reference's AMP switches)"),
    Switch("GDRN_LOSS_SCALE", "1024:2000", _loss_scale, ENGINE, "fp16: <initial scale>[:<growth interval> | :static] of the loss scale on dL/dloss, dynamic on the device (GradScaler) or :static"),
    Switch("GDRN_HALO_F32", "auto", _same("auto", "0", "1"), ENGINE, "fp32 3x3 stride-1 convs on the halo tile: plans of >= 32 RoIs | never | every plan"),
    Switch("GDRN_HALO_WAVES", "0", {"0": 0, "4": 4, "8": 8}, ENGINE, "4 / 8 force the four- / eight-wave form of the first halo kernel's 128-channel tile"),
    Switch("GDRN_V3", "", {"": (0, 0), "0": (1, 0), "2": (2, 1)}, ENGINE, "second-generation halo kernel (w_frag policy, v3_min_wg): where measured faster | never | wherever covered"),
    Switch("GDRN_FUSE_XF", "1", ON_OFF, ENGINE, "BatchNorm apply passes inside the consumer halo conv; 0: separate launches"),
    Switch("GDRN_FUSE_UP", "1", ON_OFF, ENGINE, "the head's BatchNorm + ReLU inside the upsampling launch, its backward sums in the adjoint; 0: separate launches"),
    Switch("GDRN_FC_TAIL", "1", ON_OFF, ENGINE, "fc2 finish + fc_r | fc_t + pose decode as one launch, seeded train step; 0: separate launches"),
    Switch("GDRN_GEMM_BNB", "1", ON_OFF, ENGINE, "BatchNorm-backward mask + sums in the generic kernel's epilogue; 0: a reduce pass of its own"),
    Switch("GDRN_WGRAD_STREAM", "1", _same("1", "0", "serial"), ENGINE, "bucket-end work on a second stream | one stream | one stream, the two-stream launch configuration"),
    Switch("GDRN_BUCKETS", None, {"4": 4, "5": 5}, ENGINE, "gradient bucket layout: 4 (one GPU) or 5 (data parallel); unset: by the process group"),
    Switch("GDRN_MAX_PLANS", "8", lambda v: _int(v, 1), ENGINE, "plans (an integer >= 1) kept before the least recently used one is dropped"),
    Switch("GDRN_EARLY_OPT", "1", ON_OFF, STEP, "optimizer update per gradient bucket under the backward pass; 0: behind the whole pass"),
    Switch("GDRN_GRAPH", "0", ON_OFF, STEP, "1: train_step replays forward + backward as one hipGraph"),
    Switch("GDRN_DP_CHECK_STEPS", "2", lambda v: _int(v, 0), STEP, "data-parallel steps (an integer >= 0) on which the ranks compare a parameter checksum"),
    Switch("GDRN_COMM_DTYPE", "fp32", _same("fp32", "bf16"), BENCH, "wire format of the gradient buckets (default of bench.py --comm-dtype)"),
)}


def read(name):
    """the value of switch `name` as the environment holds it NOW (its default when unset; None: unset, no default)"""
    s = TABLE[name]
    raw = os.environ.get(name, s.default)
    if raw is None:
        return None
    try:
        return s.accepts(raw) if callable(s.accepts) else s.accepts[raw]
    except (KeyError, ValueError):
        raise ValueError(f"{name}={raw!r}: {s.effect}" + ("" if callable(s.accepts) else "; one of " + ", ".join(map(repr, s.accepts)))) from None
