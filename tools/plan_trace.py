"""Launch trace of dry plans: every library call a plan would make, with every argument, as text -- on the CPU, without a GPU.

A dry Engine builds real plans on host tensors.  Here its library handle is replaced by a proxy before the plan is built: the host-only
queries (tile / rows / ok / splits ...) reach the real library, every other entry point is written down as one line and returns 0.  The
ops of plan.eval_prep, plan.fwd and plan.bwd are then called in order.  Pointers are renamed p0, p1, ... by first appearance, so two
builds that bind the same buffers to the same arguments in the same order give the same text whatever the allocator returned.

    python tools/plan_trace.py --out DIR        one text file per configuration of CONFIGS (the grid a plan.py change is diffed over)

Run it on the commit before and on the commit after a change of plan.py / engine.py and `diff -r` the two directories."""
import argparse
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# host-only queries by the end of their name (checked against cabi._SIGS) ...
QUERY = re.compile(r"_(rows|ok|tile|wfrag|splits|waves|bytes|parts|blocks|chunk|version|format)$")
# ... except the two launches that end like one (both take a stream)
LAUNCHES = ("gdrn_pack_wfrag", "gdrn_map_loss_finalize_rows")
CTX_POINTERS = ("img", "coord2d", "extents", "gt_xyz", "mask_visib", "mask_trunc", "gt_region", "cams", "centers", "whs", "ratios", "gt_rot",
                "gt_trans", "gt_trans_ratio", "points", "sym", "sym_count", "loss_w", "weighted")


def is_query(name):
    return bool(QUERY.search(name)) and name not in LAUNCHES


class Recorder:
    """stands in for Engine.lib: queries pass through, launches become lines of `self.lines`"""

    def __init__(self, lib):
        self._lib, self.lines, self.names, self._ids = lib, [], [], {}

    def pid(self, v):
        return "0" if not v else "p%d" % self._ids.setdefault(int(v), len(self._ids))

    def struct(self, s):
        return type(s).__name__ + "(" + ",".join(f"{f}={self.pid(getattr(s, f)) if t is C.c_void_p else getattr(s, f)}" for f, t in s._fields_) + ")"

    def value(self, a, t):
        if t is C.c_void_p:
            return self.pid(a)
        s = getattr(a, "_obj", None)   # C.byref(struct)
        return self.struct(s) if isinstance(s, C.Structure) else repr(a)

    def __getattr__(self, name):
        from gdrnet_amd import cabi

        if is_query(name):
            return getattr(self._lib, name)
        types = cabi._SIGS[name]

        def call(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            self.names.append(name)
            self.lines.append(name + " " + " ".join(self.value(a, t) for a, t in zip(args, types)))
            return 0

        return call


def _clean_env(env):
    """the environment of one configuration: no GDRN_* switch but the given ones.  Returns what to restore."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("GDRN_") and k not in ("GDRN_HIP_LIB", "GDRN_HIP_LIB_F16")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    return saved


def trace(dtype="bf16", B=4, bn_train=True, with_loss=True, env=None):
    """NS(text, ops, names): the trace, [(list name, index, entry points the op called)] and every recorded entry point in order."""
    import torch
    from gdrnet_amd import GDRN, cabi
    from gdrnet_amd.cfg import lm13_cfg
    from gdrnet_amd.engine import Engine

    env = dict(env or {})
    saved = _clean_env(env)
    to_table = cabi.to_device_table
    try:
        torch.manual_seed(0)
        model, _ = GDRN.build_model_optimizer(lm13_cfg(device="cpu"))
        e = Engine(dict(model.named_parameters()), dict(model.named_buffers()), dtype=dtype, dry=True)
        rec = e.lib = Recorder(e.lib)
        e._stream = lambda: 0   # (eval_refresh asks for the current stream)

        def table(structs, device):
            rec.lines.append(f"table {type(structs[0]).__name__} x{len(structs)}")
            rec.lines += ["  " + rec.struct(s) for s in structs]
            return to_table(structs, device)

        cabi.to_device_table = table
        p = e.plan(B, bn_train, with_loss)
        ctx = {n: 0x7000000000 + 4096 * i for i, n in enumerate(CTX_POINTERS)}
        ctx.update(npts=3000, Kmax=2)
        ops = []
        for nm, lst in (("prep", p.eval_prep), ("fwd", p.fwd), ("bwd", p.bwd)):
            for i, op in enumerate(lst):
                side = bool(getattr(op, "side", False))
                rec.lines.append(f"-- {nm}[{i}] side={side} defer={bool(getattr(op, 'defer', False))} seed={bool(getattr(op, 'seed', False))} "
                                 f"parts={len(getattr(op, 'parts', ()))} meta={getattr(op, 'meta', None)}")
                n0 = len(rec.names)
                op(1 if side else 0, ctx)
                ops.append((nm, i, rec.names[n0:]))
        rec.lines.append("-- keep")
        for k in p.keep:
            rec.lines.append(f"{tuple(k.shape)} {k.dtype} {rec.pid(k.data_ptr())}" if isinstance(k, torch.Tensor) else rec.struct(k))
        rec.lines.append("-- tensors")
        rec.lines += [f"{n} {rec.pid(t.data_ptr())}" for n, t in p.tensors.items()]
        rec.lines.append(f"-- grad_group {p.grad_group}")
        rec.lines.append(f"-- bucket_marks {p._bucket_marks() if p.has_backward else None}")
        rec.lines.append("-- wfmt " + " ".join(f"{k}={L.wfmt}" for k, L in e.layers.items()))
        return NS(text="\n".join(rec.lines) + "\n", ops=ops, names=rec.names)
    finally:
        cabi.to_device_table = to_table
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def _configs():
    """[(file name, dtype, B, bn_train, with_loss, env)]: the base grid (odd batch | either side of halo_min_b in fp32 | above the split-K
    bound) and one variant per environment switch of the engine"""
    out = []
    for dtype in ("bf16", "fp16", "fp32"):
        for B in (3, 4, 64, 96):
            for tr, wl in ((True, True), (False, False), (False, True), (True, False)):
                out.append((f"{dtype}_b{B}_{'T' if tr else 'F'}{'T' if wl else 'F'}", dtype, B, tr, wl, {}))
    var = [("GDRN_V3", "0"), ("GDRN_V3", "2")] + [(k, "0") for k in ("GDRN_FUSE_XF", "GDRN_GEMM_BNB", "GDRN_FUSE_UP", "GDRN_FC_TAIL")]
    var += [("GDRN_WGRAD_STREAM", "0"), ("GDRN_WGRAD_STREAM", "serial"), ("GDRN_BUCKETS", "5"), ("GDRN_HALO_WAVES", "4"), ("GDRN_HALO_WAVES", "8")]
    out += [(f"bf16_b64_TT_{k}={v}", "bf16", 64, True, True, {k: v}) for k, v in var]
    out += [(f"fp32_b64_TT_GDRN_HALO_F32={v}", "fp32", 64, True, True, {"GDRN_HALO_F32": v}) for v in ("0", "1")]
    return out


CONFIGS = _configs()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True, help="directory for one <configuration>.txt each")
    ap.add_argument("--only", default="", help="regular expression over the configuration names")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name, dtype, B, tr, wl, env in CONFIGS:
        if a.only and not re.search(a.only, name):
            continue
        try:
            text = trace(dtype, B, tr, wl, env).text
        except Exception as ex:   # a configuration that cannot be built: the message is its record
            text = f"raised {type(ex).__name__}: {ex}\n"
        with open(os.path.join(a.out, name + ".txt"), "w") as f:
            f.write(text)
        print(f"{name}: {len(text.splitlines())} lines", flush=True)


if __name__ == "__main__":
    main()
