"""Plans of the GDR-Net hot-path executor: static buffers + pre-bound C-ABI call lists for one (batch size, train / eval, losses)
configuration of one Engine (engine.py).  `Plan._build` walks the fixed graph once, one stage builder per step -- stem, 16 BasicBlocks,
geometric head, head tail, Patch-PnP, pose decode, losses (core/gdrn_modeling/models/GDRN.py:110-306, resnet_backbone.py:69-80,
cdpn_rot_head_region.py:182-193, conv_pnp_net.py:111-157) -- and appends one closure per kernel launch to `fwd` and, group by group in
reverse, to `bwd`; `run_forward` / `run_backward` replay them on the current HIP stream (and the engine's side stream).
The stage builders bind launches through the launch builders above them, one per kernel family: `_conv` (stride-1 halo kernel | generic kernel),
`_s2` (gdrn_conv3x3s2) and `_s2d` (gdrn_conv3x3s2_dgrad), each returning (op, statistics rows) -- the stride-2 pair None where the library does not
cover the shape --, `_wgrad`, and the BatchNorm glue `_bn_fwd` / `_bn_bwd`.  An op is a plain callable op(stream, ctx) that may carry `meta` (bench.py's
roofline record), `parts` (a conv paired with its BatchNorm-coefficient launch, `_with_coef`), `side` / `defer` / `bucket_end` (stream placement) and `seed`.
tools/plan_trace.py writes every launch of a plan with every argument as text, on the CPU: diff it across a change of this file."""
import ctypes as C
from types import SimpleNamespace as NS

import torch

from . import cabi
from .cabi import ACC_ROWS, PREZEROED, ConvParams, PoseParams, S2Params, S2dParams, WgradParams, check, ptr
from .engine import HEAD_CONVS, RESNET34_LAYERS, RESNET34_PLANES, _ru

F32t = torch.float32


def _launch(fn, what, args, meta=None):
    """a plain launch, one that reads nothing from ctx: fn(*args, stream).  Tensors among args go in as their device pointers, taken once,
    here; the op holds on to the tensors."""
    cargs = tuple(ptr(a) if isinstance(a, torch.Tensor) else a for a in args)

    def run(st, ctx):
        check(fn(*cargs, st), what)

    run.args = args
    if meta is not None:
        run.meta = meta
    return run


def _launch_struct(fn, what, params, meta=None):
    """a launch whose arguments travel in a parameter struct: fn(byref(params), stream).  The plan keeps the struct alive (Plan.keep)."""
    ref = C.byref(params)

    def run(st, ctx):
        s = fn(ref, st)
        if s:
            check(s, what)

    if meta is not None:
        run.meta = meta
    return run


def _bnb(key, raw, mask=None, affine=False):
    """the BatchNorm(+ReLU) whose output gradient a data-gradient launch writes: the launch's epilogue masks the gradient and reduces that
    BatchNorm's backward sums.  key: of the BatchNorm, raw: its input, mask: the stored activation the ReLU mask is read from, or None with
    affine=True: the mask is recomputed from raw * scale + shift (BatchNorm -> ReLU without a residual)"""
    return NS(key=key, raw=raw, mask=mask, affine=affine)


def _xf_bn_relu(s, **kw):
    """operand transform (xf of Plan._conv) of a conv that applies BatchNorm s + ReLU to its input on load"""
    return dict(mode=1, a=s.scale, c=s.shift, relu=True, **kw)


def _pend(x1, xf):
    """an activation that is not materialised yet: v(x1) of the transform xf, evaluated (and written out) by the conv that consumes it"""
    return NS(x1=x1, xf=xf)


def _probed(op, sink):
    """op wrapped in a pair of timing events recorded on the stream it is launched on (bench.py's in-step roofline bracket)"""
    def run(st, ctx):
        s = torch.cuda.ExternalStream(st) if st else torch.cuda.default_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        parts = getattr(op, "parts", None)   # conv launch + the BatchNorm-coefficient launch behind it: the conv alone is bracketed
        a.record(s)
        (parts[0] if parts else op)(st, ctx)
        b.record(s)
        if parts:
            parts[1](st, ctx)
        sink.append((a, b, op.meta, bool(getattr(op, "side", False))))
    run.side = getattr(op, "side", False)
    return run


class Plan:
    """Static buffers + pre-bound call lists for one (batch size, train/eval) configuration."""

    def __init__(self, eng, B, bn_train, with_loss):
        self.e = eng
        self.B = B
        self.bn_train = bn_train
        self.with_loss = with_loss
        self.has_backward = bn_train and with_loss
        self.fwd = []          # callables f(stream, ctx)
        self.bwd_groups = []   # list of lists, appended in forward order, executed reversed
        self.keep = []         # keep ctypes structs alive
        self.bn = {}           # bn key -> NS(mean, invstd, scale, shift, sums)
        self.eval_prep = []        # eval-mode BN scale/shift launches (run when parameters / running stats changed)
        self._fold_hooked = False
        self._eval_sig = None
        self._unpack_pending = []  # (forward group index, layer)
        self._wreduce = {}         # layer key -> (workspace, nsplit, Cout, Cin) of the halo weight-gradient partials
        self._wgrad_deferred = []  # (forward group index, layer, WgradParams, flops) of the halo weight gradients
        self.tensors = {}          # name -> activation / gradient buffer (inspection by the tests)
        self._zero_regions = []    # fp32 tensors the backward accumulates into with atomics: cleared by ONE gdrn_zero_multi launch
        self.generation = 0        # bumped by every run_forward: a backward checks its activations are still the plan's
        self.head_valid = True     # plan.head_out holds the logits of the last forward (False: inference without cfg.TEST.USE_PNP skipped them)
        self.grad_group = {}       # parameter name -> forward index of the backward group that completes its gradient
        self.acc_rows, self.acc, self.losses, self.pose_rows = 0, None, None, None   # map- / pose-loss partial rows and the 8 losses (plans with losses)
        self.fc_tail = self._fc2 = None   # (fc2 workspace, splits), (f2, fc2 bias, fc_rt layer): fc2's finish pass inside the pose launch
        self.op_events = None      # bench.py: a list here makes run_backward bracket its conv launches with timing events
        self._front_n = 0          # bucket-end ops placed in FRONT of the stem group (see _bucket_end)
        self._marks = None         # _bucket_marks(), computed once
        self._build()
        if self.has_backward:
            self._finish_unpack()
            self._build_zero_table()
        self.bwd_groups = [[op for op in g if op is not None] for g in self.bwd_groups]
        if self.has_backward:
            self._merge_forks()
        self.bwd = [op for g in reversed(self.bwd_groups) for op in g]

    # ---- op builders -------------------------------------------------------------------------
    def _E(self, *shape, dtype=None):
        """a plan buffer, pinned in self.keep: the pre-bound C structs hold RAW device pointers, so a buffer referenced only through them
        would otherwise be returned to the caching allocator when the plan is built and be handed out again while the kernels still
        write to it"""
        t = self.e._empty(*shape, dtype=dtype)
        self.keep.append(t)
        return t

    def _hook_fold(self):
        """the first folded BatchNorm of an eval plan puts Engine.eval_refresh in front of the plan's eval-mode preparation"""
        if not self._fold_hooked:
            self.eval_prep.append(lambda st, ctx: self.e.eval_refresh())
            self._fold_hooked = True

    def _macs(self, L, npix):
        """true (unpadded) multiply-adds of layer L, whichever of its three products a launch computes.  npix: pixels per image of the smaller of
        its two maps -- the output of a conv (also of the 7x7 stem and of fc1, a conv onto one pixel), the input of the ConvTranspose
        (Hin*Win*Cin*Cout*k^2)"""
        return self.B * npix * L.O * L.I * L.KK

    @staticmethod
    def _meta(kernel, macs, nbytes, layer):
        """an op's record for the roofline measurement in bench.py: kernel instantiation, algorithmic FLOPs and bytes (SURVEY 8(d) convention:
        activations in + out once, weights once, at the storage width)"""
        return dict(kernel=kernel, flops=2.0 * macs, bytes=float(nbytes), layer=layer)

    def _fill_bnb(self, p, bnb):
        """the BatchNorm-backward epilogue fields of a ConvParams / S2Params / S2dParams from a _bnb record"""
        sb = self.bn[bnb.key]
        p.bnb_x, p.bnb_mask, p.bnb_cs = ptr(bnb.raw), ptr(bnb.mask), bnb.raw.shape[-1]
        p.bnb_mean, p.bnb_invstd, p.bnb_rows = ptr(sb.mean), ptr(sb.invstd), ptr(self.stats)  # stats scratch is idle in backward
        if bnb.affine:
            assert hasattr(p, "bnb_scale"), type(p).__name__
            p.bnb_scale, p.bnb_shift = ptr(sb.scale), ptr(sb.shift)

    def _with_coef(self, conv, bnkey, nrows):
        """conv: a data-gradient launch whose epilogue left nrows rows of BatchNorm bnkey's backward sums in self.stats.  Returns the pair (conv,
        coefficient launch): rows -> that BatchNorm's backward coefficients (+ dgamma / dbeta), for its apply pass or for the conv that applies
        them on load"""
        assert 0 < nrows and nrows * 2 * self.bn[bnkey].C <= self.stats.numel(), (bnkey, nrows)
        coef = self._bn_coef_op(bnkey, self.stats, nrows)

        def run(st, ctx):
            conv(st, ctx)
            coef(st, ctx)

        run.parts = (conv, coef)  # (the conv launch alone, what follows it): bench.py times the kernel, not the pair
        run.meta = conv.meta
        return run

    def _halo_layer(self, L):
        """does layer L run on the stride-1 3x3 halo kernel in this plan?"""
        e = self.e
        # (fp32 parity mode: only plans of the BASELINE sizes, see Engine.__init__)
        return e.use_halo and self.B >= e.halo_min_b and L.kind == "conv" and L.wfF is not None and not L.s2

    def _operand_layout(self, L, cp, which, npix):
        """w_frag of a halo launch cp: the layout of layer L's operand copy `which` ("f" forward, "d" data gradient, "e" eval mode, BatchNorm folded
        in), negotiated with the library by the first plan that uses the copy.  npix: output pixels per image."""
        e = self.e
        # the operand's layout is a property of the LAYER, not of whichever plan happens to be built first (a bs = 4 smoke
        # plan used to pin the first halo kernel's layout for the bs = 64 training plan): the library is asked at the canonical batch
        # size of the path (64 RoIs) unless this plan is bigger
        m_plan = cp.M
        cp.M = max(cp.M, 64 * npix)
        cp.w_frag = e.v3_policy   # (the query reads the policy from w_frag; the answer goes back into it below)
        want = int(e.lib.gdrn_conv3x3_wfrag(C.byref(cp)))
        cp.M = m_plan
        if not L.wfmt.get(which):
            L.wfmt[which] = want if want in (1, 2) else 1
            e._pack_dirty = True    # the operand copy is (re)built in that layout by the next repack
        cp.w_frag = L.wfmt[which]  # an operand has ONE layout: later plans (other batch sizes) follow the first one

    def _conv(self, L, x, xs, y, Hi, Wi, Ho, Wo, stride, pad, mode=0, w=None, rows=None, cin=None, cout=None, x_cs=None,
              y_cs=None, bias=None, addend=None, add_cs=0, act=0, out_f32=0, stats=None, KH=None, KW=None, bnb=None, evalw=False, xf=None):
        """a launch of layer L on the stride-1 halo kernel (_halo_layer) or on the generic kernel.  w given: the layer's data gradient (operand
        copy wd).  Returns (op, rows of BatchNorm statistics its epilogue writes).
        bnb (_bnb): data-gradient launch whose output is the gradient w.r.t. that BatchNorm(+ReLU)'s output -- the epilogue masks it and
        accumulates the BN-backward sums (see _fusable), so the BN backward is only its apply pass; the coefficient launch is paired with it.
        xf = dict(mode, x2, a, b, c, c2, msc, msh, out, relu): the conv's input is v(x, x2) evaluated while the patch is staged
        (gdrn_hip.h, xf_mode), `out` (same shape as x) receives v -- halo launches only."""
        e = self.e
        cp = ConvParams()
        cp.x, cp.w, cp.y = ptr(x), ptr(w if w is not None else L.wf), ptr(y)
        cp.bias, cp.addend, cp.stats = ptr(bias), ptr(addend), ptr(stats)
        cp.Hi, cp.Wi, cp.Cin, cp.x_cs = Hi, Wi, cin or L.cin_f, x_cs or xs
        cp.Ho, cp.Wo, cp.Cout = Ho, Wo, cout or L.O
        cp.y_cs = y_cs or y.shape[-1]
        cp.add_cs = add_cs
        cp.KH, cp.KW, cp.stride, cp.pad = KH or L.KH, KW or L.KW, stride, pad
        cp.mode, cp.act, cp.out_f32 = mode, act, out_f32
        cp.M = self.B * (Ho // 2) * (Wo // 2) if mode == 1 else self.B * Ho * Wo
        cp.w_rows = rows or L.rows_f
        cp.dtype = e.dt
        halo = self._halo_layer(L)
        if bnb is not None:
            assert halo or e.gemm_bnb, L.key
            self._fill_bnb(cp, bnb)
        if xf is not None:
            cp.xf_mode = xf["mode"]     # (the library's kernel choice depends on addend, stored mask and operand transform)
        # eight-wave form of the small-map tile (gdrn_hip.h, halo_waves): the library's choice in the forward pass and in inference (r5, isolated:
        # 256@16x16 22.3 -> 21.7 us plain, 27.2 -> 24.6 with the BatchNorm-backward transform; 512@8x8 25.1 -> 23.8 / 30.5 -> 26.5; inference
        # 1.98 -> 1.96 ms); the data gradients of a two-stream backward pass keep four waves -- two 235-register waves per SIMD leave the
        # side stream's weight gradient no room on the CU (7.37 -> 7.70 ms per step with eight waves everywhere, 7.93 -> 7.85 on one stream)
        cp.halo_waves = e.halo_waves or (4 if (w is not None and (e.wgrad_stream or e.wgrad_force_lds)) else 0)   # ("serial": the two-stream step's launches)
        cp.v3_min_wg = e.v3_min_wg
        self.keep.append(cp)
        ref = C.byref(cp)
        if halo:
            self._operand_layout(L, cp, "e" if evalw else ("f" if w is None else "d"), Ho * Wo)
        th, tw, hbn = C.c_int(0), C.c_int(0), C.c_int(0)
        e.lib.gdrn_conv3x3_tile(ref, C.byref(th), C.byref(tw), C.byref(hbn))
        if halo and th.value <= 0:
            raise RuntimeError(f"{L.key}: no halo tiling for {Hi}x{Wi} (the generic-layout operand copy is not maintained)")
        if evalw:      # eval-mode operand with the BatchNorm scale folded in (Engine.fold)
            assert w is None
            cp.w = ptr(L.wfF_e if halo else L.wf_e)
        elif halo:     # fragment-major operand copy (forward: of wf, data gradient: of wd)
            cp.w = ptr(L.wfF if w is None else L.wdF)
        if xf is not None:
            assert halo and e.h16, L.key
            assert xf["out"] is None or (xf["out"].shape == x.shape and xf["out"].dtype == x.dtype), L.key
            assert xf.get("x2") is None or xf["x2"].shape == x.shape, L.key
            cp.xf_mode, cp.xf_relu = xf["mode"], 1 if xf.get("relu") else 0
            cp.xf_x2, cp.xf_a, cp.xf_b, cp.xf_c, cp.xf_c2 = ptr(xf.get("x2")), ptr(xf.get("a")), ptr(xf.get("b")), ptr(xf["c"]), ptr(xf.get("c2"))
            cp.xf_msc, cp.xf_msh, cp.xf_out = ptr(xf.get("msc")), ptr(xf.get("msh")), ptr(xf.get("out"))
        nrows = int((e.lib.gdrn_conv3x3_stats_rows if halo else e.lib.gdrn_conv_stats_rows)(ref))
        op = _launch_struct(e.lib.gdrn_conv3x3_halo if halo else e.lib.gdrn_conv_gemm, f"conv {L.key}", cp,
                            self._conv_meta(L, cp, (th.value, tw.value, hbn.value) if halo else None, Hi, Wi, Ho, Wo, mode, w is not None))
        return (op if bnb is None else self._with_coef(op, bnb.key, nrows)), nrows

    def _conv_meta(self, L, cp, halo_tile, Hi, Wi, Ho, Wo, mode, dgrad):
        """metadata of a _conv launch: halo_tile: (th, tw, hbn) of a halo launch, None for the generic kernel; dgrad: the launch is the layer's
        data gradient."""
        e, ref = self.e, C.byref(cp)
        bm, bn = C.c_int(0), C.c_int(0)
        e.lib.gdrn_conv_tile(ref, C.byref(bm), C.byref(bn))
        small = (Ho * Wo) if (mode == 0 and (not dgrad or L.kind == "convT")) else (Hi * Wi)   # (mode 1 and the ConvTranspose's forward: the input map)
        dn = "bf16" if e.h16 else "f32"   # (the 16-bit instantiation: its name in a trace is the same in both library builds)
        th, tw, hbn = halo_tile or (0, 0, 0)
        if halo_tile and cp.w_frag == 2:
            kname = f"conv3x3_v3_kernel<{th},{hbn},{'2,4,1' if hbn == 256 else '2,2,2'},{cp.xf_mode}>"  # (the template's name in a trace)
        elif halo_tile:
            kname = f"conv3x3_halo_kernel<{dn},{th},{tw},{hbn},{cp.xf_mode},{int(e.lib.gdrn_conv3x3_halo_waves(ref)) // 4}>"
        else:
            kname = f"conv_gemm_kernel<{dn},{bm.value},{bn.value}>"
        return self._meta(kname, self._macs(L, small), (self.B * Hi * Wi * cp.Cin + self.B * Ho * Wo * cp.Cout + cp.Cout * cp.Cin * cp.KH * cp.KW) * e.esz,
                          L.key + (":dgrad" if dgrad else ""))

    def _s2(self, L, which, x, y, Hi, Ho, Ld=None, yd=None, stats=None, stats_d=None, bias=None, bias_d=None, act=0, bnb=None):
        """a launch of the parity-plane halo kernel gdrn_conv3x3s2, a 3x3 stride-2 pad-1 conv x [B, Hi, Hi, .] -> y [B, Ho = Hi / 2, Ho, .], on operand
        copy `which` of layer L:
          "f" / "e" (eval mode, BatchNorm folded in)  the forward pass of a stage-entry or Patch-PnP conv, with the block's 1x1 shortcut conv Ld -> yd
                                                      in the same launch when given; epilogue: statistics rows (stats, stats_d) or bias + activation
          "d"                                         the data gradient of the head's ConvTranspose2d (x = its output gradient), with the
                                                      BatchNorm-backward epilogue bnb (_bnb) and the coefficient launch behind it (as in _conv)
        Returns (op, statistics rows -- of the main conv and of the shortcut alike) or None when the library does not cover the shape (the generic
        kernel keeps it)."""
        e = self.e
        w = getattr(L, {"f": "wfF", "e": "wfF_e", "d": "wdF"}[which], None)
        if not e.h16 or w is None:
            return None
        dgrad = which == "d"
        cin, cout, w_rows = (L.cin_d, L.I, L.rows_d) if dgrad else (L.cin_f, L.O, L.rows_f)
        sp = S2Params()
        sp.x, sp.w, sp.y = ptr(x), ptr(w), ptr(y)
        sp.bias, sp.stats, sp.act = ptr(bias), ptr(stats), act
        if Ld is not None:
            sp.wd, sp.yd, sp.bias_d, sp.stats_d = ptr(Ld.wf_e if which == "e" else Ld.wf), ptr(yd), ptr(bias_d), ptr(stats_d)
            sp.yd_cs, sp.wd_rows = yd.shape[-1], Ld.rows_f
            assert Ld.cin_f == L.cin_f, (L.key, Ld.key)
        if bnb is not None:
            self._fill_bnb(sp, bnb)
        sp.Hi = sp.Wi = Hi
        sp.Ho = sp.Wo = Ho
        sp.Cin, sp.x_cs, sp.Cout, sp.y_cs = cin, x.shape[-1], cout, y.shape[-1]
        sp.N, sp.w_rows, sp.dtype = self.B, w_rows, e.dt
        if not int(e.lib.gdrn_conv3x3s2_ok(C.byref(sp))):
            return None
        self.keep.append(sp)
        nrows = int(e.lib.gdrn_conv3x3s2_stats_rows(C.byref(sp)))
        role = " (data gradient)" if dgrad else ""
        maps = 1 + (Ld is not None) + (bnb is not None)   # Cout-wide maps moved: y, the shortcut's yd, the BatchNorm input the epilogue reads
        meta = self._meta(f"conv3x3s2_kernel<{'true' if Ld is not None else 'false'}>" + role,
                          self._macs(L, Ho * Ho) + (self._macs(Ld, Ho * Ho) if Ld is not None else 0),
                          (self.B * Hi * Hi * cin + maps * self.B * Ho * Ho * cout + cout * cin * 9) * 2,
                          L.key + (":dgrad" if dgrad else "") + ("+downsample" if Ld is not None else ""))
        op = _launch_struct(e.lib.gdrn_conv3x3s2, f"conv3x3s2{role} {L.key}", sp, meta)
        return (op if bnb is None else self._with_coef(op, bnb.key, nrows)), nrows

    def _s2d(self, L, which, dy, dx, Ho, Hi, Ld=None, dyd=None, bnb=None, stats=None, bias=None, act=0):
        """a launch of the parity-class kernel gdrn_conv3x3s2_dgrad, dy [B, Ho, Ho, .] -> dx [B, Hi = 2 Ho, Hi, .], on operand copy `which` of layer L:
          "d"        the data gradient of a 3x3 stride-2 conv; Ld / dyd: the block's 1x1 shortcut conv and ITS output gradient, added in the same
                     launch; bnb (_bnb): dx is the gradient w.r.t. that BatchNorm(+ReLU)'s output -- masked, its backward sums reduced in the
                     epilogue, and the coefficient launch paired with the conv (as in _conv)
          "f" / "e"  the forward pass of the head's ConvTranspose2d(3, stride 2, pad 1, output_padding 1) -- the same sum -- with a forward epilogue:
                     statistics rows (stats, train mode) or the folded BatchNorm's shift + ReLU (bias, act; eval mode)
        Returns (op, rows the epilogue writes) or None when the library does not cover the shape."""
        e = self.e
        w = getattr(L, {"f": "wfF", "e": "wfF_e", "d": "wdF"}[which], None)
        if not e.h16 or w is None:
            return None
        fwd = which != "d"
        cin, cout, w_rows = (L.O, L.cin_f, L.rows_f) if fwd else (L.cin_f, L.cin_d, L.rows_d)   # (channels of dx, of dy)
        sp = S2dParams()
        sp.dy, sp.w, sp.dx = ptr(dy), ptr(w), ptr(dx)
        sp.bias, sp.stats, sp.act = ptr(bias), ptr(stats), act
        if Ld is not None:
            sp.dyd, sp.wdd, sp.dyd_cs, sp.wdd_rows = ptr(dyd), ptr(Ld.wd), dyd.shape[-1], Ld.rows_d
            assert Ld.cin_d == L.cin_d, (L.key, Ld.key)
        if bnb is not None:
            self._fill_bnb(sp, bnb)
        sp.Hi = sp.Wi = Hi
        sp.Ho = sp.Wo = Ho
        sp.Cin, sp.dx_cs, sp.Cout, sp.dy_cs = cin, dx.shape[-1], cout, dy.shape[-1]
        sp.N, sp.w_rows, sp.dtype = self.B, w_rows, e.dt
        if not int(e.lib.gdrn_conv3x3s2_dgrad_ok(C.byref(sp))):
            return None
        self.keep.append(sp)
        nrows = int(e.lib.gdrn_conv3x3s2_dgrad_rows(C.byref(sp)))
        role = " (forward)" if fwd else ""
        tf = lambda b: "true" if b else "false"
        meta = self._meta(f"conv3x3s2_dgrad_kernel<{tf(Ld is not None)},{tf(bnb is not None)}>" + role,
                          self._macs(L, Ho * Ho) + (self._macs(Ld, Ho * Ho) if Ld is not None else 0),
                          (self.B * Hi * Hi * cin + (2 if Ld is not None else 1) * self.B * Ho * Ho * cout + cout * cin * 9) * 2,
                          L.key + ("" if fwd else ":dgrad") + ("+downsample:dgrad" if Ld is not None else ""))
        op = _launch_struct(e.lib.gdrn_conv3x3s2_dgrad, f"conv3x3s2_dgrad{role} {L.key}", sp, meta)
        return (op if bnb is None else self._with_coef(op, bnb.key, nrows)), nrows

    def _wgrad(self, L, x, dy, Hi, Wi, Ho, Wo, stride, pad, cin, cout, x_cs, dy_cs, KH=None, KW=None, defer=False):
        """the weight gradient of layer L: deferred to its bucket's grouped launch (returns None) where the 3x3 halo kernel covers it, else a
        side-stream launch of the generic kernel"""
        e = self.e
        wp = WgradParams()
        wp.x, wp.dy, wp.dw = ptr(x), ptr(dy), ptr(L.dwp)
        wp.Hi, wp.Wi, wp.Cin, wp.x_cs = Hi, Wi, cin, x_cs
        wp.Ho, wp.Wo, wp.Cout, wp.dy_cs = Ho, Wo, cout, dy_cs
        wp.KH, wp.KW, wp.stride, wp.pad = KH or L.KH, KW or L.KW, stride, pad
        wp.M, wp.dtype, wp.splits, wp.variant = self.B * Ho * Wo, e.dt, 0, 0
        self.keep.append(wp)
        # halo-tiled kernel: every 3x3 pad-1 conv, stride 1 or 2 (incl. Patch-PnP's and, roles swapped, the head's ConvTranspose)
        if e.use_halo and L.kind in ("conv", "convT") and L.KK == 9 and bool(e.lib.gdrn_conv3x3_wgrad_ok(C.byref(wp))):
            # deferred: one grouped launch per gradient bucket (see _finish_unpack) -- weight gradients are off the
            # critical path, and a grid over many layers fills the chip with far fewer pixel-range splits per layer
            # (flops, algorithmic bytes: X and dY read once at the storage width, the fp32 gradient written once)
            self._wgrad_deferred.append((len(self.bwd_groups), L, wp, (2.0 * self._macs(L, Ho * Wo),
                                                                      2.0 * self.B * (Hi * Wi * cin + Ho * Wo * cout) + 4.0 * cout * cin * 9)))
            return None

        self._zero_regions.append(self._pad16(L.dwp, e.dwp_flat))  # accumulated with fp32 atomics
        bco, bci = (64 if cout <= 64 else 128), (128 if cin % 128 == 0 else 64)
        meta = self._meta(f"conv_wgrad_kernel<{'bf16' if e.h16 else 'f32'},{bco},{bci}>", self._macs(L, Ho * Wo),
                          self.B * (Hi * Wi * cin + Ho * Wo * cout) * e.esz + 4 * cout * cin * wp.KH * wp.KW, L.key + ":wgrad")
        # feeds only the optimizer: off the data-gradient chain (side stream, see run_backward)
        return self._side(_launch_struct(e.lib.gdrn_conv_wgrad, f"conv_wgrad {L.key}", wp, meta), defer)

    @staticmethod
    def _side(op, defer=False):
        """mark a backward op whose result only the optimizer reads: it may run on the side stream.
        defer: the op may wait for the end of its gradient bucket (see _merge_forks)."""
        op.side = True
        op.defer = bool(defer)
        return op

    def _merge_forks(self):
        """Every switch of run_backward from the main stream to the side stream is an event record on the main stream, and the chain's next
        kernel starts ~7 us late behind it (r6 timeline: 11 such gaps per step).  Side ops marked `defer` -- the small weight / bias gradients of
        the fc layers and of the 1x1 shortcut convs of layer3.0 / layer4.0, whose buffers are their own -- move to the end of their bucket, in
        front of its grouped weight-gradient launch: one fork per bucket instead of one per op."""
        e = self.e
        if not e.wgrad_stream:
            return
        first = list(e.bucket_first_group)
        for bkt, g0 in enumerate(first):
            hi = first[bkt - 1] if bkt else len(self.bwd_groups)
            moved = []
            for gi in range(hi - 1, g0 - 1, -1):   # execution order: last forward group first
                g = self.bwd_groups[gi]
                moved += [op for op in g if getattr(op, "defer", False)]
                self.bwd_groups[gi] = [op for op in g if not getattr(op, "defer", False)]
            if not moved:
                continue
            g = self.bwd_groups[g0]
            at = next((i for i, op in enumerate(g) if getattr(op, "bucket_end", False)), len(g))
            if bkt == len(first) - 1 and self._front_n:
                at = 0   # (last bucket, tail overlap: its bucket-end ops sit in FRONT of the stem group)
            g[at:at] = moved

    @staticmethod
    def _pad16(t, flat):
        """the 16-byte-padded slice of the flat fp32 buffer `flat` that holds the view `t` (offsets in these buffers are multiples of 4 floats)."""
        off = (t.data_ptr() - flat.data_ptr()) // 4
        assert 0 <= off and off % 4 == 0 and off + t.numel() <= flat.numel(), off
        return flat[off: min(off + _ru(t.numel(), 4), flat.numel())]

    def _grad16(self, g):
        return self._pad16(g, self.e.grad_flat)

    def _build_zero_table(self):
        from .cabi import ZeroTask, to_device_table

        e = self.e
        chunk = e.lib.gdrn_zero_chunk()
        tasks, starts = [], [0]
        seen = set()
        for t in self._zero_regions:
            if t.data_ptr() in seen:
                continue
            seen.add(t.data_ptr())
            assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 and (t.numel() * 4) % 16 == 0, (t.shape, t.data_ptr() % 16)
            n16 = t.numel() * 4 // 16
            tasks.append(ZeroTask(p=t.data_ptr(), n16=n16))
            starts.append(starts[-1] + (n16 + chunk - 1) // chunk)
        self._zero_tab = (to_device_table(tasks, e.dev), torch.tensor(starts, dtype=torch.int32, device=e.dev), len(tasks), starts[-1])

    def _unpack(self, L):
        """packed fp32 weight gradient -> the parameter's .grad layout.  Every layer except the stem is deferred to one
        multi-tensor launch per gradient bucket (see _finish_unpack); the returned op is then a no-op marker."""
        e = self.e
        lib = e.lib
        O, I, KK = L.O, L.I, L.KK
        for n_ in L.src:
            self.grad_group[n_] = len(self.bwd_groups)
        if L.kind == "stem":
            g = e.grads[L.src[0]]
            # (side like the weight-gradient launch whose result it reads: the two stay in order on one stream)
            return self._side(_launch(lib.gdrn_unpack_stem_w, "unpack_stem_w", (L.dwp, g)))
        self._unpack_pending.append((len(self.bwd_groups), L))
        return None  # marker, dropped when the groups are flattened

    def _bn_fwd(self, bnkey, raw, rows, C_, npix, y, residual=None, relu=1, stats=None):
        """finalize (train) or eval params, then apply.  Returns list of fwd ops.  rows: partial rows of statistics the producing launch wrote (train
        mode) to stats, its scratch (default self.stats)."""
        e, lib = self.e, self.e.lib
        stats = self.stats if stats is None else stats
        s = NS(mean=e._empty(C_, dtype=torch.float32), invstd=e._empty(C_, dtype=torch.float32),
               scale=e._empty(C_, dtype=torch.float32), shift=e._empty(C_, dtype=torch.float32), C=C_, npix=npix)
        self.bn[bnkey] = s
        g, b = e.P[bnkey + ".weight"], e.P[bnkey + ".bias"]
        rm, rv, nbt = e.Bf[bnkey + ".running_mean"], e.Bf[bnkey + ".running_var"], e.Bf[bnkey + ".num_batches_tracked"]
        ops = []
        if self.bn_train:
            assert rows * 2 * C_ <= stats.numel(), (bnkey, rows, C_)  # the producer's partial rows fit the scratch
            ops.append(_launch(lib.gdrn_bn_finalize, "bn_finalize", (stats, rows, C_, float(npix), g, b, rm, rv, nbt, 0.1, 1e-5, s.mean, s.invstd,
                                                                     s.scale, s.shift, e.bn_ws)))
        else:
            # eval mode: scale/shift only depend on the parameters and running statistics -- recomputed when those changed
            # (see run_forward), not on every call (43 tiny launches = 8 % of an inference forward)
            self.eval_prep.append(_launch(lib.gdrn_bn_eval_params, "bn_eval_params", (g, b, rm, rv, 1e-5, C_, s.scale, s.shift)))
        if y is not None:
            ops.append(_launch(lib.gdrn_bn_apply, "bn_apply", (raw, s.scale, s.shift, residual, y, npix, C_, relu, e.dt)))
        return ops

    def _xf_ok(self, L):
        """can layer L's halo launches (forward and data gradient) take a fused operand transform?"""
        return self.e.fuse_xf and self.bn_train and self._halo_layer(L)   # (fuse_xf: 16-bit modes only, where every plan size runs the halo kernel)

    def _bn_coef_op(self, bnkey, rows, nrows):
        """rows [nrows][2][C] of BatchNorm-backward sums -> (ka, kb, kc) of dx = ka*g + kb*x + kc, dgamma, dbeta (one launch)."""
        e, lib = self.e, self.e.lib
        s = self.bn[bnkey]
        if getattr(s, "ka", None) is None:
            s.ka, s.kb, s.kc = (e._empty(s.C, dtype=torch.float32) for _ in range(3))
        g = e.P[bnkey + ".weight"]
        dg, db = e.grads[bnkey + ".weight"], e.grads[bnkey + ".bias"]
        self.grad_group[bnkey + ".weight"] = self.grad_group[bnkey + ".bias"] = len(self.bwd_groups)
        return _launch(lib.gdrn_bn_bwd_coef, "bn_bwd_coef", (rows, nrows, s.C, s.npix, g, s.mean, s.invstd, s.ka, s.kb, s.kc, dg, db))

    def _conv_bn_eval(self, L, bnkey, x, xs, y, Hi, Wi, Ho, Wo, stride, pad, relu, residual=None, add_cs=0, **kw):
        """eval mode: conv -> BatchNorm (-> +residual) (-> ReLU) as ONE launch, y = act(conv_{w*scale}(x) + shift + residual)."""
        f = self.e.fold(bnkey, L)
        self._hook_fold()
        return self._conv(L, x, xs, y, Hi, Wi, Ho, Wo, stride, pad, bias=f.shift, addend=residual, add_cs=add_cs, act=1 if relu else 0,
                          evalw=True, **kw)[0]

    def _fusable(self, L):
        """can the data gradient of layer L run on the halo kernel (and so carry a fused BN-backward reduction)?  Asked about stride-1 layers only."""
        e = self.e
        # (not _halo_layer: True for the stride-2 3x3 layers as well, which hold a fragment-major copy for gdrn_conv3x3s2)
        return e.use_halo and e.h16 and L.kind == "conv" and L.wfF is not None

    def _bn_bwd(self, bnkey, dy, ymask, raw, dx, g_out=None, affine_mask=False, sums="here", xf=False):
        """BatchNorm(+ReLU) backward: [reduce -> coef ->] apply.  Returns (ops, xf): xf=True leaves the apply pass to the consumer halo conv --
        the returned xf is that conv's operand transform (see _conv), which also writes dx; else None.
        sums: who reduces the backward sums --
          "here"      a reduce launch of this call, and the coefficient launch behind it
          "dgrad"     the data-gradient launch that produced dy: dy arrives masked, and its epilogue rows have been turned into the coefficients
                      already (see _conv, bnb)
          "upsample"  the upsampling adjoint that produced dy (gdrn_upsample2x_bwd_bnsums): the rows are written, only the coefficient launch
                      is left; dy itself is NOT masked
        affine_mask: BN -> ReLU without residual: the ReLU mask is recomputed from raw*scale+shift (what bn_apply
        evaluated) instead of reading the stored activation `ymask` -- one tensor pass less in both kernels."""
        e, lib = self.e, self.e.lib
        s = self.bn[bnkey]
        msc, msh = (s.scale, s.shift) if affine_mask else (None, None)
        ym = None if affine_mask else ymask
        ops = []
        if sums == "dgrad":
            self._bn_coef_op(bnkey, self.stats, 1)  # (allocates the coefficient vectors; the launch itself sits in _with_coef)
            msc = msh = ym = None                    # dy is already masked
        else:
            assert sums in ("here", "upsample"), sums
            nrows = int(lib.gdrn_bn_bwd_reduce_rows(s.npix, s.C, e.dt))
            assert nrows > 0 and nrows * 2 * s.C <= self.stats.numel(), (bnkey, nrows)
            coef = self._bn_coef_op(bnkey, self.stats, nrows)
            if sums == "here":
                ops.append(_launch(lib.gdrn_bn_bwd_reduce, "bn_bwd_reduce", (dy, ym, raw, s.mean, s.invstd, msc, msh, s.npix, s.C, self.stats, e.dt)))
            ops.append(coef)
        if xf:
            assert g_out is None and ym is None
            return ops, dict(mode=4 if msc is not None else 3, x2=raw, a=s.ka, b=s.kb, c=s.kc, msc=msc, msh=msh, out=dx, relu=False)
        ops.append(_launch(lib.gdrn_bn_bwd_apply, "bn_bwd_apply", (dy, ym, raw, s.ka, s.kb, s.kc, msc, msh, s.npix, s.C, dx, g_out, e.dt)))
        return ops, None

    def _unpack_task(self, L, packed_ptr, grad, rows_valid, rows_off=0):
        from .cabi import PackTask

        O, I, KK = L.O, L.I, L.KK
        if L.kind == "convT":  # dwp [ci=I][KK][co(out_ch)] -> weight[ci][co][k]
            a = (I, 1, KK, L.out_ch, I, 1, O, O * KK, 0, 1, KK)
        else:
            a = (rows_valid, 1, KK, L.in_ch, rows_valid, 1, I, I * KK, 0, 1, KK)
        A1, A2, T, B, A1v, A2v, Bv, s1, s2, st, sb = a
        return PackTask(src=packed_ptr, dst=grad.data_ptr(), A1=A1, A2=A2, T=T, B=B, A1v=A1v, A2v=A2v, Bv=Bv, flip=0, s1=s1, s2=s2,
                        st=st, sb=sb, n=A1v * A2v * T * Bv, frag=0, pad_=0)

    def _bucket_end(self, bkt, op):
        """place a bucket-end op (grouped weight gradient, its reduction, gradient unpack).  Behind the bucket's last group -- except for the
        LAST bucket with the side stream on: its ops only need the layers' data gradients, which exist before the stem's backward (max-pool
        backward, BatchNorm coefficients, stem weight gradient: ~0.2 ms on the main stream), so they go in FRONT of the stem group and run
        under it instead of behind it."""
        e = self.e
        op.bucket_end = True
        g = self.bwd_groups[e.bucket_first_group[bkt]]
        if e.wgrad_stream and bkt == len(e.bucket_first_group) - 1 and e.bucket_first_group[bkt] == 0:
            g.insert(self._front_n, op)
            self._front_n += 1
        else:
            g.append(op)

    def _table_op(self, fn, what, tasks, starts, tables, *extra):
        """side-stream launch fn(table of `tasks`, workgroup range starts, number of tasks, number of workgroups, *extra); `tables` keeps the
        two device tensors"""
        tab = cabi.to_device_table(tasks, self.e.dev)
        stt = torch.tensor(starts, dtype=torch.int32, device=self.e.dev)
        tables.append((tab, stt))
        op = _launch(fn, what, (tab, stt, len(tasks), starts[-1]) + extra)
        op.side = True
        return op

    def _finish_unpack(self):
        """The bucket-end work of every gradient bucket (pnp | head | layer4 | layer3 | rest): one grouped weight-gradient launch, one
        gdrn_unpack_multi and one reduction of the weight-gradient partials, appended to the backward group that completes the bucket, so
        the RCCL exchange of a bucket still starts as soon as its gradients exist."""
        from .cabi import WreduceTask

        e, lib = self.e, self.e.lib
        chunk = lib.gdrn_pack_chunk()
        assert len(self.bwd_groups) == 29, len(self.bwd_groups)
        # backward groups in forward order: stem(0) layer1(1-3) layer2(4-7) layer3(8-13) layer4(14-16) convT(17) head convs(18-23)
        # head out(24) pnp convs(25-27) fc(28)
        first_group = e.bucket_first_group  # forward index of the LAST-executed group of each bucket
        bucket_of = lambda gi: next(i for i, g0 in enumerate(first_group) if gi >= g0)
        wg_bucket = {i: [] for i in range(len(first_group))}
        for gi, L, wp, fb in self._wgrad_deferred:
            wg_bucket[bucket_of(gi)].append((L, wp, fb))
        self._wgrad_tables = []
        for bkt, items in wg_bucket.items():
            if items:
                self._bucket_end(bkt, self._grouped_wgrad(bkt, items))

        per_bucket = {i: [] for i in range(len(first_group))}
        red_bucket = {i: [] for i in range(len(first_group))}
        for gi, L in self._unpack_pending:
            bkt = bucket_of(gi)
            if L.key in self._wreduce:
                ws, nsplit, cout, cin, civ = self._wreduce[L.key]
                assert cout == (L.I if L.kind == "convT" else L.O) and civ <= cin, (L.key, cout, cin, civ)
                assert e.grads[L.src[0]].numel() == cout * civ * 9, L.key
                red_bucket[bkt].append(WreduceTask(ws=ws.data_ptr(), dst=e.grads[L.src[0]].data_ptr(), nsplit=nsplit, Cout=cout, Cin=cin,
                                                   cin_valid=civ, s_co=civ * 9, s_ci=9, s_t=1))
            elif L.key == "pnp_net.fc_rt":
                per_bucket[bkt].append(self._unpack_task(L, L.dwp.data_ptr(), e.grads["pnp_net.fc_r.weight"], 6))
                per_bucket[bkt].append(self._unpack_task(L, L.dwp.data_ptr() + 6 * L.in_ch * 4, e.grads["pnp_net.fc_t.weight"], 3))
            else:
                per_bucket[bkt].append(self._unpack_task(L, L.dwp.data_ptr(), e.grads[L.src[0]], L.O))
        self._unpack_tables = []
        for bkt, tasks in per_bucket.items():
            if not tasks:
                continue
            starts = [0]
            for t in tasks:
                starts.append(starts[-1] + (cabi.transpose_blocks(lib, t) or (t.n + chunk - 1) // chunk))   # (fc1's gradient: 64 x 64 tiles through LDS)
            self._bucket_end(bkt, self._table_op(lib.gdrn_unpack_multi, "unpack_multi", tasks, starts, self._unpack_tables))
        for bkt, tasks in red_bucket.items():
            if not tasks:
                continue
            starts = [0]
            for t in tasks:
                starts.append(starts[-1] + t.Cout * t.Cin // 256)
            self._bucket_end(bkt, self._table_op(lib.gdrn_wgrad_reduce_multi, "wgrad_reduce_multi", tasks, starts, self._unpack_tables))

    def _grouped_wgrad(self, bkt, items):
        """the halo weight gradients [(layer, WgradParams, (flops, bytes))] of gradient bucket bkt as ONE launch of the 64 x 64 tile: a common
        number of 8x8 pixel patches per workgroup, chosen so that the grid has ~wgrad_blocks workgroups; longest-running tasks first"""
        e, lib = self.e, self.e.lib
        # work of a layer in 32-pixel k-steps: an 8x8-pixel stage (stride 1) is two, a 4x8-pixel stage (stride 2) one
        geo = []
        for L, wp, flops in items:
            s2 = wp.stride == 2
            npatch = (wp.M // (wp.Ho * wp.Wo)) * (wp.Ho // (4 if s2 else 8)) * (wp.Wo // 8)
            geo.append((npatch, npatch * (1 if s2 else 2), (wp.Cout // 64) * (wp.Cin // 64)))
        # k-steps per workgroup: the grid's target, but no more than the layers of a shape class that carries >= 20 % of the bucket's work
        # have -- a layer with fewer k-steps than `per` runs as ONE split of short workgroups beside the others' long ones (r6: layer4's 128
        # against 171-256 for layer3 in their common launch: 434 us stand-alone against 322 with 128 everywhere, -0.06 ms per step;
        # profiles/r06_wgrad_bucket_balance.txt).  Small classes (the head's ConvTranspose: 1 % of its bucket) do not set the length.
        total = sum(u * t for _, u, t in geo)
        share = {}
        for _, u, t in geo:
            share[u] = share.get(u, 0) + u * t
        # (floor of 64 k-steps: only the Patch-PnP bucket sits on it -- 168 instead of 672 partial tiles for its reduction to read; r6: -0.02 ms)
        per = max(64 if self.B >= 32 else 16, min([total // e.wgrad_blocks] + [u for u, w in share.items() if 5 * w >= total]))
        tasks = []
        for (L, wp, flops), (npatch, units, tiles) in zip(items, geo):
            wp.variant = 0
            wp.ws = ptr(e.dwp_flat)  # non-null placeholder for the split query
            wp.splits = max(1, units // per)
            wp.splits = int(lib.gdrn_conv3x3_wgrad_splits(C.byref(wp)))  # normalised: no empty split
            assert wp.splits >= 1, L.key
            ws = e._empty(wp.splits * wp.Cout * wp.Cin * 9, dtype=torch.float32)
            self.keep.append(ws)
            wp.ws, wp.dw = ptr(ws), None
            # the kernel's "Cin" role = the parameter's input channels for a conv (69 real of 128 for Patch-PnP's first conv), its
            # second dimension for the ConvTranspose (weight [Cin_w][Cout_w][3][3] with x = output gradient, dy = input)
            self._wreduce[L.key] = (ws, wp.splits, wp.Cout, wp.Cin, L.O if L.kind == "convT" else L.I)
            tasks.append((-(units // wp.splits), len(tasks), wp, tiles, flops))
        tasks.sort(key=lambda t: t[:2])
        starts = [0]
        for _, _, wp, tiles, _ in tasks:
            starts.append(starts[-1] + tiles * wp.splits)
        # on the side stream (wgrad_stream) a bucket's weight gradients run under the NEXT bucket's data-gradient chain with one
        # workgroup per CU (LDS request), so that the chain's workgroups find room on every CU; the last bucket has nothing to hide under
        last_bucket = bkt == len(e.bucket_first_group) - 1
        lds = e.wgrad_side_lds if (not last_bucket and (e.wgrad_stream or e.wgrad_force_lds)) else 0
        run = self._table_op(lib.gdrn_conv3x3_wgrad_multi_lds, "conv3x3_wgrad_multi", [t[2] for t in tasks], starts, self._wgrad_tables, lds)
        run.meta = dict(kernel="conv3x3_wgrad_multi_kernel", flops=sum(t[4][0] for t in tasks), bytes=sum(t[4][1] for t in tasks),
                        layer=f"bucket{bkt}@{e.bucket_first_group[bkt]}:wgrad x{len(tasks)} ({starts[-1]} wg)")
        return run

    # ---- graph -------------------------------------------------------------------------------
    def _build(self):
        """The graph in forward order.  Every stage builder appends its launches to self.fwd and, with a backward graph, ONE group to
        self.bwd_groups; what a stage hands to the next travels in a cursor (NS) per chain:
          backbone  x, d_x (block input and its gradient buffer), Hc, inpl, prev_raw2 (bn2 input of the previous block), pend
          head      hx, d_hx, Hh, prev_bn, prev_raw, pend_h, up_next
          Patch-PnP px, d_px, Hp, cin"""
        e, lib, B = self.e, self.e.lib, self.B
        # per-tile BN partial sums, max over layers: conv tiles need <= B*32768 floats (64-pixel tiles of the 64x64 maps at 256
        # channels); the direct stem kernel writes one [2][64] row per wave
        n_stats = max(B * 32768 + 65536, 1024 * 2 * 512)  # ... and gdrn_bn_bwd_reduce writes <= 1024 rows of 2*C floats
        if e.stem_direct:
            n_stats = max(n_stats, int(lib.gdrn_stem_stats_rows(B)) * 128)
        self.stats = self._E(n_stats, dtype=F32t)
        self.stats_b = self._E(B * 4096 + 4096, dtype=F32t)   # rows of a fused 1x1 shortcut conv (gdrn_conv3x3s2: <= B * 16 tiles x 2 x 128 channels)
        bb = self._stem()
        for li, (nb, pl) in enumerate(zip(RESNET34_LAYERS, RESNET34_PLANES), start=1):
            for b in range(nb):
                self._block(bb, li, b, nb, pl)
        assert bb.pend is None
        hd = self._head_convT(bb.x, bb.d_x, bb.prev_raw2)
        for hi in range(len(HEAD_CONVS)):
            self._head_conv(hd, hi)
        assert hd.pend_h is None
        self._head_out(hd)
        pn = NS(px=self.pnp_in, d_px=self.d_pnp_in if self.has_backward else None, Hp=64, cin=128)
        for ci, gi in ((0, 1), (3, 4), (6, 7)):
            self._pnp_conv(pn, ci, gi)
        f1, f2 = self._fc_fwd(pn.px)
        if self.has_backward:
            self._fc_bwd(pn.px, pn.d_px, f1, f2)
        self._pose()

    def _stem(self):
        """image pack, conv1 7x7 stride 2, bn1, ReLU, max-pool (backward group 0).  Returns the backbone cursor."""
        e, lib, B, S, E = self.e, self.e.lib, self.B, self.bn_train, self._E
        Ls = e.layers["backbone.conv1"]
        self.img_p = e._zeros(B, 262, 272, 4)
        fused_stem = e.stem_direct and not S   # eval mode: conv + bn1 + ReLU + max-pool in one kernel (gdrn_stem_conv_pool): no raw0 / idx0
        raw0 = None if fused_stem else E(B, 128, 128, 64)
        p0 = E(B, 64, 64, 64)
        idx0 = None if fused_stem else E(B, 64, 64, 64, dtype=torch.uint8)
        flops = 2.0 * B * 128 * 128 * 64 * 147
        self.fwd.append(lambda st, ctx: check(lib.gdrn_pack_image(ctx["img"], ptr(self.img_p), B, 256, 256, 262, 272, e.dt, st), "pack_image"))
        rows = None   # (eval mode: no statistics)
        if e.stem_direct and S:
            rows = int(lib.gdrn_stem_stats_rows(B))
            self.fwd.append(_launch(lib.gdrn_stem_conv, "stem_conv", (self.img_p, e.stem_w32, raw0, self.stats, B, e.dt),
                                    dict(kernel="stem_conv_kernel", flops=flops, layer="backbone.conv1")))
        elif not fused_stem:
            op, rows = self._conv(Ls, self.img_p, 4, raw0, 262, 272, 128, 128, 2, 0, cin=64, cout=64, x_cs=4, KH=7, KW=1,
                                  stats=self.stats if S else None)
            self.fwd.append(op)
        self.fwd += self._bn_fwd("backbone.bn1", raw0, rows, 64, B * 128 * 128, None)
        s0 = self.bn["backbone.bn1"]
        if fused_stem:
            self.fwd.append(_launch(lib.gdrn_stem_conv_pool, "stem_conv_pool", (self.img_p, e.stem_w32, s0.scale, s0.shift, p0, B, e.dt),
                                    dict(kernel="stem_conv_pool_kernel", flops=flops, layer="backbone.conv1+bn1+relu+maxpool")))
        else:
            self.fwd.append(_launch(lib.gdrn_bn_relu_maxpool_fwd, "bn_relu_maxpool", (raw0, s0.scale, s0.shift, p0, idx0, B, 128, 128, 64, e.dt)))
        self.tensors.update({"stem.pool": p0} if fused_stem else {"stem.raw": raw0, "stem.pool": p0})
        if not self.has_backward:
            return NS(x=p0, d_x=None, Hc=64, inpl=64, prev_raw2=None, pend=None)
        d_p0 = E(B, 64, 64, 64)
        g_stem = E(B, 128, 128, 64)
        self.tensors.update({"stem.d_pool": d_p0, "stem.g": g_stem})
        if e.stem_direct:
            # the max-pool backward also emits the BatchNorm-backward sums of the gradient it writes (one partial row per workgroup): no
            # separate reduce pass over the two 134 MB tensors.  The stem has no data gradient: its BatchNorm-backward apply is evaluated
            # inside the weight-gradient kernel while the dy tile is staged (no 134 MB d_raw0 round trip, dy read once instead of once per
            # kernel row)
            mp_rows = int(lib.gdrn_maxpool_bwd_rows(B, 128, 128, 64, e.dt))
            assert mp_rows * 2 * 64 <= self.stats.numel()
            grp = [_launch(lib.gdrn_maxpool_bwd, "maxpool_bwd", (d_p0, idx0, raw0, s0.scale, s0.shift, g_stem, B, 128, 128, 64, s0.mean if mp_rows else None,
                                                                s0.invstd if mp_rows else None, self.stats if mp_rows else None, e.dt))]
            gw = e.grads["backbone.conv1.weight"]
            assert gw.is_contiguous() and gw.dtype == torch.float32
            sw_ws = e._empty(int(lib.gdrn_stem_wgrad_parts(B)) * 64 * 224, dtype=torch.float32)
            grp.append(self._bn_coef_op("backbone.bn1", self.stats, mp_rows))  # rows -> (a, b, c), dgamma, dbeta; the apply is fused below
            self._zero_regions.append(self._grad16(gw))
            self.grad_group["backbone.conv1.weight"] = len(self.bwd_groups)
            grp.append(_launch(lib.gdrn_stem_wgrad, "stem_wgrad", (self.img_p, g_stem, raw0, s0.ka, s0.kb, s0.kc, B, sw_ws, gw, e.dt | PREZEROED),
                               dict(kernel="stem_wgrad_kernel", flops=flops, layer="backbone.conv1:wgrad")))
        else:
            grp = [_launch(lib.gdrn_maxpool_bwd, "maxpool_bwd", (d_p0, idx0, raw0, s0.scale, s0.shift, g_stem, B, 128, 128, 64, None, None, None, e.dt))]
            grp += self._bn_bwd("backbone.bn1", g_stem, None, raw0, g_stem)[0]   # (in place)
            grp.append(self._wgrad(Ls, self.img_p, g_stem, 262, 272, 128, 128, 2, 0, 64, 64, 4, 64, KH=7, KW=1))
            grp.append(self._unpack(Ls))
        self.bwd_groups.append(grp)
        return NS(x=p0, d_x=d_p0, Hc=64, inpl=64, prev_raw2=None, pend=None)

    def _block(self, c, li, b, nb, pl):
        """BasicBlock b of layer li (nb blocks, pl planes) behind the backbone cursor c, which it advances.
        c.pend: the block input c.x is not materialised yet -- it is v = relu(a*x1 + b*x2 + c) of the previous block's bn2 output and
        identity, evaluated (and written to c.x) by THIS block's conv1 while it stages its patch (xf, see _conv)"""
        e, B, E = self.e, self.B, self._E
        pfx = f"backbone.layer{li}.{b}"
        stride = 2 if (b == 0 and li > 1) else 1
        Ho = c.Hc // stride
        k = NS(pfx=pfx, li=li, b=b, nb=nb, pl=pl, stride=stride, Ho=Ho, L1=e.layers[pfx + ".conv1"], L2=e.layers[pfx + ".conv2"],
               Ld=e.layers.get(pfx + ".downsample.0"), rawd=None)
        k.raw1, k.a1, k.raw2, k.out = E(B, Ho, Ho, pl), E(B, Ho, Ho, pl), E(B, Ho, Ho, pl), E(B, Ho, Ho, pl)
        self.tensors.update({pfx + ".raw1": k.raw1, pfx + ".a1": k.a1, pfx + ".raw2": k.raw2, pfx + ".out": k.out})
        pend = None
        if not self.bn_train:
            self._block_eval(c, k)
        else:
            pend = self._block_fwd(c, k)
            if self.has_backward:
                self._block_bwd(c, k)
        c.x, c.Hc, c.inpl, c.prev_raw2, c.pend = k.out, Ho, pl, k.raw2, pend

    def _block_eval(self, c, k):
        """eval mode: BatchNorm folded into the preceding conv (weights pre-scaled, shift as bias) -- one launch for a 64-channel block,
        three (four) otherwise, no BatchNorm passes"""
        e, lib, B = self.e, self.e.lib, self.B
        x, Hc, inpl = c.x, c.Hc, c.inpl
        pfx, pl, Ho, stride, L1, L2, Ld, a1, out = k.pfx, k.pl, k.Ho, k.stride, k.L1, k.L2, k.Ld, k.a1, k.out
        if e.h16 and Ld is None and inpl == 64 and pl == 64 and e.use_halo and B >= e.halo_min_b and L1.wfF is not None \
                and L1.wfmt.get("e", 1) == 1 and L2.wfmt.get("e", 1) == 1 and int(lib.gdrn_block64_eval_ok(B, Hc, Hc, e.dt)):
            # 64 channels (layer1): the whole BasicBlock as ONE launch, the intermediate in LDS (r6, csrc/block64.hip)
            f1, f2 = e.fold(pfx + ".bn1", L1), e.fold(pfx + ".bn2", L2)
            L1.wfmt["e"] = L2.wfmt["e"] = 1   # (fragment-major layout of the first halo kernel: what gdrn_block64_eval reads)
            self._hook_fold()
            self.fwd.append(_launch(lib.gdrn_block64_eval, "block64_eval", (x, L1.wfF_e, f1.shift, L2.wfF_e, f2.shift, out, B, Hc, Hc, e.dt),
                                    dict(kernel="block64_eval_kernel", flops=2.0 * 2 * B * Hc * Hc * 64 * 64 * 9, layer=pfx + ".conv1+conv2")))
            del self.tensors[pfx + ".raw1"], self.tensors[pfx + ".a1"], self.tensors[pfx + ".raw2"]
            return
        s2op = None
        if Ld is not None and e.h16 and L1.wfF is not None:
            # stage entry: conv1 (3x3 stride 2) and the 1x1 shortcut in ONE launch of the parity-plane kernel (r6), BatchNorms folded
            f1, fd = e.fold(pfx + ".bn1", L1), e.fold(pfx + ".downsample.1", Ld)
            self._hook_fold()
            res = self._E(B, Ho, Ho, pl)
            s2op = self._s2(L1, "e", x, a1, Hc, Ho, Ld=Ld, yd=res, bias=f1.shift, bias_d=fd.shift, act=1)
        if s2op is not None:
            self.fwd.append(s2op[0])
        else:
            self.fwd.append(self._conv_bn_eval(L1, pfx + ".bn1", x, inpl, a1, Hc, Hc, Ho, Ho, stride, 1, relu=True))
        res = x if Ld is None else (res if s2op is not None else None)
        if Ld is not None and s2op is None:
            res = self._E(B, Ho, Ho, pl)
            self.fwd.append(self._conv_bn_eval(Ld, pfx + ".downsample.1", x, inpl, res, Hc, Hc, Ho, Ho, stride, 0, relu=False))
        self.fwd.append(self._conv_bn_eval(L2, pfx + ".bn2", a1, pl, out, Ho, Ho, Ho, Ho, 1, 1, relu=True, residual=res, add_cs=pl))

    def _block_fwd(self, c, k):
        """training forward of a BasicBlock (batch statistics).  Sets k.rawd (shortcut conv output) and returns the next block's `pend`."""
        e, B, S, E = self.e, self.B, self.bn_train, self._E
        x, Hc, inpl, pend = c.x, c.Hc, c.inpl, c.pend
        pfx, pl, Ho, stride, L1, L2, Ld, raw1, a1, raw2, out = k.pfx, k.pl, k.Ho, k.stride, k.L1, k.L2, k.Ld, k.raw1, k.a1, k.raw2, k.out
        npo = B * Ho * Ho
        assert pend is None or self._xf_ok(L1)
        s2op = None
        if Ld is not None and pend is None:
            # stage entry (r6): conv1 (3x3 stride 2) and the 1x1 shortcut conv in ONE launch of the parity-plane kernel, each with its
            # own BatchNorm-statistics rows
            rawd_ = E(B, Ho, Ho, pl)
            s2op = self._s2(L1, "f", x, raw1, Hc, Ho, Ld=Ld, yd=rawd_, stats=self.stats if S else None, stats_d=self.stats_b if S else None)
        op, rows1 = s2op or self._conv(L1, pend.x1 if pend else x, inpl, raw1, Hc, Hc, Ho, Ho, stride, 1, stats=self.stats if S else None,
                                       xf=dict(pend.xf, out=x) if pend else None)
        self.fwd.append(op)
        xf1 = self._xf_ok(L2)  # bn1 + ReLU applied by conv2 on load (which also writes a1 for the weight gradient)
        self.fwd += self._bn_fwd(pfx + ".bn1", raw1, rows1, pl, npo, None if xf1 else a1)
        op, rows2 = self._conv(L2, raw1 if xf1 else a1, pl, raw2, Ho, Ho, Ho, Ho, 1, 1, stats=self.stats if S else None,
                               xf=_xf_bn_relu(self.bn[pfx + ".bn1"], out=a1) if xf1 else None)
        self.fwd.append(op)
        # block output relu(bn2(raw2) + identity): left to the next block's conv1 when that is a halo launch
        nxt1 = e.layers.get(f"backbone.layer{k.li}.{k.b + 1}.conv1")
        xf_out = nxt1 is not None and self._xf_ok(nxt1)
        if Ld is None:
            self.fwd += self._bn_fwd(pfx + ".bn2", raw2, rows2, pl, npo, None if xf_out else out, residual=x)
            s2 = self.bn[pfx + ".bn2"]
            # relu(scale2*raw2 + x + shift2)
            return _pend(raw2, dict(mode=2, x2=x, a=s2.scale, c=s2.shift, relu=True)) if xf_out else None
        k.rawd, idn = (rawd_ if s2op is not None else E(B, Ho, Ho, pl)), (None if xf_out else E(B, Ho, Ho, pl))
        self.tensors[pfx + ".rawd"] = k.rawd
        if idn is not None:
            self.tensors[pfx + ".idn"] = idn
        self.fwd += self._bn_fwd(pfx + ".bn2", raw2, rows2, pl, npo, None)
        if s2op is not None:   # (the shortcut conv ran with conv1: only its BatchNorm's finalize is left, from its own rows -- as many as conv1's)
            self.fwd += self._bn_fwd(pfx + ".downsample.1", k.rawd, rows1, pl, npo, idn, relu=0, stats=self.stats_b)
        else:
            op, rows_d = self._conv(Ld, x, inpl, k.rawd, Hc, Hc, Ho, Ho, stride, 0, stats=self.stats if S else None)
            self.fwd.append(op)
            self.fwd += self._bn_fwd(pfx + ".downsample.1", k.rawd, rows_d, pl, npo, idn, relu=0)
        s2, sd = self.bn[pfx + ".bn2"], self.bn[pfx + ".downsample.1"]
        if xf_out:   # relu(scale2*raw2 + scale_d*rawd + shift2 + shift_d)
            return _pend(raw2, dict(mode=2, x2=k.rawd, a=s2.scale, b=sd.scale, c=s2.shift, c2=sd.shift, relu=True))
        self.fwd.append(_launch(e.lib.gdrn_bn_apply, "bn_apply", (raw2, s2.scale, s2.shift, idn, out, npo, pl, 1, e.dt)))
        return None

    def _block_bwd(self, c, k):
        """backward group of a BasicBlock: bn2, conv2, bn1, conv1 (+ shortcut) -- writes c.d_x and moves it to this block's d_out"""
        e, B, E = self.e, self.B, self._E
        x, d_x, Hc, inpl, prev_raw2 = c.x, c.d_x, c.Hc, c.inpl, c.prev_raw2
        pfx, li, b, pl, Ho, stride, L1, L2, Ld = k.pfx, k.li, k.b, k.pl, k.Ho, k.stride, k.L1, k.L2, k.Ld
        raw1, a1, raw2, out, rawd = k.raw1, k.a1, k.raw2, k.out, k.rawd
        d_out = E(B, Ho, Ho, pl)
        d_raw2, d_a1, d_raw1 = E(B, Ho, Ho, pl), E(B, Ho, Ho, pl), E(B, Ho, Ho, pl)
        self.tensors.update({pfx + ".d_out": d_out, pfx + ".d_raw2": d_raw2, pfx + ".d_a1": d_a1, pfx + ".d_raw1": d_raw1})
        # d_out comes from the next block's conv1 data gradient when that is a plain (stride-1) block of the
        # same layer: its halo epilogue has then already applied this block's output ReLU mask and reduced
        # the bn2-backward sums (and d_out itself is the residual-path gradient g2)
        # ... or, for the last block of a layer, the generic kernel's epilogue (next layer's stride-2 conv1 / the head's ConvTranspose)
        pre2 = self._fusable(e.layers[f"backbone.layer{li}.{b + 1}.conv1"]) if b + 1 < k.nb else e.gemm_bnb
        # BatchNorm-backward apply passes fused into the data-gradient conv that consumes their result (xf modes 3 / 4)
        xfb2 = pre2 and self._xf_ok(L2)
        need_dx = d_x is not None
        xfb1 = self._fusable(L2) and self._xf_ok(L1) and Ld is None and need_dx
        if pre2:
            g2 = d_out
            grp, xd2 = self._bn_bwd(pfx + ".bn2", d_out, None, raw2, d_raw2, sums="dgrad", xf=xfb2)
        else:
            g2 = E(B, Ho, Ho, pl)
            self.tensors[pfx + ".g2"] = g2
            grp, xd2 = self._bn_bwd(pfx + ".bn2", d_out, out, raw2, d_raw2, g_out=g2)
        grp.append(self._wgrad(L2, a1, d_raw2, Ho, Ho, Ho, Ho, 1, 1, pl, pl, pl, pl))
        grp.append(self._unpack(L2))
        pre1 = self._fusable(L2)
        grp.append(self._conv(L2, d_out if xfb2 else d_raw2, pl, d_a1, Ho, Ho, Ho, Ho, 1, 1, w=L2.wd, rows=L2.rows_d, cin=L2.cin_d, cout=pl,
                              bnb=_bnb(pfx + ".bn1", raw1, affine=True) if pre1 else None, xf=xd2)[0])
        ops1, xd1 = self._bn_bwd(pfx + ".bn1", d_a1, a1, raw1, d_raw1, affine_mask=True, sums="dgrad" if pre1 else "here", xf=xfb1)
        grp += ops1
        grp.append(self._wgrad(L1, x, d_raw1, Hc, Hc, Ho, Ho, stride, 1, inpl, pl, inpl, pl))
        grp.append(self._unpack(L1))
        if Ld is not None:
            d_rawd, d_xd = E(B, Ho, Ho, pl), E(B, Hc, Hc, inpl)
            self.tensors.update({pfx + ".d_rawd": d_rawd, pfx + ".d_xd": d_xd})
            grp += self._bn_bwd(pfx + ".downsample.1", g2, None, rawd, d_rawd)[0]
            grp.append(self._wgrad(Ld, x, d_rawd, Hc, Hc, Ho, Ho, stride, 0, inpl, pl, inpl, pl, defer=li >= 3))
            grp.append(self._unpack(Ld))
            # d_x = gradient w.r.t. the previous layer's last block output (mask = x): its bn2 backward is reduced by the launch that writes d_x
            bnb = _bnb(f"backbone.layer{li - 1}.{RESNET34_LAYERS[li - 2] - 1}.bn2", prev_raw2, x) if e.gemm_bnb else None
            # (r6) conv1's data gradient, the shortcut conv's data gradient and the previous block's ReLU mask + bn2-backward sums as
            # ONE launch of the parity-class kernel: no d_xd tensor (three quarters zeros), no addend pass
            s2d = self._s2d(L1, "d", d_raw1, d_x, Ho, Hc, Ld=Ld, dyd=d_rawd, bnb=bnb) if bnb else None
            if s2d is not None:
                grp.append(s2d[0])
                del self.tensors[pfx + ".d_xd"]
            else:
                grp.append(self._conv(Ld, d_rawd, pl, d_xd, Ho, Ho, Hc, Hc, 2, 0, mode=1, w=Ld.wd, rows=Ld.rows_d, cin=Ld.cin_d, cout=inpl)[0])
                grp.append(self._conv(L1, d_raw1, pl, d_x, Ho, Ho, Hc, Hc, 2, 1, mode=1, w=L1.wd, rows=L1.rows_d, cin=L1.cin_d,
                                      cout=inpl, addend=d_xd, add_cs=inpl, bnb=bnb)[0])
        elif need_dx:
            # previous block of the same layer: d_x is the gradient w.r.t. its output (mask = x, stored) and
            # feeds its bn2 backward (raw input prev_raw2)
            fuse_prev = b >= 1 and self._fusable(L1)
            grp.append(self._conv(L1, d_a1 if xfb1 else d_raw1, pl, d_x, Ho, Ho, Hc, Hc, 1, 1, w=L1.wd, rows=L1.rows_d, cin=L1.cin_d, cout=inpl,
                                  addend=g2, add_cs=pl, bnb=_bnb(f"backbone.layer{li}.{b - 1}.bn2", prev_raw2, x) if fuse_prev else None, xf=xd1)[0])
        self.bwd_groups.append(grp)
        c.d_x = d_out

    def _head_convT(self, feat, d_feat, prev_raw2):
        """the geometric head's ConvTranspose2d + BatchNorm + ReLU on the backbone's output (backward group 17).  Returns the head cursor."""
        e, B, S, T, E = self.e, self.B, self.bn_train, self.has_backward, self._E
        h = "rot_head_net.features."
        LT = e.layers[h + "0"]
        rawt, h0 = E(B, 16, 16, 256), E(B, 16, 16, 256)
        self.tensors.update({h + "0.raw": rawt, h + "0.act": h0})
        xf_first = S and (not HEAD_CONVS[0][2]) and self._xf_ok(e.layers[h + str(HEAD_CONVS[0][0])])
        # (r6) the ConvTranspose's forward pass on the parity-class kernel (8 x 8 maps: two images per tile); the generic kernel keeps odd batch sizes
        if not S:
            f = e.fold(h + "1", LT)
            self._hook_fold()
            tf = self._s2d(LT, "e", feat, h0, 8, 16, bias=f.shift, act=1)
            self.fwd.append(tf[0] if tf is not None else
                            self._conv_bn_eval(LT, h + "1", feat, 512, h0, 8, 8, 16, 16, 2, 1, relu=True, mode=1, cin=512, cout=256))
        else:
            op, rows = self._s2d(LT, "f", feat, rawt, 8, 16, stats=self.stats) or \
                self._conv(LT, feat, 512, rawt, 8, 8, 16, 16, 2, 1, mode=1, cin=512, cout=256, stats=self.stats)
            self.fwd.append(op)
            self.fwd += self._bn_fwd(h + "1", rawt, rows, 256, B * 256, None if xf_first else h0)
        d_h0 = None
        if T:
            d_h0, d_rawt = E(B, 16, 16, 256), E(B, 16, 16, 256)
            self.tensors.update({h + "0.d_act": d_h0, h + "0.d_raw": d_rawt})
            pre_t = (not HEAD_CONVS[0][2]) and self._fusable(e.layers[h + str(HEAD_CONVS[0][0])])
            grp = self._bn_bwd(h + "1", d_h0, h0, rawt, d_rawt, affine_mask=True, sums="dgrad" if pre_t else "here")[0]
            # ConvT weight grad = conv wgrad with roles swapped: "input" d_rawt (16x16, 256), "output grad" feat (8x8, 512)
            grp.append(self._wgrad(LT, d_rawt, feat, 16, 16, 8, 8, 2, 1, 256, 512, 256, 512))
            grp.append(self._unpack(LT))
            # (r6) the ConvTranspose's data gradient = a stride-2 conv of the output gradient: the parity-plane kernel with the BatchNorm-backward epilogue
            bnb = _bnb("backbone.layer4.2.bn2", prev_raw2, feat) if e.gemm_bnb else None
            grp.append(((self._s2(LT, "d", d_rawt, d_feat, 16, 8, bnb=bnb) if bnb else None) or
                        self._conv(LT, d_rawt, 256, d_feat, 16, 16, 8, 8, 2, 1, mode=0, w=LT.wd, rows=LT.rows_d, cin=256, cout=512, bnb=bnb))[0])
            self.bwd_groups.append(grp)
        # pend_h: hx = relu(bn(prev_raw)) is evaluated (and written to hx) by the next head conv while it stages its patch
        pend_h = _pend(rawt, _xf_bn_relu(self.bn[h + "1"])) if xf_first else None
        return NS(hx=h0, d_hx=d_h0, Hh=16, prev_bn=h + "1", prev_raw=rawt, pend_h=pend_h, up_next=False)

    def _head_conv(self, c, hi):
        """head conv hi of HEAD_CONVS (3x3, 256 channels, BatchNorm, ReLU; an upsampling in front of two of them) behind the head cursor c"""
        e, lib, B, S, T, E = self.e, self.e.lib, self.B, self.bn_train, self.has_backward, self._E
        h = "rot_head_net.features."
        ci, bi, up = HEAD_CONVS[hi]
        hx, d_hx, Hh, prev_bn, prev_raw, pend_h = c.hx, c.d_hx, c.Hh, c.prev_bn, c.prev_raw, c.pend_h
        Lc = e.layers[h + str(ci)]
        grp = []
        fused_up = bool(up and c.up_next)
        xin, d_in, up_bwd = hx, d_hx, None
        if up:
            assert pend_h is None
            u = E(B, 2 * Hh, 2 * Hh, 256)
            self.tensors[h + f"{ci}.up"] = u
            sp_ = self.bn.get(prev_bn)
            if fused_up:
                # (r6) BatchNorm + ReLU of the previous conv evaluated by the upsampling itself (its activation tensor is never stored), and
                # in the backward pass the upsampling's adjoint also reduces that BatchNorm's backward sums: two launches and two tensor
                # round trips less per upsampling
                self.fwd.append(_launch(lib.gdrn_bn_relu_upsample2x_fwd, "bn_relu_upsample_fwd", (prev_raw, sp_.scale, sp_.shift, u, B, Hh, Hh, 256, e.dt)))
            else:
                self.fwd.append(_launch(lib.gdrn_upsample2x_fwd, "upsample_fwd", (hx, u, B, Hh, Hh, 256, e.dt)))
            if T:
                d_in = E(B, 2 * Hh, 2 * Hh, 256)
                self.tensors[h + f"{ci}.d_up"] = d_in
                if fused_up:
                    up_bwd = _launch(lib.gdrn_upsample2x_bwd_bnsums, "upsample_bwd_bnsums",
                                     (d_in, d_hx, prev_raw, sp_.mean, sp_.invstd, sp_.scale, sp_.shift, B, Hh, Hh, 256, self.stats, e.dt))
                else:
                    up_bwd = _launch(lib.gdrn_upsample2x_bwd, "upsample_bwd", (d_in, d_hx, B, Hh, Hh, 256, e.dt))
            xin, Hh = u, 2 * Hh
        raw, act = E(B, Hh, Hh, 256), E(B, Hh, Hh, 256)
        self.tensors[h + f"{ci}.raw"] = raw
        nxt = HEAD_CONVS[hi + 1] if hi + 1 < len(HEAD_CONVS) else None
        # this conv's BatchNorm + ReLU is applied by the next head conv on load when no upsampling sits in between
        xf_next = S and nxt is not None and not nxt[2] and self._xf_ok(e.layers[h + str(nxt[0])])
        # the NEXT conv sits behind an upsampling that applies this conv's BatchNorm + ReLU itself (see `fused_up` above)
        up_next = S and e.fuse_up and nxt is not None and nxt[2] and (T or not self.with_loss)
        if not S:
            self.fwd.append(self._conv_bn_eval(Lc, h + str(bi), xin, 256, act, Hh, Hh, Hh, Hh, 1, 1, relu=True))
        else:
            op, rows = self._conv(Lc, pend_h.x1 if pend_h else xin, 256, raw, Hh, Hh, Hh, Hh, 1, 1, stats=self.stats,
                                  xf=dict(pend_h.xf, out=xin) if pend_h else None)
            self.fwd.append(op)
            self.fwd += self._bn_fwd(h + str(bi), raw, rows, 256, B * Hh * Hh, None if (xf_next or up_next) else act)
        if not up_next:
            self.tensors[h + f"{ci}.act"] = act   # (behind a fused upsampling the activation is never stored)
        d_act = None
        if T:
            d_act, d_raw = E(B, Hh, Hh, 256), E(B, Hh, Hh, 256)
            self.tensors.update({h + f"{ci}.d_act": d_act, h + f"{ci}.d_raw": d_raw})
            # d_act is produced by the NEXT head conv's data gradient; when no upsampling sits in between, that
            # launch masks it and reduces this BN's backward sums
            pre = (not nxt[2] and self._fusable(e.layers[h + str(nxt[0])])) if nxt is not None else e.gemm_bnb  # (last conv: the 1x1 output conv's data gradient)
            xfb = self._xf_ok(Lc)  # this BN's backward apply inside Lc's data-gradient launch (mode 3, or 4 = with the ReLU mask)
            # (behind a fused upsampling, that launch's adjoint has reduced this BatchNorm's backward sums)
            ops, xd = self._bn_bwd(h + str(bi), d_act, act, raw, d_raw, affine_mask=True, xf=xfb,
                                   sums="dgrad" if pre else ("upsample" if up_next else "here"))
            grp += ops
            grp.append(self._wgrad(Lc, xin, d_raw, Hh, Hh, Hh, Hh, 1, 1, 256, 256, 256, 256))
            grp.append(self._unpack(Lc))
            fuse_in = (not up) and self._fusable(Lc)  # d_in is the gradient w.r.t. the previous BN+ReLU's output
            grp.append(self._conv(Lc, d_act if xfb else d_raw, 256, d_in, Hh, Hh, Hh, Hh, 1, 1, w=Lc.wd, rows=Lc.rows_d, cin=256, cout=256,
                                  bnb=_bnb(prev_bn, prev_raw, affine=True) if fuse_in else None, xf=xd)[0])
            if up_bwd is not None:
                grp.append(up_bwd)
            self.bwd_groups.append(grp)
        c.pend_h = _pend(raw, _xf_bn_relu(self.bn[h + str(bi)])) if xf_next else None
        c.hx, c.d_hx, c.Hh, c.prev_bn, c.prev_raw, c.up_next = act, d_act, Hh, h + str(bi), raw, up_next

    def _head_out(self, c):
        """the head's 1x1 output conv and the head tail (logits -> Patch-PnP input; with losses also the map-loss sums) behind the head
        cursor c (backward group 24)"""
        e, lib, B, T, WL, E = self.e, self.e.lib, self.B, self.has_backward, self.with_loss, self._E
        h, nreg = "rot_head_net.features.", e.nreg
        hx, d_hx, prev_bn, prev_raw = c.hx, c.d_hx, c.prev_bn, c.prev_raw
        LO = e.layers[h + "23"]
        M = B * 64 * 64
        self.hs = 72
        self.head_out = E(M, self.hs, dtype=F32t)
        bias_o = e.P[h + "23.bias"]
        # 64 regions, 16-bit: the 1x1 output conv and the head tail as ONE kernel (gdrn_head_conv_tail_fwd; with losses gdrn_head_conv_tail_loss_fwd,
        # which also accumulates the map-loss sums) -- the fp32 logits still go to head_out (the backward pass and callers that return the maps
        # read them), but the forward pass does not read them back
        fused_tail = e.h16 and nreg == 64
        if not fused_tail:
            self.fwd.append(self._conv(LO, hx, 256, self.head_out, 64, 64, 64, 64, 1, 0, bias=bias_o, out_f32=1, y_cs=self.hs, cout=e.head_c)[0])
        self.pnp_in = e._zeros(M, 128)   # channels >= 5 + nreg stay zero (PREZEROED: the kernels do not re-write the pad)
        self.keep.append(self.pnp_in)
        self.tensors.update({"head_out": self.head_out, "pnp_in": self.pnp_in})
        if WL:
            # map-loss sums: totals in acc[0..7], behind them one partial row per workgroup of the kernel (ACC_ROWS: stored, then added in a fixed
            # order by gdrn_loss_finalize -- no memset launch, no atomics, run-to-run identical losses)
            self.acc_rows = int(lib.gdrn_head_conv_tail_loss_rows(B, 4096) if fused_tail else lib.gdrn_head_tail_loss_rows(B, 4096, nreg, self.hs, 128))
            if self.acc_rows <= 0:
                check(self.acc_rows or -1, "head_tail_loss_rows")
            self.acc = E(8 + 8 * self.acc_rows, dtype=torch.float64)
            self.losses = e._zeros(8, dtype=F32t)
        if fused_tail and WL:
            def head_conv_tail(st, ctx):
                check(lib.gdrn_head_conv_tail_loss_fwd(ptr(hx), 256, ptr(LO.wf), LO.rows_f, ptr(bias_o), ctx["coord2d"], ctx["extents"], ptr(self.head_out), self.hs,
                                                       ptr(self.pnp_in), 128, ctx["gt_xyz"], ctx["mask_visib"], ctx["mask_trunc"], ctx["gt_region"], ptr(self.acc),
                                                       B, 4096, nreg, e.dt | PREZEROED, st), "head_conv_tail_loss_fwd")

            head_conv_tail.meta = dict(kernel="head_conv_tail64_kernel<bf16,true>", flops=2.0 * M * 256 * e.head_c, layer=h + "23+tail+losses")
            self.fwd.append(head_conv_tail)
        elif fused_tail:
            def head_conv_tail(st, ctx):
                # ctx["want_maps"] False (GDRN.forward without cfg.TEST.USE_PNP): nobody reads the logits -- head = NULL saves their 75 MB at bs = 64
                # (head_valid: does plan.head_out hold THIS forward's logits?  readers -- GDRN._maps, tools -- assert it: ADVICE r5)
                self.head_valid = bool(ctx.get("want_maps", True))
                check(lib.gdrn_head_conv_tail_fwd(ptr(hx), 256, ptr(LO.wf), LO.rows_f, ptr(bias_o), ctx["coord2d"], ctx["extents"],
                                                  ptr(self.head_out) if ctx.get("want_maps", True) else None, self.hs,
                                                  ptr(self.pnp_in), 128, B, 4096, nreg, e.dt | PREZEROED, st), "head_conv_tail_fwd")

            head_conv_tail.meta = dict(kernel="head_conv_tail64_kernel<bf16,false>", flops=2.0 * M * 256 * e.head_c, layer=h + "23+tail")
            self.fwd.append(head_conv_tail)
        elif WL:
            # head tail + map-loss sums in one pass over the logits (train mode)
            self.fwd.append(lambda st, ctx: check(lib.gdrn_head_tail_loss_fwd(ptr(self.head_out), self.hs, ctx["coord2d"], ctx["extents"], ptr(self.pnp_in), 128,
                                                                              ctx["gt_xyz"], ctx["mask_visib"], ctx["mask_trunc"], ctx["gt_region"], ptr(self.acc),
                                                                              B, 4096, nreg, e.dt | PREZEROED | ACC_ROWS, st), "head_tail_loss_fwd"))
        else:
            self.fwd.append(lambda st, ctx: check(lib.gdrn_head_tail_fwd(ptr(self.head_out), self.hs, ctx["coord2d"], ctx["extents"],
                                                                         ptr(self.pnp_in), 128, B, 4096, nreg, e.dt | PREZEROED, st), "head_tail_fwd"))
        if not T:
            return
        self.d_head = e._zeros(M, 128)   # pad channels zero-filled once (PREZEROED)
        self.keep.append(self.d_head)
        self.d_pnp_in = E(M, 128)
        self.gw = e._zeros(8, dtype=F32t)
        self.tensors.update({"d_head": self.d_head, "d_pnp_in": self.d_pnp_in})
        grp = [lambda st, ctx: check(lib.gdrn_head_tail_bwd(ptr(self.head_out), self.hs, ptr(self.pnp_in), ptr(self.d_pnp_in), 128,
                                                            ctx["extents"], ctx["gt_xyz"], ctx["mask_visib"], ctx["mask_trunc"],
                                                            ctx["gt_region"], ptr(self.acc), ptr(self.gw), ptr(self.d_head), 128, B,
                                                            4096, nreg, e.dt | PREZEROED, st), "head_tail_bwd")]
        grp.append(self._wgrad(LO, hx, self.d_head, 64, 64, 64, 64, 1, 0, 256, e.head_c, 256, 128))
        grp.append(self._unpack(LO))
        gb = e.grads[h + "23.bias"]
        self.grad_group[h + "23.bias"] = len(self.bwd_groups)
        self._zero_regions.append(self._grad16(gb))
        grp.append(self._side(_launch(lib.gdrn_bias_grad, "bias_grad", (self.d_head, 128, M, e.head_c, gb, e.dt | PREZEROED))))
        if e.h16 and e.gemm_bnb:
            # the 1x1 output conv's data gradient on its own kernel (K = 69: the generic 128 x 128 tile ran it at 83 TFLOP/s), with the ReLU mask and
            # the BatchNorm-backward sums of the head's last BatchNorm in the epilogue as the generic kernel's bnb_* epilogue has them
            sbp = self.bn[prev_bn]
            head_dgrad = _launch(lib.gdrn_head_out_dgrad, "head_out_dgrad", (self.d_head, 128, LO.wd, LO.cin_d, prev_raw, 256, sbp.mean, sbp.invstd, sbp.scale,
                                                                             sbp.shift, d_hx, 256, self.stats, B, 4096, e.dt),
                                 self._meta("head_out_dgrad64_kernel<bf16>", self._macs(LO, 4096), M * (128 + 256 + 256) * 2, h + "23:dgrad"))
            grp.append(self._with_coef(head_dgrad, prev_bn, int(lib.gdrn_head_out_dgrad_rows(B, 4096))))
        else:
            grp.append(self._conv(LO, self.d_head, 128, d_hx, 64, 64, 64, 64, 1, 0, w=LO.wd, rows=LO.rows_d, cin=128, cout=256,
                                  bnb=_bnb(prev_bn, prev_raw, affine=True) if e.gemm_bnb else None)[0])
        self.bwd_groups.append(grp)

    def _pnp_conv(self, c, ci, gi):
        """Patch-PnP conv ci (3x3 stride 2) + GroupNorm gi + ReLU behind the Patch-PnP cursor c"""
        e, lib, B, E = self.e, self.e.lib, self.B, self._E
        q = "pnp_net.features."
        px, d_px, Hp, cin = c.px, c.d_px, c.Hp, c.cin
        Lc = e.layers[q + str(ci)]
        Ho = Hp // 2
        r, gact = E(B, Ho, Ho, 128), E(B, Ho, Ho, 128)
        mr = E(B, 32, 2, dtype=F32t)
        self.tensors.update({q + f"{ci}.raw": r, q + f"{ci}.act": gact})
        s2_ok = cin == Lc.cin_f   # (r6: the parity-plane / parity-class kernels where they cover the map)
        self.fwd.append(((self._s2(Lc, "f", px, r, Hp, Ho) if s2_ok else None) or self._conv(Lc, px, cin, r, Hp, Hp, Ho, Ho, 2, 1, cin=cin, cout=128))[0])
        gam, bet = e.P[q + f"{gi}.weight"], e.P[q + f"{gi}.bias"]
        self.fwd.append(_launch(lib.gdrn_gn_relu_fwd, "gn_relu_fwd", (r, gam, bet, gact, mr, B, Ho * Ho, 128, 32, 1e-5, e.dt)))
        d_g = None
        if self.has_backward:
            d_g, d_r = E(B, Ho, Ho, 128), E(B, Ho, Ho, 128)
            self.tensors.update({q + f"{ci}.d_act": d_g, q + f"{ci}.d_raw": d_r})
            dgam, dbet = e.grads[q + f"{gi}.weight"], e.grads[q + f"{gi}.bias"]
            self.grad_group[q + f"{gi}.weight"] = self.grad_group[q + f"{gi}.bias"] = len(self.bwd_groups)
            grp = [_launch(lib.gdrn_gn_relu_bwd, "gn_relu_bwd", (d_g, gact, r, gam, mr, d_r, dgam, dbet, B, Ho * Ho, 128, 32, e.dt | PREZEROED))]
            self._zero_regions += [self._grad16(dgam), self._grad16(dbet)]
            grp.append(self._wgrad(Lc, px, d_r, Hp, Hp, Ho, Ho, 2, 1, cin, 128, cin, 128))
            grp.append(self._unpack(Lc))
            grp.append(((self._s2d(Lc, "d", d_r, d_px, Ho, Hp) if s2_ok else None) or
                        self._conv(Lc, d_r, 128, d_px, Ho, Ho, Hp, Hp, 2, 1, mode=1, w=Lc.wd, rows=Lc.rows_d, cin=128, cout=cin))[0])
            self.bwd_groups.append(grp)
        c.px, c.d_px, c.Hp, c.cin = gact, d_g, Ho, 128

    def _fc_fwd(self, g2act):
        """fc1, fc2 and fc_r | fc_t on the last Patch-PnP activation g2act.  Returns the activations (f1, f2)."""
        e, lib, B, E = self.e, self.e.lib, self.B, self._E
        L1, L2, L3 = e.layers["pnp_net.fc1"], e.layers["pnp_net.fc2"], e.layers["pnp_net.fc_rt"]
        f1, f2 = E(B, 1024), E(B, 256)
        self.fc_out = e._zeros(B, 64, dtype=F32t)   # (columns 9 .. 63 are never written)
        self.keep.append(self.fc_out)
        self.tensors.update({"pnp_net.fc1.act": f1, "pnp_net.fc2.act": f2, "fc_out": self.fc_out})
        b1, b2 = e.P["pnp_net.fc1.bias"], e.P["pnp_net.fc2.bias"]
        if e.h16 and B <= 64:
            # fc1 is bound by reading its 16.8 MB of weights once: split-K skinny GEMM instead of 8 gather workgroups.
            # L1.wf = [1024 rows][64 taps][128 ch] = row-major [N][K] in the (pixel, channel) order of the NHWC input
            ws1 = e._zeros(16 * B * 1024 + 64, dtype=F32t)  # GDRN_LINEAR_MAX_SPLITS slabs + tickets
            self.keep.append(ws1)
            self.fwd.append(_launch(lib.gdrn_linear_splitk, "linear_splitk fc1", (g2act, L1.wf, b1, f1, B, 8192, 1024, 8192, 8192, 1024, 2, ws1, e.dt),
                                    dict(kernel="linear_splitk_kernel", flops=2.0 * B * 8192 * 1024, layer="pnp_net.fc1")))
            # fc2 (64 x 1024 -> 256) on the gather kernel is two workgroups walking K = 1024 serially (20 us for 34 MFLOP): the same split-K
            # kernel, 16 column tiles x 8 K ranges (r4)
            ws2 = e._zeros(16 * B * 256 + 64, dtype=F32t)
            self.keep.append(ws2)
            # (r6) fc2's finish pass (bias, LeakyReLU), fc_r | fc_t and the pose decode are ONE launch (gdrn_pose_loss, fc2_ws): fc2 leaves its slabs
            self.fc_tail = (ws2, int(lib.gdrn_linear_splits(1024, 256))) if e.fc_tail else None
            self.fwd.append(_launch(lib.gdrn_linear_splitk, "linear_splitk fc2",
                                    (f1, L2.wf, b2, f2, B, 1024, 256, 1024, 1024, 256, -1 if self.fc_tail else 2, ws2, e.dt),
                                    dict(kernel="linear_splitk_kernel", flops=2.0 * B * 1024 * 256, layer="pnp_net.fc2")))
        else:
            self.fwd.append(self._conv(L1, g2act, 128, f1, 8, 8, 1, 1, 1, 0, bias=b1, act=2, cin=128, cout=1024)[0])
            self.fwd.append(self._conv(L2, f1, 1024, f2, 1, 1, 1, 1, 1, 0, bias=b2, act=2, cin=1024, cout=256)[0])
        if self.fc_tail is None:
            self.fwd.append(self._conv(L3, f2, 256, self.fc_out, 1, 1, 1, 1, 1, 0, bias=e.rt_b, out_f32=1, cin=256, cout=9, y_cs=64)[0])
        self._fc2 = (f2, b2, L3)
        return f1, f2

    def _fc_bwd(self, g2act, d_g2, f1, f2):
        """backward group 28: dL/dfc from the three pose losses, then fc_r | fc_t, fc2, fc1 -- d_g2 is the gradient of g2act"""
        e, lib, B, E = self.e, self.e.lib, self.B, self._E
        L1, L2, L3 = e.layers["pnp_net.fc1"], e.layers["pnp_net.fc2"], e.layers["pnp_net.fc_rt"]
        self.dfc3 = e._zeros(3, B, 64, dtype=F32t)
        d_fc32 = e._zeros(B, 64, dtype=F32t)
        d_fc = E(B, 64)
        d_f2, d_f2p, d_f1, d_f1p = E(B, 256), E(B, 256), E(B, 1024), E(B, 1024)
        self.tensors.update({"d_fc": d_fc, "pnp_net.fc2.d_act": d_f2, "pnp_net.fc2.d_pre": d_f2p, "pnp_net.fc1.d_act": d_f1, "pnp_net.fc1.d_pre": d_f1p})
        o_rt = e.grad_offsets["pnp_net.fc_r.bias"]   # the two bias gradients' shared slot of the flat gradient buffer (Engine.__init__)
        assert e.grad_offsets["pnp_net.fc_t.bias"] == o_rt + 6 and o_rt % 4 == 0
        self._rt_gb_full = e.grad_flat[o_rt:o_rt + 12]
        self.rt_gb = self._rt_gb_full[:9]
        self._zero_regions += [self._rt_gb_full, self._grad16(e.grads["pnp_net.fc1.bias"]), self._grad16(e.grads["pnp_net.fc2.bias"])]
        g_b1, g_b2 = e.grads["pnp_net.fc1.bias"], e.grads["pnp_net.fc2.bias"]
        for n_ in ("pnp_net.fc1.bias", "pnp_net.fc2.bias", "pnp_net.fc_r.bias", "pnp_net.fc_t.bias"):
            self.grad_group[n_] = len(self.bwd_groups)
        # (skipped when the forward pass was seeded: gdrn_pose_loss has then written dL/dfc itself -- ctx["seeded"], GDRN.train_step)
        comb = _launch(lib.gdrn_combine3, "combine3", (self.dfc3, self.gw.data_ptr() + 20, d_fc32, B * 64))
        cast = _launch(lib.gdrn_cast_from_f32, "cast", (d_fc32, d_fc, B * 64, e.dt))
        comb.seed = cast.seed = True
        self.d_fc = d_fc
        bias_grad = lambda d, cs, n, g: _launch(lib.gdrn_bias_grad, "bias_grad", (d, cs, B, n, g, e.dt | PREZEROED))
        grp = [
            comb,
            cast,
            self._wgrad(L3, f2, d_fc, 1, 1, 1, 1, 1, 0, 256, 9, 256, 64, defer=True),
            self._unpack(L3),
            bias_grad(d_fc, 64, 9, self.rt_gb),   # = both .grad views
        ]
        grp.append(self._conv(L3, d_fc, 64, d_f2, 1, 1, 1, 1, 1, 0, w=L3.wd, rows=L3.rows_d, cin=64, cout=256)[0])
        grp.append(_launch(lib.gdrn_leaky_bwd, "leaky_bwd", (d_f2, f2, d_f2p, B * 256, e.dt)))
        grp.append(self._wgrad(L2, f1, d_f2p, 1, 1, 1, 1, 1, 0, 1024, 256, 1024, 256, defer=True))
        grp.append(self._unpack(L2))
        grp.append(self._side(bias_grad(d_f2p, 256, 256, g_b2), defer=True))
        grp.append(self._conv(L2, d_f2p, 256, d_f1, 1, 1, 1, 1, 1, 0, w=L2.wd, rows=L2.rows_d, cin=256, cout=1024)[0])
        grp.append(_launch(lib.gdrn_leaky_bwd, "leaky_bwd", (d_f1, f1, d_f1p, B * 1024, e.dt)))
        grp.append(self._wgrad(L1, g2act, d_f1p, 8, 8, 1, 1, 1, 0, 128, 1024, 128, 1024, defer=True))
        grp.append(self._unpack(L1))
        grp.append(self._side(bias_grad(d_f1p, 1024, 1024, g_b1), defer=True))
        if e.h16 and B <= 64 and e.fc_tail:
            # (r6) fc1's data gradient is bound by reading its 16.8 MB operand once, like its forward pass: the split-K skinny GEMM (L1.wd =
            # [8192 rows = (pixel, channel)][1024] row-major) instead of 64 gather workgroups walking K = 1024 each (39 us -> 15 + 7)
            ws1d = e._zeros(16 * B * 8192 + 64, dtype=F32t)
            self.keep.append(ws1d)
            grp.append(_launch(lib.gdrn_linear_splitk, "linear_splitk fc1:dgrad", (d_f1p, L1.wd, None, d_g2, B, 1024, 8192, 1024, 1024, 8192, 0, ws1d, e.dt),
                               dict(kernel="linear_splitk_kernel", flops=2.0 * B * 8192 * 1024, layer="pnp_net.fc1:dgrad")))
        else:
            grp.append(self._conv(L1, d_f1p, 1024, d_g2, 1, 1, 1, 1, 1, 0, w=L1.wd, rows=L1.rows_d, cin=1024, cout=8192, KH=1, KW=1, y_cs=8192)[0])
        self.bwd_groups.append(grp)

    def _pose(self):
        """pose decode (+ the pose losses and, with losses, the finalize launch of all eight) from fc_out and the per-RoI context"""
        e, lib, B, T, WL = self.e, self.e.lib, self.B, self.has_backward, self.with_loss
        self.rot = self._E(B, 3, 3, dtype=F32t)
        self.trans = self._E(B, 3, dtype=F32t)
        self.vis = e._zeros(B, 2, dtype=F32t)
        self.pose_p = PoseParams()

        def pose(st, ctx):
            pp = self.pose_p
            pp.fc, pp.fs = ptr(self.fc_out), 64
            pp.cams, pp.centers, pp.whs, pp.ratios, pp.extents = ctx["cams"], ctx["centers"], ctx["whs"], ctx["ratios"], ctx["extents"]
            pp.gt_rot, pp.gt_trans, pp.gt_trans_ratio = ctx.get("gt_rot"), ctx.get("gt_trans"), ctx.get("gt_trans_ratio")
            pp.points, pp.npts = ctx.get("points"), ctx.get("npts", 0)
            pp.sym, pp.sym_count, pp.Kmax = ctx.get("sym"), ctx.get("sym_count"), ctx.get("Kmax", 0)
            pp.N, pp.train = B, 1 if WL else 0
            pp.rot, pp.trans = ptr(self.rot), ptr(self.trans)
            pp.losses = (self.losses.data_ptr() + 20) if WL else None
            pp.dfc = ptr(self.dfc3) if T else None
            pp.vis = ptr(self.vis) if WL else None
            pp.loss_rows = ptr(self.pose_rows)
            seeded = bool(T and WL and e.h16 and ctx.get("seeded"))   # the fused train step: dL/dloss is known now, dL/dfc leaves this launch
            pp.gw, pp.dfc_comb = ((self.gw.data_ptr() + 20), ptr(self.d_fc)) if seeded else (None, None)
            if self.fc_tail is not None:
                f2_, b2_, L3_ = self._fc2
                pp.fc2_ws, pp.fc2_splits, pp.fc2_bias, pp.f2_out = ptr(self.fc_tail[0]), self.fc_tail[1], ptr(b2_), ptr(f2_)
                pp.w_rt, pp.b_rt, pp.fc_w = ptr(L3_.wf), ptr(e.rt_b), ptr(self.fc_out)
            check(lib.gdrn_pose_loss(C.byref(pp), st), "pose_loss")

        self.fwd.append(pose)
        if WL:
            self.pose_rows = self._E(B, 4, dtype=F32t)
            # ctx["loss_w"] / ctx["weighted"] (device pointers, the fused train step): the weighted loss vector it returns, written here
            self.fwd.append(lambda st, ctx: check(lib.gdrn_loss_finalize(ptr(self.acc), self.acc_rows, B, 4096, ptr(self.pose_rows), ptr(self.losses),
                                                                         ctx.get("loss_w"), ctx.get("weighted"), st), "loss_finalize"))

    # ---- execution ---------------------------------------------------------------------------
    def run_forward(self, ctx):
        e = self.e
        if e.dry:
            raise cabi.GdrnHipError("dry (build-only) engine: there is no CPU execution path")
        st = e._stream()
        self.generation += 1
        if self.bn_train:
            e.bn_epoch += 1  # the kernels update the running statistics behind autograd's back
        elif self.eval_prep:
            sig = (e.bn_epoch, tuple(t._version for t in e.P.values()), tuple(t._version for t in e.Bf.values()))
            if sig != self._eval_sig:
                for op in self.eval_prep:
                    op(st, ctx)
                self._eval_sig = sig
        for op in self.fwd:
            op(st, ctx)

    def run_backward(self, ctx, on_bucket=None):
        """ctx as in forward; self.gw must hold dL/dloss_k.  on_bucket(i) is called after the ops that
        complete gradient bucket i have been enqueued (used to overlap the RCCL all-reduce)."""
        e = self.e
        if e.dry:
            raise cabi.GdrnHipError("dry (build-only) engine: there is no CPU execution path")
        main = torch.cuda.current_stream(e.dev)
        st = main.cuda_stream
        ztab, zst, znt, znb = self._zero_tab
        check(e.lib.gdrn_zero_multi(ptr(ztab), ptr(zst), znt, znb, st), "zero_multi")
        marks = self._bucket_marks() if on_bucket is not None else {}
        # The bucket-end work (grouped weight gradients, their reduction, gradient unpack) only feeds the optimizer /
        # the RCCL exchange: it goes to a second stream behind an event, so the next bucket's dependent chain of short
        # data-gradient / BatchNorm kernels (one workgroup per CU on the small feature maps) shares the CUs with it.
        side = e.side_stream() if e.wgrad_stream else None
        used_side = in_side = False
        probe = self.op_events   # bench.py: [(start, end, meta, on_side)] HIP events around the conv launches of THIS pass
        seeded = bool(ctx.get("seeded")) and self.e.h16
        for i, op in enumerate(self.bwd):
            if seeded and getattr(op, "seed", False):
                continue   # dL/dfc was written by the forward pass's pose kernel
            if probe is not None and getattr(op, "meta", None) is not None:
                op = _probed(op, probe)
            if side is not None and getattr(op, "side", False):
                if not in_side:
                    side.wait_stream(main)  # everything enqueued so far on the main stream
                    in_side = used_side = True
                op(side.cuda_stream, ctx)
                if i in marks:
                    with torch.cuda.stream(side):
                        on_bucket(marks[i])
            else:
                in_side = False
                op(st, ctx)
                if i in marks:
                    if used_side:     # the bucket's side-stream work (weight-gradient reduction) is part of the bucket
                        side.wait_stream(main)
                        with torch.cuda.stream(side):
                            on_bucket(marks[i])
                    else:
                        on_bucket(marks[i])
        if used_side:
            main.wait_stream(side)  # the optimizer (or the caller) sees complete gradients on the main stream

    def walk_backward(self, on_bucket, before_bucket=None):
        """The backward launch list WITHOUT launching (works on a dry engine): calls before_bucket(i) / on_bucket(i) where
        run_backward calls on_bucket(i), i.e. behind the last op of gradient bucket i.  Returns [(op index, bucket)] in call order.
        For the CPU tests of the data-parallel protocol (tests/test_dist_cpu.py)."""
        marks = self._bucket_marks()
        fired = []
        for i, op in enumerate(self.bwd):
            if i in marks:
                if before_bucket is not None:
                    before_bucket(marks[i])
                on_bucket(marks[i])
                fired.append((i, marks[i]))
        return fired

    def _bucket_marks(self):
        """index of the last backward op of each gradient bucket (pnp | head | layer4 | layer3 | rest)."""
        if self._marks is not None:
            return self._marks
        n_groups = len(self.bwd_groups)
        sizes = [len(g) for g in reversed(self.bwd_groups)]
        # groups in forward order: stem(1) + 16 blocks + convT(1) + 6 head convs + head out(1) + 3 pnp convs + fc(1)
        cum, ends = 0, []
        for s in sizes:
            cum += s
            ends.append(cum - 1)
        # reversed order: fc, pnp x3 | head-out, head convs x6, convT | layer4 (3) | layer3 (6) | layer2 (4), layer1 (3), stem
        bounds = [n_groups - g0 for g0 in self.e.bucket_first_group]
        self._marks = {ends[b - 1]: i for i, b in enumerate(bounds)}
        return self._marks
