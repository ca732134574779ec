"""Forward / backward executor of GDR-Net's per-RoI hot path on the HIP kernels of libgdrn_hip.so.

The reference runs this path as ~150 ATen ops forward and their autograd backward
(core/gdrn_modeling/models/GDRN.py:110-306, resnet_backbone.py:69-80,
cdpn_rot_head_region.py:182-193, conv_pnp_net.py:111-157).  Here the fixed graph is compiled once per
(batch size, mode) into a *plan*: statically allocated NHWC buffers plus two flat lists of
pre-bound C-ABI calls (forward, backward).  Running a plan is a tight loop of ctypes calls on the
current HIP stream -- no allocation, no host synchronisation, graph-capturable.

Only PyTorch facilities used: device memory (torch.empty), streams, autograd glue.  No ATen compute
op touches activations.

This module: the Engine -- per-model state shared by every plan (packed operand copies of the weights, the flat gradient buffer and its
buckets, the side stream, the switches).  The per-batch-size launch lists live in plan.py (class Plan).
"""
import ctypes as C
import math
from collections import OrderedDict
from types import SimpleNamespace as NS

import torch

from . import cabi
from .cabi import BF16, F16, F32, check, ptr
from .switches import read

RESNET34_LAYERS = (3, 4, 6, 3)
RESNET34_PLANES = (64, 128, 256, 512)
HEAD_CONVS = ((3, 4, False), (6, 7, False), (10, 11, True), (13, 14, False), (17, 18, True), (20, 21, False))
# lowest forward-order backward-group index of the gradient buckets, and the last parameter (forward order) of each bucket but the
# last.  Data-parallel runs exchange five buckets pnp | head | layer4 | layer3 | rest (the 52 MB layer4 all-reduce starts nine blocks
# before the end of backward, the exposed tail is 5 MB); one GPU keeps layer4 + layer3 together: the grouped weight-gradient launch of
# a bucket wants ~1000 workgroups, and splitting it costs 0.13 ms per step for nothing when there is no exchange to overlap.
BUCKET_LAYOUTS = {
    5: ((25, 17, 14, 8, 0), ("rot_head_net.features.23.bias", "backbone.layer4.2.bn2.bias", "backbone.layer3.5.bn2.bias", "backbone.layer2.3.bn2.bias")),
    4: ((25, 17, 8, 0), ("rot_head_net.features.23.bias", "backbone.layer4.2.bn2.bias", "backbone.layer2.3.bn2.bias")),
}
LOSS_NAMES = ("loss_coor_x", "loss_coor_y", "loss_coor_z", "loss_mask", "loss_region", "loss_PM_R", "loss_centroid", "loss_z")


def _ru(a, b):
    return (a + b - 1) // b * b


class Engine:
    """Owns the packed (kernel-layout) weight copies and the per-batch-size plans for one GDRN module."""

    @property
    def bn_epoch(self):
        return self._bn_cell[0]

    @bn_epoch.setter
    def bn_epoch(self, v):
        self._bn_cell[0] = v

    def __init__(self, params, buffers, dtype="bf16", num_regions=64, dry=False, bn_cell=None):
        """params / buffers: dict name -> tensor with the reference's state_dict names.
        dry: build-only engine on host tensors for inspecting the launch lists without a GPU (tests); it cannot run."""
        # -- arithmetic and device.  dtype: "bf16" | "fp16" | "fp32"; the 16-bit modes run the same kernels out of two builds of the library (cabi.load)
        self.dt = {"bf16": BF16, BF16: BF16, "fp16": F16, "f16": F16, F16: F16}.get(dtype, F32)
        if self.dt == F32 and dtype not in ("fp32", "f32", F32):
            raise ValueError(f"HIP_DTYPE {dtype!r}: one of bf16, fp16, fp32")
        self.h16 = self.dt != F32          # 16-bit storage / MFMA operands (throughput modes)
        self.lib = cabi.load(self.dt)
        self.P, self.Bf = params, buffers
        self.tdt = {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32}[self.dt]
        self.esz = 2 if self.h16 else 4
        self.dev = next(iter(params.values())).device
        self.dry = bool(dry)
        if self.dev.type != "cuda" and not self.dry:
            raise cabi.GdrnHipError("the HIP engine needs parameters on a GPU device (no CPU fallback)")
        self.nreg = num_regions
        # -- the switches (switches.TABLE has one line on each, DESIGN.md section 4 what each was measured against), read HERE: an engine keeps
        # the values it was built with.  Operand transforms and the fused epilogues exist for the 16-bit formats only
        scale, dynamic, self.loss_scale_growth = read("GDRN_LOSS_SCALE")
        self._ls_host = scale if self.dt == F16 else 1.0   # static factor on dL/dloss, divided out where the optimizer reads the gradients
        self.loss_scale_dynamic = self.dt == F16 and dynamic
        self.ls_state = None   # LossScaleState, made by the first step that needs it (loss_scale_dev)
        hf = read("GDRN_HALO_F32")
        self.use_halo = self.h16 or hf != "0"
        self.halo_min_b = 1 if (self.h16 or hf == "1") else 32
        self.halo_waves = read("GDRN_HALO_WAVES")
        self.v3_policy, self.v3_min_wg = read("GDRN_V3")   # (the library reads no environment: the policy travels in gdrn_conv_params)
        ws = read("GDRN_WGRAD_STREAM")
        self.wgrad_stream, self.wgrad_force_lds = ws == "1", ws == "serial"
        self.wgrad_blocks = 1536 if ws == "0" else 768   # target workgroups of a grouped weight-gradient launch: three rounds of what is resident
        self.wgrad_side_lds = 84 * 1024                  # a side-stream weight-gradient launch asks for one workgroup per CU
        self.fuse_up = self.h16 and read("GDRN_FUSE_UP")
        self.fc_tail = self.h16 and read("GDRN_FC_TAIL")
        self.fuse_xf = self.h16 and read("GDRN_FUSE_XF")
        self.gemm_bnb = self.h16 and read("GDRN_GEMM_BNB")
        self.stem_direct = self.h16   # the dedicated stem kernels, forward and (fused with bn1's backward apply) weight gradient
        self.stem_w32 = torch.zeros(64 * 7 * 32, dtype=self.tdt, device=self.dev) if self.stem_direct else None
        nb = read("GDRN_BUCKETS")
        self.buckets_from_env = nb is not None
        if nb is None:
            import torch.distributed as _dist

            nb = 5 if (_dist.is_available() and _dist.is_initialized() and _dist.get_world_size() > 1) else 4
        self.bucket_first_group, self.bucket_marks = BUCKET_LAYOUTS[nb]
        self.max_plans = read("GDRN_MAX_PLANS")
        # -- layers, plans, gradients
        self.layers = OrderedDict()
        self._versions = {}
        self.bn_fold = {}  # bn key -> NS(scale, shift, layer): eval-mode BatchNorm folded into the preceding conv (every eval plan)
        # bumped by every training forward (running statistics changed).  Shared by the engines of one model (bn_cell; ADVICE r4: the fp16
        # inference engine of cfg.TEST.AMP_TEST must see the statistics its bf16 training twin moved through raw pointers)
        self._bn_cell = bn_cell if bn_cell is not None else [0]
        self._build_layers()
        self.plans = OrderedDict()   # (batch size, train-mode BatchNorm, losses) -> Plan, least recently used first
        self.plan_builds = 0
        self.param_names = list(self.P.keys())
        self._grad_layout()

    def _grad_layout(self):
        """the flat fp32 gradient buffer, ordered by backward completion (reverse of forward order), every parameter's view into it, the buckets"""
        self.grad_offsets = {}
        off = 0
        # fc_r | fc_t run as ONE 9-row layer (fc_rt): their bias gradients share one slot, fc_t's right behind fc_r's, so that the layer's single
        # bias_grad launch writes both in place (every reader -- Ranger, the collectives, .grad -- takes offset + numel, not padded rows)
        rb, tb = "pnp_net.fc_r.bias", "pnp_net.fc_t.bias"
        paired = rb in self.P and tb in self.P
        for n in reversed(self.param_names):
            if paired and n in (rb, tb):
                if rb not in self.grad_offsets:
                    self.grad_offsets[rb] = off
                    self.grad_offsets[tb] = off + self.P[rb].numel()
                    off += _ru(self.P[rb].numel() + self.P[tb].numel(), 4)
                continue
            self.grad_offsets[n] = off
            off += _ru(self.P[n].numel(), 4)
        self.grad_flat = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.grads = {n: self.grad_flat[self.grad_offsets[n]: self.grad_offsets[n] + self.P[n].numel()].view(self.P[n].shape)
                      for n in self.param_names}
        self.bucket_bounds = self._bucket_bounds()

    def grad_map(self):
        """parameter -> its gradient view in the flat buffer, what the optimizers take as `grads=` (built on each call)"""
        return {self.P[n]: self.grads[n] for n in self.param_names}

    # ------------------------------------------------------------------------------------------ fp16 loss scale
    @property
    def loss_scale(self):
        """the loss scale on dL/dloss (1 for bf16 / fp32).  Dynamic mode: read back from the device state -- a host synchronisation, not for the step's hot path"""
        if self.ls_state is not None:
            self._ls_host = self.ls_state.read()["scale"]
        return self._ls_host

    @loss_scale.setter
    def loss_scale(self, v):
        self._ls_host = float(v)
        if self.ls_state is not None:
            self.ls_state.write(scale=float(v))

    @property
    def loss_scale_skipped(self):
        return self.ls_state.read()["skipped"] if self.ls_state is not None else 0

    @property
    def loss_scale_good(self):
        return self.ls_state.read()["good"] if self.ls_state is not None else 0

    def loss_scale_dev(self):
        """the device-resident loss-scale state of the dynamic fp16 mode (None otherwise)"""
        if not self.loss_scale_dynamic or self.dry:
            return None
        if self.ls_state is None:
            self.ls_state = LossScaleState(self.dev, self._ls_host, self.loss_scale_growth)
        return self.ls_state

    def set_bucket_layout(self, nb):
        """switch the gradient bucket layout (4: one GPU, 5: data parallel -- the layer4 exchange starts earlier) after construction:
        dist.attach() calls this when the process group was created after the engine.  Plans are rebuilt (the grouped weight-gradient
        launches follow the buckets)."""
        if nb not in BUCKET_LAYOUTS:
            raise ValueError(f"bucket layout {nb!r}: choose 4 or 5")
        if (self.bucket_first_group, self.bucket_marks) == BUCKET_LAYOUTS[nb]:
            return False
        self.bucket_first_group, self.bucket_marks = BUCKET_LAYOUTS[nb]
        self.bucket_bounds = self._bucket_bounds()
        self._bucket_of = None
        if hasattr(self, "_pack_tasks"):
            self._pack_dirty = True   # the per-bucket operand-copy tables (repack_bucket) follow the buckets: rebuilt by the next repack()
        self.plans.clear()
        return True

    # ------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = make_stream(self.dev, "low")
        return self._side

    def _empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.tdt, device=self.dev)

    def _zeros(self, *shape, dtype=None):
        return torch.zeros(*shape, dtype=dtype or self.tdt, device=self.dev)

    def _bucket_bounds(self):
        """Flat-gradient slices in the order backward completes them: pnp (36 MB fp32), head (19), layer4 (52), layer3 (27),
        rest = layer2 + layer1 + stem (5.4): the big layer4 exchange starts nine blocks before the end of backward and the
        exposed tail is the smallest bucket."""
        marks = self.bucket_marks
        cuts = [0]
        for m in marks:
            cuts.append(self.grad_offsets[m])
        cuts.append(self.grad_flat.numel())
        return [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1) if cuts[i + 1] > cuts[i]]

    # ------------------------------------------------------------------------------------------ layers
    def _add_conv(self, key, kind, src_names, O, I, KH, KW, in_ch=None, out_ch=None, s2=False):
        """kind: conv | convT | stem | fc1 | fc.  in_ch/out_ch: channel counts of the activation buffers
        (>= I / O, padded).  Packed operands:
          wf [rows_f][KK][cin_f]  forward operand          (rows = out channels)
          wd [rows_d][KK][cin_d]  data-gradient operand    (rows = in channels)
          dwp fp32 [O_w][KK][I_w] packed weight gradient   (layout of `wf` for conv/fc, of `wd` for convT)"""
        in_ch = in_ch or _ru(I, 64)
        out_ch = out_ch or _ru(O, 64)
        KK = KH * KW
        L = NS(key=key, kind=kind, src=src_names, O=O, I=I, KH=KH, KW=KW, KK=KK, in_ch=in_ch, out_ch=out_ch, s2=s2)
        bn_rows = lambda c: 64 if c <= 64 else _ru(c, 128)
        if kind == "stem":
            L.cin_f, L.rows_f = 64, 64
            L.wf = self._zeros(64, 7, 64)
            L.wd = None
            L.dwp_shape = (64, 7, 64)
        elif kind == "convT":  # weight (Cin=O_w, Cout=I_w, k, k) with O_w = I(fwd in), I_w = O(fwd out)
            L.cin_f, L.rows_f = in_ch, bn_rows(O)
            L.wf = self._zeros(L.rows_f, KK, in_ch)  # rows = fwd out channels
            L.cin_d, L.rows_d = out_ch, bn_rows(I)
            L.wd = self._zeros(L.rows_d, KK, out_ch)  # rows = fwd in channels
            L.dwp_shape = (I, KK, out_ch)
        elif kind == "fc1":
            L.cin_f, L.rows_f = in_ch, bn_rows(O)
            L.wf = self._zeros(L.rows_f, KK, in_ch)
            L.cin_d, L.rows_d = out_ch, KK * in_ch  # 1x1 "conv" from O channels to KK*in_ch
            L.wd = self._zeros(L.rows_d, 1, out_ch)
            L.dwp_shape = (O, KK, in_ch)
        else:  # conv / fc
            L.cin_f, L.rows_f = in_ch, bn_rows(O)
            L.wf = self._zeros(L.rows_f, KK, in_ch)
            L.cin_d, L.rows_d = out_ch, bn_rows(in_ch)
            L.wd = self._zeros(L.rows_d, KK, out_ch)
            L.dwp_shape = (O, KK, in_ch)
        L.wfF = L.wdF = None
        # operand layouts of the two halo operands: 1 = gdrn_pack_wfrag, 2 = gdrn_pack_wfrag32 (second-generation kernel); chosen by the
        # library per launch (gdrn_conv3x3_wfrag) when the first plan that uses the operand is built (Plan._conv)
        L.wfmt = {"f": 0, "d": 0}
        if kind == "conv" and KK == 9 and not s2 and self.use_halo:  # halo-kernel operands (fragment-major)
            L.wfF, L.wdF = torch.zeros_like(L.wf), torch.zeros_like(L.wd)
        elif kind == "conv" and KK == 9 and s2 and self.h16:
            # stride-2 3x3 layers (r6, csrc/conv3x3s2.hip, conv3x3s2_dgrad.hip): both operands also in the fragment-major layout (gdrn_pack_wfrag);
            # the generic-layout copies stay (the generic kernel keeps the shapes those do not cover: odd batch sizes on 8-wide maps)
            L.wfF = torch.zeros_like(L.wf)
            L.wdF = torch.zeros_like(L.wd)   # ... and the data-gradient operand (taps not flipped) for gdrn_conv3x3s2_dgrad
            L.wfmt["f"] = L.wfmt["d"] = 1
        elif kind == "convT" and KK == 9 and self.h16:
            # the head's ConvTranspose2d(3, stride 2, pad 1, output_padding 1): its FORWARD pass is the sum gdrn_conv3x3s2_dgrad evaluates
            # (dy = its input, rows = its output channels, taps not flipped = `wf`): the fragment-major copy of the forward operand
            L.wfF = torch.zeros_like(L.wf)
            L.wdF = torch.zeros_like(L.wd)   # ... and of the data-gradient operand: the backward pass is a stride-2 conv (gdrn_conv3x3s2, bnb epilogue)
            L.wfmt["f"] = L.wfmt["d"] = 1
        self.layers[key] = L
        return L

    def _build_layers(self):
        self._add_conv("backbone.conv1", "stem", ["backbone.conv1.weight"], 64, 3, 7, 7)
        inpl = 64
        for li, (nb, pl) in enumerate(zip(RESNET34_LAYERS, RESNET34_PLANES), start=1):
            for b in range(nb):
                p = f"backbone.layer{li}.{b}"
                self._add_conv(p + ".conv1", "conv", [p + ".conv1.weight"], pl, inpl, 3, 3, s2=(b == 0 and li > 1))
                self._add_conv(p + ".conv2", "conv", [p + ".conv2.weight"], pl, pl, 3, 3)
                if (p + ".downsample.0.weight") in self.P:
                    self._add_conv(p + ".downsample.0", "conv", [p + ".downsample.0.weight"], pl, inpl, 1, 1, s2=True)
                inpl = pl
        h = "rot_head_net.features."
        self._add_conv(h + "0", "convT", [h + "0.weight"], 256, 512, 3, 3)
        for ci, _, up in HEAD_CONVS:
            self._add_conv(h + str(ci), "conv", [h + f"{ci}.weight"], 256, 256, 3, 3)
        self.head_c = 1 + 3 + self.nreg + 1
        self._add_conv(h + "23", "conv", [h + "23.weight"], self.head_c, 256, 1, 1, out_ch=128)
        q = "pnp_net.features."
        self.pnp_c = 3 + 2 + self.nreg
        self._add_conv(q + "0", "conv", [q + "0.weight"], 128, self.pnp_c, 3, 3, in_ch=128, s2=True)
        self._add_conv(q + "3", "conv", [q + "3.weight"], 128, 128, 3, 3, s2=True)
        self._add_conv(q + "6", "conv", [q + "6.weight"], 128, 128, 3, 3, s2=True)
        self._add_conv("pnp_net.fc1", "fc1", ["pnp_net.fc1.weight"], 1024, 128, 8, 8)
        self._add_conv("pnp_net.fc2", "fc", ["pnp_net.fc2.weight"], 256, 1024, 1, 1)
        self._add_conv("pnp_net.fc_rt", "fc", ["pnp_net.fc_r.weight", "pnp_net.fc_t.weight"], 9, 256, 1, 1)
        # packed fp32 weight-gradient scratch (zeroed once per backward; wgrad accumulates with atomics)
        tot = 0
        for L in self.layers.values():
            L.dwp_off = tot
            tot += _ru(int(math.prod(L.dwp_shape)), 4)
        self.dwp_flat = torch.zeros(tot, dtype=torch.float32, device=self.dev)
        for L in self.layers.values():
            L.dwp = self.dwp_flat[L.dwp_off: L.dwp_off + int(math.prod(L.dwp_shape))]
        self.bn_ws = torch.zeros(64 * 2 * 512, dtype=torch.float64, device=self.dev)  # gdrn_bn_finalize workspace (64*2*C doubles)
        self.rt_w = torch.zeros(9, 256, dtype=torch.float32, device=self.dev)
        self.rt_b = torch.zeros(9, dtype=torch.float32, device=self.dev)

    def _src_version(self, L):
        return tuple(self.P[n]._version for n in L.src) + tuple(self.P[n].data_ptr() for n in L.src)

    def _pack_args(self, L, which):
        """pack4 argument tuple (A1, A2, T, B, A1v, A2v, Bv, s1, s2, st, sb, flip) of operand `which` in ("f", "d")."""
        O, I, KK = L.O, L.I, L.KK
        if L.kind == "convT":  # weight[ci=I][co=O][k]; fwd rows = co, b = ci ; dgrad rows = ci, b = co
            return ((L.rows_f, 1, KK, L.cin_f, O, 1, I, KK, 0, 1, O * KK, 0) if which == "f"
                    else (L.rows_d, 1, KK, L.cin_d, I, 1, O, O * KK, 0, 1, KK, 0))
        if L.kind == "fc1":    # dgrad rows (p, c) -> src[o*I*KK + c*KK + p]
            return ((L.rows_f, 1, KK, L.cin_f, O, 1, I, I * KK, 0, 1, KK, 0) if which == "f"
                    else (KK, L.in_ch, 1, L.cin_d, KK, I, O, 1, KK, 0, I * KK, 0))
        flip = 1 if (KK == 9 and not L.s2) else 0
        return ((L.rows_f, 1, KK, L.cin_f, O, 1, I, I * KK, 0, 1, KK, 0) if which == "f"
                else (L.rows_d, 1, KK, L.cin_d, I, 1, O, KK, 0, 1, I * KK, flip))

    # ------------------------------------------------------------------------------------------ eval-mode BN folding
    def fold(self, bnkey, L):
        """Register conv layer L + the BatchNorm `bnkey` that follows it for eval-mode folding:
        y = act(conv_{w * scale}(x) + shift [+ residual]) with scale = gamma / sqrt(running_var + eps),
        shift = beta - running_mean * scale.  Returns NS(scale, shift) (filled by eval_refresh)."""
        f = self.bn_fold.get(bnkey)
        if f is None:
            C_ = self.P[bnkey + ".weight"].numel()
            f = NS(scale=self._empty(C_, dtype=torch.float32), shift=self._empty(C_, dtype=torch.float32), layer=L, C=C_)
            self.bn_fold[bnkey] = f
            L.wf_e = torch.zeros_like(L.wf)
            L.wfF_e = torch.zeros_like(L.wfF) if L.wfF is not None else None
            self._eval_tab = None  # rebuilt on the next refresh
        assert f.layer is L, (bnkey, L.key)
        return f

    def eval_refresh(self):
        """(Re)compute the folded scale / shift vectors and the scaled operand copies; the caller decides when."""
        lib, st = self.lib, self._stream()
        if not self.bn_fold:
            return
        if getattr(self, "_eval_tab", None) is None:
            chunk = lib.gdrn_pack_chunk()
            tasks, starts = [], [0]
            for bnkey, f in self.bn_fold.items():
                L = f.layer
                src = self.P[L.src[0]]
                halo_only = self.use_halo and self.halo_min_b <= 1 and L.wfF is not None and not L.s2 and L.kind == "conv"
                for dst, frag in ((L.wf_e, 0), (L.wfF_e, L.wfmt.get("e", 0) or 1)):
                    if dst is None or (halo_only and not frag):
                        continue
                    A1, A2, T, B, A1v, A2v, Bv, s1, s2, stt, sb, flip = self._pack_args(L, "f")
                    kch = B * (2 if self.h16 else 4) // 128
                    sh = (kch.bit_length() if (frag and kch > 0 and kch & (kch - 1) == 0) else 0)
                    t = cabi.PackTask(src=src.data_ptr(), dst=dst.data_ptr(), scale=f.scale.data_ptr(), A1=A1, A2=A2, T=T, B=B, A1v=A1v,
                                 A2v=A2v, Bv=Bv, flip=flip, s1=s1, s2=s2, st=stt, sb=sb, n=A1 * A2 * T * B, frag=frag, pad_=sh)
                    tasks.append(t)
                    starts.append(starts[-1] + ((A1 // 16) * (B // 64) if (frag and self.h16) else (t.n + chunk - 1) // chunk))
            self._eval_tab = (cabi.to_device_table(tasks, self.dev), torch.tensor(starts, dtype=torch.int32, device=self.dev), len(tasks), starts[-1])
        for bnkey, f in self.bn_fold.items():
            g, b = self.P[bnkey + ".weight"], self.P[bnkey + ".bias"]
            rm, rv = self.Bf[bnkey + ".running_mean"], self.Bf[bnkey + ".running_var"]
            check(lib.gdrn_bn_eval_params(ptr(g), ptr(b), ptr(rm), ptr(rv), 1e-5, f.C, ptr(f.scale), ptr(f.shift), st), "bn_eval_params")
        tab, stt, nt, nb = self._eval_tab
        check(lib.gdrn_pack_multi(ptr(tab), ptr(stt), nt, nb, self.dt, st), "pack_multi(eval)")

    def _build_pack_table(self):
        """Device task table for gdrn_pack_multi: every operand copy of every layer (stem excluded) in ONE launch."""
        chunk = self.lib.gdrn_pack_chunk()
        tasks, starts = [], [0]
        for key, L in self.layers.items():
            if L.kind == "stem":
                continue
            src = self.rt_w if key == "pnp_net.fc_rt" else self.P[L.src[0]]
            halo_only = self.use_halo and self.halo_min_b <= 1 and L.wfF is not None and not L.s2 and L.kind == "conv"  # both conv passes read the fragment-major copies
            for which, dst, frag in (("f", L.wf, 0), ("d", L.wd, 0), ("f", L.wfF, L.wfmt["f"] or 1), ("d", L.wdF, L.wfmt["d"] or 1)):
                if dst is None or (halo_only and not frag):
                    continue
                A1, A2, T, B, A1v, A2v, Bv, s1, s2, st, sb, flip = self._pack_args(L, which)
                kch = B * (2 if self.h16 else 4) // 128  # 128-byte chunks per pixel row
                sh = (kch.bit_length() if (frag and kch > 0 and kch & (kch - 1) == 0) else 0)  # 1 + log2(kch)
                t = cabi.PackTask(src=src.data_ptr(), dst=dst.data_ptr(), A1=A1, A2=A2, T=T, B=B, A1v=A1v, A2v=A2v, Bv=Bv, flip=flip,
                             s1=s1, s2=s2, st=st, sb=sb, n=A1 * A2 * T * B, frag=frag, pad_=sh)
                tasks.append(t)
                # workgroups of the task: bf16 fragment-major operands go brick by brick (16 rows x 64 b x 9 taps); row-major copies whose
                # unit-stride source index is not b (fc1's two operands, the 1x1 / fc data-gradient operands) as 64 x 64 tiles through LDS (r6)
                nblk = (A1 // 16) * (B // 64) if (frag and self.h16) else (cabi.transpose_blocks(self.lib, t) or (t.n + chunk - 1) // chunk)
                starts.append(starts[-1] + nblk)
        self._pack_tasks = cabi.to_device_table(tasks, self.dev)
        self._pack_starts = torch.tensor(starts, dtype=torch.int32, device=self.dev)
        self._pack_n = (len(tasks), starts[-1])
        # the same tasks per gradient bucket (repack_bucket): the fused train step rebuilds a bucket's operands right behind its optimizer update
        off_of = lambda t: self.grad_offsets[names_of[t.src]]
        names_of = {}
        for key, L in self.layers.items():
            if L.kind != "stem":
                names_of[(self.rt_w if key == "pnp_net.fc_rt" else self.P[L.src[0]]).data_ptr()] = L.src[0]
        self._pack_buckets = []
        for lo, hi in self.bucket_bounds:
            sel = [(t, n) for t, n in zip(tasks, [starts[i + 1] - starts[i] for i in range(len(tasks))]) if lo <= off_of(t) < hi]
            if not sel:
                self._pack_buckets.append(None)
                continue
            st_ = [0]
            for _, n in sel:
                st_.append(st_[-1] + n)
            self._pack_buckets.append((cabi.to_device_table([t for t, _ in sel], self.dev), torch.tensor(st_, dtype=torch.int32, device=self.dev), len(sel), st_[-1]))

    def repack(self, force=False):
        """(Re)build the kernel-layout operand copies of the weights after a parameter update: one multi-tensor
        launch (+ the stem's special layout) instead of ~170 per-tensor launches."""
        sig = tuple(p._version for p in self.P.values())
        if not force and self._versions.get("sig") == sig and not getattr(self, "_pack_dirty", False):
            return
        self._versions["sig"] = sig
        st = self._stream()
        lib = self.lib
        with torch.no_grad():  # fc_r | fc_t as one 9-row layer: one multi-tensor copy launch
            torch._foreach_copy_([self.rt_w[:6], self.rt_w[6:], self.rt_b[:6], self.rt_b[6:]],
                                 [self.P["pnp_net.fc_r.weight"].detach(), self.P["pnp_net.fc_t.weight"].detach(), self.P["pnp_net.fc_r.bias"].detach(),
                                  self.P["pnp_net.fc_t.bias"].detach()])
        Ls = self.layers["backbone.conv1"]
        check(lib.gdrn_pack_stem_w(ptr(self.P[Ls.src[0]]), ptr(Ls.wf), self.dt, st), "pack_stem_w")
        if self.stem_direct:
            check(lib.gdrn_pack_stem_w32(ptr(self.P[Ls.src[0]]), ptr(self.stem_w32), self.dt, st), "pack_stem_w32")
        if not hasattr(self, "_pack_tasks") or getattr(self, "_pack_dirty", False):
            self._build_pack_table()
            self._pack_dirty = False
        check(lib.gdrn_pack_multi(ptr(self._pack_tasks), ptr(self._pack_starts), self._pack_n[0], self._pack_n[1], self.dt, st), "pack_multi")

    def repack_bucket(self, b):
        """rebuild the operand copies of the layers whose parameters lie in gradient bucket b, on the current stream (the fused train step
        calls this behind the bucket's optimizer update on the side stream; mark_packed() afterwards)."""
        if not hasattr(self, "_pack_tasks") or getattr(self, "_pack_dirty", False):
            return False
        lib, st = self.lib, self._stream()
        nb = len(self.bucket_bounds)
        if b == 0:
            with torch.no_grad():  # fc_r | fc_t as one 9-row layer (pnp parameters: first bucket)
                torch._foreach_copy_([self.rt_w[:6], self.rt_w[6:], self.rt_b[:6], self.rt_b[6:]],
                                     [self.P["pnp_net.fc_r.weight"].detach(), self.P["pnp_net.fc_t.weight"].detach(), self.P["pnp_net.fc_r.bias"].detach(),
                                      self.P["pnp_net.fc_t.bias"].detach()])
        if b == nb - 1:
            Ls = self.layers["backbone.conv1"]
            if self.stem_direct:   # (the generic-layout stem operand has no reader then: one launch less at the very end of the step)
                check(lib.gdrn_pack_stem_w32(ptr(self.P[Ls.src[0]]), ptr(self.stem_w32), self.dt, st), "pack_stem_w32")
            else:
                check(lib.gdrn_pack_stem_w(ptr(self.P[Ls.src[0]]), ptr(Ls.wf), self.dt, st), "pack_stem_w")
        pb = self._pack_buckets[b]
        if pb is not None:
            check(lib.gdrn_pack_multi(ptr(pb[0]), ptr(pb[1]), pb[2], pb[3], self.dt, st), "pack_multi(bucket)")
        return True

    def mark_packed(self):
        """the operand copies match the parameters' current versions (every bucket went through repack_bucket)"""
        self._versions["sig"] = tuple(p._version for p in self.P.values())

    # ------------------------------------------------------------------------------------------ plans
    def plan(self, B, bn_train, with_loss):
        """bn_train: BatchNorm uses batch statistics (module.training); with_loss: train-mode pose
        decode + losses (do_loss=True).  The backward graph exists when both are set."""
        key = (B, bool(bn_train), bool(with_loss))
        p = self.plans.get(key)
        if p is None:
            from .plan import Plan   # (plan.py imports this module's constants: bound late)

            p = self.plans[key] = Plan(self, B, bool(bn_train), bool(with_loss))
            self.plan_builds += 1
            # bounded cache (least recently used out): a plan owns every activation / gradient buffer of its batch size -- ~11 GB for a
            # bs = 64 training plan.  Inference rounds its batch up to a power of two (GDRN._prepare), so a stream of changing
            # detection counts (gdrn_evaluator.py:549-578) lives in <= 7 plans; an evicted plan is freed once no autograd node holds it.
            while len(self.plans) > self.max_plans:
                self.plans.pop(next(iter(self.plans)))
        else:
            self.plans.move_to_end(key)
        return p


class LossScaleState:
    """gdrn_loss_scale_state (include/gdrn_hip.h) in device memory: what torch.cuda.amp.GradScaler keeps on the host (main_gdrn.py:53-56;
    engine.py:276-283).  Words: 0 flag | 1 applied | 2 skipped | 3 good | 4 growth | 5 scale (f32) | 6 1 / scale (f32) | 7 base_step | 8 last_overflowed."""

    def __init__(self, dev, scale, growth):
        self.t = torch.zeros(16, dtype=torch.int32, device=dev)
        self.f = self.t.view(torch.float32)
        self.write(scale=scale, growth=growth)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def write(self, scale=None, growth=None, base_step=None):
        """host -> device (asynchronous on the current stream).  base_step: the optimizer's step count; re-basing zeroes `applied`."""
        if scale is not None:
            self.f[5:7] = torch.tensor([float(scale), 1.0 / float(scale)], dtype=torch.float32).to(self.t.device, non_blocking=True)
        if growth is not None:
            self.t[4:5] = int(growth)
        if base_step is not None:
            self.t[7:8] = int(base_step)
            self.t[1:2] = 0

    def read(self):
        """device -> host (synchronises the current stream)"""
        v = self.t.cpu()
        fv = v.view(torch.float32)
        return dict(flag=int(v[0]), applied=int(v[1]), skipped=int(v[2]), good=int(v[3]), growth=int(v[4]), scale=float(fv[5]), inv_scale=float(fv[6]),
                    base_step=int(v[7]), last_overflowed=int(v[8]))


_hip_rt = None


def make_stream(dev, prio="normal"):
    """a HIP stream of the given priority class as a torch stream object.  "low": below torch's default streams (torch itself only hands out
    default- and higher-priority streams): created with hipStreamCreateWithPriority and wrapped; its kernels are dispatched behind those
    of default-priority streams and it never shares a hardware queue with them."""
    global _hip_rt
    # Streams made here live as long as the process: one per engine / reducer, a handful per process.  (Destroying the raw stream when its
    # wrapper object is collected was tried in r4 and is unsafe: RCCL keeps using a reducer's stream from its own threads, and objects
    # collected during interpreter teardown would call into a HIP runtime that is already gone -- both ended in SIGSEGV in the GPU suite.)
    # Callbacks the engine invokes for a finished gradient bucket (`model._on_bucket`) run with the SIDE stream current, not the compute
    # stream: work they enqueue is ordered behind the bucket's weight gradients, and whoever consumes its results on another stream has to
    # wait for it (GradReducer.on_bucket records an event for that).
    if prio == "high":
        return torch.cuda.Stream(device=dev, priority=-1)
    if prio != "low":
        return torch.cuda.Stream(device=dev)
    try:
        if _hip_rt is None:
            # the HIP runtime this process already runs on (torch ships its own copy): opened by the path it was mapped from, so that the
            # stream belongs to the same runtime instance as torch's streams and this library's launches
            path = "libamdhip64.so"
            with open("/proc/self/maps") as f:
                for line in f:
                    if "libamdhip64" in line:
                        path = line.split()[-1]
                        break
            _hip_rt = C.CDLL(path)
        least, greatest = C.c_int(0), C.c_int(0)
        _hip_rt.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest))
        h = C.c_void_p()
        with torch.cuda.device(dev):
            err = _hip_rt.hipStreamCreateWithPriority(C.byref(h), C.c_uint(1), C.c_int(max(least.value, 1)))   # hipStreamNonBlocking
        if err != 0 or not h.value:
            raise OSError(f"hipStreamCreateWithPriority returned {err}")
    except (OSError, AttributeError) as ex:   # an optimisation, not a requirement: a default-priority stream computes the same
        import logging

        logging.getLogger(__name__).warning("low-priority HIP stream unavailable (%s): using a default-priority stream", ex)
        return torch.cuda.Stream(device=dev)
    return torch.cuda.ExternalStream(h.value, device=dev)
